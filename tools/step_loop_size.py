#!/usr/bin/env python3
"""Size of the compute waves' step loops in the headline recurrent kernels, read from the built library's disassembly (the walk
of tools/kernel_budget.py / tools/check_asm_hazards.py over the gfx950 code objects): no GPU needed.

Why: with one compute wave per SIMD the dependent chain of a time step is the wave's own instruction stream - every instruction
in the loop costs 4-5 cycles of it, arithmetic or not (docs/design/recurrent_valu.md, "Step loops: the instructions that compute
nothing").  The loop is found as the innermost backward branch whose body holds a `row_ror:15` instruction (the last rotation of
the rank-space reduce, which only the compute waves execute).  A loop unrolled over several time steps holds that instruction
several times; every count is reported PER TIME STEP (rounded up).

    python tools/step_loop_size.py [libvmlmf_hip.so]        prints the counts; exit 1 above a budget
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
DEMANGLE = shutil.which("c++filt") or "c++filt"

# kernel (demangled prefix) -> row_ror:15 instructions one time step executes (backward: the reduce's add chain and the
# expansion's fmac chain; forward: the reduce's fmac chain)
KERNELS = {
    "void rec_fwd_kernel<16, 1, false, 256, 3, true>(": 1,
    "void rec3_bwd_kernel<16, 1>(": 2,
    "void rec3_bwd_kernel<16, 0>(": 2,
}
# (instructions, v_mov_b32, SALU, branches) per time step, as this walk counts them: the build before the step loops were trimmed
# (ring depth six, rolled loops, a DPP butterfly over the forward's wave partials; a count on the compiler's -S output that includes
# the loop's entry block gives 165 for the backward) ...
PARENT = {
    "void rec_fwd_kernel<16, 1, false, 256, 3, true>(": (150, 7, 15, 2),
    "void rec3_bwd_kernel<16, 1>(": (161, 16, 16, 2),
    "void rec3_bwd_kernel<16, 0>(": (161, 16, 16, 2),
}
# ... and the budget: the counts of the build that trimmed them (docs/design/recurrent_valu.md, "Step loops").  Every count has
# four instructions of slack.  rec3_bwd_kernel<16, 0> keeps a rolled loop (its occupancy rests on 136 VGPRs): ring slot by `& 7`
# and the shorter sums only.
SHIPPED = {
    "void rec_fwd_kernel<16, 1, false, 256, 3, true>(": (125, 6, 3, 1),
    "void rec3_bwd_kernel<16, 1>(": (128, 10, 3, 1),
    "void rec3_bwd_kernel<16, 0>(": (158, 13, 15, 2),
}
SLACK = 4

INS = re.compile(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):")
TARGET = re.compile(r"<[^>]*\+0x([0-9a-fA-F]+)>\s*$")
SALU_NOT_COUNTED = ("s_waitcnt", "s_barrier", "s_nop", "s_branch", "s_cbranch", "s_setprio", "s_endpgm", "s_sleep", "s_code_end")


def functions(lib):
    """{mangled name: [(address, mnemonic, operands, branch target address or None)]} of every gfx950 code object"""
    tmp = tempfile.mkdtemp(prefix="vmlmf_sl_")
    out = {}
    try:
        copy = os.path.join(tmp, "lib.so")
        shutil.copy(lib, copy)
        subprocess.run([OBJDUMP, "--offloading", copy], check=True, capture_output=True)
        for f in sorted(os.listdir(tmp)):
            if "amdgcn" not in f:
                continue
            text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", os.path.join(tmp, f)], check=True,
                                  capture_output=True, text=True).stdout
            if "row_ror:15" not in text:
                continue
            name, cur = None, None
            for raw in text.splitlines():
                head = raw.split("//")[0].rstrip()
                m = re.match(r"^<?([A-Za-z_$][\w$.]*)>?:$", head.strip())
                if m and not head.startswith((" ", "\t")):
                    name, cur = m.group(1), []
                    out[name] = cur
                    continue
                m = INS.match(raw)
                if m and cur is not None:
                    t = TARGET.search(raw) if m.group(1).startswith(("s_cbranch", "s_branch")) else None
                    cur.append((int(m.group(3), 16), m.group(1), m.group(2), t and int(t.group(1), 16)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return out


def step_loop(ins):
    """the innermost loop (backward branch .. its target) that holds a row_ror:15 instruction: the list of its instructions"""
    if not ins:
        return None
    base = ins[0][0]
    index = {a: i for i, (a, _, _, _) in enumerate(ins)}
    loops = []
    for j, (a, mn, _, t) in enumerate(ins):
        if t is None or base + t > a or base + t not in index:
            continue
        i = index[base + t]
        n = sum(1 for _, _, ops, _ in ins[i:j + 1] if "row_ror:15" in ops)
        if n:
            loops.append((i, j, n))
    # innermost: holds no other such loop.  A kernel whose loop is unrolled over several steps keeps a second, one-step loop for
    # the remainder of T: the step loop is the one that holds the most steps (it runs T / period times, the other < period).
    inner = [l for l in loops if not any(o is not l and l[0] <= o[0] and o[1] <= l[1] for o in loops)]
    if not inner:
        return None
    i, j, _ = max(inner, key=lambda l: (l[2], l[0] - l[1]))
    return ins[i:j + 1]


def counts(loop, ror_per_step):
    steps = max(1, sum(1 for _, _, ops, _ in loop if "row_ror:15" in ops) // ror_per_step)
    total = len(loop)
    movs = sum(1 for _, mn, _, _ in loop if mn.startswith("v_mov_b32"))
    salu = sum(1 for _, mn, _, _ in loop if mn.startswith("s_") and not mn.startswith(SALU_NOT_COUNTED))
    branches = sum(1 for _, mn, _, _ in loop if mn.startswith(("s_cbranch", "s_branch")))
    per = lambda v: -(-v // steps)
    return steps, (per(total), per(movs), per(salu), per(branches))


def measure(lib):
    """{demangled prefix: (time steps per trip of the loop, (instructions, v_mov_b32, SALU, branches) per time step)}"""
    fn = functions(lib)
    names = list(fn)
    dem = subprocess.run([DEMANGLE], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    out = {}
    for n, d in zip(names, dem):
        for prefix, ror in KERNELS.items():
            if d.startswith(prefix):
                loop = step_loop(fn[n])
                if loop is not None:
                    out[prefix] = counts(loop, ror)
    return out


def main(lib):
    got = measure(lib)
    bad = []
    what = ("instructions", "v_mov_b32", "SALU", "branches")
    for prefix in KERNELS:
        if prefix not in got:
            bad.append(f"{prefix}...: no step loop found (renamed? update tools/step_loop_size.py)")
            continue
        steps, c = got[prefix]
        line = f"{prefix[5:-1]}: loop of {steps} step(s); per step " + ", ".join(
            f"{c[k]} {what[k]} (parent {PARENT[prefix][k]}, budget {SHIPPED[prefix][k] + SLACK})" for k in range(4))
        print(line)
        if any(c[k] > SHIPPED[prefix][k] + SLACK for k in range(4)):
            bad.append(line)
    print(f"{len(KERNELS)} step loops, {len(bad)} above budget")
    for b in bad:
        print("  ABOVE:", b)
    return 1 if bad else 0


if __name__ == "__main__":
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "vmlmf_amd", "lib", "libvmlmf_hip.so")))
