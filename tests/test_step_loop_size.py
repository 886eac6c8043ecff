"""The compute waves' step loops of the headline recurrent kernels stay as short as they were shipped (tools/step_loop_size.py: the
built library's disassembly, no GPU): instructions, v_mov_b32, SALU instructions and branches per time step against the recorded
budget.  With one compute wave per SIMD every instruction of that loop is on the dependent chain of a step unless it falls into a
wait; index arithmetic or register copies coming back into it are a regression no parity test sees."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "vmlmf_amd", "lib", "libvmlmf_hip.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
sys.path.insert(0, os.path.join(ROOT, "tools"))
import step_loop_size as S  # noqa: E402


@pytest.fixture(scope="module")
def measured():
    if not os.path.exists(LIB):
        import vmlmf_amd._lib as L
        L.build()
    return S.measure(LIB)


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump of the ROCm toolchain not present")
@pytest.mark.parametrize("prefix", list(S.KERNELS), ids=lambda p: p[5:-1].replace(" ", ""))
def test_step_loop_within_budget(measured, prefix):
    assert prefix in measured, f"no step loop found in {prefix}...): renamed? update tools/step_loop_size.py"
    steps, got = measured[prefix]
    names = ("instructions", "v_mov_b32", "SALU", "branches")
    over = {names[k]: (got[k], S.SHIPPED[prefix][k] + S.SLACK) for k in range(4) if got[k] > S.SHIPPED[prefix][k] + S.SLACK}
    assert not over, f"{prefix}...) per time step (loop of {steps} steps), count and budget: {over}"
    assert S.SHIPPED[prefix][0] <= S.PARENT[prefix][0], "the recorded budget is no shorter than the loop it replaced"


def test_the_walk_on_a_hand_written_listing():
    """step_loop() on a listing with a one-step remainder loop and a two-step unrolled loop: the unrolled one is the step loop, and the
    counts come out per step."""
    def ins(addr, mn, ops="", target=None):
        return (addr, mn, ops, target)
    ror = "v1, v2, v3 row_ror:15 row_mask:0xf bank_mask:0xf"
    listing = [ins(0, "s_mov_b32", "s0, 0"),
               ins(4, "v_fmac_f32_dpp", ror), ins(8, "v_mov_b32_e32", "v1, v2"), ins(12, "s_add_i32", "s0, s0, 1"), ins(16, "s_cbranch_scc1", "65532", 4),
               ins(20, "v_fmac_f32_dpp", ror), ins(24, "s_barrier"), ins(28, "v_fmac_f32_dpp", ror), ins(32, "s_waitcnt", "lgkmcnt(0)"),
               ins(36, "s_add_i32", "s0, s0, 2"), ins(40, "v_mov_b32_e32", "v1, v2"), ins(44, "s_cbranch_scc1", "65529", 20),
               ins(48, "s_endpgm")]
    loop = S.step_loop(listing)
    assert [a for a, _, _, _ in loop] == list(range(20, 48, 4))
    steps, (total, movs, salu, branches) = S.counts(loop, 1)
    assert (steps, total, movs, salu, branches) == (2, 4, 1, 1, 1)
