"""What locked (variational) dropout costs (Model.locked_dropout and the per-site rates; docs/design/lm_locked.md).
  what "step"    loss + backward + clip_sgd_step of the plain and of the group PTB network (V 10 000, H 650, 2 VMLMF layers of rank 32 /
                 [32, 32]) at 32 rows of 35 steps: `elem` nn.Dropout's per-element rule at 0.5 (the model as it is without the new
                 arguments), `locked` one mask per site at the same rate, `recipe` locked at AWD-LSTM's 0.4 / 0.25 / 0.4.
  what "pair"    the AR / TAR launch pair (vmlmf_actreg_forward + _backward) at (35, 32, 650) and (70, 256, 650), p 0.5: the
                 per-element site against the locked one, where a thread draws once for its four time steps.
  what "apply"   the stand-alone launch (vmlmf_dropout_apply, drop_rows_kernel) over (R, 650) rows, R = 1120 and 8960, p 0.5: per
                 element, locked (vmlmf_dropout_apply_locked at B = 32 / 256: one draw per four-step walk) and, with --parent, the
                 parent's library loaded beside this one: the per-element launch as it was before drop_rows_kernel was rewritten.
  what "bench"   bench.py --config E --gpus 1 and --config A of this tree against another checkout (--parent DIR, built; the parent
                 commit), alternated, two runs each: the figure bench.py prints.  Skipped without --parent.
Forms are captured into graphs of --launches calls and the graphs replayed in turn for --reps rounds: device-event time per call, the
best round and the spread (max / min) - bench_tied.py's method.  No pass / fail gate.  One JSON object per line, appended to --out
(default profiles/lm_locked_bench.jsonl).
`python tools/bench_locked.py [--out FILE] [--reps 9] [--launches 10] [--parent DIR] [--steps 200] [--warmup 20]`"""
import argparse
import json
import os
import subprocess
import sys

import torch

from bench_distill import alternated_us

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

PAIRS = [(35, 32, 650), (70, 256, 650)]
AR, TAR, P = 2.0, 1.0, 0.5
RECIPE = dict(input_dropout=0.4, hidden_dropout=0.25, output_dropout=0.4)


def bench_line(tree, config, steps, warmup):
    """The JSON result line of `bench.py --config <config> --gpus 1` run in `tree`, in a process of its own."""
    cmd = [sys.executable, "bench.py", "--config", config, "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)]
    text = subprocess.run(cmd, cwd=tree, check=True, capture_output=True, text=True, timeout=600).stdout
    return json.loads([l for l in text.splitlines() if l.startswith("{") and '"metric"' in l][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_locked_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", default="step,pair,apply,bench")
    a = ap.parse_args()
    import vmlmf_amd
    from vmlmf_amd import Model, optim, unit_gradient
    from vmlmf_amd import functional as F
    dev = torch.device("cuda", torch.cuda.current_device())
    one = unit_gradient(dev)
    out = open(a.out, "a")

    def emit(rec, got=None, base=None):
        for name, (best, spread) in (got or {}).items():
            rec[f"{name}_us"], rec[f"{name}_spread"] = round(best, 2), round(spread, 3)
        for name in (got or {}):
            if name != base:
                rec[f"{name}_over_{base}"] = round(got[name][0] / got[base][0], 4)
        rec.update(device=torch.cuda.get_device_name(0))
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    torch.manual_seed(0)
    V, H, B, T = 10000, 650, 32, 35
    tok, tgt = torch.randint(0, V, (T, B), device=dev), torch.randint(0, V, (T, B), device=dev)

    def step(group, **kw):
        if group:
            model = Model.with_group_layers(V, H, 2, 0.5, 0.05, 32, [32, 32], **kw).to(dev).train()
        else:
            model = Model(V, H, 2, 0.5, 0.05, w_rank=32, u_ranks=[32], lstm_type="vmlmf", **kw).to(dev).train()
        model.dropout_state(seed=5)
        params = list(model.parameters())

        def body():
            model.zero_grad(set_to_none=True)
            loss, _ = model.loss(tok, tgt, model.state_init(B))
            loss.backward(one)
            optim.clip_sgd_step(params, 1e-3, 0.25)
        return body
    if "step" in a.only:
        for group in (False, True):
            got = alternated_us({"elem": step(group), "locked": step(group, locked_dropout=True),
                                 "recipe": step(group, locked_dropout=True, **RECIPE)}, a.launches, a.reps)
            emit({"what": "step", "net": "group" if group else "plain", "T": T, "B": B, "H": H, "V": V, "launches": a.launches, "reps": a.reps},
                 got, "elem")

    if "pair" in a.only:
        for (T_, B_, H_) in PAIRS:
            x = (0.3 * torch.randn(T_, B_, H_, device=dev)).requires_grad_(True)
            g = 1e-3 * torch.randn(T_, B_, H_, device=dev)
            state = F.dropout_state(dev, seed=11)

            def pair(site):
                def body():
                    yd, penalty, _ = vmlmf_amd.activation_regularizer(x, ar=AR, tar=TAR, p=P, snap=F.dropout_advance(state), site=site)
                    return torch.autograd.grad([yd, penalty], x, [g, one])
                return body
            got = alternated_us({"elem": pair(2), "locked": pair(F.locked_site(2))}, a.launches, a.reps)
            emit({"what": "pair", "T": T_, "B": B_, "H": H_, "p": P, "ar": AR, "tar": TAR, "launches": a.launches, "reps": a.reps}, got, "elem")

    if "apply" in a.only:
        import ctypes
        from vmlmf_amd import _lib
        libs = {"elem": _lib.lib()}
        if a.parent:
            old = ctypes.CDLL(os.path.join(a.parent, "vmlmf_amd", "lib", "libvmlmf_hip.so"))
            old.vmlmf_dropout_apply.restype, old.vmlmf_dropout_apply.argtypes = _lib.SYMBOLS["vmlmf_dropout_apply"]
            libs["parent_elem"] = old
        for R, B_ in ((1120, 32), (8960, 256)):
            xr, yr = torch.randn(R, 650, device=dev), torch.empty(R, 650, device=dev)
            snap = torch.tensor([11, 3], dtype=torch.int64, device=dev)

            def flat(lib):
                def body():
                    _lib.check(lib.vmlmf_dropout_apply(R, 650, _lib.ptr(xr), _lib.ptr(yr), P, snap.data_ptr(), 1, _lib.raw_stream(dev)))
                return body

            def locked():
                _lib.check(libs["elem"].vmlmf_dropout_apply_locked(R, B_, 650, _lib.ptr(xr), _lib.ptr(yr), P, snap.data_ptr(), 1, _lib.raw_stream(dev)))
            forms = {name: flat(lib) for name, lib in libs.items()}
            forms["locked"] = locked
            got = alternated_us(forms, a.launches, a.reps)
            emit({"what": "apply", "R": R, "B": B_, "H": 650, "p": P, "launches": a.launches, "reps": a.reps}, got, "elem")

    if "bench" in a.only and a.parent:
        for config in ("E", "A"):
            runs = {"this": [], "parent": []}
            for _ in range(2):
                for name, tree in (("this", ROOT), ("parent", a.parent)):
                    runs[name].append(bench_line(tree, config, a.steps, a.warmup))
            emit({"what": "bench", "config": config, "unit": runs["this"][0]["unit"], "steps": a.steps, "warmup": a.warmup,
                  "this": [r["value"] for r in runs["this"]], "parent": [r["value"] for r in runs["parent"]]})
    out.close()


if __name__ == "__main__":
    main()
