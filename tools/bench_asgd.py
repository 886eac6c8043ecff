"""What the NT-ASGD step costs (vmlmf_amd.optim.ASGD; docs/design/lm_asgd.md) on the plain PTB network: V 10 000, H 650, 2 VMLMF layers of
rank 32 - 13.4 M parameters in 19 tensors, embed.w and fc.w 6.5 M each.
  what "step"  the step alone on the network's real parameter list with random gradients, every form on parameters of its own, each
               captured into a graph of --launches steps; the graphs are replayed in turn, --reps rounds: device-event time per step,
               the best of the rounds and the spread (max / min).
                 sgd_*        optim.clip_sgd_step: the LM loop's step, the thing to compare averaging-off with (same run, alternated)
                 asgd_off_*   ASGD.step before start_averaging(), weight decay on
                 asgd_on_*    ASGD.step with averaging on (n >= 2: ax is read and written)
                 stock_on_*   the same rule in stock ops (asgd_step_stock), averaging on
                 *_unclipped  max_norm far above the norm: c == 1, the gradients are not stored
                 *_clipped    max_norm = 1e-9: c < 1 at every replay whatever the gradients have become (c <= 1e-9 / 1e-6)
               *_tbs: the bytes the whole step has to move over that time - the norm reads g (4 per element), the update reads p and
               g and writes p (12), reads and writes ax when averaging (+ 8) and stores g when the clip binds (+ 4) - to be read
               beside the 6.29 TB/s of a streaming read.
  what "wall"  ASGD.step against clip_grad_norm_ + torch.optim.ASGD(lambd=0) on the same tensors, averaging on, clip binding: wall
               clock between synchronisations, the forms in turn, twice; best of --reps timings of 5 calls and the spread.
No pass / fail gate.  One JSON object per line, appended to --out (default profiles/lm_asgd_bench.jsonl).
`python tools/bench_asgd.py [--out FILE] [--reps 7] [--launches 10]`"""
import argparse
import json
import os
import sys

import torch

from _timing import wall_ms
from bench_distill import alternated_us

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

V, H = 10000, 650
LR, WD = 1e-3, 1.2e-6
LOOSE, TIGHT = 1e9, 1e-9


def bytes_per_element(averaging, clipped):
    return 4 + 12 + (8 if averaging else 0) + (4 if clipped else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_asgd_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    a = ap.parse_args()
    from vmlmf_amd import Model, optim
    dev = torch.device("cuda", torch.cuda.current_device())
    out = open(a.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    torch.manual_seed(0)
    model = Model(V, H, 2, 0.5, 0.05, w_rank=32, u_ranks=[32], lstm_type="vmlmf").to(dev)
    shapes = [p.shape for p in model.parameters()]
    n = sum(p.numel() for p in model.parameters())
    grads = [1e-3 * torch.randn(s, device=dev) for s in shapes]

    def parameters():
        """The network's parameter list again, on memory of its own, every tensor with its own copy of the gradients."""
        params = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
        for p, g in zip(params, grads):
            p.grad = g.clone()
        return params

    def asgd(max_norm, averaging, stock=False):
        opt = optim.ASGD(parameters(), lr=LR, weight_decay=WD, max_norm=max_norm)
        opt.stock = stock
        if averaging:
            opt.start_averaging()
            for _ in range(2):                           # the two copying steps: from here on n >= 2
                opt.step()
        return opt.step

    def sgd(max_norm):
        params = parameters()
        return lambda: optim.clip_sgd_step(params, LR, max_norm)

    forms = {}
    for tag, max_norm in (("unclipped", LOOSE), ("clipped", TIGHT)):
        forms[f"sgd_{tag}"] = (sgd(max_norm), False, tag == "clipped")
        forms[f"asgd_off_{tag}"] = (asgd(max_norm, False), False, tag == "clipped")
        forms[f"asgd_on_{tag}"] = (asgd(max_norm, True), True, tag == "clipped")
        forms[f"stock_on_{tag}"] = (asgd(max_norm, True, stock=True), True, tag == "clipped")
    got = alternated_us({name: f[0] for name, f in forms.items()}, a.launches, a.reps)
    rec = {"what": "step", "tensors": len(shapes), "elements": n, "launches": a.launches, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "lr": LR, "weight_decay": WD}
    for name, (best, spread) in got.items():
        nbytes = bytes_per_element(forms[name][1], forms[name][2]) * n
        rec[f"{name}_us"], rec[f"{name}_spread"] = round(best, 2), round(spread, 3)
        rec[f"{name}_bytes"], rec[f"{name}_tbs"] = nbytes, round(nbytes / (best * 1e-6) / 1e12, 3)
    for tag in ("unclipped", "clipped"):
        rec[f"asgd_off_over_sgd_{tag}"] = round(got[f"asgd_off_{tag}"][0] / got[f"sgd_{tag}"][0], 3)
        rec[f"stock_over_fused_on_{tag}"] = round(got[f"stock_on_{tag}"][0] / got[f"asgd_on_{tag}"][0], 2)
    emit(rec)

    # the stock formulation: clip_grad_norm_ + torch.optim.ASGD, host and device together
    fused_step = asgd(TIGHT, True)
    tparams = parameters()
    topt = torch.optim.ASGD(tparams, lr=LR, lambd=0.0, t0=0, weight_decay=WD)

    def torch_pair():
        torch.nn.utils.clip_grad_norm_(tparams, TIGHT)
        topt.step()
    rec = {"what": "wall", "elements": n, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    for _ in range(2):                                   # the forms in turn, twice: the second round's numbers beside the first's
        for name, fn in (("fused", fused_step), ("torch_pair", torch_pair)):
            best, spread = wall_ms(fn, a.reps, calls=5, warm=2)
            rec.setdefault(f"{name}_ms", []).append(round(best, 4))
            rec.setdefault(f"{name}_spread", []).append(round(spread, 3))
    rec["torch_pair_over_fused"] = round(min(rec["torch_pair_ms"]) / min(rec["fused_ms"]), 2)
    emit(rec)
    out.close()


if __name__ == "__main__":
    main()
