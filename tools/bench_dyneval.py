"""What dynamic evaluation costs (vmlmf_amd.DynamicEval; docs/design/lm_dyneval.md) on the plain PTB network: V 10 000, H 650, 2 VMLMF
layers of rank 32 - 13.4 M parameters in 19 tensors, embed.w and fc.w 6.5 M each.
  what "step"     the update alone on the network's real parameter list, random gradients and statistics: DynamicEval.step() on the fused
                  launches (sqsum_kernel, norm_kernel, dyneval_kernel) against the same rule in stock ops (dyneval_step_stock), both
                  captured into graphs of --launches steps that are replayed in turn, --reps rounds: device-event time per step, the best
                  of the rounds and the spread (max / min).  *_tbs: the 24 bytes per element the rule has to move (the norm reads g;
                  the update reads theta, theta0, r, g and writes theta) over that time, to be read beside the 4.6 - 5 TB/s of the
                  project's in-place passes and the 6.29 TB/s of a streaming read.
  what "segment"  the whole step behind one segment - gradients freed, features, head loss with its rows, backward, update - as
                  DynamicEval.score of one segment of (T, B) positions, fused against the same loop with the update in stock ops, and
                  for orientation Model.score on the same tokens (no adaptation, no autograd).  Wall clock between synchronisations,
                  the forms in turn, twice; best of --reps timings of 5 calls and the spread.
No pass / fail gate.  One JSON object per line, appended to --out (default profiles/lm_dyneval_bench.jsonl).
`python tools/bench_dyneval.py [--out FILE] [--shapes 5x1,5x10,35x1] [--reps 7] [--launches 10]`"""
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
BYTES_PER_ELEMENT = 24


def synthetic_statistics(de, seed=0):
    """Statistics of the right shapes without a training set: r log-uniform over two decades, as gradients' RMS values spread."""
    g = torch.Generator(device=de.theta0.device).manual_seed(seed)
    sd = de.state_dict()
    rms = [10.0 ** (torch.rand(m.shape, generator=g, device=m.device) * 2.0 - 4.0) for m in sd["ms"]]
    sd.update(minibatches=1, ms=[r * r for r in rms], rms=rms, mean_rms=float(torch.stack([r.mean() for r in rms]).mean()))
    return sd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_dyneval_bench.jsonl"))
    ap.add_argument("--shapes", default="5x1,5x10,35x1")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    a = ap.parse_args()
    from vmlmf_amd import DynamicEval, Model
    dev = torch.device("cuda", torch.cuda.current_device())
    out = open(a.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    torch.manual_seed(0)
    hyper = dict(lr=1e-4, decay=0.02, eps=1e-5, max_norm=0.25)
    model = Model(V, H, 2, 0.5, 0.05, w_rank=32, u_ranks=[32], lstm_type="vmlmf").to(dev)
    twin = Model(V, H, 2, 0.5, 0.05, w_rank=32, u_ranks=[32], lstm_type="vmlmf").to(dev)
    twin.load_state_dict(model.state_dict())
    params = list(model.parameters())
    n = sum(p.numel() for p in params)
    fused, stock = DynamicEval(model, **hyper), DynamicEval(twin, **hyper)
    stats = synthetic_statistics(fused)
    fused.load_state_dict(stats)
    stock.load_state_dict(stats)
    stock.stock = True
    for m in (model, twin):
        for p in m.parameters():
            p.grad = 1e-3 * torch.randn_like(p)
    got = alternated_us({"fused": fused.step, "stock": stock.step}, a.launches, a.reps)
    rec = {"what": "step", "tensors": len(params), "elements": n, "bytes": BYTES_PER_ELEMENT * n, "launches": a.launches, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), **hyper}
    for name, (best, spread) in got.items():
        rec[f"{name}_us"], rec[f"{name}_spread"] = round(best, 2), round(spread, 3)
        rec[f"{name}_tbs"] = round(BYTES_PER_ELEMENT * n / (best * 1e-6) / 1e12, 3)
    rec["stock_over_fused"] = round(got["stock"][0] / got["fused"][0], 2)
    emit(rec)
    fused.restore()
    stock.restore()

    for shape in a.shapes.split(","):
        T, B = (int(v) for v in shape.split("x"))
        tokens = torch.randint(0, V, (T + 1, B), device=dev)
        evals = {}
        for name, m in (("fused", model), ("stock", twin)):
            de = DynamicEval(m, segment=T, **hyper)
            de.load_state_dict(stats)
            de.stock = name == "stock"
            evals[name] = de
        forms = {"fused": lambda: evals["fused"].score(tokens), "stock": lambda: evals["stock"].score(tokens),
                 "model_score": lambda: model.score(tokens)}
        rec = {"what": "segment", "T": T, "B": B, "reps": a.reps, "device": torch.cuda.get_device_name(0), **hyper}
        for _ in range(2):                                   # the forms in turn, twice: the second round's numbers beside the first's
            for name, fn in forms.items():
                best, spread = wall_ms(fn, a.reps, calls=5, warm=2)
                rec.setdefault(f"{name}_ms", []).append(round(best, 4))
                rec.setdefault(f"{name}_spread", []).append(round(spread, 3))
        rec["stock_over_fused"] = round(min(rec["stock_ms"]) / min(rec["fused_ms"]), 2)
        emit(rec)
        for de in evals.values():
            de.restore()
    out.close()


if __name__ == "__main__":
    main()
