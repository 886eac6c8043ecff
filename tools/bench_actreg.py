"""What activation regularisation costs (Model.loss's ar / tar; vmlmf_amd.activation_regularizer; docs/design/lm_actreg.md).
  what "pair"  the forward and backward of the regulariser alone on a (T, B, H) tensor of the top layer's output, the site's dropout
               at p included: `fused` is vmlmf_actreg_forward + vmlmf_actreg_backward, `stock` the formulation a user of stock ops
               writes - nn.functional.dropout, alpha * dropped.pow(2).mean() + beta * (raw[1:] - raw[:-1]).pow(2).mean(), autograd's
               backward.  Both get the head's gradient of the dropped copy and the unit gradient of the penalty.  Each form is
               captured into a graph of --launches pairs; the graphs are replayed in turn, --reps rounds: device-event time per
               pair, the best of the rounds and the spread (max / min).  fused_bytes: what the pair has to move - forward raw (and
               one row in four again) in, yd out at p > 0; backward g and raw (two rows in four again) in, d raw out.
  what "step"  loss + backward of the plain PTB network (V 10 000, H 650, 2 VMLMF layers of rank 32, p 0.5) at 32 rows of 35 steps,
               `reg` with ar=2, tar=1 against `plain` with both off - the step as it is without this feature, launch for launch -,
               alternated the same way.
No pass / fail gate.  One JSON object per line, appended to --out (default profiles/lm_actreg_bench.jsonl).
`python tools/bench_actreg.py [--out FILE] [--reps 9] [--launches 10]`"""
import argparse
import json
import os
import sys

import torch

from bench_distill import alternated_us

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPES = [(35, 32, 650), (35, 128, 650), (70, 256, 650)]
AR, TAR = 2.0, 1.0


def fused_bytes(T, B, H, p):
    n = 4 * T * B * H
    return int(n * (1 + 1 / 4 + (1 if p > 0 else 0)) + n * (1 + 1 + 2 / 4 + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_actreg_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--launches", type=int, default=10)
    a = ap.parse_args()
    import vmlmf_amd
    from vmlmf_amd import Model, unit_gradient
    from vmlmf_amd import functional as F
    dev = torch.device("cuda", torch.cuda.current_device())
    one = unit_gradient(dev)
    out = open(a.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    torch.manual_seed(0)
    for (T, B, H) in SHAPES:
        for p in (0.5, 0.0):
            x = (0.3 * torch.randn(T, B, H, device=dev)).requires_grad_(True)
            g = 1e-3 * torch.randn(T, B, H, device=dev)
            state = F.dropout_state(dev, seed=11)

            def fused():
                snap = F.dropout_advance(state) if p > 0 else None
                yd, penalty, _ = vmlmf_amd.activation_regularizer(x, ar=AR, tar=TAR, p=p, snap=snap, site=2)
                return torch.autograd.grad([yd, penalty], x, [g, one])

            def stock():
                dropped = torch.nn.functional.dropout(x, p, True) if p > 0 else x
                penalty = B * (AR * dropped.pow(2).mean() + TAR * (x[1:] - x[:-1]).pow(2).mean())
                return torch.autograd.grad([dropped, penalty], x, [g, one])

            got = alternated_us({"fused": fused, "stock": stock}, a.launches, a.reps)
            rec = {"what": "pair", "T": T, "B": B, "H": H, "p": p, "ar": AR, "tar": TAR, "launches": a.launches, "reps": a.reps,
                   "device": torch.cuda.get_device_name(0), "fused_bytes": fused_bytes(T, B, H, p)}
            for name, (best, spread) in got.items():
                rec[f"{name}_us"], rec[f"{name}_spread"] = round(best, 2), round(spread, 3)
            rec["fused_tbs"] = round(rec["fused_bytes"] / (got["fused"][0] * 1e-6) / 1e12, 3)
            rec["stock_over_fused"] = round(got["stock"][0] / got["fused"][0], 2)
            emit(rec)

    V, H, B, T = 10000, 650, 32, 35
    model = Model(V, H, 2, 0.5, 0.05, w_rank=32, u_ranks=[32], lstm_type="vmlmf").to(dev).train()
    model.dropout_state(seed=5)
    tok, tgt = torch.randint(0, V, (T, B), device=dev), torch.randint(0, V, (T, B), device=dev)

    def step(**kw):
        def body():
            model.zero_grad(set_to_none=True)
            loss, _ = model.loss(tok, tgt, model.state_init(B), **kw)
            loss.backward(one)
        return body
    got = alternated_us({"plain": step(), "reg": step(ar=AR, tar=TAR)}, a.launches, a.reps)
    rec = {"what": "step", "T": T, "B": B, "H": H, "V": V, "p": 0.5, "ar": AR, "tar": TAR, "launches": a.launches, "reps": a.reps,
           "device": torch.cuda.get_device_name(0)}
    for name, (best, spread) in got.items():
        rec[f"{name}_us"], rec[f"{name}_spread"] = round(best, 2), round(spread, 3)
    rec["reg_over_plain"] = round(got["reg"][0] / got["plain"][0], 4)
    emit(rec)
    out.close()


if __name__ == "__main__":
    main()
