"""What the general training objective costs at the LM head (functional.lm_head_objective_loss: vmlmf_objective_forward_grad, two
launches, csrc/vmlmf_head_loss.hip), at the PTB width V 10 000: R = 1120 rows (35 x 32, the LM step at 32 rows) and R = 8960
(35 x 256, BASELINE configs[4] on one GPU).  One row in eight is masked (target -1).
  fused_mask_us / fused_smooth_z_us / fused_ul35_us / fused_all_us
                                   the launch pair on a fixed (R, V) score matrix with a bias: the mask alone; label smoothing 0.1
                                   and z-loss 1e-4; unlikelihood 0.5 against 35 negatives per row; all four
  nll_us                           vmlmf_nll_forward_grad on the same matrix (no mask): the launch pair Model.loss makes by default
  stock_mask_us / stock_all_us     functional.objective_loss_stock - logsumexp, gather, mean, softmax, scatter and autograd's backward -
                                   forward and backward on scores that hold the bias
Every form is captured once into a graph of --launches calls; the graphs are then replayed in turn, --reps rounds, so the forms
alternate in one process on one clock: device-event time per call, the best of the rounds and the spread (max / min).  *_tbs is the
traffic the form has to move (a live row read and written, a masked row written) over that time, to be read beside the 6.29 TB/s
streaming read the README quotes.
  step_loss_ms / step_objective_ms the whole training step of the plain PTB model (2 layers, rank 32, T 35, B 32, dropout 0.5):
                                   forward, loss, backward - Model.loss with its defaults against Model.loss with lengths, all four
                                   terms, the default negatives and normalize="tokens", wall clock
One JSON object per line.  `python tools/bench_objective.py [--out FILE] [--rows 1120,8960] [--reps 5] [--launches 10]`"""
import argparse
import ctypes
import json
import os
import sys

import torch

from _timing import wall_ms
from bench_distill import alternated_us

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

V, H, K = 10000, 650, 35


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="1120,8960")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    a = ap.parse_args()
    from vmlmf_amd import Model, _lib, unit_gradient
    from vmlmf_amd import functional as F
    lib, _ptr = _lib.lib(), _lib.ptr
    dev = torch.device("cuda", torch.cuda.current_device())
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    torch.manual_seed(0)
    eps, zeta, alpha, B = 0.1, 1e-4, 0.5, 32
    for R in [int(r) for r in a.rows.split(",")]:
        rec = {"what": "launch", "R": R, "V": V, "K": K, "label_smoothing": eps, "z_loss": zeta, "unlikelihood": alpha,
               "launches": a.launches, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
        scores = 2.0 * torch.randn((R, V), device=dev)
        bias = torch.randn(V, device=dev)
        y = torch.randint(0, V, (R,), device=dev)
        ym = y.clone()
        ym[2::8] = -1
        masked = int((ym == -1).sum())
        neg = torch.randint(0, V, (R, K), device=dev)
        stats, db = torch.empty(5 + 4 * R, device=dev), torch.empty(V, device=dev)
        scratch = torch.empty(max(lib.vmlmf_objective_scratch_floats(R, V), lib.vmlmf_nll_grad_scratch_floats(R, V)), device=dev)
        scale, stream = ctypes.c_float(B / R), lambda: _lib.raw_stream(dev)

        def fused(e, z, u):   # (in place: from the second call on the scores are the previous call's gradient - the same traffic)
            obj = _lib.Objective(label_smoothing=e, z_loss=z, unlikelihood=u, negatives=neg.data_ptr() if u > 0 else None, k=K if u > 0 else 0)
            return lambda: _lib.check(lib.vmlmf_objective_forward_grad(R, V, _ptr(scores), _ptr(bias), _ptr(ym), scale, ctypes.byref(obj),
                                                                       _ptr(stats), stats.data_ptr() + 20, _ptr(db), _ptr(scratch), stream()))

        def nll():
            _lib.check(lib.vmlmf_nll_forward_grad(R, V, _ptr(scores), _ptr(bias), _ptr(y), scale, _ptr(stats), stats.data_ptr() + 4, _ptr(db),
                                                  _ptr(scratch), stream()))

        sb = (2.0 * torch.randn((R, V), device=dev) + bias).requires_grad_(True)
        y2 = ym.view(-1, B)

        def stock(e, z, u):
            def body():
                sb.grad = None
                F.objective_loss_stock(sb, y2, label_smoothing=e, z_loss=z, unlikelihood=u, negatives=neg if u > 0 else None)[0].backward()
            return body

        got = alternated_us({"fused_mask": fused(0.0, 0.0, 0.0), "fused_smooth_z": fused(eps, zeta, 0.0), "fused_ul35": fused(0.0, 0.0, alpha),
                             "fused_all": fused(eps, zeta, alpha), "nll": nll, "stock_mask": stock(0.0, 0.0, 0.0),
                             "stock_all": stock(eps, zeta, alpha)}, a.launches, a.reps)
        for name, (best, spread) in got.items():
            rec[f"{name}_us"], rec[f"{name}_spread"] = round(best, 2), round(spread, 3)
            if not name.startswith("stock"):
                rows_moved = 2 * R if name == "nll" else 2 * (R - masked) + masked
                rec[f"{name}_tbs"] = round(rows_moved * V * 4 / (best * 1e-6) / 1e12, 3)
        for name in ("fused_mask", "fused_smooth_z", "fused_ul35", "fused_all"):
            rec[f"{name}_over_nll"] = round(got[name][0] / got["nll"][0], 3)
        rec["stock_over_fused_mask"] = round(got["stock_mask"][0] / got["fused_mask"][0], 2)
        rec["stock_over_fused_all"] = round(got["stock_all"][0] / got["fused_all"][0], 2)
        emit(rec)
        del scores, sb, scratch, got
        torch.cuda.empty_cache()
    T = 35
    m = Model(V, H, 2, 0.5, 0.05, w_rank=32, u_ranks=[32], lstm_type="vmlmf").cuda().train()
    x, y = torch.randint(0, V, (T, B), device=dev), torch.randint(0, V, (T, B), device=dev)
    lengths = torch.randint(T // 2, T + 1, (B,), device=dev)
    unit = unit_gradient(dev)
    rec = {"what": "step", "T": T, "B": B, "V": V, "H": H, "reps": a.reps, "device": torch.cuda.get_device_name(0)}

    def step(loss_of):
        def body():
            m.zero_grad(set_to_none=True)
            loss_of().backward(unit)
        return body
    forms = {"step_loss": lambda: m.loss(x, y, m.state_init(B))[0],
             "step_objective": lambda: m.loss(x, y, m.state_init(B), lengths=lengths, label_smoothing=eps, z_loss=zeta, unlikelihood=alpha,
                                              normalize="tokens")[0]}
    for _ in range(2):                                   # the forms in turn, twice: the second round's numbers beside the first's
        for name, loss_of in forms.items():
            best, spread = wall_ms(step(loss_of), a.reps, calls=5, warm=2)
            rec.setdefault(f"{name}_ms", []).append(round(best, 4))
            rec.setdefault(f"{name}_spread", []).append(round(spread, 3))
    emit(rec)
    if out:
        out.close()


if __name__ == "__main__":
    main()
