"""What the distillation loss costs at the LM head (functional.lm_head_distill_loss: vmlmf_distill_forward_grad, two launches,
csrc/vmlmf_head_loss.hip), at the PTB width V 10 000: R = 1120 rows (35 x 32, the LM step at 32 rows) and R = 8960 (35 x 256,
BASELINE configs[4] on one GPU).
  fused_dense_us / fused_top8_us   the launch pair on a fixed (R, V) score matrix with a bias, alpha 0.5, tau 2: the teacher as an
                                   (R, V) score matrix, or as 8 tokens and scores per row
  nll_us                           vmlmf_nll_forward_grad on the same matrix: the hard loss alone, the launch pair Model.loss makes
  stock_dense_us / stock_top8_us   functional.distill_loss_stock - two log_softmax, kl_div, cross_entropy and autograd's backward -
                                   forward and backward on scores that hold the bias
Every form is captured once into a graph of --launches calls; the graphs are then replayed in turn, --reps rounds, so the forms
alternate in one process on one clock: device-event time per call, the best of the rounds and the spread (max / min).  *_tbs is the
traffic the form has to move (dense: the scores read and written and the teacher read, three matrices; top-8 and the NLL: two)
over that time, to be read beside the 6.29 TB/s streaming read the README quotes.
  step_loss_ms / step_distill_dense_ms / step_distill_top8_ms   the whole training step of the plain PTB model (2 layers, rank
                                   32, T 35, B 32, dropout 0.5): forward, loss, backward - Model.loss against Model.distill_loss
                                   with an offline teacher (tensors), wall clock
One JSON object per line.  `python tools/bench_distill.py [--out FILE] [--rows 1120,8960] [--reps 5] [--launches 10]`"""
import argparse
import ctypes
import json
import os
import sys

import torch

from _timing import wall_ms

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

V, H = 10000, 650


def alternated_us(bodies, n, reps, warm=2):
    """{name: (best us per call, max / min)}: every body captured into a graph of n calls after `warm` eager ones; reps rounds, each
    replaying every graph once, in turn."""
    graphs = {}
    for name, body in bodies.items():
        for _ in range(warm):
            body()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(n):
                body()
        g.replay()
        graphs[name] = g
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = {name: [] for name in graphs}
    for _ in range(reps):
        for name, g in graphs.items():
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            ts[name].append(1e3 * e0.elapsed_time(e1) / n)
    return {name: (min(t), max(t) / min(t)) for name, t in ts.items()}


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
    alpha, tau, B = 0.5, 2.0, 32
    for R in [int(r) for r in a.rows.split(",")]:
        rec = {"what": "launch", "R": R, "V": V, "alpha": alpha, "tau": tau, "launches": a.launches, "reps": a.reps,
               "device": torch.cuda.get_device_name(0)}
        scores = 2.0 * torch.randn((R, V), device=dev)
        bias = torch.randn(V, device=dev)
        y = torch.randint(0, V, (R,), device=dev)
        teacher = 2.0 * torch.randn((R, V), device=dev)
        tsc, tok = teacher.topk(8, dim=-1)
        tok, tsc = tok.contiguous(), tsc.contiguous()
        stats, db = torch.empty(3 + 2 * R, device=dev), torch.empty(V, device=dev)
        scratch = torch.empty(max(lib.vmlmf_distill_scratch_floats(R, V), lib.vmlmf_nll_grad_scratch_floats(R, V)), device=dev)
        scale, stream = ctypes.c_float(B / R), lambda: _lib.raw_stream(dev)
        kd_dense = _lib.Distill(alpha=alpha, temperature=tau, teacher=teacher.data_ptr())
        kd_top = _lib.Distill(alpha=alpha, temperature=tau, top_tokens=tok.data_ptr(), top_scores=tsc.data_ptr(), top=8)

        def fused(kd):      # (in place: from the second call on the scores are the previous call's gradient - the same traffic)
            return lambda: _lib.check(lib.vmlmf_distill_forward_grad(R, V, _ptr(scores), _ptr(bias), _ptr(y), scale, ctypes.byref(kd), _ptr(stats),
                                                                     stats.data_ptr() + 12, _ptr(db), _ptr(scratch), stream()))

        def nll():
            _lib.check(lib.vmlmf_nll_forward_grad(R, V, _ptr(scores), _ptr(bias), _ptr(y), scale, _ptr(stats), stats.data_ptr() + 4, _ptr(db),
                                                  _ptr(scratch), stream()))

        sb = (2.0 * torch.randn((R, V), device=dev) + bias).requires_grad_(True)
        y2 = y.view(-1, B)

        def stock(t):
            def body():
                sb.grad = None
                F.distill_loss_stock(sb, y2, t, alpha, tau)[0].backward()
            return body

        got = alternated_us({"fused_dense": fused(kd_dense), "fused_top8": fused(kd_top), "nll": nll, "stock_dense": stock(teacher),
                             "stock_top8": stock((tok, tsc))}, a.launches, a.reps)
        matrices = {"fused_dense": 3, "fused_top8": 2, "nll": 2}
        for name, (best, spread) in got.items():
            rec[f"{name}_us"], rec[f"{name}_spread"] = round(best, 2), round(spread, 3)
            if name in matrices:
                rec[f"{name}_tbs"] = round(matrices[name] * R * V * 4 / (best * 1e-6) / 1e12, 3)
        for name in ("fused_dense", "fused_top8"):
            rec[f"{name}_over_nll"] = round(got[name][0] / got["nll"][0], 3)
        rec["stock_over_fused_dense"] = round(got["stock_dense"][0] / got["fused_dense"][0], 2)
        rec["stock_over_fused_top8"] = round(got["stock_top8"][0] / got["fused_top8"][0], 2)
        emit(rec)
        del scores, teacher, sb, scratch, got
        torch.cuda.empty_cache()
    T = 35
    m = Model(V, H, 2, 0.5, 0.05, w_rank=32, u_ranks=[32], lstm_type="vmlmf").cuda().train()
    x, y = torch.randint(0, V, (T, B), device=dev), torch.randint(0, V, (T, B), device=dev)
    teacher = 2.0 * torch.randn((T, B, V), device=dev)
    tsc, tok = teacher.topk(8, dim=-1)
    unit = unit_gradient(dev)
    rec = {"what": "step", "T": T, "B": B, "V": V, "H": H, "reps": a.reps, "device": torch.cuda.get_device_name(0)}

    def step(loss_of):
        def body():
            m.zero_grad(set_to_none=True)
            loss_of().backward(unit)
        return body
    forms = {"step_loss": lambda: m.loss(x, y, m.state_init(B))[0],
             "step_distill_dense": lambda: m.distill_loss(x, y, m.state_init(B), teacher, alpha=alpha, temperature=tau)[0],
             "step_distill_top8": lambda: m.distill_loss(x, y, m.state_init(B), (tok, tsc), alpha=alpha, temperature=tau)[0]}
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
