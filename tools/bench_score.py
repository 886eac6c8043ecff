"""What scoring given text costs (Model.score / lm_score: per chunk of rows the head's GEMM and ONE launch of libvmlmf_score.so,
include/vmlmf_score.h), at the PTB size: V 10 000, H 650.
  launch_top{0,8,32}_us   the vmlmf_score_rows launch ALONE on a fixed (R, V) score matrix, R in {32, 1120} (1120 = 35 x 32, a PTB
                          minibatch), with the bias and a target in every row; 50 launches replayed from a graph, us per launch
  stock_top{0,8,32}_us    the same rows through stock ops, replayed the same way, on scores that already hold the bias:
                          log_softmax, gather (the log-probability), a comparison with the target's score summed over the row (the
                          rank, ties not even looked at) and, with top > 0, topk
  choose_us               vmlmf_lm_choose (greedy) on the same matrix: the sampler's one-pass launch, whose row loop the scoring
                          launch shares - what the rank and the keys add to it
  model_score_top{0,8}_ms Model.score of the plain PTB model (2 layers, rank 32) over T 35, B 32, eager, kept parameter images
  model_stock_top{0,8}_ms the stock spelling on the same model: log_softmax(model(x, states)[0]), then the same ops
The expectation this checks (docs/design/lm_score.md): at top = 0 the stock form makes at least three passes and three launches over
the rows, the new launch one - so launch_top0_us <= stock_top0_us at both R.
Best of --reps, and the spread (max / min).  One JSON object per line.
`python tools/bench_score.py [--out FILE] [--rows 32,1120] [--reps 5]`"""
import argparse
import json
import os
import sys

import torch

from _timing import replayed_us, wall_ms

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

V, H, N, TOPS = 10000, 650, 50, (0, 8, 32)


def timed(rec, key, unit, timing, digits):
    """rec[<key>_<unit>], rec[<key>_spread] from a timer's (best, spread)."""
    rec[f"{key}_{unit}"], rec[f"{key}_spread"] = round(timing[0], digits), round(timing[1], 3)


def stock(sb, y, top):
    """The stock-op form on scores that hold the bias: (logprob, rank[, top_logprob, top_tokens])."""
    lsm = torch.log_softmax(sb, -1)
    lp = lsm.gather(1, y[:, None])
    rank = (lsm > lp).sum(1)
    return (lp, rank) if top == 0 else (lp, rank, *torch.topk(lsm, top, -1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="32,1120")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from vmlmf_amd import Model, _lib, _score, cache_packed_parameters
    _ptr = _lib.ptr
    dev = torch.device("cuda", torch.cuda.current_device())
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    torch.manual_seed(0)
    m = Model(V, H, 2, 0.0, 0.05, w_rank=32, u_ranks=[32], lstm_type="vmlmf").cuda().eval()
    bias = m.fc.b.detach().contiguous()
    for R in [int(r) for r in a.rows.split(",")]:
        rec = {"what": "launch", "R": R, "V": V, "launches": N, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
        hrows = 0.5 * torch.randn((R, H), device=dev)
        scores = torch.mm(hrows, m.fc.w.detach().t())
        sb = scores + bias
        y = torch.randint(0, V, (R,), device=dev)
        lp, rank = torch.empty(R, device=dev), torch.empty(R, device=dev, dtype=torch.int32)
        tok = torch.empty(R, device=dev, dtype=torch.int64)
        for top in TOPS:
            toks = torch.empty((R, max(top, 1)), device=dev, dtype=torch.int64)
            tlp = torch.empty((R, max(top, 1)), device=dev)
            timed(rec, f"launch_top{top}", "us", replayed_us(lambda j: _score.score_rows(scores, bias, y, top, lp, rank, toks, tlp), N, a.reps), 3)
            timed(rec, f"stock_top{top}", "us", replayed_us(lambda j: stock(sb, y, top), N, a.reps), 3)
        timed(rec, "choose", "us", replayed_us(lambda j: _lib.check(_lib.lib().vmlmf_lm_choose(
            R, H, V, _ptr(scores), _ptr(bias), None, 0.0, None, 0, _ptr(tok), _ptr(lp), None, _lib.raw_stream(dev))), N, a.reps), 3)
        emit(rec)
    T, B = 35, 32
    cache_packed_parameters(m)
    x = torch.randint(0, V, (T + 1, B), device=dev)
    rec = {"what": "model", "T": T, "B": B, "V": V, "H": H, "reps": a.reps, "device": torch.cuda.get_device_name(0)}

    def stock_model(top):
        with torch.no_grad():
            return stock(m(x[:-1], m.state_init(B))[0], x[1:].reshape(-1), top)
    for top in (0, 8):
        timed(rec, f"model_score_top{top}", "ms", wall_ms(lambda: m.score(x, top=top), a.reps, calls=5, warm=2), 4)
        timed(rec, f"model_stock_top{top}", "ms", wall_ms(lambda: stock_model(top), a.reps, calls=5, warm=2), 4)
    emit(rec)
    if out:
        out.close()


if __name__ == "__main__":
    main()
