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
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

V, H, N, TOPS = 10000, 650, 50, (0, 8, 32)


def replayed_us(launch, reps, n=N):
    """us per call of launch() (best of `reps` replays of a graph of n calls); replayed_us.spread: max / min over the replays."""
    for _ in range(3):
        launch()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            launch()
    g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(1e3 * e0.elapsed_time(e1) / n)
    replayed_us.spread = max(ts) / min(ts)
    return min(ts)


def eager_ms(call, reps, n=5):
    """ms per call() (best of `reps` timings of n calls between synchronisations); eager_ms.spread: max / min."""
    for _ in range(2):
        call()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            call()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0) / n)
    eager_ms.spread = max(ts) / min(ts)
    return min(ts)


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
            rec[f"launch_top{top}_us"] = round(replayed_us(lambda: _score.score_rows(scores, bias, y, top, lp, rank, toks, tlp), a.reps), 3)
            rec[f"launch_top{top}_spread"] = round(replayed_us.spread, 3)
            rec[f"stock_top{top}_us"] = round(replayed_us(lambda: stock(sb, y, top), a.reps), 3)
            rec[f"stock_top{top}_spread"] = round(replayed_us.spread, 3)
        rec["choose_us"] = round(replayed_us(lambda: _lib.check(_lib.lib().vmlmf_lm_choose(
            R, H, V, _ptr(scores), _ptr(bias), None, 0.0, None, 0, _ptr(tok), _ptr(lp), None, _lib.raw_stream(dev))), a.reps), 3)
        rec["choose_spread"] = round(replayed_us.spread, 3)
        emit(rec)
    T, B = 35, 32
    cache_packed_parameters(m)
    x = torch.randint(0, V, (T + 1, B), device=dev)
    rec = {"what": "model", "T": T, "B": B, "V": V, "H": H, "reps": a.reps, "device": torch.cuda.get_device_name(0)}

    def stock_model(top):
        with torch.no_grad():
            return stock(m(x[:-1], m.state_init(B))[0], x[1:].reshape(-1), top)
    for top in (0, 8):
        rec[f"model_score_top{top}_ms"] = round(eager_ms(lambda: m.score(x, top=top), a.reps), 4)
        rec[f"model_score_top{top}_spread"] = round(eager_ms.spread, 3)
        rec[f"model_stock_top{top}_ms"] = round(eager_ms(lambda: stock_model(top), a.reps), 4)
        rec[f"model_stock_top{top}_spread"] = round(eager_ms.spread, 3)
    emit(rec)
    if out:
        out.close()


if __name__ == "__main__":
    main()
