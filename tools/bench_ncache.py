"""What scoring under a continuous cache costs (Model.cache_score / lm_cache_score: ONE launch of libvmlmf_ncache.so per call,
include/vmlmf_ncache.h), at the PTB hidden size 650, with a full cache (n = window pairs carried into the call).
  launch_us            the vmlmf_ncache_score launch ALONE on fixed buffers at (B, T, window) = (10, 35, 500), (1, 70, 2000) and
                       (32, 35, 500), parts automatic; 50 launches replayed from a graph, us per launch
  launch_parts<P>_us   the same with `parts` forced
  stock_us             the same rule in stock ops on the same tensors, replayed the same way: bmm, the band mask, two logsumexp,
                       logaddexp (the baseline, not code under test); the masks are built outside the timed region
  model_cache_score_ms Model.cache_score of the plain PTB model (2 layers, rank 32, V 10 000) per chunk of T 35 at B 10, window 500,
                       the cache full, states and cache carried: includes the copy into the (B, n + T, H) buffer
  model_score_ms       Model.score over the same chunks
The expectation this checks (docs/design/lm_ncache.md): launch_us < stock_us at all three shapes, by more than the spreads recorded.
Best of --reps, and the spread (max / min).  One JSON object per line.
`python tools/bench_ncache.py [--out FILE] [--reps 5]`"""
import argparse
import json
import math
import os
import sys

import torch

from _timing import replayed_us, wall_ms

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

H, V, N = 650, 10000, 50
SHAPES = ((10, 35, 500), (1, 70, 2000), (32, 35, 500))
PARTS = (1, 2, 4, 8, 16, 32)
THETA, LAM = 0.3, 0.1


def timed(rec, key, unit, timing, digits):
    """rec[<key>_<unit>], rec[<key>_spread] from a timer's (best, spread)."""
    rec[f"{key}_{unit}"], rec[f"{key}_spread"] = round(timing[0], digits), round(timing[1], 3)


def stock(keys, toks, lv, n, band, theta, lam):
    """The rule in stock ops: (logp, cache_logp) (T, B).  band (T, L) bool: the pairs of each position's band."""
    s = theta * torch.bmm(keys[:, n:], keys.transpose(1, 2))
    s = s.masked_fill(~band, -math.inf)
    z = torch.logsumexp(s, -1)
    hit = torch.logsumexp(s.masked_fill(toks[:, None, :] != toks[:, n:, None], -math.inf), -1)
    lc = (hit - z).t()
    return torch.logaddexp(math.log1p(-lam) + lv, math.log(lam) + lc), lc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from vmlmf_amd import Model, NeuralCache, _lib, _ncache, cache_packed_parameters
    ptr = _lib.ptr
    dev = torch.device("cuda", torch.cuda.current_device())
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    torch.manual_seed(0)
    for B, T, window in SHAPES:
        n, L = window, window + T
        rec = {"what": "launch", "B": B, "T": T, "window": window, "n": n, "H": H, "launches": N, "reps": a.reps,
               "device": torch.cuda.get_device_name(0)}
        keys = torch.tanh(torch.randn((B, L, H), device=dev))
        toks = torch.randint(0, V // 100, (B, L), device=dev)
        lv = -5 * torch.rand((T, B), device=dev) - 0.01
        logp, lc = torch.empty((T, B), device=dev), torch.empty((T, B), device=dev)
        ticket = torch.zeros(B * -(-T // 16), device=dev, dtype=torch.int32)
        ws = torch.empty(_ncache.workspace_bytes(B, T, n, window) // 4, device=dev)
        pos = torch.arange(L, device=dev)[None, :] - (n + torch.arange(T, device=dev))[:, None]
        band = (pos < 0) & (pos >= -window)

        def launch(parts):
            _ncache.LIBRARY.call(dev, "vmlmf_ncache_score", B, T, n, H, window, THETA, LAM, ptr(keys), ptr(toks), ptr(lv), ptr(logp), ptr(lc),
                                 ptr(ticket), ptr(ws), ws.numel() * 4, parts)

        launch(0)
        want_p, want_c = stock(keys, toks, lv, n, band, THETA, LAM)
        fin = torch.isfinite(want_c)
        rec["max_abs_diff_logp"] = float((logp - want_p).abs().max())
        rec["max_abs_diff_cache_logp"] = float((lc - want_c)[fin].abs().max()) if bool(fin.any()) else 0.0
        rec["same_infinities"] = bool(torch.equal(torch.isfinite(lc), fin))
        timed(rec, "launch", "us", replayed_us(lambda j: launch(0), N, a.reps), 3)
        timed(rec, "stock", "us", replayed_us(lambda j: stock(keys, toks, lv, n, band, THETA, LAM), N, a.reps), 3)
        for parts in PARTS:
            timed(rec, f"launch_parts{parts}", "us", replayed_us(lambda j: launch(parts), N, a.reps), 3)
        emit(rec)
    T, B, window = 35, 10, 500
    m = Model(V, H, 2, 0.0, 0.05, w_rank=32, u_ranks=[32], lstm_type="vmlmf").cuda().eval()
    cache_packed_parameters(m)
    x = torch.randint(0, V, (T + 1, B), device=dev)
    rec = {"what": "model", "T": T, "B": B, "V": V, "H": H, "window": window, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    carried = {"states": None, "cache": NeuralCache(B, H, dev, window), "plain": None}

    def chunk():
        _, carried["states"], carried["cache"] = m.cache_score(x, window=window, cache=carried["cache"], states=carried["states"])

    def plain():
        carried["plain"] = m.score(x, states=carried["plain"])[-1]

    timed(rec, "model_cache_score", "ms", wall_ms(chunk, a.reps, calls=5, warm=16), 4)       # 16 chunks of 35 fill the 500 pairs
    rec["cache_pairs"] = carried["cache"].n
    timed(rec, "model_score", "ms", wall_ms(plain, a.reps, calls=5, warm=16), 4)
    emit(rec)
    if out:
        out.close()


if __name__ == "__main__":
    main()
