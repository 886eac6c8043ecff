"""What the history controls of Model.generate cost (no_repeat_ngram_size, banned_sequences, frequency_penalty, presence_penalty: one
launch of libvmlmf_history.so behind the head's GEMM, include/vmlmf_history.h), at the PTB size: V 10 000, H 650, B in {1, 32},
histories of 64 and 1024 tokens.
  choice_*   the choice launch ALONE on a fixed (B, V) score matrix, 50 launches replayed from a graph, us per launch, unfiltered
             and with top_k 40 / top_p 0.9 (`_filtered`):
               decode        vmlmf_decode_choose of THIS tree, every common control on (bench_decode_controls.all_controls: theta 1.2, a
                             logit_bias with 5 % bans, 30 % of each row seen, eos held back): the yardstick
               neutral       vmlmf_history_choose on the same scores and the same common controls, the history's controls off
               history_L     ... with every control on: n = 3, three banned sequences, alpha 0.4, beta 0.6, over a history of L tokens
                             drawn from 50 (so n-grams do repeat) and the counts of its last L / 2.  The history is FULL (capacity
                             L): every launch scans L tokens, sets `overflow` and leaves the history as it is, so all 50 launches of
                             a replay do the same work
  graph_*    whole decode steps: a DecodeGraph of 16 steps of the plain32 model, replayed, ms per token, with the common controls
             and with no_repeat_ngram_size = 3 added to them
Best of --reps replays, and the spread (max / min).  One JSON object per line.
`python tools/bench_history_controls.py [--out FILE] [--batches 1,32] [--lengths 64,1024] [--reps 5]`"""
import argparse
import json
import os
import sys

import torch

from _timing import replayed_us, wall_ms
from bench_decode_controls import H, N, TOP_K, TOP_P, V, all_controls

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

NGRAM, ALPHA, BETA, ALPHABET = 3, 0.4, 0.6, 50


def history_controls(B, dev, L, on, prompt=None, capacity=None):
    """all_controls' controls as a HistoryControls; `on`: every history control too, over a full history of L tokens."""
    from vmlmf_amd import HistoryControls
    base = all_controls(B, dev)
    g = torch.Generator().manual_seed(777)
    alphabet = torch.randperm(V, generator=g)[:ALPHABET]
    a = alphabet.tolist()
    kw = dict(no_repeat_ngram_size=NGRAM, banned_sequences=[[a[0], a[1]], [a[2]], [a[3], a[4], a[5]]], frequency_penalty=ALPHA,
              presence_penalty=BETA) if on else dict()
    c = HistoryControls(B, V, dev, eos=3, min_length=1 << 30, repetition_penalty=1.2, logit_bias=base.logit_bias.cpu(), prompt=prompt,
                        capacity=L if capacity is None else capacity, **kw)
    c.seen.copy_(base.seen)
    if prompt is None:
        hist = alphabet[torch.randint(0, ALPHABET, (B, L), generator=g)]
        c.hist.copy_(hist.to(torch.int32))
        c.hist_len.fill_(L)
        count = torch.zeros((B, V), dtype=torch.int64).scatter_add_(1, hist[:, L // 2:], torch.ones((B, L - L // 2), dtype=torch.int64))
        c.count.copy_(torch.from_numpy(count.numpy().astype("uint16")))
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--lengths", default="64,1024")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from vmlmf_amd import DecodeGraph, Model, _decode, _history, _lib, dropout_advance
    dev = torch.device("cuda", torch.cuda.current_device())
    out = open(a.out, "a") if a.out else None
    lengths = [int(x) for x in a.lengths.split(",")]
    torch.manual_seed(0)
    m = Model(V, H, 2, 0.0, 0.05, w_rank=32, u_ranks=[32], lstm_type="vmlmf").cuda().eval()
    for B in [int(b) for b in a.batches.split(",")]:
        rec = {"B": B, "V": V, "H": H, "top_k": TOP_K, "top_p": TOP_P, "launches": N, "ngram": NGRAM, "alpha": ALPHA, "beta": BETA,
               "lib": os.path.basename(os.path.dirname(_lib.LIB_PATH)), "device": torch.cuda.get_device_name(0)}
        prompt = torch.randint(0, V, (4, B), device=dev)
        with torch.no_grad():
            h, st = m.features(prompt, m.state_init(B))
        hv = h[-1].contiguous()
        snap = dropout_advance(m.sampler_state(1))
        scores = torch.mm(hv, m.fc.w.t())
        bias, embed = m.fc.b.detach().contiguous(), m.embed.w.detach().contiguous()
        tok = torch.empty(B, device=dev, dtype=torch.int64)
        lp, kept, xn = torch.empty(B, device=dev), torch.empty(B, device=dev, dtype=torch.int32), torch.empty((B, H), device=dev)
        for suffix, k, p in (("", 0, 1.0), ("_filtered", TOP_K, TOP_P)):
            ctl = all_controls(B, dev)
            us, spread = replayed_us(lambda j: _decode.decode_choose(scores, bias, embed, 1.0, k, p, snap, j, ctl, tok, lp, xn, kept), N, a.reps)
            rec[f"choice_decode{suffix}_us"], rec[f"choice_decode{suffix}_spread"] = round(us, 3), round(spread, 3)
            cases = [("neutral", lengths[0], False)] + [(f"history_{L}", L, True) for L in lengths]
            for name, L, on in cases:
                ctl = history_controls(B, dev, L, on)
                us, spread = replayed_us(lambda j: _history.history_choose(scores, bias, embed, 1.0, k, p, snap, j, ctl, tok, lp, xn, kept), N,
                                         a.reps)
                rec[f"choice_{name}{suffix}_us"], rec[f"choice_{name}{suffix}_spread"] = round(us, 3), round(spread, 3)
                rec[f"choice_{name}{suffix}_over_decode"] = round(us / rec[f"choice_decode{suffix}_us"], 4)
                assert not ctl.finished.any() and (ctl.hist_len == L).all() and ctl.overflow.all()
        K = 16
        for name, ngram in (("controlled", False), ("ngram3", True)):
            if ngram:
                from vmlmf_amd import HistoryControls
                base = all_controls(B, dev, prompt)
                ctl = HistoryControls(B, V, dev, eos=3, min_length=1 << 30, repetition_penalty=1.2, logit_bias=base.logit_bias.cpu(), prompt=prompt,
                                      capacity=4096, no_repeat_ngram_size=NGRAM)
                ctl.seen.copy_(base.seen)
            else:
                ctl = all_controls(B, dev, prompt)
            g = DecodeGraph(m, hv, st, K, temperature=1.0, top_k=TOP_K, top_p=TOP_P, controls=ctl)
            g.replay()
            ms, spread = wall_ms(g.graph.replay, a.reps, calls=4)
            rec[f"graph_{name}_ms_per_token"] = round(ms / K, 5)
            rec[f"graph_{name}_spread"] = round(spread, 3)
            del g
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
