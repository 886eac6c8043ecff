"""Decoding speed of the PTB LM (Model.generate): ms per token and tokens/s, V 10 000, H 650, two layers, MyVMLSTM rank 32 and
MyVMLSTMGroup ranks [32, 32], for B in {1, 8, 32, 256}.  Paths, same process, same device:
  eager        Model.generate's decode steps (temperature 1), eager: per token the sampler launch + the layers at T = 1 on kept images
  eager_stack  the same with layer_path="stack" (stack_layers' one launch, which packs on every call)
  graph        a DecodeGraph of 16 steps, replayed
  naive        the stock-op loop a user writes without it: embed -> 2 x layer call at T = 1 -> addmm -> softmax -> multinomial
  sampler_*    the sampler alone, both forms (decoding.lm_sample form "fused" / "gemm"), 50 launches replayed from a graph
All four step timings cover the decode steps only (the prompt's pass is outside them); best of --reps, and the spread (max / min).
--top-k K / --top-p P put the filters on in the eager, graph and sampler_* paths (the stock-op loop stays unfiltered); the record carries
them.  --models plain,group picks the models.
One JSON object per line.  `python tools/bench_generate.py [--out FILE] [--batches 1,8,32,256] [--tokens 64] [--sampler-only]
[--top-k K] [--top-p P] [--models plain,group]`."""
import argparse
import json
import os
import sys

import torch

from _timing import replayed_us, wall_ms

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def _model(group):
    from vmlmf_amd import Model
    torch.manual_seed(0)
    if group:
        m = Model.with_group_layers(10000, 650, 2, 0.0, 0.05, w_rank=32, u_ranks=[32, 32])
    else:
        m = Model(10000, 650, 2, 0.0, 0.05, w_rank=32, u_ranks=[32], lstm_type="vmlmf")
    return m.cuda().eval()


def _rec(timing, B, steps):
    """A record of wall_ms()'s (ms, spread) for one pass over `steps` tokens of B rows."""
    ms, spread = timing
    return {"ms_per_token": ms / steps, "tokens_per_s": 1e3 * B * steps / ms, "spread": round(spread, 3)}


def naive(m, x, states, steps):
    """The loop of the issue: no package sampler, no kept images."""
    toks = []
    with torch.no_grad():
        for _ in range(steps):
            h = m.embed.w[x].unsqueeze(0)
            for i, rnn in enumerate(m.rnns):
                h, states[i] = rnn(h, states[i])
            p = torch.softmax(torch.addmm(m.fc.b, h[0], m.fc.w.t()), -1)
            x = torch.multinomial(p, 1)[:, 0]
            toks.append(x)
    return torch.stack(toks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1,8,32,256")
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sampler-only", action="store_true", help="only the sampler launch (e.g. of a probe build named by VMLMF_LIB)")
    ap.add_argument("--top-k", type=int, default=None, help="keep the k most likely tokens (Model.generate's top_k)")
    ap.add_argument("--top-p", type=float, default=None, help="nucleus sampling (Model.generate's top_p)")
    ap.add_argument("--models", default="plain,group")
    a = ap.parse_args()
    filters = {k: v for k, v in (("top_k", a.top_k), ("top_p", a.top_p)) if v is not None}
    from vmlmf_amd import DecodeGraph, dropout_advance, lm_sample
    from vmlmf_amd.decoding import _KeptImages, decode_steps
    dev = torch.device("cuda")
    rows = []
    out = open(a.out, "w") if a.out else None

    def emit(rec):
        rec["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        rows.append(rec)

    K = 16
    steps = a.tokens
    for group in [g == "group" for g in a.models.split(",")]:
        m = _model(group)
        name = "group[32,32]" if group else "plain32"
        for B in [int(b) for b in a.batches.split(",")]:
            prompt = torch.randint(0, 10000, (4, B), device=dev)
            res = dict({"model": name, "B": B, "V": 10000, "H": 650, "tokens": steps}, **filters)
            with torch.no_grad():
                h, st = m.features(prompt, m.state_init(B))
            snap = dropout_advance(m.sampler_state())
            hv = h[-1].contiguous()
            for form in ("fused", "gemm"):
                # the sampler alone: 50 steps replayed from a graph
                us, spread = replayed_us(lambda j: lm_sample(hv, m.fc.w, m.fc.b, 1.0, snap, j, embed=m.embed.w, form=form, **filters), 50, a.reps)
                res["sampler_%s_us" % form] = us
                res["sampler_%s_spread" % form] = round(spread, 3)
                res["sampler_%s_fc_w_GBps" % form] = 10000 * 650 * 4 / (us * 1e-6) / 1e9
            if a.sampler_only:
                emit(res)
                continue
            for path in ("layers", "stack"):
                def eager():
                    with torch.no_grad(), _KeptImages(m):
                        decode_steps(m, hv, [(s0.clone(), s1.clone()) for s0, s1 in st], steps, 1.0, snap, path, **filters)
                t = wall_ms(eager, a.reps)
                res["eager" if path == "layers" else "eager_stack"] = _rec(t, B, steps)
            g = DecodeGraph(m, hv, st, K, temperature=1.0, **filters)
            t = wall_ms(lambda: [g.replay() for _ in range(steps // K)], a.reps)
            res["graph"] = dict(_rec(t, B, steps), chunk=K)
            del g
            x0 = prompt[-1]
            t = wall_ms(lambda: naive(m, x0, [(s0.clone(), s1.clone()) for s0, s1 in st], steps), a.reps)
            res["naive"] = _rec(t, B, steps)
            emit(res)
        del m
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
