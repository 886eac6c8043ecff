"""What the truncation samplers of Model.generate cost (min_p, typical_p, epsilon_cutoff, eta_cutoff: one launch of
libvmlmf_truncate.so behind the head's GEMM, include/vmlmf_truncate.h), at the PTB size: V 10 000, H 650, B in {1, 32, 256}.
  choice_*   the choice launch ALONE on a fixed (B, V) score matrix, 50 launches replayed from a graph, us per launch:
               minp / typ / eps / eta / all   vmlmf_truncate_choose with the settings of tests/truncation_cases.py
               unfiltered, top_p              vmlmf_lm_choose and vmlmf_lm_choose_filtered (top_p 0.9): the parent's kernels, untouched
               parent_*                       those two from another build of libvmlmf_hip.so (--parent-lib FILE: the parent
                                              commit's, opened beside this tree's in the same process: one session)
  stock_*    the same stages stated in stock ops on the same scores - softmax, sort, cumsum, masks, multinomial -, the ops of one
             choice captured and replayed the same way (us per choice)
  graph_*    whole decode steps: a DecodeGraph of 16 steps of the plain model, replayed, ms per token, for no filter, min_p and typ
Best of --reps replays, and the spread (max / min).  One JSON object per line.
`python tools/bench_truncation.py [--out FILE] [--batches 1,32,256] [--reps 5] [--parent-lib FILE]`"""
import argparse
import json
import os
import sys

import torch

from _timing import replayed_us, wall_ms
from bench_decode_controls import open_parent

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

V, H, N = 10000, 650, 50
SETTINGS = {"minp": (None, None, dict(min_p=0.1)), "typ": (None, None, dict(typical_p=0.9)), "eps": (None, None, dict(epsilon_cutoff=2.0 / V)),
            "eta": (None, None, dict(eta_cutoff=8.0 / V)),
            "all": (50, 0.95, dict(min_p=0.02, typical_p=0.9, epsilon_cutoff=0.5 / V))}
NEG = float("-inf")


def stock_choice(x, tau, top_k, top_p, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
    """The stages in stock ops, as Hugging Face's warpers state them: x (B, V) scores with the bias -> tokens (B)."""
    z = x / tau
    if top_k:
        z = z.masked_fill(z < torch.topk(z, top_k).values[:, -1:], NEG)
    if top_p is not None and top_p < 1.0:
        s, i = torch.sort(z, descending=True)
        pr = torch.softmax(s, -1)
        drop = (pr.cumsum(-1) - pr) >= top_p
        z = z.masked_fill(drop.scatter(1, i, drop), NEG)
    if min_p > 0.0:
        pr = torch.softmax(z, -1)
        z = z.masked_fill(pr < min_p * pr.max(-1, keepdim=True).values, NEG)
    if typical_p < 1.0:
        ls = torch.log_softmax(z, -1)
        pr = ls.exp()
        ent = -(ls * pr).nansum(-1, keepdim=True)
        d, i = torch.sort((-ls - ent).abs(), descending=False)
        before = pr.gather(-1, i).cumsum(-1) - pr.gather(-1, i)
        drop = before >= typical_p
        z = z.masked_fill(drop.scatter(1, i, drop), NEG)
    for cut, eta in ((epsilon_cutoff, False), (eta_cutoff, True)):
        if cut > 0.0:
            pr = torch.softmax(z, -1)
            thr = cut
            if eta:
                ent = -(pr * torch.log_softmax(z, -1)).nansum(-1, keepdim=True)
                thr = torch.minimum(torch.full_like(ent, cut), (cut ** 0.5) * torch.exp(-ent))
            z = z.masked_fill((pr < thr) & (z < z.max(-1, keepdim=True).values), NEG)
    return torch.multinomial(torch.softmax(z, -1), 1)[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1,32,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    from vmlmf_amd import DecodeGraph, Model, Truncation, _lib, _truncate, dropout_advance
    _ptr = _lib.ptr
    dev = torch.device("cuda", torch.cuda.current_device())
    out = open(a.out, "a") if a.out else None
    libs = [("", _lib.lib())] + ([("parent_", open_parent(a.parent_lib))] if a.parent_lib else [])
    torch.manual_seed(0)
    m = Model(V, H, 2, 0.0, 0.05, w_rank=32, u_ranks=[32], lstm_type="vmlmf").cuda().eval()
    for B in [int(b) for b in a.batches.split(",")]:
        rec = {"B": B, "V": V, "H": H, "launches": N, "device": torch.cuda.get_device_name(0)}
        prompt = torch.randint(0, V, (4, B), device=dev)
        with torch.no_grad():
            h, st = m.features(prompt, m.state_init(B))
        hv = h[-1].contiguous()
        snap = dropout_advance(m.sampler_state(1))
        scores = torch.mm(hv, m.fc.w.t())
        bias, embed = m.fc.b.detach().contiguous(), m.embed.w.detach().contiguous()
        tok = torch.empty(B, device=dev, dtype=torch.int64)
        lp, kept, xn = torch.empty(B, device=dev), torch.empty(B, device=dev, dtype=torch.int32), torch.empty((B, H), device=dev)
        stream = lambda: _lib.raw_stream(dev)
        for prefix, lib in libs:
            def plain(j, lib=lib):
                _lib.check(lib.vmlmf_lm_choose(B, H, V, _ptr(scores), _ptr(bias), _ptr(embed), 1.0, _ptr(snap), j, _ptr(tok), _ptr(lp), _ptr(xn),
                                               stream()))

            def top_p(j, lib=lib):
                _lib.check(lib.vmlmf_lm_choose_filtered(B, H, V, _ptr(scores), _ptr(bias), _ptr(embed), 1.0, 0, 0.9, _ptr(snap), j, _ptr(tok),
                                                        _ptr(lp), _ptr(xn), _ptr(kept), stream()))
            for name, fn in (("unfiltered", plain), ("top_p", top_p)):
                us, spread = replayed_us(fn, N, a.reps)
                rec[f"choice_{prefix}{name}_us"], rec[f"choice_{prefix}{name}_spread"] = round(us, 3), round(spread, 3)
        x = scores + bias
        for name, (k, p, kw) in SETTINGS.items():
            t = Truncation(**kw)
            us, spread = replayed_us(lambda j: _truncate.truncate_choose(scores, bias, embed, 1.0, k or 0, p or 1.0, t, snap, j, None, tok, lp, xn,
                                                                         kept), N, a.reps)
            rec[f"choice_{name}_us"], rec[f"choice_{name}_spread"], rec[f"kept_{name}"] = round(us, 3), round(spread, 3), int(kept.max())
            us, spread = replayed_us(lambda j: stock_choice(x, 1.0, k, p, **kw), 10, a.reps)
            rec[f"stock_{name}_us"], rec[f"stock_{name}_spread"] = round(us, 3), round(spread, 3)
            rec[f"stock_{name}_launches"] = 10
        K = 16
        for name, kw in (("plain", dict()), ("minp", SETTINGS["minp"][2]), ("typ", SETTINGS["typ"][2])):
            g = DecodeGraph(m, hv, st, K, temperature=1.0, **kw)
            g.replay()
            ms, spread = wall_ms(g.graph.replay, a.reps, calls=4)
            rec[f"graph_{name}_ms_per_token"], rec[f"graph_{name}_spread"] = round(ms / K, 5), round(spread, 3)
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
