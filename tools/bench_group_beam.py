"""Diverse (group) beam search of the PTB LM (Model.group_beam_search): V 10 000, H 650, two MyVMLSTM layers of rank 32, at
(B, W, G) = (1, 4, 2), (1, 16, 4), (32, 4, 2), diversity_penalty 0.5.  Per shape, same process, same device, the same scores of the
head's GEMM:
  group_us                 vmlmf_beamgroup_step, n times in a graph, replayed
  plain_us                 vmlmf_beam_step at the same (B, W), timed the same way (tools/bench_beam.py's select_us)
  stock_us                 the group selection in stock ops - G sequential log_softmax + penalty + topk over a group's Wg V candidates,
                           a scatter_add for the counts, div / mod, the embedding gather (no eos handling, which would add ops)
  step_ms / plain_step_ms / stock_step_ms   the whole decode step per token - head GEMM, selection, state reorder, the layers at T = 1
                           on kept images - as a BeamGraph of 16 steps under a GroupBeams, without controls, and as the same loop with
                           the stock-op group selection, captured the same way
Best of --reps replays each, and the spread (max / min) over them.  One JSON object per line.
--against PATH: a libvmlmf_beam.so built from another commit.  Then nothing of the above is timed; per shape the plain step of that
library and of this tree's are timed alternating, --rounds times each (every round a capture of its own), and every round's figure is
kept: {"B", "W", "other_us": [...], "this_us": [...]}.
`python tools/bench_group_beam.py [--out FILE] [--shapes 1x4x2,1x16x4,32x4x2] [--reps 5] [--against PATH --rounds 6]`."""
import argparse
import json
import os
import sys

import torch

from _timing import replayed_us, wall_ms

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

V, H, L = 10000, 650, 2
K, LAMBDA = 16, 0.5


def _replayed_us(body, n, reps):
    us, spread = replayed_us(lambda j: body(), n, reps)
    return round(us, 3), round(spread, 3)


def stock_group_select(scores, bias, cum, embed, B, W, G, lam):
    """The group step's selection in stock ops: (total (B, W) raw, token (B, W), x_next (B W, H), src_row (B W))."""
    Wg = W // G
    x = (scores + bias).view(B, G, Wg, V)
    c = cum.view(B, G, Wg)
    counts = torch.zeros((B, V), device=scores.device)
    one = torch.ones((B, Wg), device=scores.device)
    totals, toks, pars = [], [], []
    for g in range(G):
        tot = (c[:, g, :, None] + torch.log_softmax(x[:, g], -1)).view(B, Wg * V)
        idx = (tot - lam * counts.repeat(1, Wg)).topk(Wg, -1).indices
        tok = idx % V
        totals.append(tot.gather(1, idx))
        toks.append(tok)
        pars.append(torch.div(idx, V, rounding_mode="floor") + g * Wg)
        counts = counts.scatter_add(1, tok, one)
    tok, par = torch.cat(toks, 1), torch.cat(pars, 1)
    src = (torch.arange(B, device=tok.device)[:, None] * W + par).reshape(-1)
    return torch.cat(totals, 1), tok, embed[tok.reshape(-1)], src


def stock_steps(m, h, states, cum, steps, B, W, G, lam):
    from vmlmf_amd.decoding import decode_layers
    for _ in range(steps):
        cum, tok, x, src = stock_group_select(torch.mm(h, m.fc.w.t()), m.fc.b, cum, m.embed.w, B, W, G, lam)
        states = [tuple(t.index_select(0, src) for t in st) for st in states]
        y, states = decode_layers(m, x.unsqueeze(0), states, "layers")
        h = y[-1]
    return h, states, cum


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="1x4x2,1x16x4,32x4x2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--against", default=None)
    ap.add_argument("--rounds", type=int, default=6)
    a = ap.parse_args()
    from vmlmf_amd import BeamGraph, GroupBeams, Model, _beam, _beamgroup, _lib
    from vmlmf_amd._lib import ptr
    from vmlmf_amd.decoding import _KeptImages
    from vmlmf_amd.functional import PackCache
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    m = Model(V, H, L, 0.0, 0.05, w_rank=32, u_ranks=[32], lstm_type="vmlmf").cuda().eval()
    out = open(a.out, "w") if a.out else None
    other = None
    if a.against:
        other = _lib.Library("libvmlmf_beam.so", _beam.SYMBOLS, "vmlmf_beam_abi_version", _beam.ABI_VERSION, "vmlmf_beam_last_error",
                             "fallback")
        other.path = os.path.abspath(a.against)
    for B, W, G in [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]:
        rec = {"B": B, "W": W, "G": G, "V": V, "H": H, "layers": L, "device": torch.cuda.get_device_name(0)}
        prompt = torch.randint(0, V, (4, B), device=dev)
        with torch.no_grad():
            h, st = m.features(prompt, m.state_init(B))
            h = h[-1].repeat_interleave(W, 0)
            st = [tuple(t.repeat_interleave(W, 0) for t in s) for s in st]
            # a search in full swing: every beam alive at a total of its own
            cum = -torch.rand(B, W, device=dev).cumsum(1)
            zero = torch.zeros((B, W), dtype=torch.int32, device=dev)
            scores = torch.mm(h, m.fc.w.t())
            bias, embed = m.fc.b.detach(), m.embed.w.detach()
            buffers = _beam.new_step_buffers(dev, B, W, V)
            if other is not None:
                outs = _beam.step_outputs(B, W, H, dev, embed)

                def plain(library):
                    return lambda: library.call(dev, "vmlmf_beam_step", B, W, H, V, ptr(scores), ptr(bias), ptr(cum), ptr(zero), ptr(zero), -1,
                                                ptr(embed), *(ptr(t) for t in outs), ptr(buffers[0]), ptr(buffers[1]), buffers[1].numel() * 8)

                rec["other_us"], rec["this_us"] = [], []
                for _ in range(a.rounds):
                    rec["other_us"].append(_replayed_us(plain(other), a.launches, a.reps)[0])
                    rec["this_us"].append(_replayed_us(plain(_beam.LIBRARY), a.launches, a.reps)[0])
            else:
                controls = GroupBeams(B, W, V, dev, G, LAMBDA)
                rec["group_us"], rec["group_spread"] = _replayed_us(
                    lambda: _beamgroup.group_select(scores, bias, cum, zero, zero, -1, embed, controls, buffers), a.launches, a.reps)
                rec["plain_us"], rec["plain_spread"] = _replayed_us(lambda: _beam.beam_select(scores, bias, cum, zero, zero, -1, embed, buffers),
                                                                    a.launches, a.reps)
                rec["stock_us"], rec["stock_spread"] = _replayed_us(lambda: stock_group_select(scores, bias, cum, embed, B, W, G, LAMBDA),
                                                                    a.launches, a.reps)
                # the whole step, graphed
                for name, c in (("step_ms", controls), ("plain_step_ms", None)):
                    g = BeamGraph(m, h, st, K, W, None, cum, zero, zero, controls=c)
                    ms, spread = wall_ms(g.replay, a.reps)
                    rec[name], rec[name.replace("_ms", "_spread")] = round(ms / K, 5), round(spread, 3)
                    del g
                caches = [PackCache() for mod in m.modules() if hasattr(mod, "kernel_params")]
                with _KeptImages(m, caches):
                    side = torch.cuda.Stream(dev)
                    side.wait_stream(torch.cuda.current_stream(dev))
                    with torch.cuda.stream(side):
                        stock_steps(m, h, st, cum, 2, B, W, G, LAMBDA)
                    torch.cuda.current_stream(dev).wait_stream(side)
                    sg = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(sg):
                        keep = stock_steps(m, h, st, cum, K, B, W, G, LAMBDA)
                    ms, spread = wall_ms(sg.replay, a.reps)
                    rec["stock_step_ms"], rec["stock_step_spread"] = round(ms / K, 5), round(spread, 3)
                    del sg, keep
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
