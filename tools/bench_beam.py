"""Beam search of the PTB LM (Model.beam_search): V 10 000, H 650, two MyVMLSTM layers of rank 32, at (B, W) = (1, 4), (1, 16), (32, 4).
Per shape, same process, same device:
  select_gather_us   the two hand-written launches of a step - vmlmf_beam_step on the (B W, V) scores of the head's GEMM, then
                     vmlmf_beam_gather over the 2 L state tensors - n times in a graph, replayed
  stock_us           the stock-op sequence that does the same work on the same scores (bias add, log_softmax, add, topk, div, mod,
                     embedding gather, 2 L index_select; no eos handling, which would add ops), timed the same way
  step_ms / stock_step_ms   the whole decode step per token - head GEMM, selection, state reorder, the layers at T = 1 on kept
                     images - as a BeamGraph of 16 steps against the same loop with the stock-op selection, captured the same way;
                     eager_step_ms / stock_eager_step_ms the two loops eager
Best of --reps replays each, and the spread (max / min) over them.  One JSON object per line.
`python tools/bench_beam.py [--out FILE] [--shapes 1x4,1x16,32x4] [--reps 5]`."""
import argparse
import json
import os
import sys

import torch

from _timing import replayed_us, wall_ms

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

V, H, L = 10000, 650, 2


def _replayed_us(body, n, reps):
    """us per iteration of `body`, n of them captured into one graph; best of `reps` replays, and max / min."""
    us, spread = replayed_us(lambda j: body(), n, reps)
    return us, round(spread, 3)


def _wall_ms(fn, per, reps):
    ms, spread = wall_ms(fn, reps)
    return ms / per, round(spread, 3)


def stock_select(scores, bias, cum, embed, states, B, W):
    """The step's selection and state reorder in stock ops."""
    lsm = torch.log_softmax(scores + bias, -1)
    total, idx = (cum[:, :, None] + lsm.view(B, W, V)).view(B, W * V).topk(W, -1)
    par, tok = torch.div(idx, V, rounding_mode="floor"), idx % V
    x = embed[tok.reshape(-1)]
    src = (torch.arange(B, device=idx.device)[:, None] * W + par).reshape(-1)
    return total, tok, x, [t.index_select(0, src) for t in states]


def stock_steps(m, h, states, cum, steps, B, W):
    from vmlmf_amd.decoding import decode_layers
    for _ in range(steps):
        cum, tok, x, flat = stock_select(torch.mm(h, m.fc.w.t()), m.fc.b, cum, m.embed.w, [t for st in states for t in st], B, W)
        states = [(flat[2 * i], flat[2 * i + 1]) for i in range(L)]
        y, states = decode_layers(m, x.unsqueeze(0), states, "layers")
        h = y[-1]
    return h, states, cum


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="1x4,1x16,32x4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    a = ap.parse_args()
    from vmlmf_amd import BeamGraph, Model, _beam, beam_gather
    from vmlmf_amd.functional import PackCache
    from vmlmf_amd.decoding import _KeptImages, beam_steps
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    m = Model(V, H, L, 0.0, 0.05, w_rank=32, u_ranks=[32], lstm_type="vmlmf").cuda().eval()
    out = open(a.out, "w") if a.out else None
    K = 16
    for B, W in [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]:
        rec = {"B": B, "W": W, "V": V, "H": H, "layers": L, "device": torch.cuda.get_device_name(0)}
        prompt = torch.randint(0, V, (4, B), device=dev)
        with torch.no_grad():
            h, st = m.features(prompt, m.state_init(B))
            h = h[-1].repeat_interleave(W, 0)
            st = [tuple(t.repeat_interleave(W, 0) for t in s) for s in st]
            # a search in full swing: every beam alive at a total of its own
            cum = -torch.rand(B, W, device=dev).cumsum(1)
            zero = torch.zeros((B, W), dtype=torch.int32, device=dev)
            scores = torch.mm(h, m.fc.w.t())
            flat = [t for s in st for t in s]
            bias, embed = m.fc.b.detach(), m.embed.w.detach()
            buffers = _beam.new_step_buffers(dev, B, W, V)

            def ours():
                o = _beam.beam_select(scores, bias, cum, zero, zero, -1, embed, buffers)
                beam_gather(flat, o[6])

            rec["select_gather_us"], rec["select_gather_spread"] = _replayed_us(ours, a.launches, a.reps)
            rec["select_us"], rec["select_spread"] = _replayed_us(lambda: _beam.beam_select(scores, bias, cum, zero, zero, -1, embed, buffers),
                                                                  a.launches, a.reps)
            rec["stock_us"], rec["stock_spread"] = _replayed_us(lambda: stock_select(scores, bias, cum, embed, flat, B, W), a.launches, a.reps)
            # the whole step, graphed
            g = BeamGraph(m, h, st, K, W, None, cum, zero, zero)
            rec["step_ms"], rec["step_spread"] = _wall_ms(g.replay, K, a.reps)
            del g
            caches = [PackCache() for mod in m.modules() if hasattr(mod, "kernel_params")]
            with _KeptImages(m, caches):
                side = torch.cuda.Stream(dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    stock_steps(m, h, st, cum, 2, B, W)
                torch.cuda.current_stream(dev).wait_stream(side)
                sg = torch.cuda.CUDAGraph()
                with torch.cuda.graph(sg):
                    keep = stock_steps(m, h, st, cum, K, B, W)
                rec["stock_step_ms"], rec["stock_step_spread"] = _wall_ms(sg.replay, K, a.reps)
                del sg, keep
                zero2 = zero.clone()
                rec["eager_step_ms"], rec["eager_step_spread"] = _wall_ms(lambda: beam_steps(m, h, st, cum, zero, zero2, K, None), K, a.reps)
                rec["stock_eager_step_ms"], rec["stock_eager_step_spread"] = _wall_ms(lambda: stock_steps(m, h, st, cum, K, B, W), K, a.reps)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
