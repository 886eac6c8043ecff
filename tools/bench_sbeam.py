"""Stochastic beam search of the PTB LM (Model.stochastic_beam_search): V 10 000, H 650, two MyVMLSTM layers of rank 32, at (B, W) =
(1, 4), (1, 16), (32, 4).  Per shape, same process, same device, the same scores of the head's GEMM, a search in full swing (every
beam alive at a total of its own, its perturbed value that total plus a Gumbel draw):
  sbeam_us                 vmlmf_sbeam_step, n times in a graph, replayed
  plain_us                 vmlmf_beam_step at the same (B, W), timed the same way (tools/bench_beam.py's select_us)
  stock_us                 the same step in stock ops - a (B W, V) noise tensor, log_softmax, the row maximum, the conditional
                           transform, topk over a row's W V candidates, div / mod, the gathers (no eos handling, which would add ops)
                           The three alternate, --rounds times each (every round a capture of its own); every round's figure is kept,
                           the best named.
  step_ms / beam_step_ms   the whole decode step per token - head GEMM, selection, state reorder, the layers at T = 1 on kept images -
                           as a StochasticBeamGraph of 16 steps and as beam_search's BeamGraph of 16 steps from the same prompt, wall
                           clock per replay / 16
One JSON object per line.
`python tools/bench_sbeam.py [--out FILE] [--shapes 1x4,1x16,32x4] [--reps 5] [--rounds 4]`."""
import argparse
import json
import os
import sys

import torch

from _timing import replayed_us, wall_ms

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

V, H, L = 10000, 650, 2
K = 16


def stock_sbeam_select(scores, bias, cum, perturbed, embed, B, W):
    """The step's selection in stock ops: (total, perturbed (B, W), token (B, W), x_next (B W, H), src_row (B W))."""
    phi = cum.view(B * W, 1) + torch.log_softmax(scores + bias, -1)
    gt = phi - torch.log(-torch.log(torch.rand_like(phi).clamp_(1e-7, 1 - 1e-7)))
    Z = gt.amax(-1, keepdim=True)
    T = perturbed.view(B * W, 1)
    u = (T - gt) + torch.log1p(-torch.exp(gt - Z))
    G = torch.where(gt == Z, T, T - torch.relu(u) - torch.log1p(torch.exp(-u.abs())))
    val, idx = G.view(B, W * V).topk(W, -1)
    tok, par = idx % V, torch.div(idx, V, rounding_mode="floor")
    src = (torch.arange(B, device=tok.device)[:, None] * W + par).reshape(-1)
    return phi.view(B, W * V).gather(1, idx), val, tok, embed[tok.reshape(-1)], src


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="1x4,1x16,32x4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--launches", type=int, default=50)
    a = ap.parse_args()
    from vmlmf_amd import BeamGraph, Model, StochasticBeamGraph, StochasticBeams, _beam, _sbeam, dropout_advance
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    m = Model(V, H, L, 0.0, 0.05, w_rank=32, u_ranks=[32], lstm_type="vmlmf").cuda().eval()
    out = open(a.out, "w") if a.out else None
    for B, W in [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]:
        rec = {"B": B, "W": W, "V": V, "H": H, "layers": L, "device": torch.cuda.get_device_name(0)}
        prompt = torch.randint(0, V, (4, B), device=dev)
        with torch.no_grad():
            h, st = m.features(prompt, m.state_init(B))
            h = h[-1].repeat_interleave(W, 0)
            st = [tuple(t.repeat_interleave(W, 0) for t in s) for s in st]
            cum = -torch.rand(B, W, device=dev).cumsum(1)
            perturbed = cum - torch.log(-torch.log(torch.rand(B, W, device=dev).clamp_(1e-6, 1 - 1e-6)))
            zero, draw = torch.zeros((B, W), dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
            scores = torch.mm(h, m.fc.w.t())
            bias, embed = m.fc.b.detach(), m.embed.w.detach()
            snap = dropout_advance(m.sampler_state(1))
            own, shared = StochasticBeams(B, W, V, dev).buffers(), _beam.new_step_buffers(dev, B, W, V)
            bodies = {"sbeam_us": lambda j: _sbeam.sbeam_select(scores, bias, cum, zero, zero, perturbed, draw, snap, -1, embed, own),
                      "plain_us": lambda j: _beam.beam_select(scores, bias, cum, zero, zero, -1, embed, shared),
                      "stock_us": lambda j: stock_sbeam_select(scores, bias, cum, perturbed, embed, B, W)}
            for name in bodies:
                rec[name + "_rounds"] = []
            for _ in range(a.rounds):
                for name, body in bodies.items():
                    rec[name + "_rounds"].append(round(replayed_us(body, a.launches, a.reps)[0], 3))
            for name in bodies:
                rec[name] = min(rec[name + "_rounds"])
            # the whole step, graphed
            g = StochasticBeamGraph(m, h, st, K, W, snap)
            ms, spread = wall_ms(g.replay, a.reps)
            rec["step_ms"], rec["step_spread"] = round(ms / K, 5), round(spread, 3)
            del g
            g = BeamGraph(m, h, st, K, W, None)
            ms, spread = wall_ms(g.replay, a.reps)
            rec["beam_step_ms"], rec["beam_step_spread"] = round(ms / K, 5), round(spread, 3)
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
