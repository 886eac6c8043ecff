"""Contrastive search of the PTB LM (Model.contrastive_search): V 10 000, H 650, two MyVMLSTM layers of rank 32, at (B, k, t) =
(1, 4, 128), (1, 8, 1024), (32, 4, 512), penalty_alpha 0.6 - t the length of every row's history.  Per shape, same process, same
device, the same inputs (the candidates of a real step, the history of a real prompt):
  choose_us     vmlmf_contrast_choose, n times in a graph, replayed - in front of every launch one small copy puts hist_len back to t
                (the launch appends a row and moves the length on), so every launch reads t rows
  stock_us      the same step composed from stock ops - normalise, bmm with hist[:, :t], amax, the value, argmax, the gathers, the
                appended row, src_row - behind the same small copy, timed the same way
                Both alternate, --rounds times each (every round a capture of its own); every round's figure is kept, the best named.
  read_tbps     B t H 4 bytes of history over the best choose_us, beside 6.29 TB/s, what a float4 copy out of HBM reaches on this GPU
                (the histories here, 0.3 to 43 MB, stay in the caches between replays: the figure says how far the launch is from
                being bound by that read, not a share of HBM bandwidth)
  step_ms / greedy_step_ms   the whole decode step per token as a ContrastGraph of 16 steps from that history, and generate's greedy
                step (DecodeGraph, temperature 0) from the same prompt, wall clock per replay / 16
  rows_choosing_differently / their_value_gap   rows in which the two forms choose different candidates, and how far apart in value
                (fp64) those candidates are: a tie at fp32 resolution, if anything
  roomy_us / early_us   the launch on a history of t rows, and of 16 rows, in a capacity of t + 1024 (the automatic number of workgroups
                comes from the capacity: what the parts beyond the history cost)
  parts_us      --sweep: the launch with 1, 2, ... 64 workgroups forced per row (the outputs are the same bits for each)
One JSON object per line.
`python tools/bench_contrast.py [--out FILE] [--shapes 1x4x128,1x8x1024,32x4x512] [--reps 5] [--rounds 4] [--sweep]`."""
import argparse
import json
import os
import sys

import torch

from _timing import replayed_us, wall_ms

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

V, H, L = 10000, 650, 2
K, ALPHA = 16, 0.6
HBM_COPY_TBPS = 6.29


def stock_choose(cand_h, cand_tok, cand_logp, hist, t, alpha, B, k):
    """The step in stock ops on the kernel's inputs: (token, logprob, chosen, sim, h_next, src_row); hist[:, t] receives the unit row."""
    u = cand_h / cand_h.norm(dim=-1, keepdim=True).clamp_min(1e-30)
    sim = torch.bmm(u.view(B, k, -1), hist[:, :t].transpose(1, 2)).amax(-1)
    chosen = ((1.0 - alpha) * cand_logp.exp() - alpha * sim).argmax(-1)
    rows = torch.arange(B, device=cand_h.device) * k + chosen
    hist[:, t] = u[rows]
    return (cand_tok.gather(1, chosen[:, None])[:, 0], cand_logp.gather(1, chosen[:, None])[:, 0], chosen, sim, cand_h[rows],
            rows.repeat_interleave(k).to(torch.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="1x4x128,1x8x1024,32x4x512")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    from vmlmf_amd import ContrastControls, ContrastGraph, DecodeGraph, Model, lm_contrast_step, lm_score
    from vmlmf_amd.decoding import decode_layers
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    m = Model(V, H, L, 0.0, 0.05, w_rank=32, u_ranks=[32], lstm_type="vmlmf").cuda().eval()
    out = open(a.out, "w") if a.out else None
    for B, k, t in [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]:
        rec = {"B": B, "k": k, "t": t, "V": V, "H": H, "layers": L, "alpha": ALPHA, "device": torch.cuda.get_device_name(0)}
        prompt = torch.randint(0, V, (t, B), device=dev)
        with torch.no_grad():
            hs, st = m.features(prompt, m.state_init(B))
            wide = [tuple(s.repeat_interleave(k, 0) for s in pair) for pair in st]
            # the candidates of the first step behind that prompt
            _, _, cand_tok, cand_logp = lm_score(hs[-1], m.fc.w, m.fc.b, None, k)
            y, _ = decode_layers(m, m.embed(cand_tok.reshape(-1)).unsqueeze(0), wide, "layers")
            cand_h = y[-1].contiguous()
            c = ContrastControls(B, H, dev, t + 1, k, ALPHA, None, V)
            c.append(hs)
            t0 = c.hist_len.clone()

            def fused(j):
                c.hist_len.copy_(t0)
                lm_contrast_step(cand_h, cand_tok, cand_logp, c)

            def stock(j):
                c.hist_len.copy_(t0)
                stock_choose(cand_h, cand_tok, cand_logp, c.hist, t, ALPHA, B, k)

            ref = stock_choose(cand_h, cand_tok, cand_logp, c.hist.clone(), t, ALPHA, B, k)
            got = lm_contrast_step(cand_h, cand_tok, cand_logp, c)
            # where the two choose differently, how far apart the two candidates' values are (fp64, from the stock similarities)
            values = (1.0 - ALPHA) * cand_logp.double().exp() - ALPHA * ref[3].double()
            apart = (values.gather(1, ref[2][:, None]) - values.gather(1, got[2].long()[:, None])).abs()[:, 0]
            rec["rows_choosing_differently"] = int((ref[2] != got[2].long()).sum())
            rec["their_value_gap"] = float(apart.max())
            rec["max_sim_diff"] = float((ref[3] - got[3]).abs().max())
            rec["choose_us_rounds"], rec["stock_us_rounds"] = [], []
            for _ in range(a.rounds):
                rec["choose_us_rounds"].append(round(replayed_us(fused, a.launches, a.reps)[0], 3))
                rec["stock_us_rounds"].append(round(replayed_us(stock, a.launches, a.reps)[0], 3))
            rec["choose_us"], rec["stock_us"] = min(rec["choose_us_rounds"]), min(rec["stock_us_rounds"])
            if a.sweep:     # the launch at forced numbers of workgroups per row (0 above: automatic)
                rec["parts_us"] = {}
                for p in (1, 2, 4, 8, 16, 32, 64):
                    def forced(j, p=p):
                        c.hist_len.copy_(t0)
                        lm_contrast_step(cand_h, cand_tok, cand_logp, c, parts=p)
                    rec["parts_us"][str(p)] = round(replayed_us(forced, a.launches, a.reps)[0], 3)
            # a history in a capacity far larger than itself, as in the early steps of a long decode: the automatic number of
            # workgroups comes from the capacity, so parts beyond the history only take the ticket.  t rows, and 16 rows, in t + 1024
            big = ContrastControls(B, H, dev, t + 1024, k, ALPHA, None, V)
            big.append(hs)
            for name, rows in (("roomy_us", t), ("early_us", 16)):
                tn = torch.full_like(t0, rows)

                def roomy(j, tn=tn):
                    big.hist_len.copy_(tn)
                    lm_contrast_step(cand_h, cand_tok, cand_logp, big)
                rec[name] = round(replayed_us(roomy, a.launches, a.reps)[0], 3)
            del big
            rec["history_bytes"] = B * t * H * 4
            rec["read_tbps"] = round(rec["history_bytes"] / (rec["choose_us"] * 1e-6) / 1e12, 4)
            rec["hbm_copy_tbps"] = HBM_COPY_TBPS
            # the whole step, graphed: K steps a replay, the history growing by K rows a replay
            room = K * (a.reps + 3)
            cg = ContrastControls(B, H, dev, t + room, k, ALPHA, None, V)
            cg.append(hs)
            g = ContrastGraph(m, hs[-1], wide, K, cg)
            ms, spread = wall_ms(g.replay, a.reps)
            rec["step_ms"], rec["step_spread"] = round(ms / K, 5), round(spread, 3)
            del g
            d = DecodeGraph(m, hs[-1], st, K, 0.0)
            ms, spread = wall_ms(d.replay, a.reps)
            rec["greedy_step_ms"], rec["greedy_step_spread"] = round(ms / K, 5), round(spread, 3)
            del d
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
