"""Beam search of the PTB LM under controls (Model.beam_search with min_length / banned_tokens / no_repeat_ngram_size /
banned_sequences): V 10 000, H 650, two MyVMLSTM layers of rank 32, at (B, W) = (1, 4), (1, 16), (32, 4).
Per shape, same process, same device, the same scores of the head's GEMM:
  plain_us                  vmlmf_beam_step, n times in a graph, replayed (tools/bench_beam.py's select_us)
  neutral_us                vmlmf_beamctl_step with neutral controls
  closed_us                 ... with 64 tokens closed for every beam and min_length on
  all_hist64_us / all_hist1024_us   ... with the closed words, min_length, per-beam ban words and the histories carried, the beams'
                            histories 64 / 1024 tokens long (capacity 64 / 1024 + 16)
  bans_hist64_us / bans_hist1024_us the vmlmf_history_bans launch on the B W rows that forms those ban words (n = 3, two sequences)
  step_ms / ngram_step_ms   the whole decode step per token - head GEMM, selection, state reorder, the layers at T = 1 on kept images -
                            as a BeamGraph of 16 steps without controls and with no_repeat_ngram_size = 3
Best of --reps replays each, and the spread (max / min) over them.  One JSON object per line.
`python tools/bench_beam_controls.py [--out FILE] [--shapes 1x4,1x16,32x4] [--reps 5]`."""
import argparse
import ctypes
import json
import os
import sys

import torch

from _timing import replayed_us, wall_ms

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

V, H, L = 10000, 650, 2
N_GRAM, K = 3, 16


def _replayed_us(body, n, reps):
    us, spread = replayed_us(lambda j: body(), n, reps)
    return round(us, 3), round(spread, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="1x4,1x16,32x4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    a = ap.parse_args()
    from vmlmf_amd import BeamControls, BeamGraph, Model, _beam, _beamctl
    from vmlmf_amd._lib import ptr
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
            # a search in full swing: every beam alive at a total of its own
            cum = -torch.rand(B, W, device=dev).cumsum(1)
            zero = torch.zeros((B, W), dtype=torch.int32, device=dev)
            scores = torch.mm(h, m.fc.w.t())
            bias, embed = m.fc.b.detach(), m.embed.w.detach()
            buffers = _beam.new_step_buffers(dev, B, W, V)
            eos = 3
            rec["plain_us"], rec["plain_spread"] = _replayed_us(lambda: _beam.beam_select(scores, bias, cum, zero, zero, eos, embed, buffers),
                                                                a.launches, a.reps)

            def controlled(c, hist=None, hist_len=None):
                return lambda: _beamctl.beamctl_select(scores, bias, cum, zero, zero, eos if c.eos >= 0 else -1, embed, c, hist, hist_len, buffers)

            neutral = BeamControls(B, W, V, dev)
            rec["neutral_us"], rec["neutral_spread"] = _replayed_us(controlled(neutral), a.launches, a.reps)
            banned = torch.randperm(V)[:65].tolist()
            banned = [t for t in banned if t != eos][:64]
            closed = BeamControls(B, W, V, dev, banned_tokens=banned, min_length=8, eos=eos)
            rec["closed_us"], rec["closed_spread"] = _replayed_us(controlled(closed), a.launches, a.reps)
            for T0 in (64, 1024):
                # histories over a small alphabet, so that the n-gram and sequence bans find matches
                alphabet = torch.randperm(V)[:48]
                long_prompt = alphabet[torch.randint(0, 48, (T0, B))].to(dev)
                seqs = [[int(alphabet[0]), int(alphabet[1])], [int(alphabet[2]), int(alphabet[3]), int(alphabet[4])]]
                c = BeamControls(B, W, V, dev, prompt=long_prompt, capacity=T0 + K, banned_tokens=banned, min_length=8, eos=eos,
                                 no_repeat_ngram_size=N_GRAM, banned_sequences=seqs)
                hist, hist_len = c.history()
                words = c.beam_bans(hist, hist_len)
                rec[f"banned_per_beam_hist{T0}"] = round(float(sum(bin(w & 0xffffffff).count("1") for w in words.reshape(-1).tolist())) / (B * W), 2)
                # the step alone (the ban words formed once), then the ban launch alone
                outs = _beamctl.beamctl_select(scores, bias, cum, zero, zero, eos, embed, c, hist, hist_len, buffers)
                step = _beamctl.Controls(c.min_length, c.capacity, c.closed.data_ptr(), words.data_ptr(), hist.data_ptr(), hist_len.data_ptr(),
                                         outs[7].data_ptr(), outs[8].data_ptr(), c.overflow.data_ptr())

                def all_controls():
                    _beamctl.LIBRARY.call(dev, "vmlmf_beamctl_step", B, W, H, V, ptr(scores), ptr(bias), ptr(cum), ptr(zero), ptr(zero), eos,
                                          ptr(embed), ctypes.byref(step), *(ptr(t) for t in outs[:7]), ptr(buffers[0]), ptr(buffers[1]),
                                          buffers[1].numel() * 8)

                rec[f"all_hist{T0}_us"], rec[f"all_hist{T0}_spread"] = _replayed_us(all_controls, a.launches, a.reps)
                rec[f"bans_hist{T0}_us"], rec[f"bans_hist{T0}_spread"] = _replayed_us(lambda: c.beam_bans(hist, hist_len), a.launches, a.reps)
            # the whole step, graphed: without controls, and with the n-gram ban (its two launches instead of the plain one)
            g = BeamGraph(m, h, st, K, W, eos, cum, zero, zero)
            ms, spread = wall_ms(g.replay, a.reps)
            rec["step_ms"], rec["step_spread"] = round(ms / K, 5), round(spread, 3)
            del g
            c = BeamControls(B, W, V, dev, prompt=prompt, capacity=4 + K * (a.reps + 4), eos=eos, no_repeat_ngram_size=N_GRAM)
            g = BeamGraph(m, h, st, K, W, eos, cum, zero, zero, controls=c)
            ms, spread = wall_ms(g.replay, a.reps)
            rec["ngram_step_ms"], rec["ngram_step_spread"] = round(ms / K, 5), round(spread, 3)
            rec["ngram_overflowed"] = int(c.overflow.sum())
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
