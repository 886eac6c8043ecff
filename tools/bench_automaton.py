"""Decoding of the PTB LM under a token automaton (Model.generate / Model.beam_search with automaton=): V 10 000, H 650, two MyVMLSTM
layers of rank 32.  Same process, same device, the same scores of the head's GEMM; every pair is timed ALTERNATING (a, b, a, b ...),
best of --reps replays of a graph of --launches launches each, and the spread (max / min) over all of a side's replays.
  kind "choice", B in --rows, mode greedy / k40p0.9:
    automaton_us            vmlmf_automaton_choose with a 64-state table (every state closes the same half of the vocabulary, so the
                            yardstick below stays equivalent while the states move)
    decode_us               vmlmf_decode_choose under a logit_bias that closes the same tokens
  kind "beam", (B, W) in --shapes:
    automaton_us            vmlmf_automaton_beam_step (the same table, the beams in different states)
    beamctl_us              vmlmf_beamctl_step with the equivalent per-beam `bans` words
    plain_us                vmlmf_beam_step
    with --parent DIR (a directory holding another build's libvmlmf_beam.so and libvmlmf_beamctl.so, e.g. the parent commit's):
    parent_plain_us / parent_beamctl_us   the same two launches of that build on the same buffers, alternating with this tree's
  kind "step": the whole graphed step per token with and without automaton= (DecodeGraph at B in --rows, greedy; BeamGraph at --shapes)
One JSON object per line.  `python tools/bench_automaton.py [--out FILE] [--rows 1,4,32] [--shapes 1x4,1x16,32x4] [--reps 5] [--parent DIR]`."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

from _timing import replayed_us, wall_ms

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

V, H, L, S, K = 10000, 650, 2, 64, 16
ROUNDS = 2      # alternations of a pair


def alternating(bodies, n, reps):
    """{name: (best us, spread)} of the named launches, timed in turn, ROUNDS times over."""
    ts = {name: [] for name in bodies}
    for _ in range(ROUNDS):
        for name, body in bodies.items():
            us, spread = replayed_us(lambda j: body(), n, reps)
            ts[name] += [us, us * spread]
    return {name: (round(min(t), 3), round(max(t) / min(t), 3)) for name, t in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="1,4,32")
    ap.add_argument("--shapes", default="1x4,1x16,32x4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--parent", default=None)
    a = ap.parse_args()
    from vmlmf_amd import (AutomatonBeamControls, AutomatonControls, BeamGraph, DecodeControls, DecodeGraph, Model, TokenAutomaton, _automaton,
                           _beam, _beamctl, _decode, _lib, dropout_advance, dropout_state)
    from vmlmf_amd._lib import ptr
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    m = Model(V, H, L, 0.0, 0.05, w_rank=32, u_ranks=[32], lstm_type="vmlmf").cuda().eval()
    bias, embed = m.fc.b.detach(), m.embed.w.detach()
    eos = 3
    # 64 states in a ring; every state closes the same seeded half of the vocabulary (eos stays open)
    rng = np.random.Generator(np.random.PCG64(1))
    closed = rng.random(V) < 0.5
    closed[eos] = False
    nxt = np.tile(((np.arange(S) + 1) % S).astype(np.int32)[:, None], (1, V))
    nxt[:, closed] = -1
    table = TokenAutomaton(torch.from_numpy(nxt)).to(dev)
    lb = torch.zeros(V)
    lb[torch.from_numpy(closed)] = float("-inf")
    out = open(a.out, "w") if a.out else None

    def emit(rec):
        rec.update(V=V, H=H, S=S, device=torch.cuda.get_device_name(0))
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    snap = dropout_advance(dropout_state(dev, 7))
    for B in [int(v) for v in a.rows.split(",")]:
        prompt = torch.randint(0, V, (4, B), device=dev)
        with torch.no_grad():
            h, st = m.features(prompt, m.state_init(B))
            scores = torch.mm(h[-1], m.fc.w.t())
            tokens, logp = torch.empty(B, device=dev, dtype=torch.int64), torch.empty(B, device=dev)
            xn, kept = torch.empty((B, H), device=dev), torch.empty(B, device=dev, dtype=torch.int32)
            start = (torch.arange(B) * 7 % S).to(torch.int32)
            for mode, (tau, k, p) in (("greedy", (0.0, 0, 1.0)), ("k40p0.9", (1.0, 40, 0.9))):
                ca = AutomatonControls(B, V, dev, table, start, prompt=prompt)
                cd = DecodeControls(B, V, dev, logit_bias=lb, prompt=prompt)
                inv = 0.0 if tau == 0 else 1.0 / tau
                choose = lambda c: lambda: _decode.decode_choose(scores, bias, embed, inv, k, p, None if inv == 0 else snap, 0, c, tokens, logp,
                                                                 xn, kept, kind=type(c))
                t = alternating({"automaton": choose(ca), "decode": choose(cd)}, a.launches, a.reps)
                emit({"kind": "choice", "B": B, "mode": mode, "automaton_us": t["automaton"][0], "automaton_spread": t["automaton"][1],
                      "decode_us": t["decode"][0], "decode_spread": t["decode"][1]})
            # the whole graphed step per token, greedy, with and without the automaton
            rec = {"kind": "step", "form": "generate", "B": B}
            for name, controls in (("plain", None), ("automaton", AutomatonControls(B, V, dev, table, start, prompt=prompt))):
                g = DecodeGraph(m, h[-1], st, K, temperature=0.0, controls=controls)
                ms, spread = wall_ms(g.replay, a.reps)
                rec[f"{name}_step_ms"], rec[f"{name}_step_spread"] = round(ms / K, 5), round(spread, 3)
                del g
            emit(rec)

    parent = None
    if a.parent:
        parent = {name: _lib.load(os.path.join(a.parent, mod.LIBRARY.path.rsplit("/", 1)[1]), mod.SYMBOLS, mod.LIBRARY.abi_symbol, mod.ABI_VERSION,
                                  "fallback") for name, mod in (("beam", _beam), ("beamctl", _beamctl))}
    for B, W in [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]:
        prompt = torch.randint(0, V, (4, B), device=dev)
        with torch.no_grad():
            h, st = m.features(prompt, m.state_init(B))
            h = h[-1].repeat_interleave(W, 0)
            st = [tuple(t.repeat_interleave(W, 0) for t in s) for s in st]
            cum = -torch.rand(B, W, device=dev).cumsum(1)          # a search in full swing: every beam alive at a total of its own
            zero = torch.zeros((B, W), dtype=torch.int32, device=dev)
            scores = torch.mm(h, m.fc.w.t())
            buffers = _beam.new_step_buffers(dev, B, W, V)
            ca = AutomatonBeamControls(B, W, V, dev, table, eos=eos)
            state = (torch.arange(B * W, device=dev) * 7 % S).to(torch.int32)
            words = torch.from_numpy(np.packbits(np.concatenate([closed, np.zeros((-V) % 32, dtype=bool)]), bitorder="little").view(np.int32))
            words = words.to(dev).repeat(B * W, 1).contiguous()
            outs = _beam.beam_select(scores, bias, cum, zero, zero, eos, embed, buffers)
            step = _beamctl.Controls(0, 1, None, words.data_ptr(), None, None, None, None, None)

            def launch(handle, name, *controls):
                def body():
                    with _lib.on_device(dev):
                        rc = getattr(handle, name)(B, W, H, V, ptr(scores), ptr(bias), ptr(cum), ptr(zero), ptr(zero), eos, ptr(embed), *controls,
                                                   *(ptr(t) for t in outs), ptr(buffers[0]), ptr(buffers[1]), buffers[1].numel() * 8,
                                                   _lib.raw_stream(dev))
                    assert rc == 0, rc
                return body

            bodies = {"automaton": lambda: _automaton.automaton_select(scores, bias, cum, zero, zero, eos, embed, ca, state, buffers),
                      "beamctl": launch(_beamctl.lib(), "vmlmf_beamctl_step", ctypes.byref(step)),
                      "plain": launch(_beam.lib(), "vmlmf_beam_step")}
            if parent:
                bodies["parent_beamctl"] = launch(parent["beamctl"], "vmlmf_beamctl_step", ctypes.byref(step))
                bodies["parent_plain"] = launch(parent["beam"], "vmlmf_beam_step")
            t = alternating(bodies, a.launches, a.reps)
            rec = {"kind": "beam", "B": B, "W": W}
            for name, (us, spread) in t.items():
                rec[f"{name}_us"], rec[f"{name}_spread"] = us, spread
            emit(rec)
            rec = {"kind": "step", "form": "beam_search", "B": B, "W": W}
            for name, controls in (("plain", None), ("automaton", ca)):
                g = BeamGraph(m, h, st, K, W, eos, cum, zero, zero, controls=controls, **({} if controls is None else {"beam_state": state}))
                ms, spread = wall_ms(g.replay, a.reps)
                rec[f"{name}_step_ms"], rec[f"{name}_step_spread"] = round(ms / K, 5), round(spread, 3)
                del g
            emit(rec)
    if out:
        out.close()


if __name__ == "__main__":
    main()
