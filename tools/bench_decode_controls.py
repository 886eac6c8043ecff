"""What the stopping and token controls of Model.generate cost (eos, min_length, repetition_penalty, logit_bias / bans: one launch of
libvmlmf_decode.so behind the head's GEMM, include/vmlmf_decode.h), at the PTB size: V 10 000, H 650, B in {1, 32}.
  choice_*   the choice launch ALONE on a fixed (B, V) score matrix, 50 launches replayed from a graph, us per launch:
               unfiltered            vmlmf_lm_choose                                 (the parent's kernel)
               filtered              vmlmf_lm_choose_filtered, top_k 40, top_p 0.9   (the parent's kernel)
               controlled            vmlmf_decode_choose, the same filters, every control on: theta 1.2, a logit_bias with 5 % bans,
                                     30 % of each row seen, eos held back by a min_length no row reaches (rows stay live: a finished
                                     row returns at once and would flatter the figure)
               controlled_unfiltered vmlmf_decode_choose without filters, the same controls
               parent_*              the first two from another build of libvmlmf_hip.so (--parent-lib FILE: the parent commit's,
                                     opened beside this tree's in the same process, so both are measured in one session)
  graph_*    whole decode steps: a DecodeGraph of 16 steps of the plain32 model, replayed, ms per token, for no filter, the filters,
             and the filters with every control on
The claim this checks (docs/design/lm_decode_controls.md): the controls add loads to the selection's first pass, not passes - so
choice_controlled - choice_filtered stays below choice_unfiltered, one whole pass over the row plus a launch.
Best of --reps replays, and the spread (max / min).  One JSON object per line.
`python tools/bench_decode_controls.py [--out FILE] [--batches 1,32] [--reps 5] [--parent-lib FILE] [--skip-controls]`
(--skip-controls: only the parent's paths - for a run under VMLMF_LIB=<another build>, which has no libvmlmf_decode.so beside it)."""
import argparse
import ctypes
import json
import os
import sys

import torch

from _timing import replayed_us, wall_ms

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

V, H, TOP_K, TOP_P, N = 10000, 650, 40, 0.9, 50


def all_controls(B, dev, prompt=None):
    """Every control on, and rows that never finish."""
    from vmlmf_amd import DecodeControls
    g = torch.Generator().manual_seed(4242)
    lb = torch.randn(V, generator=g)
    lb[torch.rand(V, generator=g) < 0.05] = float("-inf")
    lb[3] = 0.0
    c = DecodeControls(B, V, dev, eos=3, min_length=1 << 30, repetition_penalty=1.2, logit_bias=lb, prompt=prompt)
    c.seen.copy_((torch.rand((B, V), generator=g) < 0.3).to(torch.uint8))
    return c


def open_parent(path):
    """Another build of libvmlmf_hip.so beside this tree's: the two choice entry points, bound as _lib binds them."""
    from vmlmf_amd import _lib
    handle = ctypes.CDLL(os.path.abspath(path))
    for name in ("vmlmf_lm_choose", "vmlmf_lm_choose_filtered", "vmlmf_last_error"):
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = _lib.SYMBOLS[name]
    return handle


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--skip-controls", action="store_true")
    a = ap.parse_args()
    from vmlmf_amd import DecodeGraph, Model, _lib, dropout_advance
    _ptr = _lib.ptr
    dev = torch.device("cuda", torch.cuda.current_device())
    out = open(a.out, "a") if a.out else None
    libs = [("", _lib.lib())] + ([("parent_", open_parent(a.parent_lib))] if a.parent_lib else [])
    torch.manual_seed(0)
    m = Model(V, H, 2, 0.0, 0.05, w_rank=32, u_ranks=[32], lstm_type="vmlmf").cuda().eval()
    for B in [int(b) for b in a.batches.split(",")]:
        rec = {"B": B, "V": V, "H": H, "top_k": TOP_K, "top_p": TOP_P, "launches": N, "lib": os.path.basename(os.path.dirname(_lib.LIB_PATH)),
               "device": torch.cuda.get_device_name(0)}
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

            def filtered(j, lib=lib):
                _lib.check(lib.vmlmf_lm_choose_filtered(B, H, V, _ptr(scores), _ptr(bias), _ptr(embed), 1.0, TOP_K, TOP_P, _ptr(snap), j, _ptr(tok),
                                                        _ptr(lp), _ptr(xn), _ptr(kept), stream()))
            for name, fn in (("unfiltered", plain), ("filtered", filtered)):
                us, spread = replayed_us(fn, N, a.reps)
                rec[f"choice_{prefix}{name}_us"], rec[f"choice_{prefix}{name}_spread"] = round(us, 3), round(spread, 3)
        if not a.skip_controls:
            from vmlmf_amd import _decode
            for name, k, p in (("controlled", TOP_K, TOP_P), ("controlled_unfiltered", 0, 1.0)):
                ctl = all_controls(B, dev)
                us, spread = replayed_us(lambda j: _decode.decode_choose(scores, bias, embed, 1.0, k, p, snap, j, ctl, tok, lp, xn, kept), N, a.reps)
                rec[f"choice_{name}_us"], rec[f"choice_{name}_spread"] = round(us, 3), round(spread, 3)
                assert not ctl.finished.any()
            rec["controlled_minus_filtered_us"] = round(rec["choice_controlled_us"] - rec["choice_filtered_us"], 3)
        K = 16
        cases = [("plain", dict(), False), ("filtered", dict(top_k=TOP_K, top_p=TOP_P), False)]
        if not a.skip_controls:
            cases.append(("controlled", dict(top_k=TOP_K, top_p=TOP_P), True))
        for name, kw, controlled in cases:
            g = DecodeGraph(m, hv, st, K, temperature=1.0, controls=all_controls(B, dev, prompt) if controlled else None, **kw)
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
