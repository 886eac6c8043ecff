"""Randomised parity sweep of the sequence entry point against the fp64 literal oracle (tests/hip_util.py's run_hip /
run_literal / compare_all at the tolerances of the test suite): shapes, ranks, variants, optional initial states and upstream
gradients drawn at random from a seed.  Prints every case that fails or that the library refuses, and a summary line.
    python tools/fuzz_parity.py [cases] [seed] [seq|stack|rb|big|wide] [hot]
hot (modes seq, rb, stack): the same draws with their values in the saturated-gate regime of tests/hot_cases.py (biases at sigma 5, or
40 for one case in four; docs/design/value_regimes.md); a case on which the fp32 literal oracle itself uses more than a third of the
tolerance is drawn again and counted, and more than one redraw per ten cases fails the run
wide: layers at wide ranks (padded w_rank > 32 or padded hidden rank summed over groups > 128) inside the envelope the library
documents for them (include/vmlmf_hip.h): the step-wise path, fp32, w_rank <= input_size, u_rank <= hidden_size / g, padded ranks
<= 1024; mostly ranks 33 - 320, sometimes up to the cap
seq, wide: a drawn case the library refuses is a failure (the draws stay inside the envelope)
big: batches up to 1100 rows, sequences up to 200 steps, H up to 700 (more rows than CUs, the stand-alone weight-gradient
kernels, the clustered layers)
stack: 2 - 4 like layers through vmlmf_stack (the wavefront launches; initial states of every layer at random) against the
chained literal layers; stacks the library does not cover (vmlmf_stack returns None) are counted, not run."""
import os, sys, time, traceback
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import vmlmf_oracle as O
from hip_util import run_hip, run_literal, compare_all, ORDER, ranks_of, assert_out, assert_grad
from slice_rule import assert_grad_slices, compare_slices, slice_cuts
from vmlmf_amd import functional as F

import fuzz_draw as D

N = int(sys.argv[1]) if len(sys.argv) > 1 else 200
SEED = int(sys.argv[2]) if len(sys.argv) > 2 else 1
MODE = sys.argv[3] if len(sys.argv) > 3 else "seq"
HOT = len(sys.argv) > 4 and sys.argv[4] == "hot"
if len(sys.argv) > 4 and not (HOT and MODE in D.HOT_MODES):
    sys.exit("usage: fuzz_parity.py [cases] [seed] [seq|stack|rb|big|wide] [hot]   (hot: seq, rb and stack only)")
rng = D.init(SEED, MODE)        # the draws (tools/fuzz_draw.py) and draw_wide below share this stream
VARIANTS, pick, draw, draw_stack = D.VARIANTS, D.pick, D.draw, D.draw_stack
if MODE == "rb":                      # the row-block MFMA kernels wherever an instantiation exists (vmlmf_tune "rb"), else the default choice
    from vmlmf_amd import _lib
    _lib.tune("rb", 1)


def pad8(r):
    return (r + 7) // 8 * 8


def in_wide_envelope(v, I, H, rw, ru):
    """make_geo's rule for a wide layer it runs (vmlmf_api.hip), restated: wide, on the step-wise path (padded u_rank > 32, more
    than 512 thread slots or I > H), no rank above the dimension it factors, both padded ranks <= 1024; plus the shape rules of
    every layer (LM: I == H; a cell with vm: I <= H; groups divide H)."""
    G = 2 if v in (O.V2, O.V4, O.V6) else 1
    rus = ru if G == 2 else [ru]
    if H % G or (v in (O.V3, O.V4) and I != H) or (v in (O.V1, O.V2) and I > H):
        return False
    KX, KH, NT = pad8(rw), sum(pad8(r) for r in rus), G * ((H // G + 63) // 64) * 64
    wide = KX > 32 or G * KH > 128
    stepwise = KH > 32 or NT > 512 or I > H
    return wide and stepwise and rw <= I and max(rus) <= H // G and KX <= 1024 and KH <= 1024


def wide_rank(cap):
    """mostly 33 - 320, sometimes up to cap"""
    return int(rng.integers(33, min(cap, 320) + 1)) if rng.random() < 0.85 or cap <= 320 else int(rng.integers(321, cap + 1))


def draw_wide():
    while True:
        v = VARIANTS[int(rng.integers(0, len(VARIANTS)))]
        G = 2 if v in (O.V2, O.V4, O.V6) else 1
        # one side wide (sometimes both), the other from the narrow range
        side = rng.random()
        rw = wide_rank(1024) if side < 0.7 else pick(1, 32, 0.3)
        ru = [wide_rank(1024 // G) if side >= 0.35 else pick(8, 40, 0.3) for _ in range(G)]
        need_h = max(max(ru) * G, 0 if v in (O.V5, O.V6) else rw)
        H = need_h + int(rng.integers(0, 160))
        H += H % G
        I = H if v in (O.V3, O.V4) else (rw + int(rng.integers(0, H - rw + 1)) if v in (O.V1, O.V2) else rw + int(rng.integers(0, 300)))
        if H > 1100 or I > 1100 or not in_wide_envelope(v, I, H, rw, ru if G == 2 else ru[0]):
            continue
        B, T = pick(1, 48, 0.5), pick(1, 24, 0.5)
        if rng.random() < 0.15 and H <= 256:          # many rows: the chunked column sums and K = T B of the weight gradients
            B, T = int(rng.integers(64, 257)), int(rng.integers(16, 65))
        if v == O.V4 and B == 1:
            B = 2
        # parameters at 1 / sqrt(fan-in) past a contraction of 100: at the default 0.1 a K ~ 1000 layer's pre-activations reach ~10,
        # and fp32 rounding alone (a host fp32 evaluation too) then misses the outputs' absolute tolerance
        scale = min(0.1, 1.0 / float(np.sqrt(max(I, H, rw, sum(ru)))))
        return dict(v=v, B=B, T=T, I=I, H=H, rw=rw, ru=ru if G == 2 else ru[0], states=bool(rng.random() < 0.5),
                    tm=bool(rng.random() < 0.4), dy=bool(rng.random() < 0.8), dh=bool(rng.random() < 0.5), dc=bool(rng.random() < 0.4),
                    seed=int(rng.integers(0, 2**31)), scale=scale)


def layout(c):
    """seq, rb, wide: every gradient also slice by slice (tools/slice_rule.py::compare_slices; docs/design/slice_tolerances.md), which is what
    checks the draws without dy - one in five - whose dx decays over the steps.  Not in the hot regime: with saturated gates a whole gate
    block of a gradient can be rounding residue (sigmoid' = 0 in fp32), and the fp32 literal oracle itself then misses the slice rule - on 7
    of the 40 draws of `40 21 seq hot` - so those draws keep the whole-tensor rule their redraw criterion is derived for."""
    if HOT or MODE not in ("seq", "rb", "wide"):
        return None
    return dict(variant=c["v"], H=c["H"], g=2 if c["v"] in (O.V2, O.V4, O.V6) else 1, time_major=c["tm"])


def run(c, vals=None):
    if vals is not None:              # hot: the values came with the draw (fuzz_draw.draw_hot)
        got = run_hip(c["v"], *vals, time_major=c["tm"])
        ref = run_literal(c["v"], *vals, time_major=c["tm"])
        compare_all(got, ref, "fuzz")
        return
    r = np.random.Generator(np.random.PCG64(c["seed"]))
    P = O.make_params(c["v"], c["I"], c["H"], c["rw"], c["ru"], seed=c["seed"] % 1000, scale=c.get("scale", 0.1))
    shp = (c["T"], c["B"], c["I"]) if c["tm"] else (c["B"], c["T"], c["I"])
    x = r.standard_normal(shp).astype(np.float32)
    h0 = c0 = None
    if c["states"]:
        h0 = (0.5 * r.standard_normal((c["B"], c["H"]))).astype(np.float32)
        c0 = (0.5 * r.standard_normal((c["B"], c["H"]))).astype(np.float32)
    oshp = shp[:2] + (c["H"],)
    dy = r.standard_normal(oshp).astype(np.float32) if c["dy"] else None
    dhT = r.standard_normal((c["B"], c["H"])).astype(np.float32) if c["dh"] else None
    dcT = r.standard_normal((c["B"], c["H"])).astype(np.float32) if c["dc"] else None
    if dy is None and dhT is None and dcT is None:
        dhT = r.standard_normal((c["B"], c["H"])).astype(np.float32)
    got = run_hip(c["v"], P, x, h0, c0, dy, dhT, dcT, time_major=c["tm"])
    ref = run_literal(c["v"], P, x, h0, c0, dy, dhT, dcT, time_major=c["tm"])
    compare_all(got, ref, "fuzz")
    if layout(c) is not None:         # what compare_all(..., slices=layout) adds, here straight from tools/slice_rule.py
        compare_slices(got, ref, "fuzz", layout(c))


class NotCovered(Exception):
    pass


def run_stack(c, vals=None):
    """L like layers: vmlmf_stack on the GPU, the literal layers chained on the CPU (float64)."""
    r = np.random.Generator(np.random.PCG64(c["seed"]))
    v, L, B, T, I, H = c["v"], c["L"], c["B"], c["T"], c["I"], c["H"]
    Hs = c.get("Hs") or [H] * L          # (round 6: the layers of a stack may differ in hidden size; no initial states then)
    if vals is not None:              # hot: the values came with the draw (fuzz_draw.draw_hot), every layer's in the regime
        Ps, x, h0s, c0s, dy, dhT_hot = vals[:6]
        st = None if h0s is None else [np.stack(h0s), np.stack(c0s)]
    else:
        Ps = [O.make_params(v, I if l == 0 else Hs[l - 1], Hs[l], c["rw"], c["ru"], seed=c["seed"] % 1000 + l) for l in range(L)]
        shp = (T, B, I) if c["tm"] else (B, T, I)
        x = r.standard_normal(shp).astype(np.float32)
        dy = r.standard_normal(shp[:2] + (Hs[-1],)).astype(np.float32)
        st = None
        if c["states"] and len(set(Hs)) == 1:
            st = [(0.5 * r.standard_normal((L, B, H))).astype(np.float32) for _ in range(2)]
    names = ORDER[v]
    rw, ru, g = ranks_of(v, Ps[0])
    params = [[torch.tensor(np.asarray(P[k]), device="cuda").requires_grad_(True) for k in names] for P in Ps]
    xt = torch.tensor(x, device="cuda").requires_grad_(True)
    h0 = c0 = None
    if st is not None:
        h0, c0 = (torch.tensor(a, device="cuda").requires_grad_(True) for a in st)
    out = F.vmlmf_stack(v, xt, params, rw, ru, g=g, time_major=c["tm"], h0=h0, c0=c0)
    if out is None:
        raise NotCovered()
    y, hTs, cTs = out[:3]
    dhT = dhT_hot if vals is not None else [r.standard_normal((B, Hs[l])).astype(np.float32) for l in range(L)]
    loss = (y * torch.tensor(dy, device="cuda")).sum()
    for l in range(L):
        loss = loss + (hTs[l] * torch.tensor(dhT[l], device="cuda")).sum()
    loss.backward()
    torch.cuda.synchronize()
    # oracle
    Pt = [O.to_torch(P, dtype=torch.float64, requires_grad=True) for P in Ps]
    xr = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    h0r = c0r = None
    if st is not None:
        h0r, c0r = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in st)
    cur, hr = xr, []
    for l in range(L):
        cur, hT, cT = O.literal_sequence(v, Pt[l], cur, None if h0r is None else h0r[l], None if c0r is None else c0r[l],
                                         time_major=c["tm"], v4_scratch_rows=B)
        hr.append(hT)
    lr = (cur * torch.tensor(dy, dtype=torch.float64)).sum()
    for l in range(L):
        lr = lr + (hr[l] * torch.tensor(dhT[l], dtype=torch.float64)).sum()
    lr.backward()
    assert_out(y.detach().cpu().numpy(), cur.detach().numpy(), "stack.y")
    for l in range(L):
        assert_out(hTs[l].detach().cpu().numpy(), hr[l].detach().numpy(), f"stack.hT[{l}]")
    assert_grad(xt.grad.cpu().numpy(), xr.grad.numpy(), "stack.dx")
    if vals is None:                  # slice by slice as well (not the hot draws: layout())
        assert_grad_slices(xt.grad.cpu().numpy(), xr.grad.numpy(), "stack.dx", [0, 1])          # per time step and per row
    if st is not None:
        assert_grad(h0.grad.cpu().numpy(), h0r.grad.numpy(), "stack.dh0")
        assert_grad(c0.grad.cpu().numpy(), c0r.grad.numpy(), "stack.dc0")
        if vals is None:
            assert_grad_slices(h0.grad.cpu().numpy(), h0r.grad.numpy(), "stack.dh0", [(0, 1)])     # (L, B, H): per layer and row
            assert_grad_slices(c0.grad.cpu().numpy(), c0r.grad.numpy(), "stack.dc0", [(0, 1)])
    for l in range(L):
        for k, p in zip(names, params[l]):
            assert_grad(p.grad.cpu().numpy(), Pt[l][k].grad.numpy(), f"stack.G[{l}].{k}")
            cuts = None if vals is not None else slice_cuts(k, tuple(p.shape), v, Hs[l], g, c["tm"])
            if cuts is not None:
                assert_grad_slices(p.grad.cpu().numpy(), Pt[l][k].grad.numpy(), f"stack.G[{l}].{k}", cuts)


ok = refused = failed = uncovered = redrawn = 0
t0 = time.time()
for n in range(N):
    vals = None
    if HOT:
        c, vals, again = D.draw_hot()
        redrawn += again
    else:
        c = draw_stack() if MODE == "stack" else (draw_wide() if MODE == "wide" else draw())
    try:
        if MODE == "stack":
            run_stack(c, vals)
        else:
            run(c, vals)
        ok += 1
    except NotCovered:
        uncovered += 1
    except AssertionError as e:
        failed += 1
        print("FAIL", c, str(e)[:600], flush=True)
    except RuntimeError as e:
        msg = str(e)
        if "error -3" in msg or "error -2" in msg or "unsupported" in msg.lower():
            refused += 1
            print("refused", c, msg[:160], flush=True)
            if MODE in ("seq", "wide"):   # the draw is inside the envelope: a refusal is a regression
                failed += 1
        else:
            failed += 1
            print("ERROR", c, msg[:400], flush=True)
            torch.cuda.synchronize()
    except Exception as e:      # noqa: BLE001
        failed += 1
        print("EXC", c, traceback.format_exc()[-600:], flush=True)
summary = (f"fuzz {MODE}{' hot' if HOT else ''} seed {SEED}: {N} cases, {ok} ok, {refused} refused by the library, {uncovered} not covered by "
           f"the wavefront launches, {failed} FAILED, {time.time() - t0:.0f} s")
if HOT:
    summary += f", {redrawn} redrawn (fp32 oracle)"
    if redrawn > D.REDRAW_CAP * N:
        print(f"more than {D.REDRAW_CAP:.0%} of the cases had to be drawn again: the regime is not one plain fp32 can be held to", flush=True)
        failed += 1
print(summary)
sys.exit(1 if failed else 0)
