"""The saturated-gate value regime of the recurrent kernels (docs/design/value_regimes.md): inputs whose biases, x and initial cell
state drive the gates to the rails while the factors stay at the suite's scale (contractive dynamics, so plain fp32 still meets the
suite's tolerances), the statistics that prove a case is in that regime, and the case tables that tests/test_hot_regime_cpu.py
(conditions, CPU) and tests/test_gpu_hot_regime.py (the kernels, GPU) both read.  Helpers only: no test lives here."""
import numpy as np
import torch

import vmlmf_oracle as O
from hip_util import ATOL, GREL, ORDER, RTOL, run_literal

V1, V2, V3, V4, V5, V6 = O.V1, O.V2, O.V3, O.V4, O.V5, O.V6
GROUPED = (V2, V4, V6)
TIERS = {"hot": 5.0, "rail": 40.0}        # sigma of every bias
EXP_LIMIT = 88.7                          # |x| beyond which exp(x) leaves fp32: the fast gates then rest on rcp(inf) = 0
FP32_SHARE = 1.0 / 3.0                    # of the tolerance: what the fp32 literal oracle may use against the fp64 one


def is_bias(name):
    return name.startswith("b_") or name.startswith("bias_")


def param_scale(H):
    return 0.05 if H >= 650 else 0.1


def x_sigma(I):
    return 3.0 if I <= 64 else 0.9


# rows on whose first seed the fp32 literal oracle itself is beyond a third of the tolerance (tests/test_hot_regime_cpu.py) take a later
# one: base seed -> steps.  Config A's full length (plain fp32 between 0.15 and 0.9 of y's tolerance over ten seeds) and the first
# wavefront row's rail tier (its bottom layer's dia_x gradient cancels to 8e-4: eighteen tolerances in fp32)
RESEED = {100003 * 1 + 1009 * 64 + 101 * 128 + 13 * 180 + 7 * 9 + 16: 9, 100003 * 1 + 1009 * 19 + 101 * 11 + 13 * 180 + 7 * 9 + 2: 2}


def case_seed(variant, B, T, I, H, rw):
    base = 100003 * variant + 1009 * B + 101 * T + 13 * H + 7 * I + rw
    return base + 7777 * RESEED.get(base, 0)


def hot_params(variant, I, H, rw, ru, tier, rng, seed):
    """Factors and dia_* as the suite draws them (O.make_params at the suite's scale), every bias redrawn as sigma_b N(0, 1) from rng."""
    P = O.make_params(variant, I, H, rw, list(ru) if variant in GROUPED else ru[0], seed=seed, scale=param_scale(H))
    for k in ORDER[variant]:
        if is_bias(k):
            P[k] = (TIERS[tier] * rng.standard_normal(P[k].shape)).astype(np.float32)
    return P


def _states(rng, shape):
    h0 = np.clip(0.6 * rng.standard_normal(shape), -1.0, 1.0).astype(np.float32)
    c0 = (4.0 * rng.standard_normal(shape)).astype(np.float32)
    return h0, c0


def hot_inputs(variant, B, T, I, H, rw, ru, tier="hot", time_major=False, with_state=True, seed=0):
    """P, x, h0, c0, dy, dhT, dcT (numpy) of one layer in the regime.  One PCG64 stream per case, drawn in this order: biases (in
    ORDER[variant]), x, h0, c0, dy, dhT, dcT; the states are drawn even when with_state is False, so the rest does not move."""
    rng = np.random.Generator(np.random.PCG64(seed))
    P = hot_params(variant, I, H, rw, ru, tier, rng, seed + 1)
    shp = (T, B, I) if time_major else (B, T, I)
    x = (x_sigma(I) * rng.standard_normal(shp)).astype(np.float32)
    h0, c0 = _states(rng, (B, H))
    dy = rng.standard_normal(shp[:2] + (H,)).astype(np.float32)
    dhT = rng.standard_normal((B, H)).astype(np.float32)
    dcT = rng.standard_normal((B, H)).astype(np.float32)
    if not with_state:
        h0 = c0 = None
    return P, x, h0, c0, dy, dhT, dcT


def hot_stack_inputs(variant, B, T, I, Hs, rw, ru, tier="hot", time_major=False, with_state=True, seed=0):
    """A stack's inputs, the hot draw per layer: Ps (list), x, h0, c0 (lists of (B, H_l), or None), dy, dhT, dcT (lists)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    Ps = [hot_params(variant, I if l == 0 else Hs[l - 1], H, rw, ru, tier, rng, seed + 1 + l) for l, H in enumerate(Hs)]
    shp = (T, B, I) if time_major else (B, T, I)
    x = (x_sigma(I) * rng.standard_normal(shp)).astype(np.float32)
    st = [_states(rng, (B, H)) for H in Hs]
    dy = rng.standard_normal(shp[:2] + (Hs[-1],)).astype(np.float32)
    dhT = [rng.standard_normal((B, H)).astype(np.float32) for H in Hs]
    dcT = [rng.standard_normal((B, H)).astype(np.float32) for H in Hs]
    h0 = [s[0] for s in st] if with_state else None
    c0 = [s[1] for s in st] if with_state else None
    return Ps, x, h0, c0, dy, dhT, dcT


def run_stack_literal(variant, Ps, x, h0, c0, dy, dhT, dcT, time_major=False, dtype=torch.float64):
    """The literal layers chained (vmlmf.py:300-314 / vmlmf_lm.py:437-439), autograd: a stack's result as y, hT / cT (lists), dx,
    dh0 / dc0 (lists, with states) and G (list of dicts)."""
    L, B = len(Ps), x.shape[1 if time_major else 0]
    Pt = [O.to_torch(P, dtype=dtype, requires_grad=True) for P in Ps]
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    h0t = None if h0 is None else [torch.tensor(a, dtype=dtype, requires_grad=True) for a in h0]
    c0t = None if c0 is None else [torch.tensor(a, dtype=dtype, requires_grad=True) for a in c0]
    cur, loss, hs, cs = xt, 0.0, [], []
    for l in range(L):
        cur, hT, cT = O.literal_sequence(variant, Pt[l], cur, None if h0t is None else h0t[l], None if c0t is None else c0t[l],
                                         time_major=time_major, v4_scratch_rows=B)
        hs.append(hT), cs.append(cT)
        if dhT is not None:
            loss = loss + (hT * torch.tensor(dhT[l], dtype=dtype)).sum()
        if dcT is not None:
            loss = loss + (cT * torch.tensor(dcT[l], dtype=dtype)).sum()
    if dy is not None:
        loss = loss + (cur * torch.tensor(dy, dtype=dtype)).sum()
    loss.backward()
    out = {"y": cur.detach().numpy(), "hT": [h.detach().numpy() for h in hs], "cT": [c.detach().numpy() for c in cs],
           "dx": xt.grad.numpy(), "G": [{k: Pt[l][k].grad.numpy() for k in ORDER[variant]} for l in range(L)]}
    if h0t is not None:
        out["dh0"] = [a.grad.numpy() for a in h0t]
        out["dc0"] = [a.grad.numpy() for a in c0t]
    return out


# ---- the statistics of a case ------------------------------------------------------------------------------------------------------
class _Tail:
    """O._lstm_tail wrapped: every call's four pre-activations and new cell state are seen before the cell's own arithmetic."""

    def __init__(self):
        self.n = self.n4 = self.n16 = self.n88 = 0
        self.max_pre = self.max_c = 0.0
        self.po = []

    def see(self, pi, pf, po, pn, c_next):
        for p in (pi, pf, po, pn):
            a = p.detach().abs()
            self.n += a.numel()
            self.n4 += int((a > 4).sum())
            self.n16 += int((a > 16).sum())
            self.n88 += int((a > EXP_LIMIT).sum())
            self.max_pre = max(self.max_pre, float(a.max()))
        self.max_c = max(self.max_c, float(c_next.detach().abs().max()))
        self.po.append(po.detach().numpy().copy())

    def stats(self, steps_of_last_layer):
        og_low = np.all(np.stack(self.po[-steps_of_last_layer:]) < -EXP_LIMIT, axis=0)
        return {"gt4": self.n4 / self.n, "gt16": self.n16 / self.n, "gt88": self.n88 / self.n, "max_pre": self.max_pre,
                "max_c": self.max_c, "og_low": og_low}


def _watched(fn, steps):
    rec, plain = _Tail(), O._lstm_tail

    def tail(pi, pf, po, pn, c):
        h, c_next = plain(pi, pf, po, pn, c)
        rec.see(pi, pf, po, pn, c_next)
        return h, c_next
    O._lstm_tail = tail
    try:
        with torch.no_grad():
            fn()
    finally:
        O._lstm_tail = plain
    return rec.stats(steps)


def gate_stats(variant, P, x, h0, c0, time_major=False):
    """The fp64 literal oracle's forward with O._lstm_tail wrapped.  Returns the shares of |pre-activation| above 4, 16 and 88.7
    ("gt4", "gt16", "gt88"), "max_pre", "max_c" (over the new cell states) and "og_low": (B, H) bool, the (row, unit) pairs whose output gate's
    pre-activation lies below -88.7 at every step."""
    f64 = torch.float64
    T, B = (x.shape[0], x.shape[1]) if time_major else (x.shape[1], x.shape[0])
    Pt = O.to_torch(P, dtype=f64)
    st = [None if a is None else torch.tensor(a, dtype=f64) for a in (h0, c0)]
    return _watched(lambda: O.literal_sequence(variant, Pt, torch.tensor(x, dtype=f64), st[0], st[1], time_major=time_major,
                                               v4_scratch_rows=B), T)


def stack_gate_stats(variant, Ps, x, h0, c0, time_major=False):
    """gate_stats over every layer of a stack; og_low is the top layer's."""
    f64 = torch.float64
    T, B = (x.shape[0], x.shape[1]) if time_major else (x.shape[1], x.shape[0])

    def fn():
        cur = torch.tensor(x, dtype=f64)
        for l, P in enumerate(Ps):
            cur, _, _ = O.literal_sequence(variant, O.to_torch(P, dtype=f64), cur, None if h0 is None else torch.tensor(h0[l], dtype=f64),
                                           None if c0 is None else torch.tensor(c0[l], dtype=f64), time_major=time_major, v4_scratch_rows=B)
    return _watched(fn, T)


# ---- the share of the suite's tolerance a result uses ---------------------------------------------------------------------------------
def _items(res):
    for k in ("y", "hT", "cT"):
        v = res.get(k)
        if isinstance(v, list):
            for l, a in enumerate(v):
                yield f"{k}[{l}]", "out", a
        elif v is not None:
            yield k, "out", v
    for k in ("dx", "dh0", "dc0"):
        v = res.get(k)
        if isinstance(v, list):
            for l, a in enumerate(v):
                yield f"{k}[{l}]", "grad", a
        elif v is not None:
            yield k, "grad", v
    G = res.get("G")
    if isinstance(G, dict):
        for k, a in G.items():
            yield "G." + k, "grad", a
    elif G is not None:
        for l, Gl in enumerate(G):
            for k, a in Gl.items():
                yield f"G[{l}].{k}", "grad", a


def shares(got, ref, may_lack=("dx",)):
    """name -> (share of the tolerance of tests/hip_util.py used, index of the worst element, all finite) for every output and gradient of
    ref; got may lack only the names in may_lack (a first layer asks for no dx)."""
    have = {name: a for name, _, a in _items(got)}
    out = {}
    for name, kind, b in _items(ref):
        if name not in have:
            assert name in may_lack, f"{name} is missing from the result"
            continue
        a, b = np.asarray(have[name], np.float64), np.asarray(b, np.float64)
        assert a.shape == b.shape, (name, a.shape, b.shape)
        err = np.abs(a - b)
        finite = bool(np.all(np.isfinite(a)))
        err = np.where(np.isfinite(err), err, np.inf)
        if kind == "out":
            rel = err / (ATOL + RTOL * np.abs(b))
        else:
            rel = err / (GREL * max(np.abs(b).max(), 1e-6) + 1e-6)
        i = int(rel.argmax()) if rel.size else 0
        out[name] = (float(rel.flat[i]) if rel.size else 0.0, tuple(int(v) for v in np.unravel_index(i, rel.shape)) if rel.size else (), finite)
    return out


def worst(sh):
    name = max(sh, key=lambda k: sh[k][0])
    return name, sh[name][0]


def assert_shares(got, ref, tag, limit=1.0, may_lack=("dx",)):
    """Every output and gradient finite and within limit x the tolerance; on failure, per quantity the share used and the worst index.
    Returns the shares."""
    sh = shares(got, ref, may_lack)
    bad = {k: v for k, v in sh.items() if not v[2] or not v[0] <= limit}
    assert not bad, f"{tag}: beyond {limit:.3g} x the tolerance or not finite:\n" + "\n".join(
        f"  {k}: {v[0]:.3g} x tolerance at {v[1]}{'' if v[2] else ' (NON-FINITE values)'}" for k, v in sorted(sh.items(), key=lambda kv: -kv[1][0]))
    return sh


def fp32_oracle_share(variant, P, x, h0, c0, dy, dhT, dcT, time_major):
    """Worst share of the tolerance the fp32 literal oracle uses against the fp64 one: (quantity, share)."""
    a = run_literal(variant, P, x, h0, c0, dy, dhT, dcT, time_major=time_major, dtype=torch.float32)
    b = run_literal(variant, P, x, h0, c0, dy, dhT, dcT, time_major=time_major)
    return worst(shares(a, b))


def fp32_stack_share(variant, Ps, x, h0, c0, dy, dhT, dcT, time_major):
    a = run_stack_literal(variant, Ps, x, h0, c0, dy, dhT, dcT, time_major, dtype=torch.float32)
    b = run_stack_literal(variant, Ps, x, h0, c0, dy, dhT, dcT, time_major)
    return worst(shares(a, b))


# ---- the case tables -------------------------------------------------------------------------------------------------------------------
# a layer row: (variant, B, T, I, H, w_rank, u_ranks, time_major, with_state, tiers)
HOT, BOTH = ("hot",), ("hot", "rail")

VALU = [
    (V1, 7, 9, 16, 64, 8, [8], False, True, BOTH),
    (V1, 5, 41, 9, 65, 5, [11], True, True, HOT),
    (V1, 2, 3, 30, 200, 16, [24], False, False, HOT),
    (V1, 3, 4, 12, 130, 32, [32], False, True, HOT),
    (V1, 3, 3, 9, 500, 16, [32], False, False, HOT),
    (V1, 300, 3, 6, 40, 4, [4], False, False, HOT),
    (V2, 3, 4, 10, 136, 8, [16, 8], False, True, BOTH),
    (V3, 5, 4, 330, 330, 8, [24], True, True, HOT),
    (V4, 6, 3, 264, 264, 6, [8, 8], True, True, BOTH),
    (V4, 63, 31, 10, 10, 9, [11, 4], False, False, HOT),
    (V5, 5, 6, 9, 70, 5, [7], False, True, HOT),
    (V6, 4, 5, 10, 136, 8, [16, 8], False, True, HOT),
]
VALU_REC3_ROWS = 4          # the first rows also run under the rec3 masks 0 and 7

# the headline layer's three backward forms (riding workers, stand-alone weight gradients, in-row), need_dx=False
HEADLINE = [
    (V1, 64, 40, 9, 180, 16, [16], False, True, BOTH),
    (V1, 8, 41, 9, 180, 16, [16], False, False, BOTH),
]
HEADLINE_FULL = (V1, 64, 128, 9, 180, 16, [16], False, True, HOT)      # config A's length: max |c| beyond 100

RB = [
    (V1, 17, 6, 9, 180, 16, [16], False, True, BOTH),
    (V1, 2, 3, 30, 200, 16, [24], False, False, HOT),
    (V1, 33, 3, 77, 256, 24, [24], False, False, HOT),
    (V2, 20, 6, 9, 180, 16, [16, 16], False, True, HOT),
    (V4, 40, 3, 72, 72, 8, [16, 16], True, True, HOT),
    (V5, 5, 6, 9, 70, 5, [7], False, True, HOT),
]
RB_CLUSTER = [
    (V1, 18, 3, 20, 600, 8, [8], False, True, HOT),
    (V3, 5, 4, 650, 650, 32, [32], True, True, BOTH),
    (V4, 21, 3, 650, 650, 32, [32, 32], True, True, HOT),
]
RB_CLUSTER16 = RB_CLUSTER[2]        # once more with rb_cluster 16, rb_rows 16

# clustered stacks in one launch (H = 650, ranks 32 / [32] or [32, 32], time-major, states per layer): (variant, L, B, T, tiers)
RBX = [
    (V4, 2, 32, 5, HOT),
    (V3, 3, 20, 4, BOTH),
    (V4, 2, 7, 2, HOT),
]
RBX_H, RBX_RW = 650, 32

# wavefront stacks: (variant, B, T, I, hidden sizes, w_rank, u_ranks, with_state, tiers)
WAVE = [
    (V1, 19, 11, 9, [180, 180], 16, [16], True, BOTH),
    (V1, 33, 6, 77, [256, 256], 24, [24], True, HOT),
    (V2, 7, 6, 12, [64, 64], 8, [4, 6], True, HOT),
    (V5, 6, 5, 24, [72, 72], 16, [16], True, HOT),
    (V1, 5, 7, 20, [64, 100, 180], 16, [16], False, HOT),      # unequal sizes take no initial states
    (V1, 4, 1, 12, [40, 40, 40], 8, [8], True, HOT),
]

# the step-wise path; the last column: switches held while the case runs
STEPWISE = [
    (V1, 5, 4, 12, 40, 6, [40], False, True, BOTH, {}),
    (V1, 3, 3, 20, 600, 8, [8], False, False, HOT, {"rb": 0}),
    (V2, 4, 3, 10, 48, 4, [24, 20], False, True, HOT, {}),
    (V4, 7, 3, 44, 44, 5, [20, 36], True, True, HOT, {}),
    (V5, 5, 4, 77, 40, 8, [6], False, True, HOT, {}),
    (V3, 4, 3, 650, 650, 300, [300], True, True, HOT, {}),                 # a wide-rank layer
    (V1, 18, 7, 20, 600, 8, [8], True, True, HOT, {"rb": 0, "wring": 1}),   # tests/test_gpu_wring.py CASES[3] on the LDS-ring weight gradients
]

LAYER_TABLES = {"valu": VALU, "headline": HEADLINE + [HEADLINE_FULL], "rb": RB + RB_CLUSTER, "stepwise": [r[:10] for r in STEPWISE]}


def row_id(row):
    v, B, T, I, H, rw, ru, tm, st = row[:9]
    return "v%d_B%d_T%d_I%d_H%d_r%d_%s_%s%s" % (v, B, T, I, H, rw, "x".join(map(str, ru)), "tm_" if tm else "", "st" if st else "z")


def row_inputs(row, tier, B=None):
    v, B0, T, I, H, rw, ru, tm, st = row[:9]
    return hot_inputs(v, B or B0, T, I, H, rw, ru, tier, tm, st, seed=case_seed(v, B0, T, I, H, rw))


def rbx_ranks(variant):
    return [32, 32] if variant == V4 else [32]


def rbx_inputs(row, tier, B=None):
    v, L, B0, T = row[:4]
    return hot_stack_inputs(v, B or B0, T, RBX_H, [RBX_H] * L, RBX_RW, rbx_ranks(v), tier, True, True, seed=case_seed(v, B0, T, RBX_H, RBX_H, L))


def wave_inputs(row, tier):
    v, B, T, I, Hs, rw, ru, st = row[:8]
    return hot_stack_inputs(v, B, T, I, Hs, rw, ru, tier, False, st, seed=case_seed(v, B, T, I, Hs[-1], len(Hs)))
