"""The optimizer launches of csrc/vmlmf_optim.hip (Adam in its four forms, clip + SGD): the fp64 oracle of the two rules, the rounding
bounds of docs/design/optimizer_bounds.md and the cases the CPU and GPU tests share.  numpy fp64 only: nothing here touches the code
under test."""
import numpy as np

from dyneval_cases import NORM_RTOL, SIZES, STEP_CASES, U, flat_state, offsets_of  # noqa: F401  (the shared layout vocabulary)

# ---- the bounds' constants: roundings counted in the kernels' operation order (docs/design/optimizer_bounds.md) ----
K_M = 5           # g' (one fused multiply-add), g' - m, 1 - b1, the product, m + .          each of at most |m| + |(1 - b1)(g' - m)|
K_V = 6           # g' squared (2), 1 - b2, (1 - b2) g', . g', the sum                        relative: every term of v' is >= 0
K_P = 1           # p - u                                                                   of |p| + |u|
K_U = 12          # step_size: 1 - b1^s, lr / . (2); denominator: v' (K_V / 2), sqrt, 1 - b2^s and its sqrt (1.5), the division, + eps
                  # (7.5 in all); m' / denom; step_size * .   -> 11.5, rounded up              relative to |u|
P_POW = 16.0      # ulps of the device powf: the OpenCL limit OCML's pow is written to (the fallback; see the doc for why)
POW_FLOOR = 2.0 ** -149   # a denormal result of powf is off by absolute spacing, not by ulps of itself
K_SGD = 5         # norm + 1e-6, max_norm / ., g c, lr g', p - .                            of |p| + |lr c g|
K_SGD_UNCLIPPED = 2       # c = 1 exactly (no clip asked for, or the clamp binds): lr g, p - .
K_G = 3           # norm + 1e-6, max_norm / ., g c                                          relative to |c g|
EPS_NORM = float(np.float32(1e-6))     # the kernel's 1e-6f
FLT_MAX = float(np.finfo(np.float32).max)


def f32(x):
    return float(np.float32(x))


# ---- Adam ----
HYPERS = {
    "defaults": dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0),
    "wd": dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01),
    "b1_0": dict(lr=1e-3, b1=0.0, b2=0.999, eps=1e-8, wd=0.0),
    "eps_1e-3": dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-3, wd=0.0),
    "betas_.5_.75": dict(lr=2e-3, b1=0.5, b2=0.75, eps=1e-8, wd=0.0),
}
STARTS = {"0": 0, "9": 9, "999": 999, "99999": 99999, "mixed": None}     # mixed: MIXED[i % 5] for tensor i
MIXED = (0, 9, 999, 99999, 1)

BIG = 2 ** 20 + 13        # beyond ADAM_FUSED_MAX: tick_health_kernel + adam_kernel, and a grid-stride loop that wraps
LAYOUTS = {name: case for name, case in STEP_CASES.items() if name != "million"}
LAYOUTS["million"] = dict(numels=[5, BIG, 1025], pad=True, misalign={})
LAYOUTS["zero_length"] = dict(numels=[0, 5, 0, 1024, 1023, 0], pad=False, misalign={})   # numel = 0 with non-null pointers


def starts_of(key, count):
    s = STARTS[key]
    return [MIXED[i % len(MIXED)] if s is None else s for i in range(count)]


def adam_case(numels, starts, seed):
    """fp32 arrays (p, g, m, v) per tensor.  g: a tenth exact zeros, a tenth of magnitude 1e-9 .. 1e-7 (sqrt(v') at or below eps = 1e-8
    on a first step), the rest 1e-2 normal.  Moments: zero where the tensor's step count starts at 0, else sqrt(v) log-uniform over
    1e-9 .. 1e-1 (so sqrt(v') <~ eps also away from the first step, where the gradient is small too) and m = sqrt(v) * normal."""
    rng = np.random.Generator(np.random.PCG64(seed))
    p, g, m, v = [], [], [], []
    for n, s in zip(numels, starts):
        kind = rng.uniform(size=n)
        gi = 1e-2 * rng.standard_normal(n)
        tiny = 10.0 ** rng.uniform(-9.0, -7.0, n) * rng.choice([-1.0, 1.0], n)
        gi = np.where(kind < 0.1, 0.0, np.where(kind < 0.2, tiny, gi))
        root = 10.0 ** rng.uniform(-9.0, -1.0, n)
        root = np.where((kind >= 0.1) & (kind < 0.2), root * 1e-7 / (root + 1e-7), root)     # small v where g is small
        mi = root * rng.standard_normal(n)
        if s == 0:
            root, mi = np.zeros(n), np.zeros(n)
        p.append((0.1 * rng.standard_normal(n)).astype(np.float32))
        g.append(gi.astype(np.float32))
        m.append(mi.astype(np.float32))
        v.append((root.astype(np.float32)) ** 2)
    return p, g, m, v


def adam_fixture(layout, start_key, seed):
    """One Adam case as the launches see it: per-tensor arrays, the flat moment buffers (total + 1 elements), the step counters behind
    a step_index that is not the identity (tensor i owns counter count - 1 - i)."""
    case = LAYOUTS[layout]
    numels = case["numels"]
    count = len(numels)
    starts = starts_of(start_key, count)
    offsets, total = offsets_of(numels, case["pad"])
    sidx = [count - 1 - i for i in range(count)]
    p, g, m, v = adam_case(numels, starts, seed)
    steps = np.zeros(count, np.float32)
    for i, s in enumerate(starts):
        steps[sidx[i]] = s
    return dict(numels=numels, starts=starts, offsets=offsets, total=total, sidx=sidx, misalign=case["misalign"], p=p, g=g, m=m, v=v,
                m_flat=flat_state(m, offsets, total + 1), v_flat=flat_state(v, offsets, total + 1), steps=steps)


def adam_oracle(p, g, m, v, starts, *, lr, b1, b2, eps, wd):
    """torch.optim.Adam's rule in fp64 on lists of arrays from the fp32 values of the hyper-parameters; starts: each tensor's step
    count before the step.  Returns (p', m', v', mags): mags[i] holds what adam_bounds needs - |p|, |u| (the update), the first
    moment's magnitude |m| + |(1 - b1)(g' - m)|, gain = step_size / denom and the bias corrections' amplification
    r_k = b_k^s / (1 - b_k^s)."""
    lr, b1, b2, eps, wd = (f32(x) for x in (lr, b1, b2, eps, wd))
    out_p, out_m, out_v, mags = [], [], [], []
    for pi, gi, mi, vi, s0 in zip(p, g, m, v, starts):
        pi, gi, mi, vi = (np.asarray(a, np.float64) for a in (pi, gi, mi, vi))
        s = float(s0) + 1.0
        pw1, pw2 = b1 ** s, b2 ** s
        gp = gi + wd * pi
        t = (gp - mi) * (1.0 - b1)
        mn = mi + t
        vn = b2 * vi + (1.0 - b2) * gp * gp
        step_size = lr / (1.0 - pw1)
        denom = np.sqrt(vn) / np.sqrt(1.0 - pw2) + eps
        u = step_size * mn / denom
        out_p.append(pi - u)
        out_m.append(mn)
        out_v.append(vn)
        mags.append(dict(p=np.abs(pi), u=np.abs(u), m=np.abs(mi) + np.abs(t), gain=step_size / denom,
                         r1=(pw1 + POW_FLOOR / (P_POW * U)) / (1.0 - pw1) if b1 > 0 else 0.0,
                         r2=(pw2 + POW_FLOOR / (P_POW * U)) / (1.0 - pw2) if b2 > 0 else 0.0))
    return out_p, out_m, out_v, mags


def adam_bounds(mag, vn):
    """(bound on |p' - oracle|, on |m' - oracle|, on |v' - oracle|) per element, from one tensor's magnitudes and the oracle's v'."""
    bm = K_M * U * mag["m"]
    bv = K_V * U * vn
    rel = K_U * U + P_POW * U * (mag["r1"] + 0.5 * mag["r2"])
    rel = rel * (1.0 + 2.0 * rel)                     # the relative errors meet in a quotient: second order, visible only where P r is large
    bp = K_P * U * (mag["p"] + mag["u"]) + rel * mag["u"] + mag["gain"] * bm
    return bp, bm, bv


def adam_ratios(got_p, got_m, got_v, want):
    """The worst |error| / bound over every element of every tensor, for (p, m, v); an error at a zero bound counts as inf."""
    wp, wm, wv, mags = want
    worst = [0.0, 0.0, 0.0]
    for gp, gm, gv, p, m, v, mag in zip(got_p, got_m, got_v, wp, wm, wv, mags):
        for k, (got, ref, bound) in enumerate(zip((gp, gm, gv), (p, m, v), adam_bounds(mag, v))):
            if ref.size == 0:
                continue
            err = np.abs(np.asarray(got, np.float64) - ref)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(err == 0, 0.0, err / bound)
            worst[k] = max(worst[k], float(np.nan_to_num(ratio, nan=np.inf).max()))
    return worst


# ---- clip + SGD ----
def sgd_clip_oracle(p, g, *, lr, max_norm):
    """norm, c = min(1, max_norm / (norm + 1e-6)) (1 when max_norm <= 0), g' = c g, p' = p - lr g' in fp64 from the fp32 values of lr
    and max_norm.  The norm is an fp32 number in the kernel: a sum of squares beyond the largest float is inf here too, and a norm
    that is not finite leaves everything unchanged.  Returns (p', g', norm, c)."""
    lr, max_norm = f32(lr), f32(max_norm)
    p, g = ([np.asarray(a, np.float64) for a in seq] for seq in (p, g))
    with np.errstate(invalid="ignore", over="ignore"):
        sq = sum(float((a * a).sum()) for a in g)
        norm = np.inf if sq > FLT_MAX else float(np.sqrt(sq))
    if not np.isfinite(norm):
        return [a.copy() for a in p], [a.copy() for a in g], norm, 1.0
    c = 1.0 if max_norm <= 0 else min(1.0, max_norm / (norm + EPS_NORM))
    gn = [c * a for a in g]
    return [a - lr * b for a, b in zip(p, gn)], gn, norm, c


def sgd_bounds(p, gn, *, lr, c):
    """(bound on |p' - oracle|, on |g' - oracle|) per element of one tensor; gn: the oracle's g'.  c == 1: the gradient keeps its
    bits, and the norm's own error does not reach the parameters."""
    u = np.abs(f32(lr) * np.asarray(gn, np.float64))
    mag = np.abs(np.asarray(p, np.float64)) + u
    if c == 1.0:
        return K_SGD_UNCLIPPED * U * mag, np.zeros_like(u)
    return K_SGD * U * mag + NORM_RTOL * u, (K_G * U + NORM_RTOL) * np.abs(gn)


def sgd_case(numels, seed, scale=1e-2):
    rng = np.random.Generator(np.random.PCG64(seed))
    p = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in numels]
    g = []
    for n in numels:
        gi = scale * rng.standard_normal(n)
        gi[rng.uniform(size=n) < 0.1] = 0.0
        g.append(gi.astype(np.float32))
    return p, g


# the three norms relative to max_norm: clipping active, inactive (c == 1), no clipping asked for
CLIPS = {"active": 0.25, "inactive": 4.0, "off": 0.0}


# ---- fp32 emulations of the kernels' operation order (numpy), for the CPU test: each product-sum once as separate roundings and once
# ---- as a fused multiply-add; `mutate` names a known-wrong variant ----
F = np.float32


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def _muladd(a, b, c, fused):
    return _fma(a, b, c) if fused else (a * b).astype(F) + c


def adam_emulate(p, g, m_flat, v_flat, steps, offsets, sidx, *, lr, b1, b2, eps, wd, fused, mutate=None):
    """One step of adam_kernel on fp32 arrays: steps (already ticked, as tick_kernel leaves them) is read through sidx, the moments
    through the state offsets of the flat buffers (one element longer than the states, so that the shifted-offset mutation stays
    inside them).  Returns (p' per tensor, m_flat', v_flat')."""
    lr, b1, b2, eps, wd = (F(x) for x in (lr, b1, b2, eps, wd))
    m_flat, v_flat = m_flat.copy(), v_flat.copy()
    one = F(1)
    out = []
    with np.errstate(all="ignore"):
        for i, (pi, gi) in enumerate(zip(p, g)):
            si = sidx[i]
            if mutate == "neighbour_counter":
                si = sidx[(i + 1) % len(sidx)]
            s = F(steps[si]) + F({"s_minus_1": -1, "s_plus_1": 1}.get(mutate, 0))
            off = offsets[i] + (1 if mutate == "offset_plus_1" else 0)
            n = pi.size
            bc1, bc2 = one - np.power(b1, s, dtype=F), one - np.power(b2, s, dtype=F)
            step_size, bc2s = lr / bc1, np.sqrt(bc2)
            mi, vi = m_flat[off:off + n], v_flat[off:off + n]
            gp = _fma(wd, pi, gi) if wd != 0 and mutate != "adamw" else gi
            mn = _muladd(gp - mi, one - b1, mi, fused)
            vn = _muladd(vi, b2, ((one - b2) * gp) * gp, fused)
            m_flat[off:off + n], v_flat[off:off + n] = mn, vn
            if mutate == "eps_before_division":
                denom = (np.sqrt(vn) + eps) / bc2s
            else:
                denom = np.sqrt(vn) / bc2s + eps
            base = pi if mutate != "adamw" else _muladd(-(lr * wd), pi, pi, fused)
            out.append(_muladd(-step_size, mn / denom, base, fused))
    return out, m_flat, v_flat


ADAM_MUTATIONS = ("s_minus_1", "s_plus_1", "eps_before_division", "adamw", "neighbour_counter", "offset_plus_1")


def sgd_emulate(p, g, norm32, *, lr, max_norm, fused, mutate=None):
    """sgd_clip_kernel on fp32 arrays from the fp32 norm.  Returns (p', g')."""
    lr, max_norm, norm32 = F(lr), F(max_norm), F(norm32)
    if not np.isfinite(norm32):
        return [a.copy() for a in p], [a.copy() for a in g]
    coef = F(1)
    with np.errstate(all="ignore"):
        if max_norm > 0:
            coef = max_norm / (norm32 if mutate == "no_1e-6" else norm32 + F(1e-6))
            if mutate != "no_clamp":
                coef = min(coef, F(1))
        gn = [(a * coef).astype(F) for a in g]
        return [_muladd(-lr, b, a, fused) for a, b in zip(p, gn)], gn


SGD_MUTATIONS = ("no_1e-6", "no_clamp")
