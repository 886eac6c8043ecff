"""NT-ASGD (vmlmf_amd.optim.ASGD, asgd_step, vmlmf_asgd_step; docs/design/lm_asgd.md): the fp64 oracle of one step, the rounding bounds
of the doc, an fp32 emulation of the kernel's operation order with known-wrong variants, and the cases the CPU and GPU tests share.
numpy fp64 only: nothing here touches the code under test."""
import numpy as np

from dyneval_cases import NORM_RTOL, SIZES, STEP_CASES, U, flat_state, offsets_of  # noqa: F401  (the shared layout vocabulary)
from optim_cases import EPS_NORM, FLT_MAX, f32

# ---- the bounds' constants: roundings counted in the kernel's operation order (docs/design/lm_asgd.md, "Rounding") ----
K_P = 6           # c: norm + 1e-6, max_norm / . (2); g' = c g; the decay FMA; lr u; p - .      of |p| + lr (|g'| + wd |p|)
K_G = 3           # norm + 1e-6, max_norm / ., g c                                            relative to |c g|
K_A = 4           # 1 / n to fp32; p' - ax, . mu, ax + .                                       of |ax| + mu |p' - ax|
T0_OFF = -1       # the state block's "averaging off"

# hyper-parameters that are fp32 numbers, so that the oracle, torch and the kernel start from the same values
LR, WD = 0.5, 2.0 ** -6


def asgd_oracle(p, g, ax, *, k, t0, lr, wd, max_norm):
    """One applied step numbered k (1-based) in fp64 on lists of fp32 arrays, from the fp32 values of lr, wd and max_norm; t0 < 0:
    averaging off.  The norm is an fp32 number in the kernel: a sum of squares beyond the largest float is inf here too, and a norm
    that is not finite leaves everything unchanged (skipped = True).  Returns a dict: p, g, ax (the new values), norm, c, n, mode
    ("off" | "copy" | "average"), mu, skipped, and mags - per tensor what asgd_bounds needs."""
    lr, wd, max_norm = f32(lr), f32(wd), f32(max_norm)
    p, g, ax = ([np.asarray(a, np.float64) for a in seq] for seq in (p, g, ax))
    with np.errstate(invalid="ignore", over="ignore"):
        sq = sum(float((a * a).sum()) for a in g)
        norm = np.inf if sq > FLT_MAX else float(np.sqrt(sq))
    n = k - 1 - t0
    mode = "off" if t0 < 0 else ("copy" if n <= 1 else "average")
    mu = 1.0 / n if mode == "average" else 1.0
    if not np.isfinite(norm):
        return dict(p=[a.copy() for a in p], g=[a.copy() for a in g], ax=[a.copy() for a in ax], norm=norm, c=1.0, n=n, mode=mode,
                    mu=mu, skipped=True, mags=None)
    c = 1.0 if max_norm <= 0 else min(1.0, max_norm / (norm + EPS_NORM))
    out_p, out_g, out_a, mags = [], [], [], []
    for pi, gi, ai in zip(p, g, ax):
        gc = c * gi
        pn = pi - lr * (gc + wd * pi)
        an = ai.copy() if mode == "off" else (pn.copy() if mode == "copy" else ai + (pn - ai) * mu)
        out_p.append(pn)
        out_g.append(gc)
        out_a.append(an)
        mags.append(dict(sp=np.abs(pi) + lr * (np.abs(gc) + wd * np.abs(pi)), up=lr * np.abs(gc), g=np.abs(gc),
                         sa=np.abs(ai) + mu * np.abs(pn - ai)))
    return dict(p=out_p, g=out_g, ax=out_a, norm=norm, c=c, n=n, mode=mode, mu=mu, skipped=False, mags=mags)


def asgd_bounds(mag, *, c, mode, mu):
    """(bound on |p' - oracle|, on |g' - oracle|, on |ax' - oracle|) per element of one tensor.  c == 1: the gradient keeps its bits
    and the norm's own error does not reach the step; averaging off: ax keeps its bits; a copy carries p's error and nothing else."""
    clip = c < 1.0
    bp = K_P * U * mag["sp"] + (NORM_RTOL * mag["up"] if clip else 0.0)
    bg = (K_G * U + NORM_RTOL) * mag["g"] if clip else np.zeros_like(mag["g"])
    if mode == "off":
        ba = np.zeros_like(bp)
    elif mode == "copy":
        ba = bp
    else:
        ba = mu * bp + K_A * U * mag["sa"]
    return bp, bg, ba


def asgd_ratios(got_p, got_g, got_a, want):
    """The worst |error| / bound over every element of every tensor, for (p, g, ax); an error at a zero bound counts as inf."""
    worst = [0.0, 0.0, 0.0]
    for gp, gg, ga, p, g, a, mag in zip(got_p, got_g, got_a, want["p"], want["g"], want["ax"], want["mags"]):
        bounds = asgd_bounds(mag, c=want["c"], mode=want["mode"], mu=want["mu"])
        for j, (got, ref, bound) in enumerate(zip((gp, gg, ga), (p, g, a), bounds)):
            if ref.size == 0:
                continue
            err = np.abs(np.asarray(got, np.float64).reshape(ref.shape) - ref)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(err == 0, 0.0, err / bound)
            worst[j] = max(worst[j], float(np.nan_to_num(ratio, nan=np.inf).max()))
    return worst


# ---- the cases ----
# clip: max_norm as a multiple of the case's own fp64 norm (0: no clipping asked for; 4: asked for, does not bind; 0.25: binds).
# k: the applied step's number, t0: the count averaging was switched on at.  stale: ax holds values far from p (what a buffer that
# has not been written since construction, or since an earlier run, looks like) - legitimate wherever the rule does not read ax.
VARIANTS = {
    "off_first_step": dict(k=1, t0=T0_OFF, wd=0.0, clip=0.0, stale=True),
    "off_clip_decay": dict(k=7, t0=T0_OFF, wd=WD, clip=0.25, stale=True),
    "off_loose_clip": dict(k=2, t0=T0_OFF, wd=0.0, clip=4.0, stale=True),
    "n0_clip": dict(k=4, t0=3, wd=0.0, clip=0.25, stale=True),
    "n1_loose_decay": dict(k=5, t0=3, wd=WD, clip=4.0, stale=True),
    "n2_clip_decay": dict(k=6, t0=3, wd=WD, clip=0.25, stale=False),
    "n3_no_clip": dict(k=4, t0=0, wd=0.0, clip=0.0, stale=False),
    "n1000_loose_decay": dict(k=1004, t0=3, wd=WD, clip=4.0, stale=False),
    "n99999_clip_decay": dict(k=100007, t0=7, wd=WD, clip=0.25, stale=False),
}
_n = {name: v["k"] - 1 - v["t0"] for name, v in VARIANTS.items() if v["t0"] >= 0}
assert any(v["clip"] == 0.25 for v in VARIANTS.values()) and any(v["clip"] == 4.0 for v in VARIANTS.values())
assert any(v["clip"] == 0.0 for v in VARIANTS.values())
assert any(v["wd"] == 0.0 for v in VARIANTS.values()) and any(v["wd"] > 0.0 for v in VARIANTS.values())
assert any(v["t0"] < 0 for v in VARIANTS.values()) and {0, 1, 2} <= set(_n.values()) and max(_n.values()) >= 1000
# every averaging state meets a clip that binds and one that does not
for _mode in ("off", "copy", "average"):
    _clips = {v["clip"] == 0.25 for name, v in VARIANTS.items()
              if ("off" if v["t0"] < 0 else "copy" if _n[name] <= 1 else "average") == _mode}
    assert _clips == {True, False}, _mode


def asgd_case(numels, seed, stale):
    """fp32 arrays (p, g, ax) per tensor: p 0.1 normal, g 1e-2 normal with a tenth exact zeros, ax near p (an average of recent
    iterates) or, stale, 64 + normal."""
    rng = np.random.Generator(np.random.PCG64(seed))
    p = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in numels]
    g = []
    for n in numels:
        gi = 1e-2 * rng.standard_normal(n)
        gi[rng.uniform(size=n) < 0.1] = 0.0
        g.append(gi.astype(np.float32))
    if stale:
        ax = [(64.0 + rng.standard_normal(n)).astype(np.float32) for n in numels]
    else:
        ax = [(a + 0.02 * rng.standard_normal(a.size)).astype(np.float32) for a in p]
    return p, g, ax


def norm_of(g):
    return float(np.sqrt(sum(float((np.asarray(a, np.float64) ** 2).sum()) for a in g)))


def asgd_fixture(layout, variant, seed):
    """One case as the launch sees it: per-tensor arrays, offsets, the flat ax buffer, max_norm (an fp32 number), the state words
    before the call, and the oracle's answer.  The fixture, not the code under test, vouches that the clip does what the variant says."""
    case, v = STEP_CASES[layout], VARIANTS[variant]
    numels = case["numels"]
    offsets, total = offsets_of(numels, case["pad"])
    p, g, ax = asgd_case(numels, seed, v["stale"])
    max_norm = f32(v["clip"] * norm_of(g))
    want = asgd_oracle(p, g, ax, k=v["k"], t0=v["t0"], lr=LR, wd=v["wd"], max_norm=max_norm)
    assert (want["c"] < 1.0) == (v["clip"] == 0.25) and (v["clip"] == 0.25) == (0 < max_norm < want["norm"])
    assert want["c"] == 1.0 or abs(want["c"] - 0.25) < 1e-3
    return dict(numels=numels, offsets=offsets, total=total, misalign=case["misalign"], p=p, g=g, ax=ax,
                ax_flat=flat_state(ax, offsets, total), max_norm=max_norm, k=v["k"], t0=v["t0"], wd=v["wd"], lr=LR, want=want)


# ---- an fp32 emulation of the kernel's operation order (numpy), for the CPU test: the product-sums once as separate roundings and
# ---- once as fused multiply-adds; `mutate` names a known-wrong variant ----
F = np.float32


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def _muladd(a, b, c, fused):
    return _fma(a, b, c) if fused else (a * b).astype(F) + c


def asgd_emulate(p, g, ax, norm32, *, k, t0, lr, wd, max_norm, fused, mutate=None):
    """asgd_finish_kernel + asgd_kernel on fp32 arrays from the fp32 norm.  Returns (p', g', ax')."""
    lr, wd, max_norm, norm32 = F(lr), F(wd), F(max_norm), F(norm32)
    if not np.isfinite(norm32):
        return [a.copy() for a in p], [a.copy() for a in g], [a.copy() for a in ax]
    coef = F(1)
    if max_norm > 0:
        coef = min(max_norm / (norm32 + F(1e-6)), F(1))
    n = k - 1 - t0 + {"n_plus_1": 1, "n_minus_1": -1}.get(mutate, 0)
    mode = "off" if t0 < 0 else ("copy" if n <= 1 else "average")
    mu = F(1) / F(n) if mode == "average" else F(1)
    out_p, out_g, out_a = [], [], []
    with np.errstate(all="ignore"):
        for pi, gi, ai in zip(p, g, ax):
            if mutate == "decay_before_clip":
                gc = (_fma(wd, pi, gi) * coef).astype(F)
                u = gc
            else:
                gc = (gi * coef).astype(F)
                u = gc if mutate == "decay_without_lr" else _fma(wd, pi, gc)
            pn = _muladd(-lr, u, pi, fused)
            if mutate == "decay_without_lr":
                pn = _muladd(-wd, pi, pn, fused)
            if mode == "off":
                an = ai.copy()
            elif mode == "copy" and mutate != "arithmetic_copy":
                an = pn.copy()
            else:
                an = _muladd((pn - ai).astype(F), mu, ai, fused)
            out_p.append(pn)
            out_g.append(gc)
            out_a.append(an)
    return out_p, out_g, out_a


MUTATIONS = ("n_plus_1", "n_minus_1", "decay_before_clip", "decay_without_lr", "arithmetic_copy")
