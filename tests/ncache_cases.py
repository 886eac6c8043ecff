"""What the tests of Model.cache_score share (test_ncache_cpu.py, test_gpu_ncache.py): the fp64 reference of the contract in
include/vmlmf_ncache.h in plain torch, the tolerance derived per position, and the kernel-level cases.  Importing this touches no
device.

The contract.  Per batch row a cache holds pairs (k_j, w_j); for a position with output q, target y, vocabulary log-probability lv
and the band of the last m = min(window, pairs so far) pairs strictly before it:
    s_j  = theta * dot(q, k_j)
    lc   = log(sum_{j: w_j == y} exp(s_j - M)) - log(sum_j exp(s_j - M)),  M = max_j s_j       (-inf if no w_j == y)
    logp = logaddexp(log1p(-lam) + lv, log(lam) + lc)
m == 0 and lam == 0 give lv; no match gives log1p(-lam) + lv.  theta and lam are what the C ABI receives: fp32 numbers.

The tolerance.  u = 2^-24, gamma_k = k u / (1 - k u).  E = max over the band of gamma_{H+1} theta sum_i |q_i k_ji| bounds the error of
any fp32 evaluation of s_j, in any order of summation; log-sum-exp is 1-Lipschitz in the sup norm, so each of the two logarithms moves
by at most E, the sums of m terms add gamma_m each, and the fp32 exp, log and the mixture a few u relative to the magnitudes involved:
    tol = 2 E + 2 gamma_m + 32 u (1 + |lc| + |logp|)          (|lc| left out where lc = -inf: logp = log1p(-lam) + lv there)
An empty band and lam == 0 ask for more than the tolerance: the bits of lv (assert_close).
One more fact of fp32: a term exp(s_j - M) with s_j - M < log(2^-126) = -87.3 is below the normal range and may vanish.  Where the
reference's lc lies below UNDERFLOW = -80 - every matching term that far below the band's largest - an fp32 evaluation of the contract
may report any lc <= the reference's + tol, -inf included; its logp is held to tol all the same (the cache's share is < e^-80 there).
"""
import functools

import numpy as np
import torch

U = 2.0 ** -24
UNDERFLOW = -80.0


def gamma(k):
    return k * U / (1 - k * U)


# (B, T, n, window, H, V, kind, theta, lam): n pairs carried into a call over T positions.  Together: H 1 and 3 (the tail of the 4-wide
# step), 24, 650 (8-byte pieces) and 2048 (the LDS limit); T 1, 16, 17, 33 (the query-tile edges); window 1, 15, 16, 17, 64; n 0,
# window - 1, window, window + 5; window < T (the band slides inside the call), window > n + T (never full), n = 0 (the first position
# returns lv's bits); "hot": outputs tanh(4 randn) around two prototypes of either sign, so theta dot reaches about +-160
CASES = [
    (1, 1, 0, 1, 1, 2, "plain", 1.0, 0.1),
    (3, 16, 0, 15, 3, 3, "plain", 1.0, 0.1),
    (1, 17, 14, 15, 24, 2, "plain", 1.0, 0.25),
    (3, 33, 16, 16, 24, 4, "plain", 1.0, 0.1),
    (1, 33, 22, 17, 3, 5, "plain", 1.0, 0.1),
    (3, 17, 64, 64, 1, 3, "plain", 2.0, 0.1),
    (3, 17, 1, 1, 24, 2, "plain", 1.0, 0.5),
    (3, 33, 0, 64, 24, 5, "plain", -1.0, 0.1),
    (1, 16, 63, 64, 650, 4, "plain", 0.3, 0.1),
    (3, 33, 69, 64, 650, 3, "plain", 0.3, 0.1),
    (1, 33, 64, 64, 650, 3, "hot", 0.3, 0.1),
    (3, 17, 0, 17, 650, 2, "hot", 0.3, 0.1),
    (1, 17, 5, 17, 2048, 3, "plain", 0.05, 0.1),
]
SEEDS = {case: 100 + i for i, case in enumerate(CASES)}
PARTS = (1, 2, 3, 64, 0)


def case_id(case):
    B, T, n, window, H, V, kind, theta, lam = case
    return f"B{B}-T{T}-n{n}-w{window}-H{H}-V{V}-{kind}"


@functools.lru_cache(maxsize=None)
def inputs(case):
    """keys (B, n + T, H) fp32, toks (B, n + T) int64, lv (T, B) fp32 of a case, on the CPU; read-only."""
    B, T, n, window, H, V, kind, theta, lam = case
    g = torch.Generator().manual_seed(SEEDS[case])
    L = n + T
    if kind == "hot":
        proto = torch.tanh(4 * torch.randn((2, H), generator=g))
        which = torch.randint(0, 2, (B, L), generator=g)
        sign = torch.randint(0, 2, (B, L), generator=g).float() * 2 - 1
        keys = proto[which] * sign[..., None]
        fresh = torch.tanh(4 * torch.randn((B, L, H), generator=g))
        keys = torch.where(torch.rand((B, L, H), generator=g) < 0.1, fresh, keys)
    else:
        keys = torch.tanh(torch.randn((B, L, H), generator=g))
    toks = torch.randint(0, V, (B, L), generator=g)
    lv = -5 * torch.rand((T, B), generator=g) - 0.01
    return keys.float().contiguous(), toks.contiguous(), lv.float().contiguous()


def reference(keys, toks, lv, n, window, theta, lam):
    """The contract in fp64: (logp (T, B), lc (T, B), tol (T, B), m (T, B) int64 - the band's size -, matches (T, B) int64 - how many
    of the band's tokens equal the target).  keys (B, L, H), toks (B, L), lv (T, B), L = n + T; theta and lam are rounded to fp32
    first, as the C ABI receives them."""
    theta, lam = float(np.float32(theta)), float(np.float32(lam))
    k = keys.double()
    B, L, H = k.shape
    T = L - n
    s_all = theta * (k @ k.transpose(1, 2))
    a_all = abs(theta) * (k.abs() @ k.abs().transpose(1, 2))
    logp, lc, tol = (torch.zeros((T, B), dtype=torch.float64) for _ in range(3))
    ms, matches = torch.zeros((T, B), dtype=torch.int64), torch.zeros((T, B), dtype=torch.int64)
    keep, hit = (np.log1p(-lam), np.log(lam)) if lam > 0 else (0.0, -np.inf)
    for b in range(B):
        for t in range(T):
            jr = n + t
            jl = max(0, jr - window)
            m = jr - jl
            v = float(lv[t, b])
            ms[t, b] = m
            if m == 0:
                logp[t, b], lc[t, b], tol[t, b] = v, -np.inf, 32 * U * (1 + abs(v))
                continue
            s = s_all[b, jr, jl:jr]
            same = toks[b, jl:jr] == toks[b, jr]
            matches[t, b] = int(same.sum())
            c = float(torch.logsumexp(s[same], 0) - torch.logsumexp(s, 0)) if bool(same.any()) else -np.inf
            lc[t, b] = c
            if lam == 0:
                logp[t, b] = v
            elif not np.isfinite(c):
                logp[t, b] = keep + v
            else:
                logp[t, b] = np.logaddexp(keep + v, hit + c)
            E = gamma(H + 1) * float(a_all[b, jr, jl:jr].max())
            tol[t, b] = 2 * E + 2 * gamma(m) + 32 * U * (1 + (abs(c) if np.isfinite(c) else 0.0) + abs(float(logp[t, b])))
    return logp, lc, tol, ms, matches


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """reference() of a case's inputs(); read-only."""
    B, T, n, window, H, V, kind, theta, lam = case
    keys, toks, lv = inputs(case)
    return reference(keys, toks, lv, n, window, theta, lam)


def brute_force(keys, toks, lv_full, n, window, theta, lam):
    """The definition itself: per position the cache's distribution over the whole vocabulary, the mixture with the model's, its
    logarithm.  lv_full (T, B, V) fp64 log-probabilities.  Returns (logp_full (T, B, V), cache_p (T, B, V))."""
    theta, lam = float(np.float32(theta)), float(np.float32(lam))
    k = keys.double()
    B, L, H = k.shape
    T, V = L - n, lv_full.shape[-1]
    out = torch.zeros((T, B, V), dtype=torch.float64)
    cache_p = torch.zeros((T, B, V), dtype=torch.float64)
    for b in range(B):
        for t in range(T):
            jr = n + t
            jl = max(0, jr - window)
            if jr == jl:
                out[t, b] = lv_full[t, b]
                continue
            w = torch.softmax(theta * (k[b, jl:jr] @ k[b, jr]), 0)
            cache_p[t, b].index_add_(0, toks[b, jl:jr], w)
            out[t, b] = torch.log((1 - lam) * lv_full[t, b].exp() + lam * cache_p[t, b])
    return out, cache_p


def assert_close(got_logp, got_lc, ref, what, lam):
    """The outputs of an fp32 evaluation (tensors (T, B) on the CPU) against reference()'s tuple, by the rules in this module's
    docstring.  Returns the worst |error| / tol of logp and of lc over the positions that have a tolerance."""
    logp, lc, tol, ms, matches = ref
    gl, gc = got_logp.double(), got_lc.double()
    worst_p = worst_c = 0.0
    T, B = logp.shape
    for t in range(T):
        for b in range(B):
            at = (what, t, b)
            r, c, e, m, k = float(logp[t, b]), float(lc[t, b]), float(tol[t, b]), int(ms[t, b]), int(matches[t, b])
            if m == 0 or k == 0:
                assert float(gc[t, b]) == -np.inf, (at, float(gc[t, b]))        # no match: -inf exactly
            elif k == m:
                assert float(gc[t, b]) == 0.0, (at, float(gc[t, b]))            # all match: 0.0 exactly
            elif c < UNDERFLOW:
                assert float(gc[t, b]) <= c + e, (at, float(gc[t, b]), c)
            else:
                assert abs(float(gc[t, b]) - c) <= e, (at, float(gc[t, b]), c, e)
                worst_c = max(worst_c, abs(float(gc[t, b]) - c) / e)
            if m == 0 or float(np.float32(lam)) == 0:
                assert float(gl[t, b]) == r, (at, float(gl[t, b]), r)           # the bits of lv
            else:
                assert abs(float(gl[t, b]) - r) <= e, (at, float(gl[t, b]), r, e)
                worst_p = max(worst_p, abs(float(gl[t, b]) - r) / e)
    return worst_p, worst_c


def fp32_rule(keys, toks, lv, n, window, theta, lam):
    """The same rule in fp32 torch on the CPU (no code under test): (logp, lc) (T, B) fp32."""
    theta32, lam32 = np.float32(theta), np.float32(lam)
    B, L, H = keys.shape
    T = L - n
    logp, lc = torch.zeros((T, B)), torch.zeros((T, B))
    s_all = (keys @ keys.transpose(1, 2)) * float(theta32)
    for b in range(B):
        for t in range(T):
            jr = n + t
            jl = max(0, jr - window)
            if jr == jl:
                logp[t, b], lc[t, b] = lv[t, b], -np.inf
                continue
            s = s_all[b, jr, jl:jr]
            e = torch.exp(s - s.max())
            same = toks[b, jl:jr] == toks[b, jr]
            c = torch.log(e[same].sum()) - torch.log(e.sum()) if bool(same.any()) else torch.tensor(-np.inf)
            if bool(same.all()):
                c = torch.tensor(0.0)
            lc[t, b] = c
            if lam32 == 0:
                logp[t, b] = lv[t, b]
            elif not np.isfinite(float(c)):
                logp[t, b] = np.float32(np.log1p(-float(lam32))) + lv[t, b]
            else:
                logp[t, b] = torch.logaddexp(np.float32(np.log1p(-float(lam32))) + lv[t, b], np.float32(np.log(float(lam32))) + c)
    return logp, lc
