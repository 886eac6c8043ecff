"""The contract of the truncation samplers (min_p, typical_p, epsilon_cutoff, eta_cutoff of Model.generate; include/vmlmf_truncate.h)
stated in numpy and fp64, with the seeded kernel-level cases the CPU and the GPU tests share.  Test-side code: it stands on
oracle/vmlmf_decode_oracle.py (filtered_sets for top-k / top-p, the cases, the noise, judge) and never imports the package.

All of it acts on the tempered scores z = c / tau under one total order (larger z first, equal z to the lower index); a token at -inf is
never kept.  The stages run in Hugging Face's order - top_k, top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff -, each on the
distribution renormalised over the survivors of the stages before it, each keeping at least its own first token:
  min_p = a        keep v iff p_v >= a p_max, i.e. z_v - z_max >= log a; ties are in together
  typical_p = m    c_v = z_max - z_v, cbar = sum p c over the survivors (the entropy minus log S), d_v = |c_v - cbar|; in the order
                   "smaller d first, equal d to the lower index" keep the token at position j iff the mass before it is < m
  epsilon = e      keep v iff p_v >= e; the most probable survivors stay anyway
  eta = n          H the survivors' entropy: keep v iff p_v >= min(n, sqrt(n) exp(-H)); the most probable survivors stay anyway

fp32 cannot order near-equal quantities, so truncated_sets returns two sets, as filtered_sets does: `lo`, the tokens kept under every
admissible rounding, and `hi`, the tokens possibly kept.  Admissible: a score moves by `margin` (so a difference of two scores by
2 margin), a deviation - a difference of a difference and a mean of differences - by 4 margin, a cumulative mass by nucleus_eps, a
probability by the factor exp(2 margin) and the fixed-point term V 2^-40, the entropy by 2 margin plus that term.  Where an EARLIER stage left
tokens undecided (in hi, not in lo) a later stage's sums are not known exactly either: with a the share of the undecided tokens' mass,
S moves by the factor (1 + a), cbar by at most sum p |c - cbar| over them, H by at most sum p (|log p| + 1) over them plus a; the later
stage's slack grows by that.  With margin = eps = 0 both sets are the exact set.
"""
import numpy as np

import vmlmf_decode_oracle as C
from vmlmf_decode_oracle import SEED, SHAPES, STEP, TAUS, case_controlled, case_inputs, case_reference, gumbel_restated, judge  # noqa: F401

OFF = dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
SETTINGS = ["minp", "typ", "eps", "eta", "all"]


def setting(name, V):
    """(top_k, top_p, truncation keywords) of a named setting."""
    if name == "all":
        return 50 if V >= 100 else V // 2, 0.95, dict(min_p=0.02, typical_p=0.9, epsilon_cutoff=0.5 / V)
    return None, None, {"minp": dict(min_p=0.1), "typ": dict(typical_p=0.9), "eps": dict(epsilon_cutoff=2.0 / V),
                        "eta": dict(eta_cutoff=8.0 / V)}[name]


def _first(mask, key):
    """The first token of `mask` in the order "larger key first, equal keys to the lower index", as a mask."""
    out = np.zeros(mask.shape, bool)
    idx = np.flatnonzero(mask)
    if len(idx):
        out[idx[np.lexsort((idx, -key[idx]))[0]]] = True
    return out


def truncated_sets(z, top_k, top_p, trunc, margin=0.0, eps=0.0):
    """z (V) fp64 tempered scores -> (lo, hi) boolean masks over the vocabulary.  trunc: a dict with any of min_p, typical_p,
    epsilon_cutoff, eta_cutoff (missing, None, 0 / 1.0 / 0 / 0: off).  margin = eps = 0: the exact kept set, twice."""
    z = np.asarray(z, dtype=np.float64)
    V = z.shape[0]
    t = dict(OFF)
    t.update({k: v for k, v in (trunc or {}).items() if v is not None})
    fin = np.isfinite(z)
    lo, hi = C.filtered_sets(z, top_k, top_p, margin, eps)
    ex = C.filtered_sets(z, top_k, top_p)[0]
    lo, hi, ex = lo & fin, hi & fin, ex & fin
    exact = margin == 0.0 and eps == 0.0
    idx = np.arange(V)
    zmax = z[fin].max()
    mass = np.where(fin, np.exp(np.where(fin, z, 0.0) - zmax), 0.0)
    c = np.where(fin, zmax - np.where(fin, z, 0.0), np.inf)
    fp = 0.0 if exact else V * 2.0 ** -C.MASS_BITS
    rel = np.exp(2 * margin) - 1

    def undecided():
        """(share of the mass, bound on cbar's move, bound on H's move) the tokens in hi and not in lo stand for."""
        u = hi & ~lo
        if not u.any():
            return 0.0, 0.0, 0.0
        S = mass[ex].sum()
        p = mass / S
        cbar = (p[ex] * c[ex]).sum()
        a = p[u].sum()
        logp = np.abs(np.log(np.maximum(p[u], 1e-300)))
        return a, (p[u] * np.abs(c[u] - cbar)).sum(), (p[u] * (logp + 1)).sum() + a

    def close(slo, sex, shi, first):
        nonlocal lo, hi, ex
        lo, ex, hi = lo & slo, ex & sex, hi & shi
        ex |= first
        lo |= first
        hi |= lo | ex

    if t["min_p"] > 0.0:
        la = np.log(t["min_p"])
        x = np.where(fin, z - zmax, -np.inf)
        close(x >= la + 2 * margin, x >= la, x >= la - 2 * margin, _first(ex, z))

    if t["typical_p"] < 1.0:
        m = t["typical_p"]
        a, dc, _ = undecided()
        S = mass[ex].sum()
        p = mass / S
        cbar = (p[ex] * c[ex]).sum()
        d = np.abs(c - cbar)
        members = np.flatnonzero(ex)
        order = members[np.lexsort((members, d[members]))]          # smaller d first, equal d to the lower index
        before = np.full(V, np.inf)
        before[order] = np.concatenate([[0.0], np.cumsum(p[order])[:-1]])
        sex = before < m
        if exact:
            slo, shi = sex, sex
        else:
            dm = 4 * margin + dc
            em = max(eps, C.nucleus_eps(m, margin, V)) + a
            ds, cum = d[order], np.cumsum(p[order])
            at = lambda n: np.where(n > 0, cum[np.maximum(n, 1) - 1], 0.0)
            most = at(np.searchsorted(ds, d + dm, "right")) - np.where(ex, p, 0.0)      # everything that may come before v
            least = at(np.searchsorted(ds, d - dm, "left"))                               # everything that must
            slo, shi = fin & (most < m - em), fin & (least < m + em)
        close(slo, sex, shi, _first(ex, -d))

    for name in ("epsilon_cutoff", "eta_cutoff"):
        if t[name] <= 0.0:
            continue
        a, _, dh = undecided()
        S = mass[ex].sum()
        p = mass / S
        sl = rel + fp + a
        if name == "epsilon_cutoff":
            thr = thr_lo = thr_hi = t[name]
        else:
            pe = p[ex & (p > 0)]
            H = -(pe * np.log(pe)).sum()
            hm = 0.0 if exact else 2 * margin + fp + dh
            eta = t[name]
            thr, thr_lo, thr_hi = (min(eta, np.sqrt(eta) * np.exp(-h)) for h in (H, H - hm, H + hm))
        top = ex & (z == z[ex].max())
        close((p >= thr_lo * (1 + sl)) | top, (p >= thr) | top, (p >= thr_hi * (1 - sl)) | top, top)
    return lo, hi


def exact_set(z, top_k=None, top_p=None, **trunc):
    """The indices of the exact kept set."""
    lo, hi = truncated_sets(np.asarray(z, dtype=np.float64), top_k, top_p, trunc)
    assert np.array_equal(lo, hi)
    return np.flatnonzero(lo).tolist()


def case_sets(z, name, margin):
    """(lo, hi) of one row of a named setting, with the margin's nucleus_eps."""
    k, p, trunc = setting(name, z.shape[0])
    return truncated_sets(z, k, p, trunc, margin, C.nucleus_eps(p or 1.0, margin, z.shape[0]))


def ambiguous_share(z, G, name, margin):
    """Share of the rows of z (R, V) whose argmax of z + G differs between lo and hi: a property of the oracle's sets alone."""
    n = 0
    for zr, gr in zip(z, G):
        lo, hi = case_sets(zr, name, margin)
        zg = zr + gr
        n += np.flatnonzero(lo)[np.argmax(zg[lo])] != np.flatnonzero(hi)[np.argmax(zg[hi])]
    return n / z.shape[0]
