"""The fp64 oracle of the LM head's general training objective - padding mask, label smoothing, z-loss, token-level unlikelihood -
and the cases the two test files share.

With z (R, V) the scores (bias included), y (R) the targets (-1: the row is masked, m_r = 0), p = softmax(z_r), lse_r = logsumexp(z_r),
eps = label_smoothing, zeta = z_loss, alpha = unlikelihood and C_r the SET of the row's negatives (entries outside [0, V) are
padding, duplicates count once, the row's own target is ignored):

    nll_r = lse_r - z_r[y_r]                      sm_r = lse_r - mean_v z_r[v]
    zl_r  = lse_r^2                               ul_r = sum_{c in C_r} -log(max(1 - p_c, 1e-5))
    row_r = (1 - eps) nll_r + eps sm_r + zeta zl_r + alpha ul_r
    loss  = scale sum_r m_r row_r
    dz_r[v] = scale m_r (p_v - (1 - eps)[v = y_r] - eps / V + 2 zeta lse_r p_v + alpha (w_v - p_v S_r))
              w_v = p_v / (1 - p_v) if v in C_r and 1 - p_v > 1e-5, else 0;    S_r = sum_v w_v

The parts are the scale-weighted sums of m_r nll_r, m_r sm_r, m_r zl_r, m_r ul_r, not multiplied by eps, zeta, alpha; a term whose
weight is zero is not formed, so the smooth part is reported as zero at eps == 0 and the unlikelihood part at alpha == 0 (the
negatives are not read then).  Everything here is numpy in float64; the reference has no such objective, so this file is the only
oracle.  Tolerances are distill_cases.LOSS_REL and hip_util.assert_grad's default.
"""
import numpy as np

from distill_cases import LOSS_REL, log_softmax   # noqa: F401  (LOSS_REL: re-exported to the tests)

FLOOR = 1e-5
P_CAP = 0.9   # negatives are drawn from columns with p <= P_CAP: 1 - p keeps a relative error of at most about ten times p's


def member_sets(negatives, y, V):
    """(R, V) bool: column v is in C_r."""
    R = len(y)
    member = np.zeros((R, V), bool)
    if negatives is None:
        return member
    for r in range(R):
        for c in np.asarray(negatives[r]).tolist():
            if 0 <= c < V and c != y[r]:
                member[r, c] = True
    return member


def oracle(z, y, scale, eps=0.0, zeta=0.0, alpha=0.0, negatives=None):
    """z (R, V), y (R) with -1 for a masked row, negatives (R, K) or None.  Returns a dict: loss, the four parts nll / smooth / z / ul
    (scaled), the rows' four terms `rows` (4, R) (unscaled, zero in masked rows), dz (R, V) and its column sums db."""
    z = np.asarray(z, np.float64)
    y = np.asarray(y).reshape(-1)
    R, V = z.shape
    live = y != -1
    assert np.all((y >= -1) & (y < V)), "the oracle takes targets in [0, V) and the mask -1"
    logp = log_softmax(z)
    p = np.exp(logp)
    lse = z[:, 0] - logp[:, 0]
    ysafe = np.where(live, y, 0)
    rows = np.zeros((4, R))
    rows[0] = lse - z[np.arange(R), ysafe]
    if eps > 0:
        rows[1] = lse - z.mean(axis=1)
    rows[2] = lse * lse
    member = member_sets(negatives if alpha > 0 else None, y, V)
    om = 1.0 - p
    rows[3] = -(np.log(np.maximum(om, FLOOR)) * member).sum(axis=1)
    w = np.where(member & (om > FLOOR), p / np.where(om > 0, om, 1.0), 0.0)
    S = w.sum(axis=1, keepdims=True)
    onehot = np.zeros((R, V))
    onehot[np.arange(R), ysafe] = 1.0
    dz = scale * (p - (1.0 - eps) * onehot - eps / V + 2.0 * zeta * lse[:, None] * p + alpha * (w - p * S))
    dz[~live] = 0.0
    rows[:, ~live] = 0.0
    parts = scale * rows.sum(axis=1)
    loss = (1.0 - eps) * parts[0] + eps * parts[1] + zeta * parts[2] + alpha * parts[3]
    return dict(loss=loss, nll=parts[0], smooth=parts[1], z=parts[2], ul=parts[3], parts=parts, rows=rows, dz=dz, db=dz.sum(axis=0))


def assert_losses(got, want, what):
    """got = (loss, nll, smooth, z, ul) against the oracle's dict: the loss to LOSS_REL of itself, each part to LOSS_REL of the
    largest part."""
    got = [float(v.detach()) if hasattr(v, "detach") else float(v) for v in got]
    big = max(np.abs(want["parts"]).max(), 1e-30)
    assert np.isfinite(got).all(), (what, got)
    assert abs(got[0] - want["loss"]) <= LOSS_REL * max(abs(want["loss"]), 1e-30), (what, "loss", got[0], want["loss"])
    for name, g, w in zip(("nll", "smooth", "z", "ul"), got[1:], want["parts"]):
        assert abs(g - w) <= LOSS_REL * big, (what, name, g, w)


def scores_case(R, V, amp, seed, K=0, mask=True):
    """Scores z (R, V) fp32 without the bias, a bias (V), targets y (R) and negatives (R, K) int64 (None at K == 0), extending
    distill_cases.scores_case: row 0's target is column 0, the last row's column V - 1; with `mask`, rows r % 4 == 2 are masked
    (y = -1) where R >= 3.  A row's negatives are drawn only from columns whose fp64 probability - with and without the bias - is at
    most P_CAP, which is asserted; where K allows, one entry is a duplicate of another, one is the row's own target and one is -1."""
    r = np.random.Generator(np.random.PCG64(seed))
    z = (amp * r.standard_normal((R, V))).astype(np.float32)
    bias = r.standard_normal(V).astype(np.float32)
    y = r.integers(0, V, size=R).astype(np.int64)
    y[0] = 0
    if R > 1:
        y[-1] = V - 1
    if not K:
        neg = None
    else:
        p = np.maximum(np.exp(log_softmax(z.astype(np.float64))), np.exp(log_softmax(z.astype(np.float64) + bias)))
        neg = np.empty((R, K), np.int64)
        for row in range(R):
            ok = np.flatnonzero(p[row] <= P_CAP)
            special = [int(y[row]), -1][:max(K - 1, 0)]           # the target itself, padding
            n = K - len(special)
            fresh = r.choice(ok, size=min(n, len(ok)), replace=False).tolist()
            assert fresh, "no column with p <= P_CAP to draw a negative from"
            while len(fresh) < n:                                  # duplicates: from the second entry on where K allows
                fresh.append(fresh[len(fresh) % len(set(fresh))])
            if n >= 2:
                fresh[-1] = fresh[0]                               # always one duplicate
            cols = fresh + special
            neg[row] = np.asarray(cols)[r.permutation(K)] if K > 1 else cols
            real = [c for c in neg[row].tolist() if 0 <= c < V and c != y[row]]
            assert all(p[row, c] <= P_CAP for c in real)
    if mask and R >= 3:
        y[2::4] = -1
    return z, bias, y, neg
