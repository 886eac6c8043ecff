"""The fp64 oracle of knowledge distillation at the LM head, and the cases the two test files share.

With z (R, V) the student's scores (bias included), y (R) the targets, tau the temperature, Q = softmax(z / tau) and the teacher's
distribution P (dense: softmax(teacher / tau); top-k: softmax(top_scores / tau) on top_tokens, zero elsewhere):

    hard_r = logsumexp(z_r) - z_r[y_r]                      soft_r = tau^2 sum_v P_r[v] (log P_r[v] - log Q_r[v])
    loss   = scale sum_r ((1 - alpha) hard_r + alpha soft_r)
    dz_r   = scale ((1 - alpha)(softmax(z_r) - onehot(y_r)) + alpha tau (Q_r - P_r))

Everything here is numpy in float64; the reference has no distillation, so this file is the only oracle.
"""
import numpy as np

# tolerances (the project's own): loss and parts 1e-4 relative, the parts against max(|hard|, |soft|); gradients by
# hip_util.assert_grad's default.  The identical teacher at alpha = 1 has a true gradient of zero: |soft| <= 1e-4 hard and
# |dz| <= 1e-5 tau scale there.
LOSS_REL = 1e-4


def log_softmax(a):
    a = a - a.max(axis=1, keepdims=True)
    return a - np.log(np.exp(a).sum(axis=1, keepdims=True))


def oracle(z, y, scale, alpha, tau, teacher=None, top=None):
    """z (R, V), y (R); teacher (R, V) or top = (tokens (R, k), scores (R, k)).  Returns a dict: loss, hard, soft (scaled), the rows'
    hard and soft terms (unscaled), dz (R, V) and its column sums db."""
    z = np.asarray(z, np.float64)
    y = np.asarray(y).reshape(-1)
    R, V = z.shape
    rows = np.arange(R)
    logp1 = log_softmax(z)
    row_hard = -logp1[rows, y]
    logq = log_softmax(z / tau)
    P = np.zeros((R, V))
    if teacher is not None:
        logp = log_softmax(np.asarray(teacher, np.float64) / tau)
        P = np.exp(logp)
        row_soft = tau * tau * (P * (logp - logq)).sum(axis=1)
    else:
        tok, sc = np.asarray(top[0]), np.asarray(top[1], np.float64)
        assert all(len(set(t)) == len(t) for t in tok.tolist()), "top tokens must be distinct within a row"
        logpk = log_softmax(sc / tau)
        np.put_along_axis(P, tok, np.exp(logpk), axis=1)
        row_soft = tau * tau * (np.exp(logpk) * (logpk - np.take_along_axis(logq, tok, axis=1))).sum(axis=1)
    onehot = np.zeros((R, V))
    onehot[rows, y] = 1.0
    dz = scale * ((1.0 - alpha) * (np.exp(logp1) - onehot) + alpha * tau * (np.exp(logq) - P))
    hard, soft = scale * row_hard.sum(), scale * row_soft.sum()
    return dict(loss=(1.0 - alpha) * hard + alpha * soft, hard=hard, soft=soft, row_hard=row_hard, row_soft=row_soft, dz=dz, db=dz.sum(axis=0))


def assert_losses(got, want, what):
    """got = (loss, hard, soft) against the oracle's dict: the loss to LOSS_REL of itself, the parts to LOSS_REL of the larger part."""
    loss, hard, soft = (float(v.detach()) if hasattr(v, "detach") else float(v) for v in got)
    part = max(abs(want["hard"]), abs(want["soft"]))
    assert np.isfinite([loss, hard, soft]).all(), (what, got)
    assert abs(loss - want["loss"]) <= LOSS_REL * max(abs(want["loss"]), 1e-30), (what, "loss", loss, want["loss"])
    assert abs(hard - want["hard"]) <= LOSS_REL * part, (what, "hard", hard, want["hard"])
    assert abs(soft - want["soft"]) <= LOSS_REL * part, (what, "soft", soft, want["soft"])


def scores_case(R, V, amp, seed, k=0):
    """Student scores z (R, V) fp32 without the bias, a bias (V), targets y (R) - row 0's forced to column 0 and the last row's to
    column V - 1 where there are two rows -, and a teacher independent of the student: dense scores (R, V) fp32 (k == 0) or k distinct
    top tokens and scores per row.  Of a top-k teacher's rows, row r leads with the r-th (mod 3) of: the row's target, column 0,
    column V - 1 - and holds the other two behind it where k allows."""
    r = np.random.Generator(np.random.PCG64(seed))
    z = (amp * r.standard_normal((R, V))).astype(np.float32)
    bias = r.standard_normal(V).astype(np.float32)
    y = r.integers(0, V, size=R).astype(np.int64)
    y[0] = 0
    if R > 1:
        y[-1] = V - 1
    if not k:
        return z, bias, y, (amp * r.standard_normal((R, V))).astype(np.float32), None
    tok = np.empty((R, k), np.int64)
    for row in range(R):
        forced = []
        for c in np.roll([int(y[row]), 0, V - 1], -(row % 3)).tolist():
            if c not in forced:
                forced.append(c)
        forced = forced[:k]
        rest = [c for c in r.permutation(V).tolist() if c not in forced][:k - len(forced)]
        tok[row] = forced + rest
    sc = (amp * r.standard_normal((R, k))).astype(np.float32)
    return z, bias, y, None, (tok, sc)
