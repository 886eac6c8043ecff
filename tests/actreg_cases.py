"""AR / TAR of Model.loss (docs/design/lm_actreg.md): the fp64 oracle of the contract, the literal AWD-LSTM expression as its second
witness, a numpy float32 restatement of both kernels in their operation order, the counted rounding bounds, and the cases the CPU
and the GPU tests share.

Contract.  raw (T, B, H); f the dropout factors of the site; yd = raw f; m[t,b] = (t < lengths[b]) (no lengths: all ones);
    N_ar = H #{m}   N_tar = H #{t + 1 < T: m[t] m[t+1]}
    AR = sum m yd^2 / max(N_ar, 1)    TAR = sum m[t] m[t+1] (raw[t+1] - raw[t])^2 / max(N_tar, 1)
    penalty = scale (ar AR + tar TAR)                      (Model.loss: scale = B)
    d raw[t] = f (g + m s c_ar yd) + s c_tar (m[t-1] m[t] d_t - m[t] m[t+1] d_{t+1}),  d_t = raw[t] - raw[t-1],
    c_ar = 2 ar scale / max(N_ar, 1), c_tar = 2 tar scale / max(N_tar, 1), s the upstream gradient of the penalty.

Bounds (U = 2^-24, gamma(k) = k U / (1 - k U); the count: docs/design/lm_actreg.md, "Rounding").
  yd        one multiplication: the bits of float32(raw) * float32(f).
  d raw     9 roundings on the longest path (the AR term: c_ar 4, yd 1, c_ar yd 1, g + . 1, f . 1, the last addition 1), held against
            the sum of the magnitudes of the terms - |f g| + |f c_ar yd| + c_tar (|d_t| + |d_{t+1}|) - since d_t - d_{t+1} cancels.
  sums      every term carries 3 roundings (yd or the difference, its square); all terms are >= 0, so the sum is off by at most
            gamma(3 + chain) relative, chain the longest addition chain of the reduction: 4 TC in the thread, 6 + 3 in the
            workgroup, ceil(workgroups / 256) + 6 + 3 in the finishing workgroup.
  parts     + 3 (float(N), the division, the multiplication by the scale);   penalty   + 2 more (the weight, the addition).
"""
import numpy as np

U = 2.0 ** -24
TC = 4                       # time steps per workgroup row of the grid (csrc/vmlmf_dropout.hip: AR_TC)
WG = 256                     # threads per workgroup
ROUNDINGS_DRAW = 9
ROUNDINGS_TERM = 3
F32_TINY = float(np.finfo(np.float32).tiny)


def gamma(k):
    return k * U / (1.0 - k * U)


def workgroups(T, B, H):
    return -(-(B * (-(-H // 4))) // WG), -(-T // TC)


def chain(T, B, H):
    gx, gy = workgroups(T, B, H)
    return 4 * TC + 6 + 3 + -(-(gx * gy) // WG) + 6 + 3


def part_bound(T, B, H):
    return gamma(ROUNDINGS_TERM + chain(T, B, H) + 3)


def penalty_bound(T, B, H):
    return gamma(ROUNDINGS_TERM + chain(T, B, H) + 5)


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# (T, B, H): the smallest shapes at which the kernels can go wrong
SHAPES = [
    (1, 2, 8),        # a single step: no pair at all
    (2, 1, 4),        # one pair, one quad
    (5, 3, 6),        # a tail quad (two columns of the second quad)
    (3, 2, 650),      # rows that start 8 bytes off; 326 quads: a second workgroup along the columns, a batch row split over the two
    (7, 4, 256),      # 16-byte rows; exactly one workgroup of quads
    (70, 1, 8),       # eighteen blocks of time steps: more steps than a block holds
    (16, 2, 12),      # T a multiple of the block: the last block has no halo row, the first one's is row 4
    (9, 3, 5),        # an odd width (rows 4 bytes off), a third block holding one step
    (9, 40, 28),      # 280 quads: the column boundary of the grid not at a row's end, times three blocks of steps: 6 workgroups
]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def lengths_for(T, B, seed):
    """(B) lengths drawn from {0, 1, T, T + 3}, every one of them present when B allows."""
    r = np.random.Generator(np.random.PCG64(seed))
    pool = np.array([0, 1, T, T + 3], dtype=np.int64)
    out = pool[r.integers(0, 4, size=B)]
    out[:min(B, 4)] = r.permutation(pool)[:min(B, 4)]
    return out


def draw(T, B, H, seed, amp=1.0):
    """raw and the head's gradient g, float32."""
    r = np.random.Generator(np.random.PCG64(seed))
    return (amp * r.standard_normal((T, B, H))).astype(np.float32), (0.1 * r.standard_normal((T, B, H))).astype(np.float32)


# ---- the fp64 oracle -------------------------------------------------------------------------------------------------------------
def masks(T, B, lengths):
    n = np.full(B, T, dtype=np.int64) if lengths is None else np.clip(np.asarray(lengths, dtype=np.int64), 0, T)
    m = np.arange(T)[:, None] < n[None, :]
    return m, m[:-1] & m[1:]


def oracle(raw, f, lengths, ar, tar, g=None, scale=None, s=1.0, variant=None):
    """The contract in fp64.  variant: a known-wrong rule the bounds must reject - "tar_over_T" (TAR divided by T instead of T - 1
    steps), "no_first" / "no_last" (the t = 0 / t = T - 1 boundary of the TAR gradient dropped: the term of the pair that touches it is
    missing there), "ar_on_raw" (AR of raw instead of yd)."""
    raw, f = np.asarray(raw, np.float64), np.ones_like(raw, dtype=np.float64) if f is None else np.asarray(f, np.float64)
    T, B, H = raw.shape
    scale = float(B) if scale is None else float(scale)
    m, pair = masks(T, B, lengths)
    yd = raw * f
    n_ar, n_tar = H * int(m.sum()), H * int(pair.sum())
    if variant == "tar_over_T":
        n_tar = H * int(m.sum())
    a = raw if variant == "ar_on_raw" else yd
    d = raw[1:] - raw[:-1]
    s_ar, s_tar = float((m[:, :, None] * a * a).sum()), float((pair[:, :, None] * d * d).sum())
    parts = (scale * s_ar / max(n_ar, 1) if ar > 0 else 0.0, scale * s_tar / max(n_tar, 1) if tar > 0 and n_tar > 0 else 0.0)
    out = dict(yd=yd, n_ar=n_ar, n_tar=n_tar, s_ar=s_ar, s_tar=s_tar, parts=parts, penalty=ar * parts[0] + tar * parts[1])
    if g is not None:
        g = np.asarray(g, np.float64)
        c_ar, c_tar = 2.0 * ar * scale / max(n_ar, 1) * s, 2.0 * tar * scale / max(n_tar, 1) * s
        t_g = f * g
        t_ar = m[:, :, None] * c_ar * (raw if variant == "ar_on_raw" else f * yd)
        prev, nxt = np.zeros_like(raw), np.zeros_like(raw)
        prev[1:] = pair[:, :, None] * d                 # m[t-1] m[t] d_t at t
        nxt[:-1] = pair[:, :, None] * d                 # m[t] m[t+1] d_{t+1} at t
        if variant == "no_first":
            nxt[0] = 0.0
        if variant == "no_last":
            prev[T - 1] = 0.0
        out["draw"] = t_g + t_ar + c_tar * (prev - nxt)
        out["magnitude"] = np.abs(t_g) + np.abs(t_ar) + abs(c_tar) * (np.abs(prev) + np.abs(nxt))
    return out


def awd_lstm(raw, f, ar, tar, g):
    """The literal expression of AWD-LSTM's main.py - alpha dropped_h.pow(2).mean() + beta (raw_h[1:] - raw_h[:-1]).pow(2).mean() -
    under torch autograd in fp64, times B; unmasked cases only.  Returns (B alpha-term, B beta-term, d raw of (yd g).sum() + B penalty)."""
    import torch
    x = torch.tensor(np.asarray(raw, np.float64), requires_grad=True)
    ft = torch.tensor(np.asarray(f, np.float64))
    B = x.shape[1]
    dropped = x * ft
    a = dropped.pow(2).mean()
    b = (x[1:] - x[:-1]).pow(2).mean() if x.shape[0] > 1 else torch.zeros((), dtype=torch.float64)
    total = (dropped * torch.tensor(np.asarray(g, np.float64))).sum() + B * (ar * a + tar * b)
    total.backward()
    return B * float(a.detach()), B * float(b.detach()), x.grad.numpy()


# ---- the kernels' operation order in numpy float32 ------------------------------------------------------------------------------------
def _tree(a):
    """block_sum2 over the last axis of length 256: per wave lane l takes lane l + 32, + 16, ... + 1; then the four waves in order."""
    a = a.reshape(a.shape[:-1] + (4, 64)).astype(np.float32).copy()
    o = 32
    while o > 0:
        a[..., :o] = a[..., :o] + a[..., o:2 * o]
        o >>= 1
    w = a[..., 0]
    out = w[..., 0]
    for i in range(1, 4):
        out = (out + w[..., i]).astype(np.float32)
    return out


def emulate_forward(raw, f, lengths, ar, tar, scale=None):
    """vmlmf_actreg_forward in numpy float32, operation for operation: returns (yd, stats (8) float32)."""
    raw = np.asarray(raw, np.float32)
    T, B, H = raw.shape
    f = np.ones_like(raw) if f is None else np.asarray(f, np.float32)
    scale = np.float32(B if scale is None else scale)
    ar32, tar32 = np.float32(ar), np.float32(tar)
    Q = -(-H // 4)
    gx, gy = workgroups(T, B, H)
    n = np.full(B, T, dtype=np.int64) if lengths is None else np.clip(np.asarray(lengths, dtype=np.int64), 0, T)
    x = np.zeros((T + 1, B, Q * 4), np.float32)
    x[:T, :, :H] = raw
    fp = np.ones((T, B, Q * 4), np.float32)
    fp[:, :, :H] = f
    yd = (x[:T] * fp).astype(np.float32)
    s_ar = np.zeros((gy, gx * WG), np.float32)
    s_tar = np.zeros((gy, gx * WG), np.float32)
    nthreads = B * Q
    for t in range(T):
        by = t // TC
        live = np.repeat(t < n, Q)
        pair = np.repeat(t + 1 < n, Q)
        for e in range(4):
            y = yd[t].reshape(B, Q, 4)[:, :, e].reshape(-1)
            if ar > 0:
                s_ar[by, :nthreads] = np.where(live, (s_ar[by, :nthreads] + (y * y).astype(np.float32)).astype(np.float32), s_ar[by, :nthreads])
            if tar > 0:
                d = (x[t + 1].reshape(B, Q, 4)[:, :, e].reshape(-1) - x[t].reshape(B, Q, 4)[:, :, e].reshape(-1)).astype(np.float32)
                s_tar[by, :nthreads] = np.where(pair, (s_tar[by, :nthreads] + (d * d).astype(np.float32)).astype(np.float32), s_tar[by, :nthreads])
    p_ar = _tree(s_ar.reshape(gy, gx, WG)).reshape(-1)         # workgroup by * gx + bx
    p_tar = _tree(s_tar.reshape(gy, gx, WG)).reshape(-1)
    fin = np.zeros((2, WG), np.float32)
    for w in range(gx * gy):
        fin[0, w % WG] = np.float32(fin[0, w % WG] + p_ar[w])
        fin[1, w % WG] = np.float32(fin[1, w % WG] + p_tar[w])
    S = _tree(fin)
    n_ar, n_tar = int(n.sum()) * H, int(np.maximum(n - 1, 0).sum()) * H
    f_ar, f_tar = np.float32(max(n_ar, 1)), np.float32(max(n_tar, 1))
    stats = np.zeros(8, np.float32)
    if ar > 0:
        stats[1] = np.float32(scale * np.float32(S[0] / f_ar))
        stats[3] = np.float32(np.float32(np.float32(2.0) * ar32 * scale) / f_ar)
    if tar > 0:
        stats[2] = np.float32(scale * np.float32(S[1] / f_tar))
        stats[4] = np.float32(np.float32(np.float32(2.0) * tar32 * scale) / f_tar)
    stats[0] = np.float32(np.float32(ar32 * stats[1]) + np.float32(tar32 * stats[2]))
    stats[5], stats[6] = np.float32(n_ar), np.float32(n_tar)
    return yd[:, :, :H], stats


def emulate_backward(raw, f, lengths, ar, tar, g, stats, s=None):
    """vmlmf_actreg_backward in numpy float32, operation for operation.  s: the upstream gradient of the penalty, None = one."""
    raw, g = np.asarray(raw, np.float32), np.asarray(g, np.float32)
    T, B, H = raw.shape
    drop = f is not None
    c_ar, c_tar = np.float32(stats[3]), np.float32(stats[4])
    if s is not None:
        c_ar, c_tar = np.float32(np.float32(s) * c_ar), np.float32(np.float32(s) * c_tar)
    m, pair = masks(T, B, lengths)
    live = m[:, :, None]
    prev = np.zeros((T, B, 1), bool)
    nxt = np.zeros((T, B, 1), bool)
    prev[1:, :, 0], nxt[:-1, :, 0] = pair, pair
    x = raw
    u = g
    if ar > 0:
        yd = (x * np.asarray(f, np.float32)).astype(np.float32) if drop else x
        u = np.where(live, (g + (c_ar * yd).astype(np.float32)).astype(np.float32), g)
    if drop:
        u = (np.asarray(f, np.float32) * u).astype(np.float32)
    if tar > 0:
        xm = np.concatenate([np.zeros_like(x[:1]), x[:-1]])
        xp = np.concatenate([x[1:], np.zeros_like(x[:1])])
        dt, dn = (x - xm).astype(np.float32), (xp - x).astype(np.float32)
        d = np.where(prev & nxt, (dt - dn).astype(np.float32), np.where(prev, dt, -dn))
        u = np.where(prev | nxt, (u + (c_tar * d).astype(np.float32)).astype(np.float32), u)
    return u.astype(np.float32)


# ---- the checks ------------------------------------------------------------------------------------------------------------------
def check_stats(stats, want, T, B, H, ar, tar, what):
    """penalty and parts of a forward against the oracle's, within the counted bounds; a term that is off is exactly zero."""
    stats = np.asarray(stats, np.float64)
    pb, qb = part_bound(T, B, H), penalty_bound(T, B, H)
    for i, name in ((0, "ar"), (1, "tar")):
        ref = want["parts"][i]
        err = abs(stats[1 + i] - ref)
        print(f"{what}: {name}_part {stats[1 + i]!r} want {ref!r} err {err:.3e} bound {pb * abs(ref):.3e}")
        assert err <= pb * abs(ref) + F32_TINY, f"{what}: {name}_part {stats[1 + i]} vs {ref}: {err:.3e} > {pb * abs(ref):.3e}"
        if (ar, tar)[i] == 0:
            assert stats[1 + i] == 0.0, f"{what}: {name}_part formed at weight 0"
    err = abs(stats[0] - want["penalty"])
    print(f"{what}: penalty {stats[0]!r} want {want['penalty']!r} err {err:.3e} bound {qb * abs(want['penalty']):.3e}")
    assert err <= qb * abs(want["penalty"]) + F32_TINY, f"{what}: penalty {stats[0]} vs {want['penalty']}"


def draw_excess(got, want):
    """max over the elements of |got - d raw| / (gamma(9) magnitude): <= 1 inside the bound."""
    err = np.abs(np.asarray(got, np.float64) - want["draw"])
    return float((err / (gamma(ROUNDINGS_DRAW) * want["magnitude"] + F32_TINY)).max())


def check_draw(got, want, what):
    assert np.all(np.isfinite(got)), what + ": non-finite gradient"
    worst = draw_excess(got, want)
    print(f"{what}: d raw at {worst:.3f} of its bound")
    assert worst <= 1.0, f"{what}: d raw at {worst:.3f} of the counted bound"


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
