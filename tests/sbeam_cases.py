"""The step of stochastic beam search (Model.stochastic_beam_search; C ABI vmlmf_sbeam_step in libvmlmf_sbeam.so, include/vmlmf_sbeam.h)
stated in numpy and fp64, with the seeded cases that test_sbeam_cpu.py and test_gpu_sbeam.py share.  The totals are
oracle/vmlmf_decode_oracle.py's row_totals, the noise its gumbel_restated (the sampler's Philox draw: position draw B W + b W + w is row
b W + w of a "batch" of B W rows at step `draw`), the survivors are judged like step_sets' - lo <= chosen <= hi - on the fp64 perturbed
values G, under a margin PER CANDIDATE: KERNEL_MARGIN max(1, exp(T - Z)) of its parent, because dG / dgt = exp(G - gt) lets an fp32 error
of gt grow by about exp(T - Z) (docs/design/lm_sbeam.md has the bound).  Test-side code: nothing here imports the package."""
import functools

import numpy as np
import torch

import vmlmf_decode_oracle as C

EOS = C.EOS_KERNEL
NOISE_SEED, NOISE_OFFSET = 0xC0FFEE, 0               # the {seed, offset} snapshot every kernel-level case draws from

# (B, W, H, V)
BASIC = (1, 4, 16, 97)
ODD = (3, 6, 16, 1000)            # W not a power of two; a ticket per row
WIDE = (1, 32, 8, 64)             # a merge of 1024 threads, W close to V
LONG = (2, 4, 8, 12293)           # rows beyond BS_LDS_V, which re-read their scores
SINGLE = (2, 1, 16, 97)           # W = 1: the sampler's own draw
KERNEL_CASES = [BASIC, ODD, WIDE, LONG, SINGLE]
# base: every beam live at a total and a perturbed value of its own; finished: about a quarter of the beams finished, the last beam
# of every row among them (W = 1: row 0); first: beam 0 at (0, 0), the others at -inf - the first step of a search
VARIANTS = ["base", "finished", "first"]
DRAWS = [0, 5]                    # the steps taken so far: every case runs at both
# chosen so that every row of every case, variant and draw is clear at its margins in the fp64 reference (test_sbeam_cpu.py asserts it)
SEEDS = {BASIC: 1, ODD: 1, WIDE: 1, LONG: 1, SINGLE: 1}


def case_id(case):
    return "x".join(str(v) for v in case)


@functools.lru_cache(maxsize=None)
def kernel_case(case, variant="base"):
    """The fp32 inputs of a kernel-level case: h (B W, H), w (V, H), bias (V), cum (B, W), finished (B, W) bool, length (B, W) int32,
    perturbed (B, W) - CPU tensors drawn in this order from torch.Generator().manual_seed(SEEDS[case]).  A beam's perturbed value is
    its total plus a Gumbel draw, as in a running search."""
    B, W, H, V = case
    g = torch.Generator().manual_seed(SEEDS[case])
    h = torch.randn(B * W, H, generator=g)
    w = torch.randn(V, H, generator=g) * 0.1
    b = torch.randn(V, generator=g)
    cum = -3 * torch.rand(B, W, generator=g)
    fin = torch.rand(B, W, generator=g) < 0.25
    length = ((torch.arange(B * W) * 3) % 5 + 1).to(torch.int32).view(B, W)
    u = torch.rand(B, W, generator=g).clamp(1e-6, 1 - 1e-6)
    T = cum - torch.log(-torch.log(u))
    if variant == "finished":
        if W > 1:
            fin[:, W - 1] = True
            fin[:, 0] = False
        else:
            fin[:] = False
            fin[0, 0] = True
    else:
        fin = torch.zeros((B, W), dtype=torch.bool)
    if variant == "first":
        cum = torch.full((B, W), float("-inf"))
        cum[:, 0] = 0.0
        T = cum.clone()
    return h, w, b, cum, fin, length, T


def noise(B, W, V, draw, seed=NOISE_SEED, offset=NOISE_OFFSET):
    """(B, W, V) fp64 Gumbel noise of the step: the sampler's draw at position draw B W + b W + w."""
    return C.gumbel_restated(seed, offset, draw, B * W, V)[1].reshape(B, W, V)


def conditional(T, Z, gt):
    """G of include/vmlmf_sbeam.h in fp64: T (W, 1), Z (W, 1), gt (W, V)."""
    with np.errstate(all="ignore"):
        u = (T - gt) + np.log1p(-np.exp(gt - Z))
        G = T - np.maximum(u, 0.0) - np.log1p(np.exp(-np.abs(u)))
    G = np.where(gt == Z, T, G)
    return np.where(np.isneginf(T) | np.isneginf(gt), -np.inf, G)


def sbeam_sets(G, valid, W, m):
    """step_sets under a margin per candidate.  G, valid, m (W, V).  Returns (top, lo, hi): top - the flat indices of the first W
    candidates (larger G first, equal G to the lower flat index), in order; lo - the candidates that stay ahead of every candidate
    outside top whatever error within the margins either carries; hi - the candidates that can reach the last of top."""
    flat = np.flatnonzero(np.asarray(valid).ravel())
    g, mm = np.asarray(G, dtype=np.float64).ravel()[flat], np.asarray(m, dtype=np.float64).ravel()[flat]
    assert len(flat) >= W and not np.isnan(g).any()
    order = np.lexsort((flat, -g))
    top, rest = order[:W], order[W:]
    best_out = (g[rest] + mm[rest]).max() if len(rest) else -np.inf
    worst_in = (g[top] - mm[top]).min()
    lo = set(flat[g - mm > best_out].tolist())
    hi = set(flat[g + mm >= worst_in].tolist())
    assert lo <= set(flat[top].tolist()) <= hi
    return flat[top], lo, hi


def in_order(G, m, top):
    """Whether the order of the survivors is beyond fp32's reach too: consecutive G apart by more than both margins."""
    g, mm = np.asarray(G).ravel()[top], np.asarray(m).ravel()[top]
    return bool((g[:-1] - mm[:-1] > g[1:] + mm[1:]).all())


def sbeam_row(x, cum, T, finished, eos, gumbel, margin):
    """One batch row in fp64.  x (W, V) scores with the bias, cum, T (W), finished (W) bool, gumbel (W, V).  Returns (phi (W, V) - the
    plain totals -, gt, G, valid, m - each candidate's margin -, top, lo, hi)."""
    cum, T = np.asarray(cum, dtype=np.float64), np.asarray(T, dtype=np.float64)
    phi, valid = C.row_totals(x, cum, finished, eos)
    W = phi.shape[0]
    fin = np.asarray(finished, dtype=bool) & (eos is not None)
    gt = phi + gumbel
    Z = gt.max(1, keepdims=True)
    G = conditional(T[:, None], Z, gt)
    with np.errstate(all="ignore"):
        amp = np.exp(T - Z[:, 0])
    amp = np.where(np.isfinite(amp), np.maximum(amp, 1.0), 1.0)
    for w in np.flatnonzero(fin):                      # a finished beam keeps its value, exactly
        G[w, eos], amp[w] = T[w], 1.0
    m = margin * amp[:, None] * np.ones_like(G)
    return (phi, gt, G, valid, m) + sbeam_sets(G, valid, W, m)


def scores64(case, variant="base"):
    B, W, H, V = case
    h, w, b = kernel_case(case, variant)[:3]
    return (h.double() @ w.double().t() + b.double()).view(B, W, V).numpy()


@functools.lru_cache(maxsize=None)
def kernel_oracle(case, variant="base", draw=0, seed=NOISE_SEED):
    """Per batch row sbeam_row's results for a kernel-level case at C.KERNEL_MARGIN."""
    B, W, H, V = case
    _, _, _, cum, fin, _, T = kernel_case(case, variant)
    x, gum = scores64(case, variant), noise(B, W, V, draw, seed)
    return [sbeam_row(x[r], cum[r].double().numpy(), T[r].double().numpy(), fin[r].numpy(), EOS, gum[r], C.KERNEL_MARGIN) for r in range(B)]


# ---- the statistical case: B rows that share one row of scores over V tokens, at the first step of a search ----
STAT_B, STAT_H, STAT_V = 512, 4, 6
STAT_SEED = 1                                          # ... of the scores; the noise is NOISE_SEED's
CHI2_999 = {5: 20.515, 29: 58.301}                     # the 0.999 quantiles of chi-square with V - 1 and V (V - 1) - 1 degrees of freedom


@functools.lru_cache(maxsize=None)
def stat_case(W):
    """h (B W, H) - every row the same -, w (V, H), bias (V), and a first step's cum, finished, length, perturbed."""
    g = torch.Generator().manual_seed(STAT_SEED)
    h = torch.randn(1, STAT_H, generator=g).expand(STAT_B * W, STAT_H).contiguous()
    w = torch.randn(STAT_V, STAT_H, generator=g) * 0.3
    b = torch.randn(STAT_V, generator=g) * 0.5
    cum = torch.full((STAT_B, W), float("-inf"))
    cum[:, 0] = 0.0
    zeros = torch.zeros((STAT_B, W), dtype=torch.int32)
    return h, w, b, cum, zeros.bool(), zeros.clone(), cum.clone()


@functools.lru_cache(maxsize=None)
def stat_oracle(W):
    """(p (V) - the row's softmax in fp64 -, rows: sbeam_row's results per batch row)."""
    h, w, b, cum, fin, _, T = stat_case(W)
    x = (h.double() @ w.double().t() + b.double()).view(STAT_B, W, STAT_V).numpy()
    gum = noise(STAT_B, W, STAT_V, 0)
    rows = [sbeam_row(x[r], cum[r].double().numpy(), T[r].double().numpy(), fin[r].numpy(), None, gum[r], C.KERNEL_MARGIN)
            for r in range(STAT_B)]
    return torch.softmax(torch.from_numpy(x[0, 0]), 0).numpy(), rows


def chi_square(counts, expected):
    counts, expected = np.asarray(counts, dtype=np.float64).ravel(), np.asarray(expected, dtype=np.float64).ravel()
    keep = expected > 0
    return float((((counts - expected) ** 2)[keep] / expected[keep]).sum())


def stat_statistic(W, tokens):
    """The chi-square statistic and its degrees of freedom of `tokens` (B, W) - the first W tokens drawn per row - against the
    distribution of a sample without replacement: W = 1 the softmax p, W = 2 the ordered pairs p_i p_j / (1 - p_i)."""
    p = stat_oracle(W)[0]
    V = STAT_V
    tokens = np.asarray(tokens)
    if W == 1:
        return chi_square(np.bincount(tokens[:, 0], minlength=V), STAT_B * p), V - 1
    assert W == 2
    expected = STAT_B * p[:, None] * p[None, :] / (1.0 - p[:, None])
    np.fill_diagonal(expected, 0.0)
    counts = np.zeros((V, V))
    np.add.at(counts, (tokens[:, 0], tokens[:, 1]), 1)
    assert np.trace(counts) == 0
    return chi_square(counts, expected), V * (V - 1) - 1


# ---- model level ----
# Along a search the best hypothesis keeps its value T while its total falls by a few nats a step, so exp(T - Z) - the bound on
# dG / dgt the kernel-level margin is made of - grows past any use (e^25 after eight steps) although almost every candidate's own
# exp(G - gt) stays near 1.  The model-level walk therefore propagates INTERVALS instead: G rises with T and with gt and falls with Z,
# so errors up to d_gt in every gt (and with them in Z = max gt) and up to d_T in a parent's T leave G inside
#   [conditional(T - d_T, Z + d_gt, gt - d_gt), conditional(T + d_T, Z - d_gt, gt + d_gt)]
# - the upper end is T + d_T itself for a candidate that can reach the maximum, the lower end T - d_T for a maximum nobody can overtake.
MODEL_B, MODEL_W, MODEL_STEPS, MODEL_EOS, MODEL_SEED = 2, 4, 8, C.MODEL_EOS, 5


def sbeam_bounds(x, cum, T, finished, eos, gumbel, d_gt, d_T):
    """One batch row in fp64 with the interval every candidate's G stays in: x (W, V), cum, T, d_T (W), finished (W) bool, gumbel (W, V),
    d_gt a number.  Returns (phi, G, valid, G_lo, G_hi)."""
    cum, T, d_T = (np.asarray(t, dtype=np.float64) for t in (cum, T, d_T))
    phi, valid = C.row_totals(x, cum, finished, eos)
    fin = np.asarray(finished, dtype=bool) & (eos is not None)
    gt = phi + gumbel
    Z = gt.max(1, keepdims=True)
    Tc, dc = T[:, None], d_T[:, None]
    G = conditional(Tc, Z, gt)
    G_hi = conditional(Tc + dc, Z - d_gt, np.minimum(gt + d_gt, Z - d_gt))
    G_lo = conditional(Tc - dc, Z + d_gt, gt - d_gt)
    second = np.sort(gt, 1)[:, -2:-1] if gt.shape[1] > 1 else np.full_like(Z, -np.inf)
    safe = (gt == Z) & (second + d_gt < gt - d_gt)                   # a maximum that stays one
    G_lo = np.where(safe, Tc - dc, G_lo)
    for w in np.flatnonzero(fin):                                     # a finished beam keeps its value, exactly
        G[w, eos], G_lo[w, eos], G_hi[w, eos] = T[w], T[w] - d_T[w], T[w] + d_T[w]
    return phi, G, valid, G_lo, G_hi


def interval_sets(G, G_lo, G_hi, valid, W):
    """sbeam_sets on intervals: (top, lo, hi) - lo: the candidates whose lower end stays ahead of every upper end outside top; hi: those
    whose upper end reaches the lowest lower end of top."""
    flat = np.flatnonzero(np.asarray(valid).ravel())
    g, a, b = (np.asarray(t, dtype=np.float64).ravel()[flat] for t in (G, G_lo, G_hi))
    assert len(flat) >= W and not np.isnan(g).any()
    order = np.lexsort((flat, -g))
    top, rest = order[:W], order[W:]
    best_out = b[rest].max() if len(rest) else -np.inf
    lo = set(flat[a > best_out].tolist())
    hi = set(flat[b >= a[top].min()].tolist())
    assert lo <= set(flat[top].tolist()) <= hi
    return flat[top], lo, hi


# ---- deep in a search, at kernel level: the totals a few steps' worth below the values, T - Z about 25 ----
DEEP_CASES, DEEP_SHIFT = [ODD, LONG], 25.0


@functools.lru_cache(maxsize=None)
def deep_case(case):
    """kernel_case(case, "base") with every total DEEP_SHIFT lower: what a search looks like after eight steps."""
    h, w, b, cum, fin, length, T = kernel_case(case, "base")
    return h, w, b, cum - DEEP_SHIFT, fin, length, T


@functools.lru_cache(maxsize=None)
def deep_oracle(case, draw=0):
    """Per batch row (phi, G, valid, G_lo, G_hi, top, lo, hi): sbeam_bounds under errors of C.KERNEL_MARGIN in gt and none in T."""
    B, W, H, V = case
    _, _, _, cum, fin, _, T = deep_case(case)
    x, gum = scores64(case, "base"), noise(B, W, V, draw)
    rows = []
    for r in range(B):
        got = sbeam_bounds(x[r], cum[r].double().numpy(), T[r].double().numpy(), fin[r].numpy(), EOS, gum[r], C.KERNEL_MARGIN, np.zeros(W))
        rows.append(got + interval_sets(got[1], got[3], got[4], got[2], W))
    return rows
