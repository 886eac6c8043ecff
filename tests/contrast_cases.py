"""The step of contrastive search (include/vmlmf_contrast.h) stated in numpy fp64, and the seeded kernel-level cases that
test_contrast_cpu.py and test_gpu_contrast.py share.  Imports nothing from the package and touches no device.

The error bound.  u = 2^-24.  A cosine formed from fp32 unit vectors is off by at most (2 H + 16) u to first order, whatever the order
of summation: H u from the dot product of two vectors of norm <= 1 + eps (sum |a_i b_i| <= 1, each of the H partial sums rounded once),
and (H / 2 + 3) u per vector from its norm (a sum of H squares: relative error <= H u, halved by the square root, + u for the root,
+ u for the reciprocal) and the rounding of the stored product (+ u) - twice, one for the candidate and one for the history row -
and 10 u of slack for the second-order terms.  The maximum over the history adds nothing.  Derived, not measured.
A choice is CLEAR when the fp64 best value beats the runner-up by more than 2 (alpha bound + 4 u): alpha bound for the similarity on
either side, 4 u for expf (2 ulp of p <= 1), the two products and the difference.  The seeds below make every choice clear."""
import functools

import numpy as np

U = 2.0 ** -24
EOS = 3
ALPHA = 0.6
VOCAB = 50                      # the candidates' tokens and log-probabilities come from rows of this many logits
PAD = 3                         # Tcap = t + PAD: room for the appended row and a guard

# (B, k, H, t)
KERNEL_CASES = [(1, 4, 16, 5), (3, 5, 100, 63), (2, 16, 8, 64), (1, 1, 16, 65), (2, 8, 650, 257), (4, 2, 64, 1)]
VARIANTS = ["base", "finished", "twin", "alpha0", "alpha1"]
TWIN = 0                        # the candidate that repeats a history row in the `twin` variant: the most probable one
TWIN_SCALE = 3.0

# one seed per case, settled on the CPU (test_contrast_cpu.py asserts it): every choice of every variant is clear
SEEDS = {(1, 4, 16, 5): 0, (3, 5, 100, 63): 0, (2, 16, 8, 64): 0, (1, 1, 16, 65): 0, (2, 8, 650, 257): 0, (4, 2, 64, 1): 0}


def case_id(case):
    return "B%d-k%d-H%d-t%d" % tuple(case)


def bound(H):
    """The first-order worst case of a cosine from fp32 unit vectors."""
    return (2 * H + 16) * U


def margin(alpha, H, extra=0.0):
    """What the fp64 best must beat the runner-up by for the fp32 choice to be determined."""
    return 2.0 * (alpha * bound(H) + 4 * U + extra)


def alpha_of(variant):
    return {"alpha0": 0.0, "alpha1": 1.0}.get(variant, ALPHA)


def twin_row(t):
    return t // 2


@functools.lru_cache(maxsize=None)
def kernel_case(case, variant="base", seed=None):
    """numpy inputs of one launch: cand_h (B k, H) fp32, cand_tok (B, k) int64, cand_logp (B, k) fp32 (the k most probable of VOCAB
    tokens, in the total order), hist_raw (B, t, H) fp32 - the vectors vmlmf_contrast_append normalises -, finished, length (B) int32,
    alpha, Tcap.  The variants share the base draws."""
    B, k, H, t = case
    rng = np.random.Generator(np.random.PCG64(1000 + (SEEDS[case] if seed is None else seed)))
    cand_h = rng.standard_normal((B * k, H)).astype(np.float32)
    hist_raw = (rng.standard_normal((B, t, H)) * rng.uniform(0.5, 2.0, (B, t, 1))).astype(np.float32)
    logits = rng.standard_normal((B, VOCAB)) * 2.0
    logp = logits - np.log(np.exp(logits).sum(1, keepdims=True))
    order = np.lexsort((np.arange(VOCAB)[None, :].repeat(B, 0), -logp), axis=1)[:, :k]
    cand_tok = order.astype(np.int64)
    cand_logp = np.take_along_axis(logp, order, 1).astype(np.float32)
    length = rng.integers(0, 5, B).astype(np.int32)
    finished = np.zeros(B, dtype=np.int32)
    if variant == "finished":
        finished[0::2] = 1                                # row 0 always; with B > 1 row 1 stays live
    if variant == "twin":
        for b in range(B):
            cand_h[b * k + TWIN] = np.float32(TWIN_SCALE) * hist_raw[b, twin_row(t)]
    return dict(cand_h=cand_h, cand_tok=cand_tok, cand_logp=cand_logp, hist_raw=hist_raw, finished=finished, length=length,
                alpha=alpha_of(variant), Tcap=t + PAD)


def unit64(x):
    """Rows of x as fp64 unit vectors; a zero row stays zero."""
    x = np.asarray(x, dtype=np.float64)
    n = np.sqrt((x * x).sum(-1, keepdims=True))
    return np.divide(x, n, out=np.zeros_like(x), where=n > 0)


def choose(values):
    """(j*, gap): the largest value, equal values to the lower j, a NaN loses to every number, all NaN: 0; gap = best - runner-up
    (inf with fewer than two numbers)."""
    v = np.asarray(values, dtype=np.float64)
    ok = ~np.isnan(v)
    if not ok.any():
        return 0, np.inf
    w = np.where(ok, v, -np.inf)
    j = int(np.argmax(w))                                 # (the first of equal maxima)
    rest = np.delete(w, j)
    rest = rest[~np.isneginf(rest)] if len(rest) else rest
    return j, (w[j] - rest.max() if len(rest) else np.inf)


def step(cand_h, cand_logp, hist_rows, alpha):
    """One row's step in fp64: cand_h (k, H), cand_logp (k), hist_rows (t, H) raw vectors -> (sim (k), values (k), j*, gap)."""
    c = unit64(cand_h)
    h = unit64(hist_rows)
    sim = (c @ h.T).max(1) if len(h) else np.zeros(len(c))
    values = (1.0 - alpha) * np.exp(np.asarray(cand_logp, dtype=np.float64)) - alpha * sim
    j, gap = choose(values)
    return sim, values, j, gap


@functools.lru_cache(maxsize=None)
def kernel_oracle(case, variant="base", seed=None):
    """Per row b: (sim (k), values (k), j*, gap) of the live step - whether the row is finished or not."""
    B, k, H, t = case
    c = kernel_case(case, variant, seed)
    return [step(c["cand_h"][b * k:(b + 1) * k], c["cand_logp"][b], c["hist_raw"][b], c["alpha"]) for b in range(B)]


def all_clear(case, seed=None):
    B, k, H, t = case
    return all(row[3] > margin(alpha_of(v), H) for v in VARIANTS for row in kernel_oracle(case, v, seed))
