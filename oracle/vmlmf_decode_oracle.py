"""The decoder's contracts stated in numpy and fp64: what Model.generate, Model.beam_search and Model.score (vmlmf_amd/decoding.py,
scoring.py; include/vmlmf_hip.h, vmlmf_decode.h, vmlmf_beam.h, vmlmf_score.h) are held to by tests/, with the seeded kernel-level
cases the CPU and the GPU tests share.  Like vmlmf_oracle.py this is test-side code: the shipped package never imports it, and nothing
here imports the package - a model is whatever object the caller passes (its state_dict(), rnns and lstm_type are read).

  the sampler's draw      gumbel_restated
  top-k / top-p           filtered_sets, nucleus_eps, judge, ambiguous_share; the cases SHAPES x SETTINGS x TAUS
  controls                controlled_scores, next_state; the cases' seen / logit_bias / eos (case_controls, case_controlled)
  scoring                 score_oracle
  beam search             step_sets, row_totals; kernel_case / kernel_oracle; oracle_beam_search over the literal layers
"""
import functools

import numpy as np
import torch

import vmlmf_oracle as O

MARGIN = 2e-3          # |score| differences fp32 cannot order after ~30 recurrent steps (scores are O(1))
LP_TOL = 2e-4          # log-probabilities against the oracle's log-softmax
SITE_SAMPLE = 0x53414D50   # VMLMF_SITE_SAMPLE (include/vmlmf_hip.h): the token sampler's Philox site


# ---- the literal layers under the head ----
def _oracle_scores(m, tokens):
    """fp64 literal forward of `m` over tokens (T, B) from zero states: (scores (T, B, V), [(hT, cT)])."""
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    variant = O.V4 if m.lstm_type == "vmgroup" else O.V3
    h = sd["embed.w"][tokens.cpu()]
    B = tokens.shape[1]
    states = []
    for i in range(len(m.rnns)):
        P = {k.split(".", 2)[2]: v for k, v in sd.items() if k.startswith(f"rnns.{i}.")}
        H = m.rnns[i].hidden_size
        z = torch.zeros(B, H, dtype=torch.float64)
        h, hT, cT = O.literal_sequence(variant, P, h, z, z.clone(), g=2, time_major=True, v4_scratch_rows=B)
        states.append((hT, cT))
    scores = torch.addmm(sd["fc.b"], h.reshape(-1, h.shape[2]), sd["fc.w"].t()).view(h.shape[0], B, -1)
    return scores, states


# ---- the sampler's draw ----
def gumbel_restated(seed, offset, step, B, V):
    """(B, V) Gumbel noise of the sampler at `step`: counter (step B + b, v >> 2, SITE_SAMPLE, offset low word), key (seed low,
    seed high + offset high), word = out[v & 3], u = ((word >> 8) + 0.5) 2^-24, G = -log(-log u) in fp64."""
    v = np.arange(V)
    ctr = np.zeros((B, V, 4), dtype=np.uint32)
    ctr[..., 0] = (step * B + np.arange(B, dtype=np.int64)).astype(np.uint32)[:, None]
    ctr[..., 1] = (v >> 2).astype(np.uint32)[None, :]
    ctr[..., 2] = np.uint32(SITE_SAMPLE)
    ctr[..., 3] = np.uint32(offset & 0xFFFFFFFF)
    key = np.array([seed & 0xFFFFFFFF, ((seed >> 32) + (offset >> 32)) & 0xFFFFFFFF], dtype=np.uint32)
    w = O.philox4x32_10(ctr, key)
    word = np.take_along_axis(w, np.broadcast_to((v & 3)[None, :, None], (B, V, 1)), axis=2)[..., 0]
    u = ((word >> 8).astype(np.float64) + 0.5) * 2.0 ** -24
    return u, -np.log(-np.log(u))


# ---- top-k and nucleus (top-p): the filters act on the tempered scores z = scores / tau under one total order (larger z first, equal z
# to the lower index).  fp32 scores cannot order near-equal tokens, so the oracle returns two sets per row: `lo`, the tokens kept under
# any admissible rounding, and `hi`, the tokens possibly kept ----
# the kernel holds a token's mass in fixed point with 40 fractional bits (the row's largest token weighs 2^40): a rounding of at most
# 2^-41 per token against a sum of at least 2^40 - the issue's V 2^-31 term, adjusted to this format
MASS_BITS = 40


def nucleus_eps(p, margin, V):
    """How far a cumulative mass may be off: the score margin carried into the probabilities, and the fixed-point rounding."""
    return p * (np.exp(2 * margin) - 1) + V * 2.0 ** -MASS_BITS


def filtered_sets(z, top_k, top_p, margin=0.0, eps=0.0):
    """z (V) fp64 tempered scores -> (lo, hi) boolean masks over the vocabulary.  margin = eps = 0: the exact kept set, twice.
    top_k None / 0 / >= V and top_p None / 1.0: off."""
    V = z.shape[0]
    order = np.lexsort((np.arange(V), -z))            # larger z first, equal z to the lower index
    zs = z[order]
    k = V if not top_k or top_k >= V else int(top_k)
    lo = np.ones(V, bool)
    hi = np.ones(V, bool)
    if k < V and margin == 0.0:
        lo = np.zeros(V, bool)
        lo[order[:k]] = True                          # the first k of the order: equal scores are told apart by their index
        hi = lo.copy()
    elif k < V:
        lo = z > zs[k] + margin                       # above the (k+1)-th score by more than the margin
        hi = z >= zs[k - 1] - margin                  # not below the k-th score by more than the margin
    if top_p is not None and top_p < 1.0:
        mass = np.exp(zs[:k] - zs[0])
        mass /= mass.sum()
        before = np.concatenate([[0.0], np.cumsum(mass)[:-1]])          # mass of the tokens before sorted position j < k
        # a token beyond position k can only enter in the place of the last one top-k kept (a score within the margin of it)
        before_all = np.concatenate([before, np.full(V - k, before[-1])])
        b = np.empty(V)
        b[order] = before_all
        lo &= b < top_p - eps
        hi &= b < top_p + eps
    lo[order[0]] = True                               # the first token is always kept
    hi |= lo
    return lo, hi


def judge(z, G, lo, hi, token, kept, margin, what):
    """The rule a filtered GPU choice passes by.  z, G (V) fp64; returns whether the row is unambiguous (argmax over lo == over hi)."""
    zg = z + G
    best_lo = np.flatnonzero(lo)[np.argmax(zg[lo])]
    best_hi = np.flatnonzero(hi)[np.argmax(zg[hi])]
    assert hi[token], (what, "token outside hi", token)
    assert zg[token] >= zg[best_lo] - margin, (what, "a kept token beats it", token, best_lo, zg[token], zg[best_lo])
    if kept is not None:
        assert lo.sum() <= kept <= hi.sum(), (what, "kept", kept, lo.sum(), hi.sum())
    if best_lo == best_hi:
        assert token == best_lo or abs(zg[token] - zg[best_lo]) <= margin, (what, token, best_lo)
    return best_lo == best_hi


def ambiguous_share(z, G, k, p, margin):
    """Share of the rows of z (R, V) whose argmax of z + G differs between lo and hi: a property of the oracle's sets alone."""
    n = 0
    for zr, gr in zip(z, G):
        lo, hi = filtered_sets(zr, k, p, margin, nucleus_eps(p or 1.0, margin, zr.shape[0]))
        zg = zr + gr
        n += np.flatnonzero(lo)[np.argmax(zg[lo])] != np.flatnonzero(hi)[np.argmax(zg[hi])]
    return n / z.shape[0]


# ---- the kernel-level cases of the filters ----
LDS_ROW = 12288                                       # the longest row whose keys the choice kernel holds in LDS (SF_LDS_V)
SHAPES = [(3, 32, 97), (19, 40, 33), (40, 700, 1000), (1, 650, 10000), (2, 16, LDS_ROW + 5)]
SETTINGS = ["k10", "p0.9", "kp"]
TAUS = [0.7, 1.0]
SEED, STEP = 0x5EED_F117, 3


def setting(name, V):
    return {"k10": (10, None), "p0.9": (None, 0.9), "kp": (50 if V >= 100 else V // 2, 0.9)}[name]


@functools.lru_cache(maxsize=None)
def case_inputs(B, H, V):
    """h (B, H), w (V, H) scaled as the unfiltered tests' (0.1), bias (V), embed (V, H): CPU tensors from a seeded generator."""
    g = torch.Generator().manual_seed(1000 * B + V)
    h = torch.randn(B, H, generator=g)
    w = torch.randn(V, H, generator=g) * 0.1
    b = torch.randn(V, generator=g)
    e = torch.randn(V, H, generator=g)
    return h, w, b, e


@functools.lru_cache(maxsize=None)
def case_reference(B, H, V):
    """fp64 scores (B, V) and the sampler's noise G (B, V) at (SEED, offset 0, STEP)."""
    h, w, b, _ = case_inputs(B, H, V)
    scores = (h.double() @ w.double().t() + b.double()).numpy()
    return scores, gumbel_restated(SEED, 0, STEP, B, V)[1]


# ---- stopping and token controls (include/vmlmf_decode.h), per live row, on the fp32 scores x:
#   1. repetition   r = seen[v] ? (x > 0 ? x / theta : x theta) : x
#   2. bias         c = r + logit_bias[v]                       (entries finite or -inf)
#   3. min length   c[eos] = -inf while length < min_length
# then the choice above runs on c ----
def controlled_scores(x, seen, theta, logit_bias, eos, min_length, length):
    """Steps 1 - 3 in fp64.  x (..., V) raw scores; seen (..., V) bool; logit_bias (V) or None; eos a token or None; length (...) or a
    scalar: the rows' lengths so far.  Returns c (..., V)."""
    x = np.asarray(x, dtype=np.float64)
    r = np.where(np.asarray(seen, dtype=bool), np.where(x > 0, x / theta, x * theta), x)
    c = r if logit_bias is None else r + np.asarray(logit_bias, dtype=np.float64)
    c = np.array(np.broadcast_to(c, x.shape), dtype=np.float64)
    if eos is not None:
        below = np.broadcast_to(np.asarray(length) < min_length, x.shape[:-1])
        c[..., eos] = np.where(below, -np.inf, c[..., eos])
    return c


def next_state(seen, length, finished, tokens, eos):
    """Step 6 for live rows: (seen, length, finished) after `tokens` (B); finished rows are left as they are."""
    seen, length, finished = seen.copy(), length.copy(), finished.copy()
    for b, t in enumerate(tokens):
        if finished[b]:
            continue
        seen[b, t] = True
        length[b] += 1
        if eos is not None and t == eos:
            finished[b] = 1
    return seen, length, finished


# ---- the kernel-level cases of the controls: the filters' cases, with controls ----
CONTROL_SETTINGS = SETTINGS + ["off"]
THETA, EOS, MIN_LENGTH = 1.3, 7, 1


def control_setting(name, V):
    return (None, None) if name == "off" else setting(name, V)


def z_margin(tau, theta=THETA, base=1e-4):
    """fp32 against fp64 on the tempered controlled score: the score's own margin, scaled by what the penalty can multiply it by."""
    return base * max(theta, 1.0 / theta) / tau


@functools.lru_cache(maxsize=None)
def case_controls(B, H, V):
    """(seen (B, V) bool, logit_bias (V) fp32 with -inf entries): the draws in this order from PCG64(4242 + V).  theta = THETA,
    eos = EOS held back by min_length = MIN_LENGTH (every row's length is 0)."""
    rng = np.random.Generator(np.random.PCG64(4242 + V))
    seen = rng.random((B, V)) < 0.3
    lb = rng.standard_normal(V).astype(np.float32)
    lb[rng.random(V) < 0.1] = -np.inf
    return seen, lb


@functools.lru_cache(maxsize=None)
def case_controlled(B, H, V):
    """fp64 raw scores (B, V), controlled scores (B, V) and the sampler's noise G (B, V) of a kernel-level case."""
    scores, G = case_reference(B, H, V)
    seen, lb = case_controls(B, H, V)
    return scores, controlled_scores(scores, seen, THETA, lb, EOS, MIN_LENGTH, 0), G


# ---- scoring: per row, on x = bias + scores in fp32, the tokens' ORDER is larger x first, equal x to the lower index;
# logprob = x[y] - logsumexp(x); rank = how many tokens are ahead of y in the order; the top tokens are the order's first `top` ----
def score_oracle(scores_f32, bias_f32, targets, top):
    """scores (R, V) fp32, bias (V) fp32 or None, targets (R) integers (< 0: no target) or None, top in [0, V].  x is formed by the fp32
    add, the order by np.lexsort on (x descending, index ascending), the log-probabilities in fp64 from x.  Returns (logprob (R) f64,
    rank (R) int64, top_tokens (R, top) int64, top_logprob (R, top) f64, order (R, V)); a row without a target has (0.0, -1)."""
    s = np.asarray(scores_f32, dtype=np.float32)
    x = s + (np.float32(0) if bias_f32 is None else np.asarray(bias_f32, dtype=np.float32)[None, :])
    assert x.dtype == np.float32
    R, V = x.shape
    y = np.full(R, -1, dtype=np.int64) if targets is None else np.asarray(targets, dtype=np.int64)
    x64 = x.astype(np.float64)
    m = x64.max(1)
    lse = m + np.log(np.exp(x64 - m[:, None]).sum(1))
    order = np.stack([np.lexsort((np.arange(V), -x[r])) for r in range(R)])
    place = np.empty_like(order)
    np.put_along_axis(place, order, np.broadcast_to(np.arange(V), (R, V)), 1)      # place[r, v]: how many tokens are ahead of v
    has = y >= 0
    yc = np.where(has, y, 0)
    rows = np.arange(R)
    logprob = np.where(has, x64[rows, yc] - lse, 0.0)
    rank = np.where(has, place[rows, yc], -1)
    top_tokens = order[:, :top].astype(np.int64)
    top_logprob = np.take_along_axis(x64, top_tokens, 1) - lse[:, None]
    return logprob, rank, top_tokens, top_logprob, order


# ---- beam search: the rule a GPU step is judged by.  Of a batch row's candidates (flat index w V + v, fp64 total) and a margin m,
# step_sets returns the exact first W of the total order (larger total first, equal totals to the lower flat index), `lo` - the
# candidates above the (W + 1)-th total by more than m: whatever fp32 does, they must be kept - and `hi` - the candidates not below the
# W-th total by more than m: nothing else may be kept.  A step passes when lo <= chosen <= hi and |chosen| = W; it is CLEAR when
# lo == hi, and then the chosen set is the oracle's exactly ----
EOS_KERNEL = 7
KERNEL_MARGIN = 1e-4     # the margin the filtered-sampling tests use on the same GEMM scores
KERNEL_CASES = [(3, 4, 32, 97), (5, 3, 40, 33), (2, 8, 700, 1000), (1, 16, 650, 10000), (1, 5, 16, 12293), (7, 1, 32, 97), (2, 32, 32, 97)]
MODEL_CASES = [("group", 3, 4, 11), ("plain", 3, 4, 13), ("plain", 2, 8, 11)]     # kind, B, W, prompt seed
MODEL_EOS, MODEL_STEPS = 3, 12



def step_sets(totals, valid, W, m):
    """totals, valid (W, V): the fp64 totals of one batch row's candidates and which of them exist (a finished beam offers eos alone).
    Returns (top, lo, hi): top - the flat indices of the first W candidates, in order; lo, hi - sets of flat indices (see above)."""
    flat = np.flatnonzero(np.asarray(valid).ravel())
    t = np.asarray(totals, dtype=np.float64).ravel()[flat]
    assert len(flat) >= W and not np.isnan(t).any()
    order = np.lexsort((flat, -t))                       # by total, larger first; equal totals by flat index
    top = flat[order[:W]]
    t_w = t[order[W - 1]]
    t_next = t[order[W]] if len(flat) > W else -np.inf
    lo = set(flat[t > t_next + m].tolist())
    hi = set(flat[t >= t_w - m].tolist())
    assert lo <= set(top.tolist()) <= hi
    return top, lo, hi


def row_totals(x, cum, finished, eos):
    """x (W, V) fp64 scores with the bias, cum (W), finished (W) bool -> (totals (W, V), valid (W, V)) of one batch row."""
    lsm = torch.log_softmax(torch.as_tensor(x, dtype=torch.float64), -1).numpy()
    totals = np.asarray(cum, dtype=np.float64)[:, None] + lsm
    valid = np.ones(totals.shape, dtype=bool)
    for w in np.flatnonzero(np.asarray(finished)):
        if eos is not None:
            valid[w] = False
            valid[w, eos] = True
            totals[w, eos] = cum[w]
    return totals, valid


def kernel_case(B, W, H, V):
    """The prescribed fp32 inputs of a kernel-level case, and lengths of the test's own (1 .. 5)."""
    g = torch.Generator().manual_seed(1000 * B + V + W)
    h = torch.randn(B * W, H, generator=g)
    w = torch.randn(V, H, generator=g) * 0.1
    b = torch.randn(V, generator=g)
    cum = -3 * torch.rand(B, W, generator=g)
    finished = torch.rand(B, W, generator=g) < 0.25
    length = ((torch.arange(B * W) * 3) % 5 + 1).to(torch.int32).view(B, W)
    return h, w, b, cum, finished, length


_KERNEL_ORACLE = {}


def kernel_oracle(case, finished=None):
    """Per batch row (totals, valid, top, lo, hi) of a kernel-level case in fp64 (computed once per case)."""
    key = (case, None if finished is None else tuple(finished.reshape(-1).tolist()))
    if key not in _KERNEL_ORACLE:
        B, W, H, V = case
        h, w, b, cum, fin, _ = kernel_case(*case)
        fin = fin if finished is None else finished
        x = (h.double() @ w.double().t() + b.double()).view(B, W, V).numpy()
        rows = []
        for r in range(B):
            totals, valid = row_totals(x[r], cum[r].double().numpy(), fin[r].numpy(), EOS_KERNEL)
            rows.append((totals, valid) + step_sets(totals, valid, W, KERNEL_MARGIN))
        _KERNEL_ORACLE[key] = rows
    return _KERNEL_ORACLE[key]


def model_margin(j):
    return MARGIN + 2 * (j + 1) * LP_TOL


def oracle_last_scores(m, seqs):
    """fp64 literal forward over seqs (T, R) from zero states: the scores after the last token (R, V), and the final states."""
    scores, states = _oracle_scores(m, seqs)
    return scores[-1].numpy(), states


def oracle_beam_search(m, prompt, W, steps, eos):
    """Beam search in fp64 along the oracle's own path (the literal layers over every hypothesis' whole prefix, step by step).
    Returns (clear: one bool per (step, batch row), finished (B, W) at the end, hyps (steps, B, W), cum (B, W))."""
    T0, B = prompt.shape
    hyps = np.zeros((0, B, W), dtype=np.int64)
    cum = np.full((B, W), -np.inf)
    cum[:, 0] = 0.0
    fin = np.zeros((B, W), dtype=bool)
    clear = []
    for j in range(steps):
        seqs = torch.cat([prompt[:, :, None].expand(T0, B, W), torch.from_numpy(hyps)]).reshape(T0 + j, B * W)
        x, _ = oracle_last_scores(m, seqs)
        x = x.reshape(B, W, -1)
        V = x.shape[-1]
        new_h, new_c, new_f = np.zeros((j + 1, B, W), dtype=np.int64), np.zeros((B, W)), np.zeros((B, W), dtype=bool)
        for b in range(B):
            totals, valid = row_totals(x[b], cum[b], fin[b], eos)
            top, lo, hi = step_sets(totals, valid, W, model_margin(j))
            clear.append(lo == hi)
            for r, f in enumerate(top):
                par, tok = divmod(int(f), V)
                new_h[:j, b, r], new_h[j, b, r] = hyps[:, b, par], tok
                new_c[b, r], new_f[b, r] = totals[par, tok], fin[b, par] or tok == eos
        hyps, cum, fin = new_h, new_c, new_f
    return clear, fin, hyps, cum
