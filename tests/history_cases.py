"""The history controls of Model.generate (no_repeat_ngram_size, banned_sequences, frequency_penalty, presence_penalty; C ABI
vmlmf_history_choose / vmlmf_history_bans in libvmlmf_history.so, include/vmlmf_history.h) stated in numpy and fp64, with the seeded
kernel-level cases that test_history_controls_cpu.py and test_gpu_history_controls.py share.  Everything else of the decoder's
contracts - the choice, the filters, the other controls, their cases - is oracle/vmlmf_decode_oracle.py's, imported here as C.
Test-side code: nothing here imports the package.

Per live row, on the fp32 scores x (include/vmlmf_history.h):
  1. repetition   r = seen[v] ? (x > 0 ? x / theta : x theta) : x
  2. penalties    q = (r - alpha count[v]) - (count[v] > 0 ? beta : 0)
  3. bias         c = q + logit_bias[v]
  4. min length   c[eos] = -inf while length < min_length
  5. history bans c[v] = -inf for v in ban_set(history, ...)
then the choice of vmlmf_decode_oracle (filtered_sets / judge) runs on c."""
import functools

import numpy as np

import vmlmf_decode_oracle as C


# ---- the ban set of one row ----
def ban_set(h, V, n, seqs):
    """h: the row's tokens so far (prompt included); n = no_repeat_ngram_size (0: off); seqs: lists of tokens.  Returns a (V) bool mask.
    n-grams: for every i in [0, L - n] with h[i .. i + n - 1) == h[L - n + 1 .. L): ban h[i + n - 1]; nothing while L + 1 < n.
    Sequences: a sequence of one token is always banned; s of m > 1 tokens bans s[m - 1] when L >= m - 1 and the row ends in s[:m - 1]."""
    h = [int(t) for t in h]
    L = len(h)
    out = np.zeros(V, dtype=bool)
    if n >= 1 and L + 1 >= n:
        tail = h[L - n + 1:L]
        for i in range(0, L - n + 1):
            if h[i:i + n - 1] == tail:
                out[h[i + n - 1]] = True
    for s in seqs:
        m = len(s)
        if m == 1 or (L >= m - 1 and h[L - m + 1:L] == list(s[:m - 1])):
            out[s[m - 1]] = True
    return out


def ban_set_by_dictionary(h, V, n, seqs):
    """The same set, formed the way Hugging Face's NoRepeatNGramLogitsProcessor and NoBadWordsLogitsProcessor form theirs: every n-gram
    of the history goes into a dictionary from its first n - 1 tokens to the tokens that followed them; the entry of the history's
    last n - 1 tokens is banned.  A second implementation, for the first to be compared with."""
    h = tuple(int(t) for t in h)
    L = len(h)
    out = np.zeros(V, dtype=bool)
    if n >= 1 and not L + 1 < n:
        followers = {}
        for gram in zip(*[h[i:] for i in range(n)]):
            followers.setdefault(gram[:-1], []).append(gram[-1])
        for t in followers.get(h[L + 1 - n:L], []):
            out[t] = True
    for s in seqs:
        prefix, last = tuple(s[:-1]), s[-1]
        if len(prefix) == 0 or (len(prefix) <= L and h[L - len(prefix):] == prefix):
            out[last] = True
    return out


# ---- the scores the choice runs on ----
def history_scores(x, seen, count, theta, alpha, beta, logit_bias, eos, min_length, length, bans):
    """Steps 1 - 5 in fp64.  x, seen, count, bans (..., V); logit_bias (V) or None; eos a token or None; length (...) or a scalar."""
    x = np.asarray(x, dtype=np.float64)
    cnt = np.asarray(count, dtype=np.float64)
    r = np.where(np.asarray(seen, dtype=bool), np.where(x > 0, x / theta, x * theta), x)
    q = (r - alpha * cnt) - np.where(cnt > 0, beta, 0.0)
    c = q if logit_bias is None else q + np.asarray(logit_bias, dtype=np.float64)
    c = np.array(np.broadcast_to(c, x.shape), dtype=np.float64)
    if eos is not None:
        below = np.broadcast_to(np.asarray(length) < min_length, x.shape[:-1])
        c[..., eos] = np.where(below, -np.inf, c[..., eos])
    c[np.asarray(bans, dtype=bool)] = -np.inf
    return c


def next_history(hist, count, finished_before, tokens):
    """Step 7's history part for live rows: (hist as a list of lists, count) after `tokens`; finished rows are left as they are."""
    hist, count = [list(h) for h in hist], count.copy()
    for b, t in enumerate(tokens):
        if not finished_before[b]:
            hist[b].append(int(t))
            count[b, t] = min(int(count[b, t]) + 1, 65535)
    return hist, count


def unpack(words, V):
    """(B, ceil(V / 32)) 32-bit words of vmlmf_history_bans -> (B, V) bool."""
    w = np.ascontiguousarray(np.asarray(words).astype(np.int32)).view(np.uint8)
    return np.unpackbits(w, axis=1, bitorder="little")[:, :V].astype(bool)


# ---- the kernel-level cases: vmlmf_decode_oracle's (SHAPES, CONTROL_SETTINGS, TAUS; seen, logit_bias, theta, eos, min_length of
# case_controls, every length 0), with a history ----
ALPHABET, HIST_LEN, PROMPT_LEN = 12, 24, 8
N_GRAM, ALPHA, BETA = 2, 0.4, 0.6


@functools.lru_cache(maxsize=None)
def case_history(B, H, V):
    """(hist (B, 24) int64, count (B, V) int64, sequences): the draws in this order from PCG64(777 + V): an alphabet of 12 tokens, the
    rows' 24 tokens from it; a row's first 8 tokens are its prompt, count is the bincount of the other 16; the sequences are
    [a0, a1], [a2], [a3, a4, a5] of the alphabet."""
    rng = np.random.Generator(np.random.PCG64(777 + V))
    alphabet = rng.choice(V, ALPHABET, replace=False)
    hist = alphabet[rng.integers(0, ALPHABET, (B, HIST_LEN))].astype(np.int64)
    count = np.stack([np.bincount(row[PROMPT_LEN:], minlength=V) for row in hist]).astype(np.int64)
    a = [int(t) for t in alphabet]
    return hist, count, [[a[0], a[1]], [a[2]], [a[3], a[4], a[5]]]


@functools.lru_cache(maxsize=None)
def case_bans(B, H, V):
    hist, _, seqs = case_history(B, H, V)
    return np.stack([ban_set(row, V, N_GRAM, seqs) for row in hist])


@functools.lru_cache(maxsize=None)
def case_scores(B, H, V):
    """fp64 raw scores (B, V), history scores (B, V), the sampler's noise G (B, V) and the ban sets (B, V) of a kernel-level case."""
    scores, G = C.case_reference(B, H, V)
    seen, lb = C.case_controls(B, H, V)
    _, count, _ = case_history(B, H, V)
    bans = case_bans(B, H, V)
    return scores, history_scores(scores, seen, count, C.THETA, ALPHA, BETA, lb, C.EOS, C.MIN_LENGTH, 0, bans), G, bans


# the edge histories of the ban set: (n, sequences, histories) over a 97-token vocabulary
EDGE_V = 97
EDGES = [
    (3, [], [[], [4], [4, 5], [4, 5, 4], [4, 5, 6, 4, 5], [4, 5, 6, 4, 5, 7, 4, 5]]),       # L = 0, n - 2, n - 1, n, and matches
    (1, [], [[], [9], [9, 3, 9, 96]]),                                                      # n = 1 bans the history
    (5, [], [[1, 2, 3], [1, 2, 3, 4], [1, 2, 3, 4, 1, 2, 3, 4]]),                            # n > L + 1, n = L + 1, n < L + 1
    (2, [], [[8, 8, 8], [8], [8, 8], [0, 96, 0]]),                                          # a a a: overlapping matches
    (0, [[7, 8, 9, 10], [11], [5, 6]], [[7], [7, 8, 9], [1, 7, 8, 9], [5], [6, 5], []]),     # a prefix longer than the history
    (2, [[4, 5, 31], [32, 64]], [[4, 5, 4, 5], [32, 4, 32], [5, 4, 5, 4, 5]]),               # both kinds together; the bitmap's words
]
