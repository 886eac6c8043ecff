"""Weight tying and word-level embedding dropout (docs/design/lm_tied.md): the cases the CPU and the GPU tests share, their seeded
draws, and the numpy statement of the contract of vmlmf_embed_dropout_forward_ex / vmlmf_embed_backward_ex.

Contract.  tokens (R) in [0, V); f (R, H) the element factors of (seed, offset, site 0, p), all ones at p == 0; fw (V) the word
factors, vmlmf_oracle.dropout_factors(seed, offset, SITE_WORD, V, 1, word_p)[:, 0], all ones at word_p == 0.
    forward    out[r] = (w[tok_r] * fw[tok_r]) * f[r]                       two float32 multiplications, in that order
    backward   s[v]  = sum over the positions p with tok_p == v, ascending, of dy[p] * f[p]     float32, one addition per position
               c[v]  = fw[v] * s[v]                                          one float32 multiplication (none at word_p == 0)
               accumulate == 0: dW[v] = c[v]; zeros on rows no token hit and rows of a dropped word
               accumulate == 1: dW[v] = base[v] + c[v] on rows that are hit and whose word is kept (one float32 addition); every other
                                row keeps the bits of base
The kernels form dy[p] * f[p] + s as one fused multiply-add, as the entry points before them do; the cases here use p in {0, 0.5}, where
f is 0, 1 or 2 and the product is exact, so the fused form and the two-step form below have the same bits.

Bound against the exact (fp64) value: a row with h hits carries h roundings in s, one in c and one in the addition onto base, so
|dW[v] - exact| <= gamma(h + 2) (|base[v]| + |fw[v]| sum |dy[p] f[p]|), gamma(k) = k U / (1 - k U), U = 2^-24.

Shapes sit at the partition boundaries of the kernels' geometry: four vocabulary rows per workgroup, 256 columns per round with a quad
per lane, bit words of 32 positions read 64 at a time."""
import numpy as np

import vmlmf_oracle as O

U = 2.0 ** -24
SEED = 0x5EED5EED1234          # with offsets 7 / 8 / 9 it drops 5 / 10 / 6 of 12 words at word_p = 0.5; 2064 and 2058 of 4096 at 7 / 8
SITE_WORD = 0x574F5244         # include/vmlmf_hip.h: VMLMF_SITE_WORD
OFFSETS = (7, 8, 9)

# (R, V, H)
SHAPES = [
    (1, 4, 8),          # the smallest
    (33, 10, 8),        # a second bit word; V % 4 != 0
    (40, 7, 5),         # odd width, a tail quad
    (70, 12, 650),      # the PTB width: rows 8 bytes off (no 16-byte path on every second one), a third column round
    (64, 8, 256),       # exactly one column round
    (64, 8, 260),       # one quad more
    (16, 6, 1024),      # the widest
    (2080, 12, 8),      # 65 bit words: a second round of 64
]
IDS = ["x".join(map(str, s)) for s in SHAPES]
PATTERNS = ["equal", "permutation", "unhit", "last"]
DROPS = [(0.0, 0.0), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5)]          # (p, word_p)


def gamma(k):
    return k * U / (1.0 - k * U)


def tokens(R, V, pattern, seed=0):
    """(R) int64: every token equal; a permutation of the vocabulary (repeated when R > V); tokens that leave rows unhit (even ids
    only, and never the last row); random ones with the token V - 1 at both ends."""
    r = np.random.Generator(np.random.PCG64(1000 + seed))
    if pattern == "equal":
        return np.full(R, V // 2, dtype=np.int64)
    if pattern == "permutation":
        return r.permutation(V).astype(np.int64)[np.arange(R) % V]
    if pattern == "unhit":
        even = np.arange(0, max(V - 1, 1), 2, dtype=np.int64)
        return even[r.integers(0, len(even), size=R)]
    if pattern == "last":
        t = r.integers(0, V, size=R).astype(np.int64)
        t[0] = t[-1] = V - 1
        return t
    raise ValueError(pattern)


def draw(R, V, H, seed):
    """(w (V, H), dy (R, H), base (V, H)) float32."""
    r = np.random.Generator(np.random.PCG64(seed))
    return (r.standard_normal((V, H)).astype(np.float32), (0.1 * r.standard_normal((R, H))).astype(np.float32),
            r.standard_normal((V, H)).astype(np.float32))


def element_factors(R, H, p, offset, site=0, seed=SEED):
    return np.ones((R, H), np.float32) if p == 0 else O.dropout_factors(seed, offset, site, R, H, p)


def word_factors(V, word_p, offset, seed=SEED):
    return np.ones(V, np.float32) if word_p == 0 else O.dropout_factors(seed, offset, SITE_WORD, V, 1, word_p)[:, 0]


def forward(w, tok, f, fw, variant=None):
    """The gather in float32.  variant "f_first": the known-wrong order (w f) fw."""
    w = np.asarray(w, np.float32)
    if variant == "f_first":
        return ((w[tok] * f).astype(np.float32) * fw[tok][:, None]).astype(np.float32)
    return ((w[tok] * fw[tok][:, None]).astype(np.float32) * f).astype(np.float32)


def ordered_sum(tok, dy, f, V, weights=None):
    """s (V, H): the float32 sum of dy[p] f[p] in ascending position order (weights: a further per-position factor, for the wrong
    rules)."""
    dy, f = np.asarray(dy, np.float32), np.asarray(f, np.float32)
    s = np.zeros((V, dy.shape[1]), np.float32)
    term = (dy * f).astype(np.float32)
    if weights is not None:
        term = (term * np.asarray(weights, np.float32)[:, None]).astype(np.float32)
    for p in range(len(tok)):
        s[tok[p]] = (s[tok[p]] + term[p]).astype(np.float32)
    return s


def table_gradient(tok, dy, f, fw, V, base=None, variant=None):
    """dW of the contract in float32; base given: accumulate == 1.  Known-wrong rules - "fw_by_position": the word factor looked up by
    the position's index instead of by its token; "dropped_accumulated": a dropped word's row still takes its (unscaled) sum."""
    hit = np.bincount(tok, minlength=V) > 0
    kept = np.asarray(fw) != 0
    if variant == "fw_by_position":
        c = ordered_sum(tok, dy, f, V, weights=np.asarray(fw)[np.arange(len(tok)) % V])
        kept = np.ones(V, bool)
    else:
        s = ordered_sum(tok, dy, f, V)
        c = (np.asarray(fw, np.float32)[:, None] * s).astype(np.float32)
        if variant == "dropped_accumulated":
            c, kept = np.where(kept[:, None], c, s), np.ones(V, bool)
    if base is None:
        return np.where((hit & kept)[:, None], c, np.float32(0.0)).astype(np.float32)
    out = np.array(base, np.float32, copy=True)
    rows = hit & kept
    out[rows] = (out[rows] + c[rows]).astype(np.float32)
    return out


def exact(tok, dy, f, fw, V, base=None):
    """(value, magnitude, hits) in fp64: the contract without rounding, the sum of the magnitudes of its terms, the hits per row."""
    term = np.asarray(dy, np.float64) * np.asarray(f, np.float64) * np.asarray(fw, np.float64)[tok][:, None]
    val = np.zeros((V, term.shape[1]))
    mag = np.zeros_like(val)
    np.add.at(val, tok, term)
    np.add.at(mag, tok, np.abs(term))
    if base is not None:
        val, mag = val + np.asarray(base, np.float64), mag + np.abs(np.asarray(base, np.float64))
    return val, mag, np.bincount(tok, minlength=V)


def excess(got, tok, dy, f, fw, V, base=None):
    """max over the elements of |got - exact| / (gamma(hits + 2) magnitude): <= 1 inside the bound."""
    val, mag, hits = exact(tok, dy, f, fw, V, base)
    bound = gamma(hits + 2.0)[:, None] * mag + float(np.finfo(np.float32).tiny)
    return float((np.abs(np.asarray(got, np.float64) - val) / bound).max())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def cases():
    """(id, R, V, H, pattern, p, word_p, offset): every shape with every token pattern, the dropout settings and offsets rotating over
    them so that each shape meets all four settings."""
    out = []
    for i, (R, V, H) in enumerate(SHAPES):
        for j, pattern in enumerate(PATTERNS):
            for k, (p, word_p) in enumerate(DROPS):
                out.append((f"{IDS[i]}-{pattern}-p{p}-w{word_p}", R, V, H, pattern, p, word_p, OFFSETS[(i + j + k) % 3]))
    return out


# ---- Model twins -----------------------------------------------------------------------------------------------------------------
def twins(make, device="cpu"):
    """(tied, untied): two models from `make()` with the same values everywhere, the untied twin's fc.w a copy of the table."""
    import torch
    a, b = make(), make()
    b.load_state_dict(a.state_dict())
    a.tie_weights()
    with torch.no_grad():
        b.fc.w.copy_(a.embed.w)
        b.embed.w.copy_(a.embed.w)
    return a.to(device), b.to(device)
