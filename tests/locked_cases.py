"""Locked (variational) dropout (docs/design/lm_locked.md): the rule restated and the case tables the CPU and the GPU tests share.

THE RULE.  A site's locked factors are ONE (B, H) mask per forward pass, shared by every time step: the factor of (t, b, n) is the
per-element scheme's factor at position b - counter (b, column >> 2, site | VMLMF_SITE_LOCKED, offset low word) under the same key -
so with the numpy Philox restatement that tests/test_dropout.py pins on Random123's known answers (vmlmf_oracle.dropout_factors):

    locked[t, b, n] = dropout_factors(seed, offset, site | 2^31, rows=B, H, p)[b, n]        for every t

The site word carries the flag, so a site's locked stream is apart from its per-element stream.  Everything a kernel does with the
factors is what it does with per-element ones; the restatements of tied_cases.py (gather, table gradient) and actreg_cases.py (AR /
TAR) are therefore reused on these factor tensors, with their tolerances."""
import numpy as np

import vmlmf_oracle as O

SITE_LOCKED = 1 << 31                 # include/vmlmf_hip.h: VMLMF_SITE_LOCKED
SEED = 0x5EED5EED1234
OFFSETS = (7, 2 ** 32 + 5)            # the second reaches the key's high word
RECIPE = (0.4, 0.25, 0.4)             # AWD-LSTM's PTB command: --dropouti, --dropouth, --dropout

# (T, B, H).  drop_rows_kernel under a locked mask: a thread keeps (b, four columns) for four steps - T = 3 and 2 a short walk, 4
# exactly one, 35 eight full walks and one of three; H = 7 / 2 / 130 a tail quad, 650 the PTB width (rows 8 bytes off); B = 1, 5, 33.
FACTOR_SHAPES = [(3, 5, 7), (4, 1, 2), (2, 33, 130), (35, 16, 650)]
FACTOR_IDS = ["x".join(map(str, s)) for s in FACTOR_SHAPES]
# (T, B, V, H) of the embedding entries: odd widths, a width over two column rounds, the widest the kernels take
EMBED_SHAPES = [(5, 2, 9, 30), (3, 2, 7, 33), (11, 3, 50, 652), (4, 1, 5, 1024)]
EMBED_IDS = ["x".join(map(str, s)) for s in EMBED_SHAPES]
LAYER_CASES = [(3, 2), (6, 21), (17, 4)]          # (B, T) of one row-block layer at H = 650; B = 17: a second row block, a partial one
WAVE_CASES = [(2, 6, 5, 32, 8, 8), (3, 9, 7, 100, 16, 16), (2, 5, 1, 64, 8, 16)]      # (L, B, T, H, w_rank, u_rank): test_dropout.py's
ACTREG_T = (1, 3, 4, 5, 9)            # the four-step walk of the AR / TAR kernels and its halo
ACTREG_H = (5, 650)
MODEL_SHAPES = [(32, 6, 5), (650, 20, 4)]         # (H, B, T): the step-wise layers / the row-block layers


def locked_site(site):
    return int(site) | SITE_LOCKED


def locked_mask(seed, offset, site, B, H, p, Hg=None, gstride=0):
    """The (B, H) float32 factors of a site's locked dropout: the restatement at position b."""
    if p == 0:
        return np.ones((B, H), np.float32)
    return O.dropout_factors(seed, offset, locked_site(site), B, H, p, Hg=Hg, gstride=gstride)


def locked_factors(seed, offset, site, T, B, H, p, Hg=None, gstride=0):
    """... as the (T, B, H) tensor a CPU restatement multiplies by."""
    return np.ascontiguousarray(np.broadcast_to(locked_mask(seed, offset, site, B, H, p, Hg, gstride)[None], (T, B, H)))


def rate_bound(p, n):
    """Five standard deviations of the observed drop rate over n independent draws."""
    return 5.0 * np.sqrt(p * (1.0 - p) / n)


def repeating_tokens(T, B, V, seed=0):
    """(T, B) int64 tokens in which one word stands at every time step of batch row 0 (the same word under the same row mask) and in
    every batch row of time step 0 (the same word under different row masks); the rest random, the last word of the vocabulary among
    them."""
    r = np.random.Generator(np.random.PCG64(2000 + seed))
    tok = r.integers(0, V, size=(T, B)).astype(np.int64)
    tok[:, 0] = V // 2
    tok[0, :] = V // 2
    tok[-1, -1] = V - 1
    return tok


def zero_pattern_is_locked(y):
    """Does the zero pattern of activations y (T, B, H) not depend on t?"""
    z = np.asarray(y) == 0
    return bool((z == z[:1]).all())
