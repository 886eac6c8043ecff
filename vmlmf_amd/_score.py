"""ctypes binding of the C ABI in include/vmlmf_score.h (libvmlmf_score.so, built in-tree by csrc/Makefile beside libvmlmf_hip.so):
scoring given text - a target token's log-probability and rank per row of scores, and the row's most probable tokens (Model.score,
lm_score; scoring.py).  The library is loaded on the first scoring call: a training or a generating process never opens it.

There is no fallback: if the library is missing, or a call fails, this raises.
"""
from __future__ import annotations

import ctypes

from . import _lib
from ._lib import ptr

ABI_VERSION = 1
MAX_TOP = 32    # VMLMF_SCORE_MAX_TOP

# every symbol include/vmlmf_score.h declares: (restype, argtypes)
_vp, _i = ctypes.c_void_p, ctypes.c_int
SYMBOLS = {
    "vmlmf_score_abi_version": (_i, []),
    "vmlmf_score_last_error": (ctypes.c_char_p, []),
    "vmlmf_score_rows": (_i, [_i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
}

LIBRARY = _lib.Library("score", SYMBOLS, ABI_VERSION, "stock-op fallback for Model.score")
lib, loaded, check = LIBRARY.handle, LIBRARY.loaded, LIBRARY.check


def check_top(top, V, who="lm_score"):
    """`top` as the C ABI takes it.  ValueError outside [0, min(32, V)]."""
    k = int(top)
    if not 0 <= k <= min(MAX_TOP, V):
        raise ValueError(f"vmlmf_amd.{who}: top must lie in [0, min({MAX_TOP}, V = {V})], got {top}")
    return k


def score_rows(scores, bias, targets, top, logprob, rank, top_tokens, top_logprob):
    """The vmlmf_score_rows launch on checked, contiguous arguments: scores (R, V) without the bias; outputs are written in place."""
    R, V = scores.shape
    LIBRARY.call(scores.device, "vmlmf_score_rows", R, V, ptr(scores), ptr(bias), ptr(targets), int(top), ptr(logprob), ptr(rank),
                 ptr(top_tokens), ptr(top_logprob))
