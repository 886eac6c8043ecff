"""ctypes binding of the C ABI in include/vmlmf_truncate.h (libvmlmf_truncate.so, built in-tree by csrc/Makefile beside
libvmlmf_hip.so): the truncation samplers of the LM decoder - min_p, typical_p, epsilon_cutoff and eta_cutoff of Model.generate.  The
library is loaded on the first truncated call: every other generate(), and a training process, never open it.

There is no fallback: if the library is missing, or a call fails, this raises.
"""
from __future__ import annotations

import ctypes
import math

from . import _decode, _lib
from ._lib import ptr

ABI_VERSION = 1


class TruncationStruct(ctypes.Structure):
    """struct vmlmf_truncation"""
    _fields_ = [("min_p", ctypes.c_float), ("typical_p", ctypes.c_float), ("epsilon_cutoff", ctypes.c_float), ("eta_cutoff", ctypes.c_float)]


# every symbol include/vmlmf_truncate.h declares: (restype, argtypes)
_vp, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
SYMBOLS = {
    "vmlmf_truncate_abi_version": (_i, []),
    "vmlmf_truncate_last_error": (ctypes.c_char_p, []),
    "vmlmf_truncate_choose": (_i, [_i, _i, _i, _vp, _vp, _vp, _f, _i, _f, ctypes.POINTER(TruncationStruct), _vp, _i,
                                   ctypes.POINTER(_decode.Controls), _vp, _vp, _vp, _vp, _vp]),
}

LIBRARY = _lib.Library("truncate", SYMBOLS, ABI_VERSION, "stock-op fallback for the truncation samplers of Model.generate")
lib, loaded, check = LIBRARY.handle, LIBRARY.loaded, LIBRARY.check

HISTORY_REFUSAL = ("vmlmf_amd: min_p / typical_p / epsilon_cutoff / eta_cutoff together with the history controls (no_repeat_ngram_size, "
                   "banned_sequences, frequency_penalty, presence_penalty) is out of scope: the truncated choice runs under the "
                   "stopping and token controls (eos, min_length, repetition_penalty, logit_bias, banned_tokens) only")


def _number(name, value, lo, hi, lo_open, hi_open, off):
    """`value` as a float inside the interval, None as `off`; ValueError otherwise."""
    if value is None:
        return off
    try:
        x = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"vmlmf_amd: {name} must be a number, got {value!r}") from None
    inside = (x > lo if lo_open else x >= lo) and (x < hi if hi_open else x <= hi)
    if not (math.isfinite(x) and inside):
        rng = f"{'(' if lo_open else '['}{lo:g}, {hi:g}{')' if hi_open else ']'}"
        raise ValueError(f"vmlmf_amd: {name} must lie in {rng} (None / {off:g}: off), got {value}")
    return x


class Truncation:
    """The four truncation samplers of Model.generate as one checked value (include/vmlmf_truncate.h has the contract):
      min_p            a in (0, 1]: keep the tokens with p >= a p_max                                   (None / 0: off)
      typical_p        m in (0, 1): locally typical sampling - the tokens nearest the entropy, mass m   (None / 1: off)
      epsilon_cutoff   in (0, 1): keep the tokens with p >= epsilon                                     (None / 0: off)
      eta_cutoff       in (0, 1): keep the tokens with p >= min(eta, sqrt(eta) exp(-entropy))           (None / 0: off)
    `.on`: whether any of them is.  ValueError for a value outside its range.  Building one touches no device and opens no library."""

    __slots__ = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")

    def __init__(self, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None):
        self.min_p = _number("min_p", min_p, 0.0, 1.0, False, False, 0.0)
        self.typical_p = _number("typical_p", typical_p, 0.0, 1.0, True, False, 1.0)
        self.epsilon_cutoff = _number("epsilon_cutoff", epsilon_cutoff, 0.0, 1.0, False, True, 0.0)
        self.eta_cutoff = _number("eta_cutoff", eta_cutoff, 0.0, 1.0, False, True, 0.0)

    @property
    def on(self):
        return self.min_p > 0.0 or self.typical_p < 1.0 or self.epsilon_cutoff > 0.0 or self.eta_cutoff > 0.0

    def struct(self):
        return TruncationStruct(self.min_p, self.typical_p, self.epsilon_cutoff, self.eta_cutoff)

    def __repr__(self):
        return (f"Truncation(min_p={self.min_p}, typical_p={self.typical_p}, epsilon_cutoff={self.epsilon_cutoff}, "
                f"eta_cutoff={self.eta_cutoff})")


def truncation(min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None, history=False):
    """The keywords of Model.generate as a Truncation, or None where none of them is on.  ValueError for a value outside its range,
    and for any of them on together with the history controls."""
    t = Truncation(min_p, typical_p, epsilon_cutoff, eta_cutoff)
    if t.on and history:
        raise ValueError(HISTORY_REFUSAL)
    return t if t.on else None


def truncate_choose(scores, bias, embed, inv, top_k, top_p, trunc, state, step, controls, tokens, logp, xn, kept):
    """The launch of vmlmf_truncate_choose on checked, contiguous arguments: scores (B, V) without the bias; controls: a DecodeControls
    whose class takes a truncation (TRUNCATION_REFUSAL), or None; outputs (and the controls' state) are written in place."""
    B, V = scores.shape
    dev = scores.device
    c = None
    if controls is not None:
        _decode.check_launch(controls, _decode.DecodeControls, B, V, dev, "lm_sample")
        if controls.TRUNCATION_REFUSAL is not None:
            raise ValueError(controls.TRUNCATION_REFUSAL)
        held = controls.struct()
        c = ctypes.byref(held)
    H = embed.shape[1] if embed is not None else 1
    t = trunc.struct()
    LIBRARY.call(dev, "vmlmf_truncate_choose", B, H, V, ptr(scores), ptr(bias), ptr(embed), inv, top_k, top_p, ctypes.byref(t), ptr(state),
                 int(step), c, ptr(tokens), ptr(logp), ptr(xn), ptr(kept))
