"""ctypes binding of the C ABI in include/vmlmf_decode.h (libvmlmf_decode.so, built in-tree by csrc/Makefile beside libvmlmf_hip.so):
the controlled choice of the LM decoder - eos, minimum length, repetition penalty, logit bias and bans of Model.generate.  The library
is loaded on the first controlled call: a plain generate(), and a training process, never open it.

There is no fallback: if the library is missing, or a call fails, this raises.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from ._lib import ptr

ABI_VERSION = 1


class Controls(ctypes.Structure):
    """struct vmlmf_decode_controls"""
    _fields_ = [("repetition_penalty", ctypes.c_float), ("eos", ctypes.c_int32), ("min_length", ctypes.c_int32), ("pad", ctypes.c_int32),
                ("logit_bias", ctypes.c_void_p), ("seen", ctypes.c_void_p), ("finished", ctypes.c_void_p), ("length", ctypes.c_void_p)]


# every symbol include/vmlmf_decode.h declares: (restype, argtypes)
_vp, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
SYMBOLS = {
    "vmlmf_decode_abi_version": (_i, []),
    "vmlmf_decode_last_error": (ctypes.c_char_p, []),
    "vmlmf_decode_choose": (_i, [_i, _i, _i, _vp, _vp, _vp, _f, _i, _f, _vp, _i, ctypes.POINTER(Controls), _vp, _vp, _vp, _vp, _vp]),
}

LIBRARY = _lib.Library("decode", SYMBOLS, ABI_VERSION, "stock-op fallback for the controlled choice of Model.generate")
lib, loaded, check = LIBRARY.handle, LIBRARY.loaded, LIBRARY.check


def controls_on(eos=None, repetition_penalty=1.0, logit_bias=None, banned_tokens=None):
    """Whether these arguments of Model.generate ask for the controlled launch (min_length alone does not: it needs eos)."""
    return eos is not None or repetition_penalty != 1.0 or logit_bias is not None or banned_tokens is not None


def check_controls(V, eos=None, min_length=0, repetition_penalty=1.0, logit_bias=None, banned_tokens=None):
    """The arguments as the C ABI takes them: (eos or -1, min_length, theta, banned indices).  ValueError for everything the contract
    refuses that can be told without looking at logit_bias's values (check_bias does that)."""
    try:
        theta = float(repetition_penalty)
    except (TypeError, ValueError):
        raise ValueError(f"vmlmf_amd: repetition_penalty must be a finite number > 0, got {repetition_penalty!r}") from None
    if not (theta > 0.0 and math.isfinite(theta)):
        raise ValueError(f"vmlmf_amd: repetition_penalty must be finite and > 0 (1: off), got {repetition_penalty}")
    n = int(min_length)
    if n < 0:
        raise ValueError(f"vmlmf_amd: min_length must be >= 0, got {min_length}")
    if n > 0 and eos is None:
        raise ValueError(f"vmlmf_amd: min_length={min_length} needs eos (the token it holds back)")
    e = -1 if eos is None else int(eos)
    if eos is not None and not 0 <= e < V:
        raise ValueError(f"vmlmf_amd: eos={eos} is not a token of the vocabulary ({V})")
    banned = [] if banned_tokens is None else [int(t) for t in banned_tokens]
    for t in banned:
        if not 0 <= t < V:
            raise ValueError(f"vmlmf_amd: banned token {t} is not a token of the vocabulary ({V})")
    if logit_bias is not None:
        if not (isinstance(logit_bias, torch.Tensor) and logit_bias.dtype == torch.float32 and tuple(logit_bias.shape) == (V,)):
            raise ValueError(f"vmlmf_amd: logit_bias must be a ({V},) float32 tensor (one entry per token, shared by the rows)")
    return e, n, theta, banned


def check_bias(V, logit_bias, banned, eos, min_length):
    """ValueError for a NaN or +inf in logit_bias, and for a bias (bans included) that leaves nothing to choose: no finite token at
    all, or - while eos is held back by min_length - none besides eos.  Reads the tensor back once.  Returns how many tokens are closed
    (eos, while min_length holds it back, among them)."""
    if logit_bias is None:
        open_ = torch.ones(V, dtype=torch.bool)
    else:
        lb = logit_bias.detach().to("cpu")
        if bool(torch.isnan(lb).any()) or bool((lb == float("inf")).any()):
            raise ValueError("vmlmf_amd: logit_bias entries must be finite or -inf (a ban): found NaN or +inf")
        open_ = lb != float("-inf")
    if banned:
        open_[torch.tensor(banned, dtype=torch.int64)] = False
    if not bool(open_.any()):
        raise ValueError("vmlmf_amd: logit_bias / banned_tokens leave no token to choose")
    if min_length > 0 and eos >= 0:
        open_[eos] = False
        if not bool(open_.any()):
            raise ValueError("vmlmf_amd: logit_bias / banned_tokens leave no token besides eos, which min_length holds back")
    return V - int(open_.sum())


class DecodeControls:
    """The controls of one decode over B rows of a V-token vocabulary and their per-row state on `device` (include/vmlmf_decode.h):
      eos                  a row that emits it is finished: its later tokens are eos, with log-probability 0
      min_length           eos cannot be chosen before a row has emitted this many tokens (needs eos)
      repetition_penalty   theta > 0: the score x of a token the row has held becomes x / theta (x > 0) or x theta (Keskar et al., CTRL)
      logit_bias           (V) fp32 added to every row's scores, entries finite or -inf; banned_tokens: indices, shorthand for -inf
      prompt               (T0, B) int64: the rows' tokens so far - `seen` starts as their set (stock ops, once)
    Owns seen (B, V) uint8, finished (B) int32, length (B) int32; every controlled lm_sample launch updates them in place, so one
    object is one decode: make a new one (or clone()) for another.  ValueError for whatever the contract refuses - all of it before any
    device work, except that logit_bias's values are read back once."""

    def __init__(self, B, V, device, eos=None, min_length=0, repetition_penalty=1.0, logit_bias=None, banned_tokens=None, prompt=None,
                 _checked=False):
        B, V = int(B), int(V)
        self.eos, self.min_length, self.repetition_penalty, banned = check_controls(V, eos, min_length, repetition_penalty, logit_bias,
                                                                                    banned_tokens)
        if prompt is not None and not (isinstance(prompt, torch.Tensor) and prompt.dtype == torch.int64 and prompt.dim() == 2
                                       and prompt.shape[1] == B):
            raise ValueError(f"vmlmf_amd: DecodeControls takes a (T0, {B}) int64 prompt")
        if not _checked:    # (Model.generate has: it refuses before anything else, and reads logit_bias back once)
            check_bias(V, logit_bias, banned, self.eos, self.min_length)
        self.B, self.V, self.device = B, V, torch.device(device)
        if logit_bias is None and not banned:
            self.logit_bias = None
        else:
            lb = torch.zeros(V, dtype=torch.float32) if logit_bias is None else logit_bias.detach().to("cpu", copy=True)
            if banned:
                lb[torch.tensor(banned, dtype=torch.int64)] = float("-inf")
            self.logit_bias = lb.to(self.device).contiguous()
        self.seen = torch.zeros((B, V), dtype=torch.uint8, device=self.device)
        if prompt is not None and prompt.shape[0] > 0:
            self.seen.scatter_(1, prompt.to(self.device).t().clamp(0, V - 1).contiguous(), 1)   # (clamped: never a store outside the row)
        self.finished = torch.zeros(B, dtype=torch.int32, device=self.device)
        self.length = torch.zeros(B, dtype=torch.int32, device=self.device)

    STATE = ("seen", "finished", "length")                                  # the buffers a launch moves on: what clone() copies
    LIBRARY, ENTRY, STRUCT = LIBRARY, "vmlmf_decode_choose", Controls       # where decode_choose goes with these controls
    TRUNCATION_REFUSAL = None       # a subclass whose choice cannot run under a Truncation: lm_sample's ValueError for the two together

    def clone(self):
        """The same controls on a copy of ALL the state (a DecodeGraph's warm-up runs on one)."""
        c = object.__new__(type(self))
        c.__dict__.update(self.__dict__)
        for name in self.STATE:
            setattr(c, name, getattr(self, name).clone())
        return c

    def values(self):       # STRUCT's fields by name; the pointers are this object's buffers
        return dict(repetition_penalty=self.repetition_penalty, eos=self.eos, min_length=self.min_length, logit_bias=ptr(self.logit_bias),
                    seen=ptr(self.seen), finished=ptr(self.finished), length=ptr(self.length))

    def struct(self):       # the host struct ENTRY reads
        return self.STRUCT(**self.values())


def check_launch(controls, kind, B, V, dev, what):
    """RuntimeError unless `controls` is a `kind` for B rows of V tokens on dev - and the history, where it keeps one, (B, capacity)."""
    if not isinstance(controls, kind) or (controls.B, controls.V) != (B, V) or controls.seen.device != dev:
        raise RuntimeError(f"vmlmf_amd.{what}: controls must be a {kind.__name__} for {B} rows of {V} tokens on {dev}")
    if "hist" in controls.STATE and (tuple(controls.hist.shape) != (B, controls.capacity) or not controls.hist.is_contiguous()):
        raise RuntimeError(f"vmlmf_amd.{what}: controls.hist must be a contiguous ({B}, capacity = {controls.capacity}) tensor")


def decode_choose(scores, bias, embed, inv, top_k, top_p, state, step, controls, tokens, logp, xn, kept, kind=DecodeControls):
    """The launch of the controls' ENTRY on checked, contiguous arguments: scores (B, V) without the bias; outputs are written in place."""
    B, V = scores.shape
    dev = scores.device
    check_launch(controls, kind, B, V, dev, "lm_sample")
    H = embed.shape[1] if embed is not None else 1
    c = controls.struct()
    controls.LIBRARY.call(dev, controls.ENTRY, B, H, V, ptr(scores), ptr(bias), ptr(embed), inv, top_k, top_p, ptr(state), int(step),
                          ctypes.byref(c), ptr(tokens), ptr(logp), ptr(xn), ptr(kept))
