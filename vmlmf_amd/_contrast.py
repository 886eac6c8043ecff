"""ctypes binding of the C ABI in include/vmlmf_contrast.h (libvmlmf_contrast.so, built in-tree by csrc/Makefile beside
libvmlmf_hip.so): the step of contrastive search of the LM decoder - Model.contrastive_search.  The library is loaded on the first
launch: generate(), beam_search(), group_beam_search(), score() and a training process never open it, nor does building the controls.

There is no fallback: if the library is missing, or a call fails, this raises.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from ._lib import ptr

ABI_VERSION = 1
MAX_K = 16            # VMLMF_CONTRAST_MAX_K
MAX_PARTS = 64        # VMLMF_CONTRAST_MAX_PARTS
LDS_FLOATS = 14336    # VMLMF_CONTRAST_LDS_FLOATS

# every symbol include/vmlmf_contrast.h declares: (restype, argtypes)
_vp, _sz, _i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
SYMBOLS = {
    "vmlmf_contrast_abi_version": (_i, []),
    "vmlmf_contrast_last_error": (ctypes.c_char_p, []),
    "vmlmf_contrast_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "vmlmf_contrast_append": (_i, [_i, _i, _i, _vp, _vp, _vp, _i, _vp]),
    "vmlmf_contrast_choose": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, ctypes.c_float, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                   _vp, _sz, _i, _vp]),
}

LIBRARY = _lib.Library("contrast", SYMBOLS, ABI_VERSION, "stock-op fallback for the contrastive-search step")
lib, loaded, check = LIBRARY.handle, LIBRARY.loaded, LIBRARY.check


def check_contrast(top_k, penalty_alpha, V=None, H=None):
    """(k, alpha) as the C ABI takes them; ValueError for top_k outside [1, min(16, V)], for a penalty_alpha outside [0, 1] or not
    finite and for an H whose k unit candidates do not fit the kernel's LDS budget (k * 4 * ceil(H / 4) > 14336 floats)."""
    k = int(top_k)
    hi = MAX_K if V is None else min(MAX_K, int(V))
    if not 1 <= k <= hi:
        raise ValueError(f"vmlmf_amd: top_k must lie in [1, min({MAX_K}, V)] = [1, {hi}], got {top_k}")
    alpha = float(penalty_alpha)
    if not (math.isfinite(alpha) and 0.0 <= alpha <= 1.0):
        raise ValueError(f"vmlmf_amd: penalty_alpha must lie in [0, 1], got {penalty_alpha}")
    if H is not None and k * 4 * ((int(H) + 3) // 4) > LDS_FLOATS:
        raise ValueError(f"vmlmf_amd: top_k={k} candidates of hidden size {H} exceed the contrastive step's LDS budget "
                         f"(top_k * 4 * ceil(H / 4) <= {LDS_FLOATS} floats)")
    return k, alpha


def workspace_bytes(B):
    """vmlmf_contrast_workspace_bytes without opening the library: MAX_PARTS workgroups' MAX_K partial maxima per row."""
    return int(B) * MAX_PARTS * MAX_K * 4


class ContrastControls:
    """What one contrastive search over B rows carries from step to step on `device` (include/vmlmf_contrast.h): hist (B, capacity, H)
    fp32 - the unit vectors of the top layer's outputs behind every token of a row so far -, hist_len (B) int32 - on the device, so
    that a captured step stays valid as the history grows -, finished and length (B) int32, k = top_k, alpha = penalty_alpha, eos
    (-1: none) and the step's buffers (ticket, workspace).  append(h) takes in h (T, B, H) - how the prompt enters -;
    lm_contrast_step moves everything on in place.  capacity must cover the prompt and every step.  Building it opens no library.
    ValueError for what check_contrast refuses, capacity < 1 and an eos outside [0, V)."""

    def __init__(self, B, H, device, capacity, top_k=4, penalty_alpha=0.6, eos=None, V=None):
        self.B, self.H, self.capacity = int(B), int(H), int(capacity)
        self.k, self.alpha = check_contrast(top_k, penalty_alpha, V, self.H)
        if self.B < 1 or self.capacity < 1:
            raise ValueError(f"vmlmf_amd: ContrastControls needs B >= 1 and capacity >= 1, got {B} and {capacity}")
        self.eos = -1 if eos is None else int(eos)
        if eos is not None and not (0 <= self.eos and (V is None or self.eos < int(V))):
            raise ValueError(f"vmlmf_amd: eos={eos} is not a token of the vocabulary ({V})")
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.hist = torch.empty((self.B, self.capacity, self.H), device=dev, dtype=torch.float32)
        self.hist_len = torch.zeros(self.B, device=dev, dtype=torch.int32)
        self.finished = torch.zeros(self.B, device=dev, dtype=torch.int32)
        self.length = torch.zeros(self.B, device=dev, dtype=torch.int32)
        self.ticket = torch.zeros(self.B, device=dev, dtype=torch.int32)
        self.workspace = torch.empty(workspace_bytes(self.B) // 4, device=dev, dtype=torch.float32)

    def append(self, h):
        """The rows h (T, B, H) behind every row's history, as unit vectors (vmlmf_contrast_append)."""
        contrast_append(h, self)

    def clone(self):
        """A copy with buffers of its own (a ContrastGraph's warm-up runs on one)."""
        c = object.__new__(ContrastControls)
        c.__dict__.update(self.__dict__)
        for name in ("hist", "hist_len", "finished", "length"):
            setattr(c, name, getattr(self, name).clone())
        c.ticket, c.workspace = torch.zeros_like(self.ticket), torch.empty_like(self.workspace)
        return c


def _require(t, what, dtype=torch.float32):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f"vmlmf_amd: {what} is not on a HIP device; the contrastive-search step runs only as HIP kernels on an "
                           "MI355X (no CPU fallback). Move the model and inputs to 'cuda'.")
    if t.dtype != dtype:
        raise RuntimeError(f"vmlmf_amd: {what} must be {dtype}, got {t.dtype}")


def contrast_append(h, controls):
    """vmlmf_contrast_append: h (T, B, H) fp32 behind the histories of `controls`."""
    _require(h, "h")
    c = controls
    if h.dim() != 3 or tuple(h.shape[1:]) != (c.B, c.H) or h.device != c.device:
        raise RuntimeError(f"vmlmf_amd.contrast_append: h must be (T, {c.B}, {c.H}) on {c.device}, got {tuple(h.shape)} on {h.device}")
    if h.shape[0] == 0:
        return
    h = h.contiguous()
    LIBRARY.call(c.device, "vmlmf_contrast_append", c.B, h.shape[0], c.H, ptr(h), ptr(c.hist), ptr(c.hist_len), c.capacity)


def lm_contrast_step(cand_h, cand_tok, cand_logp, controls, parts=0):
    """One step of contrastive search in ONE launch (vmlmf_contrast_choose, csrc/vmlmf_contrast.hip; include/vmlmf_contrast.h has the
    contract): cand_h (B k, H) - the top layer's output behind candidate j of row b at row b k + j -, cand_tok (B, k) int64 and
    cand_logp (B, k) the candidates' tokens and log-probabilities.  Per live row: sim[j] = the largest cosine of candidate j with the
    row's history, j* = argmax_j (1 - alpha) exp(cand_logp[j]) - alpha sim[j] (equal values to the lower j, a NaN loses); the unit
    vector of cand_h[j*] goes behind the row's history and hist_len, finished and length of `controls` move on in place.  A finished
    row gives (eos, 0.0, chosen 0) and keeps its history.
    Returns (token (B) int64, logprob (B), chosen (B) int32, sim (B, k), h_next (B, H) = cand_h[b k + j*], src_row (B k) int32 =
    b k + j*: the state row every candidate row of the block continues - beam_gather's argument).
    parts: how many workgroups share a row's history (0: automatic); the results are the same bits for every value."""
    c = controls
    if not isinstance(c, ContrastControls):
        raise RuntimeError(f"vmlmf_amd.lm_contrast_step: controls must be a ContrastControls, got {type(c).__name__}")
    _require(cand_h, "cand_h")
    _require(cand_tok, "cand_tok", torch.int64)
    _require(cand_logp, "cand_logp")
    B, k, H = c.B, c.k, c.H
    if tuple(cand_h.shape) != (B * k, H) or tuple(cand_tok.shape) != (B, k) or tuple(cand_logp.shape) != (B, k) or cand_h.device != c.device:
        raise RuntimeError(f"vmlmf_amd.lm_contrast_step: cand_h must be ({B * k}, {H}), cand_tok and cand_logp ({B}, {k}) on {c.device}")
    if not 0 <= int(parts) <= MAX_PARTS:
        raise ValueError(f"vmlmf_amd.lm_contrast_step: parts must lie in [0, {MAX_PARTS}] (0: automatic), got {parts}")
    dev = c.device
    cand_h, cand_tok, cand_logp = cand_h.contiguous(), cand_tok.contiguous(), cand_logp.contiguous()
    token = torch.empty(B, device=dev, dtype=torch.int64)
    logprob = torch.empty(B, device=dev, dtype=torch.float32)
    chosen = torch.empty(B, device=dev, dtype=torch.int32)
    sim = torch.empty((B, k), device=dev, dtype=torch.float32)
    h_next = torch.empty((B, H), device=dev, dtype=torch.float32)
    src = torch.empty(B * k, device=dev, dtype=torch.int32)
    LIBRARY.call(dev, "vmlmf_contrast_choose", B, k, H, c.capacity, ptr(cand_h), ptr(cand_tok), ptr(cand_logp), c.alpha, c.eos, ptr(c.hist),
                 ptr(c.hist_len), ptr(c.finished), ptr(c.length), ptr(token), ptr(logprob), ptr(chosen), ptr(sim), ptr(h_next), ptr(src),
                 ptr(c.ticket), ptr(c.workspace), c.workspace.numel() * 4, int(parts))
    return token, logprob, chosen, sim, h_next, src
