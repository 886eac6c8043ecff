"""ctypes binding of the C ABI in include/vmlmf_ncache.h (libvmlmf_ncache.so, built in-tree by csrc/Makefile beside
libvmlmf_hip.so): scoring a text under the language model mixed with a continuous cache - Model.cache_score.  The library is loaded
on the first launch: generate(), beam_search(), score(), contrastive_search() and a training process never open it, nor does building
a NeuralCache.

There is no fallback: if the library is missing, or a call fails, this raises.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from ._lib import ptr

ABI_VERSION = 1
MAX_H = 2048          # VMLMF_NCACHE_MAX_H
MAX_PARTS = 64        # VMLMF_NCACHE_MAX_PARTS
TILE = 16             # queries of a workgroup, keys of a key tile

# every symbol include/vmlmf_ncache.h declares: (restype, argtypes)
_vp, _sz, _i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
SYMBOLS = {
    "vmlmf_ncache_abi_version": (_i, []),
    "vmlmf_ncache_last_error": (ctypes.c_char_p, []),
    "vmlmf_ncache_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "vmlmf_ncache_score": (_i, [_i, _i, _i, _i, _i, ctypes.c_float, ctypes.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _vp]),
}

LIBRARY = _lib.Library("ncache", SYMBOLS, ABI_VERSION, "stock-op fallback for the continuous-cache scoring")
lib, loaded, check = LIBRARY.handle, LIBRARY.loaded, LIBRARY.check


def check_ncache(window, theta, lam, H=None):
    """(window, theta, lam) as the C ABI takes them; ValueError for a window < 1, a theta that is not finite, a lam outside [0, 1) or
    NaN and an H outside [1, 2048] (a tile of 16 queries waits in the kernel's LDS)."""
    w = int(window)
    if w < 1 or w != window:
        raise ValueError(f"vmlmf_amd: window must be an integer >= 1, got {window}")
    th = float(theta)
    if not math.isfinite(th):
        raise ValueError(f"vmlmf_amd: theta must be finite, got {theta}")
    la = float(lam)
    if not 0.0 <= la < 1.0:
        raise ValueError(f"vmlmf_amd: lam must lie in [0, 1), got {lam}")
    if H is not None and not 1 <= int(H) <= MAX_H:
        raise ValueError(f"vmlmf_amd: hidden size {H} is outside the cache-scoring kernel's [1, {MAX_H}] (16 queries wait in LDS)")
    return w, th, la


def workspace_bytes(B, T, n, window):
    """vmlmf_ncache_workspace_bytes without opening the library: per tile of 16 queries and per tile of 16 keys of the union of its
    bands - min(window + 15, n + T) keys, rounded up to whole key tiles - three numbers per query."""
    width = -(-min(int(window) + TILE - 1, int(n) + int(T)) // TILE) * TILE
    return int(B) * -(-int(T) // TILE) * 3 * width * 4


class NeuralCache:
    """What a continuous cache over B rows carries from call to call on `device` (include/vmlmf_ncache.h): keys (B, n, H) fp32 - the
    top layer's outputs behind the last n tokens of a row, oldest first -, toks (B, n) int64 - the token that followed each - and the
    count n <= window, the same for every row.  lm_cache_score moves it on in place: a call over T positions forms ONE (B, n + T, H)
    buffer from the carried keys and the call's outputs, and the cache keeps that buffer's last min(window, n + T) rows.  Building it
    opens no library and works on the CPU.  ValueError for B, H or window < 1 and an H beyond the kernel's limit."""

    def __init__(self, B, H, device, window=500):
        self.B, self.H = int(B), int(H)
        if self.B < 1 or self.H < 1:
            raise ValueError(f"vmlmf_amd: NeuralCache needs B >= 1 and H >= 1, got {B} and {H}")
        self.window = check_ncache(window, 0.0, 0.0, self.H)[0]
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self._ticket = self._workspace = None
        self.reset()

    @property
    def n(self):
        return self.keys.shape[1]

    def reset(self):
        """Forget every pair."""
        self.keys = torch.empty((self.B, 0, self.H), device=self.device, dtype=torch.float32)
        self.toks = torch.empty((self.B, 0), device=self.device, dtype=torch.int64)

    def clone(self):
        """A copy with buffers of its own."""
        c = object.__new__(NeuralCache)
        c.__dict__.update(self.__dict__)
        c.keys, c.toks = self.keys.clone(), self.toks.clone()
        c._ticket = c._workspace = None
        return c

    def extended(self, h, targets):
        """(keys (B, n + T, H), toks (B, n + T)): the carried pairs and, behind them, those of h (T, B, H) and targets (T, B) - the one
        copy a call makes."""
        return torch.cat([self.keys, h.transpose(0, 1)], dim=1), torch.cat([self.toks, targets.t()], dim=1)

    def keep(self, keys, toks):
        """Carry the last min(window, L) pairs of the buffers extended() returned (views of them: no second copy)."""
        lo = max(0, keys.shape[1] - self.window)
        self.keys, self.toks = keys[:, lo:], toks[:, lo:]

    def update(self, h, targets):
        """Take the pairs of h (T, B, H) and targets (T, B) in without scoring them."""
        self.keep(*self.extended(h, targets))

    def buffers(self, T, n):
        """(ticket, workspace) of a launch over T positions behind n pairs: the tickets zero - every launch leaves them so -, both
        grown when a call needs more."""
        tiles = self.B * -(-T // TILE)
        if self._ticket is None or self._ticket.numel() < tiles:
            self._ticket = torch.zeros(tiles, device=self.device, dtype=torch.int32)
        words = workspace_bytes(self.B, T, n, self.window) // 4
        if self._workspace is None or self._workspace.numel() < words:
            self._workspace = torch.empty(words, device=self.device, dtype=torch.float32)
        return self._ticket, self._workspace


def _require(t, what, dtype=torch.float32):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f"vmlmf_amd: {what} is not on a HIP device; the continuous-cache scoring runs only as a HIP kernel on an "
                           "MI355X (no CPU fallback). Move the model and inputs to 'cuda'.")
    if t.dtype != dtype:
        raise RuntimeError(f"vmlmf_amd: {what} must be {dtype}, got {t.dtype}")


def lm_cache_score(h, targets, vocab_logp, cache, theta=0.3, lam=0.1, parts=0):
    """Score T positions per row under the model mixed with a continuous cache in ONE launch (vmlmf_ncache_score,
    csrc/vmlmf_ncache.hip; include/vmlmf_ncache.h has the contract): h (T, B, H) fp32 - the top layer's outputs -, targets (T, B) int64,
    vocab_logp (T, B) fp32 - the vocabulary's log-probability of every target (lm_score's) -, cache a NeuralCache.  Per position, with
    the band of the last m = min(window, pairs so far) pairs (k_j, w_j) strictly before it:
      s_j = theta dot(h[t, b], k_j);  cache_logp = log sum_{j: w_j == target} exp(s_j - M) - log sum_j exp(s_j - M),  M = max_j s_j
      logp = logaddexp(log1p(-lam) + vocab_logp, log(lam) + cache_logp)
    (m == 0 or lam == 0: vocab_logp's bits; no w_j equals the target: cache_logp = -inf, logp = log1p(-lam) + vocab_logp; every w_j
    equals it: cache_logp = 0.0 exactly.)  A position's own pair enters the cache behind it.  Returns (logp, cache_logp), both (T, B),
    and moves `cache` on in place.  parts: how many workgroups share a tile of 16 queries (0: automatic); the results are the same
    bits for every value.  No autograd, no host synchronisation."""
    c = cache
    if not isinstance(c, NeuralCache):
        raise RuntimeError(f"vmlmf_amd.lm_cache_score: cache must be a NeuralCache, got {type(c).__name__}")
    _, theta, lam = check_ncache(c.window, theta, lam, c.H)
    if not 0 <= int(parts) <= MAX_PARTS:
        raise ValueError(f"vmlmf_amd.lm_cache_score: parts must lie in [0, {MAX_PARTS}] (0: automatic), got {parts}")
    _require(h, "h")
    _require(targets, "targets", torch.int64)
    _require(vocab_logp, "vocab_logp")
    B, H = c.B, c.H
    if h.dim() != 3 or tuple(h.shape[1:]) != (B, H) or h.device != c.device:
        raise RuntimeError(f"vmlmf_amd.lm_cache_score: h must be (T, {B}, {H}) on {c.device}, got {tuple(h.shape)} on {h.device}")
    T = h.shape[0]
    if tuple(targets.shape) != (T, B) or tuple(vocab_logp.shape) != (T, B):
        raise RuntimeError(f"vmlmf_amd.lm_cache_score: targets and vocab_logp must be ({T}, {B})")
    dev = c.device
    logp = torch.empty((T, B), device=dev, dtype=torch.float32)
    cache_logp = torch.empty((T, B), device=dev, dtype=torch.float32)
    if T == 0:
        return logp, cache_logp
    with torch.no_grad():
        n = c.n
        keys, toks = c.extended(h.detach(), targets)
        lv = vocab_logp.detach().contiguous()
        ticket, workspace = c.buffers(T, n)
        LIBRARY.call(dev, "vmlmf_ncache_score", B, T, n, H, c.window, theta, lam, ptr(keys), ptr(toks), ptr(lv), ptr(logp), ptr(cache_logp),
                     ptr(ticket), ptr(workspace), workspace.numel() * 4, int(parts))
        c.keep(keys, toks)
    return logp, cache_logp
