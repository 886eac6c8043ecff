"""ctypes binding of the C ABI in include/vmlmf_beamctl.h (libvmlmf_beamctl.so, built in-tree by csrc/Makefile beside libvmlmf_hip.so):
the beam-search step of the LM decoder under controls - min_length, banned_tokens, no_repeat_ngram_size and banned_sequences of
Model.beam_search.  The library is loaded on the first controlled beam call: a plain beam_search(), and a training process, never
open it.  The per-beam n-gram and sequence ban sets come from vmlmf_history_bans (libvmlmf_history.so, _history.py), which is opened
only when one of those two controls is on.

There is no fallback: if the library is missing, or a call fails, this raises.
"""
from __future__ import annotations

import ctypes

import torch

from . import _decode, _history, _lib
from ._beam import BeamPolicy, check_step_controls, launch_step
from ._lib import ptr

ABI_VERSION = 1


class Controls(ctypes.Structure):
    """struct vmlmf_beamctl_controls"""
    _fields_ = [("min_length", ctypes.c_int32), ("hist_capacity", ctypes.c_int32), ("closed", ctypes.c_void_p), ("bans", ctypes.c_void_p),
                ("hist", ctypes.c_void_p), ("hist_len", ctypes.c_void_p), ("hist_out", ctypes.c_void_p), ("hist_len_out", ctypes.c_void_p),
                ("overflow", ctypes.c_void_p)]


# every symbol include/vmlmf_beamctl.h declares: (restype, argtypes)
_vp, _sz, _i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
SYMBOLS = {
    "vmlmf_beamctl_abi_version": (_i, []),
    "vmlmf_beamctl_last_error": (ctypes.c_char_p, []),
    "vmlmf_beamctl_workspace_bytes": (_sz, [_i, _i, _i]),
    "vmlmf_beamctl_step": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, ctypes.POINTER(Controls), _vp, _vp, _vp, _vp, _vp, _vp,
                                _vp, _vp, _vp, _sz, _vp]),
}

LIBRARY = _lib.Library("beamctl", SYMBOLS, ABI_VERSION, "stock-op fallback for the controlled beam-search step")
lib, loaded, check = LIBRARY.handle, LIBRARY.loaded, LIBRARY.check


def controls_on(min_length=0, banned_tokens=None, no_repeat_ngram_size=0, banned_sequences=None):
    """Whether these arguments of Model.beam_search ask for the controlled step."""
    return min_length != 0 or banned_tokens is not None or no_repeat_ngram_size != 0 or banned_sequences is not None


def check_beam_controls(V, W, eos=None, min_length=0, banned_tokens=None, no_repeat_ngram_size=0, banned_sequences=None, prompt_length=0,
                        steps=None):
    """The arguments as the C ABI takes them: (eos or -1, min_length, banned indices, n, sequences as lists of ints).  ValueError for
    whatever _decode.check_controls and _history.check_history refuse for the same arguments (min_length > 0 without eos among them),
    for eos among banned_tokens (a finished beam must be able to offer it), and - `steps` given: a search of that many steps - for a
    vocabulary in which a live beam might run short of W candidates: V < closed + prompt_length + steps + len(sequences) + W, where
    `closed` counts banned_tokens and, under min_length, eos.  (A beam's ban set holds at most one token per sequence and at most as
    many n-gram tokens as it has history: a sufficient condition, stated once for every combination of the controls.)"""
    e, n_min, _, banned = _decode.check_controls(V, eos=eos, min_length=min_length, banned_tokens=banned_tokens)
    if e >= 0 and e in banned:
        raise ValueError(f"vmlmf_amd: eos={e} is among banned_tokens: a finished beam offers eos alone")
    closed = _decode.check_bias(V, None, banned, e, n_min)
    n, seqs, _, _ = _history.check_history(V, no_repeat_ngram_size, banned_sequences)
    if steps is not None:
        need = closed + int(prompt_length) + int(steps) + len(seqs) + int(W)
        if V < need:
            raise ValueError(f"vmlmf_amd: the beam controls might leave a beam fewer than {W} candidates: the vocabulary ({V}) must hold "
                             f"bans + prompt + steps + sequences + beams = {need}")
    return e, n_min, banned, n, seqs


def pack_words(tokens, V):
    """The tokens as a ban set of ceil(V / 32) 32-bit words (bit v & 31 of word v >> 5: vmlmf_history_bans' layout), an int32 CPU tensor."""
    words = [0] * ((V + 31) // 32)
    for t in tokens:
        words[t >> 5] |= 1 << (t & 31)
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32)


class BeamControls(BeamPolicy):
    """The controls of one beam search over B batch rows of W beams and a V-token vocabulary on `device` (include/vmlmf_beamctl.h).
    They only close candidates - a candidate is offered or it is not -, so `scores` stay sums of plain log-probabilities:
      eos                    the token that finishes a beam (the search's own eos, needed by min_length)
      min_length             a live beam that has emitted fewer tokens does not offer eos
      banned_tokens          tokens no live beam offers
      no_repeat_ngram_size   n >= 1: no n-gram of a hypothesis - prompt included - comes twice
      banned_sequences       lists of tokens: a sequence's last token is closed while the hypothesis ends in the tokens before it
      prompt                 (T0, B) int64: every beam's history starts as its batch row's prompt
      capacity               the longest history a beam can hold, prompt included (default: the prompt and 1024 tokens); a step on a
                             full history leaves it as it is and sets the batch row's `overflow`
    Owns the `closed` words, the flat sequence arrays and overflow (B) int32.  The histories are CARRIED, not owned: history() gives the
    first (hist (B W, capacity), hist_len (B W)) - None, None without an n-gram or sequence control -, every lm_beam_step(...,
    controls=, hist=, hist_len=) returns the survivors' as fresh buffers.  `carried` names them as lm_beam_step's keywords - ("hist",
    "hist_len"), or () where no history is kept -, first_carried() gives those of a search that starts, select() is the step's launches.
    ValueError for whatever check_beam_controls refuses, before any device work; whether W candidates always stay open depends on the
    steps that follow, which Model.beam_search checks."""

    def __init__(self, B, W, V, device, prompt=None, capacity=None, min_length=0, banned_tokens=None, no_repeat_ngram_size=0,
                 banned_sequences=None, eos=None):
        super().__init__(B, W, V, device)
        B, W, V, dev = self.B, self.W, self.V, self.device
        self.eos, self.min_length, self.banned, self.no_repeat_ngram_size, self.sequences = check_beam_controls(
            V, W, eos, min_length, banned_tokens, no_repeat_ngram_size, banned_sequences)
        if prompt is not None and not (isinstance(prompt, torch.Tensor) and prompt.dtype == torch.int64 and prompt.dim() == 2
                                       and prompt.shape[1] == B):
            raise ValueError(f"vmlmf_amd: BeamControls takes a (T0, {B}) int64 prompt")
        capacity = _history.check_capacity("BeamControls", capacity, int(prompt.shape[0]) if prompt is not None else 0)
        self.capacity = capacity
        self.keeps_history = self.no_repeat_ngram_size > 0 or bool(self.sequences)
        self.carried = ("hist", "hist_len") if self.keeps_history else ()
        self.overflow = torch.zeros(B, dtype=torch.int32, device=dev)
        self.closed = pack_words(self.banned, V).to(dev) if self.banned else None
        self.seq_tokens, self.seq_offsets = _history.flat_sequences(self.sequences, dev)
        self._hist0 = None
        if self.keeps_history:
            hist, hist_len = _history.prompt_history(prompt, B, V, capacity, dev)
            self._hist0 = (hist.repeat_interleave(W, 0).contiguous(), hist_len.repeat_interleave(W, 0))

    def history(self):
        """(hist (B W, capacity) int32, hist_len (B W) int32) of a search that starts: the prompt, repeated for the W beams of a batch
        row - fresh copies; (None, None) when no history is kept."""
        if self._hist0 is None:
            return None, None
        return self._hist0[0].clone(), self._hist0[1].clone()

    def first_carried(self):
        """[hist, hist_len] of a search that starts - [] when no history is kept."""
        return list(self.history()) if self.keeps_history else []

    def select(self, scores, bias, cum, finished, length, eos, embed, buffers=None, hist=None, hist_len=None):
        """lm_beam_step's selection under these controls (beamctl_select)."""
        return beamctl_select(scores, bias, cum, finished, length, eos, embed, self, hist, hist_len, buffers)

    def clone(self):
        """The same controls on a copy of the state (overflow; a BeamGraph's warm-up runs on one)."""
        c = object.__new__(type(self))
        c.__dict__.update(self.__dict__)
        c.overflow = self.overflow.clone()
        return c

    def beam_bans(self, hist, hist_len):
        """Every beam's own ban set for its next token, (B W, ceil(V / 32)) int32 words: ONE vmlmf_history_bans launch on the B W rows
        of hist / hist_len (libvmlmf_history.so - opened here, on the first call)."""
        return _history.launch_bans(hist, hist_len, self.capacity, self.no_repeat_ngram_size, self.seq_tokens, self.seq_offsets, self.V)


def beamctl_select(scores, bias, cum, finished, length, eos, embed, controls, hist=None, hist_len=None, buffers=None):
    """The launches of a controlled step on checked, contiguous arguments (scores (B W, V) without the bias, eos an int, -1: none): with
    a history, vmlmf_history_bans on the B W rows, then vmlmf_beamctl_step.  Returns lm_beam_step's seven results and (hist, hist_len) of
    the survivors behind them - fresh buffers, or (None, None) when the controls keep no history."""
    B, W = cum.shape
    V = scores.shape[1]
    dev = scores.device
    check_step_controls(controls, BeamControls, B, W, V, dev, eos)
    cap = controls.capacity
    bans = hist_out = len_out = None
    if controls.keeps_history:
        for t, what, shape in ((hist, "hist", (B * W, cap)), (hist_len, "hist_len", (B * W,))):
            if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.int32 and tuple(t.shape) == shape
                    and t.is_contiguous()):
                raise RuntimeError(f"vmlmf_amd.lm_beam_step: {what} must be a contiguous int32 {shape} tensor on {dev} (BeamControls.history())")
        bans = controls.beam_bans(hist, hist_len)
        hist_out, len_out = torch.empty_like(hist), torch.empty_like(hist_len)
    else:
        hist = hist_len = None
    c = Controls(controls.min_length, cap, ptr(controls.closed), ptr(bans), ptr(hist), ptr(hist_len), ptr(hist_out), ptr(len_out),
                 ptr(controls.overflow) if hist is not None else None)
    outs = launch_step(LIBRARY, "vmlmf_beamctl_step", scores, bias, cum, finished, length, eos, embed, buffers, before=(ctypes.byref(c),))
    return (*outs, hist_out, len_out)
