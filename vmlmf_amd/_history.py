"""ctypes binding of the C ABI in include/vmlmf_history.h (libvmlmf_history.so, built in-tree by csrc/Makefile beside libvmlmf_hip.so):
the choice of the LM decoder under controls that need a row's sequence of tokens - no_repeat_ngram_size, banned_sequences,
frequency_penalty and presence_penalty of Model.generate.  The library is loaded on the first call with one of them: a plain or a
controlled generate() without them, and a training process, never open it.

There is no fallback: if the library is missing, or a call fails, this raises.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _decode, _lib, _truncate
from ._decode import DecodeControls
from ._lib import ptr

ABI_VERSION = 1
MAX_V = 65536                # VMLMF_HISTORY_MAX_V: the widest vocabulary history bans are accepted for (the ban bitmap lives in LDS)
MAX_SEQUENCE_TOKENS = 4096   # the tokens of all banned sequences together: every row's workgroup walks the list in every step


class Controls(ctypes.Structure):
    """struct vmlmf_history_controls: struct vmlmf_decode_controls, then the history's fields"""
    _fields_ = _decode.Controls._fields_ + [
        ("no_repeat_ngram_size", ctypes.c_int32), ("frequency_penalty", ctypes.c_float), ("presence_penalty", ctypes.c_float),
        ("pad1", ctypes.c_int32), ("hist", ctypes.c_void_p), ("hist_len", ctypes.c_void_p), ("hist_capacity", ctypes.c_int32),
        ("pad2", ctypes.c_int32), ("count", ctypes.c_void_p), ("overflow", ctypes.c_void_p), ("seq_tokens", ctypes.c_void_p),
        ("seq_offsets", ctypes.c_void_p), ("n_sequences", ctypes.c_int32), ("pad3", ctypes.c_int32)]


# every symbol include/vmlmf_history.h declares: (restype, argtypes)
_vp, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
SYMBOLS = {
    "vmlmf_history_abi_version": (_i, []),
    "vmlmf_history_last_error": (ctypes.c_char_p, []),
    "vmlmf_history_choose": (_i, [_i, _i, _i, _vp, _vp, _vp, _f, _i, _f, _vp, _i, ctypes.POINTER(Controls), _vp, _vp, _vp, _vp, _vp]),
    "vmlmf_history_bans": (_i, [_i, _i, ctypes.POINTER(Controls), _vp, _vp]),
}

LIBRARY = _lib.Library("history", SYMBOLS, ABI_VERSION, "stock-op fallback for the history controls of Model.generate")
lib, loaded, check = LIBRARY.handle, LIBRARY.loaded, LIBRARY.check


def history_on(no_repeat_ngram_size=0, banned_sequences=None, frequency_penalty=0.0, presence_penalty=0.0):
    """Whether these arguments of Model.generate ask for the history launch."""
    return no_repeat_ngram_size != 0 or banned_sequences is not None or frequency_penalty != 0.0 or presence_penalty != 0.0


def check_history(V, no_repeat_ngram_size=0, banned_sequences=None, frequency_penalty=0.0, presence_penalty=0.0, prompt_length=0, steps=None,
                  closed=0):
    """The arguments as the C ABI takes them: (n, sequences as lists of ints, alpha, beta).  ValueError for a negative n, a negative or
    non-finite penalty, an empty sequence or one with a token outside [0, V), more than MAX_SEQUENCE_TOKENS sequence tokens in all, a
    vocabulary wider than MAX_V with a ban on, and - with a ban on and `steps` given: a decode of that many steps - for a vocabulary that
    might run out of open tokens: V <= closed + prompt_length + steps + len(sequences) + 1, where `closed` counts the tokens the other
    controls hold at -inf.  (A row's ban set holds at most one token per sequence and at most as many n-gram tokens as it has history,
    prompt_length + steps - 1 at the last step: beyond the bound a token always stays open.)"""
    try:
        n = int(no_repeat_ngram_size)
    except (TypeError, ValueError):
        raise ValueError(f"vmlmf_amd: no_repeat_ngram_size must be an integer >= 0, got {no_repeat_ngram_size!r}") from None
    if n < 0 or n != no_repeat_ngram_size:
        raise ValueError(f"vmlmf_amd: no_repeat_ngram_size must be an integer >= 0 (0: off), got {no_repeat_ngram_size}")
    pen = []
    for name, value in (("frequency_penalty", frequency_penalty), ("presence_penalty", presence_penalty)):
        try:
            x = float(value)
        except (TypeError, ValueError):
            raise ValueError(f"vmlmf_amd: {name} must be a finite number >= 0, got {value!r}") from None
        if not (x >= 0.0 and math.isfinite(x)):
            raise ValueError(f"vmlmf_amd: {name} must be finite and >= 0 (0: off), got {value}")
        pen.append(x)
    seqs = []
    for s in (banned_sequences or []):
        try:
            s = [int(t) for t in s]
        except TypeError:
            raise ValueError(f"vmlmf_amd: banned_sequences must be a list of lists of tokens, got {s!r} in it") from None
        if not s:
            raise ValueError("vmlmf_amd: banned_sequences holds an empty sequence")
        for t in s:
            if not 0 <= t < V:
                raise ValueError(f"vmlmf_amd: banned sequence token {t} is not a token of the vocabulary ({V})")
        seqs.append(s)
    total = sum(len(s) for s in seqs)
    if total > MAX_SEQUENCE_TOKENS:
        raise ValueError(f"vmlmf_amd: banned_sequences hold {total} tokens, more than {MAX_SEQUENCE_TOKENS} in all")
    if n > 0 or seqs:
        if V > MAX_V:
            raise ValueError(f"vmlmf_amd: no_repeat_ngram_size / banned_sequences need a vocabulary of at most {MAX_V} tokens, got {V}")
        need = int(closed) + int(prompt_length) + int(steps or 0) + len(seqs) + 1
        if steps is not None and V <= need:
            raise ValueError(f"vmlmf_amd: no_repeat_ngram_size / banned_sequences might leave no token to choose: the vocabulary ({V}) "
                             f"must exceed bans + prompt + steps + sequences + 1 = {need}")
    return n, seqs, pen[0], pen[1]


def check_capacity(who, capacity, T0):
    """For HistoryControls and BeamControls (`who`): `capacity`, default the prompt's T0 tokens and 1024; ValueError unless it holds them."""
    capacity = T0 + 1024 if capacity is None else int(capacity)
    if capacity < max(T0, 1):
        raise ValueError(f"vmlmf_amd: {who}: capacity={capacity} must be >= 1 and hold the prompt ({T0} tokens)")
    return capacity


def prompt_history(prompt, B, V, capacity, dev):
    """(hist (B, capacity) int32, hist_len (B) int32) on dev that hold the (T0, B) prompt (None: empty), its tokens clamped into [0, V)."""
    T0 = 0 if prompt is None else int(prompt.shape[0])
    hist = torch.zeros((B, capacity), dtype=torch.int32, device=dev)
    if T0 > 0:
        hist[:, :T0] = prompt.to(dev).t().clamp(0, V - 1).to(torch.int32)
    return hist, torch.full((B,), T0, dtype=torch.int32, device=dev)


def flat_sequences(sequences, dev):
    """(seq_tokens, seq_offsets) int32 on dev: the sequences end to end, and where each starts and the last ends; (None, None) for none."""
    if not sequences:
        return None, None
    offsets = torch.tensor([0] + [len(s) for s in sequences]).cumsum(0).to(torch.int32)
    return torch.tensor([t for s in sequences for t in s], dtype=torch.int32).to(dev), offsets.to(dev)


class HistoryControls(DecodeControls):
    """DecodeControls, and the controls that need a row's sequence of tokens (include/vmlmf_history.h):
      no_repeat_ngram_size   n >= 1: no n-gram of a row's tokens - prompt included - comes twice (n = 1: no token does)
      banned_sequences       lists of tokens: a sequence's last token is closed while the row ends in the tokens before it
      frequency_penalty      alpha >= 0: a token's score loses alpha times the number of times the row has GENERATED it ...
      presence_penalty       beta >= 0: ... and beta once it has generated it at all
      capacity               the longest history a row can hold, prompt included (default: the prompt and 1024 tokens); a launch on a
                             full history leaves it as it is and sets the row's `overflow` - later n-gram bans then miss the newest tokens
      prompt                 (T0, B) int64: `seen` starts as the set of its tokens, `hist` as the tokens themselves (stock ops, once)
    Owns, beside seen / finished / length: hist (B, capacity) int32, hist_len (B) int32, count (B, V) uint16, overflow (B) int32.
    Every lm_sample launch with these controls updates all of them in place - one object is one decode.  ValueError for whatever
    check_history and DecodeControls refuse, before any device work.  Whether a token always stays open depends on how many steps
    follow, which this object does not know: Model.generate checks that (check_history's `steps`); where nothing is open a launch
    gives token 0."""

    def __init__(self, B, V, device, no_repeat_ngram_size=0, banned_sequences=None, frequency_penalty=0.0, presence_penalty=0.0,
                 capacity=None, prompt=None, _checked=False, **decode_controls):
        T0 = int(prompt.shape[0]) if isinstance(prompt, torch.Tensor) and prompt.dim() == 2 else 0
        self.capacity = check_capacity("HistoryControls", capacity, T0)
        super().__init__(B, V, device, prompt=prompt, _checked=_checked, **decode_controls)
        self.no_repeat_ngram_size, self.sequences, self.frequency_penalty, self.presence_penalty = check_history(
            int(V), no_repeat_ngram_size, banned_sequences, frequency_penalty, presence_penalty)
        self.hist, self.hist_len = prompt_history(prompt, self.B, self.V, self.capacity, self.device)
        self.count = torch.zeros((self.B, self.V), dtype=torch.int16, device=self.device).view(torch.uint16)
        self.overflow = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self.seq_tokens, self.seq_offsets = flat_sequences(self.sequences, self.device)

    STATE = DecodeControls.STATE + ("hist", "hist_len", "count", "overflow")
    LIBRARY, ENTRY, STRUCT = LIBRARY, "vmlmf_history_choose", Controls
    TRUNCATION_REFUSAL = _truncate.HISTORY_REFUSAL

    def values(self):
        return dict(super().values(), no_repeat_ngram_size=self.no_repeat_ngram_size, frequency_penalty=self.frequency_penalty,
                    presence_penalty=self.presence_penalty, hist=ptr(self.hist), hist_len=ptr(self.hist_len), hist_capacity=self.capacity,
                    count=ptr(self.count), overflow=ptr(self.overflow), seq_tokens=ptr(self.seq_tokens),
                    seq_offsets=ptr(self.seq_offsets), n_sequences=len(self.sequences))


def history_choose(*args):      # decode_choose where only a HistoryControls will do: the vmlmf_history_choose launch
    _decode.decode_choose(*args, kind=HistoryControls)


def launch_bans(hist, hist_len, capacity, n, seq_tokens, seq_offsets, V, eos=-1, finished=None):
    """ONE vmlmf_history_bans launch on given buffers - hist (R, capacity), hist_len (R), n = no_repeat_ngram_size, flat_sequences' two -:
    (R, ceil(V / 32)) int32 words, bit v & 31 of word v >> 5 set when v is banned; with eos and finished (R), a finished row's are zero."""
    R, dev = hist_len.numel(), hist.device
    out = torch.empty((R, (V + 31) // 32), dtype=torch.int32, device=dev)
    c = Controls(repetition_penalty=1.0, eos=eos, finished=ptr(finished), no_repeat_ngram_size=n, hist=ptr(hist), hist_len=ptr(hist_len),
                 hist_capacity=capacity, seq_tokens=ptr(seq_tokens), seq_offsets=ptr(seq_offsets),
                 n_sequences=0 if seq_offsets is None else seq_offsets.numel() - 1)
    LIBRARY.call(dev, "vmlmf_history_bans", R, V, ctypes.byref(c), ptr(out))
    return out


def history_bans(controls):
    """The ban sets of the rows' NEXT choice (step 5 of the contract): launch_bans on the controls' own buffers.  No state moves."""
    B, V, dev = controls.B, controls.V, controls.seen.device
    if dev.type != "cuda":
        raise RuntimeError("vmlmf_amd.history_bans runs on the HIP kernel only: the controls must live on 'cuda' (no CPU fallback)")
    _decode.check_launch(controls, HistoryControls, B, V, dev, "history_bans")
    return launch_bans(controls.hist, controls.hist_len, controls.capacity, controls.no_repeat_ngram_size, controls.seq_tokens,
                       controls.seq_offsets, V, controls.eos, controls.finished)
