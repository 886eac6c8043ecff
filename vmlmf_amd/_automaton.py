"""ctypes binding of the C ABI in include/vmlmf_automaton.h (libvmlmf_automaton.so, built in-tree by csrc/Makefile beside
libvmlmf_hip.so): decoding under a token automaton - automaton= of Model.generate and Model.beam_search.  The library is loaded on
the first constrained call: every other generate() and beam_search(), and a training process, never open it; building a TokenAutomaton or
the controls on the CPU does not either.

There is no fallback: if the library is missing, or a call fails, this raises.
"""
from __future__ import annotations

import ctypes
from collections import deque

import numpy as np
import torch

from . import _decode, _lib
from ._beam import BeamPolicy, check_step_controls, launch_step
from ._beamctl import pack_words
from ._decode import DecodeControls
from ._lib import ptr

ABI_VERSION = 1


class Table(ctypes.Structure):
    """struct vmlmf_token_automaton"""
    _fields_ = [("next", ctypes.c_void_p), ("S", ctypes.c_int32), ("pad", ctypes.c_int32)]


class Controls(ctypes.Structure):
    """struct vmlmf_automaton_controls: struct vmlmf_decode_controls, then the table's fields, row_state and dead"""
    _fields_ = _decode.Controls._fields_ + [("next", ctypes.c_void_p), ("S", ctypes.c_int32), ("pad1", ctypes.c_int32),
                                            ("row_state", ctypes.c_void_p), ("dead", ctypes.c_void_p)]


# every symbol include/vmlmf_automaton.h declares: (restype, argtypes)
_vp, _sz, _i, _f = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_float
SYMBOLS = {
    "vmlmf_automaton_abi_version": (_i, []),
    "vmlmf_automaton_last_error": (ctypes.c_char_p, []),
    "vmlmf_automaton_choose": (_i, [_i, _i, _i, _vp, _vp, _vp, _f, _i, _f, _vp, _i, ctypes.POINTER(Controls), _vp, _vp, _vp, _vp, _vp]),
    "vmlmf_automaton_workspace_bytes": (_sz, [_i, _i, _i]),
    "vmlmf_automaton_beam_step": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, ctypes.POINTER(Table), _vp, _vp, _vp, _vp,
                                       _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
}

LIBRARY = _lib.Library("automaton", SYMBOLS, ABI_VERSION, "stock-op fallback for decoding under a token automaton")
lib, loaded, check = LIBRARY.handle, LIBRARY.loaded, LIBRARY.check

GENERATE_REFUSAL = ("vmlmf_amd: automaton= together with {what} is out of scope: the constrained choice runs under the stopping and token "
                    "controls (eos, min_length, repetition_penalty, logit_bias, banned_tokens) only")
BEAM_REFUSAL = ("vmlmf_amd: automaton= together with {what} is out of scope: the constrained beam step runs under eos, min_length and "
                "banned_tokens only")


def _tokens(V, tokens, what):
    """`tokens` as a list of ints in [0, V); ValueError otherwise."""
    try:
        out = [int(t) for t in tokens]
    except TypeError:
        raise ValueError(f"vmlmf_amd: TokenAutomaton.{what} takes sequences of tokens, got {tokens!r}") from None
    for t in out:
        if not 0 <= t < V:
            raise ValueError(f"vmlmf_amd: TokenAutomaton.{what}: token {t} is not a token of the vocabulary ({V})")
    return out


def _then(V, then, what):
    """-1 for "free", else the eos token; ValueError otherwise."""
    if isinstance(then, str):
        if then != "free":
            raise ValueError(f"vmlmf_amd: TokenAutomaton.{what}: then must be 'free' or the eos token, got {then!r}")
        return -1
    return _tokens(V, [then], what)[0]


class TokenAutomaton:
    """A finite automaton over the V tokens of a vocabulary as a dense table next (S, V) int32 on a device (include/vmlmf_automaton.h):
    next[s, v] >= 0 - in state s token v is open and leads to that state; next[s, v] < 0 - s does not offer v.  eos is a token like any
    other: a state is accepting iff it offers eos.  A state outside [0, S) offers nothing.  `start` is the state a row begins in.
    Validated once, on the host: next must be a 2-D integer tensor (or array) of S >= 1 rows with S V < 2^31, next.max() < S, start in
    [0, S); it is kept as a contiguous int32 tensor on the device it was given on (to(device): a copy elsewhere, made once).
    Constructors, all built on the host: forced, one_of, template, avoiding."""

    def __init__(self, next, start=0):
        t = next if isinstance(next, torch.Tensor) else torch.as_tensor(np.asarray(next))
        if t.dim() != 2 or t.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64) or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError("vmlmf_amd: TokenAutomaton takes next as an (S, V) integer table with S, V >= 1")
        S, V = int(t.shape[0]), int(t.shape[1])
        if S * V >= 1 << 31:
            raise ValueError(f"vmlmf_amd: TokenAutomaton: S V = {S * V} must stay below 2^31")
        if int(t.max()) >= S:
            raise ValueError(f"vmlmf_amd: TokenAutomaton: next holds state {int(t.max())}, outside [0, S = {S})")
        if not (isinstance(start, int) and 0 <= start < S):
            raise ValueError(f"vmlmf_amd: TokenAutomaton: start={start!r} must be a state in [0, {S})")
        self.next = t.detach().to(torch.int32).contiguous()
        self.S, self.V, self.start = S, V, start
        self._copies = {}
        self._host = None

    @property
    def device(self):
        return self.next.device

    def to(self, device):
        """This automaton with its table on `device` (self where it already is; a copy is made once per device)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device == self.next.device:
            return self
        got = self._copies.get(device)
        if got is None:
            got = self._copies[device] = object.__new__(TokenAutomaton)
            got.__dict__.update(self.__dict__)
            got.next, got._copies = self.next.to(device), {}
        return got

    def host(self):
        """The table as a numpy array (read back once)."""
        if self._host is None:
            self._host = self.next.cpu().numpy()
        return self._host

    def table(self):
        """struct vmlmf_token_automaton of this table"""
        return Table(self.next.data_ptr(), self.S, 0)

    # ---- constructors ----
    @classmethod
    def template(cls, V, slots, then="free"):
        """One slot per position, each a token or a collection of allowed tokens; then anything ("free") or `then` = eos only."""
        V = int(V)
        end = _then(V, then, "template")
        slots = [_tokens(V, [s] if isinstance(s, (int, np.integer)) else s, "template") for s in slots]
        for s in slots:
            if not s:
                raise ValueError("vmlmf_amd: TokenAutomaton.template: a slot allows no token")
        n = len(slots)
        nx = np.full((n + (1 if end < 0 else 2), V), -1, dtype=np.int32)
        for i, s in enumerate(slots):
            nx[i, s] = i + 1
        if end < 0:
            nx[n, :] = n            # free: every token, for ever
        else:
            nx[n, end] = n + 1      # eos alone ...
            nx[n + 1, end] = n + 1  # ... and behind it (a decode without the eos control keeps emitting it)
        return cls(torch.from_numpy(nx))

    @classmethod
    def forced(cls, V, tokens, then="free"):
        """Exactly these tokens; then anything ("free") or `then` = eos only."""
        return cls.template(V, [[t] for t in _tokens(int(V), tokens, "forced")], then)

    @classmethod
    def one_of(cls, V, sequences, then="free"):
        """A trie: exactly one of the sequences; then anything ("free": a sequence's last token leads straight there) or `then` = eos
        only (a sequence that is a prefix of another may stop or go on)."""
        V = int(V)
        end = _then(V, then, "one_of")
        seqs = [_tokens(V, s, "one_of") for s in sequences]
        if not seqs or any(not s for s in seqs):
            raise ValueError("vmlmf_amd: TokenAutomaton.one_of takes at least one sequence, none of them empty")
        rows, terminal = [{}], [False]
        FREE = -2
        for s in seqs:
            node = 0
            for i, t in enumerate(s):
                last = i == len(s) - 1
                if end < 0 and last:
                    rows[node][t] = FREE
                    break
                nxt = rows[node].get(t)
                if nxt == FREE:
                    break                       # a shorter sequence already leads to "anything" here
                if nxt is None:
                    rows.append({})
                    terminal.append(False)
                    nxt = rows[node][t] = len(rows) - 1
                node = nxt
                if last:
                    terminal[node] = True
        n = len(rows)
        nx = np.full((n + 1, V), -1, dtype=np.int32)
        for i, row in enumerate(rows):
            for t, j in row.items():
                nx[i, t] = n if j == FREE else j
            if terminal[i]:
                nx[i, end] = n
        if end < 0:
            nx[n, :] = n
        else:
            nx[n, end] = n
        return cls(torch.from_numpy(nx))

    @classmethod
    def avoiding(cls, V, sequences):
        """The Aho-Corasick automaton of the sequences: a state is the longest suffix of the history that is a proper prefix of a
        sequence; token v is closed in a state iff some sequence ends in v and its other tokens are a suffix of the history - the rule
        of banned_sequences (a sequence of one token is always closed).  Everything else is open."""
        V = int(V)
        seqs = [_tokens(V, s, "avoiding") for s in sequences]
        if any(not s for s in seqs):
            raise ValueError("vmlmf_amd: TokenAutomaton.avoiding: an empty sequence")
        child, bad = [{}], [False]
        for s in seqs:
            node = 0
            for t in s:
                nxt = child[node].get(t)
                if nxt is None:
                    child.append({})
                    bad.append(False)
                    nxt = child[node][t] = len(child) - 1
                node = nxt
            bad[node] = True
        n = len(child)
        goto = np.zeros((n, V), dtype=np.int64)     # the full transition function over the trie's nodes, breadth first
        fail = [0] * n
        for t, c in child[0].items():
            goto[0, t] = c
        queue = deque(child[0].values())
        while queue:
            u = queue.popleft()
            bad[u] = bad[u] or bad[fail[u]]
            goto[u] = goto[fail[u]]
            for t, c in child[u].items():
                fail[c] = int(goto[fail[u], t])
                goto[u, t] = c
                queue.append(c)
        bad = np.asarray(bad)
        keep = np.flatnonzero(~bad)                 # (the root is never bad: no sequence is empty)
        number = np.full(n, -1, dtype=np.int64)
        number[keep] = np.arange(keep.size)
        return cls(torch.from_numpy(number[goto[keep]].astype(np.int32)))

    # ---- running it ----
    def advance(self, tokens, state=None):
        """The states (B) int32 of B rows after the (T, B) tokens, from `state` (B) (None: start), with stock ops on the table's device
        and ONE read-back.  ValueError if a row takes a closed transition, holds a token outside the vocabulary or starts outside [0, S)."""
        if not (isinstance(tokens, torch.Tensor) and tokens.dim() == 2 and tokens.dtype == torch.int64):
            raise ValueError("vmlmf_amd: TokenAutomaton.advance takes (T, B) int64 tokens")
        dev, B = self.next.device, tokens.shape[1]
        tokens = tokens.to(dev)
        st = torch.full((B,), self.start, dtype=torch.int64, device=dev) if state is None else state.to(dev).to(torch.int64).reshape(-1)
        if st.numel() != B:
            raise ValueError(f"vmlmf_amd: TokenAutomaton.advance: state must hold {B} states")
        wrong = (st < 0) | (st >= self.S)
        for t in tokens:
            wrong = wrong | (t < 0) | (t >= self.V)
            st = self.next[st.clamp(0, self.S - 1), t.clamp(0, self.V - 1)].to(torch.int64)
            wrong = wrong | (st < 0)
        if bool(wrong.any()):
            raise ValueError("vmlmf_amd: TokenAutomaton.advance: a row takes a closed transition (or holds a token or a state out of range)")
        return st.to(torch.int32)

    def open_tokens(self, state):
        """The tokens `state` offers, ascending (none for a state outside [0, S))."""
        state = int(state)
        return [] if not 0 <= state < self.S else np.flatnonzero(self.host()[state] >= 0).tolist()

    def accepts(self, tokens, state=None, eos=None):
        """Whether the automaton can emit this sequence of tokens from `state` (None: start): every transition is open.  With eos, the
        walk ends behind the first eos (what follows a finished row's eos is padding)."""
        s, nx = self.start if state is None else int(state), self.host()
        for t in (tokens.tolist() if isinstance(tokens, torch.Tensor) else tokens):
            t = int(t)
            if not (0 <= s < self.S and 0 <= t < self.V) or nx[s, t] < 0:
                return False
            s = int(nx[s, t])
            if eos is not None and t == eos:
                break
        return True

    def check_reachable(self, states, closed=None, eos=-1, min_length=0):
        """ValueError unless every state reachable from `states` offers a token that `closed` ((V) bool, numpy) leaves open - and, with
        min_length > 0, one besides eos.  With eos >= 0 the walk does not go through eos: a row behind it is finished and its state is
        not looked at again."""
        nx = self.host()
        usable = nx >= 0
        if closed is not None:
            usable = usable & ~closed[None, :]
        follow = usable.copy()
        if eos >= 0:
            follow[:, eos] = False
        if eos >= 0 and min_length > 0:
            usable = follow
        seen = np.zeros(self.S, dtype=bool)
        frontier = np.unique(np.asarray(states, dtype=np.int64))
        while frontier.size:
            seen[frontier] = True
            stuck = frontier[~usable[frontier].any(axis=1)]
            if stuck.size:
                what = "no open token" if not (eos >= 0 and min_length > 0) else "no open token besides eos, which min_length holds back"
                raise ValueError(f"vmlmf_amd: automaton state {int(stuck[0])} is reachable and has {what} (banned_tokens and -inf biases "
                                 "counted)")
            nxt = np.unique(nx[frontier][follow[frontier]])
            frontier = nxt[~seen[nxt]]

    def __repr__(self):
        return f"TokenAutomaton(S={self.S}, V={self.V}, start={self.start}, device={self.next.device})"


def check_automaton(automaton, V, B, automaton_state):
    """The start states of B rows as a (B) int64 numpy array.  ValueError unless `automaton` is a TokenAutomaton over V tokens and
    automaton_state is None (every row at automaton.start) or a (B) int32 tensor of states in [0, S).  Reads automaton_state back once."""
    if not isinstance(automaton, TokenAutomaton):
        raise ValueError(f"vmlmf_amd: automaton must be a vmlmf_amd.TokenAutomaton, got {type(automaton).__name__}")
    if automaton.V != V:
        raise ValueError(f"vmlmf_amd: the automaton is over {automaton.V} tokens, the vocabulary has {V}")
    if automaton_state is None:
        return np.full(B, automaton.start, dtype=np.int64)
    if not (isinstance(automaton_state, torch.Tensor) and automaton_state.dtype == torch.int32 and tuple(automaton_state.shape) == (B,)):
        raise ValueError(f"vmlmf_amd: automaton_state must be a ({B},) int32 tensor (one state per row), or None")
    st = automaton_state.detach().cpu().numpy().astype(np.int64)
    if st.size and (st.min() < 0 or st.max() >= automaton.S):
        raise ValueError(f"vmlmf_amd: automaton_state holds a state outside [0, S = {automaton.S})")
    return st


def closed_tokens(V, logit_bias, banned):
    """(V) bool numpy: the tokens a -inf bias or a ban closes (logit_bias already checked: _decode.check_bias)."""
    closed = np.zeros(V, dtype=bool)
    if logit_bias is not None:
        closed |= (logit_bias.detach().cpu() == float("-inf")).numpy()
    if banned:
        closed[np.asarray(banned, dtype=np.int64)] = True
    return closed


class AutomatonControls(DecodeControls):
    """DecodeControls, and a TokenAutomaton the rows walk (include/vmlmf_automaton.h): per step a row's state closes the tokens its table
    row does not offer - the choice launch applies that beside the other controls - and moves on with the chosen token.
      automaton      a TokenAutomaton over V tokens (used on `device`: automaton.to(device))
      state          (B) int32 start states, or None: automaton.start for every row.  The prompt is NOT consumed: pass
                     automaton.advance(prompt) where it should be
    Owns, beside seen / finished / length: row_state (B) int32 and dead (B) int32 - set, and never cleared, where a row had nothing to
    choose.  Every lm_sample launch with these controls (vmlmf_automaton_choose) updates all of them in place - one object is one decode."""

    def __init__(self, B, V, device, automaton, state=None, _checked=False, **decode_controls):
        start = check_automaton(automaton, int(V), int(B), state)
        super().__init__(B, V, device, _checked=_checked, **decode_controls)
        if not _checked:
            automaton.check_reachable(start, closed_tokens(self.V, self.logit_bias, None), self.eos, self.min_length)
        self.automaton = automaton.to(self.device)
        self.row_state = torch.from_numpy(start.astype(np.int32)).to(self.device)
        self.dead = torch.zeros(self.B, dtype=torch.int32, device=self.device)

    STATE = DecodeControls.STATE + ("row_state", "dead")
    LIBRARY, ENTRY, STRUCT = LIBRARY, "vmlmf_automaton_choose", Controls
    TRUNCATION_REFUSAL = GENERATE_REFUSAL.format(what="min_p / typical_p / epsilon_cutoff / eta_cutoff")

    def values(self):
        return dict(super().values(), next=ptr(self.automaton.next), S=self.automaton.S, row_state=ptr(self.row_state), dead=ptr(self.dead))


class AutomatonBeamControls(BeamPolicy):
    """The controls of one beam search over B batch rows of W beams under a TokenAutomaton on `device` (include/vmlmf_automaton.h):
      automaton, state   as AutomatonControls': (B) int32 start states of the batch rows (None: automaton.start)
      eos, min_length, banned_tokens   Model.beam_search's, as BeamControls'
    They only close candidates, so scores stay sums of plain log-probabilities.  Owns the `closed` words.  The beams' states are CARRIED,
    not owned: start() gives the first beam_state (B W) int32, every lm_beam_step(..., controls=, beam_state=) returns the survivors' as a
    fresh buffer behind its seven results.  `carried` names it as lm_beam_step's keyword, first_carried() is [start()], select() the
    step's launch."""

    carried = ("beam_state",)

    def __init__(self, B, W, V, device, automaton, state=None, eos=None, min_length=0, banned_tokens=None, _checked=False):
        super().__init__(B, W, V, device)
        B, W, V = self.B, self.W, self.V
        start = check_automaton(automaton, V, B, state)
        self.eos, self.min_length, _, self.banned = _decode.check_controls(V, eos=eos, min_length=min_length, banned_tokens=banned_tokens)
        if self.eos >= 0 and self.eos in self.banned:
            raise ValueError(f"vmlmf_amd: eos={self.eos} is among banned_tokens: a finished beam offers eos alone")
        if not _checked:
            automaton.check_reachable(start, closed_tokens(V, None, self.banned), self.eos, self.min_length)
        self.automaton = automaton.to(self.device)
        self.closed = pack_words(self.banned, V).to(self.device) if self.banned else None
        self._start = torch.from_numpy(start.astype(np.int32)).to(self.device).repeat_interleave(W, 0).contiguous()

    def start(self):
        """beam_state (B W) int32 of a search that starts: every beam of a batch row in the row's start state - a fresh copy."""
        return self._start.clone()

    def first_carried(self):
        return [self.start()]

    def select(self, scores, bias, cum, finished, length, eos, embed, buffers=None, beam_state=None):
        """lm_beam_step's selection under these controls (automaton_select)."""
        return automaton_select(scores, bias, cum, finished, length, eos, embed, self, beam_state, buffers)


def automaton_select(scores, bias, cum, finished, length, eos, embed, controls, beam_state=None, buffers=None):
    """The vmlmf_automaton_beam_step launch on checked, contiguous arguments (scores (B W, V) without the bias, eos an int, -1: none).
    Returns lm_beam_step's seven results and the survivors' beam_state (B W) int32 - a fresh buffer - behind them."""
    B, W = cum.shape
    V = scores.shape[1]
    dev = scores.device
    check_step_controls(controls, AutomatonBeamControls, B, W, V, dev, eos)
    if beam_state is None:
        beam_state = controls.start()
    if not (isinstance(beam_state, torch.Tensor) and beam_state.device == dev and beam_state.dtype == torch.int32
            and tuple(beam_state.shape) == (B * W,) and beam_state.is_contiguous()):
        raise RuntimeError(f"vmlmf_amd.lm_beam_step: beam_state must be a contiguous int32 ({B * W},) tensor on {dev} "
                           "(AutomatonBeamControls.start())")
    state_out = torch.empty_like(beam_state)
    table = controls.automaton.table()
    outs = launch_step(LIBRARY, "vmlmf_automaton_beam_step", scores, bias, cum, finished, length, eos, embed, buffers,
                       before=(controls.min_length, ptr(controls.closed), ctypes.byref(table), ptr(beam_state), ptr(state_out)))
    return (*outs, state_out)
