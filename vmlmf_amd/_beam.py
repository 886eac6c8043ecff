"""ctypes binding of the C ABI in include/vmlmf_beam.h (libvmlmf_beam.so, built in-tree by csrc/Makefile beside libvmlmf_hip.so):
the beam-search step of the LM decoder.  The library is loaded on the first beam call - a training process never opens it.

There is no fallback: if the library is missing, or a call fails, this raises.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import ptr

ABI_VERSION = 1
MAX_BEAMS = 32
MAX_TENSORS = 16

# every symbol include/vmlmf_beam.h declares: (restype, argtypes)
_vp, _sz, _i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
SYMBOLS = {
    "vmlmf_beam_abi_version": (_i, []),
    "vmlmf_beam_last_error": (ctypes.c_char_p, []),
    "vmlmf_beam_workspace_bytes": (_sz, [_i, _i, _i]),
    "vmlmf_beam_step": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "vmlmf_beam_gather": (_i, [_i, _i, _i, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp]),
    "vmlmf_beam_backtrack": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
}

LIBRARY = _lib.Library("beam", SYMBOLS, ABI_VERSION, "stock-op fallback for the beam-search step")
lib, loaded, check = LIBRARY.handle, LIBRARY.loaded, LIBRARY.check


def check_beams(beams, V=None):
    """beams as the C ABI takes it; ValueError for beams < 1, beams > MAX_BEAMS and beams > V."""
    W = int(beams)
    if W < 1 or W > MAX_BEAMS:
        raise ValueError(f"vmlmf_amd: beams must lie in [1, {MAX_BEAMS}], got {beams}")
    if V is not None and W > V:
        raise ValueError(f"vmlmf_amd: beams={W} exceeds the vocabulary ({V} tokens): a beam offers V candidates")
    return W


def _require(t, what, dtype=torch.float32):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f"vmlmf_amd: {what} is not on a HIP device; the beam-search step runs only as HIP kernels on an MI355X "
                           "(no CPU fallback). Move the model and inputs to 'cuda'.")
    if t.dtype != dtype:
        raise RuntimeError(f"vmlmf_amd: {what} must be {dtype}, got {t.dtype}")


_BUFFERS = {}


def step_buffers(dev, B, W, V, library=None):
    """(ticket (B) int32 - zero, and left zero by every launch -, workspace) of a beam step at this shape, kept per (library, device,
    stream): launches that share them must be ordered on one stream.  library: the side library whose vmlmf_<name>_workspace_bytes sizes
    the workspace (default: this one; the controlled, automaton and group steps need what vmlmf_beam_step needs) - a pair is never
    shared between two libraries.  Not to be called inside a stream capture (BeamGraph brings its own)."""
    key = (library or LIBRARY, dev.index, _lib.raw_stream(dev).value, B, W, V)
    got = _BUFFERS.get(key)
    if got is None:
        got = _BUFFERS[key] = new_step_buffers(dev, B, W, V, library)
    return got


def new_step_buffers(dev, B, W, V, library=None):
    """A ticket and a workspace of one's own (a captured graph's: its launches must not meet another stream's on one ticket), sized
    as step_buffers' by `library`."""
    nbytes = (library or LIBRARY).workspace_bytes(B, W, V)
    return torch.zeros(B, device=dev, dtype=torch.int32), torch.empty((nbytes + 7) // 8, device=dev, dtype=torch.int64)


class BeamPolicy:
    """What lm_beam_step, decoding.beam_steps and BeamGraph ask of a `controls` object - a beam step that differs from the plain one
    over B batch rows of W beams and a V-token vocabulary on `device` -, with the defaults of a policy that carries nothing:
      carried            the names of the tensors it hands on from step to step behind cum, finished and length (lm_beam_step's keywords)
      first_carried()    those tensors for a search that starts
      first_beams()      (cum, finished, length), each (B, W), of a search that starts: beam 0 of a row at score 0, the others at -inf
      select(scores, bias, cum, finished, length, eos, embed, buffers, **carried)    the step's launch on checked arguments: the seven
                         results of lm_beam_step, the survivors' carried tensors behind them (each policy's own; None is the plain step)
      clone()            what a graph's warm-up runs on: a copy of whatever state a launch moves (default: none, the object itself)
      new_buffers()      a (ticket, workspace) pair of its own for a captured graph, of the size ITS step needs
      keeps_history, eos, min_length    what check_step_controls reads (it holds no eos of its own: the step's is used)
    ValueError for what check_beams refuses, before any device work."""

    carried = ()
    keeps_history = False
    eos, min_length = -1, 0

    def __init__(self, B, W, V, device):
        self.B, self.V = int(B), int(V)
        self.W = check_beams(W, self.V)
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev                           # (with its index: what a launch's tensors are compared with)

    def first_carried(self):
        return []

    def first_beams(self):
        cum = torch.full((self.B, self.W), float("-inf"), device=self.device)
        cum[:, 0] = 0.0
        return cum, torch.zeros_like(cum, dtype=torch.int32), torch.zeros_like(cum, dtype=torch.int32)

    def new_buffers(self):
        return new_step_buffers(self.device, self.B, self.W, self.V)

    def clone(self):
        return self


def check_carried(controls, given):
    """TypeError for a keyword among `given` - carried tensors by name - that the controls (None: the plain step) do not carry."""
    names = () if controls is None else controls.carried
    for name in given:
        if name not in names:
            who = "the plain beam step" if controls is None else f"this {type(controls).__name__}"
            raise TypeError(f"vmlmf_amd: {name}= is not carried by {who} (it carries {', '.join(names) or 'nothing'})")


def lm_beam_step(h, weight, bias, cum, finished, length, eos, embed=None, buffers=None, controls=None, **carried):
    """One step of beam search over B batch rows of W beams (cum is (B, W)): the head's GEMM over the beams' top-layer outputs h (B W, H)
    - row b W + w is beam w of batch row b -, then ONE launch (vmlmf_beam_step, csrc/vmlmf_beam.hip) that forms every candidate's total
    cum[b, w] + log_softmax(h fc.w^T + bias)[v] in fp32, keeps the W best of each batch row under the total order (larger total first,
    equal totals to the lower flat index w V + v) and writes them in that order.  A finished beam (finished[b, w] set and eos given)
    offers (w, eos) alone, at its total so far.
    finished: (B, W) bool or int32; length: (B, W) int32; eos: a token, or None - then no beam is finished, whatever `finished` says.
    Returns (parent (B, W) int32, token (B, W) int64, total (B, W) fp32, finished (B, W) int32, length (B, W) int32,
    x_next (B W, H) = embed[token] or None without embed, src_row (B W) int32 = b W + parent: the state row a survivor continues).
    buffers: (ticket, workspace) of new_step_buffers() - default: the current stream's.
    controls: a BeamPolicy - the selection is then its select(), which takes the tensors it carries (controls.carried) as keywords
    **carried and returns the survivors' behind the seven results; a keyword it does not carry is a TypeError.
    A BeamControls (_beamctl.py: min_length, banned_tokens, no_repeat_ngram_size, banned_sequences) - the selection is
    ONE launch of vmlmf_beamctl_step (csrc/vmlmf_beamctl.hip, a library of its own) in which a live beam withholds what the controls
    close, behind ONE vmlmf_history_bans launch on the beams' histories hist (B W, capacity) / hist_len (B W) when an n-gram or a
    sequence control is on; the totals of what is offered are the plain step's to the bit.  Two more results follow the seven: the
    survivors' (hist, hist_len), fresh buffers - (None, None) when the controls keep no history.
    An AutomatonBeamControls (_automaton.py: a TokenAutomaton, min_length, banned_tokens) - the selection is ONE launch of
    vmlmf_automaton_beam_step (csrc/vmlmf_automaton.hip) on beam_state (B W) int32, the beams' states (default: controls.start()); one
    more result follows the seven: the survivors' states, a fresh buffer.
    A GroupBeams (_beamgroup.py: groups, diversity_penalty) - the selection is ONE launch of vmlmf_beamgroup_step
    (csrc/vmlmf_beamgroup.hip), the same kernel whose merge runs group by group; the seven results, nothing carried.
    A StochasticBeams (_sbeam.py) whose `state` is set - the selection is lm_sbeam_step's ONE launch of vmlmf_sbeam_step on perturbed
    (B, W) and draw (B); the survivors' perturbed and draw + 1 follow the seven."""
    if carried:
        check_carried(controls, carried)
    h2, w, *rest = check_step("lm_beam_step", h, weight, bias, cum, finished, length, eos, embed)
    args = (torch.mm(h2, w.t()), *rest)
    if controls is None:
        return beam_select(*args, buffers)
    return controls.select(*args, buffers, **carried)


def check_step(caller, h, weight, bias, cum, finished, length, eos, embed):
    """What a beam step (`caller`: lm_beam_step, lm_sbeam_step - named in the messages) asks of its arguments: fp32 h, weight, cum and -
    where given - bias and embed on a HIP device, cum (B, W) with W beams the C ABI takes, h (B W, H) against weight (V, H), bias (V)
    and embed (V, H), finished (bool or int32) and length (int32) like cum, eos None or a token.  Returns (h (B W, H), weight, bias,
    cum, finished as int32, length, eos as an int - -1: none -, embed), the tensors contiguous."""
    for t, what in ((h, "h"), (weight, "weight"), (cum, "cum")):
        _require(t, what)
    if bias is not None:
        _require(bias, "bias")
    if embed is not None:
        _require(embed, "embedding table")
    if cum.dim() != 2:
        raise RuntimeError(f"vmlmf_amd.{caller}: cum must be (B, W), got {tuple(cum.shape)}")
    B, W = cum.shape
    h2 = h.reshape(-1, h.shape[-1]).contiguous()
    H = h2.shape[1]
    w = weight.contiguous()
    V = w.shape[0]
    check_beams(W, V)
    if h2.shape[0] != B * W or w.shape[1] != H or (bias is not None and bias.numel() != V) or (embed is not None and tuple(embed.shape) != (V, H)):
        raise RuntimeError(f"vmlmf_amd.{caller}: h {tuple(h.shape)} must be (B W, H) for cum {tuple(cum.shape)}, weight "
                           f"{tuple(weight.shape)} (V, H), bias / embed (V) / (V, H)")
    if tuple(finished.shape) != (B, W) or tuple(length.shape) != (B, W):
        raise RuntimeError(f"vmlmf_amd.{caller}: finished and length must be (B, W) like cum")
    _require(length, "length", torch.int32)
    if finished.dtype == torch.bool:
        finished = finished.to(torch.int32)
    _require(finished, "finished", torch.int32)
    eos_c = -1 if eos is None else int(eos)
    if eos is not None and not 0 <= eos_c < V:
        raise ValueError(f"vmlmf_amd.{caller}: eos={eos} is not a token of the vocabulary ({V})")
    return (h2, w, None if bias is None else bias.contiguous(), cum.contiguous(), finished.contiguous(), length.contiguous(), eos_c,
            None if embed is None else embed.contiguous())


def step_outputs(B, W, H, dev, embed):
    """The seven results of a beam step, uninitialised: parent, token, total, finished, length (B, W), x_next (B W, H) - None without
    embed -, src_row (B W)."""
    parent = torch.empty((B, W), device=dev, dtype=torch.int32)
    token = torch.empty((B, W), device=dev, dtype=torch.int64)
    total = torch.empty((B, W), device=dev, dtype=torch.float32)
    fin = torch.empty((B, W), device=dev, dtype=torch.int32)
    ln = torch.empty((B, W), device=dev, dtype=torch.int32)
    src = torch.empty(B * W, device=dev, dtype=torch.int32)
    xn = torch.empty((B * W, H), device=dev, dtype=torch.float32) if embed is not None else None
    return parent, token, total, fin, ln, xn, src


def check_step_controls(controls, kind, B, W, V, dev, eos):
    """RuntimeError unless `controls` is a `kind` for B x W beams over V tokens on dev; ValueError if it holds another eos than the step's."""
    if not isinstance(controls, kind) or (controls.B, controls.W, controls.V) != (B, W, V) or controls.device != dev:
        a = "an" if kind.__name__[0] in "AEIOU" else "a"
        raise RuntimeError(f"vmlmf_amd.lm_beam_step: controls must be {a} {kind.__name__} for {B} x {W} beams over {V} tokens on {dev}")
    if (controls.eos >= 0 or controls.min_length > 0) and controls.eos != eos:
        raise ValueError(f"vmlmf_amd.lm_beam_step: the controls' eos ({controls.eos}) is not the step's ({eos})")


def launch_step(library, entry, scores, bias, cum, finished, length, eos, embed, buffers, before=(), behind=(), sized_by=None):
    """ONE launch of a beam step - `entry` of `library` - on checked, contiguous arguments (scores (B W, V) without the bias, eos an
    int, -1: none): the 21 arguments every step's entry point shares, in ABI order - B, W, H, V, the five inputs, eos, embed, the seven
    outputs, ticket, workspace, workspace_bytes -, the entry point's own `before` the outputs or `behind` workspace_bytes.  buffers:
    (ticket, workspace), default: the current stream's of the library `sized_by` (step_buffers).  Returns step_outputs' seven."""
    B, W = cum.shape
    V = scores.shape[1]
    dev = scores.device
    ticket, ws = buffers if buffers is not None else step_buffers(dev, B, W, V, sized_by)
    H = embed.shape[1] if embed is not None else 1
    outs = step_outputs(B, W, H, dev, embed)
    library.call(dev, entry, B, W, H, V, ptr(scores), ptr(bias), ptr(cum), ptr(finished), ptr(length), eos, ptr(embed), *before,
                 *map(ptr, outs), ptr(ticket), ptr(ws), ws.numel() * 8, *behind)
    return outs


def beam_select(scores, bias, cum, finished, length, eos, embed, buffers=None):
    """The vmlmf_beam_step launch on checked, contiguous arguments: scores (B W, V) without the bias, eos an int (-1: none).
    lm_beam_step's results."""
    return launch_step(LIBRARY, "vmlmf_beam_step", scores, bias, cum, finished, length, eos, embed, buffers)


def beam_gather(tensors, src_row):
    """[t.index_select(0, src_row) for t in tensors] in ONE launch (vmlmf_beam_gather): up to MAX_TENSORS fp32 tensors of one shape
    (..., H) whose leading dimensions flatten to the src_row.numel() rows (a layer's (B W, H) state, or nn.LSTM's (1, B W, H)).
    src_row: int32.  Returns new tensors; the inputs are not written."""
    tensors = list(tensors)
    if not 1 <= len(tensors) <= MAX_TENSORS:
        raise ValueError(f"vmlmf_amd.beam_gather: 1 .. {MAX_TENSORS} tensors a launch, got {len(tensors)}")
    _require(src_row, "src_row", torch.int32)
    rows = src_row.numel()
    shape = tensors[0].shape
    H = shape[-1]
    for t in tensors:
        _require(t, "a state tensor")
        if t.shape != shape or t.numel() != rows * H:
            raise RuntimeError(f"vmlmf_amd.beam_gather: every tensor must be {tuple(shape)} with {rows} rows of {H}, got {tuple(t.shape)}")
    srcs = [t.contiguous() for t in tensors]
    dsts = [torch.empty_like(t) for t in srcs]
    n = len(srcs)
    sp = (_vp * n)(*[t.data_ptr() for t in srcs])
    dp = (_vp * n)(*[t.data_ptr() for t in dsts])
    rows_c = src_row.contiguous()
    LIBRARY.call(srcs[0].device, "vmlmf_beam_gather", n, rows, H, ptr(rows_c), sp, dp)
    return dsts


def beam_backtrack(parent, token, order=None):
    """The hypotheses behind the last step's slots: parent (steps, B, W) int32 and token (steps, B, W) int64 as lm_beam_step wrote
    them -> (steps, B, W) int64 where [:, b, w] is the hypothesis ending in slot order[b, w] (None: slot w), read back through the parent
    pointers (vmlmf_beam_backtrack: one thread per (b, w))."""
    _require(parent, "parent", torch.int32)
    _require(token, "token", torch.int64)
    if parent.dim() != 3 or parent.shape != token.shape:
        raise RuntimeError("vmlmf_amd.beam_backtrack: parent and token must both be (steps, B, W)")
    steps, B, W = parent.shape
    if order is not None:
        _require(order, "order", torch.int32)
        if tuple(order.shape) != (B, W):
            raise RuntimeError("vmlmf_amd.beam_backtrack: order must be (B, W)")
        order = order.contiguous()
    out = torch.empty_like(token, memory_format=torch.contiguous_format)
    if steps == 0:
        return out
    p, t = parent.contiguous(), token.contiguous()
    LIBRARY.call(p.device, "vmlmf_beam_backtrack", steps, B, W, ptr(p), ptr(t), ptr(order), ptr(out))
    return out
