"""ctypes binding of the C ABI in include/vmlmf_sbeam.h (libvmlmf_sbeam.so, built in-tree by csrc/Makefile beside
libvmlmf_hip.so): the step of stochastic beam search of the LM decoder - Model.stochastic_beam_search.  The library is loaded on the
first stochastic step: generate(), beam_search(), score(), contrastive_search(), cache_score() and a training process never open it.

There is no fallback: if the library is missing, or a call fails, this raises.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._beam import _require, check_beams, check_step, step_outputs
from ._lib import ptr

ABI_VERSION = 1

# every symbol include/vmlmf_sbeam.h declares: (restype, argtypes)
_vp, _sz, _i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
SYMBOLS = {
    "vmlmf_sbeam_abi_version": (_i, []),
    "vmlmf_sbeam_last_error": (ctypes.c_char_p, []),
    "vmlmf_sbeam_workspace_bytes": (_sz, [_i, _i, _i]),
    "vmlmf_sbeam_step": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp,
                              _vp, _vp, _vp, _vp]),
}

LIBRARY = _lib.Library("sbeam", SYMBOLS, ABI_VERSION, "stock-op fallback for the stochastic beam-search step")
lib, loaded, check = LIBRARY.handle, LIBRARY.loaded, LIBRARY.check


def check_sbeam(beams, V=None):
    """beams as the C ABI takes it (check_beams): ValueError for beams < 1, beams > 32 and beams > V."""
    return check_beams(beams, V)


class StochasticBeams:
    """What one stochastic beam search (Kool, van Hoof and Welling) over B batch rows of W beams and a V-token vocabulary on `device`
    owns: its ticket words and workspace (created on the first launch, so a CPU object costs nothing and opens no library).  start()
    gives a search's first (cum, finished, length, perturbed, draw): beam 0 of a row at total 0 and perturbed value 0, the others at
    -inf, no step drawn.  ValueError for what check_sbeam refuses, before any device work."""

    def __init__(self, B, W, V, device):
        self.B, self.V = int(B), int(V)
        self.W = check_sbeam(W, self.V)
        if self.B < 1:
            raise ValueError(f"vmlmf_amd: StochasticBeams needs B >= 1 batch rows, got {B}")
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self._buffers = None

    def start(self):
        """(cum, finished, length, perturbed, draw) of a search that starts."""
        B, W, dev = self.B, self.W, self.device
        cum = torch.full((B, W), float("-inf"), device=dev)
        cum[:, 0] = 0.0
        zeros = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        return cum, zeros(B, W), zeros(B, W), cum.clone(), zeros(B)

    def buffers(self):
        """(ticket (B) int32 - zero, and left zero by every launch -, workspace): this object's own, so its launches never meet
        another search's on one ticket.  Not to be created inside a stream capture (a graph's warm-up creates them)."""
        if self._buffers is None:
            nbytes = lib().vmlmf_sbeam_workspace_bytes(self.B, self.W, self.V)
            self._buffers = (torch.zeros(self.B, device=self.device, dtype=torch.int32),
                             torch.empty((nbytes + 7) // 8, device=self.device, dtype=torch.int64))
        return self._buffers


def lm_sbeam_step(h, weight, bias, cum, finished, length, perturbed, draw, state, eos, embed=None, buffers=None):
    """One step of stochastic beam search over B batch rows of W beams (cum is (B, W)): the head's GEMM over the beams' top-layer
    outputs h (B W, H) - row b W + w is beam w of batch row b -, then ONE launch (vmlmf_sbeam_step, csrc/vmlmf_sbeam.hip; include/
    vmlmf_sbeam.h has the contract): every candidate's total phi = cum[b, w] + log_softmax(h fc.w^T + bias)[v] in fp32 with
    lm_beam_step's bits, perturbed by the sampler's Gumbel noise at position draw[b] B W + b W + w, conditioned top-down on the
    parent's perturbed value; the W candidates of each batch row with the largest perturbed values survive, in that order.
    perturbed (B, W) fp32: the beams' perturbed values; draw (B) int32: the steps taken so far; state: a {seed, offset} snapshot of
    dropout_advance() - two int64 on the device; finished, length, eos, embed: lm_beam_step's.
    Returns lm_beam_step's seven results (parent, token, total, finished, length, x_next, src_row) and behind them the survivors'
    perturbed (B, W) and draw + 1 (B), fresh buffers.  buffers: (ticket, workspace) of a StochasticBeams.buffers() - default: a pair
    kept per (device, stream, B, W, V)."""
    h2, w, bias, cum, finished, length, eos_c, embed = check_step("lm_sbeam_step", h, weight, bias, cum, finished, length, eos, embed)
    B, W = cum.shape
    _require(perturbed, "perturbed")
    if tuple(perturbed.shape) != (B, W) or tuple(draw.shape) != (B,):
        raise RuntimeError("vmlmf_amd.lm_sbeam_step: finished, length and perturbed must be (B, W) like cum, draw (B)")
    _require(draw, "draw", torch.int32)
    if not (isinstance(state, torch.Tensor) and state.is_cuda and state.dtype == torch.int64 and state.numel() == 2):
        raise RuntimeError("vmlmf_amd.lm_sbeam_step: state must be a {seed, offset} snapshot: two int64 on the device")
    return sbeam_select(torch.mm(h2, w.t()), bias, cum, finished, length, perturbed.contiguous(), draw.contiguous(), state.contiguous(),
                        eos_c, embed, buffers)


_BUFFERS = {}


def sbeam_select(scores, bias, cum, finished, length, perturbed, draw, state, eos, embed, buffers=None):
    """The vmlmf_sbeam_step launch on checked, contiguous arguments: scores (B W, V) without the bias, eos an int (-1: none).
    lm_sbeam_step's results."""
    B, W = cum.shape
    V = scores.shape[1]
    dev = scores.device
    if buffers is None:
        key = (dev.index, _lib.raw_stream(dev).value, B, W, V)
        if key not in _BUFFERS:
            _BUFFERS[key] = StochasticBeams(B, W, V, dev).buffers()
        buffers = _BUFFERS[key]
    ticket, ws = buffers
    H = embed.shape[1] if embed is not None else 1
    parent, token, total, fin, ln, xn, src = step_outputs(B, W, H, dev, embed)
    pert, drawn = torch.empty_like(total), torch.empty_like(draw)
    LIBRARY.call(dev, "vmlmf_sbeam_step", B, W, H, V, ptr(scores), ptr(bias), ptr(cum), ptr(finished), ptr(length), eos, ptr(embed),
                 ptr(parent), ptr(token), ptr(total), ptr(fin), ptr(ln), ptr(xn), ptr(src), ptr(ticket), ptr(ws), ws.numel() * 8,
                 ptr(perturbed), ptr(pert), ptr(draw), ptr(drawn), ptr(state))
    return parent, token, total, fin, ln, xn, src, pert, drawn
