"""ctypes binding of the C ABI in include/vmlmf_sbeam.h (libvmlmf_sbeam.so, built in-tree by csrc/Makefile beside
libvmlmf_hip.so): the step of stochastic beam search of the LM decoder - Model.stochastic_beam_search.  The library is loaded on the
first stochastic step: generate(), beam_search(), score(), contrastive_search(), cache_score() and a training process never open it.

There is no fallback: if the library is missing, or a call fails, this raises.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._beam import BeamPolicy, _require, check_beams, check_step, check_step_controls, launch_step, new_step_buffers
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


class StochasticBeams(BeamPolicy):
    """Stochastic beam search (Kool, van Hoof and Welling) over B batch rows of W beams and a V-token vocabulary on `device` as a beam
    policy: lm_beam_step(controls=), decoding.beam_steps and BeamGraph(controls=) take it as they take BeamControls.  It carries the
    beams' perturbed values and the steps drawn so far (`carried` is ("perturbed", "draw")); select() is the step's ONE launch
    (vmlmf_sbeam_step) on `state`, the {seed, offset} snapshot every step draws from - None until whoever builds the object for a
    search sets it.  start() gives a search's first (cum, finished, length, perturbed, draw): beam 0 of a row at total 0 and perturbed
    value 0, the others at -inf, no step drawn.  It owns a ticket and a workspace (buffers(): created on the first call, so a CPU
    object costs nothing and opens no library).  ValueError for what check_sbeam refuses, before any device work."""

    carried = ("perturbed", "draw")

    def __init__(self, B, W, V, device):
        super().__init__(B, W, V, device)
        if self.B < 1:
            raise ValueError(f"vmlmf_amd: StochasticBeams needs B >= 1 batch rows, got {B}")
        self.state = None
        self._buffers = None

    def start(self):
        """(cum, finished, length, perturbed, draw) of a search that starts."""
        return (*self.first_beams(), *self.first_carried())

    def first_carried(self):
        """[perturbed, draw] of a search that starts: start()'s last two."""
        return [self.first_beams()[0], torch.zeros(self.B, dtype=torch.int32, device=self.device)]

    def new_buffers(self):
        """A (ticket, workspace) pair sized by vmlmf_sbeam_workspace_bytes: half as much again as the plain step's."""
        return new_step_buffers(self.device, self.B, self.W, self.V, LIBRARY)

    def buffers(self):
        """(ticket (B) int32 - zero, and left zero by every launch -, workspace): this object's own, so its launches never meet
        another search's on one ticket.  Not to be created inside a stream capture (a graph's warm-up creates them)."""
        if self._buffers is None:
            self._buffers = self.new_buffers()
        return self._buffers

    def select(self, scores, bias, cum, finished, length, eos, embed, buffers=None, perturbed=None, draw=None):
        """lm_beam_step's selection by perturbed values (sbeam_select on `state`): the seven results, the survivors' perturbed, draw + 1.
        RuntimeError while `state` is None."""
        if self.state is None:
            raise RuntimeError("vmlmf_amd: this StochasticBeams has no `state` yet: set the {seed, offset} snapshot (dropout_advance()) "
                               "its steps draw from")
        if buffers is not None:         # (a pair of new_buffers() is sized for B, W, V; the stream's default is sized for the step's own)
            check_step_controls(self, StochasticBeams, *cum.shape, scores.shape[1], scores.device, eos)
        _check_noise("lm_beam_step", cum, perturbed, draw, self.state)
        return sbeam_select(scores, bias, cum, finished, length, perturbed.contiguous(), draw.contiguous(), self.state.contiguous(), eos,
                            embed, buffers)


def _check_noise(caller, cum, perturbed, draw, state):
    """RuntimeError unless perturbed is (B, W) fp32 like cum, draw (B) int32 and state two int64, all on a HIP device."""
    B, W = cum.shape
    _require(perturbed, "perturbed")
    if tuple(perturbed.shape) != (B, W) or tuple(draw.shape) != (B,):
        raise RuntimeError(f"vmlmf_amd.{caller}: finished, length and perturbed must be (B, W) like cum, draw (B)")
    _require(draw, "draw", torch.int32)
    if not (isinstance(state, torch.Tensor) and state.is_cuda and state.dtype == torch.int64 and state.numel() == 2):
        raise RuntimeError(f"vmlmf_amd.{caller}: state must be a {{seed, offset}} snapshot: two int64 on the device")


def lm_sbeam_step(h, weight, bias, cum, finished, length, perturbed, draw, state, eos, embed=None, buffers=None):
    """One step of stochastic beam search over B batch rows of W beams (cum is (B, W)): the head's GEMM over the beams' top-layer
    outputs h (B W, H) - row b W + w is beam w of batch row b -, then ONE launch (vmlmf_sbeam_step, csrc/vmlmf_sbeam.hip; include/
    vmlmf_sbeam.h has the contract): every candidate's total phi = cum[b, w] + log_softmax(h fc.w^T + bias)[v] in fp32 with
    lm_beam_step's bits, perturbed by the sampler's Gumbel noise at position draw[b] B W + b W + w, conditioned top-down on the
    parent's perturbed value; the W candidates of each batch row with the largest perturbed values survive, in that order.
    perturbed (B, W) fp32: the beams' perturbed values; draw (B) int32: the steps taken so far; state: a {seed, offset} snapshot of
    dropout_advance() - two int64 on the device; finished, length, eos, embed: lm_beam_step's.
    Returns lm_beam_step's seven results (parent, token, total, finished, length, x_next, src_row) and behind them the survivors'
    perturbed (B, W) and draw + 1 (B), fresh buffers.  buffers: (ticket, workspace) of a StochasticBeams.buffers() - default: the
    current stream's (step_buffers, sized by this library)."""
    h2, w, bias, cum, finished, length, eos_c, embed = check_step("lm_sbeam_step", h, weight, bias, cum, finished, length, eos, embed)
    _check_noise("lm_sbeam_step", cum, perturbed, draw, state)
    return sbeam_select(torch.mm(h2, w.t()), bias, cum, finished, length, perturbed.contiguous(), draw.contiguous(), state.contiguous(),
                        eos_c, embed, buffers)


def sbeam_select(scores, bias, cum, finished, length, perturbed, draw, state, eos, embed, buffers=None):
    """The vmlmf_sbeam_step launch on checked, contiguous arguments: scores (B W, V) without the bias, eos an int (-1: none).
    lm_sbeam_step's results."""
    pert, drawn = torch.empty_like(perturbed), torch.empty_like(draw)
    outs = launch_step(LIBRARY, "vmlmf_sbeam_step", scores, bias, cum, finished, length, eos, embed, buffers, sized_by=LIBRARY,
                       behind=(ptr(perturbed), ptr(pert), ptr(draw), ptr(drawn), ptr(state)))
    return (*outs, pert, drawn)
