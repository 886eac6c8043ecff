"""ctypes binding of the C ABI in include/vmlmf_beamgroup.h (libvmlmf_beamgroup.so, built in-tree by csrc/Makefile beside
libvmlmf_hip.so): the step of diverse (group) beam search of the LM decoder - Model.group_beam_search.  The library is loaded on the
first group step: beam_search(), generate(), score() and a training process never open it.

There is no fallback: if the library is missing, or a call fails, this raises.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from ._beam import BeamPolicy, check_beams, check_step_controls, launch_step

ABI_VERSION = 1

# every symbol include/vmlmf_beamgroup.h declares: (restype, argtypes)
_vp, _sz, _i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
SYMBOLS = {
    "vmlmf_beamgroup_abi_version": (_i, []),
    "vmlmf_beamgroup_last_error": (ctypes.c_char_p, []),
    "vmlmf_beamgroup_workspace_bytes": (_sz, [_i, _i, _i]),
    "vmlmf_beamgroup_step": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i,
                                  ctypes.c_float, _vp]),
}

LIBRARY = _lib.Library("beamgroup", SYMBOLS, ABI_VERSION, "stock-op fallback for the group beam-search step")
lib, loaded, check = LIBRARY.handle, LIBRARY.loaded, LIBRARY.check


def check_groups(beams, groups, diversity_penalty, V=None):
    """(W, G, lambda) as the C ABI takes them; ValueError for what check_beams refuses, for groups < 1, for groups that do not divide
    beams and for a diversity_penalty that is negative or not finite."""
    W = check_beams(beams, V)
    G = int(groups)
    if G < 1:
        raise ValueError(f"vmlmf_amd: groups must be >= 1, got {groups}")
    if W % G != 0:
        raise ValueError(f"vmlmf_amd: groups={G} must divide beams={W}: a group owns beams / groups slots")
    lam = float(diversity_penalty)
    if not (math.isfinite(lam) and lam >= 0.0):
        raise ValueError(f"vmlmf_amd: diversity_penalty must be finite and >= 0, got {diversity_penalty}")
    return W, G, lam


def group_start(B, W, groups, device):
    """(cum, finished, length), each (B, W), of a group search that starts: the first slot g W / G of every group at score 0, the
    others at -inf."""
    W, G, _ = check_groups(W, groups, 0.0)
    cum = torch.full((B, W), float("-inf"), device=device)
    cum[:, ::W // G] = 0.0
    return cum, torch.zeros((B, W), dtype=torch.int32, device=device), torch.zeros((B, W), dtype=torch.int32, device=device)


class GroupBeams(BeamPolicy):
    """The grouping of one diverse beam search (Vijayakumar et al.) over B batch rows of W beams and a V-token vocabulary on `device`
    (include/vmlmf_beamgroup.h): `groups` = G divides W, group g owns slots g W / G .. (g + 1) W / G - 1 of a row and keeps the best of
    its own beams' candidates under total - diversity_penalty n, n the number of survivors the groups before it chose in this step with
    the same token; the totals stay raw, so `scores` stay sums of plain log-probabilities.  It carries nothing from step to step
    (`carried` is (), first_carried() is []) and owns no state; select() is the step's ONE launch (vmlmf_beamgroup_step), so
    lm_beam_step(controls=), decoding.beam_steps and BeamGraph(controls=) take it as they take BeamControls.  start() gives a search's
    first (cum, finished, length).  ValueError for what check_groups refuses, before any device work."""

    def __init__(self, B, W, V, device, groups=2, diversity_penalty=0.5):
        super().__init__(B, W, V, device)
        _, self.groups, self.diversity_penalty = check_groups(self.W, groups, diversity_penalty, self.V)

    def start(self):
        """(cum, finished, length) of a search that starts (group_start)."""
        return group_start(self.B, self.W, self.groups, self.device)

    first_beams = start

    def select(self, scores, bias, cum, finished, length, eos, embed, buffers=None):
        """lm_beam_step's selection in groups (group_select)."""
        return group_select(scores, bias, cum, finished, length, eos, embed, self, buffers)


def group_select(scores, bias, cum, finished, length, eos, embed, controls, buffers=None):
    """The vmlmf_beamgroup_step launch on checked, contiguous arguments (scores (B W, V) without the bias, eos an int, -1: none).
    lm_beam_step's seven results."""
    check_step_controls(controls, GroupBeams, *cum.shape, scores.shape[1], scores.device, eos)
    return launch_step(LIBRARY, "vmlmf_beamgroup_step", scores, bias, cum, finished, length, eos, embed, buffers,
                       behind=(controls.groups, controls.diversity_penalty))
