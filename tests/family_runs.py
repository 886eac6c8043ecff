"""What the GPU tests of the recurrent kernel families share (tests/test_gpu_hot_regime.py, test_gpu_structure.py, test_gpu_slices.py):
the kernel-selection switches as a fixture, the library's own plan and launch counters that prove which family ran a case, and the run
of a stack through vmlmf_stack.  Helpers only: no test lives here."""
import ctypes
import os

import numpy as np
import pytest
import torch

import hot_cases as HC
from hip_util import ORDER, run_hip
from vmlmf_amd import _lib
from vmlmf_amd import functional as F

DEV = "cuda"
SWITCH_DEFAULTS = {"rb": -1, "rb_cluster": 0, "rb_rows": 0, "rec3": 6, "wride": 1, "inrow": -1, "wring": -1}


@pytest.fixture
def switches():
    """Set kernel-selection switches for one case; every one goes back to its default afterwards."""
    touched = []

    def tune(key, value):
        touched.append(key)
        _lib.tune(key, value)
    yield tune
    for key in touched:
        _lib.tune(key, SWITCH_DEFAULTS[key])


def kernel_counts(fn):
    """Launch counts of the library's internal kernels while fn() runs (vmlmf_profile_*)."""
    lib = _lib.lib()
    usec = (ctypes.c_float * _lib.NKERNELS)()
    cnt = (ctypes.c_int32 * _lib.NKERNELS)()
    lib.vmlmf_profile_enable((1 << _lib.NKERNELS) - 1)
    try:
        out = fn()
        torch.cuda.synchronize()
        lib.vmlmf_profile_read(usec, cnt, 1)
    finally:
        lib.vmlmf_profile_enable(0)
    return out, {lib.vmlmf_kernel_name(k).decode(): cnt[k] for k in range(_lib.NKERNELS)}


def family_of(row):
    """The family the library plans for a layer under the current switches: "rb" (row blocks; with the workgroup count), "stepwise" or
    "valu"."""
    v, B, T, I, H, rw, ru, tm = row[:8]
    g = 2 if v in HC.GROUPED else 1
    s = _lib.query(_lib.make_desc(v, B, T, I, H, rw, ru, g=g, time_major=tm, training=True))
    if s.rows_per_wg in (4, 8, 16):
        return "rb", s.workgroups
    slots = g * ((H // g + 63) // 64) * 64
    return ("stepwise" if s.kh > 32 or slots > 512 or I > H else "valu"), s.workgroups


def headline_forms(row, switches, run):
    """The headline layer's three backward forms on the same input - riding workers, stand-alone weight gradients, in-row - each proven by
    its launch counts.  run(): one forward and backward with need_dx=False.  Returns {form: result}."""
    assert family_of(row)[0] == "valu"
    forms = {}
    switches("inrow", 0)
    switches("wride", 1)
    forms["riding"], c = kernel_counts(run)
    assert _lib.tune_get("wride") == 1, "the riding workers switched themselves off"
    assert c["rec_bwd_kernel"] == 1 and c["wgrad_mfma_kernel"] == 0 and c["finish2_kernel"] == 1, ("riding", c)
    switches("wride", 0)
    forms["stand-alone"], c = kernel_counts(run)
    assert c["rec_bwd_kernel"] == 1 and c["wgrad_mfma_kernel"] == 1 and c["finish2_kernel"] == 0, ("stand-alone", c)
    switches("wride", 1)
    switches("inrow", 1)
    forms["in-row"], c = kernel_counts(run)
    assert c["rec_bwd_kernel"] == 1 and c["wgrad_mfma_kernel"] == 0 and c["dqx_dx_kernel"] == 0 and c["finish2_kernel"] == 0, ("in-row", c)
    return forms


def run_layer_as(family, row, held, switches, P, inp, backward=True):
    """One layer case on the family its table names, proven by the switches it forces (held), the library's plan and its launch counters.
    inp: x, h0, c0, dy, dhT, dcT.  Returns {form: result of run_hip}: one form per family, but for "headline" its three backward forms
    (need_dx=False) and, as "with-dx", the default form with a gradient for x.  backward=False: the forward alone, one form."""
    v, B, tm = row[0], row[1], row[7]
    for key, value in held.items():
        switches(key, value)
    fam, wgs = family_of(row)
    kind = family.split(".")[0]
    tag = f"{HC.row_id(row)} is planned on {(fam, wgs)}, not on {family}"

    def run(need_dx=True):
        return run_hip(v, P, *(inp if backward else inp[:3]), time_major=tm, need_dx=need_dx)
    if kind in ("valu", "headline"):
        assert fam == "valu", tag
        got, counts = kernel_counts(run)
        assert counts["rec_fwd_kernel"] == 1 and (counts["rec_bwd_kernel"] == 1 or not backward), counts
        if kind == "valu" or not backward:
            return {family: got}
        forms = headline_forms(row, switches, lambda: run(need_dx=False))
        forms["with-dx"] = got
        return forms
    if kind in ("rb", "rb_cluster", "rb_cluster16"):
        assert fam == "rb" and (wgs > (B + 15) // 16) == (kind != "rb"), tag
        return {family: run()}
    assert kind == "stepwise" and fam == "stepwise", tag
    rings = _lib.tune_get("wring_launches")
    got = run()
    if held.get("wring") == 1 and backward:
        assert _lib.tune_get("wring_launches") > rings, "the weight gradients did not go through the LDS ring"
    return {family: got}


def run_stack(variant, Ps, x, h0, c0, dy, dhT, dcT, rw, ru, time_major, clustered):
    g = 2 if variant in HC.GROUPED else 1
    L, names = len(Ps), ORDER[variant]
    T, B, I = (x.shape[0], x.shape[1], x.shape[2]) if time_major else (x.shape[1], x.shape[0], x.shape[2])
    Hs = [HC.O.hidden_size_of(variant, P) for P in Ps]
    cfg = F._layer_cfg(variant, g, rw, ru, time_major, "f32")
    Hp = Hs[0] if len(set(Hs)) == 1 else tuple(Hs)
    assert F._stack_plan(cfg, L, B, T, I, Hp, True) is not None, "the stack entry point does not cover this stack"
    # the two forms behind vmlmf_stack_* divide the layers between them (include/vmlmf_hip.h): clusters of row-block workgroups for
    # layers beyond one CU, the wavefront kernels for layers of at most four waves of units - told apart by the layer's own plan
    fam = family_of((variant, B, T, Hs[-2] if L > 1 else I, Hs[-1], rw, ru, time_major))[0]
    assert fam == ("rb" if clustered else "valu"), f"the stack's layers are planned on {fam}: the other stack family"
    if clustered:
        assert F.stack_takes_dropout(cfg, L, B, T, I, Hp, True)
    params = [[torch.tensor(np.asarray(P[k]), device=DEV).requires_grad_(True) for k in names] for P in Ps]
    xg = torch.tensor(x, device=DEV).requires_grad_(True)
    h0g = None if h0 is None else torch.tensor(np.stack(h0), device=DEV).requires_grad_(True)
    c0g = None if c0 is None else torch.tensor(np.stack(c0), device=DEV).requires_grad_(True)
    os.environ["VMLMF_STACK"] = "1"
    try:
        out = F.vmlmf_stack(variant, xg, params, rw, ru, g=g, time_major=time_major, h0=h0g, c0=c0g)
    finally:
        os.environ.pop("VMLMF_STACK", None)
    assert out is not None, "vmlmf_stack declined the stack"
    y, hs, cs = out[:3]
    res = {"y": y.detach().cpu().numpy(), "hT": [h.detach().cpu().numpy() for h in hs], "cT": [c.detach().cpu().numpy() for c in cs]}
    if dy is None and dhT is None and dcT is None:         # the forward alone
        torch.cuda.synchronize()
        return res
    loss = 0.0 if dy is None else (y * torch.tensor(dy, device=DEV)).sum()
    for l in range(L):
        loss = loss + (hs[l] * torch.tensor(dhT[l], device=DEV)).sum() + (cs[l] * torch.tensor(dcT[l], device=DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    res.update({"dx": xg.grad.cpu().numpy(), "G": [{k: p.grad.cpu().numpy() for k, p in zip(names, params[l])} for l in range(L)]})
    if h0g is not None:
        res["dh0"], res["dc0"] = list(h0g.grad.cpu().numpy()), list(c0g.grad.cpu().numpy())
    return res
