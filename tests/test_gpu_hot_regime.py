"""GPU parity of every recurrent kernel family with saturated gates and large cell states (tests/hot_cases.py; the conditions are
checked on the CPU by tests/test_hot_regime_cpu.py; docs/design/value_regimes.md): biases at sigma 5 ("hot") or 40 ("rail": pre-activations
past +-88.7, where the fast gates' exp leaves fp32 and the result rests on rcp(inf) = 0), x at sigma 3, c0 at sigma 4.  Against the fp64
literal oracle at the unchanged tolerances of tests/hip_util.py.  Every case proves which family ran it - by the switch it forces, the
library's own plan (vmlmf_query, _stack_plan) and its launch counters - and fails if that is another one than its table names."""
import ctypes
import os

import numpy as np
import pytest
import torch

import hot_cases as HC
from hip_util import ORDER, compare_all, run_hip, run_literal
from vmlmf_amd import _lib
from vmlmf_amd import functional as F

pytestmark = pytest.mark.gpu
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


# ---- one reference per (row, tier), shared by every test that runs the row ---------------------------------------------------------
_REF = {}


def layer_case(row, tier):
    key = (HC.row_id(row), tier)
    if key not in _REF:
        inp = HC.row_inputs(row, tier)
        _REF[key] = (inp, run_literal(row[0], *inp, time_major=row[7]), HC.gate_stats(row[0], *inp[:4], row[7]) if tier == "rail" else None)
    return _REF[key]


WORST = {}


def note(family, sh, tag):
    name, share = HC.worst(sh)
    if share >= WORST.get(family, ("", -1.0))[1]:
        WORST[family] = (f"{tag}.{name}", share)
    print(f"\nhot-regime {family}: worst {WORST[family][0]} {WORST[family][1]:.3f}")


def rail_limits(y, og_low, time_major, tag):
    """The limits the fast gates must reach on the rails: |y| <= 1 everywhere, and y exactly 0 (or below 1e-30) where the output gate's
    pre-activation is below -88.7 at every step (og_low: (row, unit), from the fp64 oracle's pre-activations)."""
    assert np.all(np.isfinite(y)), f"{tag}: y has non-finite values"
    assert np.all(np.abs(y) <= 1.0), f"{tag}: |y| reaches {np.abs(y).max()!r} at {np.unravel_index(np.abs(y).argmax(), y.shape)}"
    assert og_low.any(), f"{tag}: no unit with its output gate below -88.7 at every step"
    cut = (y if time_major else np.swapaxes(y, 0, 1))[:, og_low]
    assert np.all(np.abs(cut) < 1e-30), f"{tag}: y = {np.abs(cut).max()!r} where sigmoid(po) must have reached 0 ({int(og_low.sum())} units)"


def check_layer(got, row, tier, family, tag):
    inp, ref, st = layer_case(row, tier)
    sh = HC.assert_shares(got, ref, f"{tag} {HC.row_id(row)} {tier} (every output and gradient must be finite)")
    compare_all(got, ref, tag)
    if tier == "rail":
        rail_limits(got["y"], st["og_low"], row[7], f"{tag} {HC.row_id(row)}")
    note(family, sh, f"{HC.row_id(row)}.{tier}")
    return sh


def run_layer(row, tier, need_dx=True):
    inp, _, _ = layer_case(row, tier)
    return run_hip(row[0], *inp, time_major=row[7], need_dx=need_dx)


def tiered(rows, tiers_at):
    return [(row, tier) for row in rows for tier in row[tiers_at]]


def ids(v):
    if isinstance(v, tuple) and len(v) >= 10 and isinstance(v[4], int) and isinstance(v[6], list):
        return HC.row_id(v)
    if isinstance(v, tuple):
        return "_".join("x".join(map(str, e)) if isinstance(e, list) else str(e) for e in v if not isinstance(e, (tuple, bool, dict)))
    return str(v)


# ---- register-resident VALU kernels (vmlmf_rec_fwd.inc, vmlmf_rec_bwd.inc, vmlmf_rec3.inc) ---------------------------------------------
VALU_RUNS = [(row, tier, 6) for row, tier in tiered(HC.VALU, 9)] + \
            [(row, tier, mask) for row, tier in tiered(HC.VALU[:HC.VALU_REC3_ROWS], 9) for mask in (0, 7)]


@pytest.mark.parametrize("row,tier,rec3", VALU_RUNS, ids=ids)
def test_register_resident_kernels(row, tier, rec3, switches):
    switches("rec3", rec3)
    assert family_of(row)[0] == "valu", f"{HC.row_id(row)} is planned on {family_of(row)}"
    got, counts = kernel_counts(lambda: run_layer(row, tier))
    assert counts["rec_fwd_kernel"] == 1 and counts["rec_bwd_kernel"] == 1, counts
    check_layer(got, row, tier, "valu", f"valu.rec3={rec3}")


# ---- the headline layer's three backward forms on the same inputs (vmlmf_rec_bwd.inc riding, stand-alone, vmlmf_rec4.inc) ---------------
def _headline_forms(row, tier, switches):
    assert family_of(row)[0] == "valu"
    forms = {}
    switches("inrow", 0)
    switches("wride", 1)
    forms["riding"], c = kernel_counts(lambda: run_layer(row, tier, need_dx=False))
    assert _lib.tune_get("wride") == 1, "the riding workers switched themselves off"
    assert c["rec_bwd_kernel"] == 1 and c["wgrad_mfma_kernel"] == 0 and c["finish2_kernel"] == 1, ("riding", c)
    switches("wride", 0)
    forms["stand-alone"], c = kernel_counts(lambda: run_layer(row, tier, need_dx=False))
    assert c["rec_bwd_kernel"] == 1 and c["wgrad_mfma_kernel"] == 1 and c["finish2_kernel"] == 0, ("stand-alone", c)
    switches("wride", 1)
    switches("inrow", 1)
    forms["in-row"], c = kernel_counts(lambda: run_layer(row, tier, need_dx=False))
    assert c["rec_bwd_kernel"] == 1 and c["wgrad_mfma_kernel"] == 0 and c["dqx_dx_kernel"] == 0 and c["finish2_kernel"] == 0, ("in-row", c)
    return forms


@pytest.mark.parametrize("row,tier", tiered(HC.HEADLINE, 9), ids=ids)
def test_headline_backward_forms(row, tier, switches):
    forms = _headline_forms(row, tier, switches)
    problems = []
    for name, got in forms.items():
        try:
            check_layer(got, row, tier, "headline", name)
        except AssertionError as e:
            problems.append(str(e))
    assert not problems, "\n".join(problems)
    for name in ("stand-alone", "in-row"):       # the recurrence itself is the same arithmetic in every form
        for k in ("y", "dh0", "dc0"):
            if k in forms["riding"]:
                assert np.array_equal(forms["riding"][k], forms[name][k]), f"{k}: riding and {name} differ"


def test_headline_layer_at_full_length():
    """Config A's own length: max |c| beyond 100, where plain fp32 already uses a sizeable part of the outputs' tolerance."""
    row, tier = HC.HEADLINE_FULL, "hot"
    assert family_of(row)[0] == "valu"
    got, counts = kernel_counts(lambda: run_layer(row, tier, need_dx=False))
    assert counts["rec_fwd_kernel"] == 1 and counts["rec_bwd_kernel"] == 1, counts
    check_layer(got, row, tier, "headline", "full-length")


# ---- row-block MFMA kernels (vmlmf_rb.inc), single workgroups and clusters ---------------------------------------------------------------
RB_RUNS = [(row, tier, False, False) for row, tier in tiered(HC.RB, 9)] + [(row, tier, True, False) for row, tier in tiered(HC.RB_CLUSTER, 9)] + \
          [(HC.RB_CLUSTER16, "hot", True, True)]


@pytest.mark.parametrize("row,tier,cluster,sixteen", RB_RUNS, ids=ids)
def test_row_block_kernels(row, tier, cluster, sixteen, switches):
    switches("rb", 1)
    if sixteen:
        switches("rb_cluster", 16)
        switches("rb_rows", 16)
    fam, wgs = family_of(row)
    assert fam == "rb", f"{HC.row_id(row)} is planned on {fam}"
    assert (wgs > (row[1] + 15) // 16) == cluster, f"{wgs} workgroups for {row[1]} rows"
    check_layer(run_layer(row, tier), row, tier, "rb", "rb.cluster16" if sixteen else "rb")


# ---- the step-wise path (vmlmf_generic.hip) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,tier", [(row, tier) for row in HC.STEPWISE for tier in row[9]], ids=ids)
def test_step_wise_path(row, tier, switches):
    for key, value in row[10].items():
        switches(key, value)
    assert family_of(row)[0] == "stepwise", f"{HC.row_id(row)} is planned on {family_of(row)}"
    rings = _lib.tune_get("wring_launches")
    got = run_layer(row, tier)
    if row[10].get("wring") == 1:
        assert _lib.tune_get("wring_launches") > rings, "the weight gradients did not go through the LDS ring"
    check_layer(got, row, tier, "stepwise", "stepwise")


# ---- stacks: clustered layers in one launch (vmlmf_rbx.hip) and the wavefront launches (vmlmf_wave.inc) ------------------------------------
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
    loss = (y * torch.tensor(dy, device=DEV)).sum()
    for l in range(L):
        loss = loss + (hs[l] * torch.tensor(dhT[l], device=DEV)).sum() + (cs[l] * torch.tensor(dcT[l], device=DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    res = {"y": y.detach().cpu().numpy(), "hT": [h.detach().cpu().numpy() for h in hs], "cT": [c.detach().cpu().numpy() for c in cs],
           "dx": xg.grad.cpu().numpy(), "G": [{k: p.grad.cpu().numpy() for k, p in zip(names, params[l])} for l in range(L)]}
    if h0g is not None:
        res["dh0"], res["dc0"] = list(h0g.grad.cpu().numpy()), list(c0g.grad.cpu().numpy())
    return res


def check_stack(variant, inp, rw, ru, time_major, clustered, tier, family, tag):
    got = run_stack(variant, *inp, rw, ru, time_major, clustered)
    ref = HC.run_stack_literal(variant, *inp, time_major)
    sh = HC.assert_shares(got, ref, f"{tag} {tier} (every output and gradient must be finite)", may_lack=())
    if tier == "rail":
        rail_limits(got["y"], HC.stack_gate_stats(variant, *inp[:4], time_major)["og_low"], time_major, tag)
    note(family, sh, f"{tag}.{tier}")


@pytest.mark.parametrize("row,tier", tiered(HC.RBX, 4), ids=ids)
def test_clustered_stacks_in_one_launch(row, tier):
    v = row[0]
    check_stack(v, HC.rbx_inputs(row, tier), HC.RBX_RW, HC.rbx_ranks(v), True, True, tier, "rbx", "rbx.v%d.L%d.B%d.T%d" % row[:4])


@pytest.mark.parametrize("row,tier", tiered(HC.WAVE, 8), ids=ids)
def test_wavefront_stacks(row, tier):
    v, B, T, I, Hs, rw, ru = row[:7]
    check_stack(v, HC.wave_inputs(row, tier), rw, ru, False, False, tier, "wave", "wave.v%d.B%d.T%d.I%d.H%s" % (v, B, T, I, "_".join(map(str, Hs))))
