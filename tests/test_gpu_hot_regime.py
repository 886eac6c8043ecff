"""GPU parity of every recurrent kernel family with saturated gates and large cell states (tests/hot_cases.py; the conditions are
checked on the CPU by tests/test_hot_regime_cpu.py; docs/design/value_regimes.md): biases at sigma 5 ("hot") or 40 ("rail": pre-activations
past +-88.7, where the fast gates' exp leaves fp32 and the result rests on rcp(inf) = 0), x at sigma 3, c0 at sigma 4.  Against the fp64
literal oracle at the unchanged tolerances of tests/hip_util.py.  Every case proves which family ran it - by the switch it forces, the
library's own plan (vmlmf_query, _stack_plan) and its launch counters - and fails if that is another one than its table names."""
import numpy as np
import pytest

import hot_cases as HC
from family_runs import family_of, headline_forms, kernel_counts, run_stack, switches  # noqa: F401  (switches is a fixture)
from hip_util import compare_all, run_hip, run_literal
from vmlmf_amd import _lib

pytestmark = pytest.mark.gpu
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
    return headline_forms(row, switches, lambda: run_layer(row, tier, need_dx=False))


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
