"""The slice-wise gradient rule (tests/hip_util.py::assert_grad_slices; docs/design/slice_tolerances.md) checked without a GPU: it sees
errors the whole-tensor rule cannot, its map of gate and group blocks is the oracle's own, and every input the GPU slice tests use
(tests/slice_cases.py) is one plain fp32 can be held to - the fp32 literal oracle against itself in fp64 stays within a third of the slice
tolerance on every slice, and no slice is so small that it would be skipped.  The oracle is what is measured here, never the kernels."""
import numpy as np
import pytest
import torch

import hot_cases as HC
import slice_cases as SC
import vmlmf_oracle as O
from hip_util import ORDER, TINY, assert_grad, assert_grad_slices, compare_all, compare_slices, run_literal, slice_cuts, slice_report

# ---- (a) mutants of the fp32 oracle's result that the whole-tensor rule passes and the slice rule must catch -----------------------------
DECAY = (O.V1, 7, 41, 16, 64, 8, [8], False, True, HC.HOT)                # dhT only: max |dx[t]| falls from 1e-1 to 1e-10 towards t = 0
GROUPS = (O.V2, 3, 6, 10, 136, 8, [16, 8], False, True, HC.HOT)


def _pair(row, pattern, inputs=None):
    inp = inputs or SC.ordinary_inputs(row, pattern)
    got = run_literal(row[0], *inp, time_major=row[7], dtype=torch.float32)
    ref = run_literal(row[0], *inp, time_major=row[7])
    return got, ref


_PAIRS = {}


def pair(name):
    if name not in _PAIRS:
        if name == "decay":
            _PAIRS[name] = (DECAY,) + _pair(DECAY, "last")
        elif name == "rows":
            _PAIRS[name] = (DECAY,) + _pair(DECAY, "rows")
        else:
            # upstream gradient on the last state alone, the units of group 0 at a twentieth of group 1's: u_h_1[j] feeds destination group j,
            # so its two group blocks then differ in size like the rows of a weighted batch do
            P, x, h0, c0, _, dhT, dcT = SC.ordinary_inputs(GROUPS, "last")
            w = np.where(np.arange(GROUPS[4]) < GROUPS[4] // 2, np.float32(0.05), np.float32(1.0))
            _PAIRS[name] = (GROUPS,) + _pair(GROUPS, None, (P, x, h0, c0, None, dhT * w, dcT * w))
    return _PAIRS[name]


def _cuts(row, name, arr):
    return slice_cuts(name, np.shape(arr), row[0], row[4], SC._g(row[0]), row[7])


def _dx_first_step(got, ref, row):
    got["dx"][:, 0] *= 1.01
    return "dx"


def _dx_first_half_zero(got, ref, row):
    got["dx"][:, :row[2] // 2] = 0
    return "dx"


def _forget_block_of_b_x(got, ref, row):
    H = row[4]
    got["G"]["b_x"][H:2 * H] *= np.float32(1 + 5e-4)       # b_x.chunk(4, 1) is (i, f, o, n): literal_step
    return "G.b_x"


def _smallest_row_of_dh0(got, ref, row):
    got["dh0"][row[1] - 1] = 0                              # row B - 1 carries 1e-6 of row 0's upstream gradient
    return "dh0"


def _one_group_of_u_h_1(got, ref, row):
    g = int(np.argmin([np.abs(ref["G"]["u_h_1"][j]).max() for j in range(2)]))
    got["G"]["u_h_1"][g] *= np.float32(1 + 5e-4)
    return "G.u_h_1"


MUTANTS = [("decay", _dx_first_step), ("decay", _dx_first_half_zero), ("decay", _forget_block_of_b_x), ("rows", _smallest_row_of_dh0),
           ("groups", _one_group_of_u_h_1)]


def _get(res, name):
    return res["G"][name[2:]] if name.startswith("G.") else res[name]


@pytest.mark.parametrize("case,mutate", MUTANTS, ids=[f"{c}-{m.__name__.strip('_')}" for c, m in MUTANTS])
def test_the_slice_rule_sees_what_the_whole_tensor_rule_cannot(case, mutate):
    row, got, ref = pair(case)
    got = {k: ({kk: vv.copy() for kk, vv in v.items()} if k == "G" else v.copy()) for k, v in got.items()}
    name = mutate(got, ref, row)
    a, b = _get(got, name), _get(ref, name)
    assert not np.array_equal(a, _get(pair(case)[1], name)), "the mutant changed nothing"
    assert_grad(a, b, name)                               # the gap: today's rule passes the mutant
    with pytest.raises(AssertionError, match="worst slice"):
        assert_grad_slices(a, b, name, _cuts(row, name.split(".")[-1], b))
    with pytest.raises(AssertionError, match="worst slice"):
        compare_all(got, ref, "mutant", slices=SC.layout(row[0], row[4], row[7]))
    compare_all(got, ref, "mutant")                       # slices=None is today's behaviour


@pytest.mark.parametrize("case", ["decay", "rows", "groups"])
def test_the_unmutated_fp32_oracle_passes_both_rules(case):
    row, got, ref = pair(case)
    compare_all(got, ref, case)
    rep = compare_all(got, ref, case, slices=SC.layout(row[0], row[4], row[7]))
    assert rep["skipped"] == 0 and rep["worst"][1] <= HC.FP32_SHARE, rep
    print(f"\n{case}: fp32 oracle worst slice {rep['worst'][0]} {rep['worst'][1]:.4f} x tolerance")


def test_the_decaying_case_has_steps_the_whole_tensor_rule_cannot_see():
    row, got, ref = pair("decay")
    per_step = np.abs(ref["dx"]).max(axis=(0, 2))
    hidden = int((per_step < 1e-4 * per_step.max()).sum())
    print(f"\nmax |dx[t]| from {per_step[-1]:.1e} (last step) down to {per_step[0]:.1e} (first); {hidden} of {row[2]} steps below 1e-4 of the maximum")
    assert hidden >= row[2] // 2 and per_step.min() > TINY


def test_the_rule_is_the_suites_gradient_tolerance():
    import hip_util
    import slice_rule
    assert slice_rule.GREL == hip_util.GREL == 1e-4 and slice_rule.TINY == TINY == 2.0 ** -100
    assert hip_util.slice_cuts is slice_rule.slice_cuts and hip_util.slice_report is slice_rule.slice_report


def test_tiny_slices_are_skipped_and_counted_and_the_message_names_the_worst_slice():
    b = np.ones((3, 4))
    b[1] = 2.0 ** -101
    a = b.copy()
    a[1] = 0.0
    assert assert_grad_slices(a, b, "t", [0]) == 1
    a[2, 3] += 3e-4
    with pytest.raises(AssertionError, match=r"axes \(0,\) index \(2,\).* 3 x its tolerance"):
        assert_grad_slices(a, b, "t", [0])
    assert slice_report(a, b, [[("left", (slice(None), slice(0, 2))), ("right", (slice(None), slice(2, 4)))]])[0] == "right"
    with pytest.raises(AssertionError, match="non-finite"):
        assert_grad_slices(np.full((3, 4), np.nan), b, "t", [0])
    with pytest.raises(AssertionError):          # no absolute floor: an error of 1e-9 in a slice of size 1e-6 is 1e-3 of it
        assert_grad_slices(np.array([[1e-6 + 1e-9], [1.0]]), np.array([[1e-6], [1.0]]), "t", [0])


# ---- (b) the map of gate and group blocks is the oracle's own --------------------------------------------------------------------------------
LAYOUT_ROWS = [(O.V1, 3, 3, 5, 12, 3, [4], False, True), (O.V2, 3, 3, 5, 12, 3, [4, 2], False, True), (O.V3, 3, 3, 12, 12, 3, [4], True, True),
               (O.V4, 3, 3, 12, 12, 3, [4, 2], True, True), (O.V6, 3, 3, 5, 12, 3, [4, 2], False, True)]


def _single_gate_gradients(row, gate):
    """The fp64 oracle's parameter gradients when only the pre-activation gradient of one gate (0..3 = i, f, o, n of O._lstm_tail) is let
    through at every step: O._lstm_tail is wrapped so that the other three gates' pre-activations pass no gradient back."""
    plain = O._lstm_tail

    def tail(*pre_and_c):
        pre = [p if k == gate else p.detach() for k, p in enumerate(pre_and_c[:4])]
        return plain(*pre, pre_and_c[4])
    O._lstm_tail = tail
    try:
        return run_literal(row[0], *SC.ordinary_inputs(row), time_major=row[7])["G"]
    finally:
        O._lstm_tail = plain


@pytest.mark.parametrize("row", LAYOUT_ROWS, ids=lambda r: f"v{r[0]}")
def test_every_block_of_the_map_belongs_to_exactly_one_gate(row):
    v, H, g = row[0], row[4], SC._g(row[0])
    runs = [_single_gate_gradients(row, gate) for gate in range(4)]
    seen = 0
    for name in ORDER[v]:
        cuts = slice_cuts(name, runs[0][name].shape, v, H, g, row[7])
        if cuts is None or not isinstance(cuts[-1], list):  # u_h_s is cut per group only: every gate reaches every group
            continue
        blocks = cuts[-1]                                  # the gate blocks (the cut before it, where there is one, is per group)
        covered = np.zeros(runs[0][name].shape, int)
        for label, idx in blocks:
            covered[idx] += 1
            touched = [gate for gate in range(4) if np.any(runs[gate][name][idx] != 0)]
            assert len(touched) == 1, f"v{v} {name} {label}: touched by the gates {touched}"
            full = runs[touched[0]][name][idx]
            assert np.all(full != 0), f"v{v} {name} {label}: gate {touched[0]} leaves part of the block untouched"
        assert np.all(covered == 1), f"v{v} {name}: the blocks do not tile the tensor"
        per_gate = [sum(bool(np.any(runs[gate][name][idx] != 0)) for _, idx in blocks) for gate in range(4)]
        assert len(set(per_gate)) == 1 and per_gate[0] * 4 == len(blocks), (name, per_gate)
        seen += 1
    bias = "bias_x" if v in (O.V2, O.V6) else "b_x"
    for gate in range(4):                                  # the issue's own statement: one block of b_x, the other three exactly zero
        blocks = slice_cuts(bias, runs[gate][bias].shape, v, H, g, row[7])[0]
        assert sum(bool(np.any(runs[gate][bias][idx] != 0)) for _, idx in blocks) == 1
    assert seen >= 4


def test_the_map_names_the_tensors_the_rule_is_asked_for():
    for v, names in ORDER.items():
        row = (v, 3, 3, 12, 12, 3, [4, 2] if v in HC.GROUPED else [4])
        P = O.make_params(v, 12, 12, 3, row[6] if v in HC.GROUPED else 4)
        for name in names:
            cuts = slice_cuts(name, P[name].shape, v, 12, SC._g(v))
            sliced = v != O.V5 and (name in ("v_x", "v_h", "w_x", "w_h", "b_x", "b_h", "bias_x", "bias_h") or name[:4] in ("u_h_", "v_h_", "u_h.", "v_h."))
            assert (cuts is not None) == sliced, (v, name, cuts)
            if name[:4] in ("u_h_", "u_h.", "v_h_", "v_h."):
                assert cuts[0] == 0 and (len(cuts) == 2) == name.startswith("v"), (v, name, cuts)
    assert slice_cuts("dx", (3, 4, 5), O.V1, 12) == [0, 1] and slice_cuts("dh0", (3, 12), O.V1, 12) == [0]


# ---- (c) every input of the GPU slice tests is within reach of plain fp32 ----------------------------------------------------------------
@pytest.mark.parametrize("case,pattern", SC.GPU_LAYER_CASES + SC.GPU_STACK_CASES, ids=SC.case_id)
def test_gpu_slice_cases_are_admissible(case, pattern):
    rep = SC.fp32_slice_report(case, pattern)
    print(f"\n{SC.case_id((case, pattern))}: fp32 oracle worst slice {rep['worst'][0]} {rep['worst'][1]:.4f} x tolerance, {rep['skipped']} skipped")
    assert rep["skipped"] == 0, rep
    assert rep["worst"][1] <= HC.FP32_SHARE, rep


def test_the_case_tables_cover_every_family_in_both_patterns():
    fams = {"valu", "headline", "rb", "rb_cluster", "rb_cluster16", "stepwise", "rbx", "wave"}
    for pattern in SC.PATTERNS:
        assert {c[0].split(".")[0] for c, p in SC.GPU_LAYER_CASES + SC.GPU_STACK_CASES if p == pattern} == fams, pattern
    assert all(c[1][2] <= 24 for c in SC.LAST_LAYERS if c[1] in SC.LONG.values())
    rows = [c[1] for c in SC.ROWS_LAYERS]
    for table in (HC.VALU, HC.HEADLINE, HC.RB, HC.RB_CLUSTER, [r[:10] for r in HC.STEPWISE]):
        assert all(r in rows for r in table if r[1] >= 2)


# ---- the bit comparison of tests/test_gpu_structure.py, on made-up results ---------------------------------------------------------------------
def test_the_structural_tests_compare_bits_rows_and_steps():
    import test_gpu_structure as S
    assert S.probe_rows(2) == [0, 1] and S.probe_rows(6) == [0, 5] and S.probe_rows(7) == [0, 5, 6] and S.probe_rows(40) == [0, 5, 16, 39]
    y = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)          # time-major: (T, B, H)
    base = {"f": {"y": y, "hT": [y[0], y[1]]}}
    S.same_bits(base, {"f": {"y": y.copy(), "hT": [y[0].copy(), y[1].copy()]}}, ("y", "hT"), True, "same")
    other = {"f": {"y": y.copy(), "hT": [y[0].copy(), y[1].copy()]}}
    other["f"]["y"][1, 2, 0] = np.float32(1e-45) + y[1, 2, 0] * np.float32(1 + 2 ** -23)      # one ulp, step 1, row 2
    S.same_bits(base, other, ("y",), True, "other rows", rows=[0, 1])
    S.same_bits(base, other, ("y",), True, "earlier steps", steps=slice(0, 1))
    with pytest.raises(AssertionError, match="1 of 4 values changed bits"):
        S.same_bits(base, other, ("y",), True, "that row", rows=[2], steps=slice(1, None))
    zero = {"f": {"y": np.zeros((2, 3, 4), np.float32)}}
    with pytest.raises(AssertionError, match="changed bits"):              # -0.0 is not +0.0
        S.same_bits(zero, {"f": {"y": -zero["f"]["y"]}}, ("y",), True, "signed zero")
    other["f"]["hT"][1][2, 3] += 1
    with pytest.raises(AssertionError, match=r"f.hT\[1\]"):
        S.same_bits(base, other, ("hT",), True, "a layer's state", rows=[2])
    assert S.cut(y, "y", False, rows=[1]).shape == (1, 3, 4) and S.cut(y, "y", False, steps=slice(0, 2)).shape == (2, 2, 4)
