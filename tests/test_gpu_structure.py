"""GPU: two exact properties of every recurrent kernel family, and exact zeros (docs/design/slice_tolerances.md).  The rows of a batch are
independent and time is causal, so a hand-off race, a tile that reads its neighbour's row or a tape slot read one step early changes bits
these tests hold fixed - whether or not the result stays inside a tolerance.  Every comparison is on bits (uint32 views: -0.0 is not +0.0);
each case first runs its base input twice, and a family that is not bit-reproducible on identical input fails there.  The cases are
tests/hot_cases.py's tables with ordinary values (tests/slice_cases.py), each proven to run on its family (tests/family_runs.py), and the
five bf16 cases of tests/test_gpu_bf16.py for the properties that need no tolerance."""
import numpy as np
import pytest

import hot_cases as HC
import slice_cases as SC
from family_runs import run_layer_as, run_stack, switches  # noqa: F401  (switches is a fixture)
from hip_util import compare_all, compare_slices, run_literal
from test_gpu_bf16 import CASES as BF16_CASES
from test_gpu_bf16 import run_hip_dtype
from vmlmf_amd import _lib

pytestmark = pytest.mark.gpu
BF16 = [("bf16", tuple(c) + (HC.HOT,), {}) for c in BF16_CASES]
CASES = SC.LAYER_ROWS + BF16 + SC.STACK_ROWS
OUT, GRAD = ("y", "hT", "cT"), ("dx", "dh0", "dc0")


def is_stack(case):
    return isinstance(case[1][4], list)


def probe_rows(B):
    """Row 0, the last row, one row inside a 16-row tile and the first row of the second tile."""
    return sorted({0, B - 1} | ({5} if B > 5 else set()) | ({16} if B > 16 else set()))


def base_inputs(case):
    row = case[1]
    if is_stack(case):
        return SC.ordinary_stack_inputs(*row, "dense")
    if case[0] == "bf16":       # that file's own parameters (its ranks_of takes one u_rank)
        inp = SC.ordinary_inputs(row)
        return (HC.O.make_params(row[0], row[3], row[4], row[5], row[6][0], seed=row[4] + row[5]),) + inp[1:]
    return SC.ordinary_inputs(row)


def run(case, switches, P, inp, backward=True):
    """{form: result} of one run of the case on its family; a result's hT, cT, dh0, dc0 are lists over the layers for a stack."""
    family, row = case[0], case[1]
    if is_stack(case):
        v, B, T, I, Hs, rw, ru, tm, st = row
        x, h0, c0, dy, dhT, dcT = inp
        return {family: run_stack(v, P, x, h0, c0, *((dy, dhT, dcT) if backward else (None, None, None)), rw, ru, tm, family == "rbx")}
    if family == "bf16":
        v, B, T, I, H, rw, ru, tm = row[:8]
        assert _lib.query(_lib.make_desc(v, B, T, I, H, rw, ru, time_major=tm, dtype="bf16")).rows_per_wg == 16
        return {family: run_hip_dtype(v, P, *inp, tm, "bf16")}
    return run_layer_as(family, row, case[2], switches, P, inp, backward)


def _arrays(res, keys):
    for k in keys:
        v = res.get(k)
        if isinstance(v, list):
            for l, a in enumerate(v):
                yield f"{k}[{l}]", k, a
        elif v is not None:
            yield k, k, v


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cut(a, key, tm, rows=None, steps=None):
    """The rows and/or time steps of one result array: y and dx carry both axes, states and their gradients rows alone."""
    if key in ("y", "dx"):
        if rows is not None:
            a = np.take(a, rows, axis=1 if tm else 0)
        if steps is not None:
            a = a[steps] if tm else a[:, steps]
        return a
    assert steps is None
    return a if rows is None else a[rows]


def same_bits(base, other, keys, tm, what, rows=None, steps=None):
    problems = []
    for form, res in base.items():
        for name, key, a in _arrays(res, keys):
            b = dict((n, arr) for n, _, arr in _arrays(other[form], keys))[name]
            a, b = bits(cut(a, key, tm, rows, steps)), bits(cut(b, key, tm, rows, steps))
            if not np.array_equal(a, b):
                idx = tuple(int(i) for i in np.argwhere(a != b)[0])
                problems.append(f"{form}.{name}: {int((a != b).sum())} of {a.size} values changed bits, first at {idx} of the compared part")
    assert not problems, f"{what}:\n" + "\n".join(problems)


_BASE = {}


def base_run(case, switches):
    """The base input's result, run twice: a family whose two runs differ in the bits of an output or of dx, dh0, dc0 is not reproducible,
    and fails every test of its case.  (The parameter gradients are sums over rows and steps and are compared by tolerance, never on bits.)"""
    key = SC.case_id(case)
    if key not in _BASE:
        inp = base_inputs(case)
        first, second = run(case, switches, inp[0], inp[1:]), run(case, switches, inp[0], inp[1:])
        try:
            same_bits(first, second, OUT + GRAD, case[1][7], f"{key}: two runs on identical input differ - the family is not bit-reproducible")
            _BASE[key] = (inp, first, None)
        except AssertionError as e:
            _BASE[key] = (inp, first, str(e))
    inp, first, problem = _BASE[key]
    assert problem is None, problem
    return inp, first


def redraw(rng, a, where, scale=1.0):
    """a with the entries at the index `where` drawn anew (N(0, 1) x scale)."""
    b = a.copy()
    b[where] = (scale * rng.standard_normal(b[where].shape)).astype(np.float32)
    return b


def each(v, fn):
    return None if v is None else [fn(a) for a in v] if isinstance(v, list) else fn(v)


def case_rng(case, salt):
    row = case[1]
    return np.random.Generator(np.random.PCG64(HC.case_seed(row[0], row[1], row[2], row[3], row[4][-1] if is_stack(case) else row[4], row[5]) + salt))


@pytest.mark.parametrize("case", [c for c in CASES if len(probe_rows(c[1][1])) < c[1][1]], ids=SC.case_id)      # a row outside the probes
def test_rows_are_independent(case, switches):
    """Every row outside the probe set redrawn - x at three times the scale, new states, new upstream gradients: the probe rows of every
    output and of dx, dh0, dc0 keep their bits."""
    row, tm = case[1], case[1][7]
    B, R = row[1], probe_rows(row[1])
    (P, x, h0, c0, dy, dhT, dcT), base = base_run(case, switches)
    rng = case_rng(case, 1)
    others = np.setdiff1d(np.arange(B), R)
    seq = (slice(None), others) if tm else (others,)
    inp = (redraw(rng, x, seq, 3.0), each(h0, lambda a: redraw(rng, a, others, 0.5)), each(c0, lambda a: redraw(rng, a, others, 0.5)),
           redraw(rng, dy, seq), each(dhT, lambda a: redraw(rng, a, others)), each(dcT, lambda a: redraw(rng, a, others)))
    same_bits(base, run(case, switches, P, inp), OUT + GRAD, tm, f"{SC.case_id(case)}: rows {R} changed when the other rows were redrawn", rows=R)


SEQUENCES = [c for c in CASES if c[1][2] > 1]          # T = 1 has no earlier step


def _t0s(T):
    return sorted({T // 2, T - 1})


@pytest.mark.parametrize("case", SEQUENCES, ids=SC.case_id)
def test_time_is_causal_forward(case, switches):
    """x redrawn from step t0 on, in every row: y before t0 keeps its bits."""
    row, tm = case[1], case[1][7]
    T = row[2]
    (P, x, h0, c0, dy, dhT, dcT), base = base_run(case, switches)
    for t0 in _t0s(T):
        late = slice(t0, None) if tm else (slice(None), slice(t0, None))
        inp = (redraw(case_rng(case, 2 + t0), x, late), h0, c0, dy, dhT, dcT)
        got = run(case, switches, P, inp, backward=case[0] == "bf16")
        base_fwd = {form: base.get(form, base.get("with-dx")) for form in got}        # the headline layer's forms share one forward
        same_bits(base_fwd, got, ("y",), tm, f"{SC.case_id(case)}: y before step {t0} changed when x from step {t0} on was redrawn", steps=slice(0, t0))


@pytest.mark.parametrize("case", SEQUENCES, ids=SC.case_id)
def test_time_is_causal_backward(case, switches):
    """dy redrawn before step t0, the forward inputs untouched: dx from t0 on keeps its bits."""
    row, tm = case[1], case[1][7]
    T = row[2]
    (P, x, h0, c0, dy, dhT, dcT), base = base_run(case, switches)
    for t0 in _t0s(T):
        early = slice(0, t0) if tm else (slice(None), slice(0, t0))
        inp = (x, h0, c0, redraw(case_rng(case, 50 + t0), dy, early), dhT, dcT)
        same_bits(base, run(case, switches, P, inp), ("dx",), tm,
                  f"{SC.case_id(case)}: dx from step {t0} on changed when dy before step {t0} was redrawn", steps=slice(t0, None))


_REF_R = {}


def reference_on_probe_rows(case, P, x, h0, c0, dy, dhT, dcT, R):
    """The fp64 oracle's parameter gradients on the probe rows alone: a batch of len(R) rows."""
    key = SC.case_id(case)
    if key not in _REF_R:
        row, tm = case[1], case[1][7]

        def seq(a):
            return np.take(a, R, axis=1 if tm else 0)
        args = (seq(x), each(h0, lambda a: a[R]), each(c0, lambda a: a[R]), seq(dy), each(dhT, lambda a: a[R]), each(dcT, lambda a: a[R]))
        ref = HC.run_stack_literal(row[0], P, *args, tm) if is_stack(case) else run_literal(row[0], P, *args, time_major=tm)
        _REF_R[key] = {"G": ref["G"]}
    return _REF_R[key]


@pytest.mark.parametrize("case", [c for c in CASES if c[0] != "bf16"], ids=SC.case_id)
def test_rows_without_upstream_gradient_get_and_give_exactly_nothing(case, switches):
    """dy, dhT, dcT zero outside the probe rows: dx, dh0, dc0 are exactly zero there, and every parameter gradient is the fp64 oracle's on the
    probe rows alone, slice by slice - the other rows add nothing to a sum whose scale the full batch no longer sets."""
    row, tm = case[1], case[1][7]
    B, R = row[1], probe_rows(row[1])
    (P, x, h0, c0, dy, dhT, dcT), _ = base_run(case, switches)
    others = np.setdiff1d(np.arange(B), R)

    def zeroed(a, where):
        b = a.copy()
        b[where] = 0
        return b
    seq = (slice(None), others) if tm else (others,)
    inp = (x, h0, c0, zeroed(dy, seq), each(dhT, lambda a: zeroed(a, others)), each(dcT, lambda a: zeroed(a, others)))
    forms = run(case, switches, P, inp)
    ref = reference_on_probe_rows(case, P, *inp, R)
    problems = []
    for form, got in forms.items():
        for name, key, a in _arrays(got, GRAD):
            rest = cut(a, key, tm, rows=others)
            if np.any(rest != 0):
                problems.append(f"{form}.{name}: {int((rest != 0).sum())} non-zero values in rows without upstream gradient, max |.| {np.abs(rest).max():.3e}")
        try:
            H = row[4]
            if is_stack(case):
                HC.assert_shares({"G": got["G"]}, ref, f"{SC.case_id(case)}.{form}", may_lack=())
                report = compare_slices({"G": got["G"]}, ref, f"{SC.case_id(case)}.{form}", SC.layout(row[0], H, tm))
            else:
                report = compare_all({"G": got["G"]}, ref, f"{SC.case_id(case)}.{form}", slices=SC.layout(row[0], H, tm))
            print(f"\nzeros {case[0]}.{form}: worst slice {report['worst'][0]} {report['worst'][1]:.3f}")
        except AssertionError as e:
            problems.append(str(e))
    assert not problems, f"{SC.case_id(case)}:\n" + "\n".join(problems)
