"""GPU: the gradients of every recurrent kernel family slice by slice (tests/hip_util.py::assert_grad_slices at GREL = 1e-4 of each
slice's own maximum, no absolute floor; docs/design/slice_tolerances.md) under the two upstream-gradient patterns the whole-tensor rule is
blind to: the last state alone (dx decays by orders of magnitude towards t = 0) and rows of loss weights from 1 down to 1e-6.  The cases are
tests/slice_cases.py's: hot_cases' tables with ordinary values, each proven to run on its family (tests/family_runs.py); that plain fp32 can
be held to them is tests/test_slice_compare_cpu.py's part.  Against the fp64 literal oracle."""
import pytest

import hot_cases as HC
import slice_cases as SC
from family_runs import run_layer_as, run_stack, switches  # noqa: F401  (switches is a fixture)
from hip_util import compare_all, compare_slices

pytestmark = pytest.mark.gpu
WORST = {}


def note(family, report, tag):
    name, share = report["worst"]
    if share >= WORST.get(family, ("", -1.0))[1]:
        WORST[family] = (f"{tag}: {name}", share)
    print(f"\nslices {family}: this case {name} {share:.3f}; worst so far {WORST[family][0]} {WORST[family][1]:.3f}")


@pytest.mark.parametrize("case,pattern", SC.GPU_LAYER_CASES, ids=SC.case_id)
def test_layer_gradients_by_slice(case, pattern, switches):
    family, row, held = case
    inp, ref = SC.layer_case(row, pattern)
    forms = run_layer_as(family, row, held, switches, inp[0], inp[1:])
    problems = []
    for form, got in forms.items():
        try:
            report = compare_all(got, ref, f"{SC.case_id((case, pattern))}.{form}", slices=SC.layout(row[0], row[4], row[7]))
            assert report["skipped"] == 0, f"{form}: {report['skipped']} slices below 2^-100"
            note(family if form == family else f"{family}.{form}", report, SC.case_id((case, pattern)))
        except AssertionError as e:
            problems.append(str(e))
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("case,pattern", SC.GPU_STACK_CASES, ids=SC.case_id)
def test_stack_gradients_by_slice(case, pattern):
    family, row = case
    v, B, T, I, Hs, rw, ru, tm, st = row
    inp, ref = SC.stack_case(row, pattern)
    got = run_stack(v, *inp, rw, ru, tm, family == "rbx")
    HC.assert_shares(got, ref, SC.case_id((case, pattern)), may_lack=())          # the whole-tensor rules, as the other stack tests apply them
    report = compare_slices(got, ref, SC.case_id((case, pattern)), SC.layout(v, Hs, tm))
    assert report["skipped"] == 0, report
    note(family, report, SC.case_id((case, pattern)))
