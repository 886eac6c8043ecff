"""GPU: the step loops of the headline recurrences (rec_fwd_kernel with the x-projection wave, rec3_bwd_kernel) around everything their
unrolled form depends on - sequence lengths around the ring depth and the unroll period of eight and their remainders, one to three
compute waves with and without pad lanes, input widths, ranks 16 and 8, one and two groups (the rank-major partials choose their
columns by group), with and without initial states, gradients into the whole output and into the last step only, the riding workers
and the stand-alone weight gradients, the rec3 masks that reach the touched kernels, Net.loss with the classifier and the criterion
riding.  Every case runs at B <= 4 against the fp64 literal oracle with the comparisons of tests/test_gpu_slices.py (the whole-tensor
rules of tests/hip_util.py and every gradient slice by slice, docs/design/slice_tolerances.md).

Bit checks that need no second build: a sequence in one call against the same sequence in two calls with the state carried (the
step's arithmetic must not depend on where in the ring or in the unrolled period a step falls), and a repeated step."""
import numpy as np
import pytest
import torch

import hot_cases as HC
import slice_cases as SC
import vmlmf_oracle as O
from family_runs import SWITCH_DEFAULTS, family_of, kernel_counts, switches  # noqa: F401  (switches is a fixture)
from hip_util import ORDER, assert_grad, compare_all, compare_slices, run_hip, run_literal
from vmlmf_amd import _lib

pytestmark = pytest.mark.gpu
V1, V2, V6 = O.V1, O.V2, O.V6
LENGTHS = (1, 2, 5, 6, 7, 8, 9, 13, 16, 17)


def _row(T, H=180, I=9, r=16, st=True, v=V1, B=3, ru=None):
    return (v, B, T, I, H, r, ru or [r], False, st, HC.HOT)


# (row, pattern): every length at the headline shape, states and patterns alternating; the other widths, ranks and groups at a length
# below the period, one on it and one beyond it
CASES = [(_row(T, st=(i % 2 == 0)), ("dense", "last")[i % 2]) for i, T in enumerate(LENGTHS)] + \
        [(_row(T, st=(i % 2 == 1)), ("last", "dense")[i % 2]) for i, T in enumerate((7, 8, 17))] + \
        [(_row(T, H=H, B=2 + (H % 3)), p) for H in (60, 100, 130, 192) for T, p in ((5, "dense"), (9, "last"), (17, "dense"))] + \
        [(_row(T, I=I, st=False), p) for I in (2, 16) for T, p in ((9, "dense"), (16, "last"))] + \
        [(_row(T, H=H, r=8, B=4), p) for H in (100, 180) for T, p in ((6, "last"), (17, "dense"))] + \
        [(_row(T, H=H, I=10, r=8, v=v, ru=[16, 8]), p) for v, H in ((V2, 100), (V2, 136), (V6, 136)) for T, p in ((9, "dense"), (17, "last"))]

# The riding workers take a launch only from four chunks of 64 (time step, row) pairs on: at B = 4 from T = 64.  Lengths on the period,
# one and seven beyond it; the launch counts prove that the workers rode.
RIDING = [(_row(T, st=(i % 2 == 0), B=4), ("dense", "last")[i % 2]) for i, T in enumerate((64, 65, 71, 72))]

# form -> (switches held, need_dx)
FORMS = {
    "with-dx": ({}, True),
    "riding": ({"inrow": 0, "wride": 1}, False),
    "stand-alone": ({"inrow": 0, "wride": 0}, False),
    "rec3=0": ({"rec3": 0}, True),
    "rec3=7": ({"rec3": 7}, True),
}
_REF = {}


def case_id(c):
    return HC.row_id(c[0]) + "-" + c[1] if isinstance(c, tuple) and isinstance(c[0], tuple) else str(c)


def reference(row, pattern):
    key = (HC.row_id(row), pattern)
    if key not in _REF:
        inp = SC.ordinary_inputs(row, pattern)
        _REF[key] = (inp, run_literal(row[0], *inp, time_major=row[7]))
    return _REF[key]


@pytest.mark.parametrize("case", CASES + RIDING, ids=case_id)
def test_step_loops_against_the_oracle(case, switches):
    row, pattern = case
    rides = case in RIDING
    inp, ref = reference(row, pattern)
    assert family_of(row)[0] == "valu", "not a layer of the persistent VALU kernels"
    problems = []
    for form, (held, need_dx) in FORMS.items():
        for key, value in held.items():
            switches(key, value)
        got, counts = kernel_counts(lambda: run_hip(row[0], inp[0], *inp[1:], time_major=row[7], need_dx=need_dx))
        for key in held:
            switches(key, SWITCH_DEFAULTS[key])
        assert counts["rec_fwd_kernel"] == 1 and counts["rec_bwd_kernel"] == 1, (form, counts)
        if rides and form == "riding":          # (family_runs.headline_forms)
            assert _lib.tune_get("wride") == 1 and counts["wgrad_mfma_kernel"] == 0 and counts["finish2_kernel"] == 1, (form, counts)
        if rides and form == "stand-alone":
            assert counts["wgrad_mfma_kernel"] == 1 and counts["finish2_kernel"] == 0, (form, counts)
        try:
            report = compare_all(got, ref, f"{case_id(case)}.{form}", slices=SC.layout(row[0], row[4], row[7]))
            assert report["skipped"] == 0, f"{form}: {report['skipped']} slices below 2^-100"
        except AssertionError as e:
            problems.append(str(e))
    assert not problems, "\n".join(problems)


# ---- Net.loss: the classifier and the criterion riding on the forward launch, the gradients finished behind the backward ------------------
def _net(T, H, seed):
    from vmlmf_amd import MyLSTM, MyVMLMFCell, Net
    torch.manual_seed(seed)
    net = Net(9, layer_sizes=[H], w_rank=16, u_rank=[16], model=MyLSTM, cell=MyVMLMFCell).to("cuda")
    x, tgt = O.synthetic_batch(4, T, 9, seed=seed + 17)
    return net, torch.tensor(x, device="cuda"), torch.tensor(tgt, device="cuda")


def _net_reference(net, x, tgt):
    f64 = torch.float64
    cell = net.rnn.rnncells[0]
    Pt = {k: getattr(cell, k).detach().cpu().to(f64).requires_grad_(True) for k in ORDER[V1]}
    W = net.lin.weight.detach().cpu().to(f64).requires_grad_(True)
    b = net.lin.bias.detach().cpu().to(f64).requires_grad_(True)
    loss, _ = O.literal_train_step_har(Pt, W, b, x.cpu().to(f64), tgt.cpu())
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in Pt.items()}, W.grad.numpy(), b.grad.numpy()


def _grads(net):
    return {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}


def _same_bytes(a, b, what):
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{what}: {k} differs"


@pytest.mark.parametrize("T,H,wride", [(5, 180, 1), (8, 180, 0), (17, 180, 1), (9, 130, 1), (16, 192, 0), (71, 180, 1)])
def test_net_loss_two_steps_and_a_second_backward(T, H, wride, switches):
    switches("wride", wride)
    net, x, tgt = _net(T, H, seed=100 * T + H)
    ref_loss, ref_G, ref_W, ref_b = _net_reference(net, x, tgt)
    cell = net.rnn.rnncells[0]
    steps = []
    for _ in range(2):                       # two steps in a row over the same buffers: rings and progress words start over
        net.zero_grad()
        loss = net.loss(x, tgt)
        loss.backward(retain_graph=True)
        first = _grads(net)
        assert abs(loss.item() - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (loss.item(), ref_loss)
        tag = f"net.loss T={T} H={H} wride={wride}"
        got = {"G": {k: getattr(cell, k).grad.cpu().numpy() for k in ORDER[V1]}}
        for k in ORDER[V1]:
            assert_grad(got["G"][k], ref_G[k], f"{tag}.{k}")
        report = compare_slices(got, {"G": ref_G}, tag, SC.layout(V1, H, False))
        assert report["skipped"] == 0, report
        assert_grad(net.lin.weight.grad.cpu().numpy(), ref_W, tag + ".lin.weight")
        assert_grad(net.lin.bias.grad.cpu().numpy(), ref_b, tag + ".lin.bias")
        net.zero_grad()
        loss.backward()                      # the same graph once more: the tape is read again, the progress words start at zero
        _same_bytes(first, _grads(net), tag + ", second backward")
        steps.append((loss.detach().clone(), first))
    assert torch.equal(steps[0][0].view(torch.int32), steps[1][0].view(torch.int32)), "the repeated step's loss differs"
    _same_bytes(steps[0][1], steps[1][1], "the repeated step")


# ---- bits: one call over T = 17 against 8 + 9 steps with the state carried ----------------------------------------------------------------
def _bits_equal(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    n = int((a.view(np.uint32) != b.view(np.uint32)).sum())
    assert n == 0, f"{what}: {n} of {a.size} values differ in their bits (max abs diff {np.abs(a - b).max():.3g})"


@pytest.mark.parametrize("H,I,form,T,cut,B", [(180, 9, "riding", 17, 8, 3), (180, 9, "with-dx", 17, 8, 3), (130, 9, "stand-alone", 17, 8, 3),
                                               (100, 9, "with-dx", 17, 8, 3), (180, 1, "with-dx", 17, 8, 3), (180, 9, "riding", 129, 64, 4)])
def test_one_call_equals_two_calls_with_the_state_carried(H, I, form, T, cut, B, switches):
    """y, hT, cT of 17 steps in one call are, byte for byte, those of 8 steps and then 9 with (h, c) carried; dh0 and dc0 of the backward
    are those of the backward over the last 9 steps handed to the backward over the first 8 as dhT, dcT.  (The kernels before the step
    loops were unrolled satisfy this too: a step's arithmetic depends on neither its ring slot nor its index.)  Once more at 129 = 64 + 65
    steps of four rows, where every call is long enough for the riding workers, and at I = 1 - an input width the literal oracle cannot
    run (its x.squeeze() drops the axis), so that the oracle cases above start at I = 2.  Run twice: a repeated call gives identical
    bytes."""
    held, need_dx = FORMS[form]
    for key, value in held.items():
        switches(key, value)
    row = _row(T, H=H, I=I, st=True, B=B)
    P, x, h0, c0, dy, dhT, dcT = SC.ordinary_inputs(row, "dense")
    whole = run_hip(V1, P, x, h0, c0, dy, dhT, dcT, need_dx=need_dx)
    again = run_hip(V1, P, x, h0, c0, dy, dhT, dcT, need_dx=need_dx)
    for k in ("y", "hT", "cT", "dh0", "dc0"):
        _bits_equal(whole[k], again[k], f"repeated call, {k}")
    for k in whole["G"]:
        _bits_equal(whole["G"][k], again["G"][k], f"repeated call, G.{k}")
    head = run_hip(V1, P, x[:, :cut], h0, c0, need_dx=need_dx)
    tail, counts = kernel_counts(lambda: run_hip(V1, P, x[:, cut:], head["hT"], head["cT"], dy[:, cut:], dhT, dcT, need_dx=need_dx))
    if T > 100:
        assert counts["wgrad_mfma_kernel"] == 0 and counts["finish2_kernel"] == 1, ("the workers did not ride", counts)
    _bits_equal(np.concatenate([head["y"], tail["y"]], axis=1), whole["y"], "y")
    _bits_equal(tail["hT"], whole["hT"], "hT")
    _bits_equal(tail["cT"], whole["cT"], "cT")
    first = run_hip(V1, P, x[:, :cut], h0, c0, dy[:, :cut], tail["dh0"], tail["dc0"], need_dx=need_dx)
    _bits_equal(first["dh0"], whole["dh0"], "dh0")
    _bits_equal(first["dc0"], whole["dc0"], "dc0")
