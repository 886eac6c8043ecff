"""GPU: AR / TAR - vmlmf_actreg_forward / _backward through functional.activation_regularizer, Model.loss's ar / tar and a captured
training step - against the fp64 oracle of actreg_cases.py within the counted rounding bounds, against the stock formulation on the
same factors, and on bits: the dropped copy is dropout()'s, runs repeat, rows and distant time steps do not see each other."""
import ctypes

import numpy as np
import pytest
import torch

import actreg_cases as C
from hip_util import assert_grad
import vmlmf_amd
from vmlmf_amd import Model, _lib, optim, unit_gradient
from vmlmf_amd import functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 0x5EED5EED1234
WEIGHTS = ((2.0, 1.0, None), (0.0, 1.0, 0.75), (2.0, 0.0, None))      # (ar, tar, upstream gradient of the penalty; None: the unit one)


def snapshot(offset=7):
    return torch.tensor([SEED, offset], dtype=torch.int64, device=DEV)


def on_device(a, dtype=None):
    return None if a is None else torch.as_tensor(a, dtype=dtype).to(DEV)


def run(raw, g, ar, tar, p=0.0, snap=None, site=2, lengths=None, desc=None, s=None):
    """One forward and backward of the fused pair: (yd, [penalty, ar_part, tar_part], d raw, x) - device tensors but the stats."""
    x = on_device(raw).requires_grad_(True)
    yd, penalty, parts = vmlmf_amd.activation_regularizer(x, ar=ar, tar=tar, p=p, snap=snap, site=site, lengths=lengths, layer_desc=desc)
    up = unit_gradient(x.device) if s is None else torch.tensor(s, device=DEV)
    (grad,) = torch.autograd.grad([yd, penalty], x, [on_device(g), up])
    return yd.detach(), torch.stack([penalty.detach(), *parts]).cpu().numpy(), grad, x


def stock64(raw, g, f, ar, tar, lengths, s):
    """activation_regularizer_stock in fp64 on the device, on the same factors: ([penalty, ar_part, tar_part], d raw)."""
    x = on_device(raw, torch.float64).requires_grad_(True)
    yd, penalty, parts = F.activation_regularizer_stock(x, ar=ar, tar=tar, factors=None if f is None else f.double(), lengths=lengths)
    outs, ups = [yd], [on_device(g, torch.float64)]
    if penalty.requires_grad:       # (a penalty without a term - T == 1 under tar alone - is a constant)
        outs, ups = outs + [penalty], ups + [torch.tensor(1.0 if s is None else float(np.float32(s)), dtype=torch.float64, device=DEV)]
    (grad,) = torch.autograd.grad(outs, x, ups)
    return np.array([float(penalty.detach()), float(parts[0]), float(parts[1])]), grad.cpu().numpy()


@pytest.mark.parametrize("masked", [False, True], ids=["all", "lengths"])
@pytest.mark.parametrize("p", [0.0, 0.5], ids=["p0", "p0.5"])
@pytest.mark.parametrize("shape", C.SHAPES, ids=C.IDS)
def test_the_pair_against_the_oracle_and_the_stock_formulation(shape, p, masked):
    T, B, H = shape
    i = C.SHAPES.index(shape)
    raw, g = C.draw(T, B, H, 10 * i + int(2 * p) + (5 if masked else 0), amp=1.0 if i % 3 else 30.0)
    lengths = C.lengths_for(T, B, 50 + i) if masked else None
    n = on_device(lengths) if i % 2 else (None if lengths is None else torch.as_tensor(lengths, dtype=torch.int32))   # device int64 / CPU int32
    snap = snapshot() if p > 0 else None
    f = F.dropout_factors(T * B, H, p, snap, 2).view(T, B, H) if p > 0 else None
    fn = None if f is None else f.cpu().numpy()
    for ar, tar, s in WEIGHTS:
        what = f"{shape} p {p} masked {masked} ar {ar} tar {tar} s {s}"
        yd, stats, grad, x = run(raw, g, ar, tar, p, snap, 2, n, s=s)
        if p > 0:       # the dropped copy has dropout()'s bits - at every position, masked ones included
            assert torch.equal(yd.view(torch.int32), F.dropout(x.detach(), p, snap, 2).view(torch.int32)), what
        else:           # nothing was written: it IS raw
            assert yd.data_ptr() == x.data_ptr(), what
        want = C.oracle(raw, fn, lengths, ar, tar, g, s=1.0 if s is None else float(np.float32(s)))
        C.check_stats(stats, want, T, B, H, ar, tar, what)
        C.check_draw(grad.cpu().numpy(), want, what)
        # the second opinion: the stock formulation in fp64 on the same factors
        sstats, sgrad = stock64(raw, g, f, ar, tar, n, s)
        assert np.all(np.abs(stats.astype(np.float64) - sstats) <= C.penalty_bound(T, B, H) * np.abs(sstats) + C.F32_TINY), (what, stats, sstats)
        err = np.abs(grad.cpu().numpy().astype(np.float64) - sgrad)
        assert np.all(err <= C.gamma(C.ROUNDINGS_DRAW) * want["magnitude"] + C.F32_TINY), (what, err.max())
        # masked positions get exactly f g
        m, _ = C.masks(T, B, lengths)
        fg = on_device(g) if f is None else F.dropout(on_device(g), p, snap, 2)
        assert torch.equal(grad[on_device(~m)], fg[on_device(~m)]), what


def test_with_a_layer_descriptor_the_factors_are_the_layers():
    """A group layer at the PTB size applies its dropout inside its launches, with its thread slots as the generator's columns."""
    T, B, H = 3, 2, 650
    desc = _lib.make_desc(_lib.V4_LM_GROUP, B, T, H, H, 32, [32, 32], g=2, time_major=True, training=True)
    assert _lib.lib().vmlmf_dropout_fused(ctypes.byref(desc)) == 1
    raw, g = C.draw(T, B, H, 21)
    snap = snapshot(3)
    f = F.dropout_factors(T * B, H, 0.5, snap, 2, layer_desc=desc).view(T, B, H)
    assert not torch.equal(f, F.dropout_factors(T * B, H, 0.5, snap, 2).view(T, B, H))
    lengths = np.array([3, 2])
    yd, stats, grad, x = run(raw, g, 2.0, 1.0, 0.5, snap, 2, on_device(lengths), desc=desc)
    assert torch.equal(yd.view(torch.int32), (x.detach() * f).view(torch.int32))
    want = C.oracle(raw, f.cpu().numpy(), lengths, 2.0, 1.0, g)
    C.check_stats(stats, want, T, B, H, 2.0, 1.0, "group layer")
    C.check_draw(grad.cpu().numpy(), want, "group layer")


def test_two_runs_give_the_same_bits_and_leave_the_ticket_zero():
    for (T, B, H) in ((9, 40, 28), (3, 2, 650), (70, 1, 8)):
        raw, g = C.draw(T, B, H, 31)
        n = on_device(C.lengths_for(T, B, 8))
        a = run(raw, g, 2.0, 1.0, 0.5, snapshot(), 2, n, s=0.75)
        b = run(raw, g, 2.0, 1.0, 0.5, snapshot(), 2, n, s=0.75)
        assert torch.equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and torch.equal(a[2], b[2])
    torch.cuda.synchronize()
    tickets = [t for k, t in F._TICKET.items() if k[0] == "actreg"]
    assert tickets and all(int((t[0] if isinstance(t, list) else t).abs().sum()) == 0 for t in tickets)


def test_rows_and_distant_steps_do_not_see_each_other():
    T, B, H = 20, 5, 12
    raw, g = C.draw(T, B, H, 41)
    n = on_device(np.array([20, 20, 7, 20, 20]))
    base = run(raw, g, 2.0, 1.0, 0.5, snapshot(), 2, n)[2]
    # another row's activations and gradient change: the counts stay, so every other row keeps its bits
    other, og = raw.copy(), g.copy()
    other[:, 1] *= 3.0
    og[:, 1] += 1.0
    got = run(other, og, 2.0, 1.0, 0.5, snapshot(), 2, n)[2]
    keep = [0, 2, 3, 4]
    assert torch.equal(got[:, keep], base[:, keep]) and not torch.equal(got[:, 1], base[:, 1])
    # d raw[t] depends on raw[t - 1 .. t + 1] only: steps 8 (the first of a block of four) and 15 (the last of one) change
    for t0 in (8, 15):
        moved = raw.copy()
        moved[t0] += 0.5
        got = run(moved, g, 0.0, 1.0, 0.5, snapshot(), 2, n)[2]         # (tar alone: with ar the sums would not move either - the
        ref = run(raw, g, 0.0, 1.0, 0.5, snapshot(), 2, n)[2]           #  gradient has no term in them)
        far = [t for t in range(T) if abs(t - t0) > 1]
        assert torch.equal(got[far], ref[far]) and not torch.equal(got[t0 - 1:t0 + 2], ref[t0 - 1:t0 + 2])


def test_a_row_constant_in_time_has_a_tar_gradient_of_exactly_zero():
    T, B, H = 19, 3, 6
    raw, _ = C.draw(T, B, H, 51)
    raw[:, 1] = raw[0, 1]
    for p in (0.0, 0.5):
        grad = run(raw, np.zeros_like(raw), 0.0, 1.0, p, snapshot() if p else None, 2, None)[2]
        assert int(grad[:, 1].abs().view(torch.int32).sum()) == 0 and float(grad[:, 0].abs().max()) > 0
    stats = run(raw[:, 1:2], np.zeros_like(raw[:, 1:2]), 0.0, 1.0)[1]
    assert stats[0] == 0.0 and stats[2] == 0.0
    # T == 1 and lengths that leave no pair: TAR is 0, not NaN
    assert np.array_equal(run(raw[:1], raw[:1], 0.0, 1.0)[1], np.zeros(3, np.float32))
    assert np.array_equal(run(raw, raw, 0.0, 1.0, lengths=on_device(np.array([1, 0, 1])))[1], np.zeros(3, np.float32))


# ---- through Model ----------------------------------------------------------------------------------------------------------------
def lm(H, B, T, layers=2):
    torch.manual_seed(5)
    V = 120
    m = Model(V, H, layers, 0.5, 0.08, w_rank=8 if H < 100 else 32, u_ranks=[8 if H < 100 else 32], lstm_type="vmlmf").to(DEV).train()
    r = np.random.Generator(np.random.PCG64(4))
    tok = torch.tensor(r.integers(0, V, size=(T, B)), device=DEV)
    tgt = torch.tensor(r.integers(0, V, size=(T, B)), device=DEV)
    return m, tok, tgt


@pytest.mark.parametrize("H,B,T,fused", [(32, 6, 5, 0), (650, 20, 4, 1)], ids=["top_dropout_apart", "top_dropout_in_launch"])
def test_model_loss_keeps_the_plain_calls_bits_and_matches_the_stock_formulation(H, B, T, fused):
    m, tok, tgt = lm(H, B, T)
    rnn = m.rnns[-1]
    desc = _lib.make_desc(rnn.variant, B, T, H, H, rnn.w_rank, [rnn.u_ranks], g=1, time_major=True, training=True)
    assert _lib.lib().vmlmf_dropout_fused(ctypes.byref(desc)) == fused
    lengths = torch.tensor([T] * (B - 2) + [1, T + 3], device=DEV)
    for kw in (dict(), dict(lengths=lengths, label_smoothing=0.1)):
        m.dropout_state(seed=SEED)
        plain, st0 = m.loss(tok, tgt, m.state_init(B), return_parts=True, **kw)
        m.dropout_state(seed=SEED)
        out, st1 = m.loss(tok, tgt, m.state_init(B), ar=2.0, tar=1.0, return_parts=True, **kw)
        assert len(plain) == 5 and len(out) == 7
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(plain[1:], out[1:5]))      # nll and the other head parts
        assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(st0, st1))
        assert float(out[5]) > 0 and float(out[6]) > 0 and not out[5].requires_grad
        assert float(out[0].detach()) == pytest.approx(float(plain[0].detach()) + 2.0 * float(out[5]) + float(out[6]), rel=1e-6)
        # parameter gradients: the same step with the regulariser in stock ops on the same factors
        m.zero_grad()
        out[0].backward(unit_gradient(out[0].device))
        got = {k: v.grad.clone() for k, v in m.named_parameters()}
        m.zero_grad()
        m.dropout_state(seed=SEED)
        raw, _, (p, snap, site, layer_desc) = m._features(tok, m.state_init(B), raw_top=True)
        assert (layer_desc is not None) == bool(fused)
        f = F.dropout_factors(T * B, H, p, snap, site, layer_desc=layer_desc).view(T, B, H)
        yd, penalty, parts = F.activation_regularizer_stock(raw, ar=2.0, tar=1.0, factors=f, lengths=kw.get("lengths"), batch_scale=B)
        ref = F.lm_head_objective_loss(yd, m.fc.w, m.fc.b, tgt, **kw) + penalty
        ref.backward(unit_gradient(ref.device))
        assert float(out[0].detach()) == pytest.approx(float(ref.detach()), rel=1e-5)
        assert float(out[5]) == pytest.approx(float(parts[0]), rel=1e-5) and float(out[6]) == pytest.approx(float(parts[1]), rel=1e-5)
        for k, v in m.named_parameters():
            assert_grad(got[k].cpu().numpy(), v.grad.cpu().numpy(), k)
    # without parts and with everything else off the head is lm_head_loss, and the values are the same
    m.dropout_state(seed=SEED)
    loss, _ = m.loss(tok, tgt, m.state_init(B), ar=2.0, tar=1.0)
    m.dropout_state(seed=SEED)
    parts, _ = m.loss(tok, tgt, m.state_init(B), ar=2.0, tar=1.0, return_parts=True)
    assert float(loss.detach()) == pytest.approx(float(parts[0].detach()), rel=1e-5)
    # eval mode: no dropout anywhere, AR on the raw output
    m.eval()
    with torch.no_grad():
        h, _ = m.features(tok, m.state_init(B))
        out, _ = m.loss(tok, tgt, m.state_init(B), ar=2.0, tar=1.0, return_parts=True)
    want = C.oracle(h.cpu().numpy(), None, None, 2.0, 1.0)
    C.check_stats(torch.stack([2.0 * out[5] + out[6], out[5], out[6]]).cpu().numpy(), dict(want, penalty=2.0 * want["parts"][0] + want["parts"][1]),
                  T, B, H, 2.0, 1.0, "eval")


def test_a_captured_step_draws_fresh_masks_and_has_the_eager_calls_values():
    B, T = 6, 5
    m, tok, tgt = lm(32, B, T)
    state = m.dropout_state(seed=SEED)
    seen = {}

    class Feed(torch.nn.Module):          # GraphedTrainStep calls criterion(model(x), target): the LM's loss needs both
        def __init__(self, net):
            super().__init__()
            self.net = net

        def forward(self, x):
            return x

    def criterion(x, t):
        out, _ = m.loss(x, t, m.state_init(B), ar=2.0, tar=1.0, return_parts=True)
        seen["out"] = out
        return out[0]
    step = vmlmf_amd.GraphedTrainStep(Feed(m), criterion, optim.Adam(m.parameters(), lr=0.0), tok, tgt, warmup=1)    # lr 0: only the masks move
    captured = seen["out"]
    replays = []
    for _ in range(2):
        before = state.clone()
        step(tok, tgt)
        torch.cuda.synchronize()
        assert state.tolist() == [SEED, int(before[1]) + 1]
        values = [v.clone() for v in captured]
        state.copy_(before)                                        # the eager call from the same state
        eager, _ = m.loss(tok, tgt, m.state_init(B), ar=2.0, tar=1.0, return_parts=True)
        assert torch.equal(values[5].view(torch.int32), eager[5].view(torch.int32)) and torch.equal(values[6].view(torch.int32), eager[6].view(torch.int32))
        assert torch.equal(values[1].view(torch.int32), eager[1].view(torch.int32)) and torch.equal(values[0].view(torch.int32), eager[0].view(torch.int32))
        replays.append(values)
    assert not torch.equal(replays[0][5], replays[1][5]) and not torch.equal(replays[0][6], replays[1][6]) and not torch.equal(replays[0][1], replays[1][1])
