"""AR / TAR of Model.loss without a GPU: the fp64 oracle of actreg_cases.py against the literal AWD-LSTM expression; a float32
restatement of both kernels in their operation order stays inside the counted bounds, known-wrong rules break them; Model.loss and
activation_regularizer on CPU tensors (the stock-op path) against the oracle, values and gradients; the parts; the refusals, from
Python and from the C entry points; ar = tar = 0 never enters the new code."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import actreg_cases as C
import vmlmf_amd
import vmlmf_oracle as O
from vmlmf_amd import Model, _lib
from vmlmf_amd import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED5EED1234
# the stock formulation under autograd takes another order than the kernels: per term of d raw at most 3 roundings in the coefficient
# (weight, scale, count), 1 in yd or the difference, 2 in the square's backward (grad * d twice, added), 1 in the factor and up to 3
# additions where autograd accumulates the terms = 10; its sums are torch's, at worst one addition per element
STOCK_DRAW = 10


def factors(T, B, H, p, site=2, offset=7):
    return None if p == 0 else O.dropout_factors(SEED, offset, site, T * B, H, p).reshape(T, B, H)


def cases():
    for i, (T, B, H) in enumerate(C.SHAPES):
        for p in (0.0, 0.5):
            for masked in (False, True):
                yield T, B, H, p, (C.lengths_for(T, B, 50 + i) if masked else None), 10 * i + int(2 * p) + (5 if masked else 0)


def test_the_oracle_is_the_awd_lstm_expression_on_unmasked_cases():
    for i, (T, B, H) in enumerate(C.SHAPES):
        if T * B * H > 20000:
            continue
        for p in (0.0, 0.5):
            raw, g = C.draw(T, B, H, 100 + i)
            f = factors(T, B, H, p)
            f = np.ones_like(raw) if f is None else f
            want = C.oracle(raw, f, None, 2.0, 1.0, g)
            a, b, grad = C.awd_lstm(raw, f, 2.0, 1.0, g)
            assert want["parts"][0] == pytest.approx(a, rel=1e-12)
            assert want["parts"][1] == pytest.approx(b, rel=1e-12, abs=0.0) and (T > 1 or want["parts"][1] == 0.0)
            assert np.allclose(want["draw"], grad, rtol=1e-11, atol=1e-14)
    # T == 1: torch's mean over no element is NaN, the contract says 0
    raw, _ = C.draw(1, 2, 8, 1)
    assert np.isnan(float((torch.tensor(raw)[1:] - torch.tensor(raw)[:-1]).pow(2).mean()))
    assert C.oracle(raw, None, None, 2.0, 1.0)["parts"][1] == 0.0 and C.oracle(raw, None, [1, 0], 0.0, 1.0)["penalty"] == 0.0


def test_the_oracle_masks_positions_and_pairs_by_the_lengths():
    T, B, H = 5, 4, 3
    raw, g = C.draw(T, B, H, 3)
    want = C.oracle(raw, None, [0, 1, 5, 8], 2.0, 1.0, g)
    assert want["n_ar"] == H * (0 + 1 + 5 + 5) and want["n_tar"] == H * (0 + 0 + 4 + 4)
    assert np.array_equal(want["draw"][:, 0], g[:, 0].astype(np.float64))            # a row of length 0: g alone
    assert np.array_equal(want["draw"][1:, 1], g[1:, 1].astype(np.float64))           # length 1: position 0 has AR, no pair
    assert not np.array_equal(want["draw"][0, 1], g[0, 1].astype(np.float64))
    ar_only = C.oracle(raw, None, [0, 1, 5, 8], 2.0, 0.0, g)
    assert np.allclose(want["draw"][0, 1], ar_only["draw"][0, 1], rtol=0, atol=0)


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.IDS)
def test_a_float32_emulation_of_the_kernels_order_stays_inside_the_bounds(shape):
    T, B, H = shape
    for (t, b, h, p, lengths, seed) in cases():
        if (t, b, h) != shape:
            continue
        raw, g = C.draw(T, B, H, seed, amp=1.0 if seed % 3 else 30.0)
        f = factors(T, B, H, p)
        for ar, tar, s in ((2.0, 1.0, None), (0.0, 1.0, 0.75), (2.0, 0.0, None)):
            what = f"{shape} p {p} masked {lengths is not None} ar {ar} tar {tar} s {s}"
            yd, stats = C.emulate_forward(raw, f, lengths, ar, tar)
            want = C.oracle(raw, f, lengths, ar, tar, g, s=1.0 if s is None else float(np.float32(s)))
            assert C.same_bits(yd, want["yd"].astype(np.float32)), what
            C.check_stats(stats, want, T, B, H, ar, tar, what)
            assert stats[5] == np.float32(want["n_ar"]) and stats[6] == np.float32(want["n_tar"])
            got = C.emulate_backward(raw, f, lengths, ar, tar, g, stats, s)
            C.check_draw(got, want, what)
            m, _ = C.masks(T, B, lengths)                       # masked positions: exactly f g
            fg = g if f is None else (f * g).astype(np.float32)
            assert np.array_equal(got[~m], fg[~m]), what


def test_known_wrong_rules_break_the_bounds():
    for (T, B, H), lengths in (((5, 3, 6), None), ((7, 4, 256), None), ((9, 3, 5), [9, 4, 12])):
        raw, g = C.draw(T, B, H, 77)
        f = factors(T, B, H, 0.5)
        want = C.oracle(raw, f, lengths, 2.0, 1.0, g)
        # dividing TAR by T steps instead of T - 1: the part and every TAR gradient
        wrong = C.oracle(raw, f, lengths, 2.0, 1.0, g, variant="tar_over_T")
        assert abs(wrong["parts"][1] - want["parts"][1]) > C.part_bound(T, B, H) * want["parts"][1]
        with pytest.raises(AssertionError):
            C.check_stats(np.array([wrong["penalty"], *wrong["parts"]]), want, T, B, H, 2.0, 1.0, "tar_over_T")
        assert C.draw_excess(wrong["draw"], want) > 1.0
        # a boundary of the TAR gradient dropped
        for variant, t in (("no_first", 0), ("no_last", T - 1)):
            wrong = C.oracle(raw, f, lengths, 2.0, 1.0, g, variant=variant)
            assert C.draw_excess(wrong["draw"], want) > 1.0, variant
            with pytest.raises(AssertionError):
                C.check_draw(wrong["draw"], want, variant)
            rest = np.ones(T, bool)
            rest[t] = False
            assert np.array_equal(wrong["draw"][rest], want["draw"][rest])           # ... and nothing else
        # AR on raw instead of the dropped copy
        wrong = C.oracle(raw, f, lengths, 2.0, 1.0, g, variant="ar_on_raw")
        assert abs(wrong["parts"][0] - want["parts"][0]) > C.part_bound(T, B, H) * want["parts"][0]
        assert C.draw_excess(wrong["draw"], want) > 1.0
    # the bounds themselves: a handful of units in the last place, growing with the reduction
    assert C.chain(1, 2, 8) == 16 + 9 + 1 + 9 and C.chain(70, 256, 650) == 16 + 9 + 12 + 9
    assert C.workgroups(35, 32, 650) == (21, 9) and C.workgroups(9, 40, 28) == (2, 3)
    assert 5e-7 < C.gamma(C.ROUNDINGS_DRAW) < 6e-7 and C.penalty_bound(70, 256, 650) < 4e-6


# ---- activation_regularizer and Model.loss on CPU tensors --------------------------------------------------------------------------
def stock_bounds(n):
    return C.gamma(C.ROUNDINGS_TERM + n + 3), C.gamma(C.ROUNDINGS_TERM + n + 5)


@pytest.mark.parametrize("shape", [(1, 2, 8), (5, 3, 6), (7, 4, 32)], ids=["1x2x8", "5x3x6", "7x4x32"])
def test_the_cpu_path_against_the_oracle_values_and_gradients(shape):
    T, B, H = shape
    for masked in (False, True):
        for p in (0.0, 0.5):
            raw, g = C.draw(T, B, H, 9 + T)
            lengths = C.lengths_for(T, B, 4) if masked else None
            x = torch.tensor(raw, requires_grad=True)
            torch.manual_seed(11)
            yd, penalty, (ar_part, tar_part) = vmlmf_amd.activation_regularizer(x, ar=2.0, tar=1.0, p=p,
                                                                                lengths=None if lengths is None else torch.tensor(lengths))
            torch.manual_seed(11)
            f = torch.nn.functional.dropout(torch.ones(T, B, H), p, True).numpy() if p > 0 else None
            want = C.oracle(raw, f, lengths, 2.0, 1.0, g, s=0.5)
            assert C.same_bits(yd.detach().numpy(), want["yd"].astype(np.float32))
            assert (yd is x) == (p == 0) and not ar_part.requires_grad and not tar_part.requires_grad and penalty.requires_grad
            pb, qb = stock_bounds(T * B * H)
            assert abs(float(ar_part) - want["parts"][0]) <= pb * want["parts"][0] + C.F32_TINY
            assert abs(float(tar_part) - want["parts"][1]) <= pb * want["parts"][1] + C.F32_TINY
            assert abs(float(penalty.detach()) - want["penalty"]) <= qb * want["penalty"] + C.F32_TINY
            (grad,) = torch.autograd.grad([yd, penalty], x, [torch.tensor(g), torch.tensor(0.5)])
            err = np.abs(grad.numpy().astype(np.float64) - want["draw"])
            assert np.all(err <= C.gamma(STOCK_DRAW) * want["magnitude"] + C.F32_TINY), err.max()


def small_model(dropout=0.0, layers=2):
    torch.manual_seed(5 + layers)
    model = Model(64, 32, layers, dropout, 0.1, lstm_type="custom")
    x, y = torch.randint(0, 64, (6, 3)), torch.randint(0, 64, (6, 3))
    return model, x, y


@pytest.mark.parametrize("masked", [False, True], ids=["all", "lengths"])
def test_model_loss_on_the_cpu_is_the_contract(masked):
    model, x, y = small_model()
    lengths = torch.tensor([6, 0, 4]) if masked else None
    kw = dict(lengths=lengths) if masked else {}
    h, _ = model.features(x, model.state_init(3))
    want = C.oracle(h.detach().numpy(), None, None if lengths is None else lengths.numpy(), 2.0, 1.0)
    plain, _ = model.loss(x, y, model.state_init(3), return_parts=True, **kw)
    out, states = model.loss(x, y, model.state_init(3), ar=2.0, tar=1.0, return_parts=True, **kw)
    assert len(plain) == 5 and len(out) == 7 and len(states) == 2
    assert all(torch.equal(a, b) for a, b in zip(plain[1:], out[1:5]))                 # the head's parts: the plain call's bits
    pb, qb = stock_bounds(h.numel())
    assert abs(float(out[5]) - want["parts"][0]) <= pb * want["parts"][0] and abs(float(out[6]) - want["parts"][1]) <= pb * want["parts"][1]
    assert not out[5].requires_grad and not out[6].requires_grad
    assert float(out[0].detach()) == pytest.approx(float(plain[0].detach()) + want["penalty"], rel=1e-6)
    # loss / B is AWD-LSTM's objective with its alpha and beta (unmasked), under both normalize settings
    if not masked:
        awd = float(plain[0].detach()) / 3 + 2.0 * float(h.detach().pow(2).mean()) + 1.0 * float((h.detach()[1:] - h.detach()[:-1]).pow(2).mean())
        for normalize in ("rows", "tokens"):
            loss, _ = model.loss(x, y, model.state_init(3), ar=2.0, tar=1.0, normalize=normalize)
            assert float(loss.detach()) / 3 == pytest.approx(awd, rel=1e-6)
    # gradients: the same objective written out in stock ops on the features
    model.zero_grad()
    loss, _ = model.loss(x, y, model.state_init(3), ar=2.0, tar=1.0, **kw)
    loss.backward()
    got = {k: v.grad.clone() for k, v in model.named_parameters()}
    model.zero_grad()
    h, _ = model.features(x, model.state_init(3))
    m = torch.ones(6, 3, dtype=torch.bool) if lengths is None else torch.arange(6)[:, None] < lengths[None, :]
    n_ar, n_tar = max(32 * int(m.sum()), 1), max(32 * int((m[1:] & m[:-1]).sum()), 1)
    penalty = 3 * (2.0 * (h.pow(2) * m[:, :, None]).sum() / n_ar + 1.0 * ((h[1:] - h[:-1]).pow(2) * (m[1:] & m[:-1])[:, :, None]).sum() / n_tar)
    ref = F.lm_head_objective_loss(h, model.fc.w, model.fc.b, y, **kw) + penalty
    ref.backward()
    for k, v in model.named_parameters():
        scale = max(float(v.grad.abs().max()), 1e-6)
        assert float((got[k] - v.grad).abs().max()) <= 1e-5 * scale + 1e-8, k


def test_training_mode_on_the_cpu_drops_the_top_output_once_and_regularises_the_raw_one():
    model, x, y = small_model(dropout=0.5)
    model.train()
    seen = {}
    real = F.activation_regularizer_stock

    def spy(raw, **kw):
        seen.update(raw=raw, **kw)
        return real(raw, **kw)
    F.activation_regularizer_stock = spy
    try:
        out, _ = model.loss(x, y, model.state_init(3), ar=2.0, tar=1.0, return_parts=True)
    finally:
        F.activation_regularizer_stock = real
    raw, f = seen["raw"], seen["factors"]
    assert set(f.unique().tolist()) == {0.0, 2.0} and not (raw == 0).any()              # the top output came undropped
    want = C.oracle(raw.detach().numpy(), f.numpy(), None, 2.0, 1.0)
    pb, _ = stock_bounds(raw.numel())
    assert abs(float(out[5]) - want["parts"][0]) <= pb * want["parts"][0] and abs(float(out[6]) - want["parts"][1]) <= pb * want["parts"][1]
    out[0].backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())


def test_the_parts_their_scaling_and_which_one_is_not_formed():
    model, x, y = small_model()
    st = lambda: model.state_init(3)
    both, _ = model.loss(x, y, st(), ar=2.0, tar=1.0, return_parts=True)
    heavy, _ = model.loss(x, y, st(), ar=4.0, tar=3.0, return_parts=True)
    assert torch.equal(both[5], heavy[5]) and torch.equal(both[6], heavy[6])             # not multiplied by their weights
    # (the loss is a float32 near heavy[0]: the difference carries its half unit in the last place twice over)
    assert float((heavy[0] - heavy[1]).detach()) == pytest.approx(4.0 * float(both[5]) + 3.0 * float(both[6]), rel=0, abs=2.0 ** -22 * float(heavy[0].detach()))
    only_ar, _ = model.loss(x, y, st(), ar=2.0, return_parts=True)
    only_tar, _ = model.loss(x, y, st(), tar=1.0, return_parts=True)
    assert torch.equal(only_ar[5], both[5]) and float(only_ar[6]) == 0.0 and torch.equal(only_tar[6], both[6]) and float(only_tar[5]) == 0.0
    h, _ = model.features(x, st())
    assert float(both[5]) == pytest.approx(3 * float(h.detach().pow(2).mean()), rel=1e-6)           # B AR, B TAR
    assert float(both[6]) == pytest.approx(3 * float((h.detach()[1:] - h.detach()[:-1]).pow(2).mean()), rel=1e-6)
    # a term that is off is not formed: NaN activations in it do not reach the loss
    raw = torch.full((1, 2, 4), 3.0)
    _, penalty, parts = vmlmf_amd.activation_regularizer(raw, ar=0.0, tar=1.0)
    assert float(penalty.detach()) == 0.0 and float(parts[0]) == 0.0 and float(parts[1]) == 0.0        # T == 1: 0, not NaN
    plain, _ = model.loss(x, y, st(), return_parts=True)
    assert len(plain) == 5 and len(model.loss(x, y, st(), ar=0.0, tar=0.0, return_parts=True)[0]) == 5


def test_every_bad_argument_is_a_value_error_before_any_work():
    model, x, y = small_model()

    class Tripwire(Exception):
        pass

    def trip(*a, **k):
        raise Tripwire
    model.features = model._features = trip
    st = model.state_init(3)
    bad = [dict(ar=-1.0), dict(tar=-0.5), dict(ar=float("nan")), dict(tar=float("inf")), dict(ar=True), dict(tar=False), dict(ar="2"),
           dict(ar=2.0, lengths=torch.tensor([6.0, 4.0, 1.0])), dict(tar=1.0, label_smoothing=1.0), dict(ar=2.0, normalize="mean"),
           dict(ar=2.0, unlikelihood=0.5, negatives=torch.zeros(6, 3, 0, dtype=torch.int64))]
    for kw in bad:
        with pytest.raises(ValueError):
            model.loss(x, y, st, **kw)
    with pytest.raises(Tripwire):                      # a good call reaches the layers
        model.loss(x, y, st, ar=2.0)
    with pytest.raises(TypeError):                     # keyword-only
        vmlmf_amd.activation_regularizer(torch.zeros(2, 2, 4), 2.0, 1.0)
    raw = torch.zeros(2, 3, 4)
    for kw in (dict(ar=-1.0, tar=0.0), dict(ar=0.0, tar=True), dict(ar=1.0, tar=1.0, p=1.0), dict(ar=1.0, tar=1.0, p=-0.1),
               dict(ar=1.0, tar=1.0, lengths=torch.tensor([1, 2]))):
        with pytest.raises(ValueError):
            vmlmf_amd.activation_regularizer(raw, **kw)
    with pytest.raises(ValueError):
        vmlmf_amd.activation_regularizer(torch.zeros(3, 4), ar=1.0, tar=1.0)
    sig = inspect.signature(Model.loss).parameters
    assert sig["ar"].default == 0.0 and sig["tar"].default == 0.0 and sig["ar"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(vmlmf_amd.activation_regularizer).parameters) == ["raw", "ar", "tar", "p", "snap", "site", "lengths",
                                                                                   "layer_desc", "batch_scale"]
    assert list(inspect.signature(Model.features).parameters) == ["self", "x", "states"]


def test_with_both_weights_at_zero_the_new_code_is_never_entered():
    model, x, y = small_model()
    today, _ = model.loss(x, y, model.state_init(3))
    masked, _ = model.loss(x, y, model.state_init(3), lengths=torch.tensor([6, 2, 6]))

    class Tripwire(Exception):
        pass

    def trip(*a, **k):
        raise Tripwire
    model._regularized_loss = trip
    real = F.activation_regularizer, F.activation_regularizer_stock
    F.activation_regularizer = F.activation_regularizer_stock = trip
    try:
        for kw in (dict(), dict(ar=0.0, tar=0.0), dict(ar=0, tar=0.0)):
            loss, _ = model.loss(x, y, model.state_init(3), **kw)
            assert torch.equal(loss, today), kw
        loss, _ = model.loss(x, y, model.state_init(3), ar=0.0, tar=0.0, lengths=torch.tensor([6, 2, 6]))
        assert torch.equal(loss, masked)
        with pytest.raises(Tripwire):
            model.loss(x, y, model.state_init(3), tar=1.0)
    finally:
        F.activation_regularizer, F.activation_regularizer_stock = real


def test_the_library_exports_the_entry_points_and_refuses_bad_arguments():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "vmlmf_hip.h")).read()
    for name in ("vmlmf_actreg_forward", "vmlmf_actreg_backward"):
        assert hasattr(handle, name) and name in _lib.SYMBOLS and f"int {name}(" in header
    assert "size_t vmlmf_actreg_scratch_floats(" in header and f"#define VMLMF_ACTREG_STATS {_lib.ACTREG_STATS}\n" in header
    assert _lib.ABI_VERSION == 13 and handle.vmlmf_abi_version() == 13
    for name in ("activation_regularizer", "activation_regularizer_stock"):
        assert name in vmlmf_amd.__all__ and getattr(vmlmf_amd, name) is getattr(F, name)
    lib = _lib.lib()
    for (T, B, H) in C.SHAPES + [(35, 32, 650), (70, 256, 650)]:
        gx, gy = C.workgroups(T, B, H)
        assert lib.vmlmf_actreg_scratch_floats(T, B, H) == 2 * gx * gy
    assert lib.vmlmf_actreg_scratch_floats(0, 2, 8) == 0
    fake = ctypes.c_void_p(4096)                       # the launch is never reached: no device is touched
    fl = ctypes.c_float

    def fwd(T=2, B=2, H=8, raw=fake, yd=fake, ar=2.0, tar=1.0, scale=2.0, p=0.5, state=fake, stats=fake, scratch=fake, ticket=fake):
        return lib.vmlmf_actreg_forward(T, B, H, raw, yd, None, fl(ar), fl(tar), fl(scale), fl(p), state, 1, None, stats, scratch, ticket, None)

    def bwd(T=2, B=2, H=8, raw=fake, g=fake, draw=ctypes.c_void_p(8192), ar=2.0, tar=1.0, p=0.5, state=fake, stats=fake):
        return lib.vmlmf_actreg_backward(T, B, H, raw, g, draw, None, fl(ar), fl(tar), fl(p), state, 1, None, stats, None, None)
    for kw in (dict(T=0), dict(B=0), dict(H=0), dict(raw=None), dict(yd=None), dict(ar=-1.0), dict(tar=float("nan")), dict(ar=float("inf")),
               dict(scale=-1.0), dict(p=1.0), dict(p=-0.5), dict(state=None), dict(stats=None), dict(scratch=None), dict(ticket=None)):
        assert fwd(**kw) == _lib.E_BADARG, kw
        assert lib.vmlmf_last_error().decode()
    for kw in (dict(T=0), dict(raw=None), dict(g=None), dict(draw=None), dict(draw=fake), dict(tar=-1.0), dict(p=1.0), dict(state=None),
               dict(stats=None)):
        assert bwd(**kw) == _lib.E_BADARG, kw
    assert fwd(T=1 << 17, B=1 << 15) == _lib.E_UNSUPPORTED
    wrong = _lib.make_desc(_lib.V3_LM, 2, 2, 16, 16, 4, [4], time_major=True)
    assert lib.vmlmf_actreg_forward(2, 2, 8, fake, fake, None, fl(2.0), fl(1.0), fl(2.0), fl(0.5), fake, 1, ctypes.byref(wrong), fake, fake,
                                    fake, None) == _lib.E_BADARG
