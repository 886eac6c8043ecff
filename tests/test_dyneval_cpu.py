"""CPU: dynamic evaluation (vmlmf_amd.dyneval) in its stock-op form against the fp64 oracle, the argument checks, the way back to
theta0, the statistics' round trip and what score() puts back when something is raised.  The fused launches: test_gpu_dyneval.py."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import dyneval_cases as C
import vmlmf_amd
from vmlmf_amd import DynamicEval, Model, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYPER = dict(lr=C.LR, decay=C.DECAY, eps=C.EPS)


def small_model(seed=0):
    torch.manual_seed(seed)
    return Model(64, 8, 1, 0.0, 0.1, lstm_type="custom")      # the dense layer in stock ops: what runs on the CPU


def text(seed, T, B, V=64):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, V, (T, B), generator=g)


def with_statistics(model, **hyper):
    de = DynamicEval(model, **{**HYPER, **hyper})
    states = None
    for k in range(3):
        states = de.accumulate(text(10 + k, 6, 3), text(20 + k, 6, 3), states)
    de.finalize()
    return de


@pytest.mark.parametrize("max_norm", [0.0, 1e3, 0.05])
def test_the_stock_step_is_the_oracle(max_norm):
    """Elementwise within the rounding bound of the stock ops' order (no more roundings than the kernel's), plus what the fp32
    norm's error adds through the clip coefficient."""
    numels = C.SIZES
    theta, theta0, r, g = C.step_case(numels, seed=4)
    m = C.mean_rms(r)
    new, norm, scale, clamped = C.step_oracle(theta, theta0, r, g, lr=C.LR, decay=C.DECAY, m=m, eps=C.EPS, max_norm=max_norm)
    bound = np.concatenate(clamped)
    assert bound.any() and not bound.all()
    params = [torch.tensor(a) for a in theta]
    grads = [torch.tensor(a) for a in g]
    got = vmlmf_amd.dyneval_step_stock(params, grads, [torch.tensor(a) for a in theta0], [torch.tensor(a) for a in r], lr=C.LR,
                                       decay=C.DECAY, inv_mean_rms=1.0 / m, eps=C.EPS, max_norm=max_norm)
    assert abs(float(got) - norm) <= C.NORM_RTOL * norm
    assert max_norm == 0 or (max_norm == 0.05) == (norm > max_norm)            # one variant clips, one does not
    upd = C.update_term(r, g, lr=C.LR, eps=C.EPS, max_norm=max_norm, norm=norm)
    for p, want, s, u, g0, gt in zip(params, new, scale, upd, g, grads):
        tol = C.K_ROUNDINGS * C.U * s + (C.NORM_RTOL * u if max_norm > 0 else 0.0)
        assert (np.abs(p.numpy().astype(np.float64) - want) <= tol).all()
        assert np.array_equal(gt.numpy().view(np.uint32), g0.view(np.uint32))       # gradients: never written


def test_the_stock_step_skips_on_a_norm_that_is_not_finite():
    theta, theta0, r, g = C.step_case([5, 1025, 3], seed=5)
    g[1][17] = np.nan
    params = [torch.tensor(a) for a in theta]
    args = ([torch.tensor(a) for a in theta0], [torch.tensor(a) for a in r])
    kw = dict(lr=C.LR, decay=C.DECAY, inv_mean_rms=1.0 / C.mean_rms(r), eps=C.EPS, max_norm=0.25)
    norm = vmlmf_amd.dyneval_step_stock(params, [torch.tensor(a) for a in g], *args, **kw)
    assert not np.isfinite(float(norm))
    assert all(np.array_equal(p.numpy().view(np.uint32), a.view(np.uint32)) for p, a in zip(params, theta))
    g[1][17] = 0.5
    norm = vmlmf_amd.dyneval_step_stock(params, [torch.tensor(a) for a in g], *args, **kw)
    assert np.isfinite(float(norm)) and all(not np.array_equal(p.numpy(), a) for p, a in zip(params, theta))


def test_the_stock_accumulation_is_the_oracle():
    numels = C.SIZES
    ms = [torch.zeros(n) for n in numels]
    want = [np.zeros(n) for n in numels]
    for k in range(3):
        _, _, _, g = C.step_case(numels, seed=30 + k)
        vmlmf_amd.dyneval_accumulate_stock([torch.tensor(a) for a in g], ms)
        want = C.accumulate_oracle(want, g)
    for a, b in zip(ms, want):
        assert (np.abs(a.numpy().astype(np.float64) - b) <= 2 * (3 + 1) * C.U * b).all()     # (square and sum: two roundings a call)


def test_the_stock_loop_is_the_oracle_loop():
    """DynamicEval.score on the CPU against the fp64 loop on the same model in fp64: statistics, five segments (the last one short),
    the clamp binding on part of the elements.  Bounds from the formats: a log-probability is about ln 64 = 4.2, where fp32 steps by
    2^-21; a logsumexp over 64 scores behind 8-wide products and a carried LSTM state is allowed 16 of those steps.  A parameter
    takes five updates of at most K_ROUNDINGS * 2^-24 * (|theta| + |pull| + |update|) <= 13 * 6e-8 * 0.2 = 1.6e-7 each, and the fp32
    gradient's own error (1e-5 relative of updates of a few 1e-3) adds less: 1e-6.  (Measured: 5.4e-7 and 3.8e-8.)"""
    model = small_model()
    de = with_statistics(model, max_norm=0.25)
    tokens = text(1, 22, 2)
    model64 = copy.deepcopy(model).double()
    r = [a.numpy() for a in de._views(de.rms)]
    raw = np.concatenate([(C.DECAY * a.astype(np.float64) / de.mean_rms).ravel() for a in r])
    assert (raw > 1).any() and (raw < 1).any()
    want, _ = C.loop_oracle(C.module_forward(model64), list(model64.parameters()), r, de.mean_rms, tokens[:-1], tokens[1:],
                            [(h.double(), c.double()) for h, c in model64.state_init(2)], segment=5, lr=C.LR, decay=C.DECAY, eps=C.EPS, max_norm=0.25)
    with de:
        got, _ = de.score(tokens)
        moved = [float((p.detach() - p0).abs().max()) for p, p0 in zip(model.parameters(), de._views(de.theta0))]
        for p, q in zip(model.parameters(), model64.parameters()):
            assert float((p.detach().double() - q.detach()).abs().max()) <= 1e-6
    assert min(moved) > 0
    assert got.shape == (21, 2) and got.dtype == torch.float32
    assert np.abs(got.numpy() - want).max() <= 16 * 2.0 ** -21
    # the adaptation is visible: behind the first segment the predictions are not the static model's
    static = DynamicEval(model, lr=0.0, decay=0.0)
    static.load_state_dict(de.state_dict())
    plain, _ = static.score(tokens)
    assert torch.equal(plain[:5], got[:5]) and not torch.equal(plain[5:], got[5:])


@pytest.mark.parametrize("kw", [dict(lr=-1e-3), dict(lr=float("nan")), dict(decay=-0.1), dict(decay=float("inf")), dict(eps=0.0),
                                dict(eps=-1e-5), dict(max_norm=float("nan")), dict(segment=0), dict(segment=2.5), dict(lr="1")])
def test_bad_hyper_parameters_are_value_errors_before_any_work(kw, monkeypatch):
    model = small_model()

    def tripwire(*a, **k):
        raise AssertionError("work before the argument checks")
    monkeypatch.setattr(torch, "zeros", tripwire)
    with pytest.raises(ValueError):
        DynamicEval(model, **{**HYPER, **kw})


def test_lr_and_decay_have_no_defaults():
    with pytest.raises(TypeError):
        DynamicEval(small_model(), lr=1e-3)
    with pytest.raises(TypeError):
        DynamicEval(small_model(), decay=1e-3)
    with pytest.raises(TypeError):
        DynamicEval(small_model(), 1e-3, 1e-3)


def test_models_the_step_cannot_cover_are_value_errors(monkeypatch):
    stock = Model(64, 8, 1, 0.0, 0.1)                       # nn.LSTM layers: their backward needs train mode
    many = small_model()
    many.extra = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(2)) for _ in range(_lib.MAX_TENSORS)])
    half = small_model()
    half.fc.b.data = half.fc.b.data.double()
    monkeypatch.setattr(torch, "zeros", lambda *a, **k: (_ for _ in ()).throw(AssertionError("work before the checks")))
    for model in (stock, many, half):
        with pytest.raises(ValueError):
            DynamicEval(model, **HYPER)


def test_the_order_of_the_calls_is_enforced():
    de = DynamicEval(small_model(), **HYPER)
    with pytest.raises(RuntimeError):
        de.finalize()
    with pytest.raises(RuntimeError):
        de.score(text(1, 7, 2))
    with pytest.raises(RuntimeError):
        de.step()
    de.accumulate(text(2, 6, 3), text(3, 6, 3))
    de.finalize()
    with pytest.raises(RuntimeError):
        de.accumulate(text(2, 6, 3), text(3, 6, 3))
    for bad in (text(1, 1, 2), text(1, 7, 2).float(), text(1, 7, 2)[0]):
        with pytest.raises(ValueError):
            de.score(bad)
    with pytest.raises(ValueError):
        de.score(text(1, 7, 2), text(1, 6, 2))


def test_restore_and_with_give_back_theta0s_bits():
    model = small_model()
    before = [p.detach().clone() for p in model.parameters()]
    de = with_statistics(model)
    de.score(text(1, 12, 2))
    assert not any(torch.equal(p, b) for p, b in zip(model.parameters(), before))
    de.restore()
    assert all(torch.equal(p, b) for p, b in zip(model.parameters(), before))
    with pytest.raises(KeyError):
        with de:
            de.score(text(1, 12, 2))
            assert not torch.equal(model.fc.w, before[-2])
            raise KeyError("mid-evaluation")
    assert all(torch.equal(p.detach().view(torch.int32), b.view(torch.int32)) for p, b in zip(model.parameters(), before))


def test_the_statistics_round_trip():
    model = small_model()
    de = with_statistics(model)
    sd = copy.deepcopy(de.state_dict())
    other = DynamicEval(model, **HYPER)
    other.load_state_dict(sd)
    assert other.minibatches == 3 and other.mean_rms == de.mean_rms
    assert torch.equal(other.rms, de.rms) and torch.equal(other.ms, de.ms)
    with pytest.raises(RuntimeError):
        other.accumulate(text(2, 6, 3), text(3, 6, 3))                  # final statistics stay final
    tokens = text(1, 12, 2)
    with de:
        a, _ = de.score(tokens)
    with other:
        b, _ = other.score(tokens)
    assert torch.equal(a, b)
    # statistics saved before finalize() go on accumulating
    mid = DynamicEval(model, **HYPER)
    mid.accumulate(text(10, 6, 3), text(20, 6, 3))
    late = DynamicEval(model, **HYPER)
    late.load_state_dict(mid.state_dict())
    assert late.rms is None and late.minibatches == 1 and torch.equal(late.ms, mid.ms)
    sd["ms"] = sd["ms"][:-1]
    with pytest.raises(ValueError):
        DynamicEval(model, **HYPER).load_state_dict(sd)


def test_flags_are_restored_after_an_exception_mid_score(monkeypatch):
    model = small_model()
    de = with_statistics(model)
    model.train()
    model.rnns[0].eval()
    model.embed.w.requires_grad_(False)
    modes = [m.training for m in model.modules()]
    calls = []
    step = de.step

    def failing():
        calls.append(model.training)
        if len(calls) == 2:
            raise KeyError("second segment")
        return step()
    monkeypatch.setattr(de, "step", failing)
    with torch.no_grad():
        with pytest.raises(KeyError):
            de.score(text(1, 16, 2))
        assert not torch.is_grad_enabled()
    assert calls == [False, False]                                       # dropout off inside
    assert [m.training for m in model.modules()] == modes
    assert [p.requires_grad for p in model.parameters()] == [False] + [True] * (len(list(model.parameters())) - 1)


def test_return_rows_leaves_the_default_call_alone_and_is_not_differentiable():
    from vmlmf_amd import functional as F
    model = small_model()
    x, y = text(1, 6, 3), text(2, 6, 3)
    h, _ = model.features(x, model.state_init(3))
    plain = F.lm_head_loss(h, model.fc.w, model.fc.b, y)
    loss, rows = F.lm_head_loss(h, model.fc.w, model.fc.b, y, return_rows=True)
    assert torch.equal(plain, loss) and rows.shape == (18,) and not rows.requires_grad and loss.requires_grad
    scores = model(x, model.state_init(3))[0].detach().double()
    want, _ = C.rows_and_loss(scores, y)
    assert float((rows.double() - want).abs().max()) <= 1e-5


def test_the_library_exports_the_two_entry_points_and_refuses_bad_lists():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "vmlmf_hip.h")).read()
    for name in ("vmlmf_dyneval_accumulate", "vmlmf_dyneval_step"):
        assert hasattr(handle, name) and name in _lib.SYMBOLS and f"int {name}(" in header
    assert "DynamicEval" in vmlmf_amd.__all__ and vmlmf_amd.DynamicEval is vmlmf_amd.dyneval.DynamicEval
    lib = _lib.lib()
    tl = _lib.TensorList()
    buf = (ctypes.c_float * 8)()
    at = ctypes.addressof(buf)
    for count in (0, _lib.MAX_TENSORS + 1):                             # the launch is never reached: no device is touched
        tl.count = count
        assert lib.vmlmf_dyneval_accumulate(ctypes.byref(tl), at, None) == _lib.E_BADARG
        assert lib.vmlmf_dyneval_step(ctypes.byref(tl), at, at, 0.1, 0.1, 1.0, 1e-5, 0.0, at, at, None) == _lib.E_BADARG
    tl.count = 1
    tl.param[0], tl.grad[0], tl.numel[0] = at, at, 4
    assert lib.vmlmf_dyneval_accumulate(ctypes.byref(tl), None, None) == _lib.E_BADARG
    assert lib.vmlmf_dyneval_step(ctypes.byref(tl), None, at, 0.1, 0.1, 1.0, 1e-5, 0.0, at, at, None) == _lib.E_BADARG
    assert lib.vmlmf_dyneval_step(ctypes.byref(tl), at, at, 0.1, 0.1, 1.0, 1e-5, 0.0, None, at, None) == _lib.E_BADARG
    tl.state_offset[0] = -4
    assert lib.vmlmf_dyneval_accumulate(ctypes.byref(tl), at, None) == _lib.E_BADARG
    assert lib.vmlmf_dyneval_accumulate(None, at, None) == _lib.E_BADARG
