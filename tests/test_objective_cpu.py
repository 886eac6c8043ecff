"""CPU: the general training objective of the LM head - the fp64 oracle of objective_cases.py against F.cross_entropy, the stock-op
formulation under autograd against the oracle, context_negatives, the argument checks and Model.loss's keywords on CPU tensors."""
import os
import sys

import numpy as np
import pytest
import torch

import objective_cases as C
import vmlmf_amd
from vmlmf_amd import Model
from vmlmf_amd import functional as F

COMBOS = [(0.0, 0.0, 0.0, 0), (0.1, 0.0, 0.0, 0), (0.0, 1e-2, 0.0, 0), (0.0, 0.0, 0.7, 1), (0.0, 0.0, 0.7, 8), (0.1, 1e-2, 0.7, 64)]


@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5])
def test_the_oracle_is_cross_entropy_with_label_smoothing_and_ignore_index(eps, mask):
    R, V = 13, 64
    z, bias, y, _ = C.scores_case(R, V, 2.0, 5, 0, mask=mask)
    zt = torch.tensor(z.astype(np.float64) + bias, requires_grad=True)
    yt = torch.tensor(np.where(y == -1, -100, y))
    want = torch.nn.functional.cross_entropy(zt, yt, label_smoothing=eps, ignore_index=-100, reduction="sum")
    want.backward()
    got = C.oracle(zt.detach().numpy(), y, 1.0, eps=eps)
    assert mask == bool((y == -1).any())
    assert abs(got["loss"] - want.item()) <= 1e-12 * abs(want.item())
    assert np.abs(got["dz"] - zt.grad.numpy()).max() <= 1e-13
    assert np.all(got["dz"][y == -1] == 0.0)


def stock64(z, bias, y, B, eps, zeta, alpha, neg):
    zt = torch.tensor(z.astype(np.float64) + bias, requires_grad=True)
    out = F.objective_loss_stock(zt, torch.tensor(y).reshape(-1, B), label_smoothing=eps, z_loss=zeta, unlikelihood=alpha,
                                 negatives=None if neg is None else torch.tensor(neg))
    out[0].backward()
    return out, zt.grad.numpy()


@pytest.mark.parametrize("eps,zeta,alpha,K", COMBOS)
def test_the_stock_formulation_under_autograd_is_the_oracle_in_fp64(eps, zeta, alpha, K):
    """Loss, parts and the closed-form gradient, with masked rows, duplicate, padding and target-equal negatives, amplitude 2 and 30."""
    R, V, B = 12, 64, 3
    for amp in (2.0, 30.0):
        z, bias, y, neg = C.scores_case(R, V, amp, 11 + K, K)
        want = C.oracle(z.astype(np.float64) + bias, y, B / R, eps, zeta, alpha, neg)
        out, grad = stock64(z, bias, y, B, eps, zeta, alpha, neg)
        got = [v.item() for v in out]
        assert abs(got[0] - want["loss"]) <= 1e-12 * abs(want["loss"]), (amp, got[0], want["loss"])
        assert np.abs(np.array(got[1:]) - want["parts"]).max() <= 1e-12 * np.abs(want["parts"]).max(), (amp, got, want["parts"])
        assert np.abs(grad - want["dz"]).max() <= 1e-13 * max(np.abs(want["dz"]).max(), 1.0), amp
        if alpha > 0 and amp == 2.0:                   # (at amplitude 30 a lone negative's probability can round to nothing)
            assert want["ul"] > 0


def test_the_clamp_has_the_floors_value_and_no_gradient():
    V = 64
    z = np.zeros((1, V))
    z[0, 5] = 20.0
    y, neg = np.array([1]), np.array([[5, 7]])
    want = C.oracle(z, y, 1.0, alpha=1.0, negatives=neg)
    without = C.oracle(z, y, 1.0, alpha=1.0, negatives=np.array([[7, -1]]))
    assert abs((want["ul"] - without["ul"]) + np.log(1e-5)) <= 1e-12
    assert np.array_equal(want["dz"], without["dz"])
    out, grad = stock64(z.astype(np.float32), np.zeros(V, np.float32), y, 1, 0.0, 0.0, 1.0, neg)
    assert abs(out[4].item() - want["ul"]) <= 1e-12 * want["ul"] and np.abs(grad - want["dz"]).max() <= 1e-14


def test_a_target_outside_the_vocabulary_is_nan_with_a_finite_gradient_in_stock_ops():
    z, bias, y, _ = C.scores_case(8, 64, 2.0, 3, 0)
    y[1] = 64
    out, grad = stock64(z, bias, y, 2, 0.1, 1e-2, 0.0, None)
    assert np.isnan(out[0].item()) and np.isnan(out[1].item()) and np.isfinite(out[3].item()) and np.isfinite(grad).all()


def test_context_negatives_is_the_python_loop():
    torch.manual_seed(0)
    x = torch.randint(0, 9, (7, 3))
    got = vmlmf_amd.context_negatives(x)
    assert got.shape == (7, 3, 7) and got.dtype == torch.int64
    for t in range(7):
        for b in range(3):
            assert got[t, b].tolist() == [int(x[j, b]) for j in range(t + 1)] + [-1] * (6 - t)
    with pytest.raises(ValueError):
        vmlmf_amd.context_negatives(x.float())


def small_model(layers=1):
    torch.manual_seed(3 + layers)
    model = Model(64, 32, layers, 0.0, 0.1)
    x, y = torch.randint(0, 64, (6, 3)), torch.randint(0, 64, (6, 3))
    return model, x, y


def test_every_bad_argument_is_a_value_error_before_any_work():
    model, x, y = small_model()

    class Tripwire(Exception):
        pass

    def features(*a, **k):
        raise Tripwire
    model.features = features
    st = model.state_init(3)
    neg = torch.zeros(6, 3, 4, dtype=torch.int64)
    bad = [dict(label_smoothing=1.0), dict(label_smoothing=-0.1), dict(label_smoothing=float("nan")), dict(label_smoothing=True),
           dict(z_loss=-1.0), dict(z_loss=float("inf")), dict(z_loss=float("nan")),
           dict(unlikelihood=-0.5), dict(unlikelihood=float("inf")), dict(unlikelihood=float("nan")),
           dict(normalize="mean"), dict(normalize=None),
           dict(lengths=[6, 4, 1]), dict(lengths=torch.tensor([6, 4])), dict(lengths=torch.tensor([6.0, 4.0, 1.0])),
           dict(lengths=torch.tensor([True, False, True])), dict(lengths=torch.tensor([[6, 4, 1]])),
           dict(unlikelihood=0.5, negatives=neg.int()), dict(unlikelihood=0.5, negatives=neg.tolist()),
           dict(unlikelihood=0.5, negatives=neg[:5]), dict(unlikelihood=0.5, negatives=neg.reshape(-1)),
           dict(unlikelihood=0.5, negatives=torch.zeros(6, 3, 0, dtype=torch.int64)),
           dict(unlikelihood=0.5, negatives=torch.zeros(6, 3, 257, dtype=torch.int64))]
    for kw in bad:
        with pytest.raises(ValueError):
            model.loss(x, y, st, **kw)
    with pytest.raises(Tripwire):                      # a good call reaches the features
        model.loss(x, y, st, label_smoothing=0.1)
    with pytest.raises(TypeError):                     # keyword-only
        model.loss(x, y, st, torch.tensor([6, 4, 1]))
    h, w, b = torch.randn(6, 3, 32), torch.randn(64, 32), torch.randn(64)
    for kw in bad + [dict(unlikelihood=0.5)]:          # the function has no x: no default negatives
        with pytest.raises(ValueError):
            F.lm_head_objective_loss(h, w, b, y, **kw)
    assert vmlmf_amd.lm_head_objective_loss is F.lm_head_objective_loss


def test_model_loss_with_everything_off_has_todays_bits_on_the_cpu():
    model, x, y = small_model()
    h, _ = model.features(x, model.state_init(3))
    today = F.lm_head_loss(h, model.fc.w, model.fc.b, y)      # what Model.loss was: this call on the features and nothing else
    for kw in (dict(), dict(normalize="tokens"), dict(negatives=torch.zeros(6, 3, 2, dtype=torch.int64))):
        loss, states = model.loss(x, y, model.state_init(3), **kw)
        assert torch.equal(loss, today) and len(states) == 1


@pytest.mark.parametrize("layers", [1, 2])
def test_model_loss_with_all_four_on_is_the_stock_formula_on_the_models_scores(layers):
    model, x, y = small_model(layers)
    lengths = torch.tensor([6, 4, 1])
    kw = dict(label_smoothing=0.1, z_loss=1e-2, unlikelihood=0.7)
    for normalize in ("rows", "tokens"):
        model.zero_grad()
        out, _ = model.loss(x, y, model.state_init(3), lengths=lengths, normalize=normalize, return_parts=True, **kw)
        assert len(out) == 5 and not any(t.requires_grad for t in out[1:])
        out[0].backward()
        got = {n: p.grad.clone() for n, p in model.named_parameters()}
        model.zero_grad()
        scores, _ = model(x, model.state_init(3))
        want = F.objective_loss_stock(scores, y, lengths=lengths, negatives=vmlmf_amd.context_negatives(x), normalize=normalize, **kw)
        want[0].backward()
        for a, c in zip(out, want):
            assert torch.allclose(a, c.detach(), rtol=1e-6, atol=0.0)
        for n, p in model.named_parameters():
            assert torch.allclose(got[n], p.grad, rtol=1e-5, atol=1e-8), n
        # ... and the oracle on the same scores
        ym = np.where(np.arange(6)[:, None] < lengths.numpy()[None, :], y.numpy(), -1).reshape(-1)
        scale = 3 / 18 if normalize == "rows" else 3 / 11
        ref = C.oracle(scores.detach().numpy(), ym, scale, 0.1, 1e-2, 0.7, vmlmf_amd.context_negatives(x).reshape(18, 6).numpy())
        C.assert_losses(out, ref, normalize)


def test_full_lengths_with_token_normalisation_is_row_normalisation():
    model, x, y = small_model()
    full = torch.tensor([6, 6, 6])
    a, _ = model.loss(x, y, model.state_init(3), lengths=full, normalize="tokens", label_smoothing=0.1, return_parts=True)
    b, _ = model.loss(x, y, model.state_init(3), lengths=full, normalize="rows", label_smoothing=0.1, return_parts=True)
    c, _ = model.loss(x, y, model.state_init(3), normalize="tokens", label_smoothing=0.1, return_parts=True)
    for u, v, w in zip(a, b, c):
        assert torch.allclose(u, v, rtol=1e-6, atol=0.0) and torch.equal(v, w)
    none, _ = model.loss(x, y, model.state_init(3), lengths=torch.tensor([0, 0, 0]), normalize="tokens", unlikelihood=0.5, return_parts=True)
    assert all(t.item() == 0.0 for t in none)


def test_the_library_exports_and_refuses_bad_arguments_under_abi_13():
    import ctypes
    from vmlmf_amd import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("vmlmf_objective_scratch_floats", "vmlmf_objective_forward_grad"):
        assert hasattr(handle, name) and name in _lib.SYMBOLS
    lib = _lib.lib()
    assert lib.vmlmf_abi_version() == _lib.ABI_VERSION == 13
    assert lib.vmlmf_objective_scratch_floats(7, 64) == 7 * 64 and lib.vmlmf_objective_scratch_floats(8960, 10000) == 512 * 10000
    assert ctypes.sizeof(_lib.Objective) == 40
    fake = ctypes.c_void_p(4096)
    call = lambda V, obj: lib.vmlmf_objective_forward_grad(4, V, fake, None, fake, ctypes.c_float(1.0), ctypes.byref(obj), fake, fake, None, fake, None)
    O = _lib.Objective
    for obj in (O(label_smoothing=1.0), O(label_smoothing=-0.1), O(label_smoothing=float("nan")), O(z_loss=-1.0), O(z_loss=float("inf")),
                O(unlikelihood=-1.0), O(unlikelihood=float("nan")), O(k=-1), O(k=257, negatives=4096), O(unlikelihood=0.5),
                O(unlikelihood=0.5, negatives=4096, k=0), O(unlikelihood=0.5, k=4)):
        assert call(8, obj) == _lib.E_BADARG and len(lib.vmlmf_last_error()) > 10
    assert call(10, O()) == _lib.E_UNSUPPORTED and b"12288" in lib.vmlmf_last_error()
    assert call(12292, O(label_smoothing=0.1)) == _lib.E_UNSUPPORTED


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="llvm-objdump of the ROCm toolchain not present")
def test_the_objective_kernels_use_no_scratch_and_keep_two_workgroups_per_cu():
    """objective_grad_kernel claims __launch_bounds__(256, 2): one instantiation, its VGPRs + AGPRs within 256, nothing spilled, the
    bitmap and the reduction words its only LDS; its finish likewise."""
    from vmlmf_amd import _lib
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_budget
    ks = {d: k for d, k in kernel_budget.kernels(_lib.LIB_PATH).items() if "objective_" in d}
    assert len(ks) == 2 and any("objective_grad_kernel" in d for d in ks) and any("objective_finish_kernel" in d for d in ks), sorted(ks)
    for d, k in ks.items():
        assert k.get("scratch_insts", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, (d, k)
        assert k.get("vgpr_count", 0) + k.get("agpr_count", 0) <= 256, (d, k)
        assert k.get("group_segment_fixed_size", 0) <= 2048, (d, k)
