"""CPU: knowledge distillation at the LM head (functional.lm_head_distill_loss, Model.distill_loss; C ABI vmlmf_distill_*) - the
exports, the stock-op fallback against the fp64 oracle of distill_cases.py, the oracle's identities, the refusals, the teacher
module's handling, and the register budget of the built kernels."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import distill_cases as D
from hip_util import assert_grad
import vmlmf_amd
from vmlmf_amd import Model, _lib
from vmlmf_amd import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
H = 8
GRID = [(3, 1, 8), (5, 1, 1028), (3, 2, 10000), (2, 2, 12288)]          # (T, B, V): R = 3, 5, 6, 4


def test_the_library_exports_and_binds_the_two_entry_points_under_abi_13():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("vmlmf_distill_scratch_floats", "vmlmf_distill_forward_grad"):
        assert hasattr(handle, name) and name in _lib.SYMBOLS
    lib = _lib.lib()
    assert lib.vmlmf_abi_version() == _lib.ABI_VERSION == 13
    assert lib.vmlmf_distill_scratch_floats(7, 64) == 7 * 64 and lib.vmlmf_distill_scratch_floats(8960, 10000) == 512 * 10000
    assert "lm_head_distill_loss" in vmlmf_amd.__all__ and vmlmf_amd.lm_head_distill_loss is F.lm_head_distill_loss
    # host-side refusals, each with a text: no teacher form, both forms, a top outside [1, 32], a width that is no multiple of four
    fake = ctypes.c_void_p(4096)
    call = lambda V, kd: lib.vmlmf_distill_forward_grad(4, V, fake, None, fake, ctypes.c_float(1.0), ctypes.byref(kd), fake, fake, None, fake, None)
    both = _lib.Distill(alpha=0.5, temperature=2.0, teacher=4096, top_tokens=4096, top_scores=4096, top=4)
    for kd in (_lib.Distill(alpha=0.5, temperature=2.0), both, _lib.Distill(alpha=0.5, temperature=2.0, top_tokens=4096, top_scores=4096, top=33),
               _lib.Distill(alpha=1.5, temperature=2.0, teacher=4096), _lib.Distill(alpha=0.5, temperature=0.0, teacher=4096)):
        assert call(8, kd) == _lib.E_BADARG and len(lib.vmlmf_last_error()) > 10
    assert call(10, _lib.Distill(alpha=0.5, temperature=2.0, teacher=4096)) == _lib.E_UNSUPPORTED and b"12288" in lib.vmlmf_last_error()
    assert call(12292, _lib.Distill(alpha=0.5, temperature=2.0, teacher=4096)) == _lib.E_UNSUPPORTED


def head_case(T, B, V, amp, seed, k):
    """h (T, B, H), weight (V, H), bias (V) whose scores have about the amplitude `amp`, the targets and the teacher of
    distill_cases.scores_case."""
    _, bias, y, dense, top = D.scores_case(T * B, V, amp, seed, k)
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(T, B, H, generator=g)
    w = torch.randn(V, H, generator=g) * (amp / H ** 0.5)
    return h, w, torch.tensor(bias), torch.tensor(y).view(T, B), dense, top


def oracle_for(h, w, b, y, alpha, tau, dense, top):
    hd, wd = h.double().reshape(-1, H).numpy(), w.double().numpy()
    z = hd @ wd.T + (0.0 if b is None else b.double().numpy())
    want = D.oracle(z, y.numpy(), y.size(1) / z.shape[0], alpha, tau, teacher=dense, top=top)
    want["dh"], want["dw"] = (want["dz"] @ wd).reshape(h.shape), want["dz"].T @ hd
    return want


@pytest.mark.parametrize("k", [0, 8], ids=["dense", "top8"])
@pytest.mark.parametrize("T,B,V", GRID)
def test_the_stock_op_fallback_against_the_fp64_oracle(T, B, V, k):
    """CPU tensors take distill_loss_stock under autograd: loss, parts and the gradients of h, weight and bias; score amplitude 2
    and 30, tau 1, 2, 4, alpha 0.3 and 1, with and without bias; the targets include column 0 and column V - 1."""
    for amp in (2.0, 30.0):
        h0, w0, b0, y, dense, top = head_case(T, B, V, amp, 11 + V, k)
        assert 0 in y and V - 1 in y
        teacher = torch.tensor(dense) if dense is not None else (torch.tensor(top[0]).view(T, B, k), torch.tensor(top[1]).view(T, B, k))
        for tau in (1.0, 2.0, 4.0):
            for alpha in (0.3, 1.0):
                for use_bias in (True, False):
                    h, w = h0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
                    b = b0.clone().requires_grad_(True) if use_bias else None
                    got = F.lm_head_distill_loss(h, w, b, y, teacher, alpha=alpha, temperature=tau, return_parts=True)
                    assert not got[1].requires_grad and not got[2].requires_grad
                    got[0].backward()
                    want = oracle_for(h0, w0, b0 if use_bias else None, y, alpha, tau, dense, top)
                    what = f"amp {amp} tau {tau} alpha {alpha} bias {use_bias}"
                    D.assert_losses(got, want, what)
                    assert_grad(h.grad.numpy(), want["dh"], what + ": dh")
                    assert_grad(w.grad.numpy(), want["dw"], what + ": dw")
                    if use_bias:
                        assert_grad(b.grad.numpy(), want["db"], what + ": db")


def test_the_identical_teacher_at_alpha_one_has_no_loss_and_no_gradient():
    """The true soft loss and gradient are zero: relative error means nothing, so |soft| <= 1e-4 hard and |dz| <= 1e-5 tau scale."""
    for (T, B, V) in GRID:
        for amp in (2.0, 30.0):
            z0, bias, y, _, _ = D.scores_case(T * B, V, amp, 5, 0)
            for tau in (1.0, 2.0, 4.0):
                z = torch.tensor(z0).requires_grad_(True)
                loss, hard, soft = F.distill_loss_stock(z, torch.tensor(y).view(T, B), z.detach().clone(), 1.0, tau)
                loss.backward()
                assert abs(soft.item()) <= 1e-4 * hard.item() and abs(loss.item() - soft.item()) <= 1e-6 * hard.item()
                assert z.grad.abs().max().item() <= 1e-5 * tau * (B / (T * B)), (T, B, V, amp, tau, z.grad.abs().max().item())


def test_the_oracles_identities():
    T, B, V = 3, 2, 8
    z, bias, y, dense, _ = D.scores_case(T * B, V, 2.0, 3, 0)
    z = z.astype(np.float64) + bias
    scale = B / (T * B)
    # alpha = 0 is nll_loss (the reference's own formulation, which vmlmf_amd.nll_loss runs on CPU tensors)
    want = D.oracle(z, y, scale, 0.0, 2.0, teacher=dense)
    ref = vmlmf_amd.nll_loss(torch.tensor(z), torch.tensor(y).view(T, B))
    assert abs(want["loss"] - ref.item()) <= 1e-12 * ref.item() and want["loss"] == want["hard"]
    # top-k with k = V is the dense teacher
    tok = np.stack([np.random.Generator(np.random.PCG64(r)).permutation(V) for r in range(T * B)])
    full = D.oracle(z, y, scale, 0.3, 2.0, top=(tok, np.take_along_axis(dense, tok, axis=1)))
    dn = D.oracle(z, y, scale, 0.3, 2.0, teacher=dense)
    assert abs(full["loss"] - dn["loss"]) <= 1e-12 * dn["loss"] and np.abs(full["dz"] - dn["dz"]).max() <= 1e-14
    # a per-row constant added to the teacher changes nothing
    shifted = D.oracle(z, y, scale, 0.3, 2.0, teacher=dense.astype(np.float64) + np.arange(T * B)[:, None] * 3.0)
    assert abs(shifted["soft"] - dn["soft"]) <= 1e-12 * dn["soft"] and np.abs(shifted["dz"] - dn["dz"]).max() <= 1e-14
    # ... through the fallback as well, where an upstream gradient of 2.5 scales all three gradients
    h0, w0, b0, yy, dense, _ = head_case(T, B, V, 2.0, 4, 0)
    grads = []
    for up, teacher in ((1.0, dense), (2.5, dense), (1.0, dense + 7.0)):
        h, w, b = (t.clone().requires_grad_(True) for t in (h0, w0, b0))
        (up * F.lm_head_distill_loss(h, w, b, yy, torch.tensor(teacher), alpha=0.3, temperature=2.0)).backward()
        grads.append([t.grad.double().numpy() for t in (h, w, b)])
    for g1, g25, gs in zip(*grads):
        assert_grad(g25, 2.5 * g1, "upstream 2.5")
        assert_grad(gs, g1, "teacher + constant")
    # and alpha = 0 of the function is lm_head_loss's value
    h, w, b = (t.clone().requires_grad_(True) for t in (h0, w0, b0))
    a0 = F.lm_head_distill_loss(h, w, b, yy, torch.tensor(dense), alpha=0.0, return_parts=True)
    assert abs(a0[0].item() - F.lm_head_loss(h0, w0, b0, yy).item()) <= 1e-5 * a0[0].item() and a0[1].item() == a0[0].item()


def test_every_refusal_is_a_valueerror_raised_without_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", no_library)
    T, B, V = 3, 2, 8
    h, w, b = torch.randn(T, B, H), torch.randn(V, H), torch.randn(V)
    y = torch.randint(0, V, (T, B))
    dense = torch.randn(T, B, V)
    tok, sc = torch.zeros(T, B, 4, dtype=torch.int64), torch.randn(T, B, 4)
    bad_kw = [dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(temperature=0.0), dict(temperature=-1.0),
              dict(temperature=float("inf")), dict(temperature=float("nan"))]
    for kw in bad_kw:
        with pytest.raises(ValueError):
            F.lm_head_distill_loss(h, w, b, y, dense, **kw)
    bad_teachers = [torch.randn(T, B, V + 1), torch.randn(T + 1, B, V), dense.double(), dense[0, 0], (tok, sc[..., :3]), (tok.int(), sc), (tok, sc.double()),
                    (torch.zeros(T, B, 33, dtype=torch.int64), torch.randn(T, B, 33)), (torch.zeros(T, B, 0, dtype=torch.int64), torch.randn(T, B, 0)),
                    (tok,), None, "teacher"]
    for teacher in bad_teachers:
        with pytest.raises(ValueError):
            F.lm_head_distill_loss(h, w, b, y, teacher)
    student = Model(V, H, 1, 0.0, 0.1)
    x = torch.randint(0, V, (T, B))
    for kw in bad_kw + [dict(top=-1), dict(top=33), dict(top=2.0), dict(top=4)]:           # (top with a tensor teacher: nothing to reduce)
        with pytest.raises(ValueError):
            student.distill_loss(x, y, student.state_init(B), dense, **kw)
    for teacher in bad_teachers[:8]:
        with pytest.raises(ValueError):
            student.distill_loss(x, y, student.state_init(B), teacher)
    with pytest.raises(ValueError):
        student.distill_loss(x, y, student.state_init(B), Model(V, H, 1, 0.0, 0.1), top=33)


def test_model_distill_loss_with_a_teacher_model_on_the_cpu():
    """Arity, the teacher's states carried over two minibatches, no gradient into the teacher, its train / eval flags restored -
    after an exception inside the call as well."""
    torch.manual_seed(1)
    T, B, V = 4, 3, 12
    student, teacher = Model(V, H, 1, 0.0, 0.1), Model(V, 16, 2, 0.5, 0.1)
    teacher.train()
    teacher.rnns[1].eval()                                    # a mixed state: every module's own flag comes back
    flags = [m.training for m in teacher.modules()]
    x = torch.randint(0, V, (2 * T, B))
    y = torch.randint(0, V, (2 * T, B))
    out = student.distill_loss(x[:T], y[:T], student.state_init(B), teacher)
    assert len(out) == 3 and out[0].dim() == 0 and out[0].requires_grad
    loss1, states, tstates = out
    assert [m.training for m in teacher.modules()] == flags
    out2 = student.distill_loss(x[T:], y[T:], student.detach(states), teacher, teacher_states=tstates, return_parts=True)
    assert len(out2) == 3 and len(out2[0]) == 3
    # the carried states are those of the teacher over both minibatches in one piece, in eval mode (no dropout)
    teacher.eval()
    with torch.no_grad():
        scores, whole = teacher(x, teacher.state_init(B))
    for (h2, c2), (hw, cw) in zip(out2[2], whole):
        assert torch.allclose(h2, hw, atol=1e-6) and torch.allclose(c2, cw, atol=1e-6)
    # ... and the loss is the functional call on that teacher's scores
    hfeat, _ = student.features(x[T:], student.detach(states))
    want = F.lm_head_distill_loss(hfeat, student.fc.w, student.fc.b, y[T:], scores.view(2 * T, B, V)[T:], return_parts=True)
    assert all(abs(a.item() - b.item()) <= 1e-6 * abs(b.item()) for a, b in zip(out2[0], want))
    # top=k on the CPU: the k best of the teacher's scores
    top = student.distill_loss(x[:T], y[:T], student.state_init(B), teacher, top=4)
    values, tokens = scores.view(2 * T, B, V)[:T].topk(4, dim=-1)
    hfeat, _ = student.features(x[:T], student.state_init(B))
    assert abs(top[0].item() - F.lm_head_distill_loss(hfeat, student.fc.w, student.fc.b, y[:T], (tokens, values)).item()) <= 1e-6 * top[0].item()
    (loss1 + out2[0][0]).backward()
    assert all(p.grad is None for p in teacher.parameters()) and all(p.grad is not None for p in student.parameters())
    # a tensor teacher: (loss, states)
    assert len(student.distill_loss(x[:T], y[:T], student.state_init(B), scores.view(2 * T, B, V)[:T])) == 2

    class Broken(Model):
        def forward(self, x, states):
            raise KeyError("inside the teacher")

    broken = Broken(V, H, 2, 0.5, 0.1).train()
    broken.dropout.eval()
    flags = [m.training for m in broken.modules()]
    with pytest.raises(KeyError):
        student.distill_loss(x[:T], y[:T], student.state_init(B), broken)
    assert [m.training for m in broken.modules()] == flags


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump of the ROCm toolchain not present")
def test_the_distillation_kernels_use_no_scratch_and_keep_two_workgroups_per_cu():
    """distill_grad_kernel claims __launch_bounds__(256, 2): its VGPRs + AGPRs must stay within 256, and nothing of a row may spill;
    the same for the finish it shares with the NLL head, with one row-loss vector and with two."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_budget
    ks = {d: k for d, k in kernel_budget.kernels(_lib.LIB_PATH).items() if "distill_" in d or "head_loss_" in d}
    grad = [d for d in ks if "distill_grad_kernel<" in d]
    assert len(grad) == 2 and any("DenseTeacher" in d for d in grad) and any("TopTeacher" in d for d in grad), sorted(ks)
    assert all(any(f"head_loss_finish_kernel<{parts}>" in d for d in ks) for parts in (1, 2)) and len(ks) == 4, sorted(ks)
    for d, k in ks.items():
        assert k.get("scratch_insts", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, (d, k)
        assert k.get("vgpr_count", 0) + k.get("agpr_count", 0) <= 256, (d, k)
