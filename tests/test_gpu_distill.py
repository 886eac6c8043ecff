"""GPU: knowledge distillation at the LM head - vmlmf_distill_forward_grad through the C ABI, functional.lm_head_distill_loss under
autograd and in a captured graph, Model.distill_loss - against the fp64 oracle of distill_cases.py and the stock-op formulation."""
import ctypes

import numpy as np
import pytest
import torch

import distill_cases as D
from abi_arena import FILLS, Arena, assert_same_bits, assert_written
from hip_util import assert_grad
from vmlmf_amd import Model, _lib, optim, unit_gradient
from vmlmf_amd import functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (R, V, B): one quad and 255 idle threads; 257 quads - thread 0 alone has a second slot; the PTB width; every slot full; one
# workgroup walks two rows, 512 column partials are finished; several workgroups walk three rows
SHAPES = [(1, 8, 1), (3, 1028, 1), (5, 10000, 1), (4, 12288, 2), (513, 64, 3), (1030, 64, 2)]
FORMS = [0, 1, 8, 32]               # dense, top-k


def call(R, V, scale, z, bias, y, alpha, tau, dense=None, top=None, alloc=None):
    """One vmlmf_distill_forward_grad on copies of the numpy operands; returns (loss (3), rowloss (2, R), dz (R, V), dbias (V) or None)
    as device tensors.  alloc(shape, dtype, init, name): where the buffers come from (default: torch)."""
    if alloc is None:
        def alloc(shape, dtype, init, name):
            t = torch.empty(shape, dtype=dtype, device=DEV)
            return t if init is None else t.copy_(torch.as_tensor(init).reshape(t.shape))
    lib = _lib.lib()
    zt = alloc((R, V), torch.float32, z, "scores")
    bt = None if bias is None else alloc((V,), torch.float32, bias, "bias")
    yt = alloc((R,), torch.int64, y, "y")
    kd = _lib.Distill(alpha=alpha, temperature=tau)
    keep = []
    if dense is not None:
        keep.append(alloc((R, V), torch.float32, dense, "teacher"))
        kd.teacher = keep[0].data_ptr()
    else:
        k = top[0].shape[1]
        keep += [alloc((R, k), torch.int64, top[0], "top_tokens"), alloc((R, k), torch.float32, top[1], "top_scores")]
        kd.top_tokens, kd.top_scores, kd.top = keep[0].data_ptr(), keep[1].data_ptr(), k
    loss = alloc((3,), torch.float32, None, "loss")
    rowloss = alloc((2, R), torch.float32, None, "rowloss")
    db = None if bias is None else alloc((V,), torch.float32, None, "dbias")
    scratch = alloc((int(lib.vmlmf_distill_scratch_floats(R, V)),), torch.float32, None, "scratch")
    _lib.check(lib.vmlmf_distill_forward_grad(R, V, zt.data_ptr(), _lib.ptr(bt), yt.data_ptr(), ctypes.c_float(scale), ctypes.byref(kd),
                                              loss.data_ptr(), rowloss.data_ptr(), _lib.ptr(db), scratch.data_ptr(),
                                              _lib.raw_stream(torch.device(DEV, torch.cuda.current_device()))))
    torch.cuda.synchronize()
    return loss, rowloss, zt, db


@pytest.mark.parametrize("k", FORMS, ids=["dense", "top1", "top8", "top32"])
@pytest.mark.parametrize("R,V,B", SHAPES)
def test_the_c_abi_against_the_fp64_oracle(R, V, B, k):
    """Loss triple, rowloss, the in-place gradient and dbias (against the fp64 column sums of the returned gradient) over alpha 0,
    0.3, 1, tau 1, 2, 4, score amplitude 2 and 30, with and without bias; top-k rows hold the target, column 0 and column V - 1."""
    k = min(k, V)
    scale = B / R
    for amp in (2.0, 30.0):
        z, bias, y, dense, top = D.scores_case(R, V, amp, 100 + R + V + k, k)
        if top is not None and R >= 3:
            assert all(any(c in top[0][r] for r in range(R)) for c in (0, V - 1)) and any(y[r] in top[0][r] for r in range(R))
        for use_bias in (True, False):
            zfull = z.astype(np.float64) + (bias if use_bias else 0.0)
            for tau in (1.0, 2.0, 4.0):
                for alpha in (0.0, 0.3, 1.0):
                    want = D.oracle(zfull, y, scale, alpha, tau, teacher=dense, top=top)
                    loss, rowloss, dz, db = call(R, V, scale, z, bias if use_bias else None, y, alpha, tau, dense, top)
                    what = f"amp {amp} bias {use_bias} tau {tau} alpha {alpha}"
                    D.assert_losses(loss.cpu().numpy(), want, what)
                    rl = rowloss.cpu().numpy().astype(np.float64)
                    part = max(np.abs(want["row_hard"]).max(), np.abs(want["row_soft"]).max())
                    assert np.abs(rl[0] - want["row_hard"]).max() <= D.LOSS_REL * part, what
                    assert np.abs(rl[1] - want["row_soft"]).max() <= D.LOSS_REL * part, what
                    g = dz.cpu().numpy().astype(np.float64)
                    assert_grad(g, want["dz"], what + ": dz")
                    if use_bias:
                        assert_grad(db.cpu().numpy(), g.sum(0), what + ": dbias = the column sums of dz")


def test_the_identical_teacher_at_alpha_one_has_no_loss_and_no_gradient():
    """The true soft loss and gradient are zero there: |soft| <= 1e-4 hard, |dz| <= 1e-5 tau scale (not a case for assert_grad)."""
    for R, V, B in SHAPES[:5]:
        z, bias, y, _, _ = D.scores_case(R, V, 30.0, 9, 0)
        for tau in (1.0, 2.0, 4.0):
            loss, _, dz, _ = call(R, V, B / R, z, None, y, 1.0, tau, dense=z)
            total, hard, soft = loss.tolist()
            assert abs(soft) <= 1e-4 * hard and total == soft, (R, V, tau, loss.tolist())
            assert dz.abs().max().item() <= 1e-5 * tau * B / R, (R, V, tau, dz.abs().max().item())


def test_alpha_zero_is_the_nll_head_and_a_target_outside_the_vocabulary_is_nan():
    R, V, B = 513, 64, 3
    z, bias, y, dense, _ = D.scores_case(R, V, 2.0, 21, 0)
    loss, rowloss, dz, db = call(R, V, B / R, z, bias, y, 0.0, 2.0, dense)
    lib = _lib.lib()
    zt, bt, yt = torch.tensor(z, device=DEV), torch.tensor(bias, device=DEV), torch.tensor(y, device=DEV)
    stats, db2 = torch.empty(1 + R, device=DEV), torch.empty(V, device=DEV)
    scratch = torch.empty(lib.vmlmf_nll_grad_scratch_floats(R, V), device=DEV)
    _lib.check(lib.vmlmf_nll_forward_grad(R, V, zt.data_ptr(), bt.data_ptr(), yt.data_ptr(), ctypes.c_float(B / R), stats.data_ptr(),
                                          stats.data_ptr() + 4, db2.data_ptr(), scratch.data_ptr(), _lib.raw_stream(torch.device(DEV, 0))))
    torch.cuda.synchronize()
    assert abs(loss[0].item() - stats[0].item()) <= 1e-4 * stats[0].item() and loss[0].item() == loss[1].item()
    assert_grad(dz.cpu().numpy(), zt.cpu().numpy(), "dz at alpha 0 vs vmlmf_nll_forward_grad")
    assert_grad(db.cpu().numpy(), db2.cpu().numpy(), "dbias at alpha 0 vs vmlmf_nll_forward_grad")
    assert_grad(rowloss[0].cpu().numpy(), stats[1:].cpu().numpy(), "row losses at alpha 0")
    # through the function alpha == 0 IS lm_head_loss: the same launches, the same bits; the teacher is not read
    torch.manual_seed(4)
    h, w, b = torch.randn(5, 6, 24, device=DEV), 0.3 * torch.randn(64, 24, device=DEV), torch.randn(64, device=DEV)
    yy = torch.randint(0, 64, (5, 6), device=DEV)
    grads = []
    for fn in (lambda *a: F.lm_head_loss(*a), lambda *a: F.lm_head_distill_loss(*a, torch.full((5, 6, 64), float("nan"), device=DEV), alpha=0.0)):
        leaves = [t.clone().requires_grad_(True) for t in (h, w, b)]
        out = fn(*leaves, yy)
        out.backward(unit_gradient(out.device))
        grads.append([out.detach()] + [t.grad for t in leaves])
    for a, c in zip(*grads):
        assert torch.equal(a, c)
    # a target outside [0, V): NaN hard and total at every alpha, alpha == 1 included; nothing is read out of bounds
    for bad in (-1, V):
        y2 = y.copy()
        y2[7] = bad
        for alpha in (0.3, 1.0):
            loss, rowloss, dz, _ = call(R, V, B / R, z, bias, y2, alpha, 2.0, dense)
            assert np.isnan(loss[0].item()) and np.isnan(loss[1].item()) and np.isfinite(loss[2].item())
            assert np.isnan(rowloss[0, 7].item()) and torch.isfinite(dz).all()


def call_nll(R, V, scale, z, bias, y, alloc=None):
    """One vmlmf_nll_forward_grad on copies of the numpy operands; returns (loss (1), rowloss (R), dz (R, V), dbias (V) or None)."""
    if alloc is None:
        def alloc(shape, dtype, init, name):
            t = torch.empty(shape, dtype=dtype, device=DEV)
            return t if init is None else t.copy_(torch.as_tensor(init).reshape(t.shape))
    lib = _lib.lib()
    zt = alloc((R, V), torch.float32, z, "scores")
    bt = None if bias is None else alloc((V,), torch.float32, bias, "bias")
    yt = alloc((R,), torch.int64, y, "y")
    loss = alloc((1,), torch.float32, None, "loss")
    rowloss = alloc((R,), torch.float32, None, "rowloss")
    db = None if bias is None else alloc((V,), torch.float32, None, "dbias")
    scratch = alloc((int(lib.vmlmf_nll_grad_scratch_floats(R, V)),), torch.float32, None, "scratch")
    _lib.check(lib.vmlmf_nll_forward_grad(R, V, zt.data_ptr(), _lib.ptr(bt), yt.data_ptr(), ctypes.c_float(scale), loss.data_ptr(),
                                          rowloss.data_ptr(), _lib.ptr(db), scratch.data_ptr(),
                                          _lib.raw_stream(torch.device(DEV, torch.cuda.current_device()))))
    torch.cuda.synchronize()
    return loss, rowloss, zt, db


# one row, every lane but two padding; a partly filled last slot; all twelve slots full; one workgroup walks two rows (its column
# sums carry over); every workgroup walks two or three rows and the finish groups 512 partial rows
NLL_SHAPES = [(1, 8, 1), (3, 1028, 1), (4, 12288, 2), (513, 64, 3), (1030, 64, 2)]


@pytest.mark.parametrize("R,V,B", NLL_SHAPES)
def test_nll_forward_grad_against_the_fp64_oracle_at_alpha_zero(R, V, B):
    """vmlmf_nll_forward_grad: the loss, its rows, the in-place gradient and dbias against the oracle's hard part, score amplitude
    2 and 30, with and without bias."""
    scale = B / R
    for amp in (2.0, 30.0):
        z, bias, y, _, _ = D.scores_case(R, V, amp, 200 + R + V, 0)
        for use_bias in (True, False):
            want = D.oracle(z.astype(np.float64) + (bias if use_bias else 0.0), y, scale, 0.0, 1.0, teacher=z)
            loss, rowloss, dz, db = call_nll(R, V, scale, z, bias if use_bias else None, y)
            what = f"amp {amp} bias {use_bias}"
            assert np.isfinite(loss.item()) and abs(loss.item() - want["hard"]) <= D.LOSS_REL * abs(want["hard"]), (what, loss.item(), want["hard"])
            rl = rowloss.cpu().numpy().astype(np.float64)
            assert np.abs(rl - want["row_hard"]).max() <= D.LOSS_REL * np.abs(want["row_hard"]).max(), what
            assert_grad(dz.cpu().numpy(), want["dz"], what + ": dz")
            if use_bias:
                assert_grad(db.cpu().numpy(), want["db"], what + ": dbias")


@pytest.mark.parametrize("bad", [-1, 64], ids=["minus_one", "V"])
def test_nll_forward_grad_with_a_target_outside_the_vocabulary_is_nan_with_a_finite_gradient(bad):
    R, V, B = 513, 64, 3
    z, bias, y, _, _ = D.scores_case(R, V, 2.0, 22, 0)
    y[7] = bad
    loss, rowloss, dz, db = call_nll(R, V, B / R, z, bias, y)
    assert np.isnan(loss.item()) and np.isnan(rowloss[7].item())
    assert torch.isfinite(rowloss[:7]).all() and torch.isfinite(rowloss[8:]).all()
    assert torch.isfinite(dz).all() and torch.isfinite(db).all()


def test_nll_forward_grad_on_poisoned_exactly_sized_buffers_between_guard_bands():
    """loss is 1 float and rowloss R floats; the same bits whatever the scratch and the outputs held before, twice in a row as well."""
    R, V, B = 513, 64, 3
    z, bias, y, _, _ = D.scores_case(R, V, 2.0, 34, 0)
    runs = []
    for fill in FILLS + (FILLS[0],):
        arena = Arena(DEV, fill)
        out = call_nll(R, V, B / R, z, bias, y, alloc=lambda shape, dtype, init, name: arena.buf(shape, dtype, init=init, name=name))
        assert out[0].numel() == 1 and out[1].numel() == R
        arena.check_guards()
        for name, t in zip(("loss", "rowloss", "scores", "dbias"), out):
            assert_written(arena, name, t)
        runs.append([t.clone() for t in out])
    for other in runs[1:]:
        for name, a, c in zip(("loss", "rowloss", "scores", "dbias"), runs[0], other):
            assert_same_bits(name, a, c, "between fills / runs")


@pytest.mark.parametrize("k", [0, 8], ids=["dense", "top8"])
@pytest.mark.parametrize("R,V,B", [(3, 1028, 1), (513, 64, 3)])
def test_poisoned_exactly_sized_buffers_between_guard_bands(R, V, B, k):
    """The same bits whatever the scratch and the outputs held before, twice in a row as well; every output element written; no
    byte outside a buffer touched."""
    z, bias, y, dense, top = D.scores_case(R, V, 2.0, 33, k)
    runs = []
    for fill in FILLS + (FILLS[0],):
        arena = Arena(DEV, fill)
        loss, rowloss, dz, db = call(R, V, B / R, z, bias, y, 0.3, 2.0, dense, top,
                                     alloc=lambda shape, dtype, init, name: arena.buf(shape, dtype, init=init, name=name))
        arena.check_guards()
        for name, t in (("loss", loss), ("rowloss", rowloss), ("scores", dz), ("dbias", db)):
            assert_written(arena, name, t)
        runs.append([t.clone() for t in (loss, rowloss, dz, db)])
    for other in runs[1:]:
        for name, a, c in zip(("loss", "rowloss", "scores", "dbias"), runs[0], other):
            assert_same_bits(name, a, c, "between fills / runs")


def stock(h, w, b, y, teacher, alpha, tau):
    """The stock-op formulation in fp64 on the CPU: (loss, hard, soft) and, after backward, the leaves' gradients."""
    leaves = [t.detach().double().cpu().requires_grad_(True) for t in (h, w, b)]
    teacher = teacher.detach().double().cpu() if isinstance(teacher, torch.Tensor) else (teacher[0].cpu(), teacher[1].detach().double().cpu())
    scores = torch.addmm(leaves[2], leaves[0].reshape(-1, leaves[0].shape[-1]), leaves[1].t())
    return F.distill_loss_stock(scores, y.cpu(), teacher, alpha, tau), leaves


@pytest.mark.parametrize("k", [0, 8], ids=["dense", "top8"])
def test_autograd_on_a_small_projection_against_fp64_stock_ops(k):
    torch.manual_seed(3)
    Hs, Vs, Ts, Bs = 24, 64, 5, 6
    h0, w0, b0 = torch.randn(Ts, Bs, Hs, device=DEV), 0.3 * torch.randn(Vs, Hs, device=DEV), torch.randn(Vs, device=DEV)
    y = torch.randint(0, Vs, (Ts, Bs), device=DEV)
    dense = 2.0 * torch.randn(Ts, Bs, Vs, device=DEV)
    teacher = dense if k == 0 else tuple(reversed(dense.topk(k, dim=-1)))
    for up in (None, 2.5):
        h, w, b = (t.clone().requires_grad_(True) for t in (h0, w0, b0))
        got = F.lm_head_distill_loss(h, w, b, y, teacher, alpha=0.4, temperature=2.0, return_parts=True)
        assert not got[1].requires_grad and not got[2].requires_grad
        if up is None:
            got[0].backward(unit_gradient(got[0].device))
        else:
            (up * got[0]).backward()
        (wl, wh, ws), leaves = stock(h0, w0, b0, y, teacher, 0.4, 2.0)
        ((up or 1.0) * wl).backward()
        D.assert_losses([v.item() for v in got], dict(loss=wl.item(), hard=wh.item(), soft=ws.item()), f"up {up}")
        for name, a, c in zip("hwb", (h, w, b), leaves):
            assert_grad(a.grad.cpu().numpy(), c.grad.numpy(), f"d{name}, upstream {up}")


def models(layers):
    torch.manual_seed(7 + layers)
    V, Hm = 64, 32
    student = Model(V, Hm, layers, 0.0, 0.1, w_rank=4, u_ranks=[4], lstm_type="vmlmf").to(DEV)
    teacher = Model(V, Hm, layers, 0.0, 0.1, w_rank=16, u_ranks=[16], lstm_type="vmlmf").to(DEV)
    x, y = torch.randint(0, V, (5, 3), device=DEV), torch.randint(0, V, (5, 3), device=DEV)
    return student, teacher, x, y


def stock_model_loss(student, teacher, x, y, alpha, tau):
    """The stock formulation on the same two models: the teacher's scores without autograd, the student's through forward()."""
    with torch.no_grad():
        tscores, _ = teacher(x, teacher.state_init(x.size(1)))
    scores, _ = student(x, student.state_init(x.size(1)))
    return F.distill_loss_stock(scores, y, tscores, alpha, tau)


@pytest.mark.parametrize("layers", [1, 2])
def test_model_distill_loss_of_a_rank_4_student_against_a_rank_16_teacher(layers):
    student, teacher, x, y = models(layers)
    teacher.train()
    out = student.distill_loss(x, y, student.state_init(3), teacher, alpha=0.5, temperature=2.0, return_parts=True)
    assert len(out) == 3 and teacher.training and all(p.grad is None for p in teacher.parameters())
    out[0][0].backward()
    got = {n: p.grad.clone() for n, p in student.named_parameters()}
    student.zero_grad()
    want = stock_model_loss(student, teacher.eval(), x, y, 0.5, 2.0)
    want[0].backward()
    D.assert_losses([v.item() for v in out[0]], dict(loss=want[0].item(), hard=want[1].item(), soft=want[2].item()), "Model.distill_loss")
    for n, p in student.named_parameters():
        assert_grad(got[n].cpu().numpy(), p.grad.cpu().numpy(), n)
    # top=8: the functional call on teacher.score(top=8)'s outputs
    top = student.distill_loss(x, y, student.state_init(3), teacher, top=8)
    _, _, tokens, logprobs, _ = teacher.score(x, y, states=teacher.state_init(3), top=8)
    hfeat, _ = student.features(x, student.state_init(3))
    ref = F.lm_head_distill_loss(hfeat, student.fc.w, student.fc.b, y, (tokens, logprobs))
    assert top[0].item() == ref.item() and len(top) == 3


def test_three_clipped_sgd_steps_end_at_the_stock_op_loops_parameters():
    student, teacher, x, y = models(2)
    twin = Model(64, 32, 2, 0.0, 0.1, w_rank=4, u_ranks=[4], lstm_type="vmlmf").to(DEV)
    twin.load_state_dict(student.state_dict())
    for _ in range(3):
        for m, loss in ((student, lambda: student.distill_loss(x, y, student.state_init(3), teacher)[0]),
                        (twin, lambda: stock_model_loss(twin, teacher, x, y, 0.5, 2.0)[0])):
            m.zero_grad()
            loss().backward()
            optim.clip_sgd_step(list(m.parameters()), 1.0, 0.25)
    for (n, p), q in zip(student.named_parameters(), twin.parameters()):
        assert torch.allclose(p, q, atol=2e-5, rtol=1e-3), (n, (p - q).abs().max().item())


@pytest.mark.parametrize("k", [0, 8], ids=["dense", "top8"])
def test_the_head_loss_captured_into_a_graph_replays_to_the_eager_bits(k):
    torch.manual_seed(5)
    Hs, Vs, Ts, Bs = 24, 64, 5, 6
    h, w, b = (t.requires_grad_(True) for t in (torch.randn(Ts, Bs, Hs, device=DEV), 0.3 * torch.randn(Vs, Hs, device=DEV), torch.randn(Vs, device=DEV)))
    y = torch.randint(0, Vs, (Ts, Bs), device=DEV)
    dense = 2.0 * torch.randn(Ts, Bs, Vs, device=DEV)
    teacher = dense if k == 0 else tuple(t.contiguous() for t in reversed(dense.topk(k, dim=-1)))

    def step():
        for t in (h, w, b):
            t.grad = None
        out = F.lm_head_distill_loss(h, w, b, y, teacher, alpha=0.3, temperature=4.0, return_parts=True)
        out[0].backward(unit_gradient(out[0].device))
        return [*out, h.grad, w.grad, b.grad]

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                              # the eager warm-up: the GEMM forms are timed here, outside the capture
        for _ in range(2):
            eager = [t.clone() for t in step()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for name, a, c in zip(("loss", "hard", "soft", "dh", "dw", "db"), eager, captured):
        assert_same_bits(name, a, c, "between the eager call and the replay")
