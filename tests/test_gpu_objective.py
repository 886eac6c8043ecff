"""GPU: the LM head's general training objective - vmlmf_objective_forward_grad through the C ABI, functional.lm_head_objective_loss
under autograd and in a captured graph, Model.loss's keywords - against the fp64 oracle of objective_cases.py and the stock-op
formulation."""
import ctypes

import numpy as np
import pytest
import torch

import objective_cases as C
from abi_arena import FILLS, Arena, assert_same_bits, assert_written
from hip_util import assert_grad
from test_gpu_distill import call_nll
from vmlmf_amd import Model, _lib, context_negatives, optim, unit_gradient
from vmlmf_amd import functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"

# test_gpu_distill.py's: one quad; a second slot for thread 0 alone; the PTB width; every slot full; 512 partials with a workgroup
# walking two rows; three rows per workgroup
SHAPES = [(1, 8, 1), (3, 1028, 1), (5, 10000, 1), (4, 12288, 2), (513, 64, 3), (1030, 64, 2)]
# (eps, zeta, alpha, K); K is capped at V.  The first: a mask only
COMBOS = [(0.0, 0.0, 0.0, 0), (0.1, 0.0, 0.0, 0), (0.0, 1e-2, 0.0, 0), (0.0, 0.0, 0.7, 1), (0.0, 0.0, 0.7, 8), (0.1, 1e-2, 0.7, 256)]


def _torch_alloc(shape, dtype, init, name):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    return t if init is None else t.copy_(torch.as_tensor(init).reshape(t.shape))


def _stream():
    return _lib.raw_stream(torch.device(DEV, torch.cuda.current_device()))


def call(R, V, scale, z, bias, y, eps=0.0, zeta=0.0, alpha=0.0, neg=None, scale_dev=None, alloc=_torch_alloc):
    """One vmlmf_objective_forward_grad on copies of the numpy operands; returns (loss (5), rowloss (4, R), dz (R, V), dbias (V) or
    None) as device tensors.  alloc(shape, dtype, init, name): where the buffers come from."""
    lib = _lib.lib()
    zt = alloc((R, V), torch.float32, z, "scores")
    bt = None if bias is None else alloc((V,), torch.float32, bias, "bias")
    yt = alloc((R,), torch.int64, y, "y")
    obj = _lib.Objective(label_smoothing=eps, z_loss=zeta, unlikelihood=alpha)
    keep = []
    if neg is not None:
        keep.append(alloc(neg.shape, torch.int64, neg, "negatives"))
        obj.negatives, obj.k = keep[-1].data_ptr(), neg.shape[1]
    if scale_dev is not None:
        keep.append(alloc((1,), torch.float32, np.float32(scale_dev), "scale_dev"))
        obj.scale_dev = keep[-1].data_ptr()
    loss = alloc((5,), torch.float32, None, "loss")
    rowloss = alloc((4, R), torch.float32, None, "rowloss")
    db = None if bias is None else alloc((V,), torch.float32, None, "dbias")
    scratch = alloc((int(lib.vmlmf_objective_scratch_floats(R, V)),), torch.float32, None, "scratch")
    _lib.check(lib.vmlmf_objective_forward_grad(R, V, zt.data_ptr(), _lib.ptr(bt), yt.data_ptr(), ctypes.c_float(scale), ctypes.byref(obj),
                                                loss.data_ptr(), rowloss.data_ptr(), _lib.ptr(db), scratch.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return loss, rowloss, zt, db


@pytest.mark.parametrize("R,V,B", SHAPES)
def test_the_c_abi_against_the_fp64_oracle(R, V, B):
    """Loss and the four parts, rowloss, the in-place gradient and dbias (against the fp64 column sums of the returned gradient) over
    the six term combinations, score amplitude 2 and 30, with and without bias, with and without a device scale; rows r % 4 == 2 are
    masked and their gradient rows are exactly zero; the negatives hold a duplicate, the target and padding."""
    scale = B / R
    for amp in (2.0, 30.0):
        for eps, zeta, alpha, K in COMBOS:
            K = min(K, V)
            z, bias, y, neg = C.scores_case(R, V, amp, 300 + R + V, K)
            for use_bias in (True, False):
                zfull = z.astype(np.float64) + (bias if use_bias else 0.0)
                for sdev in (None, 1.7):
                    total = scale if sdev is None else scale * float(np.float32(sdev))
                    want = C.oracle(zfull, y, total, eps, zeta, alpha, neg)
                    loss, rowloss, dz, db = call(R, V, scale, z, bias if use_bias else None, y, eps, zeta, alpha, neg, sdev)
                    what = f"amp {amp} bias {use_bias} eps {eps} zeta {zeta} alpha {alpha} K {K} scale_dev {sdev}"
                    got = loss.cpu().numpy()
                    print(what, "loss", got, "want", want["loss"], want["parts"])
                    C.assert_losses(got, want, what)
                    rl = rowloss.cpu().numpy().astype(np.float64)
                    big = np.abs(want["rows"]).max()
                    for p, name in enumerate(("nll", "smooth", "z", "ul")):
                        assert np.abs(rl[p] - want["rows"][p]).max() <= C.LOSS_REL * big, (what, name)
                    g = dz.cpu().numpy().astype(np.float64)
                    assert_grad(g, want["dz"], what + ": dz")
                    assert not g[y == -1].any(), what + ": a masked row's gradient is zeros"
                    if use_bias:
                        assert_grad(db.cpu().numpy(), g.sum(0), what + ": dbias = the column sums of dz")


@pytest.mark.parametrize("R,V,B", [(513, 64, 3), (5, 10000, 1)])
def test_everything_off_without_a_masked_row_has_the_bits_of_the_nll_head(R, V, B):
    z, bias, y, _ = C.scores_case(R, V, 2.0, 41, 0, mask=False)
    loss, rowloss, dz, db = call(R, V, B / R, z, bias, y)
    nloss, nrow, ndz, ndb = call_nll(R, V, B / R, z, bias, y)
    assert_same_bits("loss", loss[:1], nloss, "against vmlmf_nll_forward_grad")
    assert_same_bits("nll part", loss[1:2], nloss, "against vmlmf_nll_forward_grad")
    assert_same_bits("rowloss[0]", rowloss[0], nrow, "against vmlmf_nll_forward_grad")
    assert_same_bits("scores", dz, ndz, "against vmlmf_nll_forward_grad")
    assert_same_bits("dbias", db, ndb, "against vmlmf_nll_forward_grad")


def test_the_clamp_has_the_floors_value_and_no_gradient():
    """One negative at score +20 over a flat row of 64: 1 - p is about 1.3e-7, under the floor of 1e-5."""
    V = 64
    z = np.zeros((1, V), np.float32)
    z[0, 5] = 20.0
    y = np.array([1], np.int64)
    loss, rowloss, dz, _ = call(1, V, 1.0, z, None, y, alpha=0.7, neg=np.array([[5, -1]], np.int64))
    floor = -np.log(1e-5)
    assert abs(loss[4].item() - floor) <= 1e-6 * floor and abs(rowloss[3, 0].item() - floor) <= 1e-6 * floor
    _, _, without, _ = call(1, V, 1.0, z, None, y, alpha=0.7, neg=np.array([[-1, -1]], np.int64))
    assert_same_bits("scores", dz, without, "with the clamped negative and without it")
    assert_grad(dz.cpu().numpy(), C.oracle(z, y, 1.0, alpha=0.7, negatives=[[5]])["dz"], "dz under the clamp")


def test_a_bad_target_is_nan_with_a_finite_gradient_and_the_mask_everywhere_is_zero():
    R, V, B = 513, 64, 3
    z, bias, y, neg = C.scores_case(R, V, 2.0, 43, 8)
    y2 = y.copy()
    y2[7] = V
    loss, rowloss, dz, db = call(R, V, B / R, z, bias, y2, 0.1, 1e-2, 0.7, neg)
    assert np.isnan(loss[0].item()) and np.isnan(loss[1].item()) and torch.isfinite(loss[2:]).all()
    assert np.isnan(rowloss[0, 7].item()) and torch.isfinite(rowloss[0, :7]).all() and torch.isfinite(rowloss[0, 8:]).all()
    assert torch.isfinite(dz).all() and torch.isfinite(db).all()
    loss, rowloss, dz, db = call(R, V, B / R, z, bias, np.full(R, -1, np.int64), 0.1, 1e-2, 0.7, neg)
    assert not loss.any() and not rowloss.any() and not dz.any() and not db.any()


@pytest.mark.parametrize("R,V,B", [(3, 1028, 1), (513, 64, 3)])
def test_poisoned_exactly_sized_buffers_between_guard_bands(R, V, B):
    """All four terms on: the same bits whatever the scratch and the outputs held before, twice in a row as well; every output
    element written, masked rows included; no byte outside a buffer touched."""
    z, bias, y, neg = C.scores_case(R, V, 2.0, 47, min(256, V))
    runs = []
    for fill in FILLS + (FILLS[0],):
        arena = Arena(DEV, fill)
        out = call(R, V, B / R, z, bias, y, 0.1, 1e-2, 0.7, neg, 1.7,
                   alloc=lambda shape, dtype, init, name: arena.buf(shape, dtype, init=init, name=name))
        arena.check_guards()
        assert out[0].numel() == 5 and out[1].numel() == 4 * R
        for name, t in zip(("loss", "rowloss", "scores", "dbias"), out):
            assert_written(arena, name, t)
        runs.append([t.clone() for t in out])
    for other in runs[1:]:
        for name, a, c in zip(("loss", "rowloss", "scores", "dbias"), runs[0], other):
            assert_same_bits(name, a, c, "between fills / runs")


KW = dict(label_smoothing=0.1, z_loss=1e-2, unlikelihood=0.7)


def test_autograd_on_a_small_projection_against_fp64_stock_ops():
    torch.manual_seed(3)
    Hs, Vs, Ts, Bs = 16, 64, 4, 3
    h0, w0, b0 = torch.randn(Ts, Bs, Hs, device=DEV), 0.3 * torch.randn(Vs, Hs, device=DEV), torch.randn(Vs, device=DEV)
    y = torch.randint(0, Vs, (Ts, Bs), device=DEV)
    neg = torch.randint(-1, Vs, (Ts, Bs, 5), device=DEV)
    lengths = torch.tensor([4, 2, 3], device=DEV)
    for normalize in ("rows", "tokens"):
        for up in (None, 2.5):
            h, w, b = (t.clone().requires_grad_(True) for t in (h0, w0, b0))
            got = F.lm_head_objective_loss(h, w, b, y, lengths=lengths, negatives=neg, normalize=normalize, return_parts=True, **KW)
            assert len(got) == 5 and not any(t.requires_grad for t in got[1:])
            if up is None:
                got[0].backward(unit_gradient(got[0].device))
            else:
                (up * got[0]).backward()
            leaves = [t.detach().double().cpu().requires_grad_(True) for t in (h0, w0, b0)]
            scores = torch.addmm(leaves[2], leaves[0].reshape(-1, Hs), leaves[1].t())
            want = F.objective_loss_stock(scores, y.cpu(), lengths=lengths.cpu(), negatives=neg.cpu(), normalize=normalize, **KW)
            ((up or 1.0) * want[0]).backward()
            parts = np.array([v.item() for v in want[1:]])
            C.assert_losses([v.item() for v in got], dict(loss=want[0].item(), parts=parts), f"{normalize}, upstream {up}")
            for name, a, c in zip("hwb", (h, w, b), leaves):
                assert_grad(a.grad.cpu().numpy(), c.grad.numpy(), f"d{name}, {normalize}, upstream {up}")


def model_case(layers):
    torch.manual_seed(7 + layers)
    V, Hm = 64, 32
    model = Model(V, Hm, layers, 0.0, 0.1, w_rank=4, u_ranks=[4], lstm_type="vmlmf").to(DEV)
    x, y = torch.randint(0, V, (6, 3), device=DEV), torch.randint(0, V, (6, 3), device=DEV)
    return model, x, y, torch.tensor([6, 4, 1], device=DEV)


def stock_model_loss(model, x, y, lengths, normalize="rows"):
    scores, _ = model(x, model.state_init(x.size(1)))
    return F.objective_loss_stock(scores, y, lengths=lengths, negatives=context_negatives(x), normalize=normalize, **KW)


@pytest.mark.parametrize("layers", [1, 2])
def test_model_loss_of_a_rank_4_model_against_the_stock_formula_on_its_own_scores(layers):
    model, x, y, lengths = model_case(layers)
    for normalize in ("rows", "tokens"):
        model.zero_grad()
        out, states = model.loss(x, y, model.state_init(3), lengths=lengths, normalize=normalize, return_parts=True, **KW)
        assert len(out) == 5 and len(states) == layers
        out[0].backward()
        got = {n: p.grad.clone() for n, p in model.named_parameters()}
        model.zero_grad()
        want = stock_model_loss(model, x, y, lengths, normalize)
        want[0].backward()
        C.assert_losses([v.item() for v in out], dict(loss=want[0].item(), parts=np.array([v.item() for v in want[1:]])), normalize)
        assert out[4].item() > 0
        for n, p in model.named_parameters():
            assert_grad(got[n].cpu().numpy(), p.grad.cpu().numpy(), n)
    plain, _ = model.loss(x, y, model.state_init(3))       # every keyword at its default: lm_head_loss, its bits
    h, _ = model.features(x, model.state_init(3))
    assert torch.equal(plain, F.lm_head_loss(h, model.fc.w, model.fc.b, y))


def test_three_clipped_sgd_steps_end_at_the_stock_op_loops_parameters():
    model, x, y, lengths = model_case(2)
    twin = Model(64, 32, 2, 0.0, 0.1, w_rank=4, u_ranks=[4], lstm_type="vmlmf").to(DEV)
    twin.load_state_dict(model.state_dict())
    for _ in range(3):
        for m, loss in ((model, lambda: model.loss(x, y, model.state_init(3), lengths=lengths, normalize="tokens", **KW)[0]),
                        (twin, lambda: stock_model_loss(twin, x, y, lengths, "tokens")[0])):
            m.zero_grad()
            loss().backward()
            optim.clip_sgd_step(list(m.parameters()), 1.0, 0.25)
    for (n, p), q in zip(model.named_parameters(), twin.parameters()):
        assert torch.allclose(p, q, atol=2e-5, rtol=1e-3), (n, (p - q).abs().max().item())


@pytest.mark.parametrize("normalize", ["rows", "tokens"])
def test_the_head_loss_captured_into_a_graph_replays_to_the_eager_bits(normalize):
    torch.manual_seed(5)
    Hs, Vs, Ts, Bs = 24, 64, 5, 6
    h, w, b = (t.requires_grad_(True) for t in (torch.randn(Ts, Bs, Hs, device=DEV), 0.3 * torch.randn(Vs, Hs, device=DEV), torch.randn(Vs, device=DEV)))
    y = torch.randint(0, Vs, (Ts, Bs), device=DEV)
    neg = torch.randint(-1, Vs, (Ts, Bs, 7), device=DEV)
    lengths = torch.tensor([5, 4, 3, 2, 1, 5], device=DEV)

    def step():
        for t in (h, w, b):
            t.grad = None
        out = F.lm_head_objective_loss(h, w, b, y, lengths=lengths, negatives=neg, normalize=normalize, return_parts=True, **KW)
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
    for name, a, c in zip(("loss", "nll", "smooth", "z", "ul", "dh", "dw", "db"), eager, captured):
        assert_same_bits(name, a, c, "between the eager call and the replay")
