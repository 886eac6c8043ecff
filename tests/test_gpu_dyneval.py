"""GPU: dynamic evaluation on the fused launches (vmlmf_dyneval_step / vmlmf_dyneval_accumulate, csrc/vmlmf_optim.hip) against the fp64
oracle of tests/dyneval_cases.py, and DynamicEval's loop on tiny models.  docs/design/lm_dyneval.md has the contract and the bound."""
import copy

import numpy as np
import pytest
import torch

import dyneval_cases as C
import vmlmf_amd
from vmlmf_amd import DynamicEval, Model

pytestmark = pytest.mark.gpu
DEV = "cuda"
HYPER = dict(lr=C.LR, decay=C.DECAY, eps=C.EPS)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def on_device(arrays, misalign, which):
    """One device tensor per array; the ones `misalign` names for `which` are one-float-offset views of a larger allocation."""
    out = []
    for i, a in enumerate(arrays):
        if misalign.get(i) == which:
            buf = torch.zeros(a.size + 5, device=DEV)
            t = buf[1:1 + a.size]
            t.copy_(torch.from_numpy(a))
            assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        else:
            t = torch.from_numpy(a).to(DEV)
            assert t.data_ptr() % 16 == 0
        out.append(t)
    return out


def device_case(name, seed):
    case = C.STEP_CASES[name]
    numels = case["numels"]
    theta, theta0, r, g = C.step_case(numels, seed)
    offsets, total = C.offsets_of(numels, case["pad"])
    if not case["pad"] and len(numels) > 1:
        assert any(o % 4 for o in offsets)
    flat0 = torch.from_numpy(C.flat_state(theta0, offsets, total)).to(DEV)
    flatr = torch.from_numpy(C.flat_state(r, offsets, total)).to(DEV)
    return (theta, theta0, r, g), offsets, total, flat0, flatr, case["misalign"]


@pytest.mark.parametrize("name", list(C.STEP_CASES))
def test_the_step_is_the_oracle_elementwise(name):
    """Every element within K_ROUNDINGS * 2^-24 * (|theta| + |ld (theta0 - theta)| + |lr c g / (r + eps)|) of the fp64 rule: all n % 4,
    one and several workgroups, 16-byte accesses, the scalar loop under packed state offsets and under one-float-offset views,
    1 and 48 tensors, a tensor beyond 2^20 elements.  The clamp decay r / m > 1 binds on part of the elements."""
    (theta, theta0, r, g), offsets, _, flat0, flatr, mis = device_case(name, seed=11)
    m = C.mean_rms(r)
    want, norm, scale, clamped = C.step_oracle(theta, theta0, r, g, lr=C.LR, decay=C.DECAY, m=m, eps=C.EPS, max_norm=0.0)
    bound = np.concatenate(clamped)
    assert bound.any() and not bound.all()
    params, grads = on_device(theta, mis, "param"), on_device(g, mis, "grad")
    versions = [p._version for p in params]
    got = vmlmf_amd.dyneval_step(params, grads, flat0, flatr, offsets, inv_mean_rms=1.0 / m, max_norm=0.0, **HYPER)
    assert abs(float(got) - norm) <= C.NORM_RTOL * norm
    assert all(p._version > v for p, v in zip(params, versions))
    worst = 0.0
    for p, w, s, g0, gt in zip(params, want, scale, g, grads):
        err = np.abs(p.cpu().numpy().astype(np.float64) - w)
        worst = max(worst, float((err / (C.U * s)).max()))
        assert (err <= C.K_ROUNDINGS * C.U * s).all()
        assert np.array_equal(gt.cpu().numpy().view(np.uint32), g0.view(np.uint32))
    print(f"dyneval step {name}: worst error {worst:.2f} x 2^-24 x magnitude (bound {C.K_ROUNDINGS})")


@pytest.mark.parametrize("name", ["padded", "misaligned_views", "million"])
def test_norm_and_clip(name):
    """max_norm above the norm, below it, and 0: the norm against fp64 at clip_sgd_step's tolerance, the parameters against the oracle
    under the same bound plus what that tolerance of the norm is worth through c, the gradients' bits as they were."""
    (theta, theta0, r, g), offsets, _, flat0, flatr, mis = device_case(name, seed=12)
    m = C.mean_rms(r)
    grads = on_device(g, mis, "grad")
    before = [bits(t) for t in grads]
    clipped = []
    for factor in (4.0, 0.25, 0.0):
        _, norm, _, _ = C.step_oracle(theta, theta0, r, g, lr=C.LR, decay=C.DECAY, m=m, eps=C.EPS, max_norm=0.0)
        max_norm = factor * norm
        want, _, scale, _ = C.step_oracle(theta, theta0, r, g, lr=C.LR, decay=C.DECAY, m=m, eps=C.EPS, max_norm=max_norm)
        upd = C.update_term(r, g, lr=C.LR, eps=C.EPS, max_norm=max_norm, norm=norm)
        params = on_device(theta, mis, "param")
        got = vmlmf_amd.dyneval_step(params, grads, flat0, flatr, offsets, inv_mean_rms=1.0 / m, max_norm=max_norm, **HYPER)
        assert abs(float(got) - norm) <= C.NORM_RTOL * norm
        for p, w, s, u in zip(params, want, scale, upd):
            assert (np.abs(p.cpu().numpy().astype(np.float64) - w) <= C.K_ROUNDINGS * C.U * s + C.NORM_RTOL * u).all()
        assert all(torch.equal(bits(t), b) for t, b in zip(grads, before))
        clipped.append(params[-1].cpu())
    assert torch.equal(clipped[0], clipped[2]) and not torch.equal(clipped[0], clipped[1])    # above the norm: c = 1, as without


def test_a_norm_that_is_not_finite_skips_the_step():
    (theta, theta0, r, g), offsets, _, flat0, flatr, _ = device_case("million", seed=13)
    m = C.mean_rms(r)
    bad = [a.copy() for a in g]
    bad[1][2 ** 20 + 1] = np.nan
    params = on_device(theta, {}, "param")
    before = [bits(p) for p in params]
    kw = dict(inv_mean_rms=1.0 / m, max_norm=0.25, **HYPER)
    norm = vmlmf_amd.dyneval_step(params, on_device(bad, {}, "grad"), flat0, flatr, offsets, **kw)
    assert not np.isfinite(float(norm))
    assert all(torch.equal(bits(p), b) for p, b in zip(params, before))
    norm = vmlmf_amd.dyneval_step(params, on_device(g, {}, "grad"), flat0, flatr, offsets, **kw)
    want, ref, scale, _ = C.step_oracle(theta, theta0, r, g, lr=C.LR, decay=C.DECAY, m=m, eps=C.EPS, max_norm=0.25)
    upd = C.update_term(r, g, lr=C.LR, eps=C.EPS, max_norm=0.25, norm=ref)
    assert abs(float(norm) - ref) <= C.NORM_RTOL * ref
    for p, w, s, u in zip(params, want, scale, upd):
        assert (np.abs(p.cpu().numpy().astype(np.float64) - w) <= C.K_ROUNDINGS * C.U * s + C.NORM_RTOL * u).all()


@pytest.mark.parametrize("name", list(C.STEP_CASES))
def test_accumulate_is_the_oracle(name):
    """Three calls: every element of ms within (3 + 1) * 2^-24 relative of fp64 (one fused multiply-add per call)."""
    case = C.STEP_CASES[name]
    numels = case["numels"]
    offsets, total = C.offsets_of(numels, case["pad"])
    ms = torch.zeros(total, device=DEV)
    want = [np.zeros(n) for n in numels]
    for k in range(3):
        _, _, _, g = C.step_case(numels, seed=40 + k)
        grads = on_device(g, case["misalign"], "grad")
        before = [bits(t) for t in grads]
        vmlmf_amd.dyneval_accumulate(grads, ms, offsets)
        assert all(torch.equal(bits(t), b) for t, b in zip(grads, before))
        want = C.accumulate_oracle(want, g)
    got = ms.cpu().numpy()
    covered = np.zeros(total, bool)
    for o, w in zip(offsets, want):
        assert (np.abs(got[o:o + w.size].astype(np.float64) - w) <= (3 + 1) * C.U * w).all()
        covered[o:o + w.size] = True
    assert not got[~covered].any()                                  # the padding between the tensors is not written


def test_the_three_launches_capture_and_replay():
    """step()'s launches in one torch.cuda.graph - one stream, a straight line - replayed twice: two eager steps, to the bit."""
    (theta, theta0, r, g), offsets, _, flat0, flatr, mis = device_case("misaligned_views", seed=14)
    kw = dict(inv_mean_rms=1.0 / C.mean_rms(r), max_norm=0.25, **HYPER)
    grads = on_device(g, mis, "grad")
    eager, graphed = on_device(theta, mis, "param"), on_device(theta, mis, "param")
    norms = [vmlmf_amd.dyneval_step(eager, grads, flat0, flatr, offsets, **kw) for _ in range(2)]
    norm = torch.zeros((), device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        vmlmf_amd.dyneval_step(graphed, grads, flat0, flatr, offsets, norm=norm, **kw)
    for p, a in zip(graphed, theta):                                # whatever the capture did or did not run: start from theta
        p.copy_(torch.from_numpy(a))
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(eager, graphed))
    assert torch.equal(bits(norm), bits(norms[1])) and not torch.equal(eager[-1].cpu(), torch.from_numpy(theta[-1]))


# ---- the loop on tiny models ----
V, H, B = 64, 8, 2


def tiny_model(seed=0):
    torch.manual_seed(seed)
    return Model(V, H, 1, 0.0, 0.1, w_rank=4, u_ranks=[4], lstm_type="vmlmf").to(DEV)


def text(seed, T, width=B):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, V, (T, width), generator=g).to(DEV)


def with_statistics(model, stock=False, **hyper):
    de = DynamicEval(model, **{**HYPER, **hyper})
    de.stock = stock
    states = None
    for k in range(3):
        states = de.accumulate(text(10 + k, 6, 3), text(20 + k, 6, 3), states)
    de.finalize()
    return de


TOKENS = 22            # 21 positions: segments of 5, 5, 5, 5 and 1


def test_without_a_step_score_is_model_loss_segment_by_segment():
    """lr = decay = 0: the parameters keep their bits, and -logprobs of a segment, summed in the finish launch's order and scaled as
    Model.loss scales, is Model.loss on that segment to the bit: the rows ARE the loss launch's."""
    model = tiny_model()
    before = [bits(p) for p in model.parameters()]
    de = DynamicEval(model, lr=0.0, decay=0.0)
    de.load_state_dict(with_statistics(model).state_dict())
    tokens = text(1, TOKENS)
    logprobs, states = de.score(tokens)
    assert logprobs.shape == (TOKENS - 1, B) and logprobs.dtype == torch.float32
    assert all(torch.equal(bits(p), b) for p, b in zip(model.parameters(), before))
    assert all(p.grad is None for p in model.parameters())
    x, y = tokens[:-1], tokens[1:]
    carried = model.state_init(B)
    model.eval()
    for lo in range(0, TOKENS - 1, 5):
        hi = min(lo + 5, TOKENS - 1)
        loss, carried = model.loss(x[lo:hi], y[lo:hi].contiguous(), model.detach(carried))     # (under autograd, as score() runs it)
        scale = torch.tensor(float(B) / float((hi - lo) * B), dtype=torch.float32)
        assert torch.equal(bits(scale * C.butterfly_sum(-logprobs[lo:hi])), bits(loss))
    for (h, c), (h2, c2) in zip(states, carried):
        assert torch.equal(h, h2) and torch.equal(c, c2)


def test_scores_come_before_the_adaptation_they_cause_and_calls_compose():
    model = tiny_model()
    de = with_statistics(model, max_norm=0.25)
    theta0 = [bits(p) for p in model.parameters()]
    static = DynamicEval(model, lr=0.0, decay=0.0)
    static.load_state_dict(de.state_dict())
    tokens = text(1, TOKENS)
    plain, _ = static.score(tokens)
    whole, end = de.score(tokens)
    adapted = [p.detach().clone() for p in model.parameters()]
    assert torch.equal(bits(whole[:5]), bits(plain[:5]))            # the first segment: the trained model's predictions
    assert all(not torch.equal(whole[lo:lo + 5], plain[lo:lo + 5]) for lo in (5, 10, 15)) and not torch.equal(whole[20:], plain[20:])
    assert all(not torch.equal(bits(p), b) for p, b in zip(model.parameters(), theta0))
    de.restore()
    assert all(torch.equal(bits(p), b) for p, b in zip(model.parameters(), theta0))
    first, mid = de.score(tokens[:11])
    second, end2 = de.score(tokens[10:], states=mid)
    assert torch.equal(bits(torch.cat([first, second])), bits(whole))
    assert all(torch.equal(bits(p), bits(q)) for p, q in zip(model.parameters(), adapted))
    assert all(torch.equal(a, b) for s, s2 in zip(end, end2) for a, b in zip(s, s2))
    with de:
        pass
    assert all(torch.equal(bits(p), b) for p, b in zip(model.parameters(), theta0))


def test_kept_parameter_images_follow_the_adaptation():
    model = tiny_model()
    vmlmf_amd.cache_packed_parameters(model)
    tokens = text(1, TOKENS)
    model.score(tokens)                                             # the images of theta0 are kept now
    de = with_statistics(model)
    de.score(tokens)
    fresh = tiny_model(seed=5)
    fresh.load_state_dict(model.state_dict())
    got, want = model.score(tokens), fresh.score(tokens)
    assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(got[1], want[1])


def stock_and_fused(build, tokens, **hyper):
    """DynamicEval.score on two copies of one model: the fused launches and the same loop in stock ops on the device.  Returns
    ((logprobs, parameters) fused, (logprobs, parameters) stock, the stock evaluation)."""
    model = build()
    twin = copy.deepcopy(model)
    fused, stock = with_statistics(model, **hyper), with_statistics(twin, stock=True, **hyper)
    a, _ = fused.score(tokens)
    b, _ = stock.score(tokens)
    return (a, list(model.parameters())), (b, list(twin.parameters())), stock


@pytest.fixture(scope="module")
def stock_deviation():
    """What the stock fp32 loop on the device is away from the fp64 loop (the oracle's literal VMLMF language model under
    loop_oracle) on test 6's model and text: (logprobs, parameters), max abs.  The measure of the loop's fp32 rounding that the
    fused path is held to four times of - measured here, never taken from the code under test."""
    model = tiny_model()
    names = [n for n, _ in model.named_parameters()]
    params64 = [p.detach().cpu().double().requires_grad_(True) for p in model.parameters()]
    stock = with_statistics(model, stock=True, max_norm=0.25)
    tokens = text(1, TOKENS)
    r = [a.cpu().numpy() for a in stock._views(stock.rms)]
    raw = np.concatenate([(C.DECAY * a.astype(np.float64) / stock.mean_rms).ravel() for a in r])
    assert (raw > 1).any() and (raw < 1).any()
    cpu = tokens.cpu()
    states = [(torch.zeros(B, H, dtype=torch.float64), torch.zeros(B, H, dtype=torch.float64))]
    want, _ = C.loop_oracle(C.literal_forward(names, 1), params64, r, stock.mean_rms, cpu[:-1], cpu[1:], states, segment=5, lr=C.LR,
                            decay=C.DECAY, eps=C.EPS, max_norm=0.25)
    got, _ = stock.score(tokens)
    dlog = float(np.abs(got.cpu().numpy() - want).max())
    dpar = max(float((p.detach().cpu().double() - q.detach()).abs().max()) for p, q in zip(model.parameters(), params64))
    print(f"dyneval stock fp32 loop against the fp64 loop: logprobs {dlog:.3e}, parameters {dpar:.3e}")
    assert 0 < dlog < 1e-4 and 0 < dpar < 1e-5                     # a loop that follows the oracle at all (the CPU test's bounds, x 10)
    return dlog, dpar


def assert_loops_agree(fused, stock, deviation):
    dlog, dpar = deviation
    elog = float((fused[0] - stock[0]).abs().max())
    epar = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(fused[1], stock[1]))
    print(f"dyneval fused against stock loop: logprobs {elog:.3e} (allowed {4 * dlog:.3e}), parameters {epar:.3e} (allowed {4 * dpar:.3e})")
    assert elog <= 4 * dlog and epar <= 4 * dpar


def test_the_fused_loop_is_the_stock_loop(stock_deviation):
    """Same model, same text, lr and decay on, clipping on: the fused path within four times the stock fp32 loop's own deviation from
    the fp64 loop (its operation order differs, and FMA contraction is legitimate)."""
    fused, stock, _ = stock_and_fused(tiny_model, text(1, TOKENS), max_norm=0.25)
    assert_loops_agree(fused, stock, stock_deviation)


def group_model():
    torch.manual_seed(2)
    return Model.with_group_layers(V, 32, 1, 0.0, 0.1, w_rank=4, u_ranks=[4, 4]).to(DEV)


def wide_model():
    torch.manual_seed(3)
    return Model(V, 64, 1, 0.0, 0.1, w_rank=40, u_ranks=[40], lstm_type="vmlmf").to(DEV)


@pytest.mark.parametrize("build", [group_model, wide_model])
def test_every_layer_familys_gradients_reach_the_step(build, stock_deviation):
    """MyVMLSTMGroup layers and a rank beyond 32 (the step-wise path): accumulate -> finalize -> score over two segments against the
    stock loop, and every parameter has moved."""
    tokens = text(4, 11)
    fused, stock, de = stock_and_fused(build, tokens, max_norm=0.25)
    assert_loops_agree(fused, stock, stock_deviation)
    assert all(not torch.equal(p.detach(), p0) for p, p0 in zip(stock[1], de._views(de.theta0)))
    assert all(float(r.max()) > 0 for r in de._views(de.rms))      # every tensor had a gradient in the statistics
