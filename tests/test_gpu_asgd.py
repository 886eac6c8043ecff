"""GPU: NT-ASGD on the fused launches (vmlmf_asgd_step, csrc/vmlmf_optim.hip) against the fp64 oracle of tests/asgd_cases.py element by
element, against clip_sgd_step bit for bit, under a captured graph, and ASGD's loop on tiny models.  docs/design/lm_asgd.md has the
contract and the bound."""
import copy

import numpy as np
import pytest
import torch

import asgd_cases as C
import vmlmf_amd
from vmlmf_amd import Model, _lib, optim

pytestmark = pytest.mark.gpu
DEV = "cuda"
PATTERN = 0x7FC12345            # a NaN with a payload: any arithmetic on it, and any write of another value, shows


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


def state_words(k, t0):
    words = optim.new_asgd_state("cpu")
    words[_lib.ASGD_STEP], words[_lib.ASGD_T0] = k - 1, t0
    return words.to(DEV)


def patterned_ax(fx):
    """The flat ax buffer on the device: the case's values in the tensors' slices, PATTERN in the padding between them."""
    flat = np.full(fx["total"], PATTERN, np.int32).view(np.float32)
    covered = np.zeros(fx["total"], bool)
    for a, o in zip(fx["ax"], fx["offsets"]):
        flat[o:o + a.size] = a
        covered[o:o + a.size] = True
    return torch.from_numpy(flat.copy()).to(DEV), covered


def device_step(fx):
    params, grads = on_device(fx["p"], fx["misalign"], "param"), on_device(fx["g"], fx["misalign"], "grad")
    ax, covered = patterned_ax(fx)
    words = state_words(fx["k"], fx["t0"])
    norm = optim.asgd_step(params, grads, ax, words, fx["offsets"], lr=fx["lr"], weight_decay=fx["wd"], max_norm=fx["max_norm"])
    return params, grads, ax, covered, words, norm


# ---- 1. every layout, element by element ----
@pytest.mark.parametrize("variant", list(C.VARIANTS))
@pytest.mark.parametrize("layout", list(C.STEP_CASES))
def test_the_step_is_the_oracle_elementwise(layout, variant):
    """Parameters, gradients and ax within the doc's bounds of the fp64 rule: all n % 4, one and several workgroups, 16-byte accesses,
    the scalar loop under packed state offsets and under one-float-offset views, 1 and 48 tensors, a tensor beyond 2^20 elements;
    averaging off, n = 0, 1, 2 and large, the clip binding and not, with and without decay."""
    fx = C.asgd_fixture(layout, variant, seed=31)
    want = fx["want"]
    if not C.STEP_CASES[layout]["pad"] and len(fx["numels"]) > 1:
        assert any(o % 4 for o in fx["offsets"])
    params, grads, ax, covered, words, norm = device_step(fx)
    assert abs(float(norm) - want["norm"]) <= C.NORM_RTOL * want["norm"]
    flat = ax.cpu().numpy()
    got_a = [flat[o:o + n] for o, n in zip(fx["offsets"], fx["numels"])]
    worst = C.asgd_ratios([p.cpu().numpy() for p in params], [g.cpu().numpy() for g in grads], got_a, want)
    print(f"asgd step {layout} {variant}: worst error / bound  p {worst[0]:.3f}  g {worst[1]:.3f}  ax {worst[2]:.3f}")
    assert max(worst) <= 1.0, worst
    if want["c"] == 1.0:                                            # the gradients' bits as they were
        assert all(np.array_equal(g.cpu().numpy().view(np.uint32), g0.view(np.uint32)) for g, g0 in zip(grads, fx["g"]))
    assert (flat.view(np.int32)[~covered] == PATTERN).all()         # the padding between the slices is not written
    w = words.cpu().tolist()
    assert (w[_lib.ASGD_STEP], w[_lib.ASGD_T0], w[_lib.ASGD_GO]) == (fx["k"], fx["t0"], 1)
    assert w[_lib.ASGD_MODE] == {"off": _lib.ASGD_MODE_OFF, "copy": _lib.ASGD_MODE_COPY, "average": _lib.ASGD_MODE_AVERAGE}[want["mode"]]
    mu = words[_lib.ASGD_MU:_lib.ASGD_MU + 1].view(torch.float32).item()
    assert mu == float(np.float32(want["mu"]))                      # 1 / n rounded once to fp32: part of the contract


# ---- 2. the first phase is the LM loop users already run ----
@pytest.mark.parametrize("clip", [0.25, 4.0, 0.0])
@pytest.mark.parametrize("layout", ["misaligned_views", "count_48", "million"])
def test_without_decay_and_average_the_bits_are_clip_sgd_steps(layout, clip):
    case = C.STEP_CASES[layout]
    p, g, _ = C.asgd_case(case["numels"], seed=32, stale=True)
    max_norm = float(np.float32(clip * C.norm_of(g)))
    offsets, total = C.offsets_of(case["numels"], case["pad"])
    ours, ours_g = on_device(p, case["misalign"], "param"), on_device(g, case["misalign"], "grad")
    theirs = [torch.nn.Parameter(t) for t in on_device(p, case["misalign"], "param")]
    theirs_g = on_device(g, case["misalign"], "grad")
    for t, tg in zip(theirs, theirs_g):
        t.grad = tg
    ax = torch.full((total,), 3.0, device=DEV)
    norm = optim.asgd_step(ours, ours_g, ax, state_words(1, C.T0_OFF), offsets, lr=C.LR, weight_decay=0.0, max_norm=max_norm)
    ref = optim.clip_sgd_step(theirs, C.LR, max_norm)
    assert torch.equal(bits(norm), bits(ref)) and (clip == 0.25) == (0 < max_norm < float(ref))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(ours, theirs))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(ours_g, theirs_g))
    assert (clip == 0.25) == (not torch.equal(ours_g[-1].cpu(), torch.from_numpy(g[-1])))    # written when the clip binds, only then
    assert not torch.equal(ours[-1].cpu(), torch.from_numpy(p[-1])) and bool(ax.eq(3.0).all())


# ---- 3. what ax is at the edges ----
@pytest.mark.parametrize("layout", ["padded", "packed_offsets", "misaligned_views"])
def test_the_first_two_averaged_steps_copy_and_averaging_off_writes_nothing(layout):
    for variant in ("n0_clip", "n1_loose_decay"):
        fx = C.asgd_fixture(layout, variant, seed=33)
        params, _, ax, covered, _, _ = device_step(fx)
        flat = bits(ax).numpy()
        for p, o in zip(params, fx["offsets"]):
            assert np.array_equal(flat[o:o + p.numel()], bits(p).numpy())                     # p's bits, not p's value
        assert (flat[~covered] == PATTERN).all()
    for variant in ("off_first_step", "off_clip_decay"):
        fx = C.asgd_fixture(layout, variant, seed=34)
        fx["ax"] = [np.full(a.size, PATTERN, np.int32).view(np.float32) for a in fx["ax"]]  # a NaN: a load-and-store would keep it,
        params, _, ax, _, _, _ = device_step(fx)                                              # arithmetic or a copy of p would not
        assert (bits(ax).numpy() == PATTERN).all()
        assert all(np.isfinite(p.cpu().numpy()).all() for p in params)


# ---- 4. a norm that is not finite ----
def test_a_nan_gradient_skips_the_step_and_the_next_one_lands_on_its_n():
    torch.manual_seed(1)
    params = [torch.nn.Parameter(0.1 * torch.randn(n, device=DEV)) for n in (5, 2 ** 20 + 3, 1025)]
    opt = optim.ASGD(params, lr=C.LR, weight_decay=C.WD, max_norm=0.25)

    def give(bad=False):
        gen = torch.Generator(device=DEV).manual_seed(7)
        for p in params:
            p.grad = 1e-2 * torch.randn(p.shape, device=DEV, generator=gen)
        if bad:
            params[1].grad[2 ** 20 + 1] = float("nan")
    for _ in range(3):
        give()
        opt.step()
    opt.start_averaging()                                           # t0 = 3
    for _ in range(3):                                              # n = 0, 1, 2
        give()
        opt.step()
    twin_params = [p.detach().clone() for p in params]
    twin_ax, twin_words = opt.ax.clone(), opt._words.clone()
    give(bad=True)
    before = [bits(t) for t in params] + [bits(p.grad) for p in params] + [bits(opt.ax), bits(opt._words[:_lib.ASGD_GO])]
    versions = [p._version for p in params]
    opt.step()
    assert not np.isfinite(float(opt.last_norm))
    after = [bits(t) for t in params] + [bits(p.grad) for p in params] + [bits(opt.ax), bits(opt._words[:_lib.ASGD_GO])]
    assert all(torch.equal(a, b) for a, b in zip(after, before))
    assert int(opt._words[_lib.ASGD_GO]) == 0 and int(opt._words[_lib.ASGD_STEP]) == 6
    assert all(p._version > v for p, v in zip(params, versions))
    give()
    twin_grads = [p.grad.detach().clone() for p in params]
    opt.step()                                                      # as if the skipped one had never been asked for: n = 3
    optim.asgd_step(twin_params, twin_grads, twin_ax, twin_words, opt._offsets, lr=C.LR, weight_decay=C.WD, max_norm=0.25)
    assert np.isfinite(float(opt.last_norm)) and int(opt._words[_lib.ASGD_STEP]) == 7
    assert opt._words[_lib.ASGD_MU:_lib.ASGD_MU + 1].view(torch.float32).item() == float(np.float32(1.0 / 3.0))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(params, twin_params)) and torch.equal(bits(opt.ax), bits(twin_ax))
    assert all(torch.equal(bits(a), bits(p.grad)) for a, p in zip(twin_grads, params))
    assert not torch.equal(bits(params[0]), before[0])


# ---- 5. one capture, start_averaging() between replays ----
def test_a_captured_step_goes_on_working_across_start_averaging():
    case = C.STEP_CASES["misaligned_views"]
    p, g, _ = C.asgd_case(case["numels"], seed=35, stale=True)

    def build():
        params = [torch.nn.Parameter(t) for t in on_device(p, case["misalign"], "param")]
        fresh = on_device(g, case["misalign"], "grad")
        for t, tg in zip(params, fresh):
            t.grad = tg
        return params, fresh, optim.ASGD(params, lr=C.LR, weight_decay=C.WD, max_norm=0.25 * C.norm_of(g))

    def rewind(params, grads):                                      # the step scales the gradients in place: each step gets g again
        for t, a in zip(grads, g):
            t.copy_(torch.from_numpy(a))

    eager_p, eager_g, eager = build()
    for k in range(4):
        if k == 2:
            eager.start_averaging()
        rewind(eager_p, eager_g)
        eager.step()
    graph_p, graph_g, graphed = build()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.step()
    with torch.no_grad():                                           # whatever the capture did or did not run: start from the start
        for t, a in zip(graph_p, p):
            t.copy_(torch.from_numpy(a))
        graphed._words.copy_(optim.new_asgd_state(DEV))
    for k in range(4):
        if k == 2:
            graphed.start_averaging()
        rewind(graph_p, graph_g)
        graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(eager_p, graph_p))
    assert torch.equal(bits(eager.ax), bits(graphed.ax)) and torch.equal(bits(eager._words), bits(graphed._words))
    assert torch.equal(bits(eager.last_norm), bits(graphed.last_norm))
    assert eager._words.cpu().tolist()[:2] == [4, 2] and int(eager._words[_lib.ASGD_MODE]) == _lib.ASGD_MODE_COPY
    assert not torch.equal(bits(eager.ax_views()[-1]), bits(torch.from_numpy(p[-1])))


# ---- 6. a two-layer Model ----
V, H, B, T = 64, 8, 2, 5


def text(seed, rows, width=B):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, V, (rows, width), generator=g).to(DEV)


def test_six_minibatches_of_a_two_layer_model_and_the_averaged_score():
    """test_asgd_cpu.py's loop on the device: before each step a copy takes the parameters, ax and counters and then the stock
    step; the fused step and the stock step both lie within the element-wise bound of the fp64 rule applied to the state in front
    of the step.  Then the exchange: score inside averaged() is score of a copy loaded with ax, to the bit; outside, the plain
    model's - the kept packed images followed both ways."""
    torch.manual_seed(0)
    model = Model(V, H, 2, 0.0, 0.1, w_rank=4, u_ranks=[4], lstm_type="vmlmf").to(DEV)
    vmlmf_amd.cache_packed_parameters(model)
    params = list(model.parameters())
    opt = optim.ASGD(params, lr=C.LR, weight_decay=C.WD, max_norm=0.25, nonmono=5)
    carried = model.state_init(B)
    modes = []
    for k in range(1, 7):
        x, y = text(40 + k, T), text(60 + k, T)
        opt.zero_grad(set_to_none=True)
        loss, carried = model.loss(x, y, model.detach(carried))
        loss.backward()
        live = [i for i, p in enumerate(params) if p.grad is not None]
        assert len(live) == len(params)
        twin_p = [params[i].detach().clone() for i in live]
        twin_g = [params[i].grad.detach().clone() for i in live]
        twin_ax, twin_words = opt.ax.clone(), opt._words.clone()
        before_a = [a.cpu().numpy().copy() for a in opt.ax_views()]
        words = opt._words.cpu().tolist()
        assert words[_lib.ASGD_STEP] == k - 1
        want = C.asgd_oracle([t.cpu().numpy() for t in twin_p], [t.cpu().numpy() for t in twin_g], before_a, k=k,
                             t0=words[_lib.ASGD_T0], lr=C.LR, wd=C.WD, max_norm=0.25)
        modes.append((want["mode"], want["c"] < 1))
        opt.step()
        optim.asgd_step_stock(twin_p, twin_g, twin_ax, twin_words, opt._offsets, lr=C.LR, weight_decay=C.WD, max_norm=0.25)
        assert abs(float(opt.last_norm) - want["norm"]) <= C.NORM_RTOL * want["norm"]
        for label, got in (("fused", ([p.detach() for p in params], [p.grad for p in params], opt.ax_views())),
                           ("stock", (twin_p, twin_g, [twin_ax[o:o + t.numel()] for o, t in zip(opt._offsets, twin_p)]))):
            worst = C.asgd_ratios(*([t.cpu().numpy() for t in seq] for seq in got), want)
            print(f"asgd model step {k} {label}: worst error / bound  p {worst[0]:.3f}  g {worst[1]:.3f}  ax {worst[2]:.3f}")
            assert max(worst) <= 1.0, (k, label, worst)
        assert torch.equal(twin_words[:2].cpu(), opt._words[:2].cpu()) and int(opt._words[_lib.ASGD_MODE]) == int(twin_words[_lib.ASGD_MODE])
        if k == 2:
            opt.start_averaging()
    assert [m for m, _ in modes] == ["off", "off", "copy", "copy", "average", "average"]
    tokens = text(9, 12)
    model.eval()
    plain = model.score(tokens)                                     # the images of the plain parameters are kept now
    loaded = copy.deepcopy(model)
    with torch.no_grad():
        for q, a in zip(loaded.parameters(), opt.ax_views()):
            q.copy_(a)
    want_avg = loaded.score(tokens)
    own = [bits(p) for p in params]
    with opt.averaged():
        got_avg = model.score(tokens)
    assert torch.equal(bits(got_avg[0]), bits(want_avg[0])) and not torch.equal(bits(got_avg[0]), bits(plain[0]))
    again = model.score(tokens)
    assert torch.equal(bits(again[0]), bits(plain[0]))
    assert all(torch.equal(bits(p), o) for p, o in zip(params, own))
