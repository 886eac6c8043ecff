"""CPU: NT-ASGD (vmlmf_amd.optim.ASGD; docs/design/lm_asgd.md) in its stock-op form against the fp64 oracle of tests/asgd_cases.py and
against clip_grad_norm_ + torch.optim.ASGD, the trigger, the exchange with the average, the state's round trip, the argument checks
and the C ABI's refusals.  The fused launches: test_gpu_asgd.py."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import asgd_cases as C
import vmlmf_amd
from vmlmf_amd import Model, _lib, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(t):
    return t.detach().clone().contiguous().view(torch.int32)          # (a copy: on the CPU a view would follow the tensor)


def state_words(k, t0):
    """The state block in front of applied step k."""
    words = optim.new_asgd_state("cpu")
    words[_lib.ASGD_STEP], words[_lib.ASGD_T0] = k - 1, t0
    return words


def assert_within(got_p, got_g, got_a, want, label):
    worst = C.asgd_ratios(got_p, got_g, got_a, want)
    print(f"asgd {label}: worst error / bound  p {worst[0]:.3f}  g {worst[1]:.3f}  ax {worst[2]:.3f}")
    assert max(worst) <= 1.0, (label, worst)
    return worst


# ---- 1. the rule ----
@pytest.mark.parametrize("variant", list(C.VARIANTS))
def test_the_stock_step_is_the_oracle(variant):
    fx = C.asgd_fixture("packed_offsets", variant, seed=3)
    params, grads = [torch.tensor(a) for a in fx["p"]], [torch.tensor(a) for a in fx["g"]]
    ax, words = torch.tensor(fx["ax_flat"]), state_words(fx["k"], fx["t0"])
    norm = optim.asgd_step_stock(params, grads, ax, words, fx["offsets"], lr=fx["lr"], weight_decay=fx["wd"], max_norm=fx["max_norm"])
    want = fx["want"]
    assert abs(float(norm) - want["norm"]) <= C.NORM_RTOL * want["norm"]
    got_a = [ax[o:o + n].numpy() for o, n in zip(fx["offsets"], fx["numels"])]
    assert_within([p.numpy() for p in params], [g.numpy() for g in grads], got_a, want, variant)
    w = words.tolist()
    assert (w[_lib.ASGD_STEP], w[_lib.ASGD_T0], w[_lib.ASGD_GO]) == (fx["k"], fx["t0"], 1)
    assert w[_lib.ASGD_MODE] == {"off": _lib.ASGD_MODE_OFF, "copy": _lib.ASGD_MODE_COPY, "average": _lib.ASGD_MODE_AVERAGE}[want["mode"]]
    mu, c = words[_lib.ASGD_MU:_lib.ASGD_MU + 1].view(torch.float32).item(), words[_lib.ASGD_COEF:_lib.ASGD_COEF + 1].view(torch.float32).item()
    assert mu == float(np.float32(want["mu"])) and abs(c - want["c"]) <= (2 * C.U + C.NORM_RTOL) * want["c"]
    if want["mode"] == "copy":
        assert all(np.array_equal(a.view(np.uint32), p.numpy().view(np.uint32)) for a, p in zip(got_a, params))


@pytest.mark.parametrize("fused", [False, True])
def test_the_bound_is_not_vacuous(fused):
    """The kernel's operation order in fp32 (numpy) holds the bound on every variant; each known-wrong variant breaks it somewhere."""
    broken = {m: False for m in C.MUTATIONS}
    for variant in C.VARIANTS:
        fx = C.asgd_fixture("packed_offsets", variant, seed=4)
        want = fx["want"]
        kw = dict(k=fx["k"], t0=fx["t0"], lr=fx["lr"], wd=fx["wd"], max_norm=fx["max_norm"], fused=fused)
        norm32 = np.float32(want["norm"])
        assert max(C.asgd_ratios(*C.asgd_emulate(fx["p"], fx["g"], fx["ax"], norm32, **kw), want)) <= 1.0, variant
        for m in C.MUTATIONS:
            if max(C.asgd_ratios(*C.asgd_emulate(fx["p"], fx["g"], fx["ax"], norm32, mutate=m, **kw), want)) > 1.0:
                broken[m] = True
    assert all(broken.values()), broken


K0, STEPS, MAX_NORM = 3, 9, 0.05
NUMELS = [5, 1025, 3, 64]


def nine_gradients():
    """Gradients of nine steps whose norms lie on both sides of MAX_NORM (the fixture vouches for it)."""
    rng = np.random.Generator(np.random.PCG64(21))
    out = []
    for k in range(STEPS):
        scale = 1e-2 if k % 2 else 5e-4
        out.append([(scale * rng.standard_normal(n)).astype(np.float32) for n in NUMELS])
    norms = [C.norm_of(g) for g in out]
    assert any(v > 2 * MAX_NORM for v in norms) and any(v < MAX_NORM / 2 for v in norms)
    return out


@pytest.mark.parametrize("wd", [0.0, C.WD])
def test_nine_steps_of_the_stock_step_and_of_torchs_pair_are_the_oracles(wd):
    """asgd_step_stock, and clip_grad_norm_ + torch.optim.ASGD(lambd=0, t0=K0, weight_decay=wd), step by step from their own fp32
    state: every element within the doc's bound of the fp64 rule.  Averaging starts behind step K0: n = 0, 1, 2 ... 5.  (torch
    copies the parameters into ax from its first step on; where the rule has averaging off its ax is not compared.)"""
    p0, _, _ = C.asgd_case(NUMELS, seed=20, stale=False)
    offsets, total = C.offsets_of(NUMELS, True)
    grads9 = nine_gradients()
    # the package's stock step
    params = [torch.tensor(a) for a in p0]
    ax, words = torch.full((total,), 7.0), optim.new_asgd_state("cpu")
    # torch's pair
    tparams = [torch.nn.Parameter(torch.tensor(a)) for a in p0]
    topt = torch.optim.ASGD(tparams, lr=C.LR, lambd=0.0, t0=K0, weight_decay=wd)
    seen = set()
    for k in range(1, STEPS + 1):
        g = grads9[k - 1]
        t0 = K0 if k > K0 else C.T0_OFF
        if k == K0 + 1:
            words[_lib.ASGD_T0] = words[_lib.ASGD_STEP]            # what start_averaging() does
        before_a = [ax[o:o + n].numpy().copy() for o, n in zip(offsets, NUMELS)]
        want = C.asgd_oracle([p.numpy() for p in params], g, before_a, k=k, t0=t0, lr=C.LR, wd=wd, max_norm=MAX_NORM)
        seen.add((want["mode"], want["c"] < 1))
        grads = [torch.tensor(a) for a in g]
        optim.asgd_step_stock(params, grads, ax, words, offsets, lr=C.LR, weight_decay=wd, max_norm=MAX_NORM)
        assert_within([p.numpy() for p in params], [t.numpy() for t in grads],
                      [ax[o:o + n].numpy() for o, n in zip(offsets, NUMELS)], want, f"stock step {k}")
        assert int(words[_lib.ASGD_STEP]) == k
        # torch, from ITS state
        tbefore_a = [topt.state[p]["ax"].detach().numpy().copy() if p in topt.state and "ax" in topt.state[p] else np.zeros(n, np.float32)
                     for p, n in zip(tparams, NUMELS)]
        twant = C.asgd_oracle([p.detach().numpy() for p in tparams], g, tbefore_a, k=k, t0=t0, lr=C.LR, wd=wd, max_norm=MAX_NORM)
        for p, a in zip(tparams, g):
            p.grad = torch.tensor(a)
        torch.nn.utils.clip_grad_norm_(tparams, MAX_NORM)
        topt.step()
        got_a = [topt.state[p]["ax"].detach().numpy() for p in tparams]
        if twant["mode"] == "off":
            got_a = twant["ax"]
        assert_within([p.detach().numpy() for p in tparams], [p.grad.numpy() for p in tparams], got_a, twant, f"torch step {k}")
    assert seen >= {("off", True), ("off", False), ("copy", True), ("copy", False), ("average", True), ("average", False)}
    assert offsets[1] == 8 and bool(ax[5:8].eq(7.0).all())   # the padding behind the five-element tensor is not written


def test_a_norm_that_is_not_finite_skips_the_stock_step():
    p, g, ax = C.asgd_case(NUMELS, seed=22, stale=False)
    offsets, total = C.offsets_of(NUMELS, True)
    g[1][17] = np.nan
    params, grads = [torch.tensor(a) for a in p], [torch.tensor(a) for a in g]
    flat, words = torch.tensor(C.flat_state(ax, offsets, total)), state_words(6, 3)
    before = [bits(t) for t in params + grads + [flat]]
    norm = optim.asgd_step_stock(params, grads, flat, words, offsets, lr=C.LR, weight_decay=C.WD, max_norm=MAX_NORM)
    assert not np.isfinite(float(norm))
    assert all(torch.equal(bits(t), b) for t, b in zip(params + grads + [flat], before))
    assert (int(words[_lib.ASGD_STEP]), int(words[_lib.ASGD_T0]), int(words[_lib.ASGD_GO])) == (5, 3, 0)


# ---- 2. the trigger ----
TRIGGER = [
    # nonmono, metrics, the index of the observe() call that switches averaging on (None: never)
    (5, [10, 9, 8, 7, 6, 5, 4, 3, 2, 1], None),                   # always improving
    (5, [5, 6, 7, 8, 9, 10], None),                               # len(history) > nonmono first holds at the seventh call
    (5, [5, 6, 7, 8, 9, 10, 11], 6),
    (5, [5, 4, 3, 2, 1, 0, 6], 6),                                # worse than the best of history[:-5] = [5]
    (5, [5, 4, 3, 2, 1, 0, 5, 4.5], 7),                           # equal is not worse; then worse than min([5, 4])
    (5, [9, 1, 8, 8, 8, 8, 8, 8, 0.5], 7),                        # min(history[:-5]) = 1 once the 1 has left the last five
    (1, [3, 2, 1], None),
    (1, [3, 4], None),                                            # len(history) = 1 is not > 1
    (1, [3, 2, 2.5], None),                                       # min(history[:-1]) = min([3]) is not below 2.5
    (1, [3, 2, 1, 2.5], 3),
]


def awd_lstm_trigger(nonmono, metrics):
    """The reference loop's own lines: `if 't0' not in ... and len(best_val_loss) > nonmono and val_loss > min(best_val_loss[:-nonmono])`."""
    history, started = [], None
    for i, m in enumerate(metrics):
        if started is None and len(history) > nonmono and m > min(history[:-nonmono]):
            started = i
        history.append(m)
    return started


@pytest.mark.parametrize("row", range(len(TRIGGER)))
def test_the_non_monotone_trigger(row):
    nonmono, metrics, _ = TRIGGER[row]
    want = TRIGGER[row][2]
    opt = optim.ASGD([torch.nn.Parameter(torch.ones(3))], lr=C.LR, nonmono=nonmono)
    started = None
    for i, m in enumerate(metrics):
        on = opt.observe(m)
        assert on == opt.averaging
        if on and started is None:
            started = i
    assert started == want and opt.history == [float(m) for m in metrics]


def test_the_trigger_table_is_what_it_says():
    """The table's third column, written by hand, against the reference loop's lines."""
    for nonmono, metrics, at in TRIGGER:
        assert awd_lstm_trigger(nonmono, metrics) == at, (nonmono, metrics)
    assert {awd_lstm_trigger(n, m) is None for n, m, _ in TRIGGER} == {True, False}


# ---- a tiny optimizer on the CPU ----
def stepped(wd=C.WD, steps=6, start_after=2, seed=5):
    torch.manual_seed(seed)
    params = [torch.nn.Parameter(0.1 * torch.randn(n)) for n in (5, 12, 3)]
    opt = optim.ASGD(params, lr=C.LR, weight_decay=wd, max_norm=MAX_NORM, nonmono=2)
    for k in range(steps):
        for p in params:
            p.grad = 1e-2 * torch.randn_like(p)
        opt.step()
        if k + 1 == start_after:
            opt.start_averaging()
    return opt, params


# ---- 3. averaged() ----
def test_averaged_exchanges_and_puts_back_whatever_is_raised():
    opt, params = stepped()
    own, avg = [bits(p) for p in params], [bits(a) for a in opt.ax_views()]
    assert not any(torch.equal(a, b) for a, b in zip(own, avg))
    versions = [p._version for p in params]
    address = opt.ax.data_ptr()
    with opt.averaged():
        assert all(torch.equal(bits(p), a) for p, a in zip(params, avg))
        assert all(torch.equal(bits(a), o) for a, o in zip(opt.ax_views(), own))
        inside = [p._version for p in params]
        assert all(b > a for a, b in zip(versions, inside))
    assert all(torch.equal(bits(p), o) for p, o in zip(params, own)) and all(torch.equal(bits(a), b) for a, b in zip(opt.ax_views(), avg))
    assert all(b > a for a, b in zip(inside, [p._version for p in params]))
    with pytest.raises(KeyError):
        with opt.averaged():
            assert torch.equal(bits(params[1]), avg[1])
            raise KeyError("mid-validation")
    assert all(torch.equal(bits(p), o) for p, o in zip(params, own)) and all(torch.equal(bits(a), b) for a, b in zip(opt.ax_views(), avg))
    assert opt.ax.data_ptr() == address


def test_averaged_before_averaging_has_started_is_a_runtime_error():
    opt, params = stepped(start_after=None)
    before = [bits(p) for p in params]
    with pytest.raises(RuntimeError):
        with opt.averaged():
            pass
    assert all(torch.equal(bits(p), b) for p, b in zip(params, before)) and not opt.averaging


# ---- 4. state_dict / load_state_dict ----
def test_the_state_round_trip_keeps_bits_and_addresses():
    opt, params = stepped(steps=5)
    opt.observe(3.0)
    sd = copy.deepcopy(opt.state_dict())
    assert sd["step"] == 5 and sd["t0"] == 2 and sd["averaging"] is True and sd["history"] == [3.0]
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(sd["ax"], opt.ax_views()))
    other, oparams = stepped(steps=1, start_after=None, seed=6)
    ax_at, words_at, norm_at = other.ax.data_ptr(), other._words.data_ptr(), other.last_norm.data_ptr()
    other.load_state_dict(sd)
    assert (other.ax.data_ptr(), other._words.data_ptr(), other.last_norm.data_ptr()) == (ax_at, words_at, norm_at)
    assert torch.equal(bits(other.ax), bits(opt.ax)) and torch.equal(other._words[:2], opt._words[:2])
    assert other.averaging and other.history == [3.0] and other.param_groups[0]["weight_decay"] == C.WD
    again = other.state_dict()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(again["ax"], sd["ax"]))
    assert {k: v for k, v in again.items() if k != "ax"} == {k: v for k, v in sd.items() if k != "ax"}
    # the loaded optimizer goes on where the saved one does: the same n, the same bits
    for src, dst in zip(params, oparams):
        dst.data.copy_(src.data)
        src.grad = torch.full_like(src, 1e-3)
        dst.grad = torch.full_like(dst, 1e-3)
    opt.step()
    other.step()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(params, oparams)) and torch.equal(bits(opt.ax), bits(other.ax))
    sd["ax"] = sd["ax"][:-1]
    with pytest.raises(ValueError):
        other.load_state_dict(sd)


# ---- 5. refusals ----
@pytest.mark.parametrize("kw", [dict(lr=-1e-3), dict(lr=float("nan")), dict(lr=float("inf")), dict(weight_decay=-0.1),
                                dict(weight_decay=float("nan")), dict(max_norm=-1.0), dict(max_norm=float("inf")), dict(nonmono=0),
                                dict(nonmono=2.5), dict(lr="1")])
def test_bad_hyper_parameters_are_value_errors_before_any_work(kw, monkeypatch):
    params = [torch.nn.Parameter(torch.ones(3))]

    def tripwire(*a, **k):
        raise AssertionError("work before the argument checks")
    monkeypatch.setattr(torch, "zeros", tripwire)
    monkeypatch.setattr(torch, "tensor", tripwire)
    with pytest.raises(ValueError):
        optim.ASGD(params, **{**dict(lr=C.LR), **kw})


def test_parameter_lists_the_step_cannot_cover_are_value_errors(monkeypatch):
    many = [torch.nn.Parameter(torch.zeros(2)) for _ in range(_lib.MAX_TENSORS + 1)]
    half = [torch.nn.Parameter(torch.zeros(2)), torch.nn.Parameter(torch.zeros(2, dtype=torch.float64))]
    strided = [torch.nn.Parameter(torch.zeros(4, 4).t()[:, :2])]
    groups = [dict(params=[torch.nn.Parameter(torch.zeros(2))]), dict(params=[torch.nn.Parameter(torch.zeros(2))])]
    monkeypatch.setattr(torch, "zeros", lambda *a, **k: (_ for _ in ()).throw(AssertionError("work before the checks")))
    for params in (many, half, strided, groups, []):
        with pytest.raises(ValueError):
            optim.ASGD(params, lr=C.LR)
    assert len(many) == 49


def test_hyper_parameters_are_read_from_the_group_at_every_step():
    opt, params = stepped(steps=0, start_after=None)
    for p in params:
        p.grad = torch.full_like(p, 1e-3)
    before = [p.detach().clone() for p in params]
    opt.param_groups[0].update(lr=0.25, weight_decay=0.0, max_norm=0.0)
    opt.step()
    assert all(torch.equal(p.detach(), b - 0.25 * torch.full_like(b, 1e-3)) for p, b in zip(params, before))
    opt.param_groups[0]["lr"] = -1.0
    with pytest.raises(ValueError):
        opt.step()


# ---- 6. symbols ----
def test_the_library_exports_the_entry_point_and_refuses_bad_arguments():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "vmlmf_hip.h")).read()
    assert hasattr(handle, "vmlmf_asgd_step") and "vmlmf_asgd_step" in _lib.SYMBOLS and "int vmlmf_asgd_step(" in header
    assert _lib.ABI_VERSION == 13 and handle.vmlmf_abi_version() == 13
    for name in ("WORDS", "STEP", "T0", "COEF", "MU", "GO", "MODE", "T0_OFF", "MODE_OFF", "MODE_COPY", "MODE_AVERAGE"):
        value = str(getattr(_lib, "ASGD_" + name))
        assert f"#define VMLMF_ASGD_{name} {value}\n" in header or f"#define VMLMF_ASGD_{name} ({value})\n" in header, name
    assert vmlmf_amd.optim.ASGD is optim.ASGD and issubclass(optim.ASGD, torch.optim.Optimizer)
    lib = _lib.lib()
    tl = _lib.TensorList()
    buf = (ctypes.c_float * 8)()
    at = ctypes.addressof(buf)
    for count in (0, _lib.MAX_TENSORS + 1):                             # the launch is never reached: no device is touched
        tl.count = count
        assert lib.vmlmf_asgd_step(ctypes.byref(tl), at, at, 0.1, 0.0, 0.0, at, at, None) == _lib.E_BADARG
    tl.count = 1
    tl.param[0], tl.grad[0], tl.numel[0] = at, at, 4
    for hole in range(4):                                               # ax, state, norm, scratch
        ptrs = [None if j == hole else at for j in range(4)]
        assert lib.vmlmf_asgd_step(ctypes.byref(tl), ptrs[0], ptrs[1], 0.1, 0.0, 0.0, ptrs[2], ptrs[3], None) == _lib.E_BADARG
    tl.state_offset[0] = -4
    assert lib.vmlmf_asgd_step(ctypes.byref(tl), at, at, 0.1, 0.0, 0.0, at, at, None) == _lib.E_BADARG
    tl.state_offset[0], tl.numel[0] = 0, -1
    assert lib.vmlmf_asgd_step(ctypes.byref(tl), at, at, 0.1, 0.0, 0.0, at, at, None) == _lib.E_BADARG
    tl.numel[0], tl.grad[0] = 4, None
    assert lib.vmlmf_asgd_step(ctypes.byref(tl), at, at, 0.1, 0.0, 0.0, at, at, None) == _lib.E_BADARG
    assert lib.vmlmf_asgd_step(None, at, at, 0.1, 0.0, 0.0, at, at, None) == _lib.E_BADARG


# ---- 7. a tiny Model, six minibatches ----
def text(seed, T, B, V=64):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, V, (T, B), generator=g)


def test_six_minibatches_of_a_tiny_model_step_by_step():
    """Model (V 64, H 8, one layer, B 2, T 5) with state carry.  Before each step a deep copy takes the model's parameters, ax and
    counters; the optimizer steps the model, the functional stock step steps the copy; both lie within the element-wise bound of
    the fp64 rule applied to the state in front of the step, so no free tolerance for drift is needed."""
    torch.manual_seed(0)
    model = Model(64, 8, 1, 0.0, 0.1, lstm_type="custom")
    params = list(model.parameters())
    opt = optim.ASGD(params, lr=C.LR, weight_decay=C.WD, max_norm=0.25, nonmono=5)
    carried = model.state_init(2)
    modes = []
    for k in range(1, 7):
        x, y = text(40 + k, 5, 2), text(60 + k, 5, 2)
        opt.zero_grad(set_to_none=True)
        loss, carried = model.loss(x, y, model.detach(carried))
        loss.backward()
        live = [i for i, p in enumerate(params) if p.grad is not None]
        assert len(live) >= 4
        twin_p = [params[i].detach().clone() for i in live]
        twin_g = [params[i].grad.detach().clone() for i in live]
        twin_ax, twin_words = opt.ax.clone(), opt._words.clone()
        offsets = [opt._offsets[i] for i in live]
        before_a = [opt.ax_views()[i].numpy().copy() for i in live]
        words = opt._words.tolist()
        assert words[_lib.ASGD_STEP] == k - 1
        want = C.asgd_oracle([t.numpy() for t in twin_p], [t.numpy() for t in twin_g], before_a, k=k, t0=words[_lib.ASGD_T0], lr=C.LR,
                             wd=C.WD, max_norm=0.25)
        modes.append((want["mode"], want["c"] < 1))
        opt.step()
        optim.asgd_step_stock(twin_p, twin_g, twin_ax, twin_words, offsets, lr=C.LR, weight_decay=C.WD, max_norm=0.25)
        assert abs(float(opt.last_norm) - want["norm"]) <= C.NORM_RTOL * want["norm"]
        assert_within([params[i].detach().numpy() for i in live], [params[i].grad.numpy() for i in live],
                      [opt.ax_views()[i].numpy() for i in live], want, f"model step {k}")
        assert_within([t.numpy() for t in twin_p], [t.numpy() for t in twin_g],
                      [twin_ax[o:o + t.numel()].numpy() for o, t in zip(offsets, twin_p)], want, f"twin step {k}")
        assert torch.equal(twin_words, opt._words)
        if k == 2:
            opt.start_averaging()
    assert [m for m, _ in modes] == ["off", "off", "copy", "copy", "average", "average"]


# ---- 8. update_fn's signature ----
def test_clip_step_is_step_with_the_two_values_set():
    a, pa = stepped(steps=3)
    b, pb = stepped(steps=3)
    for p, q in zip(pa, pb):
        p.grad = torch.full_like(p, 3e-2)
        q.grad = torch.full_like(q, 3e-2)
    a.param_groups[0].update(lr=0.25, max_norm=0.01)
    a.step()
    norm = b.clip_step(pb, 0.25, 0.01)
    assert norm is b.last_norm and norm.dim() == 0 and torch.equal(bits(norm), bits(a.last_norm)) and float(norm) > 0.01
    assert b.param_groups[0]["lr"] == 0.25 and b.param_groups[0]["max_norm"] == 0.01
    assert all(torch.equal(bits(p), bits(q)) for p, q in zip(pa, pb)) and torch.equal(bits(a.ax), bits(b.ax))
    assert all(torch.equal(bits(p.grad), bits(q.grad)) for p, q in zip(pa, pb))
