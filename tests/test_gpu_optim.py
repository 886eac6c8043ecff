"""GPU: the optimizer launches of csrc/vmlmf_optim.hip - Adam in its four forms (adam_fused_kernel; tick_health_kernel, tick_kernel or
adam_gate_kernel in front of adam_kernel) and clip + SGD (sqsum_kernel, norm_kernel, sgd_clip_kernel) - element by element against the
fp64 oracle of tests/optim_cases.py, within the counted bounds of docs/design/optimizer_bounds.md, on every alignment path, and the
verdicts of the two guards word by word."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import optim_cases as C
import vmlmf_amd
from abi_arena import FILL_NAN, Arena
from vmlmf_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
GO, TICKET, SKIPPED = _lib.GUARD_GO, 65, _lib.GUARD_SKIPPED
WHOLE_STEP = _lib.ADAM_FIRST | _lib.ADAM_LAST
ROUTES = ("plain", "guarded", "ex")          # vmlmf_adam_step, vmlmf_adam_step_guarded, vmlmf_adam_step_ex


@pytest.fixture(autouse=True)
def clean_health_word():
    """Earlier tests may have written non-finite gradients that no guarded step consumed."""
    torch.cuda.synchronize()
    _lib.tune("clear_health", 0)


@contextlib.contextmanager
def scanning_gate():
    _lib.tune("adam_guard", 2)
    try:
        yield
    finally:
        _lib.tune("adam_guard", 1)


def words(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def place(a, misaligned=False):
    """(view, address) of the fp32 array on the device inside an allocation of its own; misaligned: one float behind a 16-byte
    boundary.  The address is kept beside the view: torch has none for a tensor without elements."""
    buf = torch.zeros(a.size + 8, device=DEV)
    o = 1 if misaligned else 0
    view = buf[o:o + a.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    ptr = buf.data_ptr() + 4 * o
    assert ptr % 16 == 4 * o
    return view, ptr


def tensor_list(params, grads, numels, offsets=None, sidx=None):
    tl = _lib.TensorList()
    for i, ((_, p), (_, g), n) in enumerate(zip(params, grads, numels)):
        tl.param[i], tl.grad[i], tl.numel[i] = p, g, n
        tl.state_offset[i] = 0 if offsets is None else offsets[i]
        tl.step_index[i] = 0 if sidx is None else sidx[i]
    tl.count = len(numels)
    return tl


def adam_call(route, tl, state, hyper, guard=None, flags=WHOLE_STEP):
    lib = _lib.lib()
    stream = _lib.raw_stream(state["m"].device)
    args = (ctypes.byref(tl), state["m"].data_ptr(), state["v"].data_ptr(), state["steps"].data_ptr(),
            *(float(hyper[k]) for k in ("lr", "b1", "b2", "eps", "wd")))
    if route == "plain":
        _lib.check(lib.vmlmf_adam_step(*args, stream))
    elif route == "guarded":
        _lib.check(lib.vmlmf_adam_step_guarded(*args, guard.data_ptr(), stream))
    else:
        _lib.check(lib.vmlmf_adam_step_ex(*args, guard.data_ptr(), flags, stream))


def new_guard():
    return torch.zeros(_lib.GUARD_WORDS, device=DEV, dtype=torch.int32)


def assert_guard(guard, go, skipped):
    w = words(guard)
    assert (w[GO], w[SKIPPED], w[TICKET]) == (go, skipped, 0), (w[GO], w[SKIPPED], w[TICKET])
    assert not np.delete(w, [GO, TICKET, SKIPPED]).any()


def device_adam(fx):
    """The fixture on the device: parameters and gradients as the layout places them, the flat moments, the counters, the list."""
    mis = fx.get("misalign", {})
    params = [place(a, mis.get(i) == "param") for i, a in enumerate(fx["p"])]
    grads = [place(a, mis.get(i) == "grad") for i, a in enumerate(fx["g"])]
    state = dict(m=torch.from_numpy(fx["m_flat"]).to(DEV), v=torch.from_numpy(fx["v_flat"]).to(DEV),
                 steps=torch.from_numpy(fx["steps"]).to(DEV))
    return params, grads, state, tensor_list(params, grads, fx["numels"], fx["offsets"], fx["sidx"])


def read_adam(fx, params, state):
    m, v = state["m"].cpu().numpy(), state["v"].cpu().numpy()
    spans = list(zip(fx["offsets"], fx["numels"]))
    return [p.cpu().numpy() for p, _ in params], [m[o:o + n] for o, n in spans], [v[o:o + n] for o, n in spans]


def snapshot(params, state):
    return [words(p) for p, _ in params] + [words(state[k]) for k in ("m", "v", "steps")]


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def assert_adam_step(fx, params, grads, state, hyper, label=None):
    """Every element of p, exp_avg and exp_avg_sq within the bounds of the oracle's step from the fixture; the counters start + 1
    exactly; the gradients' bits and the state words no tensor owns as they were.  Returns the worst error / bound of (p, m, v)."""
    g = fx["g"]
    want = C.adam_oracle(fx["p"], g, fx["m"], fx["v"], fx["starts"], **hyper)
    got = read_adam(fx, params, state)
    worst = C.adam_ratios(*got, want)
    assert max(worst) <= 1.0, (label, worst)
    steps = state["steps"].cpu().numpy()
    assert all(steps[k] == s + 1 for k, s in zip(fx["sidx"], fx["starts"])), (label, steps)
    assert all(np.array_equal(words(t), a.view(np.uint32)) for (t, _), a in zip(grads, g))
    owned = np.zeros(fx["total"] + 1, bool)
    for o, n in zip(fx["offsets"], fx["numels"]):
        owned[o:o + n] = True
    for k in ("m", "v"):
        assert np.array_equal(words(state[k])[~owned], fx[k + "_flat"].view(np.uint32)[~owned]), (label, k)
    if hyper["wd"] == 0:
        for p0, gi, mi, vi, p1 in zip(fx["p"], g, fx["m"], fx["v"], got[0]):
            still = (gi == 0) & (mi == 0) & (vi == 0)
            assert np.array_equal(p1.view(np.uint32)[still], p0.view(np.uint32)[still]), label
    return worst


# ---- Adam, element by element ----
def seed_of(layout, hyper, start):
    return 100 + 31 * list(C.LAYOUTS).index(layout) + 7 * list(C.HYPERS).index(hyper) + list(C.STARTS).index(start)


@pytest.mark.parametrize("hyper", list(C.HYPERS))
@pytest.mark.parametrize("layout", list(C.LAYOUTS))
def test_adam_is_the_oracle_elementwise(layout, hyper):
    """Every layout x hyper-parameter set, at every initial step count (0 with zero moments, 9, 999, 99999, and a list whose tensors
    differ), through the three entry points in turn.  `million` takes tick_health_kernel + adam_kernel on the guarded routes."""
    hp = C.HYPERS[hyper]
    worst = np.zeros(3)
    for si, start in enumerate(C.STARTS):
        route = ROUTES[(list(C.HYPERS).index(hyper) + si) % 3]
        fx = C.adam_fixture(layout, start, seed_of(layout, hyper, start))
        params, grads, state, tl = device_adam(fx)
        guard = new_guard()
        adam_call(route, tl, state, hp, guard)
        worst = np.maximum(worst, assert_adam_step(fx, params, grads, state, hp, label=(start, route)))
        assert_guard(guard, 0 if route == "plain" else 1, 0)
    print(f"adam {layout} {hyper}: worst error / bound p {worst[0]:.3f}, m {worst[1]:.3f}, v {worst[2]:.3f}")


def with_one_more(fx, n, start, seed):
    """The fixture with one more tensor of n elements behind the others (state, counter and all)."""
    p, g, m, v = C.adam_case([n], [start], seed)
    out = dict(fx)
    count = len(fx["numels"])
    offset = (fx["total"] + 3) // 4 * 4
    out.update(numels=fx["numels"] + [n], starts=fx["starts"] + [start], offsets=fx["offsets"] + [offset], total=offset + n,
               sidx=fx["sidx"] + [count], p=fx["p"] + p, g=fx["g"] + g, m=fx["m"] + m, v=fx["v"] + v,
               steps=np.concatenate([fx["steps"], np.float32([start])]))
    for k in ("m", "v"):
        flat = np.zeros(offset + n + 1, np.float32)
        flat[:fx["total"] + 1] = fx[k + "_flat"]
        flat[offset:offset + n] = out[k][-1]
        out[k + "_flat"] = flat
    return out


def test_the_four_routes_give_the_same_bits():
    """One list of small tensors through adam_fused_kernel (guarded), tick_health_kernel + adam_kernel (the same list and a tensor
    of 2^20 + 13 elements), tick_kernel + adam_kernel (no guard) and adam_gate_kernel + adam_kernel (the scanning guard): parameters,
    moments and counters of the shared tensors to the bit, whichever form a model's sizes or guard mode select."""
    hp = C.HYPERS["wd"]
    small = C.adam_fixture("packed_offsets", "mixed", 77)
    shared = len(small["numels"])

    def run(fx, route, gate=False):
        params, grads, state, tl = device_adam(fx)
        guard = new_guard()
        with scanning_gate() if gate else contextlib.nullcontext():
            adam_call(route, tl, state, hp, guard)
        torch.cuda.synchronize()
        assert_guard(guard, 0 if route == "plain" else 1, 0)
        p, m, v = read_adam(fx, params, state)
        steps = state["steps"].cpu().numpy()
        return [a.view(np.uint32) for a in p[:shared] + m[:shared] + v[:shared]] + [steps[:shared].view(np.uint32)]

    fused = run(small, "guarded")
    two_launch = run(with_one_more(small, C.BIG, 9, 78), "guarded")
    unguarded = run(small, "plain")
    gated = run(small, "guarded", gate=True)
    for name, other in (("tick_health + adam_kernel", two_launch), ("tick + adam_kernel", unguarded), ("gate + adam_kernel", gated)):
        assert same_bits(fused, other), name
    assert not same_bits(fused[:shared], [a.view(np.uint32) for a in small["p"]])


# ---- the scanning gate ----
def list_of(numels, seed, start=9):
    """An Adam fixture over `numels` with packed state offsets."""
    count = len(numels)
    starts = [start] * count
    offsets, total = C.offsets_of(numels, False)
    sidx = [count - 1 - i for i in range(count)]
    p, g, m, v = C.adam_case(numels, starts, seed)
    return dict(numels=list(numels), starts=starts, offsets=offsets, total=total, sidx=sidx, misalign={}, p=p, g=g, m=m, v=v,
                m_flat=C.flat_state(m, offsets, total + 1), v_flat=C.flat_state(v, offsets, total + 1),
                steps=np.full(count, start, np.float32))


WIDE = 3 * 2 ** 17          # 393 216 elements: 1536 workgroups asked for, 1024 launched, the scan's grid-stride loop wraps
GATE_POSITIONS = {
    "element_0": (C.SIZES, 0, 0),
    "last_of_the_longest": (C.SIZES, 7, -1),
    "last_of_a_short_tensor_beside_a_long_one": (C.SIZES, 3, -1),
    "tensor_16_of_17": ([C.SIZES[i % 8] for i in range(17)], 16, -1),
    "tensor_47_of_48": (C.LAYOUTS["count_48"]["numels"], 47, -1),
    "beyond_262144": ([5, WIDE, 1025], 1, 300001),
}


@pytest.mark.parametrize("position", list(GATE_POSITIONS))
def test_the_scanning_gate_sees_one_bad_value_anywhere(position):
    """adam_guard = 2: one NaN, +Inf or -Inf in the listed gradients - nothing moves, GO = 0, one more skipped step, the ticket word
    back at 0, every other guard word 0.  Then a clean step on the same guard block goes ahead and is the oracle's step."""
    numels, ti, at = GATE_POSITIONS[position]
    hp = C.HYPERS["defaults"]
    fx = list_of(numels, 200 + len(numels))
    params, _, state, _ = device_adam(fx)
    guard = new_guard()
    held = snapshot(params, state)
    with scanning_gate():
        for k, bad in enumerate((np.nan, np.inf, -np.inf)):
            g = [a.copy() for a in fx["g"]]
            g[ti][at] = bad
            grads = [place(a) for a in g]
            adam_call("guarded", tensor_list(params, grads, fx["numels"], fx["offsets"], fx["sidx"]), state, hp, guard)
            torch.cuda.synchronize()
            assert same_bits(snapshot(params, state), held), bad
            assert_guard(guard, 0, k + 1)
        grads = [place(a) for a in fx["g"]]
        adam_call("guarded", tensor_list(params, grads, fx["numels"], fx["offsets"], fx["sidx"]), state, hp, guard)
        torch.cuda.synchronize()
    assert_guard(guard, 1, 3)
    worst = assert_adam_step(fx, params, grads, state, hp)
    print(f"adam behind the gate {position}: worst error / bound p {worst[0]:.3f}, m {worst[1]:.3f}, v {worst[2]:.3f}")


def test_the_scanning_gate_passes_every_finite_value_and_reads_no_empty_tensor():
    """The largest finite float, denormals and -0.0 are finite; a tensor of no elements whose pointers sit on NaN words has no element
    to look at.  The step goes ahead: the ordinary tensors are the oracle's step, the special one has taken its first moment."""
    hp = C.HYPERS["defaults"]
    fx = list_of([16] + C.SIZES, 230, start=0)
    special = np.float32([C.FLT_MAX, -C.FLT_MAX, 1e-40, -1e-45, -0.0, 0.0, 1.1754944e-38, -1.1754942e-38] * 2)
    fx["g"][0] = special
    params, grads, state, _ = device_adam(fx)
    arena = Arena(DEV, FILL_NAN, capacity=1 << 16)
    empty = arena.buf(4, torch.float32, name="empty")
    assert bool(torch.isnan(empty).all())
    # the empty entry FIRST: the scan's padding lanes repeat the first tensor of a group of sixteen
    ptrs = [(None, empty.data_ptr())]
    tl = tensor_list(ptrs + params, ptrs + grads, [0] + fx["numels"], [0] + fx["offsets"], [len(fx["numels"])] + fx["sidx"])
    state["steps"] = torch.zeros(len(fx["numels"]) + 1, device=DEV)
    guard = new_guard()
    with scanning_gate():
        adam_call("guarded", tl, state, hp, guard)
        torch.cuda.synchronize()
    assert_guard(guard, 1, 0)
    arena.check_guards()
    assert bool(torch.isnan(empty).all())
    assert np.array_equal(state["steps"].cpu().numpy(), np.ones(len(fx["numels"]) + 1, np.float32))
    got = read_adam(fx, params, state)
    want = C.adam_oracle(fx["p"], fx["g"], fx["m"], fx["v"], fx["starts"], **hp)
    assert max(C.adam_ratios(*(x[1:] for x in got), tuple(x[1:] for x in want))) <= 1.0
    huge = np.abs(special) == C.FLT_MAX
    _, bm, _ = C.adam_bounds(want[3][0], want[2][0])
    assert (np.abs(got[1][0].astype(np.float64) - want[1][0]) <= bm)[huge].all() and huge.sum() == 4


def test_optim_adam_gates_each_list_of_a_large_model_by_itself():
    """53 parameters are two lists.  Under the scanning guard every call gates its own list (include/vmlmf_hip.h: "gated per call"):
    a NaN in the second list leaves the second list as it was, the first list steps, one skipped step is counted."""
    gen = torch.Generator().manual_seed(5)
    params = [torch.nn.Parameter(torch.randn(3 + i % 7, generator=gen).to(DEV)) for i in range(53)]
    opt = vmlmf_amd.optim.Adam(params, lr=1e-2)
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen).to(DEV)
    params[50].grad[-1] = float("nan")
    held = [words(p) for p in params]
    with scanning_gate():
        opt.step()
        torch.cuda.synchronize()
        assert opt.skipped_steps() == 1
    for i, (p, h) in enumerate(zip(params, held)):
        assert np.array_equal(words(p), h) == (i >= 48), i
        assert float(opt.state[p]["step"]) == (0.0 if i >= 48 else 1.0)
        if i >= 48:
            assert not opt.state[p]["exp_avg"].any() and not opt.state[p]["exp_avg_sq"].any()


# ---- one verdict per step on the two-launch form ----
def optimizer_state(opt, params):
    """(p, m, v, step counts) of an optim.Adam as fp32 arrays; a parameter the optimizer has not seen yet has zeros."""
    p = [q.detach().cpu().numpy().ravel() for q in params]
    m = [opt.state[q]["exp_avg"].cpu().numpy().ravel() if q in opt.state and opt.state[q] else np.zeros_like(a) for q, a in zip(params, p)]
    v = [opt.state[q]["exp_avg_sq"].cpu().numpy().ravel() if q in opt.state and opt.state[q] else np.zeros_like(a) for q, a in zip(params, p)]
    steps = [float(opt.state[q]["step"]) if q in opt.state and opt.state[q] else 0.0 for q in params]
    return p, m, v, steps


def hyper_of(group):
    return dict(lr=group["lr"], b1=group["betas"][0], b2=group["betas"][1], eps=group["eps"], wd=group["weight_decay"])


def assert_optimizer_step(opt, before, grads, label=None):
    """optim.Adam's step from `before` (optimizer_state per group) under `grads` (per group: fp32 arrays, None where a parameter had
    no gradient): the stepped ones within the bounds, the others with the bits and the count they had.  Worst error / bound."""
    worst = np.zeros(3)
    for group, (p0, m0, v0, s0), gs in zip(opt.param_groups, before, grads):
        p1, m1, v1, s1 = optimizer_state(opt, group["params"])
        live = [i for i, g in enumerate(gs) if g is not None]
        pick = lambda seq: [seq[i] for i in live]
        want = C.adam_oracle(pick(p0), pick(gs), pick(m0), pick(v0), pick(s0), **hyper_of(group))
        r = C.adam_ratios(pick(p1), pick(m1), pick(v1), want)
        assert max(r) <= 1.0, (label, r)
        worst = np.maximum(worst, r)
        for i in range(len(p0)):
            if i in live:
                assert s1[i] == s0[i] + 1
            else:
                assert s1[i] == s0[i] and all(np.array_equal(a[i].view(np.uint32), b[i].view(np.uint32))
                                              for a, b in ((p0, p1), (m0, m1), (v0, v1)))
    return worst


def test_a_failed_backward_skips_the_two_launch_list_behind_it():
    """The health word set honestly: a VMLMF layer's backward under an infinite upstream gradient writes non-finite parameter gradients
    (finish_put marks the word; no worker gives up).  The step's first list is small (adam_fused_kernel, FIRST, takes the verdict), its
    second holds a tensor of 2^20 + 13 elements with finite gradients: tick_health_kernel reads guard[GO] and adam_kernel returns on
    it.  Nothing moves, one skipped step, the word is clear afterwards: the next step is the oracle's step for every tensor."""
    from vmlmf_amd import MyLSTM, MyVMLMFCell, Net
    torch.manual_seed(3)
    net = Net(9, layer_sizes=[40], w_rank=8, u_rank=[8], model=MyLSTM, cell=MyVMLMFCell).to(DEV)
    x = torch.randn(16, 12, 9, device=DEV)
    big = torch.nn.Parameter(0.1 * torch.randn(C.BIG, device=DEV))
    groups = [{"params": list(net.parameters())}, {"params": [big], "lr": 2e-3, "weight_decay": 0.01}]
    opt = vmlmf_amd.optim.Adam(groups, lr=1e-3)

    def backward(upstream):
        net.zero_grad(set_to_none=True)
        out = net(x)
        out.backward(torch.full_like(out, upstream))
        big.grad = 1e-2 * torch.randn(C.BIG, device=DEV)

    everything = [p for g in opt.param_groups for p in g["params"]]
    backward(float("inf"))
    torch.cuda.synchronize()
    _lib.check_status()                                  # nobody gave up a wait
    assert any(not torch.isfinite(p.grad).all() for p in net.parameters() if p.grad is not None)
    assert bool(torch.isfinite(big.grad).all())
    held = [words(p) for p in everything]
    opt.step()
    torch.cuda.synchronize()
    assert opt.skipped_steps() == 1
    assert_guard(opt._guard, 0, 1)
    assert all(np.array_equal(words(p), h) for p, h in zip(everything, held))
    for p in everything:
        if p.grad is not None:
            assert float(opt.state[p]["step"]) == 0.0 and not opt.state[p]["exp_avg"].any() and not opt.state[p]["exp_avg_sq"].any()
    backward(1.0)
    before = [optimizer_state(opt, g["params"]) for g in opt.param_groups]
    grads = [[None if p.grad is None else p.grad.detach().cpu().numpy().ravel() for p in g["params"]] for g in opt.param_groups]
    assert all(g is None or np.isfinite(g).all() for gs in grads for g in gs)
    opt.step()
    torch.cuda.synchronize()
    assert opt.skipped_steps() == 1
    assert_guard(opt._guard, 1, 1)
    worst = assert_optimizer_step(opt, before, grads)
    print(f"adam behind a failed step: worst error / bound p {worst[0]:.3f}, m {worst[1]:.3f}, v {worst[2]:.3f}")


# ---- clip + SGD, element by element ----
def sgd_call(tl, lr, max_norm):
    norm = torch.empty((), device=DEV)
    scratch = torch.empty(_lib.MAX_TENSORS * 64, device=DEV)
    _lib.check(_lib.lib().vmlmf_sgd_clip_step(ctypes.byref(tl), float(lr), float(max_norm), norm.data_ptr(), scratch.data_ptr(),
                                              _lib.raw_stream(norm.device)))
    return norm


def assert_sgd_step(p, g, params, grads, norm, lr, max_norm):
    """Norm, parameters and gradients against the oracle, every element; c == 1: the gradient words are the ones handed in."""
    wp, wg, ref, c = C.sgd_clip_oracle(p, g, lr=lr, max_norm=max_norm)
    assert abs(float(norm) - ref) <= C.NORM_RTOL * ref
    worst = np.zeros(2)
    for pi, gi, (pt, _), (gt, _), a, b in zip(p, g, params, grads, wp, wg):
        bp, bg = C.sgd_bounds(pi, b, lr=lr, c=c)
        ep = np.abs(pt.cpu().numpy().astype(np.float64) - a)
        eg = np.abs(gt.cpu().numpy().astype(np.float64) - b)
        assert (ep <= bp).all() and (eg <= bg).all()
        if c == 1.0:
            assert np.array_equal(words(gt), gi.view(np.uint32))
        if pi.size:
            with np.errstate(divide="ignore", invalid="ignore"):
                worst = np.maximum(worst, [np.where(ep == 0, 0, ep / bp).max(), np.where(eg == 0, 0, eg / bg).max()])
    return worst, c


LR_SGD = 0.5


@pytest.mark.parametrize("which", ["as_laid_out", "param", "grad"])
@pytest.mark.parametrize("layout", list(C.LAYOUTS))
def test_clip_sgd_is_the_oracle_elementwise(layout, which):
    """Every layout with its own placement, with every parameter misaligned (sgd_clip_kernel's scalar loop) and with every gradient
    misaligned (that and sqsum_kernel's scalar branch), at the three clips: active, inactive (the gradient words untouched), off."""
    case = C.LAYOUTS[layout]
    p, g = C.sgd_case(case["numels"], 300 + list(C.LAYOUTS).index(layout))
    _, _, norm, _ = C.sgd_clip_oracle(p, g, lr=LR_SGD, max_norm=0.0)
    worst, cs = np.zeros(2), []
    for factor in C.CLIPS.values():
        mis = case["misalign"] if which == "as_laid_out" else {i: which for i in range(len(p))}
        params = [place(a, mis.get(i) == "param") for i, a in enumerate(p)]
        grads = [place(a, mis.get(i) == "grad") for i, a in enumerate(g)]
        got = sgd_call(tensor_list(params, grads, case["numels"]), LR_SGD, factor * norm)
        w, c = assert_sgd_step(p, g, params, grads, got, LR_SGD, factor * norm)
        worst = np.maximum(worst, w)
        cs.append(c)
    assert cs[0] < 1.0 and cs[1] == 1.0 and cs[2] == 1.0
    print(f"clip + SGD {layout} {which}: worst error / bound p {worst[0]:.3f}, g {worst[1]:.3f}")


def test_clip_sgd_step_on_parameters_and_misaligned_against_aligned():
    """vmlmf_amd.optim.clip_sgd_step on Parameters, a misaligned and an aligned copy of the same data: both the oracle's step, and
    within twice the bound of each other (bit equality is not asked: the norm's summation order differs)."""
    p, g = C.sgd_case(C.SIZES, 340)
    _, _, norm, _ = C.sgd_clip_oracle(p, g, lr=LR_SGD, max_norm=0.0)
    for factor in C.CLIPS.values():
        copies = []
        for off in (0, 1):
            params = [place(a, off == 1 and i % 2 == 0) for i, a in enumerate(p)]
            grads = [place(a, off == 1 and i % 3 != 0) for i, a in enumerate(g)]
            modules = [torch.nn.Parameter(v) for v, _ in params]
            for q, (v, _), (gv, _) in zip(modules, params, grads):
                assert q.data_ptr() == v.data_ptr()
                q.grad = gv
                assert q.grad.data_ptr() == gv.data_ptr()
            versions = [q._version for q in modules]
            got = vmlmf_amd.optim.clip_sgd_step(modules, lr=LR_SGD, max_norm=factor * norm)
            assert all(q._version > v for q, v in zip(modules, versions))
            assert_sgd_step(p, g, params, grads, got, LR_SGD, factor * norm)
            copies.append((params, grads))
        wp, wg, _, c = C.sgd_clip_oracle(p, g, lr=LR_SGD, max_norm=factor * norm)
        for i, (pi, b) in enumerate(zip(p, wg)):
            bp, bg = C.sgd_bounds(pi, b, lr=LR_SGD, c=c)
            (pa, _), (pb, _) = copies[0][0][i], copies[1][0][i]
            (ga, _), (gb, _) = copies[0][1][i], copies[1][1][i]
            assert (np.abs(pa.cpu().numpy().astype(np.float64) - pb.cpu().numpy()) <= 2 * bp).all()
            assert (np.abs(ga.cpu().numpy().astype(np.float64) - gb.cpu().numpy()) <= 2 * bg).all()


@pytest.mark.parametrize("which", ["aligned", "grad"])
def test_clip_sgd_changes_nothing_without_a_gradient_or_a_finite_norm(which):
    """All-zero gradients: norm 0, parameters and gradients keep their bits.  Finite gradients whose fp32 sum of squares overflows:
    the norm comes back inf and the step is skipped."""
    p, g = C.sgd_case(C.SIZES, 350)
    zero = [np.zeros_like(a) for a in g]
    over = [a.copy() for a in g]
    over[5][:] = 3e19
    over[7][-1] = -3e19
    assert all(np.isfinite(a).all() for a in over)
    for bad, want in ((zero, 0.0), (over, np.inf)):
        assert C.sgd_clip_oracle(p, bad, lr=LR_SGD, max_norm=0.25)[2] == want
        params = [place(a) for a in p]
        grads = [place(a, which == "grad") for a in bad]
        norm = sgd_call(tensor_list(params, grads, C.SIZES), LR_SGD, 0.25)
        assert float(norm) == want
        assert all(np.array_equal(words(t), a.view(np.uint32)) for (t, _), a in zip(params, p))
        assert all(np.array_equal(words(t), a.view(np.uint32)) for (t, _), a in zip(grads, bad))


# ---- a trajectory through optim.Adam ----
def test_eight_steps_follow_the_oracle_step_by_step():
    """The never / late gradient pattern of test_fused_adam_matches_torch_adam, two parameter groups with different lr and weight
    decay, one gradient that is not contiguous: every step is held element-wise, within the bounds, against the fp64 oracle's step
    from the state read back from the device in front of it - bounds do not compound, and one wrong element at one step count shows."""
    gen = torch.Generator().manual_seed(11)
    shapes = [(9, 16), (720, 16), (1, 180), (720,), (18, 180), (5,)]
    params = [torch.nn.Parameter(torch.randn(*s, generator=gen).to(DEV)) for s in shapes]
    opt = vmlmf_amd.optim.Adam([{"params": params[:3]}, {"params": params[3:], "lr": 5e-4, "weight_decay": 0.01}], lr=2e-3)
    worst = np.zeros(3)
    for it in range(8):
        for k, p in enumerate(params):
            if k == 5 or (k == 4 and it < 2):       # never / late
                p.grad = None
            elif k == 1:
                p.grad = torch.randn(16, 720, generator=gen).to(DEV).t()
                assert not p.grad.is_contiguous()
            else:
                p.grad = torch.randn(*p.shape, generator=gen).to(DEV)
        before = [optimizer_state(opt, g["params"]) for g in opt.param_groups]
        grads = [[None if p.grad is None else p.grad.detach().cpu().contiguous().numpy().ravel() for p in g["params"]]
                 for g in opt.param_groups]
        opt.step()
        torch.cuda.synchronize()
        worst = np.maximum(worst, assert_optimizer_step(opt, before, grads, label=it))
    assert [float(opt.state[p]["step"]) for p in params[:5]] == [8.0, 8.0, 8.0, 8.0, 6.0] and opt.skipped_steps() == 0
    print(f"adam trajectory: worst error / bound p {worst[0]:.3f}, m {worst[1]:.3f}, v {worst[2]:.3f}")
