"""Weight tying and word-level embedding dropout on the GPU (docs/design/lm_tied.md): vmlmf_embed_dropout_forward_ex and
vmlmf_embed_backward_ex on the cases of tied_cases.py - against the existing entry points, the numpy restatement and an fp64 sum, to
the bit where the contract says so; rows the accumulating form must not touch are poisoned; a tied Model against its untied twin; the
fused route; embed_dropout against the stock formulation; a captured step; decoding, scoring and the optimizers on a tied model."""
import copy

import numpy as np
import pytest
import torch

import tied_cases as C
from hip_util import assert_grad
import vmlmf_amd
from vmlmf_amd import Model, _lib, optim, unit_gradient
from vmlmf_amd import functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0x7FC12345          # a NaN with a payload: a row that was rewritten, even with itself plus zero, loses these bits


def snapshot(offset):
    return torch.tensor([C.SEED, offset], dtype=torch.int64, device=DEV)


def dev(a):
    return torch.as_tensor(a).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def fwd_ex(w, tok, p, word_p, snap, out=None):
    V, H = w.shape
    out = torch.empty((tok.numel(), H), device=DEV) if out is None else out
    _lib.check(_lib.lib().vmlmf_embed_dropout_forward_ex(tok.numel(), H, V, _lib.ptr(tok), _lib.ptr(w), _lib.ptr(out), p, word_p, _lib.ptr(snap), 0,
                                                         _lib.raw_stream(w.device)))
    return out


def bwd_ex(tok, dy, V, accumulate, p, word_p, snap, dw=None):
    R, H = dy.shape
    lib = _lib.lib()
    nbytes = lib.vmlmf_embed_backward_scratch_bytes(R, V)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    dw = torch.full((V, H), float("nan"), device=DEV) if dw is None else dw
    _lib.check(lib.vmlmf_embed_backward_ex(R, H, V, _lib.ptr(tok), _lib.ptr(dy), _lib.ptr(dw), accumulate, scratch.data_ptr(), nbytes, p, word_p,
                                           _lib.ptr(snap), 0, _lib.raw_stream(dy.device)))
    return dw


def bwd_old(tok, dy, V, p, snap):
    """The entry points that were there before: vmlmf_embed_backward at p == 0, vmlmf_embed_dropout_backward otherwise."""
    R, H = dy.shape
    lib = _lib.lib()
    nbytes = lib.vmlmf_embed_backward_scratch_bytes(R, V)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    dw = torch.full((V, H), float("nan"), device=DEV)
    if p == 0:
        _lib.check(lib.vmlmf_embed_backward(R, H, V, _lib.ptr(tok), _lib.ptr(dy), _lib.ptr(dw), scratch.data_ptr(), nbytes, _lib.raw_stream(dy.device)))
    else:
        _lib.check(lib.vmlmf_embed_dropout_backward(R, H, V, _lib.ptr(tok), _lib.ptr(dy), _lib.ptr(dw), scratch.data_ptr(), nbytes, p, _lib.ptr(snap), 0,
                                                    _lib.raw_stream(dy.device)))
    return dw


def kernel_factors(R, V, H, p, word_p, snap):
    f = F.dropout_factors(R, H, p, snap, 0) if p > 0 else torch.ones((R, H), device=DEV)
    fw = vmlmf_amd.word_dropout_factors(V, word_p, snap)
    return f, fw


# ---- 1. the kernels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.SHAPES, ids=C.IDS)
def test_the_kernels_on_every_case(shape):
    R, V, H = shape
    w_np, dy_np, base_np = C.draw(R, V, H, 21)
    w, dy = dev(w_np), dev(dy_np)
    for j, pattern in enumerate(C.PATTERNS):
        tok_np = C.tokens(R, V, pattern, j)
        tok = dev(tok_np)
        hit = torch.bincount(tok, minlength=V) > 0
        for k, (p, word_p) in enumerate(C.DROPS):
            what = f"{pattern} p={p} word_p={word_p}"
            offset = C.OFFSETS[(j + k) % 3]
            snap = snapshot(offset)
            f, fw = kernel_factors(R, V, H, p, word_p, snap)
            f_np, fw_np = C.element_factors(R, H, p, offset), C.word_factors(V, word_p, offset)
            assert C.same_bits(f.cpu().numpy(), f_np) and C.same_bits(fw.cpu().numpy(), fw_np), what       # the oracle's factors
            kept = fw != 0
            if word_p > 0 and V >= 6:
                assert bool(kept.any()) and bool((~kept).any()), what                                       # both kinds of row
            # forward: two single-rounded multiplications, the word factor first
            out = fwd_ex(w, tok, p, word_p, snap)
            assert torch.equal(out, (w[tok] * fw[tok, None]) * f), what
            assert torch.equal(out, dev(C.forward(w_np, tok_np, f_np, fw_np))), what
            # backward, accumulate == 0: the existing entry points' bits, times the word factor
            old = bwd_old(tok, dy, V, p, snap)
            got = bwd_ex(tok, dy, V, 0, p, word_p, snap)
            if word_p == 0:
                assert torch.equal(bits(got), bits(old)), what
            else:
                assert torch.equal(bits(got[kept]), bits((fw[:, None] * old)[kept])) and bool((got[~kept] == 0).all()), what
            assert bool((got[~hit] == 0).all()), what
            assert C.same_bits(got.cpu().numpy(), C.table_gradient(tok_np, dy_np, f_np, fw_np, V)), what
            worst = C.excess(got.cpu().numpy(), tok_np, dy_np, f_np, fw_np, V)
            assert worst <= 1.0, (what, worst)
            # accumulate == 1 onto a random base; rows that are not hit-and-kept are poisoned and must keep their bits
            rows = hit & kept
            base = dev(base_np).clone()
            bits(base)[~rows] = POISON
            acc = bwd_ex(tok, dy, V, 1, p, word_p, snap, dw=base.clone())
            assert torch.equal(bits(acc[~rows]), bits(base[~rows])), what
            assert torch.equal(bits(acc[rows]), bits((base + got)[rows])), what
            assert C.same_bits(acc.cpu().numpy(), C.table_gradient(tok_np, dy_np, f_np, fw_np, V, base=base.cpu().numpy())), what
            clean = torch.where(rows[:, None], acc, torch.zeros_like(acc)).cpu().numpy()
            worst = C.excess(clean, tok_np, dy_np, f_np, fw_np, V, np.where(rows.cpu().numpy()[:, None], base_np, np.float32(0)))
            print(f"{C.IDS[C.SHAPES.index(shape)]} {what}: accumulate at {worst:.3f} of the bound")
            assert worst <= 1.0, (what, worst)


# ---- 2. the same bits twice; misaligned views ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(70, 12, 650), (64, 8, 260), (40, 7, 5)], ids=["70x12x650", "64x8x260", "40x7x5"])
def test_two_runs_give_the_same_bits_and_misaligned_views_work(shape):
    R, V, H = shape
    w_np, dy_np, base_np = C.draw(R, V, H, 22)
    tok = dev(C.tokens(R, V, "last", 5))
    snap = snapshot(7)
    w, dy, base = dev(w_np), dev(dy_np), dev(base_np)

    def off(t, by):          # the same values in a view that starts `by` floats behind a 256-byte boundary
        flat = torch.empty(t.numel() + by, device=DEV)
        view = flat[by:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == (4 * by) % 16
        return view
    for p, word_p in C.DROPS:
        ref_out = fwd_ex(w, tok, p, word_p, snap)
        ref0 = bwd_ex(tok, dy, V, 0, p, word_p, snap)
        ref1 = bwd_ex(tok, dy, V, 1, p, word_p, snap, dw=base.clone())
        assert torch.equal(bits(fwd_ex(w, tok, p, word_p, snap)), bits(ref_out))
        assert torch.equal(bits(bwd_ex(tok, dy, V, 0, p, word_p, snap)), bits(ref0))
        assert torch.equal(bits(bwd_ex(tok, dy, V, 1, p, word_p, snap, dw=base.clone())), bits(ref1))
        for by in (1, 2, 3):
            out = off(torch.zeros_like(ref_out), by)
            assert torch.equal(bits(fwd_ex(off(w, by), tok, p, word_p, snap, out=out)), bits(ref_out)), (p, word_p, by)
            assert torch.equal(bits(bwd_ex(tok, off(dy, by), V, 0, p, word_p, snap, dw=off(torch.zeros_like(base), 4 - by))), bits(ref0)), (p, word_p, by)
            assert torch.equal(bits(bwd_ex(tok, off(dy, 4 - by), V, 1, p, word_p, snap, dw=off(base, by))), bits(ref1)), (p, word_p, by)


# ---- 3. Model: tied against its untied twin -----------------------------------------------------------------------------------------------
T, B = 5, 3


def maker(V, H, dropout, embed_dropout=0.0, lstm_type="vmlmf"):
    def make():
        torch.manual_seed(5)
        r = 8 if H < 100 else 32
        return Model(V, H, 2, dropout, 0.08, w_rank=r, u_ranks=[r], lstm_type=lstm_type, embed_dropout=embed_dropout)
    return make


def text(V, seed=4):
    r = np.random.Generator(np.random.PCG64(seed))
    return dev(r.integers(0, V, size=(T, B))), dev(r.integers(0, V, size=(T, B)))


LOSSES = {
    "loss": lambda m, x, y, t, n: m.loss(x, y, m.state_init(B))[0],
    "ar_tar": lambda m, x, y, t, n: m.loss(x, y, m.state_init(B), ar=2.0, tar=1.0)[0],
    "lengths_z": lambda m, x, y, t, n: m.loss(x, y, m.state_init(B), lengths=n, z_loss=1e-3)[0],
    "distill": lambda m, x, y, t, n: m.distill_loss(x, y, m.state_init(B), t)[0],
    "distill_alpha0": lambda m, x, y, t, n: m.distill_loss(x, y, m.state_init(B), t, alpha=0.0)[0],      # (lm_head_loss's launches)
}


@pytest.mark.parametrize("dropout", [0.0, 0.5], ids=["p0", "p0.5"])
@pytest.mark.parametrize("V,H", [(12, 32), (96, 650)], ids=["12x32", "96x650"])
def test_a_tied_model_has_its_untied_twins_summed_gradient_to_the_bit(V, H, dropout):
    tied, twin = C.twins(maker(V, H, dropout), DEV)
    tied.train(), twin.train()
    x, y = text(V)
    torch.manual_seed(8)
    teacher, lengths = torch.randn(T, B, V, device=DEV), torch.tensor([T, 2, T + 3], device=DEV)
    for which, fn in LOSSES.items():
        tied.zero_grad(), twin.zero_grad()
        tied.dropout_state(seed=C.SEED), twin.dropout_state(seed=C.SEED)
        a, b = fn(tied, x, y, teacher, lengths), fn(twin, x, y, teacher, lengths)
        assert torch.equal(bits(a.detach()), bits(b.detach())), which
        a.backward(unit_gradient(a.device))
        b.backward(unit_gradient(b.device))
        assert torch.equal(tied.embed.w.grad, twin.embed.w.grad + twin.fc.w.grad), which
        pa, pb = dict(tied.named_parameters()), dict(twin.named_parameters())
        for name in pa:
            if name != "embed.w":
                assert torch.equal(bits(pa[name].grad), bits(pb[name].grad)), (which, name)
        # a foreign upstream gradient: the head's scaling lands in the tied gradient too
        tied.zero_grad(), twin.zero_grad()
        tied.dropout_state(seed=C.SEED), twin.dropout_state(seed=C.SEED)
        (fn(tied, x, y, teacher, lengths) * 0.5).backward()
        (fn(twin, x, y, teacher, lengths) * 0.5).backward()
        assert torch.equal(tied.embed.w.grad, twin.embed.w.grad + twin.fc.w.grad), which


# ---- 4. the fused route ---------------------------------------------------------------------------------------------------------------------
def test_a_tied_step_takes_the_accumulating_entry_once_and_keeps_the_heads_tensor():
    V, H = 96, 32
    tied, _ = C.twins(maker(V, H, 0.5), DEV)
    tied.train()
    x, y = text(V)
    tied.loss(x, y, tied.state_init(B))[0].backward()            # the forms of this shape are chosen
    tied.zero_grad(set_to_none=True)
    lib = _lib.lib()
    calls, made = [], []
    real = lib.vmlmf_embed_backward_ex
    olds = lib.vmlmf_embed_backward, lib.vmlmf_embed_dropout_backward, lib.vmlmf_embed_dropout_forward_ex

    def spy(*a):
        calls.append(a)
        return real(*a)

    def trip(*a):
        raise AssertionError("an embedding-backward entry of the untied path was called")
    forms = F.head_forms(T * B, H, V, tied.embed.w.device)
    form = forms["dw"]

    def dw_form(dz, h):
        out = form[2](dz, h)
        made.append(out.data_ptr())
        return out
    lib.vmlmf_embed_backward_ex, lib.vmlmf_embed_backward, lib.vmlmf_embed_dropout_backward = spy, trip, trip
    forms["dw"] = (form[0], form[1], dw_form, form[3])
    try:
        tied.loss(x, y, tied.state_init(B))[0].backward(unit_gradient(tied.embed.w.device))
    finally:
        forms["dw"] = form
        lib.vmlmf_embed_backward_ex, lib.vmlmf_embed_backward, lib.vmlmf_embed_dropout_backward = real, olds[0], olds[1]
    assert len(calls) == 1 and calls[0][6] == 1 and calls[0][:3] == (T * B, H, V)
    assert len(made) == 1 and tied.fc.w.grad is tied.embed.w.grad
    assert tied.fc.w.grad.data_ptr() == made[0]                  # no copy and no second (V, H) buffer: .grad IS the head product's tensor
    # an untied model: the old entries, launch for launch
    plain = maker(V, H, 0.5)().to(DEV).train()
    lib.vmlmf_embed_backward_ex = lib.vmlmf_embed_dropout_forward_ex = trip
    try:
        plain.loss(x, y, plain.state_init(B))[0].backward()
        plain.eval()
        plain.loss(x, y, plain.state_init(B))[0].backward()
    finally:
        lib.vmlmf_embed_backward_ex, lib.vmlmf_embed_dropout_forward_ex = real, olds[2]


# ---- 5. embed_dropout against the stock formulation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dropout", [0.0, 0.5], ids=["p0", "p0.5"])
def test_embed_dropout_against_the_stock_formulation_in_fp64_on_the_kernels_factors(dropout):
    V, H = 24, 32
    m = maker(V, H, dropout, embed_dropout=0.5, lstm_type="custom")().to(DEV).train()
    x, y = text(V, 6)
    m.dropout_state(seed=C.SEED)
    loss, _ = m.loss(x, y, m.state_init(B))
    loss.backward(unit_gradient(loss.device))
    # the same step in stock ops, fp64, on the factors the kernels drew from the snapshot (seed, 0)
    snap = snapshot(0)
    fw = vmlmf_amd.word_dropout_factors(V, 0.5, snap).double()
    assert bool((fw == 0).any()) and bool((fw == 2).any())
    ref = copy.deepcopy(m).double()
    ref.zero_grad()

    def factors(site):
        return (F.dropout_factors(T * B, H, dropout, snap, site) if dropout > 0 else torch.ones(T * B, H, device=DEV)).view(T, B, H).double()
    h = (ref.embed.w[x] * fw[x][..., None]) * factors(0)
    states = [(a.double(), b.double()) for a, b in ref.state_init(B)]
    for i, rnn in enumerate(ref.rnns):
        h, states[i] = rnn(h, states[i])
        h = h * factors(i + 1)
    want = vmlmf_amd.nll_loss(torch.addmm(ref.fc.b, h.reshape(-1, H), ref.fc.w.t()), y)
    want.backward()
    assert float(loss.detach()) == pytest.approx(float(want.detach()), rel=1e-5)
    for (name, p), q in zip(m.named_parameters(), ref.parameters()):
        assert_grad(p.grad.cpu().numpy(), q.grad.cpu().numpy(), name)
    dropped = (fw == 0).nonzero().flatten()
    hit = torch.bincount(x.flatten(), minlength=V) > 0
    assert bool((m.embed.w.grad[dropped] == 0).all()) and bool((m.embed.w.grad[hit & (fw != 0)] != 0).any())
    # a second call draws another word mask; eval() is the model without it, to the bit
    assert not torch.equal(vmlmf_amd.word_dropout_factors(V, 0.5, snapshot(1)), fw.float())
    again, _ = m.loss(x, y, m.state_init(B))
    assert m.dropout_state().tolist() == [C.SEED, 2] and not torch.equal(again.detach(), loss.detach())
    plain = maker(V, H, dropout, lstm_type="custom")().to(DEV)
    plain.load_state_dict(m.state_dict())
    m.eval(), plain.eval()
    with torch.no_grad():
        assert torch.equal(bits(m.loss(x, y, m.state_init(B))[0]), bits(plain.loss(x, y, plain.state_init(B))[0]))
        assert torch.equal(bits(m(x, m.state_init(B))[0]), bits(plain(x, plain.state_init(B))[0]))
    assert m.dropout_state().tolist() == [C.SEED, 2]                    # eval mode draws nothing


# ---- 6. a captured step ---------------------------------------------------------------------------------------------------------------------
def test_a_captured_tied_step_with_both_dropouts_reproduces_the_eager_bits():
    V, H = 96, 32
    m = maker(V, H, 0.5, embed_dropout=0.5)().to(DEV).train()
    m.tie_weights()
    x, y = text(V)
    state = m.dropout_state(seed=C.SEED)

    class Feed(torch.nn.Module):          # GraphedTrainStep calls criterion(model(x), target): the LM's loss needs both
        def __init__(self, net):
            super().__init__()
            self.net = net

        def forward(self, x):
            return x

    def criterion(x, t):
        return m.loss(x, t, m.state_init(B))[0]
    step = vmlmf_amd.GraphedTrainStep(Feed(m), criterion, optim.Adam(m.parameters(), lr=0.0), x, y, warmup=1)      # lr 0: only the masks move
    replays = []
    for _ in range(2):
        before = state.clone()
        loss = step(x, y)
        torch.cuda.synchronize()
        assert state.tolist() == [C.SEED, int(before[1]) + 1]
        value, grad = loss.clone(), m.embed.w.grad.clone()
        assert m.fc.w.grad is m.embed.w.grad
        state.copy_(before)                                        # the eager call from the same state
        eager = m.loss(x, y, m.state_init(B))[0]
        (g,) = torch.autograd.grad(eager, m.embed.w, unit_gradient(eager.device))
        assert torch.equal(bits(value), bits(eager.detach())) and torch.equal(bits(grad), bits(g))
        replays.append((value, grad))
    assert not torch.equal(replays[0][0], replays[1][0]) and not torch.equal(replays[0][1], replays[1][1])


# ---- 7. decoding, scoring and the optimizers on a tied model ----------------------------------------------------------------------------------
def test_decoding_scoring_and_the_optimizers_on_a_tied_model():
    V, H = 96, 32
    tied, twin = C.twins(maker(V, H, 0.0), DEV)
    tied.eval(), twin.eval()
    x, y = text(V)
    prompt = x[:3]
    with torch.no_grad():
        a, b = tied.generate(prompt, 6, temperature=0), twin.generate(prompt, 6, temperature=0)
        assert all(torch.equal(u, v) for u, v in zip(a[:2], b[:2]))
        a, b = tied.beam_search(prompt, 5, beams=3), twin.beam_search(prompt, 5, beams=3)
        assert all(torch.equal(u, v) for u, v in zip(a[:2], b[:2]))
        a, b = tied.score(x, y), twin.score(x, y)
        assert torch.equal(bits(a[0]), bits(b[0]))
    # one step of each optimizer moves the table once: by the twin's summed gradient
    for kind in ("sgd", "adam", "asgd"):
        tied, twin = C.twins(maker(V, H, 0.0), DEV)
        tied.train(), twin.train()
        params = list(tied.parameters())
        assert sum(p is tied.embed.w for p in params) == 1
        opt = {"sgd": None, "adam": optim.Adam(params, lr=0.01), "asgd": optim.ASGD(params, lr=0.5)}[kind]
        tied.loss(x, y, tied.state_init(B))[0].backward(unit_gradient(DEV))
        twin.loss(x, y, twin.state_init(B))[0].backward(unit_gradient(DEV))
        g = twin.embed.w.grad + twin.fc.w.grad
        assert torch.equal(tied.embed.w.grad, g)
        before = tied.embed.w.detach().clone()
        if kind == "sgd":
            optim.clip_sgd_step(params, 0.5, 1e9)
            assert torch.allclose(tied.embed.w.detach(), before - 0.5 * g, rtol=1e-6, atol=1e-7)
        else:
            opt.step()
            if kind == "asgd":
                assert torch.allclose(tied.embed.w.detach(), before - 0.5 * g, rtol=1e-6, atol=1e-7)
            else:
                moved = (tied.embed.w.detach() - before).abs()
                assert float(moved.max()) <= 0.01 * 1.001 and float(moved.max()) > 0.005          # Adam's first step: lr sign(g), once
        assert tied.tied and torch.equal(tied.fc.w, tied.embed.w)
    # ASGD's averaged() and dynamic evaluation put a tied model's bits back
    tied, _ = C.twins(maker(V, H, 0.0), DEV)
    tied.train()
    opt = optim.ASGD(tied.parameters(), lr=0.5)
    opt.start_averaging()
    for _ in range(3):                                     # (the average differs from the iterate from the third step on)
        tied.zero_grad()
        tied.loss(x, y, tied.state_init(B))[0].backward(unit_gradient(DEV))
        opt.step()
    iterate = {k: v.clone() for k, v in tied.state_dict().items()}
    with opt.averaged():
        assert tied.tied and not torch.equal(tied.embed.w, iterate["embed.w"])
    assert tied.tied and all(torch.equal(bits(v), bits(iterate[k])) for k, v in tied.state_dict().items())
    de = vmlmf_amd.DynamicEval(tied, lr=0.1, decay=0.01, segment=3)
    de.accumulate(x, y)
    de.finalize()
    with torch.no_grad():
        want = tied.score(x, y)[0][:3]
    got, _ = de.score(x, y)
    assert torch.allclose(got[:3], want, rtol=1e-5, atol=1e-6)                # the first segment is scored before any adaptation
    assert not torch.equal(tied.embed.w, iterate["embed.w"])
    de.restore()
    assert tied.tied and all(torch.equal(bits(v), bits(iterate[k])) for k, v in tied.state_dict().items())
