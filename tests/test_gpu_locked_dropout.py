"""GPU: locked (variational) dropout with a rate per site (docs/design/lm_locked.md).  The oracle is the project's own: the numpy
Philox restatement evaluated at position b (locked_cases.py).  The chain follows tests/test_dropout.py: (1) the factors the library
draws equal the restatement bit for bit - the flat launch, with a row-block layer's column map, at both offsets; (2) every place that
applies them - the stand-alone launch, the embedding gather and the table gradient, one row-block layer, the clustered stack, the
wavefront stacks, the AR / TAR pair, the whole Model - equals its CPU restatement with THOSE factors multiplied in, at the tolerances
the per-element tests of the same kernels use, and to the bit where those demand bits; (3) a captured step draws a fresh mask on
every replay.  The flat entries refuse the flag."""
import ctypes

import numpy as np
import pytest
import torch

import actreg_cases as A
import locked_cases as C
import tied_cases as TC
import vmlmf_oracle as O
from hip_util import ORDER, assert_grad, assert_out
from test_gpu_rbx import _compare, _inputs, _run_oracle, _run_stack
import vmlmf_amd
from vmlmf_amd import Model, _lib, unit_gradient
from vmlmf_amd import functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0x7FC12345          # a NaN with a payload: a row that was rewritten, even with itself plus zero, loses these bits


def snapshot(offset=7):
    return torch.tensor([C.SEED, offset], dtype=torch.int64, device=DEV)


def dev(a, dtype=None):
    return torch.as_tensor(a, dtype=dtype).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def off(t, by):
    """The same values in a contiguous view that starts `by` floats behind an aligned allocation."""
    flat = torch.empty(t.numel() + by, device=DEV)
    view = flat[by:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == (4 * by) % 16
    return view


def rb_desc(variant, B, T, H=650):
    g, ru = (2, [32, 32]) if variant == O.V4 else (1, [32])
    desc = _lib.make_desc(variant, B, T, H, H, 32, ru, g=g, time_major=True, training=True)
    assert _lib.lib().vmlmf_dropout_fused(ctypes.byref(desc)) == 1
    Hg = H // g
    return desc, g, ru, dict(Hg=Hg, gstride=64 * ((Hg + 63) // 64))


# ---- 1. the factors ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.FACTOR_SHAPES, ids=C.FACTOR_IDS)
def test_locked_factors_from_the_library_equal_the_restatement(shape):
    T, B, H = shape
    for offset in C.OFFSETS:
        for p, site in ((0.5, 0), (0.25, 3)):
            got = F.dropout_factors(T * B, H, p, snapshot(offset), site, locked_batch=B).cpu().numpy()
            assert np.array_equal(got, C.locked_factors(C.SEED, offset, site, T, B, H, p).reshape(T * B, H)), (offset, p, site)
    # not the per-element factors of the same site
    assert not np.array_equal(got, F.dropout_factors(T * B, H, 0.25, snapshot(offset), 3).cpu().numpy()) or T * B * H < 16


@pytest.mark.parametrize("variant", [O.V4, O.V3], ids=["group", "plain"])
def test_locked_factors_of_a_row_block_layer_use_its_thread_slots_as_columns(variant):
    B, T, H = 21, 3, 650
    desc, g, ru, cols = rb_desc(variant, B, T)
    for offset in C.OFFSETS:
        got = F.dropout_factors(T * B, H, 0.5, snapshot(offset), 2, layer_desc=desc, locked_batch=B).cpu().numpy()
        assert np.array_equal(got, C.locked_factors(C.SEED, offset, 2, T, B, H, 0.5, **cols).reshape(T * B, H))
    if g == 2:
        assert not np.array_equal(got, C.locked_factors(C.SEED, offset, 2, T, B, H, 0.5).reshape(T * B, H))


def test_the_flat_entries_refuse_the_flag_and_the_locked_ones_a_ragged_grid():
    lib = _lib.lib()
    T, B, H, V = 4, 2, 8, 5
    R = T * B
    snap = snapshot()
    x, w = torch.randn(R, H, device=DEV), torch.randn(V, H, device=DEV)
    stream = _lib.raw_stream(x.device)
    tok = torch.randint(0, V, (R,), device=DEV)
    nbytes = lib.vmlmf_embed_backward_scratch_bytes(R, V)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    flagged = 1 + _lib.SITE_LOCKED

    def poisoned(*shape):
        t = torch.empty(shape, device=DEV)
        bits(t)[:] = POISON
        return t
    y, yw = poisoned(R, H), poisoned(V, H)
    p_ = _lib.ptr
    flat = [
        lambda s: lib.vmlmf_dropout_apply(R, H, p_(x), p_(y), 0.5, p_(snap), s, stream),
        lambda s: lib.vmlmf_dropout_factors(None, R, H, 0.5, p_(snap), s, p_(y), stream),
        lambda s: lib.vmlmf_embed_dropout_forward(R, H, V, p_(tok), p_(w), p_(y), 0.5, p_(snap), s, stream),
        lambda s: lib.vmlmf_embed_dropout_backward(R, H, V, p_(tok), p_(x), p_(yw), scratch.data_ptr(), nbytes, 0.5, p_(snap), s, stream),
        lambda s: lib.vmlmf_embed_dropout_forward_ex(R, H, V, p_(tok), p_(w), p_(y), 0.5, 0.0, p_(snap), s, stream),
        lambda s: lib.vmlmf_embed_backward_ex(R, H, V, p_(tok), p_(x), p_(yw), 0, scratch.data_ptr(), nbytes, 0.5, 0.0, p_(snap), s, stream),
    ]
    for call in flat:
        assert call(flagged) == _lib.E_BADARG
    # R = 7 rows are no (T, 2) grid; B < 1
    for Rb, Bb in ((R - 1, B), (R, 0), (R, -2)):
        assert lib.vmlmf_dropout_apply_locked(Rb, Bb, H, p_(x), p_(y), 0.5, p_(snap), 1, stream) == _lib.E_BADARG
        assert lib.vmlmf_dropout_factors_locked(None, Rb, Bb, H, 0.5, p_(snap), 1, p_(y), stream) == _lib.E_BADARG
        assert lib.vmlmf_embed_dropout_forward_lk(Rb, Bb, H, V, p_(tok), p_(w), p_(y), 0.5, 0.0, p_(snap), 0, stream) == _lib.E_BADARG
        assert lib.vmlmf_embed_backward_lk(Rb, Bb, H, V, p_(tok), p_(x), p_(yw), 0, scratch.data_ptr(), nbytes, 0.5, 0.0, p_(snap), 0,
                                           stream) == _lib.E_BADARG
    torch.cuda.synchronize()
    assert bool((bits(y) == POISON).all()) and bool((bits(yw) == POISON).all())         # nothing was launched
    for call in flat:                                                                       # ... and the plain site is taken as before
        assert call(1) == 0
    # the locked entries set the flag themselves: with or without it in the site, the same factors
    a, b = torch.empty(R, H, device=DEV), torch.empty(R, H, device=DEV)
    assert lib.vmlmf_dropout_factors_locked(None, R, B, H, 0.5, p_(snap), 1, p_(a), stream) == 0
    assert lib.vmlmf_dropout_factors_locked(None, R, B, H, 0.5, p_(snap), flagged, p_(b), stream) == 0
    assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), C.locked_factors(C.SEED, 7, 1, T, B, H, 0.5).reshape(R, H))


# ---- 2. the stand-alone launch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by", [0, 1], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("shape", C.FACTOR_SHAPES + [(5, 3, 8)], ids=C.FACTOR_IDS + ["5x3x8"])
def test_stand_alone_locked_dropout_forward_and_backward(shape, by):
    T, B, H = shape
    r = np.random.Generator(np.random.PCG64(3))
    x = r.standard_normal(shape).astype(np.float32)
    dy = r.standard_normal(shape).astype(np.float32)
    for offset, p in zip(C.OFFSETS, (0.5, 0.25)):
        snap = snapshot(offset)
        xt = off(dev(x), by).requires_grad_(True)
        y = F.dropout(xt, p, snap, 1, locked=True)
        (grad,) = torch.autograd.grad(y, xt, off(dev(dy), by))
        f = C.locked_factors(C.SEED, offset, 1, T, B, H, p)
        assert np.array_equal(y.detach().cpu().numpy(), x * f)
        assert np.array_equal(grad.cpu().numpy(), dy * f)
        assert C.zero_pattern_is_locked(y.detach().cpu().numpy())
    assert F.dropout(xt, 0.0, snap, 1, locked=True) is xt


# ---- 3. the embedding: gather and table gradient -----------------------------------------------------------------------------------
def fwd_lk(w, tok, B, p, word_p, snap):
    V, H = w.shape
    out = torch.empty((tok.numel(), H), device=DEV)
    _lib.check(_lib.lib().vmlmf_embed_dropout_forward_lk(tok.numel(), B, H, V, _lib.ptr(tok), _lib.ptr(w), _lib.ptr(out), p, word_p, _lib.ptr(snap), 0,
                                                         _lib.raw_stream(w.device)))
    return out


def bwd_lk(tok, dy, B, V, accumulate, p, word_p, snap, dw=None):
    R, H = dy.shape
    lib = _lib.lib()
    nbytes = lib.vmlmf_embed_backward_scratch_bytes(R, V)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    dw = torch.full((V, H), float("nan"), device=DEV) if dw is None else dw
    _lib.check(lib.vmlmf_embed_backward_lk(R, B, H, V, _lib.ptr(tok), _lib.ptr(dy), _lib.ptr(dw), accumulate, scratch.data_ptr(), nbytes, p, word_p,
                                           _lib.ptr(snap), 0, _lib.raw_stream(dy.device)))
    return dw


@pytest.mark.parametrize("shape", C.EMBED_SHAPES, ids=C.EMBED_IDS)
def test_the_embedding_under_locked_input_dropout(shape):
    T, B, V, H = shape
    R, p = T * B, 0.5
    w_np, dy_np, base_np = TC.draw(R, V, H, 23)
    tok2 = C.repeating_tokens(T, B, V, seed=H)
    tok_np = tok2.reshape(-1)
    w, dy, tok = dev(w_np), dev(dy_np), dev(tok_np)
    hit = torch.bincount(tok, minlength=V) > 0
    for k, word_p in enumerate((0.0, 0.5)):
        offset = C.OFFSETS[k]
        snap = snapshot(offset)
        what = f"{shape} word_p={word_p}"
        f_np = C.locked_factors(C.SEED, offset, 0, T, B, H, p).reshape(R, H)
        fw_np = TC.word_factors(V, word_p, offset, seed=C.SEED)
        assert TC.same_bits(F.dropout_factors(R, H, p, snap, 0, locked_batch=B).cpu().numpy(), f_np), what
        assert TC.same_bits(vmlmf_amd.word_dropout_factors(V, word_p, snap).cpu().numpy(), fw_np), what
        # the same word under the same row mask at every step of row 0, under different row masks across step 0
        assert np.array_equal(f_np.reshape(T, B, H)[0, 0], f_np.reshape(T, B, H)[-1, 0])
        assert B == 1 or not np.array_equal(f_np.reshape(T, B, H)[0, 0], f_np.reshape(T, B, H)[0, 1])
        # the gather: two single-rounded multiplications, the word factor first
        out = fwd_lk(w, tok, B, p, word_p, snap)
        assert torch.equal(out, dev(TC.forward(w_np, tok_np, f_np, fw_np))), what      # (a dropped word's zeros carry no sign)
        assert torch.equal(out, (w[tok] * dev(fw_np)[tok, None]) * dev(f_np)), what
        kept = dev(fw_np) != 0
        rows = hit & kept
        # accumulate == 0
        got = bwd_lk(tok, dy, B, V, 0, p, word_p, snap)
        assert TC.same_bits(got.cpu().numpy(), TC.table_gradient(tok_np, dy_np, f_np, fw_np, V)), what
        assert bool((got[~rows] == 0).all()), what
        worst = TC.excess(got.cpu().numpy(), tok_np, dy_np, f_np, fw_np, V)
        assert worst <= 1.0, (what, worst)
        # accumulate == 1: rows that are not hit-and-kept are poisoned and keep their bits
        base = dev(base_np).clone()
        bits(base)[~rows] = POISON
        acc = bwd_lk(tok, dy, B, V, 1, p, word_p, snap, dw=base.clone())
        assert torch.equal(bits(acc[~rows]), bits(base[~rows])), what
        assert TC.same_bits(acc.cpu().numpy(), TC.table_gradient(tok_np, dy_np, f_np, fw_np, V, base=base.cpu().numpy())), what
        # through functional.embedding_dropout: the same bits in both directions
        wt = w.clone().requires_grad_(True)
        o2 = F.embedding_dropout(wt, dev(tok2), p, snap, 0, word_p=word_p, locked=True)
        assert o2.shape == (T, B, H) and torch.equal(bits(o2.detach().view(R, H)), bits(out)), what
        (gw,) = torch.autograd.grad(o2, wt, dy.view(T, B, H))
        assert torch.equal(bits(gw), bits(got)), what
        # ... and with the head's gradient handed over, the accumulating form
        holder = F.TiedGradient()
        holder.put(base.clone())
        o3 = F.embedding_dropout(wt, dev(tok2), p, snap, 0, word_p=word_p, grad_from=holder, locked=True)
        (gt,) = torch.autograd.grad(o3, wt, dy.view(T, B, H))
        assert torch.equal(bits(gt), bits(acc)), what


# ---- 4. one row-block layer --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", C.LAYER_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("variant", [O.V3, O.V4], ids=["plain", "group"])
def test_one_row_block_layer_with_a_locked_mask_inside_its_launches(variant, B, T):
    """y_dropped IS (the same layer's y) * F to the bit; the gradients against the literal fp64 restatement with F multiplied in."""
    H, rw, p = 650, 32, 0.4
    desc, g, ru, cols = rb_desc(variant, B, T)
    P = O.make_params(variant, H, H, rw, ru if g == 2 else ru[0], seed=31, scale=0.05)
    r = np.random.Generator(np.random.PCG64(8 + B))
    x = (0.5 * r.standard_normal((T, B, H))).astype(np.float32)
    h0 = (0.3 * r.standard_normal((B, H))).astype(np.float32)
    c0 = (0.3 * r.standard_normal((B, H))).astype(np.float32)
    dy, dhT, dcT = (r.standard_normal(s).astype(np.float32) for s in ((T, B, H), (B, H), (B, H)))
    snap = snapshot(11)
    Fd = F.dropout_factors(T * B, H, p, snap, 2, layer_desc=desc, locked_batch=B).view(T, B, H)
    Fn = C.locked_factors(C.SEED, 11, 2, T, B, H, p, **cols)
    assert np.array_equal(Fd.cpu().numpy(), Fn)
    names = ORDER[variant]

    def run(drop, upstream):
        params = [dev(np.asarray(P[k])).requires_grad_(True) for k in names]
        xg, h0g, c0g = (dev(a).requires_grad_(True) for a in (x, h0, c0))
        y, hT, cT = vmlmf_amd.vmlmf_sequence(variant, xg, h0g, c0g, params, rw, ru, g=g, time_major=True, drop=drop)
        ((y * upstream).sum() + (hT * dev(dhT)).sum() + (cT * dev(dcT)).sum()).backward()
        return y.detach(), hT.detach(), cT.detach(), [xg.grad, h0g.grad, c0g.grad] + [q.grad for q in params]

    yd, hT, cT, grads = run((p, snap, 2, True), dev(dy))
    y, hTu, cTu, _ = run(None, dev(dy) * Fd)
    assert torch.equal(yd, y * Fd) and torch.equal(hT, hTu) and torch.equal(cT, cTu)
    assert C.zero_pattern_is_locked(yd.cpu().numpy())
    # the oracle
    f64 = torch.float64
    Pt = O.to_torch(P, dtype=f64, requires_grad=True)
    xt, h0t, c0t = (torch.tensor(a, dtype=f64, requires_grad=True) for a in (x, h0, c0))
    yr, hTr, cTr = O.literal_sequence(variant, Pt, xt, h0t, c0t, time_major=True, v4_scratch_rows=B)
    ydr = yr * torch.tensor(Fn, dtype=f64)
    ((ydr * torch.tensor(dy, dtype=f64)).sum() + (hTr * torch.tensor(dhT, dtype=f64)).sum() + (cTr * torch.tensor(dcT, dtype=f64)).sum()).backward()
    assert_out(yd.cpu().numpy(), ydr.detach().numpy(), "y_dropped")
    assert_out(hT.cpu().numpy(), hTr.detach().numpy(), "hT")
    assert_out(cT.cpu().numpy(), cTr.detach().numpy(), "cT")
    for got, ref, k in zip(grads, [xt.grad, h0t.grad, c0t.grad] + [Pt[k].grad for k in names], ["dx", "dh0", "dc0"] + list(names)):
        assert_grad(got.cpu().numpy(), ref.numpy(), k)


# ---- 5. the clustered two-layer PTB stack ------------------------------------------------------------------------------------------
def test_the_clustered_stack_with_a_locked_mask_and_a_rate_per_site():
    variant, H, L, B, T = O.V4, 650, 2, 7, 2          # (the smallest co-resident batch of tests/test_gpu_rbx.py)
    desc, g, ru, cols = rb_desc(variant, B, T)
    cfg = (variant, g, 32, tuple(ru), True, _lib.DT_F32)
    assert F._stack_plan(cfg, L, B, T, H, H, True) is not None and F.stack_takes_dropout(cfg, L, B, T, H, H, True)
    Ps = [O.make_params(variant, H, H, 32, ru, seed=61 + l, scale=0.05) for l in range(L)]
    inp = _inputs(17, L, B, T, H)
    snap = snapshot(5)
    rates = (0.4, 0.25)
    got = _run_stack(variant, Ps, *inp, drops=[(rates[l], snap, l + 1, True) for l in range(L)])
    Fs = [C.locked_factors(C.SEED, 5, l + 1, T, B, H, rates[l], **cols) for l in range(L)]
    for l in range(L):
        assert np.array_equal(F.dropout_factors(T * B, H, rates[l], snap, l + 1, layer_desc=desc, locked_batch=B).cpu().numpy().reshape(T, B, H), Fs[l])
    assert C.zero_pattern_is_locked(got["y"]) and np.array_equal(got["y"] == 0, Fs[1] == 0)
    _compare(got, _run_oracle(variant, Ps, *inp, factors=Fs), "rbx.locked")


# ---- 6. the wavefront stacks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,B,T,H,rw,ru", C.WAVE_CASES, ids=lambda v: str(v))
def test_wavefront_stacks_with_a_locked_mask_and_a_rate_per_site(L, B, T, H, rw, ru):
    """A different rate behind every layer; with three layers the middle site has rate 0 (no dropout there) between two live ones."""
    variant = O.V3
    cfg = (variant, 1, rw, (ru,), True, _lib.DT_F32)
    assert F._stack_plan(cfg, L, B, T, H, H, True) is not None and F.stack_takes_dropout(cfg, L, B, T, H, H, True)
    rates = (0.5, 0.25) if L == 2 else (0.5, 0.0, 0.25)
    Ps = [O.make_params(variant, H, H, rw, ru, seed=71 + l, scale=0.1) for l in range(L)]
    r = np.random.Generator(np.random.PCG64(12))
    x = (0.5 * r.standard_normal((T, B, H))).astype(np.float32)
    h0 = (0.3 * r.standard_normal((L, B, H))).astype(np.float32)
    c0 = (0.3 * r.standard_normal((L, B, H))).astype(np.float32)
    dy = r.standard_normal((T, B, H)).astype(np.float32)
    dhT = r.standard_normal((L, B, H)).astype(np.float32)
    dcT = r.standard_normal((L, B, H)).astype(np.float32)
    snap = snapshot(23)
    names = ORDER[variant]
    params = [[dev(np.asarray(P[k])).requires_grad_(True) for k in names] for P in Ps]
    xg, h0g, c0g = (dev(a).requires_grad_(True) for a in (x, h0, c0))
    drops = [(rates[l], snap, l + 1, True) if rates[l] > 0 else None for l in range(L)]
    out = F.vmlmf_stack(variant, xg, params, rw, [ru], g=1, time_major=True, h0=h0g, c0=c0g, drops=drops)
    assert out is not None
    yd, hs, cs = out
    loss = (yd * dev(dy)).sum()
    for l in range(L):
        loss = loss + (hs[l] * dev(dhT[l])).sum() + (cs[l] * dev(dcT[l])).sum()
    loss.backward()
    Fs = [C.locked_factors(C.SEED, 23, l + 1, T, B, H, rates[l]) for l in range(L)]
    f64 = torch.float64
    Pt = [O.to_torch(P, dtype=f64, requires_grad=True) for P in Ps]
    xt, h0t, c0t = (torch.tensor(a, dtype=f64, requires_grad=True) for a in (x, h0, c0))
    cur, lossr, hr, cr = xt, 0.0, [], []
    for l in range(L):
        cur, hT, cT = O.literal_sequence(variant, Pt[l], cur, h0t[l], c0t[l], time_major=True)
        cur = cur * torch.tensor(Fs[l], dtype=f64)
        hr.append(hT), cr.append(cT)
        lossr = lossr + (hT * torch.tensor(dhT[l], dtype=f64)).sum() + (cT * torch.tensor(dcT[l], dtype=f64)).sum()
    (lossr + (cur * torch.tensor(dy, dtype=f64)).sum()).backward()
    got = yd.detach().cpu().numpy()
    assert np.array_equal(got == 0, Fs[-1] == 0) and C.zero_pattern_is_locked(got)
    assert_out(got, cur.detach().numpy(), "wf.locked.y_dropped")
    for l in range(L):
        assert_out(hs[l].detach().cpu().numpy(), hr[l].detach().numpy(), f"wf.locked.hT[{l}]")
        assert_out(cs[l].detach().cpu().numpy(), cr[l].detach().numpy(), f"wf.locked.cT[{l}]")
    assert_grad(xg.grad.cpu().numpy(), xt.grad.numpy(), "wf.locked.dx")
    assert_grad(h0g.grad.cpu().numpy(), h0t.grad.numpy(), "wf.locked.dh0")
    assert_grad(c0g.grad.cpu().numpy(), c0t.grad.numpy(), "wf.locked.dc0")
    for l in range(L):
        for k, p_ in zip(names, params[l]):
            assert_grad(p_.grad.cpu().numpy(), Pt[l][k].grad.numpy(), f"wf.locked.layer{l}.{k}")


def test_a_stack_of_unequal_hidden_sizes_leaves_its_dropout_to_the_layers():
    """hidden_layer_sizes that differ: functional.vmlmf_stack runs such a stack only without dropout (and without carried states),
    before and after this change - with drop tuples of either form it answers None and the caller chains the layers, whose own
    launches (or the stand-alone one) apply the locked mask: test 4 and test 2."""
    variant, B, T, I, Hs, rw, ru = O.V1, 4, 3, 8, (16, 24), 4, 4
    Ps = [O.make_params(variant, I if l == 0 else Hs[l - 1], Hs[l], rw, ru, seed=5 + l) for l in range(2)]
    params = [[dev(np.asarray(P[k])).requires_grad_(True) for k in ORDER[variant]] for P in Ps]
    x = torch.randn(B, T, I, device=DEV)
    snap = snapshot()
    for drops in ([(0.5, snap, 1, True), (0.25, snap, 2, True)], [(0.5, snap, 1), (0.25, snap, 2)]):
        assert F.vmlmf_stack(variant, x, params, rw, [ru], g=1, time_major=False, drops=drops) is None


@pytest.mark.parametrize("time_major", [True, False], ids=["time_major", "batch_first"])
def test_chained_layers_of_unequal_hidden_sizes_with_a_locked_mask_behind_each(time_major):
    """What that fallback does: vmlmf_sequence per layer with (p, snapshot, site, True).  These layers are outside the fused
    envelope, so the locked mask is the stand-alone launch behind the layer - over time-major rows; a batch-first layer's output
    goes through it transposed - against the fp64 oracle with the restated (T, B, H) factors multiplied in."""
    variant, B, T, I, Hs, rw, ru = O.V1, 5, 6, 8, (16, 24), 4, 4
    rates, L = (0.5, 0.25), 2
    Ps = [O.make_params(variant, I if l == 0 else Hs[l - 1], Hs[l], rw, ru, seed=5 + l) for l in range(L)]
    names = ORDER[variant]
    params = [[dev(np.asarray(P[k])).requires_grad_(True) for k in names] for P in Ps]
    r = np.random.Generator(np.random.PCG64(14))
    shape = (lambda h: (T, B, h)) if time_major else (lambda h: (B, T, h))
    x = r.standard_normal(shape(I)).astype(np.float32)
    dy = r.standard_normal(shape(Hs[-1])).astype(np.float32)
    snap = snapshot(13)
    xg = dev(x).requires_grad_(True)
    cur = xg
    for l in range(L):
        cur, _, _ = vmlmf_amd.vmlmf_sequence(variant, cur, None, None, params[l], rw, [ru], g=1, time_major=time_major,
                                             drop=(rates[l], snap, l + 1, True))
    (cur * dev(dy)).sum().backward()
    f64 = torch.float64
    Pt = [O.to_torch(P, dtype=f64, requires_grad=True) for P in Ps]
    xt = torch.tensor(x, dtype=f64, requires_grad=True)
    ref = xt
    for l in range(L):
        ref, _, _ = O.literal_sequence(variant, Pt[l], ref, None, None, time_major=time_major)
        f = torch.tensor(C.locked_factors(C.SEED, 13, l + 1, T, B, Hs[l], rates[l]), dtype=f64)
        ref = ref * (f if time_major else f.transpose(0, 1))
    (ref * torch.tensor(dy, dtype=f64)).sum().backward()
    got = cur.detach().cpu().numpy()
    assert got.shape == shape(Hs[-1])
    assert C.zero_pattern_is_locked(got if time_major else got.transpose(1, 0, 2))
    assert_out(got, ref.detach().numpy(), "chained.y_dropped")
    assert_grad(xg.grad.cpu().numpy(), xt.grad.numpy(), "chained.dx")
    for l in range(L):
        for k, p_ in zip(names, params[l]):
            assert_grad(p_.grad.cpu().numpy(), Pt[l][k].grad.numpy(), f"chained.layer{l}.{k}")


# ---- 7. AR / TAR under a locked top site -------------------------------------------------------------------------------------------
def actreg_run(raw, g, ar, tar, p, snap, site, lengths, desc=None, s=None):
    x = dev(raw).requires_grad_(True)
    yd, penalty, parts = vmlmf_amd.activation_regularizer(x, ar=ar, tar=tar, p=p, snap=snap, site=site, lengths=lengths, layer_desc=desc)
    up = unit_gradient(x.device) if s is None else torch.tensor(s, device=DEV)
    (grad,) = torch.autograd.grad([yd, penalty], x, [dev(g), up])
    return yd.detach(), torch.stack([penalty.detach(), *parts]).cpu().numpy(), grad, x


def stock64(raw, g, f, ar, tar, lengths, s):
    x = dev(raw, torch.float64).requires_grad_(True)
    yd, penalty, parts = F.activation_regularizer_stock(x, ar=ar, tar=tar, factors=f.double(), lengths=lengths)
    outs, ups = [yd], [dev(g, torch.float64)]
    if penalty.requires_grad:
        outs, ups = outs + [penalty], ups + [torch.tensor(1.0 if s is None else float(np.float32(s)), dtype=torch.float64, device=DEV)]
    (grad,) = torch.autograd.grad(outs, x, ups)
    return np.array([float(penalty.detach()), float(parts[0]), float(parts[1])]), grad.cpu().numpy()


@pytest.mark.parametrize("H", C.ACTREG_H)
@pytest.mark.parametrize("T", C.ACTREG_T)
def test_ar_and_tar_under_a_locked_top_site(T, H):
    B, p = 3, 0.5
    raw, g = A.draw(T, B, H, 10 * T + H % 7)
    cut = np.array([T, max(T - 2, 0), min(2, T)])          # T = 9: 7 and 2 end inside a walk of four steps; T = 5: 3 does
    for masked in (False, True):
        lengths = cut if masked else None
        n = None if lengths is None else dev(lengths)
        for (ar, tar, s), offset in zip(((2.0, 1.0, None), (0.0, 1.0, 0.75), (2.0, 0.0, None)), (7, 2 ** 32 + 5, 7)):
            what = f"T {T} H {H} masked {masked} ar {ar} tar {tar} s {s}"
            snap = snapshot(offset)
            fn = C.locked_factors(C.SEED, offset, 2, T, B, H, p)
            f = F.dropout_factors(T * B, H, p, snap, 2, locked_batch=B).view(T, B, H)
            assert np.array_equal(f.cpu().numpy(), fn), what
            yd, stats, grad, x = actreg_run(raw, g, ar, tar, p, snap, F.locked_site(2), n, s=s)
            # the dropped copy has the stand-alone launch's bits, at every position
            assert torch.equal(bits(yd), bits(F.dropout(x.detach(), p, snap, 2, locked=True))), what
            assert np.array_equal(yd.cpu().numpy(), raw * fn), what
            want = A.oracle(raw, fn, lengths, ar, tar, g, s=1.0 if s is None else float(np.float32(s)))
            A.check_stats(stats, want, T, B, H, ar, tar, what)
            A.check_draw(grad.cpu().numpy(), want, what)
            # the stock formulation in fp64, fed the factor tensor
            sstats, sgrad = stock64(raw, g, f, ar, tar, n, s)
            assert np.all(np.abs(stats.astype(np.float64) - sstats) <= A.penalty_bound(T, B, H) * np.abs(sstats) + A.F32_TINY), (what, stats, sstats)
            err = np.abs(grad.cpu().numpy().astype(np.float64) - sgrad)
            assert np.all(err <= A.gamma(A.ROUNDINGS_DRAW) * want["magnitude"] + A.F32_TINY), (what, err.max())
            m, _ = A.masks(T, B, lengths)
            fg = F.dropout(dev(g), p, snap, 2, locked=True)
            assert torch.equal(grad[dev(~m)], fg[dev(~m)]), what
            # the per-element form of the same site draws other factors
            other = actreg_run(raw, g, ar, tar, p, snap, 2, n, s=s)[0]
            assert T * B * H < 64 or not torch.equal(other, yd), what


def test_ar_and_tar_with_a_layer_descriptor_under_a_locked_mask():
    T, B, H = 5, 2, 650
    desc, g_, ru, cols = rb_desc(O.V4, B, T)
    raw, g = A.draw(T, B, H, 21)
    snap = snapshot(3)
    fn = C.locked_factors(C.SEED, 3, 2, T, B, H, 0.5, **cols)
    lengths = np.array([5, 3])
    yd, stats, grad, x = actreg_run(raw, g, 2.0, 1.0, 0.5, snap, F.locked_site(2), dev(lengths), desc=desc)
    assert np.array_equal(yd.cpu().numpy(), raw * fn)
    want = A.oracle(raw, fn, lengths, 2.0, 1.0, g)
    A.check_stats(stats, want, T, B, H, 2.0, 1.0, "group layer")
    A.check_draw(grad.cpu().numpy(), want, "group layer")


# ---- 8. the whole Model ------------------------------------------------------------------------------------------------------------
V_LM, L_LM = 120, 2


def lm(H, **kw):
    torch.manual_seed(5)
    r = 8 if H < 100 else 32
    return Model(V_LM, H, L_LM, 0.5, 0.08, w_rank=r, u_ranks=[r], lstm_type="vmlmf", locked_dropout=True, input_dropout=C.RECIPE[0],
                 hidden_dropout=C.RECIPE[1], output_dropout=C.RECIPE[2], **kw).to(DEV).train()


@pytest.mark.parametrize("full", [False, True], ids=["plain", "ar_tar_tied_word"])
@pytest.mark.parametrize("H,B,T", C.MODEL_SHAPES, ids=["valu_layers", "row_block_layers"])
def test_model_loss_and_backward_vs_the_fp64_restatement(H, B, T, full):
    m = lm(H, tie_weights=True, embed_dropout=0.5) if full else lm(H)
    kw = dict(ar=2.0, tar=1.0) if full else {}
    word_p = 0.5 if full else 0.0
    st = m.dropout_state(seed=C.SEED)
    st[1] = 41
    snap = st.clone()
    r = np.random.Generator(np.random.PCG64(4))
    tok = torch.tensor(r.integers(0, V_LM, size=(T, B)), device=DEV)
    tgt = torch.tensor(r.integers(0, V_LM, size=(T, B)), device=DEV)
    states = [(dev((0.2 * r.standard_normal((B, H))).astype(np.float32)), dev((0.2 * r.standard_normal((B, H))).astype(np.float32)))
              for _ in range(L_LM)]
    loss, new_states = m.loss(tok, tgt, [tuple(s) for s in states], **kw)
    assert st.tolist() == [C.SEED, 42]
    loss.backward(unit_gradient(loss.device))
    rates = m.site_rates()
    assert rates == [0.4, 0.25, 0.4]
    # the factors: the restatement at position b (one-group layers: identity columns), checked against what the library draws
    Fs = [C.locked_factors(C.SEED, 41, i, T, B, H, rates[i]) for i in range(L_LM + 1)]
    for i in range(L_LM + 1):
        assert np.array_equal(F.dropout_factors(T * B, H, rates[i], snap, i, locked_batch=B).cpu().numpy().reshape(T, B, H), Fs[i])
    fw = TC.word_factors(V_LM, word_p, 41, seed=C.SEED)
    assert np.array_equal(vmlmf_amd.word_dropout_factors(V_LM, word_p, snap).cpu().numpy(), fw)
    # the fp64 CPU restatement with the factor tensors
    f64 = torch.float64
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in m.state_dict().items() if not (full and k == "fc.w")}
    table = sd["embed.w"]
    head_w = table if full else sd["fc.w"]
    tokc = tok.cpu()
    h = (table[tokc] * torch.tensor(fw, dtype=f64)[tokc][..., None]) * torch.tensor(Fs[0], dtype=f64)
    ref_states = []
    for i in range(L_LM):
        P = {k.split(".", 2)[2]: v for k, v in sd.items() if k.startswith(f"rnns.{i}.")}
        raw, hT, cT = O.literal_sequence(O.V3, P, h, states[i][0].cpu().double(), states[i][1].cpu().double(), time_major=True)
        ref_states.append((hT, cT))
        h = raw * torch.tensor(Fs[i + 1], dtype=f64)
    penalty = 0.0
    if full:
        h, penalty, _ = F.activation_regularizer_stock(raw, ar=2.0, tar=1.0, factors=torch.tensor(Fs[L_LM], dtype=f64), batch_scale=B)
    ref = F.nll_loss(torch.addmm(sd["fc.b"], h.reshape(-1, H), head_w.t()), tgt.cpu()) + penalty
    ref.backward()
    assert abs(loss.item() - ref.item()) <= 1e-5 * max(1.0, abs(ref.item())), (loss.item(), ref.item())
    for i in range(L_LM):
        assert_out(new_states[i][0].detach().cpu().numpy(), ref_states[i][0].detach().numpy(), f"hT[{i}]")
        assert_out(new_states[i][1].detach().cpu().numpy(), ref_states[i][1].detach().numpy(), f"cT[{i}]")
    for k, v in m.named_parameters():
        assert_grad(v.grad.cpu().numpy(), sd[k].grad.numpy(), k)
    # structure, on the device outputs: the zero pattern of a site does not depend on t and differs between two batch rows
    st[1] = 41
    top, _ = m.features(tok, [tuple(s) for s in states])
    st[1] = 41
    first = F.embedding_dropout(m.embed.w, tok, rates[0], F.dropout_advance(st), 0, word_p=word_p, locked=True)
    st[1] = 41
    raw_top = m._features(tok, [tuple(s) for s in states], raw_top=True)[0].detach().cpu().numpy()
    # (an element the site keeps is zero only where what went into the site is: a dropped word's row, a unit whose output is 0.0)
    own_zeros = {0: np.broadcast_to((fw[tokc.numpy()] == 0)[..., None], (T, B, H)), L_LM: raw_top == 0}
    for y, site in ((first, 0), (top, L_LM)):
        z = y.detach().cpu().numpy() == 0
        assert np.array_equal(z, (Fs[site] == 0) | own_zeros[site]), site
        assert C.zero_pattern_is_locked(Fs[site]) and not np.array_equal(Fs[site][0, 0], Fs[site][0, 1])
    assert (raw_top == 0).mean() < 1e-3          # (an LSTM unit's output is 0.0 only where o tanh(c) rounds to it)
    # ... and element by element the two are the restatement's top layer, raw and behind its site
    assert_out(raw_top, raw.detach().numpy(), "raw top layer")
    assert_out(top.detach().cpu().numpy(), (raw.detach() * torch.tensor(Fs[L_LM], dtype=f64)).numpy(), "top site")
    # eval mode: the identity, and nothing is drawn
    m.eval()
    before = st.clone()
    plain = Model(V_LM, H, L_LM, 0.0, 0.08, w_rank=8 if H < 100 else 32, u_ranks=[8 if H < 100 else 32], lstm_type="vmlmf").to(DEV).eval()
    plain.load_state_dict(m.state_dict())
    with torch.no_grad():
        a, _ = m(tok, [tuple(s) for s in states])
        b, _ = plain(tok, [tuple(s) for s in states])
    assert torch.equal(a, b) and torch.equal(st, before)


def test_a_default_model_draws_the_per_element_factors_it_drew():
    """Built without the new arguments: the sites' factors are the per-element ones of the same snapshot - the loss of a default
    model equals the loss of one whose three rates are spelled out, to the bit, and differs from the locked model's."""
    H, B, T = 32, 6, 5
    torch.manual_seed(5)
    mk = lambda **kw: Model(V_LM, H, L_LM, 0.5, 0.08, w_rank=8, u_ranks=[8], lstm_type="vmlmf", **kw).to(DEV).train()
    a = mk()
    b = mk(input_dropout=0.5, hidden_dropout=0.5, output_dropout=0.5)
    c = mk(locked_dropout=True)
    b.load_state_dict(a.state_dict()), c.load_state_dict(a.state_dict())
    r = np.random.Generator(np.random.PCG64(4))
    tok = torch.tensor(r.integers(0, V_LM, size=(T, B)), device=DEV)
    tgt = torch.tensor(r.integers(0, V_LM, size=(T, B)), device=DEV)
    out = []
    for m in (a, b, c):
        m.dropout_state(seed=C.SEED)
        out.append(m.loss(tok, tgt, m.state_init(B))[0].detach())
    assert torch.equal(bits(out[0]), bits(out[1])) and not torch.equal(out[0], out[2])
    a.dropout_state(seed=C.SEED)
    top, _ = a.features(tok, a.state_init(B))
    assert np.array_equal(top.detach().cpu().numpy() == 0, O.dropout_factors(C.SEED, 0, L_LM, T * B, H, 0.5).reshape(T, B, H) == 0)


# ---- 9. a captured step ------------------------------------------------------------------------------------------------------------
def test_a_captured_training_step_draws_a_fresh_locked_mask_on_every_replay():
    torch.manual_seed(2)
    H, B, T, V = 650, 20, 4, 80
    m = Model(V, H, 2, 0.5, 0.05, w_rank=32, u_ranks=[32], lstm_type="vmlmf", locked_dropout=True, input_dropout=0.4, hidden_dropout=0.25,
              output_dropout=0.4).to(DEV).train()
    st = m.dropout_state(seed=C.SEED)
    tok = torch.randint(0, V, (T, B), device=DEV)
    tgt = torch.randint(0, V, (T, B), device=DEV)
    states = m.state_init(B)
    top = torch.zeros(T, B, H, device=DEV)

    def step():
        for p_ in m.parameters():
            p_.grad = None
        h, _ = m.features(tok, [tuple(s) for s in states])          # (one more forward, to look at the mask of the top site)
        top.copy_(h.detach())
        loss, _ = m.loss(tok, tgt, [tuple(s) for s in states])
        loss.backward()
        return loss

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    off0 = st[1].item()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss = step()
    losses, masks = [], []
    for _ in range(3):
        g.replay()
        losses.append(loss.item())
        masks.append((top == 0).cpu().numpy())
    assert st[1].item() == off0 + 2 * 3          # two forwards per step, each a snapshot of its own
    assert len(set(losses)) == 3, losses
    for i, z in enumerate(masks):                # replay i's top-site mask: locked, and the restatement's at that replay's offset
        assert C.zero_pattern_is_locked(z)
        assert np.array_equal(z, C.locked_factors(C.SEED, off0 + 2 * i, 2, T, B, H, 0.4) == 0)
    assert 0.3 < (masks[0][0] != masks[1][0]).mean() < 0.7          # 2 p (1 - p) = 0.48 of the elements differ between two masks
    # ... and each replay equals the eager step at the same offset
    st[1] = off0 + 2
    assert abs(step().item() - losses[1]) <= 1e-6 * abs(losses[1])
