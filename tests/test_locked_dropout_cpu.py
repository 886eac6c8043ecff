"""CPU: locked (variational) dropout with a rate per site (docs/design/lm_locked.md) - the restated rule, Model's new attributes on
CPU tensors (AWD-LSTM's LockedDropout in stock ops), the defaults that must not move, the drop tuples, and the library's surface."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import locked_cases as C
import vmlmf_oracle as O
from vmlmf_amd import Model, _lib
from vmlmf_amd import functional as F
from vmlmf_amd.lm import stack_layers

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def test_the_restated_locked_factors_are_constant_over_time_and_zero_or_the_scale():
    for p in (0.25, 0.4, 0.5):
        f = C.locked_factors(C.SEED, 7, 2, 6, 5, 130, p)
        assert f.shape == (6, 5, 130) and all(np.array_equal(f[t], f[0]) for t in range(6))
        vals = np.unique(f)
        assert len(vals) == 2 and vals[0] == 0.0 and vals[1] == np.float32(1) / (np.float32(1) - np.float32(p))
        assert C.zero_pattern_is_locked(f)
    # the flag is part of the site word: the locked stream of a site is not its per-element stream at the same positions
    a = C.locked_mask(C.SEED, 7, 2, 64, 64, 0.5)
    b = O.dropout_factors(C.SEED, 7, 2, 64, 64, 0.5)
    assert 0.4 < (a != b).mean() < 0.6
    assert np.array_equal(a, O.dropout_factors(C.SEED, 7, 2 | (1 << 31), 64, 64, 0.5))
    # batch rows, sites and offsets differ
    assert abs((a[0] != a[1]).mean() - 0.5) < C.rate_bound(0.5, 64)          # (64 columns: five sigma is 0.31)
    for other in (C.locked_mask(C.SEED, 7, 3, 64, 64, 0.5), C.locked_mask(C.SEED, 8, 2, 64, 64, 0.5)):
        assert 0.4 < (a != other).mean() < 0.6
    assert np.array_equal(C.locked_factors(C.SEED, 7, 2, 3, 4, 8, 0.0), np.ones((3, 4, 8), np.float32))


@pytest.mark.parametrize("p", [0.25, 0.4, 0.5, 0.9])
def test_the_drop_rate_over_the_independent_draws(p):
    """Under a locked mask the independent draws are the B H of one mask, not T B H: 16 x 650 = 10 400 of them."""
    B, H = 16, 650
    for offset in C.OFFSETS:
        m = C.locked_mask(C.SEED, offset, 1, B, H, p)
        assert abs((m == 0).mean() - p) < C.rate_bound(p, B * H), (p, offset, (m == 0).mean())


# ---- Model on CPU tensors ----------------------------------------------------------------------------------------------------------
V, H, L, B, T = 50, 256, 3, 40, 3          # B H = 10 240 independent draws per site


def model(**kw):
    torch.manual_seed(3)
    return Model(V, H, L, 0.5, 0.1, lstm_type="pytorch", **kw)


def tokens():
    return torch.tensor(np.random.Generator(np.random.PCG64(1)).integers(0, V, size=(T, B)))


def site_outputs(m, tok):
    """What leaves each dropout site: the inputs of the L layers (sites 0 .. L - 1) and of the projection (site L)."""
    seen = {}
    hooks = [r.register_forward_pre_hook(lambda mod, args, i=i: seen.__setitem__(i, args[0].detach().clone())) for i, r in enumerate(m.rnns)]
    hooks.append(m.fc.register_forward_pre_hook(lambda mod, args: seen.__setitem__(L, args[0].detach().clone())))
    raws = {}
    hooks += [r.register_forward_hook(lambda mod, args, out, i=i: raws.__setitem__(i, out[0].detach().clone())) for i, r in enumerate(m.rnns)]
    scores, _ = m(tok, m.state_init(B))
    for h in hooks:
        h.remove()
    return [seen[i].reshape(T, B, H).numpy() for i in range(L + 1)], [raws[i].numpy() for i in range(L)], scores.detach()


def test_a_cpu_model_locks_every_site_at_its_own_rate():
    m = model(locked_dropout=True, input_dropout=C.RECIPE[0], hidden_dropout=C.RECIPE[1], output_dropout=C.RECIPE[2]).train()
    assert m.site_rates() == [0.4, 0.25, 0.25, 0.4]
    torch.manual_seed(11)
    sites, raws, _ = site_outputs(m, tokens())
    for i, (y, p) in enumerate(zip(sites, m.site_rates())):
        z = y == 0
        assert C.zero_pattern_is_locked(y), f"site {i}: the zero pattern moves with t"
        assert abs(z[0].mean() - p) < C.rate_bound(p, B * H), (i, z[0].mean(), p)
        assert 0.1 < (z[0, 0] != z[0, 1]).mean(), f"site {i}: two batch rows share a mask"
        if i > 0:      # kept elements are the layer's output over 1 - p
            keep = ~z
            assert np.allclose(y[keep], raws[i - 1][keep] / (1 - p), rtol=1e-6, atol=0)
    # the masks of two sites, and of two forward passes, are not the same
    assert ((sites[1] == 0)[0] != (sites[2] == 0)[0]).mean() > 0.1
    again, _, _ = site_outputs(m, tokens())
    assert ((sites[0] == 0)[0] != (again[0] == 0)[0]).mean() > 0.1
    # eval mode is the identity at every site
    m.eval()
    assert m.site_rates() == [0.0] * (L + 1)
    sites, raws, a = site_outputs(m, tokens())
    assert all(np.array_equal(sites[i + 1], raws[i]) for i in range(L))
    plain = model().eval()
    plain.load_state_dict(m.state_dict())
    assert torch.equal(a, site_outputs(plain, tokens())[2])


def test_per_site_rates_without_locking_are_nn_dropouts_rule_and_a_zero_rate_skips_the_site():
    m = model(input_dropout=0.4, hidden_dropout=0.0, output_dropout=0.25).train()
    torch.manual_seed(12)
    sites, raws, _ = site_outputs(m, tokens())
    for i, p in ((0, 0.4), (L, 0.25)):
        z = sites[i] == 0
        assert not C.zero_pattern_is_locked(sites[i])
        assert abs(z.mean() - p) < C.rate_bound(p, T * B * H)
    assert all(np.array_equal(sites[i], raws[i - 1]) for i in (1, 2))


def test_a_default_model_is_what_it_was():
    m = model().train()
    assert m.locked_dropout is False and m.input_dropout is None and m.hidden_dropout is None and m.output_dropout is None
    assert m.site_rates() == [0.5] * (L + 1)
    keys = ["embed.w"] + [f"rnns.{i}.{k}" for i in range(L) for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")] + ["fc.w", "fc.b"]
    assert list(m.state_dict()) == keys
    assert list(model(locked_dropout=True, input_dropout=0.4, hidden_dropout=0.25, output_dropout=0.4).state_dict()) == keys
    # the outputs of nn.Dropout's launches, draw for draw: vmlmf_lm.py:434-440 restated on the same generator state
    tok = tokens()
    torch.manual_seed(21)
    got, _ = m(tok, m.state_init(B))
    torch.manual_seed(21)
    drop = torch.nn.Dropout(0.5)
    x = drop(m.embed.w[tok])
    for rnn, st in zip(m.rnns, m.state_init(B)):
        x, _ = rnn(x, st)
        x = drop(x)
    want = torch.addmm(m.fc.b, x.view(-1, H), m.fc.w.t())
    assert torch.equal(got, want)
    # ... and of Model.loss under ar / tar (the top site's factors drawn the way they were)
    y = torch.tensor(np.random.Generator(np.random.PCG64(2)).integers(0, V, size=(T, B)))
    torch.manual_seed(22)
    a, _ = m.loss(tok, y, m.state_init(B), ar=2.0, tar=1.0)
    torch.manual_seed(22)
    x = drop(m.embed.w[tok])
    for i, (rnn, st) in enumerate(zip(m.rnns, m.state_init(B))):
        x, _ = rnn(x, st)
        x = drop(x) if i < L - 1 else x
    f = torch.nn.functional.dropout(torch.ones_like(x), 0.5, True)
    yd, penalty, _ = F.activation_regularizer_stock(x, ar=2.0, tar=1.0, factors=f, batch_scale=B)
    b = F.nll_loss(torch.addmm(m.fc.b, yd.reshape(-1, H), m.fc.w.t()), y) + penalty
    assert float(a.detach()) == pytest.approx(float(b.detach()), rel=1e-6)


def test_model_loss_with_ar_and_tar_under_a_locked_top_site_on_the_cpu(monkeypatch):
    m = model(locked_dropout=True, output_dropout=0.4).train()
    tok = tokens()
    y = torch.tensor(np.random.Generator(np.random.PCG64(2)).integers(0, V, size=(T, B)))
    torch.manual_seed(31)
    seen = {}
    stock = F.activation_regularizer_stock

    def spy(raw, **kw):
        out = stock(raw, **kw)
        seen.update(raw=raw.detach(), factors=kw["factors"], yd=out[0].detach())
        return out
    monkeypatch.setattr(F, "activation_regularizer_stock", spy)
    loss, _ = m.loss(tok, y, m.state_init(B), ar=2.0, tar=1.0)
    loss.backward()
    # the top site's factors are ONE (1, B, H) mask, and what reaches the head is the raw output under it at every time step
    assert seen["factors"].shape == (1, B, H) and len(np.unique(seen["factors"].numpy())) == 2
    z = seen["yd"].numpy() == 0
    assert C.zero_pattern_is_locked(seen["yd"].numpy()) and np.array_equal(z[0], seen["factors"].numpy()[0] == 0)
    assert abs(z[0].mean() - 0.4) < C.rate_bound(0.4, B * H) and 0.1 < (z[0, 0] != z[0, 1]).mean()
    assert torch.equal(seen["yd"], seen["raw"] * seen["factors"])
    assert torch.isfinite(loss) and all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    raw, _, site = m._features(tok, m.state_init(B), raw_top=True)
    assert site == (0.4,) and raw.shape == (T, B, H) and not (raw == 0).any()


def test_bad_values_are_value_errors():
    m = model()
    for bad in (1, 0, "yes", None, 0.5):
        with pytest.raises(ValueError):
            m.locked_dropout = bad
    for name in ("input_dropout", "hidden_dropout", "output_dropout"):
        for bad in (True, False, 1.0, -0.1, 1.5, float("nan"), "0.3"):
            with pytest.raises(ValueError):
                setattr(m, name, bad)
        setattr(m, name, 0.3)
        assert getattr(m, name) == 0.3
        setattr(m, name, None)
        assert getattr(m, name) is None
        setattr(m, name, 0)
        assert getattr(m, name) == 0.0 and isinstance(getattr(m, name), float)
    for kw in (dict(locked_dropout=1), dict(input_dropout=True), dict(hidden_dropout=1.0), dict(output_dropout=-0.5)):
        with pytest.raises(ValueError):
            model(**kw)
        with pytest.raises(ValueError):
            Model.with_group_layers(20, 8, 2, 0.5, 0.1, 4, [2, 2], **kw)
    g = Model.with_group_layers(20, 8, 2, 0.5, 0.1, 4, [2, 2], locked_dropout=True, input_dropout=0.4, hidden_dropout=0.25, output_dropout=0.1)
    assert g.locked_dropout is True and g.train().site_rates() == [0.4, 0.25, 0.1]
    with pytest.raises(ValueError):                       # a locked mask lies over (T, B, H)
        F.dropout(torch.zeros(6, 4), 0.5, None, 1, locked=True)
    with pytest.raises(ValueError):
        F.embedding_dropout(torch.zeros(5, 4), torch.zeros(6, dtype=torch.int64), 0.5, None, locked=True)


def test_drop_tuples_three_still_mean_per_element():
    snap = object()
    assert not F.drop_locked((0.5, snap, 2)) and F.site_word((0.5, snap, 2)) == 2
    assert not F.drop_locked((0.5, snap, 2, False)) and F.site_word((0.5, snap, 2, False)) == 2
    assert F.drop_locked((0.5, snap, 2, True)) and F.site_word((0.5, snap, 2, True)) == 2 - (1 << 31) == ctypes.c_int32(C.locked_site(2)).value
    assert F.locked_site(3) == C.locked_site(3) == 0x80000003
    # stack_layers takes either form (CPU tensors: not covered, the caller loops over the layers)
    m = Model(20, 8, 2, 0.5, 0.1, w_rank=2, u_ranks=[2], lstm_type="vmlmf")
    x = torch.zeros(3, 2, 8)
    for drops in ([(0.5, None, 1), (0.5, None, 2)], [(0.5, None, 1, True), None], None):
        assert stack_layers(m.rnns, x, m.state_init(2), drops) is None
    # the stock form of the rule
    torch.manual_seed(1)
    y = F.locked_dropout_stock(torch.ones(5, 40, 256), 0.25)
    assert C.zero_pattern_is_locked(y.numpy()) and abs((y[0] == 0).double().mean().item() - 0.25) < C.rate_bound(0.25, 40 * 256)
    assert set(np.unique(y.numpy())) == {0.0, np.float32(1 / 0.75)}
    x = torch.ones(2, 3, 4)
    assert F.locked_dropout_stock(x, 0.5, training=False) is x and F.locked_dropout_stock(x, 0.0) is x


def test_the_library_exports_the_new_symbols_at_abi_13():
    lib = _lib.lib()
    assert lib.vmlmf_abi_version() == 13 == _lib.ABI_VERSION
    for name in ("vmlmf_dropout_apply_locked", "vmlmf_dropout_factors_locked", "vmlmf_embed_dropout_forward_lk", "vmlmf_embed_backward_lk"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    header = open(os.path.join(HERE, "..", "include", "vmlmf_hip.h")).read()
    assert re.search(r"#define VMLMF_ABI_VERSION 13\b", header)
    assert re.search(r"#define VMLMF_SITE_LOCKED \(\(int32_t\)\(-2147483647 - 1\)\)", header)
    assert _lib.SITE_LOCKED == -(1 << 31) == ctypes.c_int32(C.SITE_LOCKED).value
    # refusals that are made before any device work: R that is no multiple of B, B < 1
    for R, Bb in ((7, 2), (4, 0), (4, -1)):
        assert lib.vmlmf_dropout_apply_locked(R, Bb, 8, None, None, 0.5, None, 1, None) == _lib.E_BADARG
        assert lib.vmlmf_dropout_factors_locked(None, R, Bb, 8, 0.5, None, 1, None, None) == _lib.E_BADARG
        assert lib.vmlmf_embed_dropout_forward_lk(R, Bb, 8, 5, None, None, None, 0.5, 0.0, None, 0, None) == _lib.E_BADARG
        assert lib.vmlmf_embed_backward_lk(R, Bb, 8, 5, None, None, None, 0, None, 0, 0.5, 0.0, None, 0, None) == _lib.E_BADARG
