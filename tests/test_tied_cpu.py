"""Weight tying and word-level embedding dropout without a GPU (docs/design/lm_tied.md): the word factors as the oracle draws them;
the float32 restatement of the table gradient against its parts and against known-wrong rules; tie_weights / untie_weights and
everything that walks the parameters; a tied Model on CPU tensors against its untied twin, to the bit; the stock-op form of the word
dropout; the refusals, from Python and from the C entry points; the default path never enters the new code.
(clip_sgd_step and optim.Adam take HIP tensors only: their step on a tied model is in test_gpu_tied.py; here they are handed what
they would be handed, and optim.ASGD and DynamicEval - which have stock-op paths - run.)"""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import tied_cases as C
import vmlmf_amd
import vmlmf_oracle as O
from vmlmf_amd import Model, _lib
from vmlmf_amd import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the word factors ---------------------------------------------------------------------------------------------------------
def test_a_word_factor_depends_on_the_token_alone():
    fw = C.word_factors(12, 0.5, 7)
    assert [int((C.word_factors(12, 0.5, o) == 0).sum()) for o in C.OFFSETS] == [5, 10, 6]
    assert set(np.unique(fw)) == {0.0, 2.0}
    tok = np.array([3, 1, 3, 11, 1, 3])
    w = np.arange(1, 12 * 4 + 1, dtype=np.float32).reshape(12, 4)
    out = C.forward(w, tok, np.ones((6, 4), np.float32), fw)
    assert C.same_bits(out[0], out[2]) and C.same_bits(out[0], out[5]) and C.same_bits(out[1], out[4])     # one word, one factor
    assert np.all(out[1] == 0) and np.all(out[0] == 2 * w[3])                                                # word 1 dropped, 3 kept
    a, b = C.word_factors(4096, 0.5, 7), C.word_factors(4096, 0.5, 8)
    assert int((a == 0).sum()) == 2064 and int((b == 0).sum()) == 2058
    assert int(((a == 0) != (b == 0)).sum()) == 2042                      # another offset, another mask
    site0 = O.dropout_factors(C.SEED, 7, 0, 4096, 1, 0.5)[:, 0]
    assert 1856 <= int(((a == 0) != (site0 == 0)).sum()) <= 2240          # the word site does not repeat site 0's bits
    for n in (int((a == 0).sum()), int((b == 0).sum())):
        assert 1856 <= n <= 2240                                          # 6 sigma around 2048 (sigma = 32)
    assert np.all(C.word_factors(12, 0.0, 7) == 1)
    assert np.float32(C.word_factors(64, 0.25, 7).max()) == np.float32(1.0) / (np.float32(1.0) - np.float32(0.25))


# ---- 2. the float32 restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.SHAPES[:7], ids=C.IDS[:7])
def test_the_restatement_is_the_existing_sum_then_one_multiplication_and_one_addition(shape):
    R, V, H = shape
    w, dy, base = C.draw(R, V, H, 11)
    for j, pattern in enumerate(C.PATTERNS):
        tok = C.tokens(R, V, pattern, j)
        for p, word_p in C.DROPS:
            f, fw = C.element_factors(R, H, p, 8), C.word_factors(V, word_p, 8)
            s = C.ordered_sum(tok, dy, f, V)
            hit, kept = np.bincount(tok, minlength=V) > 0, fw != 0
            assert np.all(s[~hit] == 0)
            plain = C.table_gradient(tok, dy, f, np.ones(V, np.float32), V)
            assert C.same_bits(plain, s)                                                         # the existing entries' sum
            got = C.table_gradient(tok, dy, f, fw, V)
            assert C.same_bits(got[kept], (fw[:, None] * s).astype(np.float32)[kept]) and np.all(got[~kept] == 0)
            acc = C.table_gradient(tok, dy, f, fw, V, base=base)
            rows = hit & kept
            assert C.same_bits(acc[rows], (base + (fw[:, None] * s).astype(np.float32)).astype(np.float32)[rows])
            assert C.same_bits(acc[~rows], base[~rows])
            assert C.excess(got, tok, dy, f, fw, V) <= 1.0 and C.excess(acc, tok, dy, f, fw, V, base) <= 1.0


def test_known_wrong_rules_are_caught():
    R, V, H = 33, 12, 8
    w, dy, base = C.draw(R, V, H, 12)
    tok = C.tokens(R, V, "last", 3)
    f, fw = C.element_factors(R, H, 0.5, 7), C.word_factors(V, 0.5, 7)
    right = C.table_gradient(tok, dy, f, fw, V, base=base)
    assert C.excess(right, tok, dy, f, fw, V, base) <= 1.0
    for variant in ("fw_by_position", "dropped_accumulated"):
        wrong = C.table_gradient(tok, dy, f, fw, V, base=base, variant=variant)
        assert not C.same_bits(wrong, right) and C.excess(wrong, tok, dy, f, fw, V, base) > 1.0, variant
    # the order of the forward's two multiplications shows where neither factor is a power of two
    f3, fw3 = C.element_factors(R, H, 0.3, 7), C.word_factors(V, 0.1, 7)
    a, b = C.forward(w, tok, f3, fw3), C.forward(w, tok, f3, fw3, variant="f_first")
    assert not C.same_bits(a, b) and np.allclose(a, b, rtol=4 * C.U)
    first = (w[tok] * fw3[tok][:, None]).astype(np.float32)
    assert C.same_bits(a, (first * f3).astype(np.float32))


# ---- 3. tie_weights / untie_weights / tied -----------------------------------------------------------------------------------------
def make(V=64, H=32, layers=2, dropout=0.0, **kw):
    torch.manual_seed(7)
    return Model(V, H, layers, dropout, 0.1, lstm_type="custom", **kw)


def test_tying_names_the_table_once_and_survives_copies():
    model = make()
    n, numel = len(list(model.parameters())), sum(p.numel() for p in model.parameters())
    assert not model.tied
    before = model.embed.w.detach().clone()
    assert model.tie_weights() is model and model.tied and model.fc.w is model.embed.w
    assert torch.equal(model.embed.w, before)                                   # embed.w's values are kept
    assert len(list(model.parameters())) == n - 1 and sum(p.numel() for p in model.parameters()) == numel - 64 * 32
    sd = model.state_dict()
    assert "fc.w" in sd and "embed.w" in sd and torch.equal(sd["fc.w"], sd["embed.w"])
    other = make(tie_weights=True)
    assert other.tied
    with torch.no_grad():
        other.embed.w.add_(1.0)
    other.load_state_dict(sd)
    assert other.tied and torch.equal(other.embed.w, model.embed.w)
    assert copy.deepcopy(model).tied and model.to(torch.float64).tied and model.to(torch.float32).tied
    assert Model.with_group_layers(32, 16, 2, 0.0, 0.1, 4, [2, 2], tie_weights=True, embed_dropout=0.25).tied
    model.untie_weights()
    assert not model.tied and torch.equal(model.fc.w, model.embed.w) and len(list(model.parameters())) == n
    with torch.no_grad():
        model.fc.w.add_(1.0)
    assert not torch.equal(model.fc.w, model.embed.w)


def test_lm_buckets_name_a_tied_table_once_in_the_last_bucket():
    from vmlmf_amd import dp
    model = make(tie_weights=True)
    buckets = dp.lm_buckets(model)
    ids = [id(p) for b in buckets for p in b]
    assert len(ids) == len(set(ids)) == len(list(model.parameters()))
    assert [id(p) for p in buckets[-1]] == [id(model.embed.w)] and [id(p) for p in buckets[0]] == [id(model.fc.b)]
    dp.BucketedGradAllReduce(buckets)
    untied = dp.lm_buckets(make())
    assert len(untied[0]) == 2 and len(untied[-1]) == 1                          # as before


# ---- 4. a tied Model on CPU tensors against its untied twin ------------------------------------------------------------------------
LOSSES = {
    "loss": lambda m, x, y, t: m.loss(x, y, m.state_init(3))[0],
    "ar_tar": lambda m, x, y, t: m.loss(x, y, m.state_init(3), ar=2.0, tar=1.0)[0],
    "smoothing": lambda m, x, y, t: m.loss(x, y, m.state_init(3), label_smoothing=0.1)[0],
    "distill": lambda m, x, y, t: m.distill_loss(x, y, m.state_init(3), t)[0],
}


@pytest.mark.parametrize("which", list(LOSSES))
def test_the_tied_gradient_on_the_cpu_is_the_twins_sum_to_the_bit(which):
    tied, twin = C.twins(make)
    torch.manual_seed(3)
    x, y, teacher = torch.randint(0, 64, (6, 3)), torch.randint(0, 64, (6, 3)), torch.randn(6, 3, 64)
    a, b = LOSSES[which](tied, x, y, teacher), LOSSES[which](twin, x, y, teacher)
    assert torch.equal(a, b)
    a.backward()
    b.backward()
    assert torch.equal(tied.embed.w.grad, twin.embed.w.grad + twin.fc.w.grad)
    pa, pb = dict(tied.named_parameters()), dict(twin.named_parameters())
    assert set(pb) - set(pa) == {"fc.w"}
    for name in pa:
        if name != "embed.w":
            assert torch.equal(pa[name].grad, pb[name].grad), name


# ---- 5. embed_dropout on the CPU ----------------------------------------------------------------------------------------------------
def test_the_stock_form_is_the_awd_lstm_expression_and_eval_draws_nothing():
    torch.manual_seed(1)
    w, tok = torch.randn(20, 6), torch.randint(0, 20, (5, 3))
    torch.manual_seed(9)
    got = F.embedding_dropout_stock(w, tok, 0.0, 0.5)
    torch.manual_seed(9)
    mask = torch.nn.functional.dropout(torch.ones(20, 1), 0.5, True)
    assert set(mask.unique().tolist()) == {0.0, 2.0}
    assert torch.equal(got, torch.nn.functional.embedding(tok, mask.expand_as(w) * w))          # AWD-LSTM's embedded_dropout
    torch.manual_seed(9)
    both = F.embedding_dropout_stock(w, tok, 0.5, 0.5)
    torch.manual_seed(9)
    mask = torch.nn.functional.dropout(torch.ones(20, 1), 0.5, True)
    assert torch.equal(both, torch.nn.functional.dropout(torch.nn.functional.embedding(tok, mask * w), 0.5, True))
    assert torch.equal(F.embedding_dropout_stock(w, tok, 0.5, 0.5, training=False), w[tok])
    # in a Model: training mode drops whole words, eval mode draws nothing and is the model without it
    model, plain = make(embed_dropout=0.5), make()
    x = torch.randint(0, 64, (6, 3))
    assert model.embed_dropout == 0.5 and plain.embed_dropout == 0.0
    model.eval(), plain.eval()
    state = torch.get_rng_state()
    assert torch.equal(model(x, model.state_init(3))[0], plain(x, plain.state_init(3))[0])
    assert torch.equal(torch.get_rng_state(), state)
    model.train()
    seen = []
    real = F.embedding_dropout_stock
    F.embedding_dropout_stock = lambda *a, **k: seen.append(a[3]) or real(*a, **k)
    try:
        out = model(x, model.state_init(3))[0]
    finally:
        F.embedding_dropout_stock = real
    assert seen == [0.5] and not torch.equal(out, plain(x, plain.state_init(3))[0])


# ---- 6. refusals; the default path -------------------------------------------------------------------------------------------------
def test_python_arguments_are_refused():
    for bad in (1.0, -0.1, True, False, "0.5", None, float("nan")):
        with pytest.raises(ValueError):
            make(embed_dropout=bad)
        model = make()
        with pytest.raises(ValueError):
            model.embed_dropout = bad
        with pytest.raises(ValueError):
            F.embedding_dropout(torch.zeros(4, 4), torch.zeros(2, dtype=torch.int64), 0.0, None, word_p=bad)
        with pytest.raises(ValueError):
            F.embedding_dropout_stock(torch.zeros(4, 4), torch.zeros(2, dtype=torch.int64), 0.0, bad)
    model = make()
    model.embed_dropout = 0
    assert model.embed_dropout == 0.0 and isinstance(model.embed_dropout, float)
    with pytest.raises(RuntimeError):                       # the kernels take HIP tables: a missing kernel is an error, not a fallback
        F.embedding(torch.zeros(4, 4, requires_grad=True), torch.zeros(2, dtype=torch.int64), grad_from=F.TiedGradient())
    with pytest.raises(RuntimeError):
        F.embedding_dropout(torch.zeros(4, 4), torch.zeros(2, dtype=torch.int64), 0.0, None, word_p=0.5)
    with pytest.raises(RuntimeError):
        vmlmf_amd.word_dropout_factors(8, 0.5, torch.zeros(2, dtype=torch.int64))
    assert F.tied_gradient(torch.zeros(4, 4, requires_grad=True), torch.zeros(2, dtype=torch.int64)) is None      # CPU: autograd's sum
    for name in ("embedding_dropout_stock", "word_dropout_factors", "TiedGradient", "tied_gradient"):
        assert name in vmlmf_amd.__all__ and getattr(vmlmf_amd, name) is getattr(F, name)


def test_the_c_entries_refuse_bad_arguments_without_touching_a_gpu():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "vmlmf_hip.h")).read()
    for name in ("vmlmf_embed_dropout_forward_ex", "vmlmf_embed_backward_ex"):
        assert hasattr(handle, name) and name in _lib.SYMBOLS and f"int {name}(" in header
    assert f"#define VMLMF_SITE_WORD 0x{C.SITE_WORD:08X} " in header
    assert _lib.ABI_VERSION == 13 and handle.vmlmf_abi_version() == 13
    lib = _lib.lib()
    fake, other = ctypes.c_void_p(4096), ctypes.c_void_p(8192)          # the launch is never reached: no device is touched
    fl = ctypes.c_float
    need = lib.vmlmf_embed_backward_scratch_bytes(40, 7)
    assert need == 7 * 2 * 4

    def fwd(R=40, H=8, V=7, tok=fake, w=fake, out=other, p=0.5, wp=0.5, state=fake):
        return lib.vmlmf_embed_dropout_forward_ex(R, H, V, tok, w, out, fl(p), fl(wp), state, 0, None)

    def bwd(R=40, H=8, V=7, tok=fake, dy=fake, dw=other, acc=1, scratch=fake, nbytes=need, p=0.5, wp=0.5, state=fake):
        return lib.vmlmf_embed_backward_ex(R, H, V, tok, dy, dw, acc, scratch, nbytes, fl(p), fl(wp), state, 0, None)
    for kw in (dict(R=-1), dict(H=0), dict(V=0), dict(tok=None), dict(w=None), dict(out=None), dict(p=1.0), dict(p=-0.5), dict(wp=1.0),
               dict(wp=-0.25), dict(wp=float("nan")), dict(state=None), dict(state=None, p=0.0), dict(state=None, wp=0.0)):
        assert fwd(**kw) == _lib.E_BADARG, kw
        assert lib.vmlmf_last_error().decode()
    assert fwd(R=0) == 0                                                  # nothing to do, nothing launched
    for kw in (dict(R=0), dict(H=0), dict(V=0), dict(tok=None), dict(dy=None), dict(dw=None), dict(p=1.0), dict(wp=1.0), dict(wp=-0.25),
               dict(p=float("nan")), dict(state=None), dict(state=None, p=0.0), dict(state=None, wp=0.0)):
        assert bwd(**kw) == _lib.E_BADARG, kw
    for acc in (0, 1):
        assert bwd(acc=acc, H=1025) == _lib.E_UNSUPPORTED
        assert bwd(acc=acc, scratch=None) == _lib.E_WORKSPACE and bwd(acc=acc, nbytes=need - 1) == _lib.E_WORKSPACE
        assert bwd(acc=acc, H=1025, p=0.0, wp=0.0, state=None) == _lib.E_UNSUPPORTED      # no state needed with both off


def test_with_tying_off_and_no_word_dropout_the_new_code_is_never_entered():
    model = make(dropout=0.5)
    x, y = torch.randint(0, 64, (6, 3)), torch.randint(0, 64, (6, 3))

    class Tripwire(Exception):
        pass

    def trip(*a, **k):
        raise Tripwire
    real = F._embed_ex, F.embedding_dropout_stock, F.tied_gradient, F.EmbedExFn.apply, F.TiedGradient.put
    F._embed_ex = F.embedding_dropout_stock = F.tied_gradient = F.EmbedExFn.apply = F.TiedGradient.put = trip
    try:
        for train in (True, False):
            model.train(train)
            model.zero_grad()
            model.loss(x, y, model.state_init(3))[0].backward()
            model.loss(x, y, model.state_init(3), ar=1.0, label_smoothing=0.1)[0].backward()
            model.distill_loss(x, y, model.state_init(3), torch.randn(6, 3, 64))[0].backward()
            model(x, model.state_init(3))
        model.train()
        model.embed_dropout = 0.5
        with pytest.raises(Tripwire):
            model.loss(x, y, model.state_init(3))
        model.embed_dropout = 0.0
        model.tie_weights()
        with pytest.raises(Tripwire):
            model.loss(x, y, model.state_init(3))
    finally:
        F._embed_ex, F.embedding_dropout_stock, F.tied_gradient, F.EmbedExFn.apply, F.TiedGradient.put = real


# ---- 7. everything that walks the parameters meets the table once ------------------------------------------------------------------
def test_optimizers_and_dynamic_evaluation_move_a_tied_table_once():
    tied, twin = C.twins(make)
    x, y = torch.randint(0, 64, (6, 3)), torch.randint(0, 64, (6, 3))
    params = list(tied.parameters())                       # what clip_sgd_step, optim.Adam and optim.ASGD are handed
    assert sum(p is tied.embed.w for p in params) == 1 and len(params) == len(list(twin.parameters())) - 1
    # one ASGD step: the table moves once, by its one gradient - the step of a plain parameter holding the twin's summed gradient
    opt = vmlmf_amd.optim.ASGD(tied.parameters(), lr=0.5)
    tied.loss(x, y, tied.state_init(3))[0].backward()
    twin.loss(x, y, twin.state_init(3))[0].backward()
    want = (tied.embed.w.detach() - 0.5 * (twin.embed.w.grad + twin.fc.w.grad))
    opt.step()
    assert tied.tied and torch.equal(tied.embed.w.detach(), want) and torch.equal(tied.fc.w, tied.embed.w)
    # dynamic evaluation: statistics and theta0 hold the table once, restore() puts a tied model's bits back
    before = {k: v.clone() for k, v in tied.state_dict().items()}
    de = vmlmf_amd.DynamicEval(tied, lr=0.1, decay=0.01, segment=3)
    assert len(de.params) == len(params) and de.theta0.numel() == sum((p.numel() + 3) // 4 * 4 for p in params)
    de.accumulate(x, y)
    de.finalize()
    de.score(x, y)
    assert not torch.equal(tied.embed.w, before["embed.w"])
    de.restore()
    assert tied.tied and all(torch.equal(v, before[k]) for k, v in tied.state_dict().items())
