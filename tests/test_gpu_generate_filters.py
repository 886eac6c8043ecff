"""Top-k and nucleus (top-p) sampling on the GPU: vmlmf_lm_sample_filtered / vmlmf_lm_choose_filtered (csrc/vmlmf_sample.hip) through
decoding.lm_sample, Model.generate and DecodeGraph, against the fp64 oracle of oracle/vmlmf_decode_oracle.py.

A filtered token passes when it lies in the oracle's `hi` set (the tokens possibly kept), its z + G is at least the best of the `lo`
set (the tokens certainly kept) minus the margin, and lo <= kept <= hi in size; where the argmax of z + G over lo and over hi is one
token, the GPU's token is that one, or within the margin of it (vmlmf_decode_oracle.judge)."""
import ctypes

import numpy as np
import pytest
import torch

import vmlmf_decode_oracle as C
from lm_util import DEV, LP_TOL, MARGIN, _on_device, _prompt, _small, _snap, _teacher_forced, _tied_row
from vmlmf_decode_oracle import gumbel_restated

pytestmark = pytest.mark.gpu
# ---- 1. lm_sample alone against the oracle, both forms ----
@pytest.mark.parametrize("form", ["fused", "gemm"])
@pytest.mark.parametrize("tau", C.TAUS)
@pytest.mark.parametrize("name", C.SETTINGS)
@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_lm_sample_filtered_against_the_oracle(shape, name, tau, form):
    from vmlmf_amd import lm_sample
    B, H, V = shape
    h, w, b, e = _on_device(B, H, V)
    k, p = C.setting(name, V)
    tok, lp, xn, kept = lm_sample(h, w, b, tau, _snap(), C.STEP, embed=e, form=form, top_k=k, top_p=p, return_kept=True)
    scores, G = C.case_reference(B, H, V)
    margin = 1e-4 / tau
    tok_c, kept_c = tok.cpu().numpy(), kept.cpu().numpy()
    clear = 0
    for r in range(B):
        z = scores[r] / tau
        lo, hi = C.filtered_sets(z, k, p, margin, C.nucleus_eps(p or 1.0, margin, V))
        clear += C.judge(z, G[r], lo, hi, int(tok_c[r]), int(kept_c[r]), margin, f"{shape} {name} tau {tau} {form} row {r}")
    assert clear >= 0.9 * B                                           # (the oracle's sets alone: see the CPU file's test of it)
    ref = torch.log_softmax(torch.from_numpy(scores), -1).gather(-1, tok.cpu()[:, None])[:, 0]
    assert torch.allclose(lp.cpu().double(), ref, atol=1e-4, rtol=0), (lp.cpu().double() - ref).abs().max()
    assert torch.equal(xn, e[tok])


# ---- 2. filters off: nothing changed ----
@pytest.mark.parametrize("B", [3, 19])
def test_filters_off_is_the_unfiltered_call_to_the_bit(B):
    from vmlmf_amd import _lib, lm_sample
    from vmlmf_amd.functional import sample_ticket
    from vmlmf_amd.decoding import _sample_workspace
    h, w, b, e = _on_device(*{3: (3, 32, 97), 19: (19, 40, 33)}[B])
    H, V = h.shape[1], w.shape[0]
    snap = _snap(5)
    for form in ("fused", "gemm", None):
        for tau in (0.7, 0.0):
            base = lm_sample(h, w, b, tau, snap, 2, embed=e, form=form)
            for kw in (dict(top_k=None, top_p=None), dict(top_k=0), dict(top_k=V), dict(top_k=V + 7), dict(top_p=1.0), dict(top_k=0, top_p=1.0)):
                got = lm_sample(h, w, b, tau, snap, 2, embed=e, form=form, return_kept=True, **kw)
                assert all(torch.equal(x, y) for x, y in zip(base, got[:3])), (form, tau, kw)
                assert (got[3] == V).all()
    # greedy with filters set is accepted and changes nothing
    base = lm_sample(h, w, b, 0.0, None, 0, embed=e)
    got = lm_sample(h, w, b, 0.0, None, 0, embed=e, top_k=5, top_p=0.5)
    assert all(torch.equal(x, y) for x, y in zip(base, got))
    # ... and through the two filtered C ABI functions with (0, 1.0)
    lib = _lib.lib()
    dev = torch.device(DEV, torch.cuda.current_device())
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    base = lm_sample(h, w, b, 0.7, snap, 2, embed=e, form="fused")
    tok, lp, xn = torch.empty_like(base[0]), torch.empty_like(base[1]), torch.empty_like(base[2])
    kept = torch.zeros(B, dtype=torch.int32, device=DEV)
    nbytes = lib.vmlmf_lm_sample_filtered_workspace_bytes(B, V)
    ws = _sample_workspace(dev, nbytes)
    _lib.check(lib.vmlmf_lm_sample_filtered(B, H, V, ptr(h), ptr(w), ptr(b), ptr(e), 1.0 / 0.7, 0, 1.0, ptr(snap), 2, ptr(tok), ptr(lp), ptr(xn),
                                            ptr(kept), ptr(sample_ticket(dev)), ptr(ws), nbytes, _lib.raw_stream(dev)))
    assert torch.equal(tok, base[0]) and torch.equal(lp, base[1]) and torch.equal(xn, base[2]) and (kept == V).all()
    base = lm_sample(h, w, b, 0.7, snap, 2, embed=e, form="gemm")
    scores = torch.mm(h, w.t())
    tok.zero_(), lp.zero_(), xn.zero_()
    _lib.check(lib.vmlmf_lm_choose_filtered(B, H, V, ptr(scores), ptr(b), ptr(e), 1.0 / 0.7, 0, 1.0, ptr(snap), 2, ptr(tok), ptr(lp), ptr(xn),
                                            None, _lib.raw_stream(dev)))
    assert torch.equal(tok, base[0]) and torch.equal(lp, base[1]) and torch.equal(xn, base[2])
    # the ticket is back to zero after every launch, the filtered ones included
    lm_sample(h, w, b, 0.7, snap, 2, embed=e, form="fused", top_k=4, top_p=0.9)
    _lib.check(lib.vmlmf_lm_sample_filtered(B, H, V, ptr(h), ptr(w), None, None, 1.0, 3, 0.5, ptr(snap), 0, ptr(tok), None, None, None,
                                            ptr(sample_ticket(dev)), ptr(ws), nbytes, _lib.raw_stream(dev)))
    assert int(sample_ticket(dev).abs().sum()) == 0
    with pytest.raises(ValueError, match="top_k"):
        lm_sample(h, w, b, 0.7, snap, 2, top_k=-1)
    with pytest.raises(ValueError, match="top_p"):
        lm_sample(h, w, b, 0.7, snap, 2, top_p=0.0)


# ---- 3. degenerate filters are greedy ----
@pytest.mark.parametrize("form", ["fused", "gemm"])
def test_one_token_kept_is_greedy(form):
    from vmlmf_amd import lm_sample
    for shape in ((3, 32, 97), (40, 700, 1000), (2, 16, C.LDS_ROW + 5)):
        h, w, b, e = _on_device(*shape)
        greedy = lm_sample(h, w, b, 0.0, None, 0, embed=e, form=form)
        for kw in (dict(top_k=1), dict(top_p=1e-6)):
            got = lm_sample(h, w, b, 1.0, _snap(9), 1, embed=e, form=form, return_kept=True, **kw)
            assert torch.equal(got[0], greedy[0]) and torch.equal(got[2], greedy[2]), (shape, kw)
            assert torch.allclose(got[1], greedy[1], atol=1e-5)
            assert (got[3] == 1).all()


# ---- 4. ties at the boundary go to the lower index ----
@pytest.mark.parametrize("form", ["fused", "gemm"])
def test_ties_at_the_boundary_go_to_the_lower_index(form):
    from vmlmf_amd import lm_sample
    h, w, bias = _tied_row()
    z = (w.double() @ h.double()).numpy()
    assert z[40] == 2.5 and z[5] == z[20] == z[60] == 2.0 and np.sort(z)[-5] <= 1.0
    N = 2048
    hN = h.to(DEV).expand(N, -1).contiguous()
    tok, _, kept = lm_sample(hN, w.to(DEV), bias.to(DEV), 1.0, _snap(1), 0, form=form, top_k=2, return_kept=True)
    assert (kept == 2).all()
    assert sorted(set(tok.cpu().tolist())) == [5, 40]
    tok, _, kept = lm_sample(hN, w.to(DEV), bias.to(DEV), 1.0, _snap(1), 0, form=form, top_k=3, return_kept=True)
    assert (kept == 3).all() and sorted(set(tok.cpu().tolist())) == [5, 20, 40]
    # top-p with p inside the tie group: the mass before token 20 is below p, the mass before token 60 is not
    m = np.exp(z - z.max())
    p = float((m[40] + 1.5 * m[5]) / m.sum())
    assert C.filtered_sets(z, None, p)[0].nonzero()[0].tolist() == [5, 20, 40]
    tok, _, kept = lm_sample(hN, w.to(DEV), bias.to(DEV), 1.0, _snap(1), 0, form=form, top_p=p, return_kept=True)
    assert (kept == 3).all() and sorted(set(tok.cpu().tolist())) == [5, 20, 40]
    # ... and behind a top-k that cuts the group first: top-k admits tokens 5 and 20, top-p then only token 5
    mk = m[[40, 5, 20]]
    p = float((mk[0] + 0.5 * mk[1]) / mk.sum())
    tok, _, kept = lm_sample(hN, w.to(DEV), bias.to(DEV), 1.0, _snap(1), 0, form=form, top_k=3, top_p=p, return_kept=True)
    assert (kept == 2).all() and sorted(set(tok.cpu().tolist())) == [5, 40]


# ---- 5. frequencies follow the renormalised softmax over the kept set ----
@pytest.mark.parametrize("kw", [dict(top_k=8), dict(top_p=0.8)], ids=["k8", "p0.8"])
@pytest.mark.parametrize("form", ["fused", "gemm"])
def test_token_frequencies_follow_the_renormalised_softmax(form, kw):
    from vmlmf_amd import lm_sample
    g = torch.Generator().manual_seed(12)
    h = torch.randn(32, generator=g)
    w = torch.randn(97, 32, generator=g) * 0.25
    b = torch.randn(97, generator=g) * 0.5
    z = (w.double() @ h.double() + b.double()).numpy()
    margin = 1e-4
    lo, hi = C.filtered_sets(z, kw.get("top_k"), kw.get("top_p"), margin, C.nucleus_eps(kw.get("top_p", 1.0), margin, 97))
    assert np.array_equal(lo, hi) and 4 <= lo.sum() <= 40                  # the boundary is unambiguous
    N = 4096
    tok, _, kept = lm_sample(h.to(DEV).expand(N, -1).contiguous(), w.to(DEV), b.to(DEV), 1.0, _snap(0x5EED), 0, form=form,
                             return_kept=True, **kw)
    assert (kept == int(lo.sum())).all()
    p = np.where(lo, np.exp(z - z.max()), 0.0)
    p /= p.sum()
    counts = np.bincount(tok.cpu().numpy(), minlength=97)
    assert (counts[~lo] == 0).all()
    sigma = np.sqrt(N * p * (1 - p))
    assert (np.abs(counts - N * p) <= 5 * sigma + 1).all(), np.argwhere(np.abs(counts - N * p) > 5 * sigma + 1)


# ---- 6. Model.generate, teacher-forced ----
@pytest.mark.parametrize("B", [3, 40])
@pytest.mark.parametrize("kind", ["plain", "group"])
def test_generate_with_filters_against_the_oracle(kind, B, monkeypatch):
    """B = 3 on the fused form (lm_sample's switch is moved for it: the measured default takes the GEMM form at every width),
    B = 40 on the GEMM form."""
    from vmlmf_amd import decoding
    if B == 3:
        monkeypatch.setattr(decoding, "SAMPLE_FILTERED_FUSED_MAX_ROWS", 4)
    m = _small(kind)
    prompt = _prompt(B, seed=11)
    seed, tau, k, p, steps = 0x0F117E2, 0.7, 10, 0.9, 16
    tokens, logprobs, states = m.generate(prompt, steps, temperature=tau, seed=seed, top_k=k, top_p=p)
    assert tokens.shape == (steps, B) and m.sampler_state().cpu().tolist() == [seed, 1]
    scores, ref_states = _teacher_forced(m, prompt, tokens)
    scores = scores.numpy()
    margin = MARGIN / tau
    t = tokens.cpu().numpy()
    clear = 0
    for j in range(steps):
        G = gumbel_restated(seed, 0, j, B, 97)[1]
        for r in range(B):
            z = scores[j, r] / tau
            lo, hi = C.filtered_sets(z, k, p, margin, C.nucleus_eps(p, margin, 97))
            clear += C.judge(z, G[r], lo, hi, int(t[j, r]), None, margin, f"{kind} B {B} step {j} row {r}")
    assert clear >= 0.9 * steps * B
    lsm = torch.log_softmax(torch.from_numpy(scores), -1).gather(-1, tokens.cpu()[..., None])[..., 0]
    assert torch.allclose(logprobs.cpu().double(), lsm, atol=LP_TOL, rtol=0), (logprobs.cpu().double() - lsm).abs().max()
    for (h, c), (rh, rc) in zip(states, ref_states):
        assert torch.allclose(h.cpu().double(), rh, atol=1e-4) and torch.allclose(c.cpu().double(), rc, atol=1e-4)
    # the filters took part: the unfiltered call from the same seed sees the same noise and draws other tokens somewhere
    plain = m.generate(prompt, steps, temperature=tau, seed=seed)
    assert not torch.equal(plain[0], tokens)


# ---- 7. reproducibility and graphs ----
def test_filtered_draws_repeat_with_the_seed_and_replay_fresh_from_a_graph():
    from vmlmf_amd import DecodeGraph
    m = _small("group").eval()
    prompt = _prompt(4, seed=2)
    kw = dict(temperature=1.0, top_k=10, top_p=0.9)
    a = m.generate(prompt, 16, seed=11, **kw)
    b = m.generate(prompt, 16, seed=11, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])              # the log-probabilities to the bit
    nxt = m.generate(prompt, 16, **kw)
    assert not torch.equal(a[0], nxt[0])
    # a graphed chunk draws the eager call's first 8 tokens
    e = m.generate(prompt, 8, seed=21, **kw)
    c = m.generate(prompt, 8, seed=21, chunk=8, **kw)
    assert torch.equal(e[0], c[0]) and torch.equal(e[1], c[1])
    c2 = m.generate(prompt, 16, seed=21, chunk=8, **kw)
    assert torch.equal(c2[0][:8], e[0])
    # two replays of one DecodeGraph differ
    with torch.no_grad():
        h, st = m.features(prompt, m.state_init(4))
    m.sampler_state(seed=21)
    g = DecodeGraph(m, h[-1], st, 8, temperature=1.0, top_k=10, top_p=0.9)
    t1, _ = g.replay()
    t2, _ = g.replay()
    assert torch.equal(t1, e[0]) and not torch.equal(t1, t2)
    with pytest.raises(ValueError, match="top_p"):
        DecodeGraph(m, h[-1], st, 8, temperature=1.0, top_p=2.0)


def test_a_graphed_chunk_on_the_fused_filtered_form(monkeypatch):
    """The one-launch form with filters captures and replays: its ticket and its score workspace live through a graph."""
    from vmlmf_amd import decoding
    monkeypatch.setattr(decoding, "SAMPLE_FILTERED_FUSED_MAX_ROWS", 4)
    m = _small("plain").eval()
    prompt = _prompt(2, seed=3)
    kw = dict(temperature=0.8, top_k=12, top_p=0.95)
    e = m.generate(prompt, 8, seed=5, **kw)
    c = m.generate(prompt, 8, seed=5, chunk=8, **kw)
    assert torch.equal(e[0], c[0]) and torch.equal(e[1], c[1])
    monkeypatch.setattr(decoding, "SAMPLE_FILTERED_FUSED_MAX_ROWS", 0)
    g = m.generate(prompt, 8, seed=5, **kw)                                # the GEMM form: same noise, scores equal up to fp32 rounding
    assert (g[0] == e[0]).float().mean().item() >= 0.75 and torch.allclose(g[1][g[0] == e[0]], e[1][g[0] == e[0]], atol=1e-4)
