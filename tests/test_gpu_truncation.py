"""The truncation samplers on the GPU - min_p, typical_p, epsilon_cutoff, eta_cutoff: vmlmf_truncate_choose (csrc/vmlmf_truncate.hip,
libvmlmf_truncate.so) through decoding.lm_sample(truncation=...), Model.generate and DecodeGraph, against the fp64 statement of the
contract in truncation_cases.py.

A truncated token passes as a filtered token does (test_gpu_generate_filters.py): it lies in the oracle's `hi` set, its z + G is at
least the best of the `lo` set minus the margin, lo <= kept <= hi in size, and where the argmax of z + G over lo and over hi is one
token it is that one, or within the margin of it (vmlmf_decode_oracle.judge).  The share of rows where the two argmaxes differ is
capped on the CPU (test_truncation_cpu.py)."""
import numpy as np
import pytest
import torch

import truncation_cases as T
import vmlmf_decode_oracle as C
from lm_util import DEV, LP_TOL, _on_device, _prompt, _small, _snap, _tied_row

pytestmark = pytest.mark.gpu
CASES = [(shape, name, tau) for shape in T.SHAPES for name in T.SETTINGS for tau in T.TAUS]
IDS = ["x".join(map(str, s)) + f"-{n}-{t}" for s, n, t in CASES]


def _trunc(**kw):
    from vmlmf_amd import Truncation
    return Truncation(**kw)


def _judge_rows(z_rows, G, name, margin, tok, kept, what):
    clear = 0
    for r in range(z_rows.shape[0]):
        lo, hi = T.case_sets(z_rows[r], name, margin)
        assert np.isfinite(z_rows[r][tok[r]]) and kept[r] <= np.isfinite(z_rows[r]).sum()
        clear += T.judge(z_rows[r], G[r], lo, hi, int(tok[r]), int(kept[r]), margin, f"{what} row {r}")
    return clear


# ---- 1. lm_sample alone against the oracle ----
@pytest.mark.parametrize("shape,name,tau", CASES, ids=IDS)
def test_truncated_lm_sample_against_the_oracle(shape, name, tau):
    from vmlmf_amd import lm_sample
    B, H, V = shape
    h, w, b, e = _on_device(B, H, V)
    k, p, kw = T.setting(name, V)
    tok, lp, xn, kept = lm_sample(h, w, b, tau, _snap(), T.STEP, embed=e, top_k=k, top_p=p, truncation=_trunc(**kw), return_kept=True)
    scores, G = T.case_reference(B, H, V)
    margin = 1e-4 / tau
    clear = _judge_rows(scores / tau, G, name, margin, tok.cpu().numpy(), kept.cpu().numpy(), f"{shape} {name} tau {tau}")
    print(f"{shape} {name} tau {tau}: clear {clear} of {B}, kept {kept.min().item()} .. {kept.max().item()}")
    assert clear >= 0.9 * B
    ref = torch.log_softmax(torch.from_numpy(scores), -1).gather(-1, tok.cpu()[:, None])[:, 0]
    err = (lp.cpu().double() - ref).abs().max().item()
    print(f"  max |logprob - log-softmax| {err:.3e}")
    assert err <= 1e-4
    assert torch.equal(xn, e[tok])


# ---- 2. the same under DecodeControls ----
def _case_controls(shape, length=None, finished=None):
    from vmlmf_amd import DecodeControls
    B, _, V = shape
    seen, lb = C.case_controls(*shape)
    c = DecodeControls(B, V, DEV, eos=C.EOS, min_length=C.MIN_LENGTH, repetition_penalty=C.THETA, logit_bias=torch.from_numpy(lb))
    c.seen.copy_(torch.from_numpy(seen.astype(np.uint8)))
    if length is not None:
        c.length.copy_(torch.from_numpy(np.asarray(length, dtype=np.int32)))
    if finished is not None:
        c.finished.copy_(torch.from_numpy(np.asarray(finished, dtype=np.int32)))
    return c


def _state(c):
    return c.seen.cpu().numpy().astype(bool), c.length.cpu().numpy(), c.finished.cpu().numpy()


@pytest.mark.parametrize("shape,name,tau", CASES, ids=IDS)
def test_truncated_lm_sample_under_controls_against_the_oracle(shape, name, tau):
    """case_controls' seen and bias, eos held back below the minimum length: the stages run on the controlled scores, the
    log-probability stays the raw row's, the state moves as next_state says."""
    from vmlmf_amd import lm_sample
    B, H, V = shape
    h, w, b, e = _on_device(B, H, V)
    k, p, kw = T.setting(name, V)
    ctl = _case_controls(shape)
    seen0, length0, fin0 = _state(ctl)
    tok, lp, xn, kept = lm_sample(h, w, b, tau, _snap(), T.STEP, embed=e, top_k=k, top_p=p, truncation=_trunc(**kw), return_kept=True,
                                  controls=ctl)
    scores, c, G = T.case_controlled(B, H, V)
    margin = C.z_margin(tau)
    t = tok.cpu().numpy()
    clear = _judge_rows(c / tau, G, name, margin, t, kept.cpu().numpy(), f"controlled {shape} {name} tau {tau}")
    print(f"controlled {shape} {name} tau {tau}: clear {clear} of {B}, kept {kept.min().item()} .. {kept.max().item()}")
    assert clear >= 0.9 * B
    ref = torch.log_softmax(torch.from_numpy(scores), -1).gather(-1, tok.cpu()[:, None])[:, 0]      # the RAW log-softmax
    assert (lp.cpu().double() - ref).abs().max().item() <= 1e-4
    assert torch.equal(xn, e[tok]) and not (t == C.EOS).any()
    want = C.next_state(seen0, length0, fin0, t, C.EOS)
    got = _state(ctl)
    assert all(np.array_equal(x, y) for x, y in zip(got, want))


@pytest.mark.parametrize("name", ["minp", "typ"])
def test_finished_rows_are_padding_and_rows_finish(name):
    from vmlmf_amd import lm_sample
    shape = (19, 40, 33)
    B, H, V = shape
    h, w, b, e = _on_device(B, H, V)
    k, p, kw = T.setting(name, V)
    rng = np.random.Generator(np.random.PCG64(B))
    length = rng.integers(0, 3, B).astype(np.int32)                     # below, at and past min_length = 1
    finished = (rng.random(B) < 0.3).astype(np.int32)
    ctl = _case_controls(shape, length, finished)
    ctl.logit_bias[C.EOS] = 30.0                                         # eos is every free row's choice by far
    seen0, _, _ = _state(ctl)
    tok, lp, xn, kept = lm_sample(h, w, b, 0.7, _snap(), 1, embed=e, top_k=k, top_p=p, truncation=_trunc(**kw), return_kept=True, controls=ctl)
    t = tok.cpu().numpy()
    want = C.next_state(seen0, length, finished, t, C.EOS)
    assert all(np.array_equal(x, y) for x, y in zip(_state(ctl), want))
    f = torch.from_numpy(finished.astype(bool)).to(DEV)
    assert f.any() and (~f).any()
    assert (tok[f] == C.EOS).all() and (kept[f] == 0).all() and torch.equal(xn[f], e[C.EOS].expand(int(f.sum()), -1))
    assert torch.equal(lp[f], torch.zeros_like(lp[f])) and not torch.signbit(lp[f]).any()           # 0.0 exactly
    live = ~finished.astype(bool)
    assert not (t[live & (length < C.MIN_LENGTH)] == C.EOS).any()       # held back below the minimum length ...
    assert (t[live & (length >= C.MIN_LENGTH)] == C.EOS).all()          # ... free at it: those rows finished here
    assert (kept[~f] >= 1).all() and (lp[~f] < 0).all() and torch.equal(xn, e[tok])


# ---- 3. a truncation that keeps everything is the untruncated call ----
def test_keeping_everything_is_the_untruncated_call_to_the_bit():
    from vmlmf_amd import DecodeControls, lm_sample
    B, H, V = 3, 32, 97
    h, w, b, e = _on_device(B, H, V)
    snap = _snap(5)
    for tau in (0.7, 1.0):
        base = lm_sample(h, w, b, tau, snap, 2, embed=e, form="gemm")
        got = lm_sample(h, w, b, tau, snap, 2, embed=e, truncation=_trunc(min_p=1e-6), return_kept=True)
        for name, x, y in zip(("tokens", "logprob", "x_next"), base, got):
            assert torch.equal(x, y), (tau, name)
        assert (got[3] == V).all()
        # ... under neutral controls too: the controlled untruncated launch
        base = lm_sample(h, w, b, tau, snap, 2, embed=e, controls=DecodeControls(B, V, DEV))
        got = lm_sample(h, w, b, tau, snap, 2, embed=e, truncation=_trunc(min_p=1e-6), return_kept=True, controls=DecodeControls(B, V, DEV))
        assert all(torch.equal(x, y) for x, y in zip(base, got[:3])) and (got[3] == V).all()
    # nothing on, and greedy with everything on: launch for launch the calls of today
    base = lm_sample(h, w, b, 0.7, snap, 2, embed=e, top_k=10, top_p=0.9, return_kept=True)
    got = lm_sample(h, w, b, 0.7, snap, 2, embed=e, top_k=10, top_p=0.9, return_kept=True, truncation=_trunc(min_p=0, typical_p=1.0))
    assert all(torch.equal(x, y) for x, y in zip(base, got))
    base = lm_sample(h, w, b, 0.0, None, 0, embed=e)
    got = lm_sample(h, w, b, 0.0, None, 0, embed=e, truncation=_trunc(min_p=0.5, typical_p=0.2, epsilon_cutoff=0.1, eta_cutoff=0.1))
    assert all(torch.equal(x, y) for x, y in zip(base, got))
    with pytest.raises(ValueError, match="fused"):
        lm_sample(h, w, b, 0.7, snap, 2, embed=e, form="fused", truncation=_trunc(min_p=0.1))


# ---- 4. one token kept ----
def test_one_token_kept():
    from vmlmf_amd import lm_sample
    for shape in ((3, 32, 97), (40, 700, 1000), (2, 16, C.LDS_ROW + 5)):
        h, w, b, e = _on_device(*shape)
        greedy = lm_sample(h, w, b, 0.0, None, 0, embed=e, form="gemm")
        got = lm_sample(h, w, b, 1.0, _snap(9), 1, embed=e, truncation=_trunc(min_p=1.0), return_kept=True)
        assert torch.equal(got[0], greedy[0]) and torch.equal(got[2], greedy[2]) and torch.equal(got[1], greedy[1]), shape
        assert (got[3] == 1).all()
        got = lm_sample(h, w, b, 1.0, _snap(9), 1, embed=e, truncation=_trunc(typical_p=1e-9), return_kept=True)
        assert (got[3] == 1).all()
        scores, _ = T.case_reference(*shape)
        want = [T.exact_set(z, typical_p=1e-9)[0] for z in scores]              # the token nearest the entropy
        near = 0
        for r, z in enumerate(scores):                                           # ... or one as near, within the margin
            p = np.exp(z - z.max())
            p /= p.sum()
            d = np.abs(-np.log(p) + (p * np.log(p)).sum())
            near += abs(d[int(got[0][r])] - d[want[r]]) <= 4e-4
        assert near == shape[0], shape


# ---- 5. ties ----
def test_ties_are_kept_together_or_cut_by_index():
    from vmlmf_amd import lm_sample
    h, w, bias = _tied_row()
    z = (w.double() @ h.double()).numpy()
    assert z[40] == 2.5 and z[5] == z[20] == z[60] == 2.0 and np.sort(z)[-5] <= 1.0
    N = 2048
    hN = h.to(DEV).expand(N, -1).contiguous()
    run = lambda **kw: lm_sample(hN, w.to(DEV), bias.to(DEV), 1.0, _snap(1), 0, return_kept=True, truncation=_trunc(**kw))
    # min_p at the tie group's ratio keeps the whole group; a hair above it, none of it
    a = float(np.exp(-0.5))
    assert T.exact_set(z, min_p=a) == [5, 20, 40, 60]
    tok, _, kept = run(min_p=a)
    assert (kept == 4).all() and sorted(set(tok.cpu().tolist())) == [5, 20, 40, 60]
    tok, _, kept = run(min_p=a * 1.001)
    assert (kept == 1).all() and set(tok.cpu().tolist()) == {40}
    # typical: the three tied tokens share one deviation; a boundary inside the group is cut by index
    p = np.exp(z - z.max())
    p /= p.sum()
    d = np.abs(-np.log(p) + (p * np.log(p)).sum())
    order = np.lexsort((np.arange(97), d))
    pos = {int(v): int(np.flatnonzero(order == v)[0]) for v in (5, 20, 60)}
    assert pos[20] == pos[5] + 1 and pos[60] == pos[5] + 2                      # the group is contiguous in the order, by index
    before5 = p[order[:pos[5]]].sum()
    for n, m in ((1, before5 + 0.5 * p[5]), (2, before5 + 1.5 * p[5]), (3, before5 + 2.5 * p[5])):
        want = T.exact_set(z, typical_p=float(m))
        assert [v for v in (5, 20, 60) if v in want] == [5, 20, 60][:n]
        tok, _, kept = run(typical_p=float(m))
        assert (kept == len(want)).all() and set(tok.cpu().tolist()) <= set(want)
        seen = set(tok.cpu().tolist())
        assert set([5, 20, 60][:n]) <= seen and not (set([5, 20, 60][n:]) & seen)


# ---- 6. frequencies follow the renormalised softmax over the kept set ----
@pytest.mark.parametrize("name,kw", [("minp", dict(min_p=0.1)), ("typ", dict(typical_p=0.9))])
def test_token_frequencies_follow_the_renormalised_softmax(name, kw):
    from vmlmf_amd import lm_sample
    g = torch.Generator().manual_seed(12)
    h = torch.randn(32, generator=g)
    w = torch.randn(97, 32, generator=g) * 0.25
    b = torch.randn(97, generator=g) * 0.5
    z = (w.double() @ h.double() + b.double()).numpy()
    margin = 1e-4
    lo, hi = T.truncated_sets(z, None, None, kw, margin, C.nucleus_eps(1.0, margin, 97))
    assert np.array_equal(lo, hi) and 4 <= lo.sum() <= 60                  # the boundary is unambiguous
    N = 4096
    tok, _, kept = lm_sample(h.to(DEV).expand(N, -1).contiguous(), w.to(DEV), b.to(DEV), 1.0, _snap(0x5EED), 0, return_kept=True,
                             truncation=_trunc(**kw))
    assert (kept == int(lo.sum())).all()
    p = np.where(lo, np.exp(z - z.max()), 0.0)
    p /= p.sum()
    counts = np.bincount(tok.cpu().numpy(), minlength=97)
    assert (counts[~lo] == 0).all()
    sigma = np.sqrt(N * p * (1 - p))
    assert (np.abs(counts - N * p) <= 5 * sigma + 1).all(), np.argwhere(np.abs(counts - N * p) > 5 * sigma + 1)


# ---- 7. reproducibility, Model.generate and graphs ----
def test_two_runs_give_the_same_bits():
    from vmlmf_amd import lm_sample
    for shape in ((40, 700, 1000), (2, 16, C.LDS_ROW + 5)):
        h, w, b, e = _on_device(*shape)
        k, p, kw = T.setting("all", shape[2])
        kw = dict(kw, eta_cutoff=0.1 / shape[2])
        a = lm_sample(h, w, b, 0.7, _snap(3), 4, embed=e, top_k=k, top_p=p, truncation=_trunc(**kw), return_kept=True)
        c = lm_sample(h, w, b, 0.7, _snap(3), 4, embed=e, top_k=k, top_p=p, truncation=_trunc(**kw), return_kept=True)
        assert all(torch.equal(x, y) for x, y in zip(a, c))


def test_generate_truncates_repeats_with_the_seed_and_replays_from_a_graph():
    from vmlmf_amd import DecodeGraph, _truncate
    m = _small("group").eval()
    prompt = _prompt(4, seed=2)
    kw = dict(temperature=1.0, min_p=0.05, typical_p=0.9, eos=7)
    a = m.generate(prompt, 16, seed=11, **kw)
    b = m.generate(prompt, 16, seed=11, **kw)
    assert _truncate.loaded()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])              # the log-probabilities to the bit
    nxt = m.generate(prompt, 16, **kw)
    assert not torch.equal(a[0], nxt[0])
    plain = m.generate(prompt, 16, seed=11, temperature=1.0, eos=7)        # same noise, other tokens somewhere: the stages took part
    assert not torch.equal(plain[0], a[0])
    # a graphed chunk draws the eager call's first 8 tokens
    e = m.generate(prompt, 8, seed=21, return_lengths=True, **kw)
    c = m.generate(prompt, 8, seed=21, chunk=8, return_lengths=True, **kw)
    assert torch.equal(e[0], c[0]) and torch.equal(e[1], c[1]) and torch.equal(e[2], c[2])
    c2 = m.generate(prompt, 16, seed=21, chunk=8, **kw)
    assert torch.equal(c2[0][:8], e[0])
    # rows that emitted eos are padded with it
    t = c2[0].cpu().numpy()
    for r in range(4):
        hit = np.flatnonzero(t[:, r] == 7)
        assert len(hit) == 0 or (t[hit[0]:, r] == 7).all()
    # a DecodeGraph captures the truncated launch; two replays differ
    with torch.no_grad():
        h, st = m.features(prompt, m.state_init(4))
    m.sampler_state(seed=21)
    g = DecodeGraph(m, h[-1], st, 8, temperature=1.0, min_p=0.05, typical_p=0.9)
    t1, l1 = g.replay()
    t2, _ = g.replay()
    ref = m.generate(prompt, 8, seed=21, temperature=1.0, min_p=0.05, typical_p=0.9)
    assert torch.equal(t1, ref[0]) and torch.equal(l1, ref[1]) and not torch.equal(t1, t2)
    assert (l1 < 0).all() and (l1 > -20).all() and LP_TOL > 0
