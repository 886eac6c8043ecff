"""Stopping and token controls on the GPU: vmlmf_decode_choose (csrc/vmlmf_decode.hip, libvmlmf_decode.so) through
decoding.lm_sample(controls=...), Model.generate and DecodeGraph, against the fp64 oracle of oracle/vmlmf_decode_oracle.py
(controlled_scores: repetition penalty, logit bias and bans, eos held back below the minimum length) and, for the choice on those
scores, the oracle of the filters (filtered_sets / judge).

A token passes as a filtered token does (test_gpu_generate_filters.py), on the CONTROLLED tempered scores z = c / tau and with the sets
stripped of the tokens at -inf: those are never chosen and never counted in `kept`.  The margin on z is the filter tests' margin times
max(theta, 1 / theta): what the penalty can multiply an fp32 rounding of the raw score by."""
import subprocess
import sys

import numpy as np
import pytest
import torch

import vmlmf_decode_oracle as C
from lm_util import DEV, LP_TOL, MARGIN, _on_device, _prompt, _small, _snap, _teacher_forced
from vmlmf_decode_oracle import gumbel_restated

pytestmark = pytest.mark.gpu
KERNEL_CASES = [(shape, name, tau) for shape in C.SHAPES for name in C.CONTROL_SETTINGS for tau in C.TAUS]
CASE_IDS = ["x".join(map(str, s)) + f"-{n}-{t}" for s, n, t in KERNEL_CASES]


def _case_controls(shape, length=None, finished=None):
    """A fresh DecodeControls of a kernel-level case (their state moves with every launch)."""
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


def _neutral(B, V, zero_bias):
    from vmlmf_amd import DecodeControls
    return DecodeControls(B, V, DEV, logit_bias=torch.zeros(V) if zero_bias else None)


def _sets(z, k, p, margin):
    """filtered_sets on the controlled tempered scores, without the tokens at -inf."""
    lo, hi = C.filtered_sets(z, k, p, margin, C.nucleus_eps(p or 1.0, margin, z.shape[0]))
    fin = np.isfinite(z)
    return lo & fin, hi & fin


def _state(c):
    return c.seen.cpu().numpy().astype(bool), c.length.cpu().numpy(), c.finished.cpu().numpy()


# ---- 1. the controlled choice alone against the oracle ----
@pytest.mark.parametrize("shape,name,tau", KERNEL_CASES, ids=CASE_IDS)
def test_controlled_lm_sample_against_the_oracle(shape, name, tau):
    from vmlmf_amd import lm_sample
    B, H, V = shape
    h, w, b, e = _on_device(B, H, V)
    k, p = C.control_setting(name, V)
    tok, lp, xn, kept = lm_sample(h, w, b, tau, _snap(), C.STEP, embed=e, top_k=k, top_p=p, return_kept=True, controls=_case_controls(shape))
    scores, c, G = C.case_controlled(B, H, V)
    margin = C.z_margin(tau)
    tok_c, kept_c = tok.cpu().numpy(), kept.cpu().numpy()
    clear = 0
    for r in range(B):
        z = c[r] / tau
        lo, hi = _sets(z, k, p, margin)
        assert np.isfinite(z[tok_c[r]]) and kept_c[r] <= np.isfinite(z).sum()       # nothing at -inf is chosen or counted
        clear += C.judge(z, G[r], lo, hi, int(tok_c[r]), int(kept_c[r]), margin, f"{shape} {name} tau {tau} row {r}")
    print(f"{shape} {name} tau {tau}: clear {clear} of {B}")
    assert clear >= 0.9 * B                                            # (the oracle's sets alone: see the CPU file's test of it)
    ref = torch.log_softmax(torch.from_numpy(scores), -1).gather(-1, tok.cpu()[:, None])[:, 0]      # the RAW log-softmax
    err = (lp.cpu().double() - ref).abs().max().item()
    print(f"  max |logprob - raw log-softmax| {err:.3e}")
    assert err <= LP_TOL
    assert torch.equal(xn, e[tok])


# ---- 2. neutral controls are the existing kernels to the bit ----
@pytest.mark.parametrize("shape", [(3, 32, 97), (19, 40, 33), (1, 650, 10000), (2, 16, C.LDS_ROW + 5)], ids=lambda s: "x".join(map(str, s)))
def test_neutral_controls_are_the_existing_kernels_to_the_bit(shape):
    """theta = 1, no or a zero logit_bias, no eos, nothing seen: tokens, log-probabilities, counts and next rows of vmlmf_lm_choose /
    vmlmf_lm_choose_filtered (lm_sample's form "gemm") on the same scores and generator state."""
    from vmlmf_amd import lm_sample
    B, H, V = shape
    h, w, b, e = _on_device(B, H, V)
    snap = _snap(5)
    for tau, kw in ((0.7, dict()), (1.0, dict()), (0.7, dict(top_k=10)), (0.7, dict(top_p=0.9)), (1.0, dict(top_k=V // 2, top_p=0.9)),
                    (0.0, dict()), (0.0, dict(top_k=5, top_p=0.5))):
        base = lm_sample(h, w, b, tau, snap, 2, embed=e, form="gemm", return_kept=True, **kw)
        for zero_bias in (False, True):
            ctl = _neutral(B, V, zero_bias)
            got = lm_sample(h, w, b, tau, snap, 2, embed=e, return_kept=True, controls=ctl, **kw)
            for name, x, y in zip(("tokens", "logprob", "x_next", "kept"), base, got):
                assert torch.equal(x, y), (shape, tau, kw, zero_bias, name)
            assert (ctl.length == 1).all() and not ctl.finished.any() and int(ctl.seen.sum()) == B
    with pytest.raises(ValueError, match="fused"):
        lm_sample(h, w, b, 0.7, snap, 2, embed=e, form="fused", controls=_neutral(B, V, False))


# ---- 3. the state a launch leaves ----
@pytest.mark.parametrize("tau,name", [(0.0, "off"), (1.0, "off"), (0.7, "kp")])
@pytest.mark.parametrize("shape", [(19, 40, 33), (40, 700, 1000)], ids=lambda s: "x".join(map(str, s)))
def test_the_state_follows_the_tokens_and_finished_rows_are_padding(shape, tau, name):
    from vmlmf_amd import lm_sample
    B, H, V = shape
    h, w, b, e = _on_device(B, H, V)
    k, p = C.control_setting(name, V)
    rng = np.random.Generator(np.random.PCG64(B))
    length = rng.integers(0, 3, B).astype(np.int32)                     # below, at and past min_length = 1
    finished = (rng.random(B) < 0.3).astype(np.int32)
    ctl = _case_controls(shape, length, finished)
    # make eos every free row's choice by far, so that rows finish in this launch
    ctl.logit_bias[C.EOS] = 30.0
    seen0, _, _ = _state(ctl)
    tok, lp, xn, kept = lm_sample(h, w, b, tau, _snap(), 1, embed=e, top_k=k, top_p=p, return_kept=True, controls=ctl)
    t = tok.cpu().numpy()
    seen1, length1, fin1 = _state(ctl)
    want = C.next_state(seen0, length, finished, t, C.EOS)
    assert np.array_equal(seen1, want[0]) and np.array_equal(length1, want[1]) and np.array_equal(fin1, want[2])
    f = torch.from_numpy(finished.astype(bool)).to(DEV)
    assert f.any() and (~f).any()
    assert (tok[f] == C.EOS).all() and (kept[f] == 0).all() and torch.equal(xn[f], e[C.EOS].expand(int(f.sum()), -1))
    assert torch.equal(lp[f], torch.zeros_like(lp[f])) and not torch.signbit(lp[f]).any()           # 0.0 exactly
    live = ~finished.astype(bool)
    assert not (t[live & (length < C.MIN_LENGTH)] == C.EOS).any()       # held back below the minimum length ...
    assert (t[live & (length >= C.MIN_LENGTH)] == C.EOS).any()          # ... free at it: rows finished here
    assert (kept[~f] >= 1).all() and (lp[~f] < 0).all() and torch.equal(xn, e[tok])


# ---- 4. bans hold ----
def test_banned_tokens_never_appear_and_eos_waits_for_the_minimum_length():
    from vmlmf_amd import DecodeControls, lm_sample
    B, H, V = 3, 32, 97
    h, w, b, e = _on_device(B, H, V)
    rng = np.random.Generator(np.random.PCG64(97))
    banned = np.sort(rng.permutation(V)[:87])                            # 90 % of the vocabulary
    snap = _snap(77)
    for kw in (dict(), dict(top_k=20), dict(top_p=0.95)):
        ctl = DecodeControls(B, V, DEV, banned_tokens=banned.tolist(), repetition_penalty=1.1)
        toks = torch.stack([lm_sample(h, w, b, 1.5, snap, j, top_k=kw.get("top_k"), top_p=kw.get("top_p"), controls=ctl)[0] for j in range(200)])
        t = toks.cpu().numpy()
        assert not np.isin(t, banned).any(), kw
        assert len(np.unique(t)) > 3                                     # ... and the draw is a draw
        assert (ctl.length == 200).all() and not ctl.seen[:, torch.from_numpy(banned).to(DEV)].any()
    # eos is every step's favourite by far; it is held back while a row has fewer than min_length = 5 tokens, so it comes at the first
    # free step - as the sixth token -, never before the fifth
    eos = int(np.setdiff1d(np.arange(V), banned)[0])
    lb = torch.zeros(V)
    lb[eos] = 30.0
    for tau, kw in ((0.0, dict()), (1.5, dict()), (1.5, dict(top_k=3))):
        ctl = DecodeControls(B, V, DEV, eos=eos, min_length=5, logit_bias=lb, banned_tokens=banned.tolist())
        toks = torch.stack([lm_sample(h, w, b, tau, snap, j, controls=ctl, **kw)[0] for j in range(8)]).cpu().numpy()
        assert not (toks[:5] == eos).any() and (toks[5:] == eos).all(), (tau, kw, toks)
        assert (ctl.length == 6).all() and ctl.finished.all()                 # eos itself counts in the length
        assert not np.isin(toks, banned).any()


# ---- 5. ties go to the lower index ----
@pytest.mark.parametrize("seen_at,unseen_at", [(10, 30), (60, 30)])
def test_a_penalised_score_that_ties_an_unseen_one_goes_to_the_lower_index(seen_at, unseen_at):
    """2.0 seen under theta = 2 is 1.0, as the unseen token's 1.0: exact in fp32, so the index decides."""
    from vmlmf_amd import DecodeControls, lm_sample
    V, N = 97, 64
    g = torch.Generator().manual_seed(6)
    x = torch.randint(-64, 33, (V,), generator=g).float() / 64             # every other score <= 0.5
    x[seen_at], x[unseen_at] = 2.0, 1.0
    h = torch.ones(N, 1, device=DEV)
    w = x[:, None].to(DEV)
    for tau, kw in ((0.0, dict()), (1.0, dict(top_k=1))):
        ctl = DecodeControls(N, V, DEV, repetition_penalty=2.0)
        ctl.seen[:, seen_at] = 1
        tok, lp, kept = lm_sample(h, w, None, tau, _snap(3), 0, return_kept=True, controls=ctl, **kw)
        assert (tok == min(seen_at, unseen_at)).all(), (tau, kw, tok.unique().tolist())
        if kw:
            assert (kept == 1).all()
    # without the penalty the seen token's 2.0 wins wherever it sits
    ctl = DecodeControls(N, V, DEV, repetition_penalty=1.0, logit_bias=torch.zeros(V))
    ctl.seen[:, seen_at] = 1
    assert (lm_sample(h, w, None, 0.0, None, 0, controls=ctl)[0] == seen_at).all()


# ---- 6. frequencies follow the renormalised softmax of the controlled scores ----
@pytest.mark.parametrize("kw", [dict(top_k=8), dict(top_p=0.8), dict()], ids=["k8", "p0.8", "off"])
def test_token_frequencies_follow_the_renormalised_softmax_of_the_controlled_scores(kw):
    from vmlmf_amd import DecodeControls, lm_sample
    g = torch.Generator().manual_seed(12)
    h = torch.randn(32, generator=g)
    w = torch.randn(97, 32, generator=g) * 0.25
    b = torch.randn(97, generator=g) * 0.5
    x = (w.double() @ h.double() + b.double()).numpy()
    rng = np.random.Generator(np.random.PCG64(31))
    seen = rng.random(97) < 0.3
    lb = rng.standard_normal(97).astype(np.float32)
    lb[rng.random(97) < 0.2] = -np.inf
    theta = 1.5
    z = C.controlled_scores(x, seen, theta, lb, None, 0, 0)
    lo, hi = _sets(z, kw.get("top_k"), kw.get("top_p"), C.z_margin(1.0, theta))
    assert np.array_equal(lo, hi) and 4 <= lo.sum() <= 90                  # the boundary is unambiguous
    N = 4096
    ctl = DecodeControls(N, 97, DEV, repetition_penalty=theta, logit_bias=torch.from_numpy(lb))
    ctl.seen.copy_(torch.from_numpy(seen.astype(np.uint8)).expand(N, -1))
    tok, _, kept = lm_sample(h.to(DEV).expand(N, -1).contiguous(), w.to(DEV), b.to(DEV), 1.0, _snap(0x5EED), 0, return_kept=True,
                             controls=ctl, **kw)
    assert (kept == int(lo.sum())).all()
    p = np.where(lo, np.exp(np.where(lo, z, 0.0) - z[lo].max()), 0.0)
    p /= p.sum()
    counts = np.bincount(tok.cpu().numpy(), minlength=97)
    assert (counts[~lo] == 0).all()
    sigma = np.sqrt(N * p * (1 - p))
    assert (np.abs(counts - N * p) <= 5 * sigma + 1).all(), np.argwhere(np.abs(counts - N * p) > 5 * sigma + 1)


# ---- 7. Model.generate, teacher-forced ----
@pytest.mark.parametrize("B", [3, 7])
@pytest.mark.parametrize("kind", ["plain", "group"])
def test_generate_with_controls_against_the_oracle(kind, B):
    m = _small(kind)
    V, eos, banned, theta, min_length = 97, 11, 23, 1.2, 3
    prompt = _prompt(B, seed=13)
    lb = torch.zeros(V)
    lb[eos] = 0.5                                                           # rows do finish within the 12 steps
    seed, tau, k, p, steps = 0xC0DE, 0.7, 10, 0.9, 12
    kw = dict(temperature=tau, seed=seed, top_k=k, top_p=p, eos=eos, min_length=min_length, repetition_penalty=theta, logit_bias=lb,
              banned_tokens=[banned])
    tokens, logprobs, lengths, states = m.generate(prompt, steps, return_lengths=True, **kw)
    assert tokens.shape == (steps, B) and lengths.shape == (B,) and lengths.dtype == torch.int32
    assert m.sampler_state().cpu().tolist() == [seed, 1]
    scores, ref_states = _teacher_forced(m, prompt, tokens)                 # over the GPU's own history, padding included
    scores = scores.numpy()
    lbn = lb.numpy().astype(np.float64)
    lbn[banned] = -np.inf
    margin = MARGIN * max(theta, 1 / theta) / tau
    t, lp = tokens.cpu().numpy(), logprobs.cpu().double().numpy()
    seen = np.zeros((B, V), bool)
    seen[np.arange(B)[None, :], prompt.cpu().numpy()] = True
    length, finished = np.zeros(B, np.int64), np.zeros(B, np.int64)
    clear = live = 0
    for j in range(steps):
        G = gumbel_restated(seed, 0, j, B, V)[1]
        c = C.controlled_scores(scores[j], seen, theta, lbn, eos, min_length, length)
        lsm = torch.log_softmax(torch.from_numpy(scores[j]), -1).numpy()
        for r in range(B):
            if finished[r]:
                assert t[j, r] == eos and lp[j, r] == 0.0, (j, r)
                continue
            z = c[r] / tau
            lo, hi = _sets(z, k, p, margin)
            clear += C.judge(z, G[r], lo, hi, int(t[j, r]), None, margin, f"{kind} B {B} step {j} row {r}")
            live += 1
            assert abs(lp[j, r] - lsm[r, t[j, r]]) <= LP_TOL, (j, r, lp[j, r], lsm[r, t[j, r]])
        seen, length, finished = C.next_state(seen, length, finished, t[j], eos)
    print(f"{kind} B {B}: clear {clear} of {live} live choices; lengths {length.tolist()}")
    assert clear >= 0.9 * live
    assert not (t == banned).any()
    assert np.array_equal(lengths.cpu().numpy(), length) and finished.any() and (length[finished == 1] > min_length).all()
    for r in range(B):                                                      # the padding follows the tokens
        assert (t[length[r]:, r] == eos).all() and (t[:length[r] - 1, r] != eos).all()
    for (h, cc), (rh, rc) in zip(states, ref_states):
        assert torch.allclose(h.cpu().double(), rh, atol=1e-4) and torch.allclose(cc.cpu().double(), rc, atol=1e-4)
    out = m.generate(prompt, steps, **kw)
    assert len(out) == 3 and torch.equal(out[0], tokens) and torch.equal(out[1], logprobs)
    # the controls took part: the plain call from the same seed sees the same noise and draws other tokens somewhere
    plain = m.generate(prompt, steps, temperature=tau, seed=seed, top_k=k, top_p=p, return_lengths=True)
    assert len(plain) == 4 and not torch.equal(plain[0], tokens) and (plain[2] == steps).all()


# ---- 8. graphs ----
def test_chunked_greedy_is_the_eager_call_and_a_graph_continues_one_decode():
    from vmlmf_amd import DecodeControls, DecodeGraph
    m = _small("group").eval()
    B, V, eos = 4, 97, 11
    prompt = _prompt(B, seed=2)
    lb = torch.zeros(V)
    lb[eos] = 1.5
    ctl = dict(eos=eos, min_length=2, repetition_penalty=1.3, logit_bias=lb, banned_tokens=[5, 6])
    e = m.generate(prompt, 12, temperature=0.0, return_lengths=True, **ctl)
    c = m.generate(prompt, 12, temperature=0.0, chunk=4, return_lengths=True, **ctl)
    assert all(torch.equal(x, y) for x, y in zip(e[:3], c[:3]))             # tokens, log-probabilities and lengths to the bit
    assert all(torch.equal(x, y) for s, u in zip(e[3], c[3]) for x, y in zip(s, u))
    # sampling: the same seed repeats, the next call draws fresh tokens; a graphed chunk draws the eager call's first tokens
    kw = dict(temperature=1.0, top_k=10, top_p=0.9, **ctl)
    a = m.generate(prompt, 8, seed=11, **kw)
    b = m.generate(prompt, 8, seed=11, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], m.generate(prompt, 8, **kw)[0])
    g8 = m.generate(prompt, 8, seed=11, chunk=8, **kw)
    assert torch.equal(g8[0], a[0]) and torch.equal(g8[1], a[1])
    # one DecodeGraph, three replays: one decode goes on
    with torch.no_grad():
        h, st = m.features(prompt, m.state_init(B))
    m.sampler_state(seed=11)
    controls = DecodeControls(B, V, DEV, prompt=prompt, **ctl)
    seen_prompt = controls.seen.clone()
    g = DecodeGraph(m, h[-1], st, 8, temperature=1.0, top_k=10, top_p=0.9, controls=controls)
    assert torch.equal(controls.seen, seen_prompt) and not controls.length.any()       # the warm-up ran on a clone
    prev_seen, prev_fin, prev_len = controls.seen.clone(), controls.finished.clone(), controls.length.clone()
    toks = []
    for i in range(3):
        t, lp = g.replay()
        toks.append(t)
        if i == 0:
            assert torch.equal(t, a[0]) and torch.equal(lp, a[1])
        fin_before = prev_fin.bool()
        assert (t[:, fin_before] == eos).all() and (lp[:, fin_before] == 0).all()       # finished rows stay finished
        assert (controls.finished >= prev_fin).all() and (controls.seen >= prev_seen).all() and (controls.length >= prev_len).all()
        assert torch.equal(controls.length[fin_before], prev_len[fin_before])
        prev_seen, prev_fin, prev_len = controls.seen.clone(), controls.finished.clone(), controls.length.clone()
    assert not torch.equal(toks[0], toks[1])
    all_t = torch.cat([prompt] + toks)
    want = torch.zeros_like(controls.seen).scatter_(1, all_t.t().contiguous(), 1)
    live_rows = ~controls.finished.bool()
    assert torch.equal(controls.seen[live_rows], want[live_rows]) and (controls.seen <= want).all()
    assert (controls.length[live_rows] == 24).all()


# ---- 9. determinism ----
@pytest.mark.parametrize("shape,name,tau", KERNEL_CASES, ids=CASE_IDS)
def test_the_same_bits_three_times_over(shape, name, tau):
    from vmlmf_amd import lm_sample
    B, H, V = shape
    h, w, b, e = _on_device(B, H, V)
    k, p = C.control_setting(name, V)
    snap = _snap()
    runs = []
    for _ in range(3):
        ctl = _case_controls(shape)
        runs.append(lm_sample(h, w, b, tau, snap, C.STEP, embed=e, top_k=k, top_p=p, return_kept=True, controls=ctl) + (ctl.seen, ctl.length))
    for other in runs[1:]:
        assert all(torch.equal(x, y) for x, y in zip(runs[0], other))


def test_a_plain_generate_never_opens_the_library():
    code = ("import sys; sys.path[:0] = %r\n"
            "import torch, vmlmf_amd\nfrom vmlmf_amd import _decode\n"
            "from lm_util import _small, _prompt\n"
            "m = _small('plain')\n"
            "m.generate(_prompt(3), 4, temperature=0.8, seed=1, top_k=5)\nm.generate(_prompt(3), 4, temperature=0.0, chunk=2)\n"
            "torch.cuda.synchronize()\n"
            "assert not _decode.loaded() and 'libvmlmf_decode.so' not in open('/proc/self/maps').read()\n"
            "out = m.generate(_prompt(3), 4, temperature=0.8, seed=1, top_k=5, eos=3, return_lengths=True)\n"
            "torch.cuda.synchronize()\nassert _decode.loaded() and len(out) == 4\n") % [p for p in sys.path if p]
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
