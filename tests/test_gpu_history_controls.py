"""History controls on the GPU: vmlmf_history_choose and vmlmf_history_bans (csrc/vmlmf_history.hip, libvmlmf_history.so) through
decoding.lm_sample(controls=HistoryControls), _history.history_bans, Model.generate and DecodeGraph, against the numpy statement of
the contract in history_cases.py (ban_set, history_scores) and, for the choice on those scores, the reference of the filters
(vmlmf_decode_oracle: filtered_sets / judge).

The ban sets are compared exactly.  A token passes as a controlled token does (test_gpu_decode_controls.py), on the tempered history
scores z = c / tau with the sets stripped of the tokens at -inf; the margin on z is that test's, z_margin(tau): the penalty terms
alpha count and beta add an fp32 rounding of a score of order 1 to 10, three orders below the margin's base of 1e-4."""
import subprocess
import sys

import numpy as np
import pytest
import torch

import history_cases as HC
import vmlmf_decode_oracle as C
from lm_util import DEV, LP_TOL, MARGIN, _check_choices, _on_device, _prompt, _small, _snap, _teacher_forced

pytestmark = pytest.mark.gpu
KERNEL_CASES = [(shape, name, tau) for shape in C.SHAPES for name in C.CONTROL_SETTINGS for tau in C.TAUS]
CASE_IDS = ["x".join(map(str, s)) + f"-{n}-{t}" for s, n, t in KERNEL_CASES]
SHAPE_IDS = lambda s: "x".join(map(str, s))


def _case_controls(shape, neutral=False, finished=None, capacity=HC.HIST_LEN + 1, **kw):
    """A fresh HistoryControls of a kernel-level case (their state moves with every launch); neutral: the history's controls off, the
    history, the counts and everything else as in the case."""
    from vmlmf_amd import HistoryControls
    B, _, V = shape
    seen, lb = C.case_controls(*shape)
    hist, count, seqs = HC.case_history(*shape)
    args = dict() if neutral else dict(no_repeat_ngram_size=HC.N_GRAM, banned_sequences=seqs, frequency_penalty=HC.ALPHA, presence_penalty=HC.BETA)
    args.update(kw)
    c = HistoryControls(B, V, DEV, eos=C.EOS, min_length=C.MIN_LENGTH, repetition_penalty=C.THETA, logit_bias=torch.from_numpy(lb),
                        capacity=capacity, prompt=torch.from_numpy(hist[:, :HC.PROMPT_LEN].T.copy()), **args)
    assert c.hist_len.tolist() == [HC.PROMPT_LEN] * B and torch.equal(c.hist[:, :HC.PROMPT_LEN].cpu(), torch.from_numpy(hist[:, :HC.PROMPT_LEN]).int())
    c.hist[:, :HC.HIST_LEN] = torch.from_numpy(hist).to(DEV, torch.int32)
    c.hist_len.fill_(HC.HIST_LEN)
    c.count.copy_(torch.from_numpy(count.astype(np.uint16)))
    c.seen.copy_(torch.from_numpy(seen.astype(np.uint8)))
    if finished is not None:
        c.finished.copy_(torch.from_numpy(np.asarray(finished, dtype=np.int32)))
    return c


def _sets(z, k, p, margin):
    """filtered_sets on the tempered history scores, without the tokens at -inf."""
    lo, hi = C.filtered_sets(z, k, p, margin, C.nucleus_eps(p or 1.0, margin, z.shape[0]))
    fin = np.isfinite(z)
    return lo & fin, hi & fin


def _state(c):
    """Every state buffer, on the host (count as int64)."""
    return dict(seen=c.seen.cpu().numpy().astype(bool), length=c.length.cpu().numpy(), finished=c.finished.cpu().numpy(),
                hist=c.hist.cpu().numpy(), hist_len=c.hist_len.cpu().numpy(), count=_count(c),
                overflow=c.overflow.cpu().numpy())


def _count(c):
    return c.count.cpu().numpy().astype(np.int64)


def _bans(c):
    from vmlmf_amd import _history
    return HC.unpack(_history.history_bans(c).cpu().numpy(), c.V)


# ---- 1. the ban bitmaps, exactly ----
@pytest.mark.parametrize("shape", C.SHAPES, ids=SHAPE_IDS)
def test_the_ban_bitmaps_of_the_kernel_cases_exactly(shape):
    B, _, V = shape
    finished = np.zeros(B, np.int32)
    finished[B // 2] = B > 1
    ctl = _case_controls(shape, finished=finished)
    before = _state(ctl)
    got = _bans(ctl)
    want = HC.case_bans(*shape).copy()
    want[finished.astype(bool)] = False                                      # a finished row gets zeros
    assert want.any() and np.array_equal(got, want), np.argwhere(got != want)[:8]
    after = _state(ctl)
    assert all(np.array_equal(before[k], after[k]) for k in before)           # nothing of the state moves


@pytest.mark.parametrize("n,seqs,hists", HC.EDGES, ids=[str(i) for i in range(len(HC.EDGES))])
def test_the_ban_bitmaps_of_the_edge_histories_exactly(n, seqs, hists):
    from vmlmf_amd import HistoryControls
    V, cap = HC.EDGE_V, 8
    ctl = HistoryControls(len(hists), V, DEV, no_repeat_ngram_size=n, banned_sequences=seqs, capacity=cap)
    rows = np.full((len(hists), cap), V - 1, dtype=np.int32)                  # (what lies past a row's length is never matched)
    for r, h in enumerate(hists):
        rows[r, :len(h)] = h
    ctl.hist.copy_(torch.from_numpy(rows))
    ctl.hist_len.copy_(torch.tensor([len(h) for h in hists], dtype=torch.int32))
    got = _bans(ctl)
    for r, h in enumerate(hists):
        want = HC.ban_set(h, V, n, seqs)
        assert np.array_equal(got[r], want), (n, seqs, h, np.flatnonzero(got[r]).tolist(), np.flatnonzero(want).tolist())


def test_a_full_history_is_never_written_past():
    from vmlmf_amd import lm_sample
    shape = (19, 40, 33)
    B, H, V = shape
    h, w, b, e = _on_device(B, H, V)
    ctl = _case_controls(shape, capacity=HC.HIST_LEN)                         # full: 24 of 24
    guard = torch.full((B * HC.HIST_LEN + 1,), -7, dtype=torch.int32, device=DEV)
    guard[:-1] = ctl.hist.reshape(-1)
    ctl.hist = guard[:-1].view(B, HC.HIST_LEN)
    ctl.finished[3] = 1
    before = _state(ctl)
    bans = _bans(ctl)
    tok = lm_sample(h, w, b, 0.0, None, 0, controls=ctl)[0].cpu().numpy()
    after = _state(ctl)
    assert int(guard[-1]) == -7 and np.array_equal(after["hist"], before["hist"]) and np.array_equal(after["hist_len"], before["hist_len"])
    live = before["finished"] == 0
    assert np.array_equal(after["overflow"], live.astype(np.int32))           # set for the live rows, not for the finished one
    assert not bans[np.arange(B)[live], tok[live]].any()                      # the bans of the full history still held
    assert np.array_equal(after["length"], before["length"] + live) and after["count"].sum() == before["count"].sum() + live.sum()


# ---- 2. the choice against the reference ----
@pytest.mark.parametrize("shape,name,tau", KERNEL_CASES, ids=CASE_IDS)
def test_history_lm_sample_against_the_reference(shape, name, tau):
    from vmlmf_amd import lm_sample
    B, H, V = shape
    h, w, b, e = _on_device(B, H, V)
    k, p = C.control_setting(name, V)
    tok, lp, xn, kept = lm_sample(h, w, b, tau, _snap(), C.STEP, embed=e, top_k=k, top_p=p, return_kept=True, controls=_case_controls(shape))
    scores, c, G, bans = HC.case_scores(B, H, V)
    margin = C.z_margin(tau)
    tok_c, kept_c = tok.cpu().numpy(), kept.cpu().numpy()
    clear = 0
    for r in range(B):
        z = c[r] / tau
        lo, hi = _sets(z, k, p, margin)
        assert not bans[r, tok_c[r]] and np.isfinite(z[tok_c[r]]) and kept_c[r] <= np.isfinite(z).sum()    # nothing banned is chosen or counted
        clear += C.judge(z, G[r], lo, hi, int(tok_c[r]), int(kept_c[r]), margin, f"{shape} {name} tau {tau} row {r}")
    print(f"{shape} {name} tau {tau}: clear {clear} of {B}")
    assert clear >= 0.9 * B                                            # (the reference's sets alone: see the CPU file's test of it)
    ref = torch.log_softmax(torch.from_numpy(scores), -1).gather(-1, tok.cpu()[:, None])[:, 0]      # the RAW log-softmax
    err = (lp.cpu().double() - ref).abs().max().item()
    print(f"  max |logprob - raw log-softmax| {err:.3e}")
    assert err <= LP_TOL
    assert torch.equal(xn, e[tok])


# ---- 3. neutral history controls are vmlmf_decode_choose to the bit ----
@pytest.mark.parametrize("shape", [(3, 32, 97), (19, 40, 33), (1, 650, 10000), (2, 16, C.LDS_ROW + 5)], ids=SHAPE_IDS)
def test_neutral_history_controls_are_the_controlled_choice_to_the_bit(shape):
    """n = 0, no sequences, alpha = beta = 0 - over the case's eos, theta, bias and seen, a history and NONZERO counts: tokens,
    log-probabilities, next rows, kept, seen, finished and length of lm_sample(controls=DecodeControls(the same))."""
    from vmlmf_amd import DecodeControls, lm_sample
    B, H, V = shape
    h, w, b, e = _on_device(B, H, V)
    seen, lb = C.case_controls(*shape)
    snap = _snap(5)
    rng = np.random.Generator(np.random.PCG64(B + V))
    for tau, kw in ((0.7, dict()), (1.0, dict()), (0.7, dict(top_k=10)), (0.7, dict(top_p=0.9)), (1.0, dict(top_k=V // 2, top_p=0.9)),
                    (0.0, dict()), (0.0, dict(top_k=5, top_p=0.5))):
        length = rng.integers(0, 3, B).astype(np.int32)
        finished = (rng.random(B) < 0.3).astype(np.int32)
        base_ctl = DecodeControls(B, V, DEV, eos=C.EOS, min_length=C.MIN_LENGTH, repetition_penalty=C.THETA, logit_bias=torch.from_numpy(lb))
        ctl = _case_controls(shape, neutral=True, finished=finished)
        assert _count(ctl).sum() == B * (HC.HIST_LEN - HC.PROMPT_LEN)
        for c in (base_ctl, ctl):
            c.seen.copy_(torch.from_numpy(seen.astype(np.uint8)))
            c.length.copy_(torch.from_numpy(length))
            c.finished.copy_(torch.from_numpy(finished))
        base = lm_sample(h, w, b, tau, snap, 2, embed=e, return_kept=True, controls=base_ctl, **kw)
        got = lm_sample(h, w, b, tau, snap, 2, embed=e, return_kept=True, controls=ctl, **kw)
        for name, x, y in zip(("tokens", "logprob", "x_next", "kept"), base, got):
            assert torch.equal(x, y), (shape, tau, kw, name)
        for name in ("seen", "finished", "length"):
            assert torch.equal(getattr(base_ctl, name), getattr(ctl, name)), (shape, tau, kw, name)
    with pytest.raises(ValueError, match="fused"):
        lm_sample(h, w, b, 0.7, snap, 2, embed=e, form="fused", controls=_case_controls(shape))


# ---- 4. bans that bite ----
def test_a_token_that_completes_a_repeated_bigram_or_a_banned_sequence_is_not_chosen():
    from vmlmf_amd import HistoryControls, lm_sample
    shape = (19, 40, 33)
    B, H, V = shape
    h, w, b, e = _on_device(B, H, V)
    hist = HC.case_history(*shape)[0].copy()
    last, t, u, x = [v for v in range(V) if v not in set(hist.ravel().tolist())][:4]      # four tokens the case's histories do not hold
    hist[:, 2], hist[:, 3], hist[:, 4], hist[:, -2], hist[:, -1] = x, last, t, u, last    # every row holds "x last t" and ends in "u last"
    lb = torch.zeros(V)
    lb[t] = 30.0

    def run(**kw):
        ctl = HistoryControls(B, V, DEV, logit_bias=lb, capacity=HC.HIST_LEN + 1, prompt=torch.from_numpy(hist.T.copy()), **kw)
        assert (ctl.hist_len == HC.HIST_LEN).all()
        return lm_sample(h, w, b, 0.0, None, 0, controls=ctl)[0].cpu().numpy(), ctl

    assert (run()[0] == t).all() and (run(no_repeat_ngram_size=3)[0] == t).all()          # ("u last t" stood nowhere before)
    for kw in (dict(no_repeat_ngram_size=2), dict(banned_sequences=[[last, t]]), dict(banned_sequences=[[x, x], [u, last, t]])):
        tok, ctl = run(**kw)
        assert not (tok == t).any(), kw
        for r in range(B):
            assert not HC.ban_set(hist[r], V, kw.get("no_repeat_ngram_size", 0), kw.get("banned_sequences", []))[tok[r]]
        assert torch.equal(ctl.hist[:, -1].cpu(), torch.from_numpy(tok).int())
    assert (run(banned_sequences=[[t, last, t]])[0] == t).all()                            # a sequence the rows do not end in


# ---- 5. the state a launch leaves ----
@pytest.mark.parametrize("tau,name", [(0.0, "off"), (1.0, "off"), (0.7, "kp")])
@pytest.mark.parametrize("shape", [(19, 40, 33), (40, 700, 1000)], ids=SHAPE_IDS)
def test_the_state_follows_the_tokens_and_finished_rows_do_not_move(shape, tau, name):
    from vmlmf_amd import lm_sample
    B, H, V = shape
    h, w, b, e = _on_device(B, H, V)
    k, p = C.control_setting(name, V)
    rng = np.random.Generator(np.random.PCG64(B))
    finished = (rng.random(B) < 0.3).astype(np.int32)
    seqs = [q for q in HC.case_history(*shape)[2] if q != [C.EOS]]                    # (at V = 33 the case's one-token sequence is eos itself)
    ctl = _case_controls(shape, finished=finished, banned_sequences=seqs)
    ctl.length.copy_(torch.from_numpy(rng.integers(1, 3, B).astype(np.int32)))       # at and past min_length: eos is free
    ctl.logit_bias[C.EOS] = 30.0                                                      # ... and some rows finish in this launch
    s0 = _state(ctl)
    tok, lp, xn, kept = lm_sample(h, w, b, tau, _snap(), 1, embed=e, top_k=k, top_p=p, return_kept=True, controls=ctl)
    t = tok.cpu().numpy()
    s1 = _state(ctl)
    seen, length, fin = C.next_state(s0["seen"], s0["length"], s0["finished"], t, C.EOS)
    hist, count = HC.next_history([row[:HC.HIST_LEN] for row in s0["hist"]], s0["count"], finished, t)
    assert np.array_equal(s1["seen"], seen) and np.array_equal(s1["length"], length) and np.array_equal(s1["finished"], fin)
    assert np.array_equal(s1["count"], count) and np.array_equal(s1["hist_len"], [len(row) for row in hist]) and not s1["overflow"].any()
    for r in range(B):
        assert s1["hist"][r, :len(hist[r])].tolist() == hist[r] and np.array_equal(s1["hist"][r, len(hist[r]):], s0["hist"][r, len(hist[r]):])
    f = finished.astype(bool)
    assert f.any() and (~f).any() and (t[f] == C.EOS).all() and (kept.cpu().numpy()[f] == 0).all()
    assert torch.equal(lp[torch.from_numpy(f).to(DEV)], torch.zeros(int(f.sum()), device=DEV)) and torch.equal(xn, e[tok])
    assert (fin[~f] == (t[~f] == C.EOS)).all() and fin[~f].any()


def test_the_count_saturates():
    from vmlmf_amd import HistoryControls, lm_sample
    B, H, V = 3, 32, 97
    h, w, b, e = _on_device(B, H, V)
    lb = torch.zeros(V)
    lb[40] = 30.0
    ctl = HistoryControls(B, V, DEV, logit_bias=lb, frequency_penalty=0.0, capacity=4)
    preset = np.zeros((B, V), dtype=np.uint16)
    preset[0, 40], preset[1, 40] = 65535, 65534
    ctl.count.copy_(torch.from_numpy(preset))
    for j in range(2):
        assert (lm_sample(h, w, b, 0.0, None, j, controls=ctl)[0] == 40).all()
    assert _count(ctl)[:, 40].tolist() == [65535, 65535, 2] and _count(ctl).sum() == 2 * 65535 + 2
    assert ctl.hist[:, :2].eq(40).all() and (ctl.hist_len == 2).all()


# ---- 6. Model.generate ----
def _no_ngram_twice(prompt, tokens, n):
    """No n-gram that ends in a generated token stood earlier in the row."""
    seq = torch.cat([prompt.cpu(), tokens.cpu()]).numpy()
    T0 = prompt.shape[0]
    for r in range(seq.shape[1]):
        row = seq[:, r].tolist()
        grams = [tuple(row[i:i + n]) for i in range(len(row) - n + 1)]
        for i in range(max(T0 - n + 1, 0), len(grams)):
            if grams[i] in grams[:i]:
                return False
    return True


def _reference_walk(m, prompt, tokens, lb, theta=1.0, alpha=0.0, beta=0.0, n=0, seqs=()):
    """The fp64 history scores (steps, B, V) along the GPU's own tokens (teacher-forced layers; state by next_state / next_history), the
    counts at the end, the raw scores and the layers' final states."""
    raw, ref_states = _teacher_forced(m, prompt, tokens)
    scores, t = raw.numpy(), tokens.cpu().numpy()
    steps, B = t.shape
    V = scores.shape[-1]
    seen = np.zeros((B, V), bool)
    seen[np.arange(B)[None, :], prompt.cpu().numpy()] = True
    hist, count = [row.tolist() for row in prompt.cpu().numpy().T], np.zeros((B, V), np.int64)
    length, finished = np.zeros(B, np.int64), np.zeros(B, np.int64)
    out = []
    for j in range(steps):
        bans = np.stack([HC.ban_set(hist[r], V, n, list(seqs)) for r in range(B)])
        out.append(HC.history_scores(scores[j], seen, count, theta, alpha, beta, lb, None, 0, length, bans))
        hist, count = HC.next_history(hist, count, finished, t[j])
        seen, length, finished = C.next_state(seen, length, finished, t[j], None)
    return torch.from_numpy(np.stack(out)), count, raw, ref_states


@pytest.mark.parametrize("B", [3, 7])
@pytest.mark.parametrize("kind", ["plain", "group"])
def test_generate_with_history_controls_against_the_reference(kind, B):
    m = _small(kind)
    V, steps, ta, tb = 97, 12, 20, 50
    prompt = _prompt(B, seed=13)
    lb = torch.zeros(V)
    lb[ta] = lb[tb] = 10.0
    lbn = lb.double().numpy()
    margin = MARGIN                                                          # greedy, theta = 1: the model-level test's margin on the scores
    plain = m.generate(prompt, steps, temperature=0.0, logit_bias=lb)[0]
    p = plain.cpu().numpy()
    assert np.isin(p, [ta, tb]).all()                                        # the plain output alternates between the two ...
    for r in range(B):                                                       # ... and repeats a bigram within six steps
        grams = [tuple(p[i:i + 2, r]) for i in range(5)]
        assert len(set(grams)) < len(grams)
    assert not _no_ngram_twice(prompt, plain, 2) and not _no_ngram_twice(prompt, plain, 3)
    for n in (2, 3):
        tokens, logprobs, states = m.generate(prompt, steps, temperature=0.0, logit_bias=lb, no_repeat_ngram_size=n)
        assert tokens.shape == (steps, B) and not torch.equal(tokens, plain)
        assert _no_ngram_twice(prompt, tokens, n), (kind, B, n, tokens.t().tolist())
        c, _, raw, ref_states = _reference_walk(m, prompt, tokens, lbn, n=n)
        _check_choices(c, tokens, margin, f"{kind} B {B} n {n}")
        lsm = torch.log_softmax(raw, -1).gather(-1, tokens.cpu()[..., None])[..., 0]
        assert (logprobs.cpu().double() - lsm).abs().max().item() <= LP_TOL
        for (hh, cc), (rh, rc) in zip(states, ref_states):
            assert torch.allclose(hh.cpu().double(), rh, atol=1e-4) and torch.allclose(cc.cpu().double(), rc, atol=1e-4)
    # a banned sequence - the plain output's first two tokens of row 0 - never comes
    s0, s1 = int(p[0, 0]), int(p[1, 0])
    tokens = m.generate(prompt, steps, temperature=0.0, logit_bias=lb, banned_sequences=[[s0, s1]])[0]
    seq = torch.cat([prompt, tokens]).cpu().numpy()
    assert not ((seq[:-1] == s0) & (seq[1:] == s1))[prompt.shape[0] - 1:].any() and not torch.equal(tokens[:, 0], plain[:, 0])
    _check_choices(_reference_walk(m, prompt, tokens, lbn, seqs=([s0, s1],))[0], tokens, margin, f"{kind} B {B} sequence")
    # the penalties alone: after three of a token its ten points are gone
    for kw in (dict(frequency_penalty=4.0), dict(frequency_penalty=1.5, presence_penalty=6.0, repetition_penalty=1.2)):
        tokens = m.generate(prompt, steps, temperature=0.0, logit_bias=lb, **kw)[0]
        assert not torch.equal(tokens, plain), kw
        theta = kw.get("repetition_penalty", 1.0)
        c, count, _, _ = _reference_walk(m, prompt, tokens, lbn, theta=theta, alpha=kw["frequency_penalty"], beta=kw.get("presence_penalty", 0.0))
        _check_choices(c, tokens, margin * max(theta, 1 / theta), f"{kind} B {B} {kw}")
        assert count.sum() == steps * B and count.max() < np.bincount(p.ravel()).max() // B      # no token as often as the plain favourite


def test_chunked_greedy_is_the_eager_call_and_a_graph_continues_one_history():
    from vmlmf_amd import DecodeGraph, HistoryControls
    m = _small("group").eval()
    B, V = 4, 97
    prompt = _prompt(B, seed=2)
    T0 = prompt.shape[0]
    lb = torch.zeros(V)
    lb[20] = lb[50] = 10.0
    kw = dict(logit_bias=lb, no_repeat_ngram_size=2, banned_sequences=[[50, 20]], frequency_penalty=0.5, presence_penalty=0.25, eos=11, min_length=2)
    e = m.generate(prompt, 16, temperature=0.0, return_lengths=True, **kw)
    c = m.generate(prompt, 16, temperature=0.0, chunk=4, return_lengths=True, **kw)
    assert all(torch.equal(x, y) for x, y in zip(e[:3], c[:3]))             # tokens, log-probabilities and lengths to the bit
    assert all(torch.equal(x, y) for s, u in zip(e[3], c[3]) for x, y in zip(s, u))
    # sampling: a graphed chunk draws the eager call's tokens from the same seed
    skw = dict(temperature=1.0, top_k=10, top_p=0.9, **kw)
    a = m.generate(prompt, 8, seed=11, **skw)
    g8 = m.generate(prompt, 8, seed=11, chunk=8, **skw)
    assert torch.equal(g8[0], a[0]) and torch.equal(g8[1], a[1])
    # one DecodeGraph, two replays: one history goes on
    with torch.no_grad():
        h, st = m.features(prompt, m.state_init(B))
    controls = HistoryControls(B, V, DEV, prompt=prompt, capacity=T0 + 16, **kw)
    g = DecodeGraph(m, h[-1], st, 8, temperature=0.0, controls=controls)
    assert (controls.hist_len == T0).all() and not controls.length.any() and not _count(controls).any()     # the warm-up ran on a clone
    toks = torch.cat([g.replay()[0] for _ in range(2)])
    assert torch.equal(toks, e[0])
    live = ~controls.finished.bool()
    assert torch.equal(controls.length, e[2]) and not controls.overflow.any()
    full = torch.cat([prompt, toks]).t().int()
    for r in range(B):
        L = int(controls.hist_len[r])
        assert L == T0 + int(controls.length[r]) and torch.equal(controls.hist[r, :L], full[r, :L])
    assert (controls.hist_len[live] == T0 + 16).all()
    assert _count(controls).sum() == int(controls.length.sum())


# ---- 7. determinism ----
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
        out = lm_sample(h, w, b, tau, snap, C.STEP, embed=e, top_k=k, top_p=p, return_kept=True, controls=ctl)
        runs.append(out + (ctl.seen, ctl.length, ctl.finished, ctl.hist, ctl.hist_len, ctl.count.view(torch.int16), ctl.overflow))
    for other in runs[1:]:
        assert all(torch.equal(x, y) for x, y in zip(runs[0], other))


# ---- 8. the library is opened by the history's arguments only ----
def test_a_generate_without_history_arguments_never_opens_the_library():
    code = ("import sys; sys.path[:0] = %r\n"
            "import torch, vmlmf_amd\nfrom vmlmf_amd import _decode, _history\n"
            "from lm_util import _small, _prompt\n"
            "m = _small('plain')\n"
            "m.generate(_prompt(3), 4, temperature=0.8, seed=1, top_k=5)\nm.generate(_prompt(3), 4, temperature=0.0, chunk=2)\n"
            "m.generate(_prompt(3), 4, temperature=0.8, seed=1, eos=3, repetition_penalty=1.2)\n"
            "torch.cuda.synchronize()\n"
            "assert _decode.loaded() and not _history.loaded() and 'libvmlmf_history.so' not in open('/proc/self/maps').read()\n"
            "out = m.generate(_prompt(3), 4, temperature=0.8, seed=1, top_k=5, no_repeat_ngram_size=2)\n"
            "torch.cuda.synchronize()\nassert _history.loaded() and len(out) == 3\n") % [p for p in sys.path if p]
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
