"""Model.score, lm_score and the vmlmf_score_rows launch (csrc/vmlmf_score.hip, libvmlmf_score.so) on the GPU: the kernel against the
numpy oracle of oracle/vmlmf_decode_oracle.py on the very fp32 scores it read (ranks and top tokens EQUAL, log-probabilities within 1e-4 of fp64),
bit for bit against the sampler's greedy choice, and Model.score against the fp64 teacher-forced oracle of lm_util.py,
against Model.generate and Model.beam_search, and against stock ops."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from lm_util import DEV, LP_TOL, MARGIN, _oracle_scores, _prompt, _small, _teacher_forced, beam_model
from vmlmf_decode_oracle import MODEL_EOS, score_oracle

pytestmark = pytest.mark.gpu
KERNEL_TOL = 1e-4      # fp32 log-probabilities against fp64 on the same scores: the figure test_gpu_generate.py holds lm_sample to


def _launch(scores, bias, targets, top):
    """The binding on a score tensor directly; outputs start from values the kernel never writes."""
    from vmlmf_amd import _score
    R = scores.shape[0]
    lp = torch.full((R,), 7.0, device=DEV)
    rank = torch.full((R,), -7, device=DEV, dtype=torch.int32)
    toks = torch.full((R, top), -1, device=DEV, dtype=torch.int64) if top else None
    tlp = torch.full((R, top), 7.0, device=DEV) if top else None
    _score.score_rows(scores, bias, targets, top, lp, rank, toks, tlp)
    return lp, rank, toks, tlp


def _against_the_oracle(scores, bias, targets, top, got, what):
    lp, rank, toks, tlp = got
    y = None if targets is None else targets.cpu().numpy()
    olp, orank, otoks, otlp, _ = score_oracle(scores.cpu().numpy(), None if bias is None else bias.cpu().numpy(), y, top)
    assert np.array_equal(rank.cpu().numpy(), orank), (what, "rank")
    err = np.abs(lp.cpu().double().numpy() - olp).max()
    assert err <= KERNEL_TOL, (what, "logprob", err)
    if y is not None:
        assert (lp.cpu().numpy()[y < 0] == 0.0).all()
    if top:
        assert toks.dtype == torch.int64 and np.array_equal(toks.cpu().numpy(), otoks), (what, "top_tokens")
        err = np.abs(tlp.cpu().double().numpy() - otlp).max()
        assert err <= KERNEL_TOL, (what, "top_logprob", err)


# (R, V, top, bias): V at the quad (1, 3, 97), one-trip (1023, 1024, 1025) and SF_LDS_V (12288, 12289) boundaries and the PTB size
KERNEL_CASES = [(1, 1, 1, True), (3, 1, 0, False), (3, 3, 0, False), (3, 3, 1, True), (257, 97, 5, True), (3, 97, 32, False),
                (3, 1023, 5, False), (3, 1024, 32, True), (257, 1025, 32, True), (3, 1025, 1, False), (257, 10000, 0, True),
                (3, 10000, 32, False), (257, 10000, 5, False), (3, 12288, 5, True), (3, 12289, 5, False), (1, 12289, 32, True)]


@pytest.mark.parametrize("R,V,top,with_bias", KERNEL_CASES, ids=lambda v: str(v))
def test_the_kernel_against_the_oracle_on_the_same_scores(R, V, top, with_bias):
    g = torch.Generator().manual_seed(1000 * V + 10 * R + top)
    scores = (2.0 * torch.randn((R, V), generator=g)).to(DEV)
    bias = torch.randn(V, generator=g).to(DEV) if with_bias else None
    targets = torch.randint(0, V, (R,), generator=g)
    targets[torch.rand(R, generator=g) < 0.2] = -1
    targets = targets.to(DEV)
    _against_the_oracle(scores, bias, targets, top, _launch(scores, bias, targets, top), (R, V, top, with_bias))


@pytest.mark.parametrize("V,top", [(97, 5), (10000, 32), (12289, 5)])
def test_ties_across_the_cut_and_tied_targets(V, top):
    """Integer-valued scores: every row is a handful of large tie groups, the cut falls inside one and so does the target."""
    g = torch.Generator().manual_seed(V)
    R = 6
    scores = torch.randint(0, 4, (R, V), generator=g).float()
    scores[0] = 1.0                                                   # all equal
    scores[1, : top - 2] = 9.0                                        # top - 2 clear winners, then the tie group of the 3s across the cut
    scores[2] = torch.where(torch.arange(V) % 2 == 0, -0.0, 0.0)     # -0 and +0 are one tie group
    targets = torch.randint(0, V, (R,), generator=g)
    targets[0] = V - 1
    scores, targets = scores.to(DEV), targets.to(DEV)
    got = _launch(scores, None, targets, top)
    _against_the_oracle(scores, None, targets, top, got, ("ties", V, top))
    assert got[1][0].item() == V - 1 and got[2][0].tolist() == list(range(top)) and got[2][2].tolist() == list(range(top))
    bias = torch.randint(-1, 2, (V,), generator=g).float().to(DEV)
    _against_the_oracle(scores, bias, targets, top, _launch(scores, bias, targets, top), ("ties, bias", V, top))


def _exact_head(R, V, seed):
    """(h, weight) whose GEMM is exact: h is the identity, so scores[r][v] = weight[v][r]."""
    g = torch.Generator().manual_seed(seed)
    return torch.eye(R, device=DEV), torch.randn((V, R), generator=g).to(DEV)


def test_rows_without_a_target_and_lm_score_in_chunks():
    from vmlmf_amd import lm_score
    R, V, top = 7, 97, 5
    h, w = _exact_head(R, V, 5)
    bias = torch.randn(V, generator=torch.Generator().manual_seed(6)).to(DEV)
    scores = w.t().contiguous()
    y = torch.tensor([3, -1, 96, -5, 0, 41, -1], device=DEV)
    full = lm_score(h, w, bias, y.clamp(min=0), top=top)
    part = lm_score(h, w, bias, y, top=top)
    _against_the_oracle(scores, bias, y, top, part, "lm_score")
    assert part[0].shape == (R,) and part[1].dtype == torch.int32 and part[2].shape == (R, top) and part[3].shape == (R, top)
    none = y < 0
    assert (part[0][none] == 0.0).all() and (part[1][none] == -1).all()                 # 0.0 / -1 exactly
    assert torch.equal(part[0][~none], full[0][~none]) and torch.equal(part[1][~none], full[1][~none])
    assert torch.equal(part[2], full[2]) and torch.equal(part[3], full[3])              # the top outputs do not depend on the target
    # targets=None: every row is such a row; top > 0 works, top = 0 returns the two
    nolp, norank, toks, tlp = lm_score(h, w, bias, None, top=top)
    assert (nolp == 0.0).all() and (norank == -1).all() and torch.equal(toks, full[2]) and torch.equal(tlp, full[3])
    assert len(lm_score(h, w, bias, None)) == 2
    # chunks of 3, 3, 1 rows give the one-chunk bits; (.., H) inputs are flattened; no bias
    for a, b in zip(lm_score(h, w, bias, y, top=top, chunk_rows=3), part):
        assert torch.equal(a, b)
    h3 = torch.cat([h, h[:1]]).view(2, 4, R)
    out = lm_score(h3, w, None, torch.cat([y, y[:1]]), top=2, chunk_rows=5)
    _against_the_oracle(torch.cat([scores, scores[:1]]), None, torch.cat([y, y[:1]]), 2, out, "lm_score, no bias")
    # through the C ABI with targets, logprob and rank all NULL
    from vmlmf_amd import _score
    t2, l2 = torch.full((R, top), -1, device=DEV, dtype=torch.int64), torch.zeros((R, top), device=DEV)
    _score.score_rows(scores, bias, None, top, None, None, t2, l2)
    assert torch.equal(t2, full[2]) and torch.equal(l2, full[3])


def test_a_nan_and_a_target_past_the_row_stay_inside_the_row():
    R, V, top = 4, 1025, 32
    g = torch.Generator().manual_seed(8)
    scores = torch.randn((R, V), generator=g)
    scores[0, 17] = float("nan")
    scores[1, ::3] = float("nan")
    scores[2] = float("nan")
    scores = scores.to(DEV)
    targets = torch.tensor([5, 3, 0, V + 100], device=DEV)
    lp, rank, toks, tlp = _launch(scores, None, targets, top)
    assert torch.isnan(lp).all() and torch.isnan(tlp[:3]).all()
    assert ((toks >= 0) & (toks < V)).all() and ((rank >= -1) & (rank < V)).all()
    assert all(len(set(row)) == top for row in toks.tolist())
    # the row with the target past its end: NaN and -1, its top outputs as any row's
    ok = _launch(scores[3:], None, torch.tensor([7], device=DEV), top)
    assert rank[3].item() == -1 and torch.equal(toks[3:], ok[2]) and torch.equal(tlp[3:], ok[3]) and not torch.isnan(ok[0]).any()


@pytest.mark.parametrize("V", [97, 10000])
@pytest.mark.parametrize("with_bias", [True, False])
def test_bit_equality_with_the_samplers_greedy_choice(V, with_bias):
    from vmlmf_amd import _lib
    B = 5
    g = torch.Generator().manual_seed(V + 1)
    scores = (3.0 * torch.randn((B, V), generator=g)).to(DEV)
    bias = torch.randn(V, generator=g).to(DEV) if with_bias else None
    tok = torch.empty(B, device=DEV, dtype=torch.int64)
    lp = torch.empty(B, device=DEV)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    dev = torch.device(DEV, torch.cuda.current_device())
    _lib.check(_lib.lib().vmlmf_lm_choose(B, 8, V, p(scores), p(bias), None, 0.0, None, 0, p(tok), p(lp), None, _lib.raw_stream(dev)))
    slp, rank, toks, tlp = _launch(scores, bias, tok, 3)
    assert torch.equal(slp, lp) and (rank == 0).all() and torch.equal(toks[:, 0], tok) and torch.equal(tlp[:, 0], lp)
    assert torch.equal(_launch(scores, bias, tok, 0)[0], lp)          # the launch without the top outputs: the same bits


@pytest.mark.parametrize("V,top", [(10000, 8), (12289, 32), (97, 0)])
def test_determinism_and_the_captured_launch(V, top):
    from vmlmf_amd import _score
    R = 9
    g = torch.Generator().manual_seed(3)
    scores = torch.randn((R, V), generator=g).to(DEV)
    bias = torch.randn(V, generator=g).to(DEV)
    targets = torch.randint(0, V, (R,), generator=g).to(DEV)
    a, b = _launch(scores, bias, targets, top), _launch(scores, bias, targets, top)
    assert all(x is None and y is None or torch.equal(x, y) for x, y in zip(a, b))
    lp, rank = torch.zeros(R, device=DEV), torch.zeros(R, device=DEV, dtype=torch.int32)
    toks = torch.zeros((R, top), device=DEV, dtype=torch.int64) if top else None
    tlp = torch.zeros((R, top), device=DEV) if top else None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                     # linear, one stream
        _score.score_rows(scores, bias, targets, top, lp, rank, toks, tlp)
    for _ in range(2):
        for t in (lp, rank, toks, tlp):
            if t is not None:
                t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(x is None and y is None or torch.equal(x, y) for x, y in zip(a, (lp, rank, toks, tlp)))


# ---- Model.score against the fp64 teacher-forced oracle ----
T, B, TOP = 20, 3, 4


@functools.lru_cache(maxsize=None)
def _case(kind):
    """(model, tokens (T + 1, B) on the device, oracle scores (T, B, V) fp64, oracle states): computed once, left unchanged."""
    m = _small(kind)
    tokens = torch.randint(0, 97, (T + 1, B), generator=torch.Generator().manual_seed(31)).to(DEV)
    z, states = _oracle_scores(m, tokens[:-1])
    return m, tokens, z, states


def _check_against_the_oracle(out, z, targets, ref_states, what):
    logp, rank, toks, tlp, states = out
    assert logp.shape == (T, B) and rank.shape == (T, B) and rank.dtype == torch.int32
    assert toks.shape == (T, B, TOP) and toks.dtype == torch.int64 and tlp.shape == (T, B, TOP)
    y = targets.cpu()
    lsm = torch.log_softmax(z, -1)
    assert torch.allclose(logp.cpu().double(), lsm.gather(-1, y[..., None])[..., 0], atol=LP_TOL, rtol=0), what
    assert torch.allclose(tlp.cpu().double(), lsm.gather(-1, toks.cpu()), atol=LP_TOL, rtol=0), what
    for (h, c), (rh, rc) in zip(states, ref_states):
        assert torch.allclose(h.cpu().double(), rh, atol=1e-4, rtol=0) and torch.allclose(c.cpu().double(), rc, atol=1e-4, rtol=0), what
    # the rank lies between the tokens clearly ahead of the target and those not clearly behind it
    zy = z.gather(-1, y[..., None])
    lo = (z > zy + MARGIN).sum(-1)
    hi = (z > zy - MARGIN).sum(-1) - 1                                # (the target itself is within MARGIN of itself)
    r = rank.cpu().long()
    assert ((lo <= r) & (r <= hi)).all(), (what, r[(r < lo) | (r > hi)])
    # every reported top token scores at least the oracle's TOP-th largest, less MARGIN; they are distinct and in order
    kth = z.topk(TOP, -1).values[..., -1:]
    assert (z.gather(-1, toks.cpu()) >= kth - MARGIN).all(), what
    assert (tlp[..., :-1] >= tlp[..., 1:]).all() and all(len(set(row)) == TOP for row in toks.view(-1, TOP).tolist())


@pytest.mark.parametrize("kind", ["plain", "group", "wide"])
def test_model_score_against_the_teacher_forced_oracle(kind):
    m, tokens, z, ref_states = _case(kind)
    out = m.score(tokens, top=TOP)
    _check_against_the_oracle(out, z, tokens[1:], ref_states, kind)
    # the two-tensor form and the call without the top outputs: the same launch on the same rows
    two = m.score(tokens[:-1], tokens[1:], states=m.state_init(B), top=TOP)
    assert all(torch.equal(a, b) for a, b in zip(out[:4], two[:4]))
    plain = m.score(tokens)
    assert len(plain) == 3 and torch.equal(plain[0], out[0]) and torch.equal(plain[1], out[1])


def test_chunk_rows_with_an_uneven_last_chunk():
    m, tokens, z, ref_states = _case("plain")
    out = m.score(tokens, top=TOP, chunk_rows=7)                       # 60 rows: eight chunks of 7 and one of 4
    _check_against_the_oracle(out, z, tokens[1:], ref_states, "chunk_rows=7")


def test_lengths_mask_exactly_the_padding():
    m, tokens, _, _ = _case("plain")
    full = m.score(tokens, top=TOP)
    lengths = torch.tensor([20, 11, 0])
    for ln in (lengths, lengths.to(DEV), lengths.to(torch.int32)):
        logp, rank, toks, tlp, _ = m.score(tokens, lengths=ln, top=TOP)
        live = (torch.arange(T)[:, None] < lengths[None, :]).to(DEV)
        assert (logp[~live] == 0.0).all() and (rank[~live] == -1).all()
        assert torch.equal(logp[live], full[0][live]) and torch.equal(rank[live], full[1][live])
        assert torch.equal(toks, full[2]) and torch.equal(tlp, full[3])
        assert torch.allclose(logp.sum(0), torch.stack([full[0][:n, b].sum() for b, n in enumerate(lengths.tolist())]), atol=1e-5)


# ---- agreement with the decoders ----
def test_greedy_generate_is_scored_as_it_reported():
    m = _small("plain")
    prompt = _prompt(3, seed=2)
    tokens, logprobs, gstates = m.generate(prompt, 16, temperature=0.0)
    logp, rank, states = m.score(torch.cat([prompt, tokens]))
    assert (logp[-16:] - logprobs).abs().max().item() <= 2 * LP_TOL     # both sit within LP_TOL of one oracle
    z, _ = _teacher_forced(m, prompt, tokens)
    top2 = z.topk(2, -1).values
    clear = (top2[..., 0] - top2[..., 1] > MARGIN).to(DEV)
    assert clear.float().mean().item() > 0.9 and (rank[-16:][clear] == 0).all()


def test_beam_search_scores_are_the_sums_of_the_scored_tokens():
    m = beam_model("plain").to(DEV)
    eos, steps, W, Bb = MODEL_EOS, 8, 3, 2
    prompt = _prompt(Bb, seed=3)
    tokens, scores, lengths, _ = m.beam_search(prompt, steps, beams=W, eos=eos)
    assert 0 < (lengths < steps).sum().item()                          # some hypothesis finished: its padding must not count
    T0 = prompt.shape[0]
    seqs = torch.cat([prompt.repeat_interleave(W, 1), tokens.reshape(steps, Bb * W)])
    logp, _, _ = m.score(seqs, lengths=T0 - 1 + lengths.reshape(-1))
    total = logp[T0 - 1:].sum(0).view(Bb, W)
    assert (total - scores).abs().max().item() <= 2 * steps * LP_TOL, (total, scores)


# ---- what a call leaves behind ----
def test_score_leaves_the_flags_the_caches_and_the_generators_as_it_found_them(monkeypatch):
    from vmlmf_amd import Model, _score, cache_packed_parameters
    torch.manual_seed(11)
    m = Model(32, 16, 2, 0.5, 0.3, w_rank=4, u_ranks=[4], lstm_type="vmlmf").to(DEV)
    tokens = torch.randint(0, 32, (6, 2), generator=torch.Generator().manual_seed(12)).to(DEV)
    m.eval()
    want = m.score(tokens, top=3)
    m.train()
    m.rnns[1].eval()
    cache_packed_parameters(m.rnns[0])
    kept = m.rnns[0]._pack_cache
    flags = [(mod, mod.training) for mod in m.modules()]
    assert len({was for _, was in flags}) == 2
    gens = [m.dropout_state(seed=5), m.sampler_state(seed=6)]
    before = [g.clone() for g in gens]

    def untouched(what):
        assert all(mod.training == was for mod, was in flags), what
        assert m.rnns[0]._pack_cache is kept and "_pack_cache" not in m.rnns[1].__dict__, what
        assert m.dropout_state() is gens[0] and m.sampler_state() is gens[1] and all(torch.equal(g, b) for g, b in zip(gens, before)), what

    got = m.score(tokens, top=3)                                       # dropout 0.5, training mode: scored exactly as in eval mode
    untouched("score, top")
    assert all(torch.equal(a, b) for a, b in zip(got[:4], want[:4]))
    assert all(torch.equal(a, b) for sa, sb in zip(got[4], want[4]) for a, b in zip(sa, sb))
    assert not got[0].requires_grad
    plain = m.score(tokens)
    untouched("score")
    assert torch.equal(plain[0], want[0])
    real, calls = _score.score_rows, []

    def failing(*args):
        calls.append(1)
        if len(calls) == 2:
            raise RuntimeError("halfway")
        real(*args)
    monkeypatch.setattr(_score, "score_rows", failing)
    with pytest.raises(RuntimeError, match="halfway"):
        m.score(tokens, top=3, chunk_rows=4)                           # raised by the second of three launches
    untouched("score, raising")
    with pytest.raises(IndexError):
        m.score(tokens, states=m.state_init(2)[:1])
    untouched("score, raising in front of any launch")


@pytest.mark.parametrize("lstm_type", ["custom", "pytorch"])
def test_stock_layers_score_under_the_same_call(lstm_type):
    from vmlmf_amd import Model
    torch.manual_seed(9)
    m = Model(97, 32, 2, 0.0, 0.3, lstm_type=lstm_type).to(DEV).eval()
    tokens = torch.randint(0, 97, (9, 2), generator=torch.Generator().manual_seed(4)).to(DEV)
    logp, rank, toks, tlp, states = m.score(tokens, top=TOP)
    with torch.no_grad():
        scores, ref_states = m(tokens[:-1], m.state_init(2))
    lsm = torch.log_softmax(scores.double(), -1).view(8, 2, 97)
    assert torch.allclose(logp.double(), lsm.gather(-1, tokens[1:, :, None])[..., 0], atol=LP_TOL, rtol=0)
    assert torch.allclose(tlp.double(), lsm.gather(-1, toks), atol=LP_TOL, rtol=0)
    for (h, c), (rh, rc) in zip(states, ref_states):
        assert h.shape == rh.shape and torch.allclose(h, rh, atol=1e-5) and torch.allclose(c, rc, atol=1e-5)


def test_ptb_size_once_against_stock_ops():
    from vmlmf_amd import Model
    torch.manual_seed(7)
    m = Model(10000, 650, 2, 0.0, 0.1, w_rank=32, u_ranks=[32], lstm_type="vmlmf").to(DEV).eval()
    Tp, Bp, top = 4, 8, 8
    tokens = torch.randint(0, 10000, (Tp + 1, Bp), generator=torch.Generator().manual_seed(5)).to(DEV)
    logp, rank, toks, tlp, _ = m.score(tokens, top=top)
    with torch.no_grad():
        scores, _ = m(tokens[:-1], m.state_init(Bp))
    z = scores.double().view(Tp, Bp, -1)
    lsm = torch.log_softmax(z, -1)
    assert torch.allclose(logp.double(), lsm.gather(-1, tokens[1:, :, None])[..., 0], atol=1e-3, rtol=0)
    assert torch.allclose(tlp.double(), lsm.gather(-1, toks), atol=1e-3, rtol=0)
    best = z.topk(top + 1, -1)
    clear = best.values[..., top - 1] - best.values[..., top] > MARGIN
    assert clear.any()
    same = (toks.sort(-1).values == best.indices[..., :top].sort(-1).values).all(-1)
    assert same[clear].all()
