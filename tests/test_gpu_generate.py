"""Model.generate and the one-launch token sampler (vmlmf_lm_sample, csrc/vmlmf_sample.hip) against the fp64 oracle.

The oracle is teacher-forced with the GPU's tokens: the literal layers (vmlmf_oracle.literal_sequence) run over the prompt and the
generated tokens, so every choice the GPU made is judged on the scores it had in front of it.  A token passes when it is the oracle's
argmax of scores (greedy) or of scores / tau + G (sampling, G restated with the oracle's Philox) - or, where the oracle's best and the
GPU's token lie within MARGIN of each other, when fp32 cannot tell them apart."""
import numpy as np
import pytest
import torch

from lm_util import DEV, LP_TOL, MARGIN, _check_choices, _prompt, _small, _teacher_forced
from vmlmf_decode_oracle import gumbel_restated

pytestmark = pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plain", "group", "wide", "wide300"])
def test_greedy_tokens_and_logprobs_against_the_oracle(kind):
    m = _small(kind)
    prompt = _prompt(3)
    tokens, logprobs, states = m.generate(prompt, 24, temperature=0.0)
    assert tokens.shape == (24, 3) and tokens.dtype == torch.int64 and logprobs.shape == (24, 3)
    z, ref_states = _teacher_forced(m, prompt, tokens)
    _check_choices(z, tokens, MARGIN, f"{kind} greedy")
    lsm = torch.log_softmax(z, -1).gather(-1, tokens.cpu()[..., None])[..., 0]
    assert torch.allclose(logprobs.cpu().double(), lsm, atol=LP_TOL, rtol=0), (logprobs.cpu() - lsm).abs().max()
    # the returned states have taken in the prompt and every generated token
    for (h, c), (rh, rc) in zip(states, ref_states):
        assert torch.allclose(h.cpu().double(), rh, atol=1e-4) and torch.allclose(c.cpu().double(), rc, atol=1e-4)


def test_sampling_restated_with_the_oracle_philox():
    m = _small("plain")
    prompt = _prompt(3, seed=1)
    seed, tau = 0x0DDB_A11_5EED, 0.7
    tokens, logprobs, _ = m.generate(prompt, 24, temperature=tau, seed=seed)
    assert m.sampler_state().cpu().tolist() == [seed, 1]           # one snapshot per call: offset 0 was this call's
    z, _ = _teacher_forced(m, prompt, tokens)
    G = torch.stack([torch.from_numpy(gumbel_restated(seed, 0, j, 3, 97)[1]) for j in range(24)])
    _check_choices(z / tau + G, tokens, MARGIN / tau, "sampled")
    lsm = torch.log_softmax(z, -1).gather(-1, tokens.cpu()[..., None])[..., 0]
    assert torch.allclose(logprobs.cpu().double(), lsm, atol=LP_TOL, rtol=0)
    # not the greedy tokens: the noise took part
    greedy, _, _ = m.generate(prompt, 24, temperature=0.0)
    assert not torch.equal(greedy, tokens)


def test_same_seed_same_tokens_other_seed_or_next_call_fresh_ones():
    m = _small("group")
    prompt = _prompt(4, seed=2)
    a = m.generate(prompt, 16, temperature=1.0, seed=11)
    b = m.generate(prompt, 16, temperature=1.0, seed=11)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])                    # bit-identical log-probabilities
    nxt = m.generate(prompt, 16, temperature=1.0)                                  # the generator moved on
    other = m.generate(prompt, 16, temperature=1.0, seed=12)
    assert not torch.equal(a[0], nxt[0]) and not torch.equal(a[0], other[0])
    # the model's dropout generator is not the sampler's
    before = m.dropout_state().clone()
    m.generate(prompt, 4, temperature=1.0)
    assert torch.equal(m.dropout_state(), before)
    # greedy is the same every time, down to the bits
    g1, g2 = m.generate(prompt, 16, temperature=0.0), m.generate(prompt, 16, temperature=0.0)
    assert torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1])


def test_token_frequencies_follow_the_softmax():
    """4096 identical rows (the top layer's output after a prompt), one step at tau = 1: every token's count within five sigma of
    N softmax(oracle scores); fixed seed."""
    from vmlmf_amd import lm_sample, dropout_state, dropout_advance
    m = _small("plain").eval()
    with torch.no_grad():
        h, _ = m.features(_prompt(1, seed=3), m.state_init(1))
        w = m.fc.w * 25.0                  # a distribution with some shape: probabilities from ~1e-3 to ~0.1
    N = 4096
    snap = dropout_advance(dropout_state(DEV, 0x5EED))
    tokens, _ = lm_sample(h[-1].expand(N, -1), w, m.fc.b.detach(), 1.0, snap, 0)
    z = h[-1, 0].double().cpu() @ w.double().cpu().t() + m.fc.b.detach().double().cpu()
    p = torch.softmax(z, -1).numpy()
    assert p.max() > 0.03 and p.min() < 3e-3, (p.max(), p.min())
    counts = np.bincount(tokens.cpu().numpy(), minlength=97)
    sigma = np.sqrt(N * p * (1 - p))
    assert (np.abs(counts - N * p) <= 5 * sigma + 1).all(), np.argwhere(np.abs(counts - N * p) > 5 * sigma + 1)
    # and at tau = 0.5 the draws follow softmax(2 z) - here through the fused form, which walks the 4096 rows 16 at a time
    tokens, _ = lm_sample(h[-1].expand(N, -1), w, m.fc.b.detach(), 0.5, dropout_advance(dropout_state(DEV, 0x5EED)), 0, form="fused")
    p = torch.softmax(2 * z, -1).numpy()
    counts = np.bincount(tokens.cpu().numpy(), minlength=97)
    assert (np.abs(counts - N * p) <= 5 * np.sqrt(N * p * (1 - p)) + 1).all()


@pytest.mark.parametrize("group", [False, True])
@pytest.mark.parametrize("B", [1, 32])
def test_ptb_size_greedy_against_the_chained_forward(group, B):
    from vmlmf_amd import Model
    torch.manual_seed(7)
    if group:
        m = Model.with_group_layers(10000, 650, 2, 0.0, 0.1, w_rank=32, u_ranks=[32, 32]).to(DEV)
    else:
        m = Model(10000, 650, 2, 0.0, 0.1, w_rank=32, u_ranks=[32], lstm_type="vmlmf").to(DEV)
    m.eval()
    prompt = _prompt(B, T0=6, V=10000, seed=4)
    tokens, logprobs, states = m.generate(prompt, 16, temperature=0.0)
    with torch.no_grad():
        seq = torch.cat([prompt, tokens])
        scores, fstates = m(seq[:-1], m.state_init(B))
    z = scores.view(seq.shape[0] - 1, B, -1)[prompt.shape[0] - 1:].double().cpu()
    _check_choices(z, tokens, 1e-3, "ptb greedy")
    lsm = torch.log_softmax(z, -1).gather(-1, tokens.cpu()[..., None])[..., 0]
    assert torch.allclose(logprobs.cpu().double(), lsm, atol=1e-3, rtol=0)
    with torch.no_grad():
        _, fstates = m(seq, m.state_init(B))
    for (h, c), (rh, rc) in zip(states, fstates):
        assert torch.allclose(h, rh, atol=1e-4) and torch.allclose(c, rc, atol=1e-4)


def test_a_captured_chunk_draws_fresh_tokens_on_every_replay():
    from vmlmf_amd import DecodeGraph
    m = _small("plain").eval()
    prompt = _prompt(4, seed=5)
    with torch.no_grad():
        h, st = m.features(prompt, m.state_init(4))
    h = h[-1]
    m.sampler_state(seed=21)
    g = DecodeGraph(m, h, st, 8, temperature=1.0)
    t1, l1 = g.replay()
    t2, _ = g.replay()
    assert not torch.equal(t1, t2)
    m.sampler_state(seed=21)
    g2 = DecodeGraph(m, h, st, 8, temperature=1.0)
    t1b, l1b = g2.replay()
    assert torch.equal(t1, t1b) and torch.equal(l1, l1b)
    # the eager call with the same seed draws the same first chunk; the graphed generate continues across replays
    e = m.generate(prompt, 8, temperature=1.0, seed=21)
    assert torch.equal(e[0], t1)
    ge, gl, gst = m.generate(prompt, 16, temperature=0.0, chunk=8)
    ee, el, est = m.generate(prompt, 16, temperature=0.0)
    assert torch.equal(ge, ee) and torch.allclose(gl, el, atol=1e-6)
    for (a, b), (c, d) in zip(gst, est):
        assert torch.allclose(a, c, atol=1e-6) and torch.allclose(b, d, atol=1e-6)


def test_stock_layers_run_under_the_same_sampler():
    from vmlmf_amd import Model
    torch.manual_seed(9)
    m = Model(97, 32, 2, 0.0, 0.3, lstm_type="custom").to(DEV)
    prompt = _prompt(2, seed=6)
    tokens, logprobs, _ = m.generate(prompt, 8, temperature=0.0)
    with torch.no_grad():
        seq = torch.cat([prompt, tokens])
        scores, _ = m(seq[:-1], m.state_init(2))
    z = scores.view(seq.shape[0] - 1, 2, -1)[prompt.shape[0] - 1:].double().cpu()
    _check_choices(z, tokens, 1e-4, "custom greedy")
    m2 = Model(97, 32, 2, 0.0, 0.3, lstm_type="pytorch").to(DEV)
    t2, _, st2 = m2.generate(prompt, 4, temperature=0.5, seed=3)
    assert t2.shape == (4, 2) and st2[0][0].shape == (1, 2, 32)


def test_layer_paths_agree_and_the_callers_cache_setting_comes_back():
    from vmlmf_amd import cache_packed_parameters
    m = _small("plain")
    prompt = _prompt(3, seed=7)
    a = m.generate(prompt, 8, temperature=0.0, layer_path="layers")
    b = m.generate(prompt, 8, temperature=0.0, layer_path="stack")
    assert torch.equal(a[0], b[0]) and torch.allclose(a[1], b[1], atol=1e-4)
    assert all(getattr(r, "_pack_cache", None) is None for r in m.rnns)
    cache_packed_parameters(m)
    kept = [r._pack_cache for r in m.rnns]
    m.generate(prompt, 4, temperature=0.0)
    assert [r._pack_cache for r in m.rnns] == kept and all(c.fills >= 1 for c in kept)


def test_every_decode_call_leaves_the_flags_and_the_caches_as_it_found_them():
    """generate and beam_search, eager and as graphs, and a call that raises behind the prompt's checks: afterwards every module's
    train / eval flag is the caller's, a layer without kept images has no _pack_cache attribute and a layer with them its own cache."""
    from vmlmf_amd import Model, cache_packed_parameters
    torch.manual_seed(11)
    m = Model(32, 16, 2, 0.0, 0.3, w_rank=4, u_ranks=[4], lstm_type="vmlmf").to(DEV)
    m.train()
    m.rnns[1].eval()
    cache_packed_parameters(m.rnns[0])
    kept = m.rnns[0]._pack_cache
    flags = [(mod, mod.training) for mod in m.modules()]
    assert len({was for _, was in flags}) == 2
    prompt = _prompt(2, T0=2, V=32, seed=12)

    def untouched(what):
        assert all(mod.training == was for mod, was in flags), what
        assert m.rnns[0]._pack_cache is kept and "_pack_cache" not in m.rnns[1].__dict__, what

    calls = {"generate": lambda **kw: m.generate(prompt, 2, **kw), "generate chunk": lambda **kw: m.generate(prompt, 2, chunk=2, **kw),
             "beam_search": lambda **kw: m.beam_search(prompt, 2, beams=2, **kw),
             "beam_search chunk": lambda **kw: m.beam_search(prompt, 2, beams=2, chunk=2, **kw)}
    for what, call in calls.items():
        out = call()
        assert out[0].shape[:2] == (2, 2), what
        untouched(what)
    for what, call in calls.items():
        with pytest.raises(IndexError):
            call(states=m.state_init(2)[:1])       # one layer's states for two layers: raised in Python, in front of any launch
        untouched(what + ", raising")


def test_lm_sample_alone_matches_the_projection():
    from vmlmf_amd import lm_sample
    torch.manual_seed(3)
    for B, H, V in ((1, 650, 10000), (19, 40, 33), (40, 700, 1000)):
        h = torch.randn(B, H, device=DEV)
        w = torch.randn(V, H, device=DEV) * 0.1
        b = torch.randn(V, device=DEV)
        e = torch.randn(V, H, device=DEV)
        tok, lp, xn = lm_sample(h, w, b, 0.0, embed=e)
        z = (h.double() @ w.double().t() + b.double()).cpu()
        _check_choices(z[None], tok[None], 1e-4, f"lm_sample {B}x{H}x{V}")
        ref = torch.log_softmax(z, -1).gather(-1, tok.cpu()[:, None])[:, 0]
        assert torch.allclose(lp.cpu().double(), ref, atol=1e-4)
        assert torch.equal(xn, e[tok])
        tok2, lp2 = lm_sample(h, w, b, 0.0)
        assert torch.equal(tok, tok2) and torch.equal(lp, lp2)


def test_cpu_tensors_raise():
    from vmlmf_amd import Model
    m = Model(97, 32, 2, 0.0, 0.1, w_rank=8, u_ranks=[8], lstm_type="vmlmf")
    with pytest.raises(RuntimeError, match="cuda"):
        m.generate(torch.zeros((3, 2), dtype=torch.int64), 4)


def test_wide_batches_take_the_gemm_form_and_draw_the_same_noise():
    """Beyond 16 rows lm_sample takes the library GEMM + vmlmf_lm_choose: same Philox layout, so the oracle's restatement holds there too,
    and on rows where both forms see the same ordering they pick the same tokens."""
    from vmlmf_amd import lm_sample, dropout_state, dropout_advance
    m = _small("plain")
    prompt = _prompt(40, seed=8)
    seed, tau = 77, 0.7
    tokens, logprobs, _ = m.generate(prompt, 12, temperature=tau, seed=seed)
    z, _ = _teacher_forced(m, prompt, tokens)
    G = torch.stack([torch.from_numpy(gumbel_restated(seed, 0, j, 40, 97)[1]) for j in range(12)])
    _check_choices(z / tau + G, tokens, MARGIN / tau, "sampled, gemm form")
    lsm = torch.log_softmax(z, -1).gather(-1, tokens.cpu()[..., None])[..., 0]
    assert torch.allclose(logprobs.cpu().double(), lsm, atol=LP_TOL, rtol=0)
    torch.manual_seed(5)
    h = torch.randn(16, 32, device=DEV)
    snap = dropout_advance(dropout_state(DEV, 3))
    a = lm_sample(h, m.fc.w.detach(), m.fc.b.detach(), 1.0, snap, 2, embed=m.embed.w.detach(), form="fused")
    b = lm_sample(h, m.fc.w.detach(), m.fc.b.detach(), 1.0, snap, 2, embed=m.embed.w.detach(), form="gemm")
    assert (a[0] == b[0]).float().mean().item() >= 15 / 16 and torch.allclose(a[1], b[1], atol=1e-5)
    sel = a[0] == b[0]
    assert torch.equal(a[2][sel], b[2][sel])


def test_a_captured_chunk_on_the_stack_path():
    from vmlmf_amd import DecodeGraph
    m = _small("plain").eval()
    prompt = _prompt(8, seed=9)
    ge, gl, gst = m.generate(prompt, 16, temperature=0.0, chunk=8, layer_path="stack")
    ee, el, est = m.generate(prompt, 16, temperature=0.0, layer_path="stack")
    assert torch.equal(ge, ee) and torch.allclose(gl, el, atol=1e-6)
    for (a, b), (c, d) in zip(gst, est):
        assert torch.allclose(a, c, atol=1e-6) and torch.allclose(b, d, atol=1e-6)
    z, _ = _teacher_forced(m, prompt, ee)
    _check_choices(z, ee, MARGIN, "stack path greedy")


def test_null_bias_and_null_logprob_through_the_c_abi():
    import ctypes
    from vmlmf_amd import _lib, lm_sample
    from vmlmf_amd.functional import sample_ticket
    from vmlmf_amd.decoding import _sample_workspace
    torch.manual_seed(11)
    B, H, V = 5, 48, 301
    h = torch.randn(B, H, device=DEV)
    w = torch.randn(V, H, device=DEV) * 0.2
    tok, lp = lm_sample(h, w, None, 0.0)
    z = (h.double() @ w.double().t()).cpu()
    _check_choices(z[None], tok[None], 1e-4, "no bias")
    assert torch.allclose(lp.cpu().double(), torch.log_softmax(z, -1).gather(-1, tok.cpu()[:, None])[:, 0], atol=1e-4)
    lib = _lib.lib()
    t2 = torch.empty(B, dtype=torch.int64, device=DEV)
    nbytes = lib.vmlmf_lm_sample_workspace_bytes(B, V)
    ws = _sample_workspace(torch.device(DEV, torch.cuda.current_device()), nbytes)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    dev = torch.device(DEV, torch.cuda.current_device())
    _lib.check(lib.vmlmf_lm_sample(B, H, V, p(h), p(w), None, None, 0.0, None, 0, p(t2), None, None, p(sample_ticket(dev)), p(ws), nbytes,
                                   _lib.raw_stream(dev)))
    t3 = torch.empty(B, dtype=torch.int64, device=DEV)
    scores = torch.mm(h, w.t())
    _lib.check(lib.vmlmf_lm_choose(B, H, V, p(scores), None, None, 0.0, None, 0, p(t3), None, None, _lib.raw_stream(dev)))
    assert torch.equal(t2, tok)
    _check_choices(z[None], t3[None], 1e-4, "choose without bias or log-probabilities")
    assert int(sample_ticket(dev).abs().sum()) == 0            # the ticket is back to zero after every launch
