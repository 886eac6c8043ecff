"""Model.contrastive_search and its step (vmlmf_contrast_choose, csrc/vmlmf_contrast.hip) against the fp64 reference of
contrast_cases.py.  Kernel level: guard-banded buffers whose unspecified parts - history rows at and beyond hist_len, the bands - are
poisoned; every choice of every case is clear in the reference (test_contrast_cpu.py), so the discrete outputs are the reference's
exactly and the similarities lie within the derived bound.  Model level: teacher-forced on the GPU's own tokens."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import contrast_cases as CC
from lm_util import DEV, _prompt

pytestmark = pytest.mark.gpu
EOS = CC.EOS
GUARD = 64                       # elements on either side of every buffer (a multiple of four floats: hist stays 16-byte aligned)
INT_POISON = -7777


def _dev():
    return torch.device(DEV, torch.cuda.current_device())


def _banded(shape, dtype):
    """(whole, view): a poisoned flat buffer and the view of `shape` between its guard bands."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), float("nan") if dtype == torch.float32 else INT_POISON, dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + n].view(shape)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else t.dtype).clone()


def _guards_intact(whole):
    w = _bits(whole)
    poison = _bits(torch.full((1,), float("nan")))[0] if whole.dtype == torch.float32 else INT_POISON
    return bool((w[:GUARD] == poison).all() and (w[-GUARD:] == poison).all())


class Launch:
    """The buffers of one kernel-level case on the device: the history filled by vmlmf_contrast_append from poison, everything else
    between guard bands."""

    def __init__(self, case, variant):
        from vmlmf_amd import _contrast
        self.lib = _contrast.LIBRARY
        B, k, H, t = self.case = case
        c = self.c = CC.kernel_case(case, variant)
        self.Tcap = c["Tcap"]
        self.whole = {}
        for name, shape, dtype in (("hist", (B, self.Tcap, H), torch.float32), ("hist_len", (B,), torch.int32), ("finished", (B,), torch.int32),
                                   ("length", (B,), torch.int32), ("token", (B,), torch.int64), ("logprob", (B,), torch.float32),
                                   ("chosen", (B,), torch.int32), ("sim", (B, k), torch.float32), ("h_next", (B, H), torch.float32),
                                   ("src_row", (B * k,), torch.int32), ("cand_h", (B * k, H), torch.float32),
                                   ("cand_tok", (B, k), torch.int64), ("cand_logp", (B, k), torch.float32)):
            self.whole[name], view = _banded(shape, dtype)
            setattr(self, name, view)
        self.ticket = torch.zeros(B, dtype=torch.int32, device=DEV)
        self.workspace = torch.full((_contrast.workspace_bytes(B) // 4,), float("nan"), device=DEV)
        self.hist_len.zero_()
        for name in ("finished", "length", "cand_h", "cand_tok", "cand_logp"):
            getattr(self, name).copy_(torch.from_numpy(c[name]))
        self.append(torch.from_numpy(c["hist_raw"]).transpose(0, 1).contiguous().to(DEV), self.hist, self.hist_len, self.Tcap)
        self.before = {name: _bits(getattr(self, name)) for name in ("hist", "hist_len", "finished", "length")}

    def append(self, h, hist, hist_len, Tcap):
        from vmlmf_amd._lib import ptr
        T, B, H = h.shape
        self.lib.call(_dev(), "vmlmf_contrast_append", B, T, H, ptr(h), ptr(hist), ptr(hist_len), Tcap)

    def args(self, parts=0, **over):
        from vmlmf_amd._lib import ptr
        B, k, H, t = self.case
        a = dict(B=B, k=k, H=H, Tcap=self.Tcap, cand_h=ptr(self.cand_h), cand_tok=ptr(self.cand_tok), cand_logp=ptr(self.cand_logp),
                 alpha=self.c["alpha"], eos=EOS, hist=ptr(self.hist), hist_len=ptr(self.hist_len), finished=ptr(self.finished),
                 length=ptr(self.length), token=ptr(self.token), logprob=ptr(self.logprob), chosen=ptr(self.chosen), sim=ptr(self.sim),
                 h_next=ptr(self.h_next), src_row=ptr(self.src_row), ticket=ptr(self.ticket), workspace=ptr(self.workspace),
                 workspace_bytes=self.workspace.numel() * 4, parts=parts)
        a.update(over)
        return list(a.values())

    def choose(self, parts=0):
        self.lib.call(_dev(), "vmlmf_contrast_choose", *self.args(parts))
        torch.cuda.synchronize()
        return {name: _bits(getattr(self, name)) for name in ("token", "logprob", "chosen", "sim", "h_next", "src_row", "hist", "hist_len",
                                                               "finished", "length")}

    def unit_rows(self, vectors):
        """What vmlmf_contrast_append writes for `vectors` (B, H): the bits of (B, H) unit rows."""
        B, H = vectors.shape
        hist = torch.full((B, 1, H), float("nan"), device=DEV)
        self.append(vectors.view(1, B, H).contiguous(), hist, torch.zeros(B, dtype=torch.int32, device=DEV), 1)
        return _bits(hist[:, 0])


# ---- 1. the step against the reference ----
@pytest.mark.parametrize("variant", CC.VARIANTS)
@pytest.mark.parametrize("case", CC.KERNEL_CASES, ids=CC.case_id)
def test_step_against_the_reference(case, variant):
    B, k, H, t = case
    L = Launch(case, variant)
    c, Tcap = L.c, L.Tcap
    # the append: t unit rows per batch row, the rest of the history still poison
    hist0 = L.hist.cpu()
    assert L.before["hist_len"].tolist() == [t] * B
    assert torch.isnan(hist0[:, t:]).all() and not torch.isnan(hist0[:, :t]).any()
    norm_err = (hist0[:, :t].double().pow(2).sum(-1).sqrt() - 1).abs().max().item() if t else 0.0
    assert norm_err <= (H / 2 + 3) * CC.U, norm_err
    out = L.choose()
    ref = CC.kernel_oracle(case, variant)
    sim = out["sim"].view(torch.float32).double().numpy()
    live = [b for b in range(B) if not c["finished"][b]]
    worst = 0.0
    for b in range(B):
        blk = slice(b * k, (b + 1) * k)
        if c["finished"][b]:
            assert out["token"][b] == EOS and out["logprob"][b] == 0 and out["chosen"][b] == 0          # (the bits of 0.0)
            assert (out["sim"][b] == 0).all() and out["src_row"][blk].tolist() == [b * k] * k
            assert torch.equal(out["h_next"][b], _bits(L.cand_h[b * k]))
            assert torch.equal(out["hist"][b], L.before["hist"][b])                                     # nothing appended, poison included
            assert out["hist_len"][b] == t and out["finished"][b] == 1 and out["length"][b] == c["length"][b]
            continue
        rsim, values, j, gap = ref[b]
        err = np.abs(sim[b] - rsim).max()
        worst = max(worst, err)
        assert err <= CC.bound(H), (case, variant, b, err, CC.bound(H))
        assert gap > CC.margin(c["alpha"], H)                                    # clear (test_contrast_cpu.py): the choice is judged
        assert out["chosen"][b] == j, (case, variant, b, int(out["chosen"][b]), j, values)
        assert out["token"][b] == c["cand_tok"][b, j]
        assert out["logprob"][b] == _bits(torch.from_numpy(c["cand_logp"][b, j:j + 1]))[0]
        assert out["src_row"][blk].tolist() == [b * k + j] * k
        assert torch.equal(out["h_next"][b], _bits(torch.from_numpy(c["cand_h"][b * k + j])))
        assert out["hist_len"][b] == t + 1 and out["length"][b] == c["length"][b] + 1
        assert out["finished"][b] == (1 if c["cand_tok"][b, j] == EOS else 0)
        assert torch.equal(out["hist"][b, :t], L.before["hist"][b, :t]) and torch.equal(out["hist"][b, t + 1:], L.before["hist"][b, t + 1:])
    print(CC.case_id(case), variant, "max |sim - fp64|", worst, "bound", CC.bound(H))
    if variant == "twin":
        for b in live:
            assert abs(sim[b, CC.TWIN] - 1.0) <= CC.bound(H)
    # the appended row: bit for bit what vmlmf_contrast_append writes for the chosen vector
    picked = L.cand_h[torch.arange(B, device=DEV) * k + L.chosen.long()]
    expect = L.unit_rows(picked)
    for b in live:
        assert torch.equal(out["hist"][b, t], expect[b]), (case, variant, b)
    assert all(_guards_intact(w) for w in L.whole.values()), [n for n, w in L.whole.items() if not _guards_intact(w)]
    assert int(L.ticket.abs().sum()) == 0                                        # the ticket words are zero after the launch


# ---- 2. the same bits for every parts and from run to run ----
@pytest.mark.parametrize("variant", ["base", "finished", "twin"])
@pytest.mark.parametrize("case", CC.KERNEL_CASES, ids=CC.case_id)
def test_the_same_bits_for_every_parts(case, variant):
    first = Launch(case, variant).choose(0)
    for parts in (1, 2, 7, 0):
        L = Launch(case, variant)
        again = L.choose(parts)
        for name in first:
            assert torch.equal(first[name], again[name]), (case, variant, parts, name)
        assert int(L.ticket.abs().sum()) == 0 and all(_guards_intact(w) for w in L.whole.values())


# ---- 3. a NaN loses; a full history is not written past ----
def test_a_nan_candidate_loses_and_a_full_history_is_not_written_past():
    case = CC.KERNEL_CASES[0]
    B, k, H, t = case
    L = Launch(case, "alpha0")                                                   # alpha = 0: candidate 0, the most probable, would win
    L.cand_logp[0, 0] = float("nan")                                             # ... but a NaN value loses to every number
    out = L.choose()
    assert out["chosen"][0] == 1 and out["token"][0] == L.c["cand_tok"][0, 1]
    L = Launch(case, "alpha0")
    L.cand_logp[0] = float("nan")                                                # all NaN: candidate 0
    out = L.choose()
    assert out["chosen"][0] == 0 and torch.isnan(out["logprob"].view(torch.float32)[0])
    L = Launch(case, "base")                                                     # a NaN vector is taken for the zero vector: cosine 0
    L.cand_h[1, 3] = float("nan")
    out = L.choose()
    assert out["sim"][0, 1] == 0 and not torch.isnan(out["sim"].view(torch.float32)).any()
    # Tcap = t: no room.  The step still chooses; the history and its length stay as they are
    L = Launch(case, "base")
    free = L.before["hist"].clone()
    L.Tcap = t
    hist_t, view = _banded((B, t, H), torch.float32)
    view.copy_(L.hist[:, :t])
    L.whole["hist"], L.hist = hist_t, view
    out = L.choose()
    assert out["hist_len"].tolist() == [t] * B and out["chosen"][0] == CC.kernel_oracle(case, "base")[0][2]
    assert torch.equal(out["hist"], free[:, :t]) and _guards_intact(hist_t)


# ---- 4. every refusal launches nothing ----
def test_refusals_launch_nothing():
    from vmlmf_amd import _contrast, _lib
    case = CC.KERNEL_CASES[0]
    L = Launch(case, "base")
    names = ("token", "logprob", "chosen", "sim", "h_next", "src_row", "hist", "hist_len", "finished", "length")
    before = {n: _bits(getattr(L, n)) for n in names}
    fn = _contrast.lib().vmlmf_contrast_choose
    bad = [dict(B=0), dict(k=0), dict(k=17), dict(H=0), dict(Tcap=0), dict(alpha=-0.5), dict(alpha=1.5), dict(alpha=float("nan")),
           dict(eos=-2), dict(parts=-1), dict(parts=65), dict(cand_h=None), dict(hist=None), dict(token=None), dict(ticket=None),
           dict(workspace=None), dict(k=16, H=964), dict(hist=ctypes.c_void_p(L.hist.data_ptr() + 4))]
    for over in bad:
        with _lib.on_device(_dev()):
            rc = fn(*L.args(**over), _lib.raw_stream(_dev()))
        assert rc == _lib.E_BADARG, over
    with _lib.on_device(_dev()):
        assert fn(*L.args(workspace_bytes=16), _lib.raw_stream(_dev())) == _lib.E_WORKSPACE
    torch.cuda.synchronize()
    for n in names:
        assert torch.equal(before[n], _bits(getattr(L, n))), n
    assert int(L.ticket.abs().sum()) == 0


# ---- 5. the model level ----
STEPS, T0, ROWS, K, ALPHA = 8, 5, 3, 4, 0.6
FP32 = dict(atol=1e-5, rtol=1e-4)                                                 # the project's fp32 tolerance


@functools.lru_cache(maxsize=None)
def _model():
    from vmlmf_amd import Model
    torch.manual_seed(11)
    return Model(97, 16, 2, 0.0, 1.0, w_rank=8, u_ranks=[8], lstm_type="vmlmf").to(DEV)


@functools.lru_cache(maxsize=None)
def _search(**kw):
    """One contrastive search of the shared model, run once per set of arguments."""
    m = _model()
    args = dict(top_k=K, penalty_alpha=ALPHA, return_penalties=True)
    args.update(kw)
    return m.contrastive_search(_prompt(ROWS, T0), STEPS, **args)


def _features(m, seq, states=None):
    m.train(False)
    with torch.no_grad():
        return m.features(seq, m.state_init(seq.shape[1]) if states is None else list(states))


def test_the_choices_are_the_references_teacher_forced():
    m = _model()
    prompt = _prompt(ROWS, T0)
    tokens, logprobs, lengths, penalties, states = _search()
    assert tokens.shape == logprobs.shape == penalties.shape == (STEPS, ROWS) and tokens.dtype == torch.int64
    assert lengths.tolist() == [STEPS] * ROWS and lengths.dtype == torch.int32
    seq = torch.cat([prompt, tokens])
    hs, _ = _features(m, seq)                                                     # the top layer's output behind every token
    W, bias = m.fc.w.detach().double().cpu().numpy(), m.fc.b.detach().double().cpu().numpy()
    H = m.hidden_size
    # a step is judged where the reference's choice is clear by the kernel's margin widened by the head's: the candidates'
    # log-probabilities come from fp32 scores, good to the project's 1e-5, so p = exp(logp) <= 1 is good to 1e-5
    need = CC.margin(ALPHA, H, (1 - ALPHA) * 1e-5)
    unclear = []
    for s in range(STEPS):
        _, st = _features(m, seq[:T0 + s])
        logits = hs[T0 + s - 1].double().cpu().numpy() @ W.T + bias
        logp = logits - np.log(np.exp(logits - logits.max(1, keepdims=True)).sum(1, keepdims=True)) - logits.max(1, keepdims=True)
        order = np.lexsort((np.arange(97)[None, :].repeat(ROWS, 0), -logp))[:, :K]
        cand_h = []
        for j in range(K):
            y, _ = _features(m, torch.from_numpy(order[:, j]).to(DEV)[None, :], [tuple(t.clone() for t in pair) for pair in st])
            cand_h.append(y[-1].double().cpu().numpy())
        hist = hs[:T0 + s].double().cpu().numpy()
        for b in range(ROWS):
            sim, values, j, gap = CC.step(np.stack([c[b] for c in cand_h]), logp[b, order[b]], hist[:, b], ALPHA)
            if gap > need:
                assert int(tokens[s, b]) == order[b, j], (s, b, int(tokens[s, b]), order[b].tolist(), values)
                assert abs(float(penalties[s, b]) - sim[j]) <= CC.bound(H) + 1e-5, (s, b)
            else:
                unclear.append((s, b, gap))
    print("unclear steps:", unclear)
    assert not unclear, unclear                                                   # the seeds make every step clear
    assert len({tuple(col) for col in tokens.t().tolist()}) == ROWS               # (the rows differ: the test is not about one sequence)


def test_logprobs_are_scores_and_states_are_features():
    m = _model()
    prompt = _prompt(ROWS, T0)
    tokens, logprobs, lengths, penalties, states = _search()
    lp, ranks, _ = m.score(torch.cat([prompt, tokens]))
    torch.testing.assert_close(logprobs, lp[T0 - 1:], **FP32)
    assert (ranks[T0 - 1:] < K).all()                                             # every token was among its step's k candidates
    _, want = _features(m, torch.cat([prompt, tokens[:-1]]))
    assert len(states) == len(want) == 2
    for got, ref in zip(states, want):
        for a, b in zip(got, ref):
            assert a.shape == b.shape
            torch.testing.assert_close(a, b, **FP32)


def test_no_penalty_and_one_candidate_are_greedy_decoding():
    m = _model()
    prompt = _prompt(ROWS, T0)
    greedy, glp, _ = m.generate(prompt, STEPS, temperature=0)
    for kw in (dict(penalty_alpha=0.0), dict(top_k=1), dict(top_k=1, penalty_alpha=0.0)):
        tokens, logprobs, lengths, penalties, _ = _search(**kw)
        assert torch.equal(tokens, greedy), kw
        torch.testing.assert_close(logprobs, glp, **FP32)
    assert not torch.equal(_search()[0], greedy)                                  # ... and the penalty changes the text


def test_eos_pads_and_counts_as_generate_does():
    m = _model()
    prompt = _prompt(ROWS, T0)
    free = _search(penalty_alpha=0.0)[0]
    eos = int(free[2, 0])                                                         # row 0 emits it at its third step, or earlier
    tokens, logprobs, lengths, penalties, _ = _search(penalty_alpha=0.0, eos=eos)
    gt, glp, glen, _ = m.generate(prompt, STEPS, temperature=0, eos=eos, return_lengths=True)
    assert torch.equal(tokens, gt) and torch.equal(lengths, glen) and lengths.dtype == glen.dtype
    torch.testing.assert_close(logprobs, glp, **FP32)
    assert lengths[0] <= 3 and (tokens[int(lengths[0]):, 0] == eos).all() and (logprobs[int(lengths[0]):, 0] == 0).all()
    # under the penalty: the free run's tokens up to and including the first eos, then padding
    free, flp = _search()[:2]
    eos = int(free[3, 1])
    tokens, logprobs, lengths, penalties, _ = _search(eos=eos)
    for b in range(ROWS):
        hits = (free[:, b] == eos).nonzero()
        n = int(hits[0]) + 1 if len(hits) else STEPS
        assert int(lengths[b]) == n
        assert torch.equal(tokens[:n, b], free[:n, b]) and torch.equal(logprobs[:n, b], flp[:n, b])
        assert (tokens[n:, b] == eos).all() and (logprobs[n:, b] == 0).all() and (penalties[n:, b] == 0).all()
    assert int(lengths[1]) <= 4


def _same_bits(eager, graphed, what):
    assert len(eager) == len(graphed)
    for a, b in zip(eager[:-1], graphed[:-1]):
        assert torch.equal(_bits(a), _bits(b)), what
    for sa, sb in zip(eager[-1], graphed[-1]):
        for a, b in zip(sa, sb):
            assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), what


def test_chunked_replay_is_the_eager_call_bit_for_bit():
    # chunk = 1: the states in front of the last step ARE the replay's incoming states; chunk = steps: one replay
    for kw, chunks in ((dict(), (4, 1, STEPS, 2)), (dict(eos=int(_search()[0][3, 1])), (4, 1))):
        for chunk in chunks:
            _same_bits(_search(**kw), _search(chunk=chunk, **kw), (kw, chunk))
    m, prompt = _model(), _prompt(ROWS, T0)
    plain = m.contrastive_search(prompt, STEPS, K, ALPHA)
    assert len(plain) == 4 and torch.equal(plain[0], _search()[0])                # without return_penalties: four results
    # one step: chunk = 1 is the only chunk there is; the states are the prompt's
    one = m.contrastive_search(prompt, 1, K, ALPHA, return_penalties=True)
    _same_bits(one, m.contrastive_search(prompt, 1, K, ALPHA, return_penalties=True, chunk=1), "steps 1")
    assert torch.equal(one[0], _search()[0][:1])
    _, want = _features(m, prompt)
    for got, ref in zip(one[4], want):
        for a, b in zip(got, ref):
            torch.testing.assert_close(a, b, **FP32)
    # ... and the states of a chunked call are those of features over prompt + tokens[:-1], as the eager call's
    tokens, states = _search(chunk=1)[0], _search(chunk=1)[4]
    _, want = _features(m, torch.cat([prompt, tokens[:-1]]))
    for got, ref in zip(states, want):
        for a, b in zip(got, ref):
            torch.testing.assert_close(a, b, **FP32)


def test_a_graph_of_one_step_keeps_the_states_in_front_of_it():
    from vmlmf_amd import ContrastControls, ContrastGraph, decoding
    m, prompt = _model(), _prompt(ROWS, T0)
    with decoding._activations(m, prompt, None) as (hs, states):
        c = ContrastControls(ROWS, m.hidden_size, _dev(), T0 + 3, K, ALPHA, None, m.vocab_size)
        c.append(hs)
        wide = [tuple(t.repeat_interleave(K, 0) for t in st) for st in states]
        g = ContrastGraph(m, hs[-1], wide, 1, c)
        for r in range(3):
            incoming = [tuple(_bits(t) for t in st) for st in g.states]
            g.replay()
            for sa, sb in zip(g.before, incoming):
                for a, b in zip(sa, sb):
                    assert torch.equal(_bits(a), b), r                            # `before` is what came in, not what went out
            assert any(not torch.equal(_bits(a), b) for sa, sb in zip(g.states, incoming) for a, b in zip(sa, sb))


def test_penalties_are_the_kernels_similarities_and_flags_come_back():
    from vmlmf_amd import ContrastControls, beam_gather, decoding, lm_contrast_step, lm_score
    m = _model()
    prompt = _prompt(ROWS, T0)
    tokens, logprobs, lengths, penalties, _ = _search()
    with decoding._activations(m, prompt, None) as (hs, states):
        c = ContrastControls(ROWS, m.hidden_size, _dev(), T0 + STEPS, K, ALPHA, None, m.vocab_size)
        c.append(hs)
        h = hs[-1]
        states = [tuple(t.repeat_interleave(K, 0) for t in st) for st in states]
        for s in range(STEPS):
            _, _, cand_tok, cand_logp = lm_score(h, m.fc.w, m.fc.b, None, K)
            y, after = decoding.decode_layers(m, m.embed(cand_tok.reshape(-1)).unsqueeze(0), states, "layers")
            tok, lp, chosen, sim, h, src = lm_contrast_step(y[-1], cand_tok, cand_logp, c, parts=1 + s % 3)
            assert torch.equal(tok, tokens[s]) and torch.equal(_bits(lp), _bits(logprobs[s]))
            assert torch.equal(_bits(sim.gather(1, chosen.long()[:, None])[:, 0]), _bits(penalties[s]))
            states = decoding._pairs(beam_gather([t for st in after for t in st], src))
        assert c.hist_len.tolist() == [T0 + STEPS] * ROWS and c.length.tolist() == [STEPS] * ROWS
    m.train(True)
    m.rnns[0].train(False)
    m.contrastive_search(prompt, 2)
    assert m.training and not m.rnns[0].training and m.rnns[1].training and m.fc.training
    m.train(False)
