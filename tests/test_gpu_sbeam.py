"""Model.stochastic_beam_search and its selection launch (vmlmf_sbeam_step, csrc/vmlmf_sbeam.hip) against the fp64 reference of
sbeam_cases.py: every row of every kernel-level case is clear there at every candidate's margin (test_sbeam_cpu.py), so the chosen
candidates are the reference's exactly; totals are compared bit for bit with the plain beam step's; the model-level walk is
teacher-forced over the GPU's own live hypotheses."""
import numpy as np
import pytest
import torch

import sbeam_cases as SC
import vmlmf_decode_oracle as C
from lm_util import DEV, LP_TOL, _prompt, _teacher_forced

pytestmark = pytest.mark.gpu
EOS = SC.EOS


def _embed(V, H):
    return torch.randn(V, H, generator=torch.Generator().manual_seed(5))


def _dev():
    return torch.device(DEV, torch.cuda.current_device())


def _state(seed=SC.NOISE_SEED, offset=SC.NOISE_OFFSET):
    return torch.tensor([seed, offset], dtype=torch.int64, device=DEV)


def _launch(inputs, draw, seed=SC.NOISE_SEED, eos=EOS, own_buffers=True):
    """lm_sbeam_step on CPU inputs (h, w, b, cum, fin, length, T, e) -> (outputs on the CPU, ticket or None)."""
    from vmlmf_amd import StochasticBeams, lm_sbeam_step
    h, w, b, cum, fin, length, T, e = inputs
    B, W = cum.shape
    buffers = StochasticBeams(B, W, w.shape[0], _dev()).buffers() if own_buffers else None
    drawn = torch.full((B,), draw, dtype=torch.int32, device=DEV)
    out = lm_sbeam_step(h.to(DEV), w.to(DEV), b.to(DEV), cum.to(DEV), fin.to(DEV), length.to(DEV), T.to(DEV), drawn, _state(seed), eos,
                        e.to(DEV), buffers=buffers)
    assert len(out) == 9
    return [o.cpu() for o in out], None if buffers is None else buffers[0]


def _step(case, variant="base", draw=0, **kw):
    B, W, H, V = case
    inputs = SC.kernel_case(case, variant) + (_embed(V, H),)
    out, ticket = _launch(inputs, draw, **kw)
    return inputs, out, ticket


def _check_contract(V, inputs, out, draw, eos=EOS):
    """What every step must satisfy whatever its scores: the order on its own perturbed values, gathers, flags, lengths, what a finished
    beam keeps, the first survivor's value."""
    h, w, b, cum, fin, length, T, e = inputs
    parent, token, total, fin_out, len_out, xn, src, pert, drawn = out
    B, W = cum.shape
    assert parent.dtype == torch.int32 and token.dtype == torch.int64 and total.dtype == pert.dtype == torch.float32
    assert fin_out.dtype == len_out.dtype == src.dtype == drawn.dtype == torch.int32
    assert parent.shape == token.shape == total.shape == pert.shape == fin_out.shape == len_out.shape == (B, W) and drawn.shape == (B,)
    assert ((token >= 0) & (token < V)).all() and ((parent >= 0) & (parent < W)).all()
    assert drawn.tolist() == [draw + 1] * B
    flat = parent.long() * V + token
    pT = T.gather(1, parent.long())
    assert not torch.isnan(pert).any() and (pert <= pT).all()                    # no survivor's value exceeds its parent's
    assert torch.equal(pert[:, 0], T.max(1).values)                              # the first survivor inherits the row's largest, to the bit
    for r in range(B):
        assert len(set(flat[r].tolist())) == W
        for s in range(1, W):                                                    # non-increasing, equal values by rising flat index
            assert pert[r, s] < pert[r, s - 1] or (pert[r, s] == pert[r, s - 1] and flat[r, s] > flat[r, s - 1]), (r, s, pert[r], flat[r])
    assert torch.equal(xn, e[token.reshape(-1)])
    assert torch.equal(src.view(B, W), torch.arange(B, dtype=torch.int32)[:, None] * W + parent)
    pfin = fin.gather(1, parent.long()).bool() if eos is not None else torch.zeros((B, W), dtype=torch.bool)
    if eos is not None:
        assert (token[pfin] == eos).all()
        assert torch.equal(fin_out.bool(), pfin | (token == eos))
    assert torch.equal(len_out, length.gather(1, parent.long()) + (~pfin).to(torch.int32))
    assert torch.equal(total[pfin], cum.gather(1, parent.long())[pfin])          # a finished hypothesis keeps its total ...
    assert torch.equal(pert[pfin], pT[pfin])                                     # ... and its value, to the bit


# ---- 1. the step against the reference ----
@pytest.mark.parametrize("draw", SC.DRAWS)
@pytest.mark.parametrize("variant", SC.VARIANTS)
@pytest.mark.parametrize("case", SC.KERNEL_CASES, ids=SC.case_id)
def test_step_against_the_reference(case, variant, draw):
    B, W, H, V = case
    inputs, out, ticket = _step(case, variant, draw)
    _check_contract(V, inputs, out, draw)
    parent, token, total, pert = out[0], out[1], out[2], out[7]
    flat = (parent.long() * V + token).numpy()
    for r, (phi, gt, G, valid, m, top, lo, hi) in enumerate(SC.kernel_oracle(case, variant, draw)):
        assert lo == hi                                                          # every row of these cases is clear (test_sbeam_cpu.py)
        chosen = set(flat[r].tolist())
        assert len(chosen) == W and lo <= chosen <= hi, (case, variant, draw, r, sorted(chosen), top.tolist())
        p, t = parent[r].numpy(), token[r].numpy()
        ref_phi, ref_G, ref_m = phi[p, t], G[p, t], m[p, t]
        fin_ref = np.isfinite(ref_G)
        assert np.array_equal(np.isfinite(pert[r].numpy()), fin_ref) and np.array_equal(np.isfinite(total[r].numpy()), np.isfinite(ref_phi))
        e_phi = np.abs(total[r].double().numpy() - ref_phi)[np.isfinite(ref_phi)]
        e_G = (np.abs(pert[r].double().numpy() - ref_G) / ref_m)[fin_ref]
        print(SC.case_id(case), variant, draw, "row", r, "max |total - phi|", e_phi.max(initial=0.0), "max |perturbed - G| / margin",
              e_G.max(initial=0.0))
        assert e_phi.max(initial=0.0) <= C.KERNEL_MARGIN and e_G.max(initial=0.0) <= 1.0, (case, variant, draw, r)
        assert (pert[r].numpy()[~fin_ref] == -np.inf).all()
    assert int(ticket.abs().sum()) == 0                                          # the ticket words are zero after the launch
    # ... and on the stream's shared buffers, twice: the same bits
    _, again, _ = _step(case, variant, draw, own_buffers=False)
    _, third, _ = _step(case, variant, draw, own_buffers=False)
    for a, b2, c in zip(out, again, third):
        assert torch.equal(a, b2) and torch.equal(a, c)


@pytest.mark.parametrize("variant", SC.VARIANTS)
@pytest.mark.parametrize("case", SC.KERNEL_CASES, ids=SC.case_id)
def test_totals_are_the_plain_beam_steps_bit_for_bit(case, variant):
    """total of a survivor (parent, token) against vmlmf_beam_step's for the same candidate: directly where the plain step keeps it
    too, and for EVERY survivor through the controlled step whose totals are pinned to the plain step's (test_gpu_beam_controls.py):
    on the survivor's batch row with every token but the survivor's closed, every live beam offers that token alone."""
    from vmlmf_amd import BeamControls, StochasticBeams, _beam, _beamctl, _sbeam
    B, W, H, V = case
    h, w, b, cum, fin, length, T = (t.to(DEV) for t in SC.kernel_case(case, variant))
    scores, fin32 = torch.mm(h, w.t()), fin.to(torch.int32)        # ONE GEMM: the three selections below read the same scores
    draw = torch.zeros(B, dtype=torch.int32, device=DEV)
    out = _sbeam.sbeam_select(scores, b, cum, fin32, length, T, draw, _state(), EOS, None, StochasticBeams(B, W, V, _dev()).buffers())
    parent, token, total = out[0].cpu(), out[1].cpu(), out[2].cpu()
    plain = [o.cpu() for o in _beam.beam_select(scores, b, cum, fin32, length, EOS, None)[:3]]
    theirs = {(r, int(p), int(t)): plain[2][r, s] for r in range(B) for s, (p, t) in enumerate(zip(plain[0][r], plain[1][r]))}
    direct = checked = 0
    fin = fin.cpu()
    live = torch.zeros((1, W), dtype=torch.int32, device=DEV)
    for r in range(B):
        sr, cr, lr = scores[r * W:(r + 1) * W], cum[r:r + 1].contiguous(), length[r:r + 1].contiguous()
        by_token = {}
        for s in range(W):
            p, t = int(parent[r, s]), int(token[r, s])
            if (r, p, t) in theirs:
                assert torch.equal(total[r, s], theirs[(r, p, t)]), (case, variant, r, s)
                direct += 1
            if fin[r, p]:
                continue                                                         # (a finished parent: its total is cum, checked elsewhere)
            if t not in by_token:
                ctl = BeamControls(1, W, V, _dev(), banned_tokens=[v for v in range(V) if v != t])
                o = _beamctl.beamctl_select(sr, b, cr, live, lr, -1, None, ctl)
                by_token[t] = {int(pp): tt for pp, tk, tt in zip(o[0][0].cpu(), o[1][0].cpu(), o[2][0].cpu()) if int(tk) == t and not torch.isnan(tt)}
            assert p in by_token[t] and torch.equal(total[r, s], by_token[t][p]), (case, variant, r, s, p, t)
            checked += 1
    print(SC.case_id(case), variant, "bit-equal totals:", direct, "against the plain step itself,", checked, "through the controlled step")
    assert checked == int((~fin.gather(1, parent.long())).sum())


@pytest.mark.parametrize("draw", SC.DRAWS)
@pytest.mark.parametrize("case", SC.DEEP_CASES, ids=SC.case_id)
def test_deep_in_a_search(case, draw):
    """Totals 25 below the values (exp(T - Z) about e^25, as after eight steps of a search), judged by the intervals errors of
    KERNEL_MARGIN in gt leave every G in: where no maximum is in doubt the survivors are the beams' largest children, at their
    parents' values to the bit."""
    B, W, H, V = case
    inputs = SC.deep_case(case) + (_embed(V, H),)
    out, ticket = _launch(inputs, draw)
    _check_contract(V, inputs, out, draw)
    parent, token, total, pert = out[0], out[1], out[2], out[7]
    flat = (parent.long() * V + token).numpy()
    for r, (phi, G, valid, G_lo, G_hi, top, lo, hi) in enumerate(SC.deep_oracle(case, draw)):
        chosen = set(flat[r].tolist())
        assert len(chosen) == W and lo <= chosen <= hi, (case, draw, r, sorted(chosen), top.tolist())
        p, t = parent[r].numpy(), token[r].numpy()
        got = pert[r].double().numpy()
        assert (G_lo[p, t] - 1e-6 <= got).all() and (got <= G_hi[p, t] + 1e-6).all()        # (1e-6: fp32's own rounding of T - ... )
        assert np.abs(total[r].double().numpy() - phi[p, t]).max() <= C.KERNEL_MARGIN
        if lo == hi:
            assert flat[r].tolist() == top.tolist() and torch.equal(pert[r], inputs[6][r].sort(descending=True).values)
    assert int(ticket.abs().sum()) == 0


def test_another_draw_and_another_seed_give_other_tokens():
    case = SC.ODD
    base = _step(case, "base", 0)[1]
    other_draw = _step(case, "base", 5)[1]
    other_seed = _step(case, "base", 0, seed=SC.NOISE_SEED + 1)[1]
    flat = lambda o: o[0].long() * case[3] + o[1]
    assert not torch.equal(flat(base), flat(other_draw)) and not torch.equal(flat(base), flat(other_seed))
    # the reference at that seed agrees (it need not be clear there: the sets decide)
    for r, (phi, gt, G, valid, m, top, lo, hi) in enumerate(SC.kernel_oracle(case, "base", 0, SC.NOISE_SEED + 1)):
        assert lo <= set(flat(other_seed)[r].tolist()) <= hi


@pytest.mark.parametrize("W", [1, 2])
def test_the_statistical_case_equals_the_references_picks(W):
    p, rows = SC.stat_oracle(W)
    inputs = SC.stat_case(W) + (_embed(SC.STAT_V, SC.STAT_H),)
    out, ticket = _launch(inputs, 0, eos=None)
    _check_contract(SC.STAT_V, inputs, out, 0, eos=None)
    parent, token = out[0], out[1]
    assert (parent == 0).all()                                                   # the first step: every survivor from beam 0
    ref = np.array([[int(f) % SC.STAT_V for f in top] for (_, _, _, _, _, top, _, _) in rows])
    assert np.array_equal(token.numpy(), ref)                                    # (every row is clear: the picks AND their order)
    stat, df = SC.stat_statistic(W, token.numpy())
    print("W", W, "chi-square", stat, "df", df)
    assert stat < SC.CHI2_999[df]
    assert int(ticket.abs().sum()) == 0


@pytest.mark.parametrize("case", [SC.ODD, SC.LONG], ids=SC.case_id)
def test_poisoned_outputs_and_workspace_do_not_change_the_result(case):
    from vmlmf_amd import _sbeam
    from vmlmf_amd._lib import ptr
    B, W, H, V = case
    inputs, want, _ = _step(case, "finished", 5)
    h, w, b, cum, fin, length, T, e = (t.to(DEV) for t in inputs)
    scores, fin32 = torch.mm(h, w.t()), fin.to(torch.int32)
    nan, junk = float("nan"), -123456
    parent, fin_o, len_o = (torch.full((B, W), junk, dtype=torch.int32, device=DEV) for _ in range(3))
    token = torch.full((B, W), junk, dtype=torch.int64, device=DEV)
    total, pert = torch.full((B, W), nan, device=DEV), torch.full((B, W), nan, device=DEV)
    xn, src = torch.full((B * W, H), nan, device=DEV), torch.full((B * W,), junk, dtype=torch.int32, device=DEV)
    drawn, draw = torch.full((B,), junk, dtype=torch.int32, device=DEV), torch.full((B,), 5, dtype=torch.int32, device=DEV)
    nbytes = _sbeam.lib().vmlmf_sbeam_workspace_bytes(B, W, V)
    ws = torch.full((nbytes // 4,), -1, dtype=torch.int32, device=DEV)          # all ones: NaN totals, the largest keys
    ticket = torch.zeros(B, dtype=torch.int32, device=DEV)
    state = _state()
    _sbeam.LIBRARY.call(_dev(), "vmlmf_sbeam_step", B, W, H, V, ptr(scores), ptr(b), ptr(cum), ptr(fin32), ptr(length), EOS,
                        ptr(e), ptr(parent), ptr(token), ptr(total), ptr(fin_o), ptr(len_o), ptr(xn), ptr(src), ptr(ticket), ptr(ws), nbytes,
                        ptr(T), ptr(pert), ptr(draw), ptr(drawn), ptr(state))
    for got, ref in zip((parent, token, total, fin_o, len_o, xn, src, pert, drawn), want):
        assert torch.equal(got.cpu(), ref)
    assert int(ticket.abs().sum()) == 0 and draw.tolist() == [5] * B


# ---- 2. the model ----
def _model():
    from vmlmf_amd import Model
    torch.manual_seed(7)
    m = Model(97, 16, 2, 0.0, 1.0, w_rank=8, u_ranks=[8], lstm_type="vmlmf")
    with torch.no_grad():
        m.fc.b[SC.MODEL_EOS] += 2.0
    return m.to(DEV)


def _walk(m, prompt, W, steps, eos, seed):
    """The search step by step - Model.stochastic_beam_search's own prologue, its loop one step at a time: per step (parent, token,
    cum, finished, length, perturbed) on the CPU."""
    from vmlmf_amd import StochasticBeams, dropout_advance
    from vmlmf_amd.decoding import _KeptImages, beam_steps
    B = prompt.shape[1]
    m.eval()
    hist = []
    with torch.no_grad(), _KeptImages(m):
        snap = dropout_advance(m.sampler_state(seed))
        assert snap.tolist() == [seed, 0]
        h, st = m.features(prompt, m.state_init(B))
        h = h[-1].repeat_interleave(W, 0)
        st = [tuple(t.repeat_interleave(W, t.dim() - 2) for t in s) for s in st]
        beams = StochasticBeams(B, W, 97, _dev())
        beams.state = snap
        cum, fin, ln, pert, draw = beams.start()
        for j in range(steps):
            par, tok, h, st, cum, fin, ln, pert, draw = beam_steps(m, h, st, cum, fin, ln, 1, eos, controls=beams, perturbed=pert, draw=draw)
            assert draw.tolist() == [j + 1] * B
            hist.append(tuple(t.cpu() for t in (par[0], tok[0], cum, fin, ln, pert)))
    return hist


def _backtrack_py(parent, token):
    steps, B, W = parent.shape
    out = torch.zeros_like(token)
    for b in range(B):
        for w in range(W):
            cur = w
            for j in range(steps - 1, -1, -1):
                out[j, b, w] = token[j, b, cur]
                cur = int(parent[j, b, cur])
    return out


def test_stochastic_beam_search_teacher_forced():
    m = _model()
    B, W, steps, eos, seed, V = SC.MODEL_B, SC.MODEL_W, SC.MODEL_STEPS, SC.MODEL_EOS, SC.MODEL_SEED, 97
    prompt = _prompt(B, seed=13)
    tokens, scores, perturbed, lengths, states = m.stochastic_beam_search(prompt, steps, beams=W, seed=seed, eos=eos)
    assert tokens.shape == (steps, B, W) and tokens.dtype == torch.int64 and scores.shape == perturbed.shape == lengths.shape == (B, W)
    assert scores.dtype == perturbed.dtype == torch.float32 and lengths.dtype == torch.int32
    tokens, scores, perturbed, lengths = tokens.cpu(), scores.cpu(), perturbed.cpu(), lengths.cpu()
    hist = _walk(m, prompt, W, steps, eos, seed)
    par, tok = torch.stack([s[0] for s in hist]), torch.stack([s[1] for s in hist])
    assert torch.equal(_backtrack_py(par, tok), tokens) and torch.equal(hist[-1][2], scores) and torch.equal(hist[-1][5], perturbed)
    assert torch.equal(hist[-1][4], lengths)
    # every step against the oracle's layers over the GPU's own live hypotheses, the reference's totals and values carried along the
    # GPU's choices; every candidate's value under the interval that errors of model_margin(j) in gt and of the carried tolerance in
    # its parent's value leave it in (sbeam_cases.py says why the kernel-level margin is of no use along a search)
    T0, pc = prompt.shape[0], prompt.cpu()
    oc = np.full((B, W), -np.inf)
    oc[:, 0] = 0.0
    oT, ofin, tolT = oc.copy(), np.zeros((B, W), dtype=bool), np.zeros((B, W))
    clear = []
    for j in range(steps):
        hyps = _backtrack_py(par[:j], tok[:j]) if j else torch.zeros((0, B, W), dtype=torch.int64)
        seqs = torch.cat([pc[:, :, None].expand(T0, B, W), hyps]).reshape(T0 + j, B * W)
        x, _ = C.oracle_last_scores(m, seqs)
        x = x.reshape(B, W, V)
        gum = SC.noise(B, W, V, j, seed, 0)
        new_c, new_T, new_f, new_tol = np.zeros((B, W)), np.zeros((B, W)), np.zeros((B, W), dtype=bool), np.zeros((B, W))
        for b in range(B):
            p, t = par[j, b].numpy(), tok[j, b].numpy()
            phi, G, valid, G_lo, G_hi = SC.sbeam_bounds(x[b], oc[b], oT[b], ofin[b], eos, gum[b], C.model_margin(j), tolT[b])
            chosen = set((p.astype(np.int64) * V + t).tolist())
            _, lo, hi = SC.interval_sets(G, G_lo, G_hi, valid, W)
            assert len(chosen) == W and lo <= chosen <= hi, (j, b, sorted(chosen), sorted(lo), sorted(hi))
            clear.append(lo == hi)
            new_c[b], new_T[b], new_f[b] = phi[p, t], G[p, t], ofin[b, p] | (t == eos)
            new_tol[b] = np.where(np.isfinite(G[p, t]), np.maximum(G_hi[p, t] - G[p, t], G[p, t] - G_lo[p, t]), 0.0)
        # a finished hypothesis is padded with eos; its total and its value stay frozen, to the bit
        if j:
            was = hist[j - 1]
            pf = was[3].gather(1, par[j].long()).bool()
            assert (tok[j][pf] == eos).all() and torch.equal(hist[j][2][pf], was[2].gather(1, par[j].long())[pf])
            assert torch.equal(hist[j][5][pf], was[5].gather(1, par[j].long())[pf])
        oc, oT, ofin, tolT = new_c, new_T, new_f, new_tol
    fin_mask = np.isfinite(oT)
    print("clear rows", int(np.sum(clear)), "of", len(clear), "max |score - fp64|", np.abs(scores.double().numpy() - oc).max(),
          "max |perturbed - fp64|", np.abs(perturbed.double().numpy() - oT)[fin_mask].max())
    assert np.mean(clear) >= 0.9
    assert (np.abs(scores.double().numpy() - oc) <= lengths.numpy() * LP_TOL).all()
    assert (np.abs(perturbed.double().numpy() - oT)[fin_mask] <= tolT[fin_mask]).all()
    assert torch.equal(hist[-1][3].bool(), torch.from_numpy(ofin)) and ofin.any() and not ofin.all()
    for b in range(B):
        assert (perturbed[b, :-1] >= perturbed[b, 1:]).all()
        assert len({tuple(tokens[:, b, w].tolist()) for w in range(W)}) == W          # the hypotheses of a row are pairwise distinct
        for w in range(W):
            hit = (tokens[:, b, w] == eos).nonzero()
            n = int(hit[0]) + 1 if len(hit) else steps
            assert int(lengths[b, w]) == n and (tokens[n:, b, w] == eos).all()
    # scores are Model.score's sums of the hypotheses' log-probabilities
    seq = torch.cat([pc[:, :, None].expand(T0, B, W), tokens]).reshape(T0 + steps, B * W).to(DEV)
    lp = m.score(seq)[0][T0 - 1:].cpu()
    counted = torch.arange(steps)[:, None] < lengths.reshape(1, B * W)
    assert ((lp.double() * counted).sum(0).view(B, W) - scores.double()).abs().le(lengths * LP_TOL).all()
    for h, c in states:
        assert h.shape == c.shape == (B * W, 16)


def _same(a, b):
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    for (h, c), (h2, c2) in zip(a[4], b[4]):
        assert torch.equal(h, h2) and torch.equal(c, c2)


def test_seeds_the_captured_chunk_and_the_empty_call():
    m = _model()
    B, W, steps, eos = SC.MODEL_B, SC.MODEL_W, SC.MODEL_STEPS, SC.MODEL_EOS
    prompt = _prompt(B, seed=13)
    base = m.stochastic_beam_search(prompt, steps, beams=W, seed=5, eos=eos)
    fresh = m.stochastic_beam_search(prompt, steps, beams=W, eos=eos)              # the next call without a seed: another sample
    assert not torch.equal(base[0], fresh[0])
    _same(base, m.stochastic_beam_search(prompt, steps, beams=W, seed=5, eos=eos))   # the same seed: the same bits
    _same(base, m.stochastic_beam_search(prompt, steps, beams=W, seed=5, eos=eos, chunk=4))   # chunk=K: the eager call's bits
    m.stochastic_beam_search(prompt, steps, beams=W, seed=5, eos=eos)
    _same(fresh, m.stochastic_beam_search(prompt, steps, beams=W, eos=eos, chunk=2))   # ... and the second call's after that seed, chunked
    assert not torch.equal(base[0], m.stochastic_beam_search(prompt, steps, beams=W, seed=6, eos=eos)[0])
    empty = m.stochastic_beam_search(prompt, 0, beams=W, seed=5, eos=eos)
    assert empty[0].shape == (0, B, W) and empty[0].dtype == torch.int64 and (empty[3] == 0).all()
    assert empty[1][0].tolist() == empty[2][0].tolist() == [0.0] + [float("-inf")] * (W - 1)
    for h, c in empty[4]:
        assert h.shape == c.shape == (B * W, 16)


def test_one_beam_is_generate_where_the_choice_is_clear():
    m = _model()
    B, steps, V = 3, SC.MODEL_STEPS, 97
    prompt = _prompt(B, seed=3)
    agreed = 0
    for seed in range(6):
        want, _, _ = m.generate(prompt, steps, temperature=1.0, seed=seed)
        z, _ = _teacher_forced(m, prompt, want)
        clear = True
        for j in range(steps):
            gum = SC.noise(B, 1, V, j, seed, 0)
            for b in range(B):
                _, _, _, _, _, top, lo, hi = SC.sbeam_row(z[j, b:b + 1].numpy(), np.zeros(1), np.zeros(1), np.zeros(1, dtype=bool), None, gum[b],
                                                          C.model_margin(j))
                clear = clear and lo == hi and int(top[0]) == int(want[j, b])
        if not clear:
            continue
        got = m.stochastic_beam_search(prompt, steps, beams=1, seed=seed)
        assert torch.equal(got[0][:, :, 0], want), seed
        assert (got[2] == 0).all() and (got[3] == steps).all()                       # one beam: the value stays the root's
        agreed += 1
    print("seeds at which every choice is clear:", agreed, "of 6")
    assert agreed >= 2


# ---- 3. one loop, one graph: the launches a search makes ----
def test_the_search_runs_through_the_one_beam_loop_and_graph(monkeypatch):
    """An eager stochastic_beam_search is beam_steps under a StochasticBeams - per step vmlmf_sbeam_step, then vmlmf_beam_gather, one
    vmlmf_beam_backtrack at the end, never the plain step -, its graph a BeamGraph whose workspace vmlmf_sbeam_workspace_bytes sizes
    (12 bytes a candidate: the plain step's 8 are refused), and two replays of 2 captured steps are the eager call's 4, bit for bit.
    group_beam_search makes its launches in the same order."""
    from lm_util import beam_model
    from vmlmf_amd import BeamGraph, StochasticBeamGraph, _lib, _sbeam, beam_backtrack, dropout_advance
    from vmlmf_amd.decoding import _KeptImages, _widen
    B, W, V, steps, eos = 2, 3, 97, 4, 3
    m = beam_model("plain").to(DEV)
    prompt = _prompt(B, seed=13)
    calls, sized = [], []
    call, workspace_bytes = _lib.Library.call, _lib.Library.workspace_bytes
    monkeypatch.setattr(_lib.Library, "call", lambda self, dev, name, *args: (calls.append(name), call(self, dev, name, *args))[1])
    monkeypatch.setattr(_lib.Library, "workspace_bytes",
                        lambda self, *shape: (sized.append(f"vmlmf_{self.name}_workspace_bytes"), workspace_bytes(self, *shape))[1])
    tokens, scores, perturbed, lengths, _ = m.stochastic_beam_search(prompt, steps, beams=W, seed=5, eos=eos)
    assert calls == ["vmlmf_sbeam_step", "vmlmf_beam_gather"] * steps + ["vmlmf_beam_backtrack"]
    assert "vmlmf_beam_step" not in calls and set(sized) <= {"vmlmf_sbeam_workspace_bytes"}      # (the stream's pair: sbeam's own)
    del calls[:], sized[:]
    m.group_beam_search(prompt, steps, beams=W, groups=W, eos=eos)
    assert calls == ["vmlmf_beamgroup_step", "vmlmf_beam_gather"] * steps + ["vmlmf_beam_backtrack"]
    del calls[:], sized[:]
    m.eval()
    with torch.no_grad(), _KeptImages(m):
        h, st = m.features(prompt, m.state_init(B))
        graph = StochasticBeamGraph(m, h[-1].repeat_interleave(W, 0), _widen(st, W), 2, W, dropout_advance(m.sampler_state(5)), eos)
    assert isinstance(graph, BeamGraph) and graph.controls is graph.beams and graph.beams.state is graph.state
    assert set(sized) == {"vmlmf_sbeam_workspace_bytes"}                                         # not vmlmf_beam_workspace_bytes
    assert calls.count("vmlmf_sbeam_step") == 2 * 2 and "vmlmf_beam_step" not in calls           # the warm-up and the capture
    need = _sbeam.lib().vmlmf_sbeam_workspace_bytes(B, W, V)
    assert need == B * W * W * 12 and graph.buffers[1].numel() * 8 >= need and graph.buffers[0].numel() == B
    replays = [graph.replay() for _ in range(2)]
    parents, toks = (torch.cat(o) for o in zip(*replays))
    assert torch.equal(beam_backtrack(parents, toks), tokens) and torch.equal(graph.cum, scores) and torch.equal(graph.perturbed, perturbed)
    assert torch.equal(graph.length, lengths) and graph.draw.tolist() == [steps] * B
    assert int(graph.buffers[0].abs().sum()) == 0
