"""Model.group_beam_search and its selection launch (vmlmf_beamgroup_step, csrc/vmlmf_beamgroup.hip) against the fp64 reference of
group_beam_cases.py: every group of every kernel-level case is clear there (test_group_beam_cpu.py), so the chosen candidates are the
reference's exactly, in order; groups = 1 and diversity_penalty = 0 are compared bit for bit with vmlmf_beam_step; the model-level tests
are teacher-forced, group by group, over the GPU's own live hypotheses."""
import numpy as np
import pytest
import torch

import group_beam_cases as GC
import vmlmf_decode_oracle as C
from lm_util import DEV, LP_TOL, _oracle_scores, _prompt, _tied_row, beam_model

pytestmark = pytest.mark.gpu
EOS = GC.EOS


def _embed(V, H):
    return torch.randn(V, H, generator=torch.Generator().manual_seed(5))


def _dev():
    return torch.device(DEV, torch.cuda.current_device())


def _step(case, variant="base", groups=None, lam=None, own_buffers=False):
    """lm_beam_step under a GroupBeams on a kernel-level case -> (inputs on the CPU, outputs on the CPU, ticket or None)."""
    from vmlmf_amd import GroupBeams, _beam, lm_beam_step
    B, W, G, H, V, lam0 = case
    h, w, b, cum, fin, length = GC.kernel_case(case, variant)
    e = _embed(V, H)
    controls = GroupBeams(B, W, V, _dev(), G if groups is None else groups, lam0 if lam is None else lam)
    buffers = _beam.new_step_buffers(_dev(), B, W, V) if own_buffers else None
    out = lm_beam_step(h.to(DEV), w.to(DEV), b.to(DEV), cum.to(DEV), fin.to(DEV), length.to(DEV), EOS, e.to(DEV), buffers=buffers,
                       controls=controls)
    assert len(out) == 7
    return (h, w, b, cum, fin, length, e), [o.cpu() for o in out], None if buffers is None else buffers[0]


def _aug32(total, n, lam):
    """The kernel's aug restated on the host: two separately rounded fp32 operations."""
    return np.float32(total) - np.float32(np.float32(lam) * np.float32(n)) if n else np.float32(total)


def _check_contract(W, G, V, lam, inputs, out, eos=EOS):
    """What every group step must satisfy whatever its scores: groups keep to their slots, order by the fp32 aug of the step's own
    totals, gathers, flags, lengths."""
    _, _, _, cum, fin, length, e = inputs
    parent, token, total, fin_out, len_out, xn, src = out
    B, Wg = cum.shape[0], W // G
    assert parent.dtype == torch.int32 and token.dtype == torch.int64 and total.dtype == torch.float32
    assert fin_out.dtype == torch.int32 and len_out.dtype == torch.int32 and src.dtype == torch.int32
    assert parent.shape == token.shape == total.shape == fin_out.shape == len_out.shape == (B, W)
    assert ((token >= 0) & (token < V)).all()
    slot_group = torch.arange(W) // Wg
    assert torch.equal(parent // Wg, slot_group.to(torch.int32).expand(B, W))      # groups never exchange beams
    flat = parent.long() * V + token
    pfin = fin.gather(1, parent.long()).bool() if eos is not None else torch.zeros((B, W), dtype=torch.bool)
    t = total.numpy()
    for b in range(B):
        assert len(set(flat[b].tolist())) == W
        counts = {}
        for g in range(G):
            aug = [t[b, s] if pfin[b, s] else _aug32(t[b, s], counts.get(int(token[b, s]), 0), lam) for s in range(g * Wg, (g + 1) * Wg)]
            for r in range(1, Wg):      # non-increasing aug of the GPU's own totals, equal aug by rising flat index
                s = g * Wg + r
                assert aug[r] < aug[r - 1] or (aug[r] == aug[r - 1] and flat[b, s] > flat[b, s - 1]), (b, g, r, aug, flat[b])
            for s in range(g * Wg, (g + 1) * Wg):
                if not pfin[b, s]:
                    counts[int(token[b, s])] = counts.get(int(token[b, s]), 0) + 1
    if xn is not None:
        assert torch.equal(xn, e[token.reshape(-1)])
    assert torch.equal(src.view(B, W), torch.arange(B, dtype=torch.int32)[:, None] * W + parent)
    if eos is not None:
        assert (token[pfin] == eos).all()                              # a finished beam never offers another token
        assert torch.equal(fin_out.bool(), pfin | (token == eos))
    assert torch.equal(len_out, length.gather(1, parent.long()) + (~pfin).to(torch.int32))
    assert torch.equal(total[pfin], cum.gather(1, parent.long())[pfin])   # ... and at its total so far, to the bit


# ---- 1. the step against the reference ----
@pytest.mark.parametrize("variant", GC.VARIANTS)
@pytest.mark.parametrize("case", GC.KERNEL_CASES, ids=GC.case_id)
def test_group_step_against_the_reference(case, variant):
    B, W, G, H, V, lam = case
    Wg = W // G
    inputs, out, ticket = _step(case, variant, own_buffers=True)
    _check_contract(W, G, V, lam, inputs, out)
    parent, token, total = out[0], out[1], out[2]
    flat = (parent.long() * V + token).numpy()
    for b, (totals, groups) in enumerate(GC.kernel_oracle(case, variant)):
        for g, (aug, valid, top, lo, hi) in enumerate(groups):
            got = flat[b, g * Wg:(g + 1) * Wg]
            assert lo == hi                                            # every group of these cases is clear (test_group_beam_cpu.py)
            assert got.tolist() == top.tolist(), (case, variant, b, g, got.tolist(), top.tolist())
        ref = totals[parent[b].numpy(), token[b].numpy()]              # the RAW totals
        err = np.abs(total[b].double().numpy() - ref)
        err = err[np.isfinite(ref)] if np.isfinite(ref).any() else np.zeros(1)
        print(GC.case_id(case), variant, "row", b, "max |total - fp64|", err.max())
        assert err.max() <= 1e-4, (case, variant, b, err.max())
        assert np.array_equal(np.isfinite(total[b].numpy()), np.isfinite(ref))
    assert int(ticket.abs().sum()) == 0                                # the ticket words are zero after the launch
    # ... and on the stream's shared buffers, twice: bit-equal
    _, again, _ = _step(case, variant)
    _, third, _ = _step(case, variant)
    for a, b2, c in zip(out, again, third):
        assert torch.equal(a, b2) and torch.equal(a, c)
    from vmlmf_amd import _beam
    assert int(_beam.step_buffers(_dev(), B, W, V)[0].abs().sum()) == 0


# ---- 2. one group is the plain step; no penalty is the plain step on B G rows of Wg beams ----
def _selects(case, variant, groups, lam):
    """(the group launch's outputs, a function running vmlmf_beam_step as (B2, W2) on the SAME device buffers), on one scores tensor."""
    from vmlmf_amd import GroupBeams, _beam, _beamgroup
    B, W, G, H, V, _ = case
    h, w, b, cum, fin, length = GC.kernel_case(case, variant)
    e = _embed(V, H).to(DEV)
    scores = torch.mm(h.to(DEV), w.to(DEV).t())
    bias, cum, fin, length = b.to(DEV), cum.to(DEV), fin.to(torch.int32).to(DEV), length.to(DEV)
    got = _beamgroup.group_select(scores, bias, cum, fin, length, EOS, e, GroupBeams(B, W, V, _dev(), groups, lam))
    plain = lambda B2, W2: _beam.beam_select(scores, bias, cum.view(B2, W2), fin.view(B2, W2), length.view(B2, W2), EOS, e)
    return [o.cpu() for o in got], lambda B2, W2: [o.cpu() for o in plain(B2, W2)]


@pytest.mark.parametrize("variant", GC.VARIANTS)
@pytest.mark.parametrize("case", GC.KERNEL_CASES, ids=GC.case_id)
def test_one_group_is_the_plain_step_bit_for_bit(case, variant):
    B, W = case[:2]
    got, plain = _selects(case, variant, 1, case[5])
    for a, b in zip(got, plain(B, W)):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert a.reshape(-1).view(torch.uint8).tolist() == b.reshape(-1).view(torch.uint8).tolist()     # every output, bit-equal


@pytest.mark.parametrize("variant", GC.VARIANTS)
@pytest.mark.parametrize("case", GC.KERNEL_CASES, ids=GC.case_id)
def test_no_penalty_is_the_plain_step_on_each_group(case, variant):
    B, W, G = case[:3]
    Wg = W // G
    got, plain = _selects(case, variant, G, 0.0)
    ref = plain(B * G, Wg)
    names = ["parent", "token", "total", "finished", "length", "x_next", "src_row"]
    offset = (torch.arange(G, dtype=torch.int32) * Wg)[None, :, None]
    for name, a, b in zip(names, got, ref):
        if name == "parent":
            b = (b.view(B, G, Wg) + offset).view(B, W)                 # ... equal after adding g Wg
        assert a.reshape(-1).view(torch.uint8).tolist() == b.reshape(-1).view(torch.uint8).tolist(), name


# ---- 3. ties go to the lower flat index ----
def test_equal_aug_goes_to_the_lower_flat_index():
    from vmlmf_amd import GroupBeams, lm_beam_step
    h, w, bias = _tied_row()
    z = (w.double() @ h.double()).numpy()
    assert z[40] == 2.5 and z[5] == z[20] == z[60] == 2.0 and np.sort(z)[-5] <= 1.0
    V = 97

    def run(cum, G, lam):
        W = cum.shape[1]
        hN = h.to(DEV).expand(W, -1).contiguous()
        zero = torch.zeros((1, W), dtype=torch.int32, device=DEV)
        return [o.cpu() for o in lm_beam_step(hN, w.to(DEV), bias.to(DEV), cum.to(DEV), zero, zero, None,
                                              controls=GroupBeams(1, W, V, _dev(), G, lam))[:3]]
    # group 0 (beam 1 far below): (0, 40), then beam 0's tie group 5 = 20 = 60 half below it, of which 5.  Group 1 (two identical beams
    # at 0): 40 and 5 are penalised once, by 0.5 - (w, 40) now EQUALS 20 and 60, and 5 is half below: the flat index decides among
    # (2, 20), (2, 40), (2, 60), (3, 20) ... - the penalised 40 before 60, behind 20
    parent, token, total = run(torch.tensor([[0.0, -16.0, 0.0, 0.0]]), 2, 0.5)
    assert parent.tolist() == [[0, 0, 2, 2]] and token.tolist() == [[40, 5, 20, 40]]
    t = total.numpy()[0]
    assert t[0] - np.float32(0.5) == t[1] == t[2] and t[3] == t[0]     # the tie is exact in fp32, and the totals are RAW
    # two beams of one group with identical h and cum, Wg = 4: group 0 takes 40, 5, 20, 60 of beam 0; in group 1 (four identical beams)
    # 40 penalised once equals nothing else (5, 20, 60 are penalised too): (4, 40) = (5, 40) = (6, 40) = (7, 40), the beam decides
    parent, token, total = run(torch.tensor([[0.0, -16.0, -16.0, -16.0, 0.0, 0.0, 0.0, 0.0]]), 2, 0.5)
    assert parent.tolist() == [[0, 0, 0, 0, 4, 5, 6, 7]] and token.tolist() == [[40, 5, 20, 60, 40, 40, 40, 40]]
    assert (total[0, 4:] == total[0, 0]).all() and total[0, 1] == total[0, 2] == total[0, 3]
    # ... and under 0.25 the penalised 40 of every beam (a quarter below its raw total) still leads beam 4's penalised 5 = 20 = 60
    parent, token, _ = run(torch.tensor([[0.0, -16.0, -16.0, -16.0, 0.0, 0.0, 0.0, 0.0]]), 2, 0.25)
    assert parent.tolist() == [[0, 0, 0, 0, 4, 5, 6, 7]] and token.tolist() == [[40, 5, 20, 60, 40, 40, 40, 40]]
    # no penalty: identical groups
    parent, token, _ = run(torch.tensor([[0.0, -16.0, 0.0, -16.0]]), 2, 0.0)
    assert parent.tolist() == [[0, 0, 2, 2]] and token.tolist() == [[40, 5, 40, 5]]


# ---- 4. a hand-built row: the penalty flips the choice; a finished beam's eos is no choice ----
def _hand(fin, lam, cum=(0.0, -1.5, 0.0, -1.5)):
    from vmlmf_amd import GroupBeams, _beamgroup
    V, W, G = 12, 4, 2
    x = torch.full((W, V), -20.0)
    x[:, EOS], x[:, 3], x[:, 0], x[:, 1] = 5.0, 4.0, 3.0, 2.0          # eos is every live beam's best token; 3, 0 and 1 follow, a nat apart
    cum_t = torch.tensor([list(cum)])
    fin_t = torch.tensor([fin], dtype=torch.int32)
    zero = torch.zeros((1, W), dtype=torch.int32)
    out = _beamgroup.group_select(x.to(DEV), None, cum_t.to(DEV), fin_t.to(DEV), zero.to(DEV), EOS, None, GroupBeams(1, W, V, _dev(), G, lam))
    parent, token, total = (o.cpu() for o in out[:3])
    totals, groups = GC.group_step(x.double().numpy(), np.array(cum), np.array(fin, dtype=bool), EOS, W, G, lam, C.KERNEL_MARGIN)
    for aug, valid, top, lo, hi in groups:
        assert lo == hi and GC.in_order(aug, top, 0.2)                 # wide gaps: a fifth of a nat at the least
    assert (parent[0].long() * V + token[0]).tolist() == [int(f) for g in groups for f in g[2]]
    assert np.abs(total[0].double().numpy() - totals[parent[0].numpy(), token[0].numpy()]).max() <= 1e-4
    _check_contract(W, G, V, lam, (None, None, None, cum_t, fin_t.bool(), zero, None), [o.cpu() if o is not None else None for o in out])
    return list(zip(parent[0].tolist(), token[0].tolist()))


def test_the_penalty_flips_the_choice_and_a_finished_beams_eos_is_not_counted():
    live = [0, 0, 0, 0]
    # (scores relative to eos: eos 0, token 3 -1, token 0 -2, token 1 -3; beams 1 and 3 start 1.5 below beams 0 and 2)
    # no penalty: both groups take eos, then the runner-up, from their first beam
    assert _hand(live, 0.0) == [(0, EOS), (0, 3), (2, EOS), (2, 3)]
    # group 0 chose eos and 3 once each; under 3.3 group 1's eos (-3.3) and 3 (-4.3) fall behind the fresh tokens 0 (-2) and 1 (-3)
    assert _hand(live, 3.3) == [(0, EOS), (0, 3), (2, 0), (2, 1)]
    # beam 0 finished: it offers eos alone, at its total, and live beam 1's eos comes second - ONE choice of eos, not two: under 0.75
    # group 1's eos (-0.75) still leads 3 (-1); counted twice (-1.5) it would not
    assert _hand([1, 0, 0, 0], 0.75) == [(0, EOS), (1, EOS), (2, EOS), (2, 3)]
    # under 1.5 that one choice flips group 1 to the runner-up token: 3 (-1) before eos (-1.5) ...
    assert _hand([1, 0, 0, 0], 1.5) == [(0, EOS), (1, EOS), (2, 3), (2, EOS)]
    # ... and under 3.3 eos (-3.3) is out: 3 (-1), then 0 (-2), ahead of beam 3's 3 (-2.5)
    assert _hand([1, 0, 0, 0], 3.3) == [(0, EOS), (1, EOS), (2, 3), (2, 0)]
    # both beams of group 0 finished: nothing is counted, group 1 chooses eos unpenalised whatever the penalty
    assert _hand([1, 1, 0, 0], 3.3) == [(0, EOS), (1, EOS), (2, EOS), (2, 3)]
    # a finished beam of group 1 is not penalised: its eos stays at its total so far, in front of live beam 3's fresh token 0
    assert _hand([0, 0, 1, 0], 3.3, cum=(0.0, -1.5, -0.5, -1.5)) == [(0, EOS), (0, 3), (2, EOS), (3, 0)]


def test_a_group_entirely_at_minus_inf_takes_its_lowest_flat_indices():
    """All its totals are -inf, in fp32 as in fp64: the flat index decides exactly; the other groups are what they are without it."""
    from vmlmf_amd import GroupBeams, lm_beam_step
    V, H = 97, 16
    g = torch.Generator().manual_seed(3)
    w, b = torch.randn(V, H, generator=g) * 0.1, torch.randn(V, generator=g)
    for W, G, dead, expect in ((4, 4, [1], {1: [(1, 0)]}), (4, 2, [2, 3], {2: [(2, 0), (2, 1)]}), (6, 3, [2, 3], {2: [(2, 0), (2, 1)]})):
        h = torch.randn(W, H, generator=g)
        cum = -torch.rand(1, W, generator=g)
        cum[0, dead] = float("-inf")
        zero = torch.zeros((1, W), dtype=torch.int32, device=DEV)
        parent, token, total = (o.cpu() for o in lm_beam_step(h.to(DEV), w.to(DEV), b.to(DEV), cum.to(DEV), zero, zero, None,
                                                              controls=GroupBeams(1, W, V, _dev(), G, 0.5))[:3])
        for first, pairs in expect.items():
            n = len(pairs)
            assert list(zip(parent[0, first:first + n].tolist(), token[0, first:first + n].tolist())) == pairs
            assert (total[0, first:first + n] == float("-inf")).all()
        assert torch.isfinite(total).sum() == W - len(dead)


# ---- 5. Model.group_beam_search, teacher-forced group by group ----
def _backtrack_py(parent, token, order=None):
    steps, B, W = parent.shape
    out = torch.zeros_like(token)
    for b in range(B):
        for w in range(W):
            cur = w if order is None else int(order[b, w])
            for j in range(steps - 1, -1, -1):
                out[j, b, w] = token[j, b, cur]
                cur = int(parent[j, b, cur])
    return out


def _history(m, prompt, W, G, lam, steps, eos):
    """The search's per-step (parents, tokens) and its last (cum, finished, length): Model.group_beam_search's own prologue and loop."""
    from vmlmf_amd import GroupBeams
    from vmlmf_amd.decoding import _KeptImages, beam_steps
    B = prompt.shape[1]
    m.eval()
    with torch.no_grad(), _KeptImages(m):
        h, st = m.features(prompt, m.state_init(B))
        h = h[-1].repeat_interleave(W, 0)
        st = [tuple(t.repeat_interleave(W, 0) for t in s) for s in st]
        controls = GroupBeams(B, W, 97, _dev(), G, lam)
        cum, fin, ln = controls.start()
        par, tok, _, st, cum, fin, ln = beam_steps(m, h, st, cum, fin, ln, steps, eos, controls=controls)
    return par.cpu(), tok.cpu(), cum.cpu(), fin.cpu(), ln.cpu()


@pytest.mark.parametrize("kind,B,W,G,lam,seed", GC.MODEL_CASES)
def test_group_beam_search_teacher_forced(kind, B, W, G, lam, seed):
    m = beam_model(kind).to(DEV)
    eos, steps, V, Wg = GC.MODEL_EOS, GC.MODEL_STEPS, 97, W // G
    prompt = _prompt(B, seed=seed)
    tokens, scores, lengths, states = m.group_beam_search(prompt, steps, beams=W, groups=G, diversity_penalty=lam, eos=eos)
    assert tokens.shape == (steps, B, W) and tokens.dtype == torch.int64
    assert scores.shape == (B, W) and scores.dtype == torch.float32 and lengths.shape == (B, W) and lengths.dtype == torch.int32
    par, tok, cum, fin, ln = _history(m, prompt, W, G, lam, steps, eos)
    tokens, scores, lengths = tokens.cpu(), scores.cpu(), lengths.cpu()
    assert torch.equal(_backtrack_py(par, tok), tokens) and torch.equal(cum, scores) and torch.equal(ln, lengths)
    assert torch.equal(par // Wg, (torch.arange(W) // Wg).to(torch.int32).expand(steps, B, W))      # groups never exchange beams
    # every step against the oracle's layers over the GPU's own live hypotheses, every group under the counts of the GPU's own choices
    T0 = prompt.shape[0]
    pc = prompt.cpu()
    oc = np.full((B, W), -np.inf)
    oc[:, ::Wg] = 0.0
    ofin = np.zeros((B, W), dtype=bool)
    clear = []
    for j in range(steps):
        hyps = _backtrack_py(par[:j], tok[:j]) if j else torch.zeros((0, B, W), dtype=torch.int64)
        seqs = torch.cat([pc[:, :, None].expand(T0, B, W), hyps]).reshape(T0 + j, B * W)
        x, _ = C.oracle_last_scores(m, seqs)
        x = x.reshape(B, W, V)
        new_c, new_f = np.zeros((B, W)), np.zeros((B, W), dtype=bool)
        for b in range(B):
            p, t = par[j, b].numpy(), tok[j, b].numpy()
            flat = p.astype(np.int64) * V + t
            forced = [flat[g * Wg:(g + 1) * Wg] for g in range(G)]
            totals, groups = GC.group_step(x[b], oc[b], ofin[b], eos, W, G, lam, C.model_margin(j), forced=forced)
            for g, (aug, valid, top, lo, hi) in enumerate(groups):
                chosen = set(forced[g].tolist())
                assert len(chosen) == Wg and lo <= chosen <= hi, (kind, j, b, g, sorted(chosen), sorted(lo), sorted(hi))
                clear.append(lo == hi)
            new_c[b], new_f[b] = totals[p, t], ofin[b, p] | (t == eos)
        oc, ofin = new_c, new_f
    print(kind, "clear groups", int(np.sum(clear)), "of", len(clear), "max |score - fp64|", np.abs(scores.double().numpy() - oc).max())
    assert np.mean(clear) >= 0.9, (kind, int(np.sum(clear)), len(clear))
    assert (np.abs(scores.double().numpy() - oc) <= lengths.numpy() * LP_TOL).all(), np.abs(scores.double().numpy() - oc).max()
    assert torch.equal(fin.bool(), torch.from_numpy(ofin))
    for b in range(B):
        for w in range(W):
            hit = (tokens[:, b, w] == eos).nonzero()
            n = int(hit[0]) + 1 if len(hit) else steps
            assert int(lengths[b, w]) == n and (tokens[n:, b, w] == eos).all()
    # scores are the sums of the tokens' plain log-probabilities: the model's own layers over every hypothesis
    z, _ = _oracle_scores(m, torch.cat([pc[:, :, None].expand(T0, B, W), tokens]).reshape(T0 + steps, B * W))
    lsm = torch.log_softmax(z[T0 - 1:-1], -1).gather(-1, tokens.reshape(steps, B * W)[..., None])[..., 0]
    counted = torch.arange(steps)[:, None] < lengths.reshape(1, B * W)
    assert ((lsm * counted).sum(0).view(B, W) - scores.double()).abs().le(lengths * LP_TOL).all()
    # (that every state row followed its hypothesis is what the steps above rest on: step j's totals are judged against the oracle's
    # layers over each slot's whole prefix)
    for h, c in states:
        assert h.shape == c.shape == (B * W, 32)


def _same(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for (h, c), (h2, c2) in zip(a[3], b[3]):
        assert torch.equal(h, h2) and torch.equal(c, c2)


def test_determinism_the_captured_chunk_one_group_and_the_length_penalty():
    m = beam_model("plain").to(DEV)
    B, W, G, steps, eos = 3, 6, 3, 12, GC.MODEL_EOS
    Wg = W // G
    prompt = _prompt(B, seed=13)
    kw = dict(beams=W, groups=G, diversity_penalty=0.5, eos=eos)
    base = m.group_beam_search(prompt, steps, **kw)
    _same(base, m.group_beam_search(prompt, steps, **kw))              # two calls: the same bits
    _same(base, m.group_beam_search(prompt, steps, chunk=6, **kw))     # chunk=K: the eager call's bits
    # groups = 1 is beam_search
    _same(m.group_beam_search(prompt, steps, beams=4, groups=1, diversity_penalty=0.5, eos=eos), m.beam_search(prompt, steps, beams=4, eos=eos))
    # no penalty: G identical groups
    flat = m.group_beam_search(prompt, steps, beams=W, groups=G, diversity_penalty=0.0, eos=eos)
    for g in range(1, G):
        assert torch.equal(flat[0][:, :, g * Wg:(g + 1) * Wg], flat[0][:, :, :Wg]) and torch.equal(flat[1][:, g * Wg:(g + 1) * Wg], flat[1][:, :Wg])
    assert not torch.equal(base[0][:, :, Wg:2 * Wg], base[0][:, :, :Wg])       # ... and the penalty tells them apart
    # the length penalty re-sorts within each group, stably: no hypothesis leaves its group
    tokens, scores, lengths, states = (base[0].cpu(), base[1].cpu(), base[2].cpu(), base[3])
    pen = m.group_beam_search(prompt, steps, length_penalty=1.0, **kw)
    _same(pen, m.group_beam_search(prompt, steps, length_penalty=1.0, chunk=6, **kw))
    key = (scores / lengths.float()).view(B, G, Wg)
    order = torch.sort(key, dim=2, descending=True, stable=True).indices + (torch.arange(G) * Wg)[None, :, None]
    order = order.view(B, W)
    assert len(set(lengths.reshape(-1).tolist())) > 1                  # finished beams: the penalty has something to re-sort
    assert (order // Wg == torch.arange(W) // Wg).all()
    for b in range(B):
        assert torch.equal(pen[0][:, b].cpu(), tokens[:, b][:, order[b]])
        assert torch.equal(pen[1][b].cpu(), scores[b][order[b]]) and torch.equal(pen[2][b].cpu(), lengths[b][order[b]])
        pk = (pen[1][b].cpu() / pen[2][b].cpu().float()).view(G, Wg)
        assert (pk[:, :-1] >= pk[:, 1:]).all()                         # each group's block is sorted
        for (h, c), (h2, c2) in zip(states, pen[3]):
            assert torch.equal(h2[b * W:(b + 1) * W].cpu(), h[b * W:(b + 1) * W].cpu()[order[b]])
            assert torch.equal(c2[b * W:(b + 1) * W].cpu(), c[b * W:(b + 1) * W].cpu()[order[b]])
    empty = m.group_beam_search(prompt, 0, **kw)
    assert empty[0].shape == (0, B, W) and (empty[2] == 0).all() and empty[1][0].tolist() == [0.0, float("-inf")] * G


def test_cpu_tensors_raise():
    m = beam_model("plain")
    with pytest.raises(RuntimeError, match="cuda"):
        m.group_beam_search(torch.zeros((3, 2), dtype=torch.int64), 4)
