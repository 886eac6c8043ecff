"""Model.beam_search and its three launches (vmlmf_beam_step / _gather / _backtrack, csrc/vmlmf_beam.hip) against the fp64 oracle of
oracle/vmlmf_decode_oracle.py: a step passes when lo <= chosen <= hi and |chosen| = W (step_sets), and where the oracle is clear (lo == hi)
the chosen set is the oracle's exactly.  The model-level tests are teacher-forced: the oracle's literal layers run over the GPU's own
live hypotheses, so every step is judged on the scores it had in front of it."""
import numpy as np
import pytest
import torch

import vmlmf_decode_oracle as C
from lm_util import DEV, LP_TOL, MARGIN, _check_choices, _oracle_scores, _prompt, _teacher_forced, _tied_row, beam_model, cpu_prompt

pytestmark = pytest.mark.gpu
EOS = C.EOS_KERNEL


def _embed(V, H):
    return torch.randn(V, H, generator=torch.Generator().manual_seed(5))


def _step(case, finished=None, cum=None, own_buffers=False):
    """lm_beam_step on a kernel-level case -> (inputs on the CPU, outputs on the CPU, ticket or None)."""
    from vmlmf_amd import _beam, lm_beam_step
    B, W, H, V = case
    h, w, b, cum0, fin0, length = C.kernel_case(*case)
    cum = cum0 if cum is None else cum
    fin = fin0 if finished is None else finished
    e = _embed(V, H)
    buffers = _beam.new_step_buffers(torch.device(DEV, torch.cuda.current_device()), B, W, V) if own_buffers else None
    out = lm_beam_step(h.to(DEV), w.to(DEV), b.to(DEV), cum.to(DEV), fin.to(DEV), length.to(DEV), EOS, e.to(DEV), buffers=buffers)
    return (h, w, b, cum, fin, length, e), [o.cpu() for o in out], None if buffers is None else buffers[0]


def _check_contract(case, inputs, out):
    """What every step must satisfy whatever its scores: order, gathers, flags, lengths."""
    B, W, H, V = case
    _, _, _, cum, fin, length, e = inputs
    parent, token, total, fin_out, len_out, xn, src = out
    assert parent.dtype == torch.int32 and token.dtype == torch.int64 and total.dtype == torch.float32
    assert fin_out.dtype == torch.int32 and len_out.dtype == torch.int32 and src.dtype == torch.int32
    assert parent.shape == token.shape == total.shape == fin_out.shape == len_out.shape == (B, W)
    assert ((parent >= 0) & (parent < W) & (token >= 0) & (token < V)).all()
    flat = parent.long() * V + token
    t = total.numpy()
    for b in range(B):
        assert len(set(flat[b].tolist())) == W
        for r in range(1, W):      # non-increasing totals of the GPU's own, equal totals by rising flat index
            assert t[b, r] < t[b, r - 1] or (t[b, r] == t[b, r - 1] and flat[b, r] > flat[b, r - 1]), (case, b, r, t[b], flat[b])
    assert torch.equal(xn, e[token.reshape(-1)])
    assert torch.equal(src.view(B, W), torch.arange(B, dtype=torch.int32)[:, None] * W + parent)
    pfin = fin.gather(1, parent.long()).bool()
    assert (token[pfin] == EOS).all()                              # a finished beam never offers another token
    assert torch.equal(fin_out.bool(), pfin | (token == EOS))
    assert torch.equal(len_out, length.gather(1, parent.long()) + (~pfin).to(torch.int32))
    assert torch.equal(total[pfin], cum.gather(1, parent.long())[pfin])   # ... and at its total so far, to the bit


def _check_sets(case, inputs, out, margin=C.KERNEL_MARGIN):
    """lo <= chosen <= hi per batch row against the fp64 oracle of these inputs, the totals to 1e-4; returns clear per row."""
    B, W, H, V = case
    h, w, b, cum, fin = inputs[:5]
    x = (h.double() @ w.double().t() + b.double()).view(B, W, V).numpy()
    clear = []
    for r in range(B):
        totals, valid = C.row_totals(x[r], cum[r].double().numpy(), fin[r].numpy(), EOS)
        top, lo, hi = C.step_sets(totals, valid, W, margin)
        p, t = out[0][r].numpy(), out[1][r].numpy()
        chosen = set((p.astype(np.int64) * V + t).tolist())
        assert len(chosen) == W and lo <= chosen <= hi, (case, r, sorted(chosen), sorted(lo), sorted(hi))
        assert np.abs(out[2][r].double().numpy() - totals[p, t]).max() <= 1e-4
        clear.append(lo == hi)
    return clear


# ---- 1. the step against the oracle ----
@pytest.mark.parametrize("case", C.KERNEL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_beam_step_against_the_oracle(case):
    B, W, H, V = case
    inputs, out, ticket = _step(case, own_buffers=True)
    _check_contract(case, inputs, out)
    parent, token, total = out[0], out[1], out[2]
    for b, (totals, valid, top, lo, hi) in enumerate(C.kernel_oracle(case)):
        chosen = set((parent[b].long() * V + token[b]).tolist())
        assert len(chosen) == W and lo <= chosen <= hi, (case, b, sorted(chosen), sorted(lo), sorted(hi))
        assert lo == hi                                            # every row of these cases is clear (tests/test_beam_cpu.py)
        ref = totals[parent[b].numpy(), token[b].numpy()]
        assert np.abs(total[b].double().numpy() - ref).max() <= 1e-4, (case, b, np.abs(total[b].double().numpy() - ref).max())
    assert int(ticket.abs().sum()) == 0                            # the ticket words are zero after the launch
    # ... and on the stream's shared buffers, twice: bit-equal
    _, again, _ = _step(case)
    _, third, _ = _step(case)
    for a, b2, c in zip(out, again, third):
        assert torch.equal(a, b2) and torch.equal(a, c)
    from vmlmf_amd import _beam
    assert int(_beam.step_buffers(torch.device(DEV, torch.cuda.current_device()), B, W, V)[0].abs().sum()) == 0


# ---- 2. one beam is greedy ----
def test_one_beam_is_greedy():
    from vmlmf_amd import lm_sample
    case = (7, 1, 32, 97)
    none = torch.zeros((7, 1), dtype=torch.bool)
    inputs, out, _ = _step(case, finished=none)
    h, w, b, cum = inputs[:4]
    tok, lp = lm_sample(h.to(DEV), w.to(DEV), b.to(DEV), 0.0, form="gemm")
    assert torch.equal(out[1][:, 0], tok.cpu())
    assert (out[0] == 0).all()
    assert torch.allclose(out[2][:, 0], cum[:, 0] + lp.cpu(), atol=1e-5, rtol=0)
    _check_contract(case, inputs, out)


# ---- 3. ties go to the lower flat index ----
def test_ties_go_to_the_lower_flat_index():
    from vmlmf_amd import lm_beam_step
    h, w, bias = _tied_row()
    z = (w.double() @ h.double()).numpy()
    assert z[40] == 2.5 and z[5] == z[20] == z[60] == 2.0 and np.sort(z)[-5] <= 1.0
    W = 4
    hN = h.to(DEV).expand(W, -1).contiguous()
    zero = torch.zeros((1, W), dtype=torch.int32, device=DEV)
    run = lambda cum: [o.cpu() for o in lm_beam_step(hN, w.to(DEV), bias.to(DEV), cum.to(DEV), zero, zero, None)[:3]]
    # four identical beams at the same total: each beam's best token, the beams in index order
    parent, token, total = run(torch.zeros(1, W))
    assert parent.tolist() == [[0, 1, 2, 3]] and token.tolist() == [[40, 40, 40, 40]]
    assert (total == total[0, 0]).all()
    # distinct exact totals: (0, 40), then (1, 40) a quarter below, then beam 0's tie group 5 = 20 = 60 half below - the boundary
    # falls inside it, and 60 stays out
    parent, token, total = run(torch.tensor([[0.0, -0.25, -16.0, -32.0]]))
    assert parent.tolist() == [[0, 1, 0, 0]] and token.tolist() == [[40, 40, 5, 20]]
    assert total[0, 2] == total[0, 3] and total[0, 0] > total[0, 1] > total[0, 2]
    # ties across beams (identical beams at one total carry identical bits): flat index w V + v decides, the beam first
    parent, token, _ = run(torch.tensor([[0.0, 0.0, 0.0, -32.0]]))
    assert parent.tolist() == [[0, 1, 2, 0]] and token.tolist() == [[40, 40, 40, 5]]
    parent, token, _ = run(torch.tensor([[0.0, 0.0, -32.0, -32.0]]))
    assert parent.tolist() == [[0, 1, 0, 0]] and token.tolist() == [[40, 40, 5, 20]]


# ---- 4. finished beams, and beams that do not exist yet ----
def test_finished_and_missing_beams():
    case = (3, 4, 32, 97)
    B, W, H, V = case
    cum0 = C.kernel_case(*case)[3]
    # all finished, in the order a search leaves them (totals descending): nothing moves
    ordered = cum0.sort(1, descending=True).values
    inputs, out, _ = _step(case, finished=torch.ones((B, W), dtype=torch.bool), cum=ordered)
    _check_contract(case, inputs, out)
    parent, token, total, fin_out, len_out = out[:5]
    assert torch.equal(parent, torch.arange(W, dtype=torch.int32).expand(B, W))
    assert (token == EOS).all() and torch.equal(total, ordered) and torch.equal(len_out, inputs[5]) and (fin_out == 1).all()
    # beams 1 .. W - 1 at -inf (the first step of a search): every survivor extends beam 0, W finite totals
    first = torch.full((B, W), float("-inf"))
    first[:, 0] = 0.0
    none = torch.zeros((B, W), dtype=torch.bool)
    inputs, out, _ = _step(case, finished=none, cum=first)
    _check_contract(case, inputs, out)
    assert (out[0] == 0).all() and torch.isfinite(out[2]).all()
    _check_sets(case, inputs, out)
    # one missing beam among live and finished ones: never chosen
    mixed = cum0.clone()
    mixed[:, 2] = float("-inf")
    inputs, out, _ = _step(case, cum=mixed)
    _check_contract(case, inputs, out)
    _check_sets(case, inputs, out)
    assert (out[0] != 2).all() and torch.isfinite(out[2]).all()


# ---- 5. the state reorder and the read-back ----
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


@pytest.mark.parametrize("H", [32, 650])
def test_gather_and_backtrack_against_stock_ops(H):
    from vmlmf_amd import beam_backtrack, beam_gather
    g = torch.Generator().manual_seed(H)
    rows, L = 12, 2
    tensors = [torch.randn(rows, H, generator=g).to(DEV) for _ in range(2 * L)]
    kept = [t.clone() for t in tensors]
    src = torch.randint(0, rows, (rows,), generator=g).to(torch.int32).to(DEV)
    got = beam_gather(tensors, src)
    assert len(got) == 2 * L
    for t, k, o in zip(tensors, kept, got):
        assert torch.equal(o, k.index_select(0, src.long())) and torch.equal(t, k) and o.data_ptr() != t.data_ptr()
    lstm_shaped = beam_gather([t.view(1, rows, H) for t in tensors[:2]], src)      # nn.LSTM's (1, rows, H) states
    assert lstm_shaped[0].shape == (1, rows, H) and torch.equal(lstm_shaped[1][0], got[1])
    steps, B, W = 7, 3, 4
    parent = torch.randint(0, W, (steps, B, W), generator=g).to(torch.int32)
    token = torch.randint(0, 10000, (steps, B, W), generator=g)
    order = torch.stack([torch.randperm(W, generator=g) for _ in range(B)]).to(torch.int32)
    assert torch.equal(beam_backtrack(parent.to(DEV), token.to(DEV)).cpu(), _backtrack_py(parent, token))
    assert torch.equal(beam_backtrack(parent.to(DEV), token.to(DEV), order.to(DEV)).cpu(), _backtrack_py(parent, token, order))


# ---- 6. Model.beam_search, teacher-forced ----
def _history(m, prompt, W, steps, eos):
    """The search's per-step (parents, tokens) and its last (cum, finished, length): Model.beam_search's own prologue and step loop."""
    from vmlmf_amd.decoding import _KeptImages, beam_steps
    B = prompt.shape[1]
    m.eval()
    with torch.no_grad(), _KeptImages(m):
        h, st = m.features(prompt, m.state_init(B))
        h = h[-1].repeat_interleave(W, 0)
        st = [tuple(t.repeat_interleave(W, 0) for t in s) for s in st]
        cum = torch.full((B, W), float("-inf"), device=DEV)
        cum[:, 0] = 0.0
        zero = torch.zeros((B, W), dtype=torch.int32, device=DEV)
        par, tok, _, st, cum, fin, ln = beam_steps(m, h, st, cum, zero, zero.clone(), steps, eos)
    return par.cpu(), tok.cpu(), cum.cpu(), fin.cpu(), ln.cpu()


@pytest.mark.parametrize("kind,B,W,seed", C.MODEL_CASES)
def test_beam_search_teacher_forced(kind, B, W, seed):
    m = beam_model(kind).to(DEV)
    eos, steps, V = C.MODEL_EOS, C.MODEL_STEPS, 97
    prompt = _prompt(B, seed=seed)
    assert torch.equal(prompt.cpu(), cpu_prompt(B, seed=seed))
    tokens, scores, lengths, states = m.beam_search(prompt, steps, beams=W, eos=eos)
    assert tokens.shape == (steps, B, W) and tokens.dtype == torch.int64
    assert scores.shape == (B, W) and scores.dtype == torch.float32 and lengths.shape == (B, W) and lengths.dtype == torch.int32
    par, tok, cum, fin, ln = _history(m, prompt, W, steps, eos)
    tokens, scores, lengths = tokens.cpu(), scores.cpu(), lengths.cpu()
    assert torch.equal(_backtrack_py(par, tok), tokens) and torch.equal(cum, scores) and torch.equal(ln, lengths)
    # every step against the oracle over the GPU's own live hypotheses
    T0 = prompt.shape[0]
    pc = prompt.cpu()
    oc = np.full((B, W), -np.inf)
    oc[:, 0] = 0.0
    ofin = np.zeros((B, W), dtype=bool)
    clear = []
    for j in range(steps):
        hyps = _backtrack_py(par[:j], tok[:j]) if j else torch.zeros((0, B, W), dtype=torch.int64)
        seqs = torch.cat([pc[:, :, None].expand(T0, B, W), hyps]).reshape(T0 + j, B * W)
        x, _ = C.oracle_last_scores(m, seqs)
        x = x.reshape(B, W, V)
        new_c, new_f = np.zeros((B, W)), np.zeros((B, W), dtype=bool)
        for b in range(B):
            totals, valid = C.row_totals(x[b], oc[b], ofin[b], eos)
            top, lo, hi = C.step_sets(totals, valid, W, C.model_margin(j))
            p, t = par[j, b].numpy(), tok[j, b].numpy()
            chosen = set((p.astype(np.int64) * V + t).tolist())
            assert len(chosen) == W and lo <= chosen <= hi, (kind, j, b, sorted(chosen), sorted(lo), sorted(hi))
            assert valid[p, t].all()
            clear.append(lo == hi)
            new_c[b], new_f[b] = totals[p, t], ofin[b, p] | (t == eos)
        oc, ofin = new_c, new_f
    assert np.mean(clear) >= 0.9, (kind, int(np.sum(clear)), len(clear))
    assert (np.abs(scores.double().numpy() - oc) <= lengths.numpy() * LP_TOL).all(), np.abs(scores.double().numpy() - oc).max()
    # lengths and padding
    assert torch.equal(fin.bool(), torch.from_numpy(ofin)) and 0 < ofin.sum() < ofin.size
    for b in range(B):
        for w in range(W):
            hit = (tokens[:, b, w] == eos).nonzero()
            n = int(hit[0]) + 1 if len(hit) else steps
            assert int(lengths[b, w]) == n and (tokens[n:, b, w] == eos).all()
    # the states have taken in the prompt and every returned token, padding included
    _, ref = _oracle_scores(m, torch.cat([pc[:, :, None].expand(T0, B, W), tokens]).reshape(T0 + steps, B * W))
    for (h, c), (rh, rc) in zip(states, ref):
        assert h.shape == (B * W, 32)
        assert torch.allclose(h.cpu().double(), rh, atol=1e-4, rtol=0) and torch.allclose(c.cpu().double(), rc, atol=1e-4, rtol=0)


# ---- 7. one beam against generate, the length penalty, determinism, the captured chunk ----
def test_one_beam_reproduces_greedy_generate():
    m = beam_model("plain").to(DEV)
    prompt = _prompt(3, seed=13)
    m.train()
    cpu_rng, gpu_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    tokens, scores, lengths, states = m.beam_search(prompt, 12, beams=1)
    assert all(mod.training for mod in m.modules())               # the caller's flags come back
    assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(), gpu_rng)
    assert not hasattr(m, "_sample_state") and not hasattr(m, "_drop_state")     # no generator was created, let alone advanced
    assert tokens.shape == (12, 3, 1) and (lengths == 12).all()
    z, _ = _teacher_forced(m, prompt, tokens[:, :, 0])
    _check_choices(z, tokens[:, :, 0], MARGIN, "one beam")
    lsm = torch.log_softmax(z, -1).gather(-1, tokens[:, :, 0].cpu()[..., None])[..., 0].sum(0)
    assert torch.allclose(scores[:, 0].cpu().double(), lsm, atol=12 * LP_TOL, rtol=0)
    greedy, logprobs, gstates = m.generate(prompt, 12, temperature=0.0)
    assert (greedy == tokens[:, :, 0]).float().mean().item() > 0.9
    if torch.equal(greedy, tokens[:, :, 0]):
        assert torch.allclose(scores[:, 0], logprobs.sum(0), atol=1e-4, rtol=0)
        for (h, c), (gh, gc) in zip(states, gstates):
            assert torch.allclose(h, gh, atol=1e-5) and torch.allclose(c, gc, atol=1e-5)


def test_length_penalty_determinism_and_the_captured_chunk():
    m = beam_model("plain").to(DEV)
    prompt = _prompt(3, seed=13)
    eos, W = C.MODEL_EOS, 4
    base = m.beam_search(prompt, 12, beams=W, eos=eos)
    again = m.beam_search(prompt, 12, beams=W, eos=eos)
    chunked = m.beam_search(prompt, 12, beams=W, eos=eos, chunk=6)
    for other in (again, chunked):
        assert torch.equal(base[0], other[0]) and torch.equal(base[1], other[1]) and torch.equal(base[2], other[2])
        for (h, c), (h2, c2) in zip(base[3], other[3]):
            assert torch.equal(h, h2) and torch.equal(c, c2)
    tokens, scores, lengths, states = base
    assert len(set(lengths.cpu().reshape(-1).tolist())) > 1       # finished beams: the penalty has something to re-sort
    pen = m.beam_search(prompt, 12, beams=W, eos=eos, length_penalty=1.0)
    key = scores.cpu() / lengths.cpu().float()
    order = torch.sort(key, dim=1, descending=True, stable=True).indices
    assert not torch.equal(order, torch.arange(W).expand(3, W))   # ... and does
    for b in range(3):
        assert torch.equal(pen[0][:, b].cpu(), tokens[:, b].cpu()[:, order[b]])
        assert torch.equal(pen[1][b].cpu(), scores[b].cpu()[order[b]]) and torch.equal(pen[2][b].cpu(), lengths[b].cpu()[order[b]])
        for (h, c), (h2, c2) in zip(states, pen[3]):
            assert torch.equal(h2[b * W:(b + 1) * W].cpu(), h[b * W:(b + 1) * W].cpu()[order[b]])
            assert torch.equal(c2[b * W:(b + 1) * W].cpu(), c[b * W:(b + 1) * W].cpu()[order[b]])
    pen_chunked = m.beam_search(prompt, 12, beams=W, eos=eos, length_penalty=1.0, chunk=6)
    assert torch.equal(pen[0], pen_chunked[0]) and torch.equal(pen[1], pen_chunked[1])
    empty = m.beam_search(prompt, 0, beams=W, eos=eos)
    assert empty[0].shape == (0, 3, W) and (empty[2] == 0).all() and empty[1][:, 0].tolist() == [0.0] * 3


def test_cpu_tensors_raise():
    m = beam_model("plain")
    with pytest.raises(RuntimeError, match="cuda"):
        m.beam_search(torch.zeros((3, 2), dtype=torch.int64), 4)


@pytest.mark.parametrize("lstm_type", ["custom", "pytorch"])
def test_stock_layers_run_under_the_same_search(lstm_type):
    """The dense baseline layers and nn.LSTM (states (1, B, H)): scores and states against the model's own forward over each hypothesis."""
    from vmlmf_amd import Model
    torch.manual_seed(9)
    m = Model(97, 32, 2, 0.0, 1.0, lstm_type=lstm_type).to(DEV)
    B, W, steps = 2, 3, 5
    prompt = _prompt(B, seed=6)
    tokens, scores, lengths, states = m.beam_search(prompt, steps, beams=W)
    assert tokens.shape == (steps, B, W) and (lengths == steps).all()
    assert (scores[:, :-1] >= scores[:, 1:]).all()                 # best first
    seq = torch.cat([prompt[:, :, None].expand(-1, B, W), tokens]).reshape(-1, B * W)
    with torch.no_grad():
        z, ref = m(seq, m.state_init(B * W))
    lsm = torch.log_softmax(z.view(seq.shape[0], B * W, -1)[prompt.shape[0] - 1:-1].double(), -1)
    total = lsm.gather(-1, tokens.reshape(steps, B * W)[..., None])[..., 0].sum(0)
    assert torch.allclose(scores.reshape(-1).double(), total, atol=steps * LP_TOL, rtol=0)
    for (h, c), (rh, rc) in zip(states, ref):
        assert h.shape == rh.shape and torch.allclose(h, rh, atol=1e-4) and torch.allclose(c, rc, atol=1e-4)


# ---- 8. the PTB size once ----
def test_ptb_size_against_the_stock_op_step():
    """V 10 000, H 650, two plain layers, B 2, W 4, 6 steps: at every step the selection written with stock ops (log_softmax, add,
    topk, div / mod, embedding, index_select) runs on the same T = 1 layer outputs the kernel saw.  Where the stock totals separate the
    W-th from the (W + 1)-th candidate by more than 1e-4 the token sets are equal; the survivors' totals agree to 1e-4 everywhere."""
    from vmlmf_amd import Model, beam_backtrack, beam_gather, lm_beam_step
    from vmlmf_amd.decoding import _KeptImages, decode_layers
    torch.manual_seed(7)
    m = Model(10000, 650, 2, 0.0, 0.1, w_rank=32, u_ranks=[32], lstm_type="vmlmf").to(DEV).eval()
    B, W, V, steps = 2, 4, 10000, 6
    prompt = _prompt(B, T0=6, V=V, seed=4)
    tokens, scores, lengths, states = m.beam_search(prompt, steps, beams=W)
    separated = 0
    with torch.no_grad(), _KeptImages(m):
        h, st = m.features(prompt, m.state_init(B))
        h = h[-1].repeat_interleave(W, 0)
        st = [tuple(t.repeat_interleave(W, 0) for t in s) for s in st]
        cum = torch.full((B, W), float("-inf"), device=DEV)
        cum[:, 0] = 0.0
        fin = torch.zeros((B, W), dtype=torch.int32, device=DEV)
        ln = fin.clone()
        pars, toks = [], []
        for j in range(steps):
            stock = (cum[:, :, None] + torch.log_softmax(torch.addmm(m.fc.b, h, m.fc.w.t()), -1).view(B, W, V)).view(B, W * V)
            top = stock.topk(W + 1, -1)
            par, tok, cum, fin, ln, x, src = lm_beam_step(h, m.fc.w, m.fc.b, cum, fin, ln, None, m.embed.w)
            for b in range(B):
                if float(top.values[b, W - 1] - top.values[b, W]) > 1e-4:
                    separated += 1
                    assert set(top.indices[b, :W].tolist()) == set((par[b].long() * V + tok[b]).tolist()), (j, b)
            assert torch.allclose(cum, stock.gather(1, par.long() * V + tok), atol=1e-4, rtol=0)
            assert torch.equal(x, m.embed.w[tok.reshape(-1)])
            flat = beam_gather([t for s in st for t in s], src)
            for t, o in zip([t for s in st for t in s], flat):
                assert torch.equal(o, t.index_select(0, src.long()))
            st = [(flat[0], flat[1]), (flat[2], flat[3])]
            y, st = decode_layers(m, x.unsqueeze(0), st, "layers")
            h = y[-1]
            pars.append(par)
            toks.append(tok)
    assert separated >= B * steps // 2, separated               # (gaps at the top of 40 000 candidates are ~1e-2: most steps count)
    assert torch.equal(beam_backtrack(torch.stack(pars), torch.stack(toks)), tokens) and torch.equal(cum, scores)
    assert (lengths == steps).all()
    for (a, c), (a2, c2) in zip(st, states):
        assert torch.equal(a, a2) and torch.equal(c, c2)
