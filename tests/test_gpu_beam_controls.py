"""Model.beam_search under controls (min_length, banned_tokens, no_repeat_ngram_size, banned_sequences) and the launch behind them
(vmlmf_beamctl_step, csrc/vmlmf_beamctl.hip over csrc/vmlmf_beam_core.h) against the fp64 oracle under the same controls
(beam_control_cases.py): a step passes as the plain step does in test_gpu_beam.py - the contract, the order, lo <= chosen <= hi -, and
every row of the masked kernel-level cases is clear (test_beam_controls_cpu.py), so there the chosen set is the oracle's exactly.
With neutral controls the launch is vmlmf_beam_step to the bit.  The model-level tests are teacher-forced, and what the controls
promise is asserted exactly, whatever the tolerances."""
import ctypes

import numpy as np
import pytest
import torch

import beam_control_cases as K
import history_cases as HC
import vmlmf_decode_oracle as C
from abi_arena import FILLS, Arena, assert_same_bits, assert_written, assert_zero
from lm_util import DEV, LP_TOL, _prompt, beam_model, cpu_prompt

pytestmark = pytest.mark.gpu
EOS = K.EOS
NAMES = ["parent", "token", "total", "finished_out", "length_out", "x_next", "src_row"]
I32 = torch.int32


def _embed(V, H):
    return torch.randn(V, H, generator=torch.Generator().manual_seed(5))


_INPUTS = {}


def _inputs(case):
    """A kernel-level case on the device, once: (scores (B W, V) of the head's GEMM, bias, cum, finished int32, length, embed) and the
    same on the CPU (h, w, b, cum, fin bool, length, embed) for the oracle's side."""
    if case not in _INPUTS:
        B, W, H, V = case
        h, w, b, cum, fin, length = C.kernel_case(*case)
        e = _embed(V, H)
        dev = (torch.mm(h.to(DEV), w.to(DEV).t()), b.to(DEV), cum.to(DEV), fin.to(I32).to(DEV), length.to(DEV), e.to(DEV))
        _INPUTS[case] = (dev, (h, w, b, cum, fin, length, e))
    return _INPUTS[case]


def _words(mask):
    return None if mask is None else torch.from_numpy(K.pack(mask)).to(DEV).contiguous()


def ctl_step(scores, bias, cum, fin, length, eos, embed, min_length=0, closed=None, bans=None, hist=None, hist_len=None, cap=1,
             hist_out=None, overflow=None, buffers=None):
    """vmlmf_beamctl_step through its binding's Library on device tensors: closed (V) / bans (B W, V) bool masks or None; hist (B W,
    cap) / hist_len (B W) int32 or None.  Returns the seven outputs and (hist_out, hist_len_out, overflow), all on the CPU."""
    from vmlmf_amd import _beam, _beamctl
    from vmlmf_amd._lib import ptr
    B, W = cum.shape
    V = scores.shape[1]
    H = embed.shape[1]
    dev = scores.device
    ticket, ws = buffers if buffers is not None else _beam.new_step_buffers(dev, B, W, V)
    out = dict(parent=torch.empty((B, W), device=dev, dtype=I32), token=torch.empty((B, W), device=dev, dtype=torch.int64),
               total=torch.empty((B, W), device=dev), finished_out=torch.empty((B, W), device=dev, dtype=I32),
               length_out=torch.empty((B, W), device=dev, dtype=I32), x_next=torch.empty((B * W, H), device=dev),
               src_row=torch.empty(B * W, device=dev, dtype=I32))
    cw, bw = _words(closed), _words(bans)
    len_out = None
    if hist is not None:
        hist_out = torch.full_like(hist, -7) if hist_out is None else hist_out
        len_out = torch.full_like(hist_len, -7)
        overflow = torch.zeros(B, device=dev, dtype=I32) if overflow is None else overflow
    p = lambda t: None if t is None else t.data_ptr()
    c = _beamctl.Controls(min_length, cap, p(cw), p(bw), p(hist), p(hist_len), p(hist_out), p(len_out), p(overflow))
    _beamctl.LIBRARY.call(dev, "vmlmf_beamctl_step", B, W, H, V, ptr(scores), ptr(bias), ptr(cum), ptr(fin), ptr(length), eos, ptr(embed),
                          ctypes.byref(c), *(ptr(out[n]) for n in NAMES[:5]), ptr(out["x_next"]), ptr(out["src_row"]), ptr(ticket), ptr(ws),
                          ws.numel() * 8)
    torch.cuda.synchronize()
    assert int(ticket.abs().sum()) == 0                                  # the ticket words are zero after the launch
    cpu = lambda t: None if t is None else t.cpu()
    return [out[n].cpu() for n in NAMES], (cpu(hist_out), cpu(len_out), cpu(overflow))


def _case_step(case, **kw):
    dev, host = _inputs(case)
    return ctl_step(*dev[:5], EOS, dev[5], **kw)


def _check_contract(case, out, valid_rows, cum=None, fin=None, length=None):
    """What every step must satisfy whatever its scores: types, the order, the gathers, flags, lengths - and that every survivor is a
    candidate its beam offered (valid_rows: per batch row the oracle's (W, V) valid mask)."""
    B, W, H, V = case
    _, _, _, cum0, fin0, length0, e = _inputs(case)[1]
    cum, fin, length = (a if b is None else b for a, b in ((cum0, cum), (fin0, fin), (length0, length)))
    parent, token, total, fin_out, len_out, xn, src = out
    assert parent.dtype == I32 and token.dtype == torch.int64 and total.dtype == torch.float32
    assert ((parent >= 0) & (parent < W) & (token >= 0) & (token < V)).all()
    flat = parent.long() * V + token
    t = total.numpy()
    for b in range(B):
        assert len(set(flat[b].tolist())) == W
        assert valid_rows[b][parent[b].numpy(), token[b].numpy()].all(), (case, b, "a closed candidate was kept")
        for r in range(1, W):
            assert t[b, r] < t[b, r - 1] or (t[b, r] == t[b, r - 1] and flat[b, r] > flat[b, r - 1]), (case, b, r, t[b], flat[b])
    assert torch.equal(xn, e[token.reshape(-1)])
    assert torch.equal(src.view(B, W), torch.arange(B, dtype=I32)[:, None] * W + parent)
    pfin = fin.bool().gather(1, parent.long())
    assert (token[pfin] == EOS).all()
    assert torch.equal(fin_out.bool(), pfin | (token == EOS))
    assert torch.equal(len_out, length.gather(1, parent.long()) + (~pfin).to(I32))
    assert torch.equal(total[pfin], cum.gather(1, parent.long())[pfin])


def _check_sets(case, out, rows):
    """lo <= chosen <= hi per batch row against (totals, valid, top, lo, hi) of the oracle, the totals to 1e-4; returns clear per row."""
    V = case[3]
    clear = []
    for r, (totals, valid, top, lo, hi) in enumerate(rows):
        p, t = out[0][r].numpy(), out[1][r].numpy()
        chosen = set((p.astype(np.int64) * V + t).tolist())
        assert len(chosen) == case[1] and lo <= chosen <= hi, (case, r, sorted(chosen), sorted(lo), sorted(hi))
        assert np.abs(out[2][r].double().numpy() - totals[p, t]).max() <= 1e-4
        clear.append(lo == hi)
    return clear


def _oracle_rows(case, closed=None, bans=None, min_length=0, cum=None, fin=None, length=None):
    B, W, H, V = case
    h, w, b, cum0, fin0, length0, _ = _inputs(case)[1]
    cum, fin, length = (a if b_ is None else b_ for a, b_ in ((cum0, cum), (fin0, fin), (length0, length)))
    x = (h.double() @ w.double().t() + b.double()).view(B, W, V).numpy()
    return [K.controlled_step(x[r], cum[r].double().numpy(), fin[r].bool().numpy(), length[r].numpy(), EOS, W, C.KERNEL_MARGIN, closed,
                              None if bans is None else bans[r * W:(r + 1) * W], min_length) for r in range(B)]


@pytest.fixture(scope="module", autouse=True)
def plain_search_before_and_after():
    """An uncontrolled beam_search before any test of this module has run and after all of them have: the same bits."""
    m = beam_model("plain").to(DEV)
    prompt = _prompt(3, seed=13)
    run = lambda **kw: m.beam_search(prompt, 12, 4, None, C.MODEL_EOS, **kw)          # the old positional call
    before = run(), run(chunk=6)
    yield
    for was, now in zip(before, (run(), run(chunk=6))):
        assert all(torch.equal(a, b) for a, b in zip(was[:3], now[:3]))
        assert all(torch.equal(x, y) for sa, sb in zip(was[3], now[3]) for x, y in zip(sa, sb))
    assert torch.equal(before[0][0], before[1][0]) and torch.equal(before[0][1], before[1][1])


# ---- 1. neutral controls are the plain step, bit for bit ----
@pytest.mark.parametrize("case", K.KERNEL_SHAPES, ids=lambda c: "x".join(map(str, c)))
def test_neutral_controls_are_the_plain_step_to_the_bit(case):
    from vmlmf_amd import _beam
    dev, _ = _inputs(case)
    plain = [o.cpu() for o in _beam.beam_select(*dev[:5], EOS, dev[5])]
    out, hist = _case_step(case)
    assert hist == (None, None, None) and len(out) == len(plain) == 7
    for name, a, b in zip(NAMES, plain, out):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert_same_bits(name, a, b, "between vmlmf_beam_step and vmlmf_beamctl_step under neutral controls")
    # ... and with a history that closes nothing: the seven outputs are still the plain step's
    B, W, H, V = case
    h0 = torch.zeros((B * W, 4), dtype=I32, device=DEV)
    out2, _ = _case_step(case, hist=h0, hist_len=torch.zeros(B * W, dtype=I32, device=DEV), cap=4)
    for name, a, b in zip(NAMES, plain, out2):
        assert_same_bits(name, a, b, "with a history carried")


# ---- 2. masked steps against the oracle ----
@pytest.mark.parametrize("case", K.KERNEL_SHAPES, ids=lambda c: "x".join(map(str, c)))
def test_masked_steps_against_the_oracle(case):
    closed, bans = K.kernel_masks(case)
    rows = K.kernel_oracle(case)
    out, _ = _case_step(case, closed=closed, bans=bans, min_length=K.KERNEL_MIN_LENGTH)
    _check_contract(case, out, [r[1] for r in rows])
    clear = _check_sets(case, out, rows)
    assert all(clear)                                                    # (test_beam_controls_cpu.py: every row is clear)
    V = case[3]
    for r, row in enumerate(rows):
        assert set((out[0][r].long() * V + out[1][r]).tolist()) == set(row[2].tolist())
    again, _ = _case_step(case, closed=closed, bans=bans, min_length=K.KERNEL_MIN_LENGTH)
    for name, a, b in zip(NAMES, out, again):
        assert_same_bits(name, a, b, "between two runs")
    # one control at a time gives the oracle's sets under that control
    for kw in (dict(closed=closed), dict(bans=bans), dict(min_length=K.KERNEL_MIN_LENGTH)):
        one, _ = _case_step(case, **kw)
        rows1 = _oracle_rows(case, **kw)
        _check_contract(case, one, [r[1] for r in rows1])
        _check_sets(case, one, rows1)


# ---- 3. the plain step's own winners, closed ----
@pytest.mark.parametrize("case", [(3, 4, 32, 97), (1, 5, 16, 12293)], ids=lambda c: "x".join(map(str, c)))
def test_closing_the_plain_steps_winners(case):
    B, W, H, V = case
    plain, _ = _case_step(case)
    fin = _inputs(case)[1][4]
    bans = np.zeros((B * W, V), dtype=bool)
    winners = set()
    for b in range(B):
        for r in range(W):
            par, tok = int(plain[0][b, r]), int(plain[1][b, r])
            if not fin[b, par]:                                          # (a finished beam's eos cannot be closed)
                bans[b * W + par, tok] = True
                winners.add((b, par, tok))
    assert len(winners) >= B * W // 2
    out, _ = _case_step(case, bans=bans)
    rows = _oracle_rows(case, bans=bans)
    _check_contract(case, out, [r[1] for r in rows])
    _check_sets(case, out, rows)
    kept = {(b, int(out[0][b, r]), int(out[1][b, r])) for b in range(B) for r in range(W)}
    assert not kept & winners                                            # none of them returns
    # ... and through the shared words: the winners' tokens closed for every beam
    closed = np.zeros(V, dtype=bool)
    closed[[tok for _, _, tok in winners]] = True
    out, _ = _case_step(case, closed=closed)
    rows = _oracle_rows(case, closed=closed)
    _check_contract(case, out, [r[1] for r in rows])
    _check_sets(case, out, rows)
    live = ~fin.gather(1, out[0].long())
    assert not np.isin(out[1][live].numpy(), np.flatnonzero(closed)).any()


# ---- 4. too few candidates ----
def test_a_beam_with_two_open_tokens_and_a_row_with_two_candidates():
    case = (3, 4, 32, 97)
    B, W, H, V = case
    cum = torch.zeros((B, W))
    cum[:, 0] = 50.0                                                     # beam 0 ahead of the others by more than any score's spread
    none = torch.zeros((B, W), dtype=torch.bool)
    dev, _ = _inputs(case)
    bans = np.zeros((B * W, V), dtype=bool)
    bans[0] = True
    bans[0, [11, 60]] = False                                            # batch row 0: beam 0 has two open tokens
    bans[W:2 * W] = True
    bans[W + 2, [4, 90]] = False                                         # batch row 1: two candidates in all, beam 2's
    out, _ = ctl_step(dev[0], dev[1], cum.to(DEV), none.to(I32).to(DEV), dev[4], EOS, dev[5], bans=bans)
    parent, token, total = out[:3]
    # row 0: beam 0 offers its two, first (its totals lead), and the row still fills from the other beams
    assert parent[0, :2].tolist() == [0, 0] and sorted(token[0, :2].tolist()) == [11, 60] and (parent[0, 2:] != 0).all()
    assert torch.isfinite(total[0]).all() and torch.isfinite(total[2]).all()
    h, w, b_, _, _, length, _ = _inputs(case)[1]
    x = (h.double() @ w.double().t() + b_.double()).view(B, W, V).numpy()
    for r in (0, 2):                                                     # (row 1 has no W candidates for the oracle to order)
        totals, valid, top, lo, hi = K.controlled_step(x[r], cum[r].double().numpy(), none[r].numpy(), length[r].numpy(), EOS, W,
                                                       C.KERNEL_MARGIN, None, bans[r * W:(r + 1) * W], 0)
        chosen = set((parent[r].long() * V + token[r]).tolist())
        assert lo <= chosen <= hi and len(chosen) == W
    # row 1: the two candidates in order, then parent 0, token 0 and a NaN total
    assert parent[1].tolist() == [2, 2, 0, 0] and sorted(token[1, :2].tolist()) == [4, 90] and token[1, 2:].tolist() == [0, 0]
    assert total[1, 0] >= total[1, 1] and torch.isnan(total[1, 2:]).all()
    assert out[6].view(B, W)[1].tolist() == [W + 2, W + 2, W, W] and torch.equal(out[5][W + 2:2 * W], dev[5][torch.tensor([0, 0])].cpu())
    assert out[3][1].tolist() == [0, 0, 0, 0] and torch.equal(out[4][1], dev[4].cpu()[1, [2, 2, 0, 0]] + 1)


# ---- 5. min_length ----
def test_min_length_withholds_eos_until_the_length_is_reached():
    B, W, H, V = 1, 3, 16, 97
    g = torch.Generator().manual_seed(3)
    scores = torch.randn(B * W, V, generator=g)
    bias = torch.zeros(V)
    bias[EOS] = 20.0                                                     # eos is every beam's best candidate by far
    e = _embed(V, H)
    cum = torch.tensor([[0.0, -1.0, -2.0]])
    length = torch.tensor([[2, 3, 4]], dtype=I32)
    run = lambda fin, ml: ctl_step(scores.to(DEV), bias.to(DEV), cum.to(DEV), torch.tensor([fin], dtype=I32).to(DEV), length.to(DEV), EOS,
                                   e.to(DEV), min_length=ml)[0]
    parent, token, total, fin_out, len_out = run([0, 0, 0], 0)[:5]
    assert parent.tolist() == [[0, 1, 2]] and token.tolist() == [[EOS] * 3]
    parent, token, total, fin_out, len_out = run([0, 0, 0], 3)[:5]       # length 2 < 3: beam 0 withholds eos; 3 == 3 and 4: chosen
    pairs = list(zip(parent[0].tolist(), token[0].tolist()))
    assert pairs[0] == (1, EOS) and pairs[1] == (2, EOS) and pairs[2][0] == 0 and pairs[2][1] != EOS
    assert pairs[2][1] == int((scores[0] + bias).masked_fill(torch.arange(V) == EOS, -1e9).argmax())
    assert fin_out.tolist() == [[1, 1, 0]] and len_out.tolist() == [[4, 5, 3]]
    parent, token, total, fin_out, len_out = run([0, 0, 0], 5)[:5]       # below it, nobody offers eos
    assert (token != EOS).all() and (fin_out == 0).all()
    parent, token, total, fin_out, len_out = run([1, 0, 0], 5)[:5]       # a finished beam keeps offering eos, whatever its length
    assert (int(parent[0, 0]), int(token[0, 0])) == (0, EOS) and float(total[0, 0]) == 0.0 and (token[0, 1:] != EOS).all()
    assert fin_out.tolist() == [[1, 0, 0]] and int(len_out[0, 0]) == 2


# ---- 6. the histories ----
@pytest.mark.parametrize("case,cap", [((3, 4, 32, 97), 9), ((2, 32, 32, 97), 300), ((1, 5, 16, 12293), 6)], ids=["small", "W32", "long_row"])
def test_the_histories_follow_their_hypotheses(case, cap):
    B, W, H, V = case
    rng = np.random.Generator(np.random.PCG64(cap))
    hist_len = rng.integers(0, cap + 1, B * W)
    hist_len[::3] = cap                                                  # full histories among them ...
    fin = _inputs(case)[1][4]
    for b, row in enumerate(C.kernel_oracle(case)):                      # ... one of them a live parent the step is sure to keep
        hist_len[b * W + next(int(f) // V for f in row[2] if not fin[b, int(f) // V])] = cap
    hist = 1000 + rng.integers(0, 5000, (B * W, cap))                    # no token of the vocabulary looks like a history word here ...
    hist = np.where(np.arange(cap)[None] < hist_len[:, None], hist, -3)  # ... and what lies behind a length is marked
    hd, ld = torch.from_numpy(hist).to(I32).to(DEV), torch.from_numpy(hist_len).to(I32).to(DEV)
    guarded = torch.full((B * W * cap + 64,), -9, dtype=I32, device=DEV)  # hist_out, with guard words behind its last row
    out, (hist_out, len_out, overflow) = _case_step(case, hist=hd, hist_len=ld, cap=cap, hist_out=guarded[:B * W * cap].view(B * W, cap))
    plain, _ = _case_step(case)
    for name, a, b in zip(NAMES, plain, out):
        assert_same_bits(name, a, b, "with a history carried")
    want, want_len, want_over = K.next_histories(hist, hist_len, cap, out[0].numpy(), out[1].numpy(), fin.numpy())
    assert len_out.tolist() == want_len and overflow.tolist() == want_over
    assert sum(want_over) == B and any(fin[b, int(out[0][b, r])] for b in range(B) for r in range(W))   # full and finished parents occur
    for slot, row in enumerate(want):
        assert hist_out[slot, :len(row)].tolist() == row, slot
        assert (hist_out[slot, len(row):] == -9).all(), slot             # nothing is written behind the new length, let alone the row
    assert (guarded[B * W * cap:] == -9).all()
    assert torch.equal(hd.cpu(), torch.from_numpy(hist).to(I32))          # the inputs are not written


def test_the_beams_ban_sets_are_the_rows_ban_sets():
    from vmlmf_amd import BeamControls
    B, W, V, cap = 3, 4, 97, 24
    rng = np.random.Generator(np.random.PCG64(11))
    alphabet = rng.choice(V, 6, replace=False)
    seqs = [[int(alphabet[0]), int(alphabet[1])], [int(alphabet[2])], [int(alphabet[3]), int(alphabet[4]), int(alphabet[5])]]
    for n in (2, 3, 0):
        c = BeamControls(B, W, V, DEV, capacity=cap, no_repeat_ngram_size=n, banned_sequences=seqs)
        hist_len = rng.integers(0, cap + 1, B * W)
        hist = alphabet[rng.integers(0, 6, (B * W, cap))]
        words = c.beam_bans(torch.from_numpy(hist).to(I32).to(DEV), torch.from_numpy(hist_len).to(I32).to(DEV))
        assert tuple(words.shape) == (B * W, 4) and words.dtype == I32
        got = HC.unpack(words.cpu().numpy(), V)
        want = np.stack([HC.ban_set(hist[r, :hist_len[r]], V, n, seqs) for r in range(B * W)])
        assert np.array_equal(got, want) and want.sum(1).min() >= 1 and (n == 0 or want.sum(1).max() >= 3)
        assert np.array_equal(K.pack(want), words.cpu().numpy())         # the layout the step reads is the layout it is written in


def test_lm_beam_step_under_beam_controls_carries_the_histories():
    """The Python path of one step: BeamControls from tokens and sequences, lm_beam_step(controls=, hist=, hist_len=) - the ban launch
    and the step - against the oracle under the same controls, and the survivors' histories behind the seven results."""
    from vmlmf_amd import BeamControls, lm_beam_step
    case = (3, 4, 32, 97)
    B, W, H, V = case
    h, w, b, cum, fin, length, e = _inputs(case)[1]
    prompt = cpu_prompt(B, T0=6, V=12, seed=2)                            # a 12-token alphabet: bigrams repeat
    banned, seqs = [1, 40, 96], [[int(prompt[-1, 0]), 50], [60]]
    c = BeamControls(B, W, V, DEV, prompt=prompt.to(DEV), capacity=8, min_length=K.KERNEL_MIN_LENGTH, banned_tokens=banned,
                     no_repeat_ngram_size=2, banned_sequences=seqs, eos=EOS)
    hist, hist_len = c.history()
    out = lm_beam_step(h.to(DEV), w.to(DEV), b.to(DEV), cum.to(DEV), fin.to(DEV), length.to(DEV), EOS, e.to(DEV), controls=c, hist=hist,
                       hist_len=hist_len)
    assert len(out) == 9
    out, (h1, l1) = [o.cpu() for o in out[:7]], (out[7].cpu(), out[8].cpu())
    bans = np.repeat(np.stack([HC.ban_set(prompt[:, r].tolist(), V, 2, seqs) for r in range(B)]), W, 0)
    assert bans.sum(1).min() >= 1 and bans.sum(1).max() >= 2
    rows = _oracle_rows(case, closed=np.isin(np.arange(V), banned), bans=bans, min_length=K.KERNEL_MIN_LENGTH)
    _check_contract(case, out, [r[1] for r in rows])
    _check_sets(case, out, rows)
    want, want_len, over = K.next_histories(hist.cpu().numpy(), hist_len.cpu().numpy(), 8, out[0].numpy(), out[1].numpy(), fin.numpy())
    assert l1.tolist() == want_len and over == [0] * B and c.overflow.tolist() == [0] * B
    for slot, row in enumerate(want):
        assert h1[slot, :len(row)].tolist() == row
    with pytest.raises(RuntimeError, match="hist must be"):
        lm_beam_step(h.to(DEV), w.to(DEV), b.to(DEV), cum.to(DEV), fin.to(DEV), length.to(DEV), EOS, e.to(DEV), controls=c)
    with pytest.raises(ValueError, match="eos"):
        lm_beam_step(h.to(DEV), w.to(DEV), b.to(DEV), cum.to(DEV), fin.to(DEV), length.to(DEV), 5, e.to(DEV), controls=c, hist=hist,
                     hist_len=hist_len)


# ---- 7. the C ABI on poisoned, exactly sized buffers ----
def test_the_entry_point_on_poisoned_exactly_sized_buffers():
    from vmlmf_amd import _beamctl
    B, W, H, V, cap = 3, 5, 33, 97, 7
    r = np.random.Generator(np.random.PCG64(sum(map(ord, "beamctl"))))
    scores, bias = r.standard_normal((B * W, V)).astype(np.float32), (0.1 * r.standard_normal(V)).astype(np.float32)
    emb = r.standard_normal((V, H)).astype(np.float32)
    cum = -np.abs(r.standard_normal((B, W))).astype(np.float32)
    fin, ln = np.zeros((B, W), np.int32), np.full((B, W), 2, np.int32)
    fin[1, 2] = 1
    closed, bans = r.random(V) < 0.2, r.random((B * W, V)) < 0.2
    closed[7], bans[:, 7] = False, False
    hist_len = r.integers(0, cap + 1, B * W).astype(np.int32)
    hist_len[:4] = cap
    hist = r.integers(0, V, (B * W, cap)).astype(np.int32)
    nws = int(_beamctl.lib().vmlmf_beamctl_workspace_bytes(B, W, V))
    dev = torch.device("cuda", torch.cuda.current_device())
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    outs = ["parent", "token", "total", "finished_out", "length_out", "x_next", "src_row", "hist_len_out"]
    runs = []
    for fill in FILLS:
        arena = Arena(DEV, fill, capacity=1 << 20)
        a = lambda name, shape, dtype=torch.float32, init=None: arena.buf(shape, dtype, init=init, name=name)
        b = dict(scores=a("scores", (B * W, V), init=scores), bias=a("bias", V, init=bias), embed=a("embed", (V, H), init=emb),
                 cum=a("cum", (B, W), init=cum), finished=a("finished", (B, W), I32, fin), length=a("length", (B, W), I32, ln),
                 closed=a("closed", (V + 31) // 32, I32, K.pack(closed)), bans=a("bans", (B * W, (V + 31) // 32), I32, K.pack(bans)),
                 hist=a("hist", (B * W, cap), I32, hist), hist_len=a("hist_len", B * W, I32, hist_len),
                 parent=a("parent", (B, W), I32), token=a("token", (B, W), torch.int64), total=a("total", (B, W)),
                 finished_out=a("finished_out", (B, W), I32), length_out=a("length_out", (B, W), I32), x_next=a("x_next", (B * W, H)),
                 src_row=a("src_row", B * W, I32), hist_out=a("hist_out", (B * W, cap), I32), hist_len_out=a("hist_len_out", B * W, I32),
                 overflow=a("overflow", B, I32, 0), ticket=a("ticket", B, I32, 0), workspace=a("workspace", nws, torch.uint8))
        c = _beamctl.Controls(3, cap, *(b[n].data_ptr() for n in ("closed", "bans", "hist", "hist_len", "hist_out", "hist_len_out", "overflow")))
        _beamctl.LIBRARY.call(dev, "vmlmf_beamctl_step", B, W, H, V, p(b["scores"]), p(b["bias"]), p(b["cum"]), p(b["finished"]), p(b["length"]), 7,
                              p(b["embed"]), ctypes.byref(c), p(b["parent"]), p(b["token"]), p(b["total"]), p(b["finished_out"]),
                              p(b["length_out"]), p(b["x_next"]), p(b["src_row"]), p(b["ticket"]), p(b["workspace"]), nws)
        torch.cuda.synchronize()
        arena.check_guards()
        for name in outs:
            assert_written(arena, name, b[name])
        assert_zero("ticket", b["ticket"])
        got = {name: b[name].clone() for name in outs + ["overflow", "hist_out"]}
        # hist_out: the defined prefix of every slot is written, what lies behind it still holds the fill
        left = arena.unwritten(b["hist_out"]).cpu()
        for slot, L in enumerate(got["hist_len_out"].tolist()):
            assert left[slot, L:].all() and (fill == FILLS[0] or not left[slot, :L].any()), (hex(fill), slot, L)
        runs.append({k: v.cpu() for k, v in got.items()})
    for fill, run in zip(FILLS[1:], runs[1:]):
        for name in outs + ["overflow"]:
            assert_same_bits(name, runs[0][name], run[name], f"between the fills 0x{FILLS[0]:08x} and 0x{fill:08x}")
    got = runs[0]
    x = scores.astype(np.float64) + bias
    rows = [K.controlled_step(x[i * W:(i + 1) * W], cum[i].astype(np.float64), fin[i].astype(bool), ln[i], 7, W, C.KERNEL_MARGIN, closed,
                              bans[i * W:(i + 1) * W], 3) for i in range(B)]
    for i, (totals, valid, top, lo, hi) in enumerate(rows):
        chosen = set((got["parent"][i].long() * V + got["token"][i]).tolist())
        assert lo <= chosen <= hi and len(chosen) == W
        assert np.abs(got["total"][i].double().numpy() - totals[got["parent"][i].numpy(), got["token"][i].numpy()]).max() <= 1e-4
    want, want_len, over = K.next_histories(hist, hist_len, cap, got["parent"].numpy(), got["token"].numpy(), fin.astype(bool))
    assert got["hist_len_out"].tolist() == want_len and got["overflow"].tolist() == over and sum(over) > 0
    for slot, row in enumerate(want):
        assert got["hist_out"][slot, :len(row)].tolist() == row
    assert torch.equal(got["x_next"], torch.tensor(emb)[got["token"].reshape(-1)])


# ---- 8. Model.beam_search under the three settings ----
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


def _search_steps(m, prompt, W, steps, eos, kw):
    """The search's per-step (parents, tokens) and its last (cum, finished, length): Model.beam_search's own prologue and step loop."""
    from vmlmf_amd import BeamControls
    from vmlmf_amd.decoding import _KeptImages, beam_steps
    T0, B = prompt.shape
    m.eval()
    with torch.no_grad(), _KeptImages(m):
        h, st = m.features(prompt, m.state_init(B))
        h = h[-1].repeat_interleave(W, 0)
        st = [tuple(t.repeat_interleave(W, 0) for t in s) for s in st]
        cum = torch.full((B, W), float("-inf"), device=DEV)
        cum[:, 0] = 0.0
        zero = torch.zeros((B, W), dtype=I32, device=DEV)
        c = BeamControls(B, W, 97, DEV, prompt=prompt, capacity=T0 + steps, eos=eos, **kw)
        par, tok, _, st, cum, fin, ln, hist, hist_len = beam_steps(m, h, st, cum, zero, zero.clone(), steps, eos, controls=c)
    assert c.overflow.tolist() == [0] * B
    return par.cpu(), tok.cpu(), cum.cpu(), fin.cpu(), ln.cpu(), hist.cpu(), hist_len.cpu()


@pytest.mark.parametrize("name", K.SETTINGS)
@pytest.mark.parametrize("kind,B,W,seed", C.MODEL_CASES)
def test_beam_search_under_controls_teacher_forced(kind, B, W, seed, name):
    m = beam_model(kind).to(DEV)
    eos, steps, V = K.MODEL_EOS, K.MODEL_STEPS, 97
    kw = K.setting(name, kind, B, W, seed)
    n, min_length, seqs = kw["no_repeat_ngram_size"], kw.get("min_length", 0), kw.get("banned_sequences", [])
    prompt = _prompt(B, seed=seed)
    pc = prompt.cpu()
    T0 = pc.shape[0]
    tokens, scores, lengths, states = m.beam_search(prompt, steps, beams=W, eos=eos, **kw)
    assert tokens.shape == (steps, B, W) and tokens.dtype == torch.int64 and scores.dtype == torch.float32 and lengths.dtype == I32
    par, tok, cum, fin, ln, hist, hist_len = _search_steps(m, prompt, W, steps, eos, kw)
    tokens, scores, lengths = tokens.cpu(), scores.cpu(), lengths.cpu()
    assert torch.equal(_backtrack_py(par, tok), tokens) and torch.equal(cum, scores) and torch.equal(ln, lengths)
    # every step against the oracle under the controls, over the GPU's own live hypotheses
    oc = np.full((B, W), -np.inf)
    oc[:, 0] = 0.0
    ofin, olen = np.zeros((B, W), dtype=bool), np.zeros((B, W), dtype=np.int64)
    clear = []
    for j in range(steps):
        hyps = _backtrack_py(par[:j], tok[:j]) if j else torch.zeros((0, B, W), dtype=torch.int64)
        seq_in = torch.cat([pc[:, :, None].expand(T0, B, W), hyps]).reshape(T0 + j, B * W)
        x, _ = C.oracle_last_scores(m, seq_in)
        x = x.reshape(B, W, V)
        new_c, new_f, new_l = np.zeros((B, W)), np.zeros((B, W), dtype=bool), np.zeros((B, W), dtype=np.int64)
        for b in range(B):
            bans = np.stack([HC.ban_set(seq_in[:, b * W + w].tolist(), V, n, seqs) for w in range(W)])
            totals, valid, top, lo, hi = K.controlled_step(x[b], oc[b], ofin[b], olen[b], eos, W, C.model_margin(j), None, bans, min_length)
            p, t = par[j, b].numpy(), tok[j, b].numpy()
            chosen = set((p.astype(np.int64) * V + t).tolist())
            assert len(chosen) == W and lo <= chosen <= hi, (kind, name, j, b, sorted(chosen), sorted(lo), sorted(hi))
            assert valid[p, t].all()
            clear.append(lo == hi)
            new_c[b], new_f[b], new_l[b] = totals[p, t], ofin[b, p] | (t == eos), olen[b, p] + ~ofin[b, p]
        oc, ofin, olen = new_c, new_f, new_l
    print(f"{kind} {B}x{W} {name}: clear share {np.mean(clear):.3f}")
    assert np.mean(clear) >= 0.9, (kind, name, int(np.sum(clear)), len(clear))
    assert (np.abs(scores.double().numpy() - oc) <= lengths.numpy() * LP_TOL).all(), np.abs(scores.double().numpy() - oc).max()
    assert torch.equal(fin.bool(), torch.from_numpy(ofin)) and np.array_equal(lengths.numpy(), olen)
    # what the controls promise, exactly - whatever the tolerances above
    z, _ = C._oracle_scores(m, torch.cat([pc[:, :, None].expand(T0, B, W), tokens]).reshape(T0 + steps, B * W))
    lsm = torch.log_softmax(z[T0 - 1:T0 - 1 + steps], -1).gather(-1, tokens.reshape(steps, B * W)[..., None])[..., 0]
    for b in range(B):
        for w in range(W):
            L = int(lengths[b, w])
            hyp = K.until_eos(tokens[:, b, w], eos)
            assert len(hyp) == L and (tokens[L:, b, w] == eos).all()
            whole = pc[:, b].tolist() + hyp
            assert K.repeated_ngrams(whole, n) == 0, (b, w, whole)       # no n-gram twice, the prompt included
            assert not any(K.contains(whole, s) for s in seqs), (b, w, whole)
            assert L >= min_length or eos not in hyp                     # no hypothesis finishes below min_length
            assert (eos in hyp) == bool(fin[b, w])
            # the score is the sum of the hypothesis' plain log-probabilities: the controls changed no total
            assert abs(float(scores[b, w]) - float(lsm[:L, b * W + w].sum())) <= L * LP_TOL
            # the carried history is the prompt and the hypothesis
            assert hist[b * W + w, :int(hist_len[b * W + w])].tolist() == whole
    assert (lengths >= min_length).all() or min_length == 0


def test_banned_tokens_and_min_length_alone_keep_no_history():
    from vmlmf_amd import _history
    m = beam_model("plain").to(DEV)
    prompt = _prompt(3, seed=13)
    eos, W, steps = K.MODEL_EOS, 4, 12
    plain = m.beam_search(prompt, steps, beams=W, eos=eos)
    used = sorted(set(plain[0][0].reshape(-1).tolist()) - {eos})[:3]      # tokens the plain search starts with
    tokens, scores, lengths, _ = m.beam_search(prompt, steps, beams=W, eos=eos, banned_tokens=used, min_length=5)
    assert not np.isin(tokens.cpu().numpy(), used).any() and (lengths >= 5).all()
    assert not torch.equal(tokens, plain[0]) and int((plain[2] < 5).sum()) > 0
    z, _ = C._oracle_scores(m, torch.cat([prompt.cpu()[:, :, None].expand(-1, 3, W), tokens.cpu()]).reshape(-1, 3 * W))
    lsm = torch.log_softmax(z[4:4 + steps], -1).gather(-1, tokens.cpu().reshape(steps, 3 * W)[..., None])[..., 0]
    for r in range(3 * W):
        L = int(lengths.reshape(-1)[r])
        assert abs(float(scores.reshape(-1)[r]) - float(lsm[:L, r].sum())) <= L * LP_TOL


# ---- 9. one beam is greedy generate under the same controls ----
@pytest.mark.parametrize("kind,seed", [("plain", 13), ("group", 11)])
def test_one_beam_with_controls_reproduces_greedy_generate(kind, seed):
    m = beam_model(kind).to(DEV)
    prompt = _prompt(3, seed=seed)
    eos, steps = K.MODEL_EOS, 16
    free = m.generate(prompt, steps, temperature=0.0, eos=eos)[0]
    seqs = [free[:2, 0].tolist(), free[1:4, 1].tolist()]
    kw = dict(min_length=6, banned_tokens=[next(int(t) for t in free[:, 2] if int(t) != eos)], no_repeat_ngram_size=2, banned_sequences=seqs)
    greedy, logprobs, glen, _ = m.generate(prompt, steps, temperature=0.0, eos=eos, return_lengths=True, **kw)
    tokens, scores, lengths, _ = m.beam_search(prompt, steps, beams=1, eos=eos, **kw)
    assert not torch.equal(greedy, free)                                 # the controls bite
    assert torch.equal(tokens[:, :, 0], greedy)                          # token for token
    assert torch.equal(lengths[:, 0], glen)
    assert torch.allclose(scores[:, 0], logprobs.sum(0), atol=steps * LP_TOL, rtol=0)


# ---- 10. the captured chunk, a graph replayed twice, two identical calls ----
def test_chunk_graph_replays_and_repeats_are_the_eager_bits():
    from vmlmf_amd import BeamControls, BeamGraph, beam_backtrack
    from vmlmf_amd.decoding import _KeptImages
    m = beam_model("plain").to(DEV)
    B, W, eos, steps = 3, 4, K.MODEL_EOS, 12
    prompt = _prompt(B, seed=13)
    kw = K.setting("n3_min6_seqs", "plain", B, W, 13)
    kw = dict(kw, banned_tokens=[17])
    base = m.beam_search(prompt, steps, beams=W, eos=eos, **kw)
    for other in (m.beam_search(prompt, steps, beams=W, eos=eos, **kw), m.beam_search(prompt, steps, beams=W, eos=eos, chunk=6, **kw),
                  m.beam_search(prompt, steps, beams=W, eos=eos, chunk=4, **kw)):
        assert torch.equal(base[0], other[0]) and torch.equal(base[1], other[1]) and torch.equal(base[2], other[2])
        for (h, c), (h2, c2) in zip(base[3], other[3]):
            assert torch.equal(h, h2) and torch.equal(c, c2)
    pen = m.beam_search(prompt, steps, beams=W, eos=eos, length_penalty=1.0, **kw)
    assert sorted(pen[1][0].tolist()) == sorted(base[1][0].tolist())
    # a BeamGraph of 6 steps replayed twice continues its own hypotheses: the 12 eager steps
    m.eval()
    with torch.no_grad(), _KeptImages(m):
        h, st = m.features(prompt, m.state_init(B))
        h = h[-1].repeat_interleave(W, 0)
        st = [tuple(t.repeat_interleave(W, 0) for t in s) for s in st]
    c = BeamControls(B, W, 97, DEV, prompt=prompt, capacity=prompt.shape[0] + steps, eos=eos, **kw)
    g = BeamGraph(m, h, st, 6, W, eos=eos, controls=c)
    first, second = g.replay(), g.replay()
    parents, toks = torch.cat([first[0], second[0]]), torch.cat([first[1], second[1]])
    assert torch.equal(beam_backtrack(parents, toks), base[0]) and torch.equal(g.cum, base[1]) and torch.equal(g.length, base[2])
    assert g.hist_len.view(B, W).tolist() == (prompt.shape[0] + base[2]).tolist() and c.overflow.tolist() == [0] * B
    for b in range(B):
        for w in range(W):
            L = int(base[2][b, w])
            assert g.hist[b * W + w, :prompt.shape[0] + L].tolist() == prompt[:, b].tolist() + base[0][:L, b, w].tolist()
