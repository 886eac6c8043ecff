"""Decoding under a token automaton on the GPU (libvmlmf_automaton.so, include/vmlmf_automaton.h; automaton= of Model.generate and
Model.beam_search).  A table only closes tokens, so every kernel test compares with a kernel the project already has, BIT FOR BIT:
vmlmf_automaton_choose with vmlmf_decode_choose under a logit_bias that holds -inf at what the row's state closes (K1 - K4),
vmlmf_automaton_beam_step with vmlmf_beamctl_step under the ban bitmap of what every beam's state closes and with vmlmf_beam_step under
a neutral table (B1 - B3); the model-level tests compare with banned_sequences (M1, M4), with the constraint itself and Model.score (M2)
and the graphed forms with the eager ones (M3, M4).  The cases and the numpy statement of the rule are automaton_cases.py's."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import automaton_cases as A
from abi_arena import FILLS, Arena, assert_same_bits, assert_written
from lm_util import DEV, LP_TOL, _prompt, _small, _snap

pytestmark = pytest.mark.gpu
I32 = torch.int32
EOS = A.EOS
CHOICE_NAMES = ["tokens", "logprob", "x_next", "kept"]
BEAM_NAMES = ["parent", "token", "total", "finished_out", "length_out", "x_next", "src_row"]
NEG_INF = float("-inf")


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ---- the two choice launches on given device buffers ----
def _choice_outputs(B, H, make):
    return dict(tokens=make((B,), torch.int64, "tokens"), logprob=make((B,), torch.float32, "logprob"),
                x_next=make((B, H), torch.float32, "x_next"), kept=make((B,), I32, "kept"))


def _fresh(shape, dtype, name):
    return torch.empty(shape, dtype=dtype, device=DEV)


def decode_choose(scores, bias, embed, mode, snap, step, lb, seen, fin, length, eos, min_length, theta, make=_fresh):
    """vmlmf_decode_choose on device tensors; seen / fin / length are moved on in place.  Returns the four outputs."""
    from vmlmf_amd import _decode
    tau, k, p = mode
    B, V = scores.shape
    H = embed.shape[1]
    out = _choice_outputs(B, H, make)
    c = _decode.Controls(theta, eos, min_length, 0, _p(lb), _p(seen), _p(fin), _p(length))
    _decode.LIBRARY.call(scores.device, "vmlmf_decode_choose", B, H, V, _p(scores), _p(bias), _p(embed), 0.0 if tau == 0 else 1.0 / tau, k, p,
                         None if tau == 0 else _p(snap), step, ctypes.byref(c), *(_p(out[n]) for n in CHOICE_NAMES))
    return out


def automaton_choose(scores, bias, embed, mode, snap, step, lb, seen, fin, length, eos, min_length, theta, nxt, row_state, dead, make=_fresh):
    """vmlmf_automaton_choose on device tensors; seen / fin / length / row_state / dead are moved on in place."""
    from vmlmf_amd import _automaton
    tau, k, p = mode
    B, V = scores.shape
    H = embed.shape[1]
    out = _choice_outputs(B, H, make)
    c = _automaton.Controls(theta, eos, min_length, 0, _p(lb), _p(seen), _p(fin), _p(length), _p(nxt), nxt.shape[0], 0, _p(row_state), _p(dead))
    _automaton.LIBRARY.call(scores.device, "vmlmf_automaton_choose", B, H, V, _p(scores), _p(bias), _p(embed), 0.0 if tau == 0 else 1.0 / tau, k,
                            p, None if tau == 0 else _p(snap), step, ctypes.byref(c), *(_p(out[n]) for n in CHOICE_NAMES))
    return out


def _yardstick_rows(case, mode, snap, nxt, state, rows=None):
    """Per row b: the B = 1 call of vmlmf_decode_choose at step' = step B + b under the case's bias with -inf at what the row's state
    closes.  Returns {b: (outputs, seen, finished, length)} on the CPU."""
    B, V = case["scores"].shape
    bias, embed = _t(case["bias"]), _t(case["embed"])
    got = {}
    for b in (range(B) if rows is None else rows):
        lb = case["logit_bias"].copy()
        lb[A.closes(nxt, state[b])] = -np.inf
        seen, fin, length = _t(case["seen"][b:b + 1]), _t(case["finished"][b:b + 1]), _t(case["length"][b:b + 1])
        out = decode_choose(_t(case["scores"][b:b + 1]), bias, embed, mode, snap, A.CHOICE_STEP * B + b, _t(lb), seen, fin, length, EOS,
                            A.MIN_LENGTH, A.THETA)
        got[b] = ({n: t.cpu() for n, t in out.items()}, seen.cpu(), fin.cpu(), length.cpu())
    return got


def _compare_rows(what, out, seen, fin, length, want):
    for b, (wout, wseen, wfin, wlen) in want.items():
        for n in CHOICE_NAMES:
            assert_same_bits(n, out[n][b:b + 1].cpu(), wout[n], f"{what}, row {b}, against vmlmf_decode_choose")
        assert torch.equal(seen[b:b + 1].cpu(), wseen) and torch.equal(fin[b:b + 1].cpu(), wfin) and torch.equal(length[b:b + 1].cpu(), wlen), (what, b)


# ---- K1: the choice against vmlmf_decode_choose, row by row ----
K1 = [(V, B, S, m) for V in A.CHOICE_V for B in A.CHOICE_B for S in A.CHOICE_S for m in A.CHOICE_MODES]


@pytest.mark.parametrize("V,B,S,mode", K1, ids=[f"V{v}-B{b}-S{s}-{m}" for v, b, s, m in K1])
def test_the_choice_is_decode_choose_under_the_equivalent_bias(V, B, S, mode):
    case = A.choice_case(B, S, V)
    mode = A.CHOICE_MODES[mode]
    snap = _snap()
    nxt, state = case["next"], case["state"]
    seen, fin, length = _t(case["seen"]), _t(case["finished"]), _t(case["length"])
    row_state, dead = _t(state), torch.zeros(B, dtype=I32, device=DEV)
    out = automaton_choose(_t(case["scores"]), _t(case["bias"]), _t(case["embed"]), mode, snap, A.CHOICE_STEP, _t(case["logit_bias"]), seen, fin,
                           length, EOS, A.MIN_LENGTH, A.THETA, _t(nxt), row_state, dead)
    torch.cuda.synchronize()
    _compare_rows("K1", out, seen, fin, length, _yardstick_rows(case, mode, snap, nxt, state))
    tok = out["tokens"].cpu().numpy()
    for b in range(B):
        if case["finished"][b]:
            assert tok[b] == EOS and row_state[b].item() == state[b]                    # a finished row: padding, the state stays
        else:
            assert nxt[state[b], tok[b]] >= 0 and tok[b] != 5                           # an open token, never the banned one
            assert not (tok[b] == EOS and case["length"][b] < A.MIN_LENGTH)
            assert row_state[b].item() == nxt[state[b], tok[b]]
    assert not dead.any()
    if mode[1]:
        assert (out["kept"].cpu().numpy()[case["finished"] == 0] <= mode[1]).all()


def test_top_k_reaching_into_closed_tokens_keeps_the_open_ones_only():
    """Fewer than k tokens are open: top-k's cut falls among the closed tokens, none of which is kept or chosen."""
    B, S, V = 3, 5, 97
    case = A.choice_case(B, S, V)
    nxt = np.full((S, V), -1, dtype=np.int32)
    opened = {1: [3, 40, 96], 3: [0, 9, 31, 32, 64], 0: [50]}
    for s, toks in opened.items():
        nxt[s, toks] = (s + 1) % S
    case = dict(case, finished=np.zeros(B, dtype=np.int32))
    state = case["state"]
    assert sorted(state.tolist()) == [0, 1, 3]
    mode, snap = A.CHOICE_MODES["k7p0.8"], _snap()
    mode = (mode[0], mode[1], 1.0)                                                       # top_k 7 alone
    seen, fin, length = _t(case["seen"]), _t(case["finished"]), _t(case["length"])
    row_state, dead = _t(state), torch.zeros(B, dtype=I32, device=DEV)
    out = automaton_choose(_t(case["scores"]), _t(case["bias"]), _t(case["embed"]), mode, snap, A.CHOICE_STEP, _t(case["logit_bias"]), seen, fin,
                           length, EOS, A.MIN_LENGTH, A.THETA, _t(nxt), row_state, dead)
    torch.cuda.synchronize()
    _compare_rows("fewer than k open", out, seen, fin, length, _yardstick_rows(case, mode, snap, nxt, state))
    for b in range(B):
        assert out["tokens"][b].item() in opened[state[b]] and out["kept"][b].item() == len(opened[state[b]])
        assert row_state[b].item() == (state[b] + 1) % S
    assert not dead.any()


# ---- K2: a neutral table is vmlmf_decode_choose on the whole batch ----
@pytest.mark.parametrize("V", A.CHOICE_V)
@pytest.mark.parametrize("mode", list(A.CHOICE_MODES))
def test_a_neutral_table_is_decode_choose_to_the_bit(V, mode):
    B = 3
    case = A.choice_case(B, 1, V)
    mode, snap = A.CHOICE_MODES[mode], _snap()
    args = lambda: (_t(case["scores"]), _t(case["bias"]), _t(case["embed"]), mode, snap, A.CHOICE_STEP, _t(case["logit_bias"]))
    s1, f1, l1 = _t(case["seen"]), _t(case["finished"]), _t(case["length"])
    want = decode_choose(*args(), s1, f1, l1, EOS, A.MIN_LENGTH, A.THETA)
    s2, f2, l2 = _t(case["seen"]), _t(case["finished"]), _t(case["length"])
    row_state, dead = torch.zeros(B, dtype=I32, device=DEV), torch.zeros(B, dtype=I32, device=DEV)
    out = automaton_choose(*args(), s2, f2, l2, EOS, A.MIN_LENGTH, A.THETA, _t(A.neutral_table(V)), row_state, dead)
    torch.cuda.synchronize()
    for n in CHOICE_NAMES:
        assert_same_bits(n, out[n].cpu(), want[n].cpu(), "between vmlmf_decode_choose and vmlmf_automaton_choose under a neutral table")
    assert torch.equal(s1, s2) and torch.equal(f1, f2) and torch.equal(l1, l2)
    assert not row_state.any() and not dead.any()


# ---- K3 / K4: dead and invalid states, on poisoned, exactly sized buffers ----
def _arena_choice(fill, case, nxt, state, mode, snap):
    """vmlmf_automaton_choose with every buffer an exactly sized view of a poisoned arena (the table exactly S V words)."""
    B, V = case["scores"].shape
    arena = Arena(DEV, fill)
    make = lambda shape, dtype, name: arena.buf(shape, dtype, name=name)
    buf = lambda name, x, dtype: arena.buf(x.shape, dtype, init=x, name=name)
    scores, bias, embed = buf("scores", case["scores"], torch.float32), buf("bias", case["bias"], torch.float32), buf("embed", case["embed"], torch.float32)
    lb = buf("logit_bias", case["logit_bias"], torch.float32)
    seen, fin, length = buf("seen", case["seen"], torch.uint8), buf("finished", case["finished"], I32), buf("length", case["length"], I32)
    table, row_state, dead = buf("next", nxt, I32), buf("row_state", state, I32), arena.buf(B, I32, init=0, name="dead")
    snap_a = arena.buf(2, torch.int64, init=snap, name="state")
    out = automaton_choose(scores, bias, embed, mode, snap_a, A.CHOICE_STEP, lb, seen, fin, length, EOS, A.MIN_LENGTH, A.THETA, table, row_state,
                           dead, make=make)
    torch.cuda.synchronize()
    arena.check_guards()
    return arena, out, seen, fin, length, row_state, dead


@pytest.mark.parametrize("mode", list(A.CHOICE_MODES))
def test_dead_and_invalid_states_are_defined_and_stay_inside_their_buffers(mode):
    """Rows 0, 2 and 4 sit in state -1, in state S and in a state whose table row is all -1: `dead` is set, the state stays, the other
    outputs are vmlmf_decode_choose's under an all -inf bias; rows 1 and 3 between them are live and unaffected.  (The defined behaviour
    of such states: no address is formed from one.)"""
    S, V, B = 4, 97, 5
    base = A.choice_case(3, 5, V)
    rng = np.random.Generator(np.random.PCG64(3))
    case = dict(base, scores=(3 * rng.standard_normal((B, V))).astype(np.float32), seen=(rng.random((B, V)) < 0.3).astype(np.uint8),
                finished=np.zeros(B, dtype=np.int32), length=np.array([2, 9, 6, 1, 7], dtype=np.int32))
    nxt = A.random_table(S, V, 17, keep_open=(EOS,))
    nxt[2] = -1
    state = np.array([-1, 1, S, 3, 2], dtype=np.int32)
    mode, snap = A.CHOICE_MODES[mode], _snap()
    want = _yardstick_rows(case, mode, snap, nxt, state)
    results = []
    for fill in FILLS:
        arena, out, seen, fin, length, row_state, dead = _arena_choice(fill, case, nxt, state, mode, snap)
        for n in ("tokens", "x_next", "kept"):
            assert_written(arena, n, out[n])
        _compare_rows(f"K3 under fill {fill:#x}", out, seen, fin, length, want)
        assert dead.tolist() == [1, 0, 1, 0, 1]
        tok = out["tokens"].cpu().numpy()
        assert row_state.tolist() == [-1, nxt[1, tok[1]], S, nxt[3, tok[3]], 2]
        assert torch.isnan(out["logprob"][[0, 2, 4]]).all() and (out["kept"][[0, 2, 4]] == 0).all() and (out["tokens"][[0, 2, 4]] == 0).all()
        results.append({n: t.cpu() for n, t in out.items()})
    for other in results[1:]:
        for n in CHOICE_NAMES:
            assert_same_bits(n, results[0][n], other[n], "between two fills of the memory around the buffers")


# ---- the beam launches ----
def _beam_outputs(B, W, H, make):
    return dict(parent=make((B, W), I32, "parent"), token=make((B, W), torch.int64, "token"), total=make((B, W), torch.float32, "total"),
                finished_out=make((B, W), I32, "finished_out"), length_out=make((B, W), I32, "length_out"),
                x_next=make((B * W, H), torch.float32, "x_next"), src_row=make((B * W,), I32, "src_row"))


def _words(mask):
    return None if mask is None else _t(A.K.pack(mask))


def automaton_beam_step(d, eos, min_length, closed_words, nxt, state, make=_fresh, buffers=None):
    """vmlmf_automaton_beam_step on the device tensors of d (scores, bias, embed, cum, finished, length).  Returns (outputs, beam_state_out)."""
    from vmlmf_amd import _automaton, _beam
    B, W = d["cum"].shape
    V, H = d["scores"].shape[1], d["embed"].shape[1]
    ticket, ws = buffers if buffers is not None else _beam.new_step_buffers(d["scores"].device, B, W, V)
    out = _beam_outputs(B, W, H, make)
    state_out = make((B * W,), I32, "beam_state_out")
    table = _automaton.Table(nxt.data_ptr(), nxt.shape[0], 0)
    _automaton.LIBRARY.call(d["scores"].device, "vmlmf_automaton_beam_step", B, W, H, V, _p(d["scores"]), _p(d["bias"]), _p(d["cum"]),
                            _p(d["finished"]), _p(d["length"]), eos, _p(d["embed"]), min_length, _p(closed_words), ctypes.byref(table), _p(state),
                            _p(state_out), *(_p(out[n]) for n in BEAM_NAMES[:5]), _p(out["x_next"]), _p(out["src_row"]), _p(ticket), _p(ws),
                            ws.numel() * 8)
    torch.cuda.synchronize()
    assert int(ticket.abs().sum()) == 0                                  # the ticket words are zero after the launch
    return out, state_out


def beamctl_step(d, eos, min_length, closed_words, bans_words):
    """vmlmf_beamctl_step without a history: the yardstick."""
    from vmlmf_amd import _beam, _beamctl
    B, W = d["cum"].shape
    V, H = d["scores"].shape[1], d["embed"].shape[1]
    ticket, ws = _beam.new_step_buffers(d["scores"].device, B, W, V)
    out = _beam_outputs(B, W, H, _fresh)
    c = _beamctl.Controls(min_length, 1, _p(closed_words), _p(bans_words), None, None, None, None, None)
    _beamctl.LIBRARY.call(d["scores"].device, "vmlmf_beamctl_step", B, W, H, V, _p(d["scores"]), _p(d["bias"]), _p(d["cum"]), _p(d["finished"]),
                          _p(d["length"]), eos, _p(d["embed"]), ctypes.byref(c), *(_p(out[n]) for n in BEAM_NAMES[:5]), _p(out["x_next"]),
                          _p(out["src_row"]), _p(ticket), _p(ws), ws.numel() * 8)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _beam_device(B, W, V, first_step):
    case = A.beam_case(B, W, V, first_step)
    return case, {n: _t(case[n]) for n in ("scores", "bias", "embed", "cum", "finished", "length")}


def _compare_beams(what, out, want):
    for n in BEAM_NAMES:
        assert out[n].dtype == want[n].dtype and out[n].shape == want[n].shape
        assert_same_bits(n, out[n].cpu(), want[n].cpu(), what)


B1 = [(B, W, V, first) for (B, W) in A.BEAM_SHAPES for V in A.BEAM_V for first in (False, True)]


@pytest.mark.parametrize("B,W,V,first", B1, ids=[f"{b}x{w}-V{v}-{'first' if f else 'mid'}" for b, w, v, f in B1])
def test_the_beam_step_is_beamctl_step_under_the_equivalent_bans(B, W, V, first):
    case, d = _beam_device(B, W, V, first)
    nxt, state = case["next"], case["state"]
    closed = _words(case["closed"])
    out, state_out = automaton_beam_step(d, EOS, A.BEAM_MIN_LENGTH, closed, _t(nxt), _t(state))
    want = beamctl_step(d, EOS, A.BEAM_MIN_LENGTH, closed, _words(A.beam_bans(nxt, state)))
    _compare_beams("between vmlmf_beamctl_step under the states' ban bitmaps and vmlmf_automaton_beam_step", out, want)
    parent, token, total = out["parent"].cpu().numpy(), out["token"].cpu().numpy(), out["total"].cpu().numpy()
    assert not np.isnan(total).any()
    assert np.array_equal(state_out.cpu().numpy(), A.survivor_states(nxt, state, parent, token, total, case["finished"]))
    fin_parent = np.take_along_axis(case["finished"], parent, 1).astype(bool)
    assert (state_out.cpu().numpy() >= 0).all()
    live = ~fin_parent
    assert not case["closed"][token[live]].any()


# ---- B2: a neutral table is vmlmf_beam_step ----
B2 = [(B, W, V) for (B, W) in A.BEAM_SHAPES for V in A.BEAM_V]


@pytest.mark.parametrize("B,W,V", B2, ids=[f"{b}x{w}-V{v}" for b, w, v in B2])
def test_a_neutral_table_is_the_plain_beam_step_to_the_bit(B, W, V):
    from vmlmf_amd import _beam
    case, d = _beam_device(B, W, V, False)
    plain = _beam.beam_select(d["scores"], d["bias"], d["cum"], d["finished"], d["length"], EOS, d["embed"])
    out, state_out = automaton_beam_step(d, EOS, 0, None, _t(A.neutral_table(V)), torch.zeros(B * W, dtype=I32, device=DEV))
    _compare_beams("between vmlmf_beam_step and vmlmf_automaton_beam_step under a neutral table", out, dict(zip(BEAM_NAMES, plain)))
    assert not state_out.any()


# ---- B3: dead beams and rows that run short of candidates; K4 for the beam step: poisoned, exactly sized buffers ----
@pytest.mark.parametrize("V", [97, 12289])
def test_a_dead_beam_offers_nothing_and_surplus_slots_get_no_state(V):
    """Batch row 0: beam 0 in a state with two open tokens, beams 1 and 2 dead (state -1, state S), beam 3 finished: three candidates
    for four slots - the last gets a NaN total and state -1, the finished parent's survivor copies its state.  Batch row 1: one dead
    beam (a table row of -1) among live ones."""
    B, W, S = 2, 4, A.BEAM_S
    case, d = _beam_device(B, W, V, False)
    nxt = case["next"].copy()
    nxt[4] = -1
    nxt[3] = -1
    nxt[3, [11, 60]] = [2, 0]
    state = np.array([3, -1, S, 1, 0, 4, 2, 1], dtype=np.int32)
    assert case["finished"].tolist() == [[0, 0, 0, 1]] * 2
    bans = A.beam_bans(nxt, state)
    want = beamctl_step(d, EOS, 0, None, _words(bans))
    results = []
    for fill in FILLS:
        arena = Arena(DEV, fill)
        make = lambda shape, dtype, name: arena.buf(shape, dtype, name=name)
        da = {n: arena.buf(t.shape, t.dtype, init=t, name=n) for n, t in d.items()}
        table, st = arena.buf(nxt.shape, I32, init=nxt, name="next"), arena.buf(state.shape, I32, init=state, name="beam_state")
        from vmlmf_amd import _automaton
        nbytes = _automaton.lib().vmlmf_automaton_workspace_bytes(B, W, V)
        buffers = (arena.buf(B, I32, init=0, name="ticket"), arena.buf(nbytes // 8, torch.int64, name="workspace"))
        out, state_out = automaton_beam_step(da, EOS, 0, None, table, st, make=make, buffers=buffers)
        arena.check_guards()
        for n in ("parent", "token", "finished_out", "length_out", "src_row", "x_next"):
            assert_written(arena, n, out[n])
        _compare_beams(f"B3 under fill {fill:#x}", out, want)
        parent, token, total = out["parent"].cpu().numpy(), out["token"].cpu().numpy(), out["total"].cpu().numpy()
        assert np.isnan(total[0]).tolist() == [False, False, False, True] and not np.isnan(total[1]).any()
        assert sorted(zip(parent[0, :3].tolist(), token[0, :3].tolist())) == [(0, 11), (0, 60), (3, EOS)]
        assert (parent[1] != 1).all()                                                    # the dead beam of row 1 has no survivor
        so = state_out.cpu().numpy()
        assert np.array_equal(so, A.survivor_states(nxt, state, parent, token, total, case["finished"])) and so[3] == -1 and (so[4:] >= 0).all()
        results.append(dict(out, beam_state_out=state_out))
    for other in results[1:]:
        for n in BEAM_NAMES + ["beam_state_out"]:
            assert_same_bits(n, results[0][n].cpu(), other[n].cpu(), "between two fills of the memory around the buffers")


# ---- the model level ----
@pytest.fixture(scope="module", autouse=True)
def unconstrained_calls_before_and_after():
    """M5: an unconstrained generate and beam_search before any test of this module has run and after all of them have: the same bits."""
    m = _small("plain").eval()
    prompt = _prompt(3, seed=13)
    run = lambda: (m.generate(prompt, 12, temperature=0.0)[:2], m.generate(prompt, 12, temperature=0.9, seed=5, top_k=9)[:2],
                   m.beam_search(prompt, 12, 4, None, 3)[:3], m.beam_search(prompt, 12, 4, None, 3, chunk=6)[:3])
    before = run()
    yield
    for was, now in zip(before, run()):
        assert all(torch.equal(a, b) for a, b in zip(was, now))


@functools.lru_cache(maxsize=None)
def _avoid_setting():
    """The model, a prompt and banned sequences taken from the unconstrained greedy continuation: a bigram of row 0's and a trigram of
    row 2's tokens and, where row 1 emits one the prompt does not hold, a single token of row 1's - so the ban changes tokens -, none of
    them in the prompt (the first prompt seed of twenty for which that holds)."""
    m = _small("plain").eval()
    for seed in range(21, 41):
        prompt = _prompt(3, seed=seed)
        free = m.generate(prompt, 24, temperature=0.0)[0].cpu()
        pr = prompt.cpu().t().tolist()
        seqs = [free[3:5, 0].tolist(), free[6:9, 2].tolist()]
        single = [t for t in free[2:, 1].tolist() if t not in (3, 11) and not any(t in row for row in pr)]
        seqs += [single[:1]] if single else []
        if not any(A.contains_any(row, seqs) for row in pr):
            break
    assert not any(A.contains_any(row, seqs) for row in pr)
    return m, prompt, free, seqs


@pytest.mark.parametrize("kw", [dict(temperature=0.0), dict(temperature=1.0, top_k=12, seed=7)], ids=["greedy", "k12"])
def test_generate_under_avoiding_is_generate_under_banned_sequences(kw):
    from vmlmf_amd import TokenAutomaton
    m, prompt, free, seqs = _avoid_setting()
    a = TokenAutomaton.avoiding(97, seqs)
    want = m.generate(prompt, 24, banned_sequences=seqs, **kw)
    got = m.generate(prompt, 24, automaton=a, automaton_state=a.advance(prompt), **kw)
    assert torch.equal(got[0], want[0]), "tokens"
    assert_same_bits("logprobs", got[1].cpu(), want[1].cpu(), "between banned_sequences and the automaton that avoids them")
    for b in range(3):
        assert not A.contains_any(got[0][:, b].tolist(), seqs)
    if kw["temperature"] == 0.0:
        assert not torch.equal(got[0].cpu(), free)                                       # the ban changes the continuation
    assert all(torch.equal(x, y) for s, u in zip(got[2], want[2]) for x, y in zip(s, u))


@pytest.mark.parametrize("kind", ["forced", "one_of", "template"])
def test_sampling_at_a_high_temperature_satisfies_the_constraint_exactly(kind):
    from vmlmf_amd import TokenAutomaton as T
    m = _small("plain").eval()
    B, V, eos, steps = 4, 97, 3, 10
    prompt = _prompt(B, seed=4)
    free = {"forced": T.forced(V, [10, 20, 30, 40]), "one_of": T.one_of(V, [[5, 6, 7], [5, 8], [9, 10, 11, 12, 13]]),
            "template": T.template(V, [[1, 2, 4], 50, range(60, 70)])}[kind]
    stop = {"forced": T.forced(V, [10, 20, 30, 40], eos), "one_of": T.one_of(V, [[5, 6, 7], [5, 8], [9, 10, 11, 12, 13]], eos),
            "template": T.template(V, [[1, 2, 4], 50, range(60, 70)], eos)}[kind]
    tokens, logprobs, _ = m.generate(prompt, steps, temperature=1.5, seed=3, automaton=free)
    for b in range(B):
        assert free.accepts(tokens[:, b])
    if kind == "forced":
        assert tokens[:4].cpu().tolist() == [[10] * B, [20] * B, [30] * B, [40] * B]
    tokens, logprobs, lengths, _ = m.generate(prompt, steps, temperature=1.5, seed=3, automaton=stop, eos=eos, return_lengths=True)
    for b in range(B):
        row, n = tokens[:, b].tolist(), int(lengths[b])
        assert stop.accepts(row, eos=eos) and row[n - 1] == eos and eos not in row[:n - 1] and all(t == eos for t in row[n:])
        body = row[:n - 1]
        if kind == "forced":
            assert body == [10, 20, 30, 40]
        elif kind == "one_of":
            assert body in ([5, 6, 7], [5, 8], [9, 10, 11, 12, 13])
        else:
            assert len(body) == 3 and body[0] in (1, 2, 4) and body[1] == 50 and 60 <= body[2] < 70
        assert (logprobs[n:, b] == 0).all()
    # the log-probabilities are the unprocessed log-softmax of the emitted tokens: Model.score's
    scored = m.score(torch.cat([prompt, tokens]))[0][prompt.shape[0] - 1:]
    live = torch.arange(steps, device=DEV)[:, None] < lengths[None, :]
    assert ((scored - logprobs).abs()[live]).max().item() <= 2 * LP_TOL          # test_gpu_score.py's bound for generate against score


def test_chunked_and_graphed_decoding_continue_the_states():
    from vmlmf_amd import AutomatonControls, DecodeGraph, TokenAutomaton
    m, prompt, _, seqs = _avoid_setting()
    B, V, eos = 3, 97, 11
    a = TokenAutomaton.avoiding(V, seqs)
    st = a.advance(prompt)
    ctl = dict(eos=eos, min_length=2, repetition_penalty=1.3, banned_tokens=[5, 6])
    e = m.generate(prompt, 12, temperature=0.0, return_lengths=True, automaton=a, automaton_state=st, **ctl)
    c = m.generate(prompt, 12, temperature=0.0, chunk=4, return_lengths=True, automaton=a, automaton_state=st, **ctl)
    assert all(torch.equal(x, y) for x, y in zip(e[:3], c[:3]))
    assert all(torch.equal(x, y) for s, u in zip(e[3], c[3]) for x, y in zip(s, u))
    kw = dict(temperature=1.0, top_k=10, top_p=0.9, automaton=a, automaton_state=st)
    s8 = m.generate(prompt, 8, seed=11, **kw)
    g8 = m.generate(prompt, 8, seed=11, chunk=8, **kw)
    assert torch.equal(g8[0], s8[0]) and torch.equal(g8[1], s8[1])
    # one DecodeGraph replayed twice is one eager run of twice the steps (greedy: no generator between them)
    want = m.generate(prompt, 16, temperature=0.0, automaton=a, automaton_state=st)
    with torch.no_grad():
        h, states = m.features(prompt, m.state_init(B))
    controls = AutomatonControls(B, V, DEV, a, st, prompt=prompt)
    g = DecodeGraph(m, h[-1], states, 8, temperature=0.0, controls=controls)
    assert torch.equal(controls.row_state, st.to(DEV)) and not controls.length.any()            # the warm-up ran on a clone
    t1, l1 = g.replay()
    mid = controls.row_state.clone()
    t2, l2 = g.replay()
    assert torch.equal(torch.cat([t1, t2]), want[0]) and torch.equal(torch.cat([l1, l2]), want[1])
    assert torch.equal(mid, a.advance(t1, st).to(DEV)) and torch.equal(controls.row_state, a.advance(torch.cat([t1, t2]), st).to(DEV))
    assert not controls.dead.any() and (controls.length == 16).all()


def test_beam_search_under_avoiding_is_beam_search_under_banned_sequences():
    from vmlmf_amd import BeamGraph, AutomatonBeamControls, TokenAutomaton
    m, prompt, _, seqs = _avoid_setting()
    a = TokenAutomaton.avoiding(97, seqs)
    st = a.advance(prompt)
    kw = dict(beams=4, eos=3, min_length=3)
    want = m.beam_search(prompt, 12, banned_sequences=seqs, **kw)
    got = m.beam_search(prompt, 12, automaton=a, automaton_state=st, **kw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    assert_same_bits("scores", got[1].cpu(), want[1].cpu(), "between banned_sequences and the automaton that avoids them")
    # chunk= against eager, bit for bit
    ch = m.beam_search(prompt, 12, automaton=a, automaton_state=st, chunk=4, **kw)
    assert all(torch.equal(x, y) for x, y in zip(got[:3], ch[:3]))
    # beams=1 is greedy generate under the same automaton, token for token
    one = m.beam_search(prompt, 12, beams=1, automaton=a, automaton_state=st)
    greedy = m.generate(prompt, 12, temperature=0.0, automaton=a, automaton_state=st)
    assert torch.equal(one[0][:, :, 0], greedy[0])
    # a BeamGraph replayed twice against one eager run of twice the steps
    from vmlmf_amd.decoding import beam_backtrack
    B, W = 3, 4
    with torch.no_grad():
        h, states = m.features(prompt, m.state_init(B))
    controls = AutomatonBeamControls(B, W, 97, DEV, a, st, eos=3, min_length=3)
    hb = h[-1].repeat_interleave(W, 0)
    sb = [tuple(t.repeat_interleave(W, t.dim() - 2) for t in s) for s in states]
    g = BeamGraph(m, hb, sb, 6, W, 3, controls=controls)
    p1, t1 = g.replay()
    p2, t2 = g.replay()
    assert torch.equal(beam_backtrack(torch.cat([p1, p2]), torch.cat([t1, t2])), got[0]) and torch.equal(g.cum, got[1])
    hyp, fin, state = got[0].cpu().numpy(), g.finished.cpu().numpy(), g.beam_state.view(B, W).cpu().numpy()
    for b in range(B):          # the carried states are the hypotheses' (a finished beam's stopped moving at its eos)
        for w in range(W):
            if not fin[b, w]:
                assert state[b, w] == A.walk(a.host(), int(st[b]), hyp[:, b, w])


def test_a_constraint_with_fewer_sequences_than_beams_leaves_the_surplus_at_minus_infinity():
    from vmlmf_amd import TokenAutomaton
    m = _small("plain").eval()
    prompt = _prompt(2, seed=9)
    eos, seqs = 3, [[5, 6, 7], [5, 8], [9, 10, 11, 12]]
    a = TokenAutomaton.one_of(97, seqs, eos)
    tokens, scores, lengths, _ = m.beam_search(prompt, 8, beams=5, eos=eos, automaton=a)
    for b in range(2):
        real = [w for w in range(5) if scores[b, w] > NEG_INF]
        hyps = [A.K.until_eos(tokens[:, b, w].tolist(), eos) for w in real]
        assert sorted(hyps) == sorted(s + [eos] for s in seqs), (b, hyps)
        assert all(lengths[b, w].item() == len(h) for w, h in zip(real, hyps))
        assert (scores[b, len(real):] == NEG_INF).all() and real == list(range(len(seqs)))
        assert (scores[b, :2] >= scores[b, 1:3]).all()
    # every hypothesis' score is the sum of Model.score's log-probabilities of its tokens
    for b in range(2):
        for w in range(3):
            n = int(lengths[b, w])
            lp = m.score(torch.cat([prompt[:, b:b + 1], tokens[:n, b:b + 1, w]]))[0][prompt.shape[0] - 1:]
            assert abs(lp.sum().item() - scores[b, w].item()) <= 2 * n * LP_TOL
