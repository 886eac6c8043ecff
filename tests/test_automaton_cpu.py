"""Decoding under a token automaton (vmlmf_amd.TokenAutomaton, automaton= of Model.generate and Model.beam_search;
libvmlmf_automaton.so, include/vmlmf_automaton.h): what can be checked without a GPU - every constructor's table by brute force, the
rule of `avoiding` against history_cases.ban_set, advance, every refusal of the Python layer and of the C ABI, the reachability check,
what is the library's own of its build (the kernels are instantiated, not copied).  (Its exports, build rule and lazy load: its row of
test_side_libraries_cpu.py; the signatures: test_generate_cpu.py.)"""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import automaton_cases as A
import history_cases as HC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vmlmf_amd", "csrc")
V = 8


def TA():
    from vmlmf_amd import TokenAutomaton
    return TokenAutomaton


# ---- the constructors, by brute force ----
@pytest.mark.parametrize("then", ["free", 7])
def test_forced_and_template_emit_exactly_their_slots(then):
    slots = [[1], [2, 3, 5], [4]]
    for a, want_slots in ((TA().forced(V, [1, 3, 4], then), [[1], [3], [4]]), (TA().template(V, [1, (2, 3, 5), [4]], then), slots)):
        nx = a.host()
        assert a.start == 0 and a.V == V and a.next.dtype == torch.int32 and a.next.is_contiguous()
        tail = [range(V)] * 2 if then == "free" else [[7]] * 2
        for n in range(1, 6):
            want = set(itertools.product(*(list(map(list, want_slots)) + tail)[:n]))
            assert A.language(nx, 0, V, n) == want, (then, n)
    assert TA().forced(V, [], "free").host().tolist() == [[0] * V]          # nothing forced: everything, for ever


@pytest.mark.parametrize("then", ["free", 7])
def test_one_of_is_the_trie_of_its_sequences(then):
    seqs = [[1, 2], [1, 3, 4], [5], [1, 2, 6]]              # [1, 2] is a prefix of [1, 2, 6]
    a = TA().one_of(V, seqs, then)
    nx = a.host()
    for n in range(1, 6):
        want = set()
        for s in seqs:
            if then == "free":
                want |= {tuple(s[:n])} if n <= len(s) else {tuple(s) + rest for rest in itertools.product(range(V), repeat=n - len(s))}
            else:
                want.add(tuple((s + [7] * n)[:n]))
        assert A.language(nx, 0, V, n) == want, (then, n)
    if then == 7:       # a state is accepting iff it offers eos: exactly behind a whole sequence
        for s in seqs:
            for k in range(len(s) + 1):
                st = A.walk(nx, 0, s[:k])
                assert (nx[st, 7] >= 0) == (s[:k] in seqs), (s, k)
    assert a.accepts([1, 3, 4]) and a.accepts(torch.tensor([5])) and not a.accepts([1, 4]) and not a.accepts([9])
    assert a.open_tokens(0) == [1, 5] and a.open_tokens(-1) == [] and a.open_tokens(a.S) == []
    e = TA().one_of(V, seqs, 7)
    assert e.accepts([1, 2, 7, 0, 0], eos=7) and not e.accepts([1, 2, 7, 0, 0]) and not e.accepts([1, 7], eos=7)


@pytest.mark.parametrize("seqs", A.AVOID_SETS, ids=lambda s: "-".join("".join(map(str, q)) for q in s))
def test_avoiding_closes_what_banned_sequences_closes(seqs):
    a = TA().avoiding(A.AVOID_V, seqs)
    nx = a.host()
    proper = {tuple(s[:k]) for s in seqs for k in range(len(s))}
    for h in A.avoid_histories(seqs, 200, seed=len(seqs) + len(seqs[0])):
        st = A.walk(nx, a.start, h)
        assert st is not None, h                                             # a history that holds no sequence is never refused
        assert np.array_equal(A.closes(nx, st), HC.ban_set(h, A.AVOID_V, 0, seqs)), (h, st)
    # a state is the longest suffix of the history that is a proper prefix of a sequence: as many states as such prefixes can be reached
    reach = {a.start}
    for h in itertools.product(range(A.AVOID_V), repeat=4):
        for k in range(5):
            st = A.walk(nx, a.start, h[:k])
            if st is not None:
                reach.add(st)
    ok = {p for p in proper if not A.contains_any(list(p), seqs)}
    assert len(reach) == a.S == len(ok)
    # ... and brute force: the sequences of 4 tokens it emits are those that hold none of the banned ones
    assert A.language(nx, a.start, A.AVOID_V, 4) == {h for h in itertools.product(range(A.AVOID_V), repeat=4) if not A.contains_any(list(h), seqs)}


def test_the_constructors_refuse():
    T = TA()
    for call, words in ((lambda: T.forced(V, [8]), "not a token"), (lambda: T.forced(V, [1], then="stop"), "then must be"),
                        (lambda: T.forced(V, [1], then=9), "not a token"), (lambda: T.one_of(V, []), "at least one"),
                        (lambda: T.one_of(V, [[1], []]), "none of them empty"), (lambda: T.template(V, [[]]), "allows no token"),
                        (lambda: T.avoiding(V, [[]]), "empty"), (lambda: T.avoiding(V, [[1, -1]]), "not a token"),
                        (lambda: T(torch.zeros(3, dtype=torch.int32)), r"\(S, V\)"), (lambda: T(torch.zeros((2, 3))), r"\(S, V\)"),
                        (lambda: T(torch.full((2, 3), 2)), "outside"), (lambda: T(torch.zeros((2, 3), dtype=torch.int32), start=2), "start"),
                        (lambda: T(torch.zeros((2, 3), dtype=torch.int32), start=-1), "start")):
        with pytest.raises(ValueError, match=words):
            call()
    a = T(np.array([[1, -1], [-5, 0]]), start=1)                             # any integer table; negative words are closed
    assert (a.S, a.V, a.start) == (2, 2, 1) and a.next.dtype == torch.int32 and a.open_tokens(1) == [1] and a.to("cpu") is a


def test_advance_runs_rows_through_the_table_and_refuses_a_closed_transition():
    a = TA().one_of(V, [[1, 2, 3], [4, 5]], 7)
    nx = a.host()
    toks = torch.tensor([[1, 4], [2, 5]])
    st = a.advance(toks)
    assert st.dtype == torch.int32 and st.tolist() == [A.walk(nx, 0, [1, 2]), A.walk(nx, 0, [4, 5])]
    assert a.advance(torch.tensor([[3, 7]]), st).tolist() == [A.walk(nx, 0, [1, 2, 3]), A.walk(nx, 0, [4, 5, 7])]
    assert a.advance(torch.zeros((0, 3), dtype=torch.int64)).tolist() == [0, 0, 0]
    for bad, state in ((torch.tensor([[1, 4], [5, 5]]), None), (torch.tensor([[1, 8]]), None), (toks, torch.tensor([0, a.S])),
                       (toks, torch.tensor([-1, 0]))):
        with pytest.raises(ValueError, match="closed transition"):
            a.advance(bad, state)
    with pytest.raises(ValueError, match="int64"):
        a.advance(torch.zeros((2, 2), dtype=torch.int32))
    with pytest.raises(ValueError, match="must hold 2 states"):
        a.advance(toks, torch.tensor([0]))


# ---- the Python refusals ----
def _model(vocab=V):
    from vmlmf_amd import Model
    return Model(vocab, 8, 1, 0.0, 0.1, w_rank=4, u_ranks=[4], lstm_type="vmlmf")


def test_generate_and_beam_search_refuse_before_any_device_work():
    T = TA()
    m, tok = _model(), torch.zeros((3, 2), dtype=torch.int64)
    free = T.forced(V, [1, 2])
    cases = [
        (dict(automaton="x"), "must be a vmlmf_amd.TokenAutomaton"),
        (dict(automaton=T.forced(V + 1, [1])), "the vocabulary has 8"),
        (dict(automaton_state=torch.zeros(2, dtype=torch.int32)), "automaton_state needs automaton"),
        (dict(automaton=free, automaton_state=torch.zeros(3, dtype=torch.int32)), r"\(2,\) int32"),
        (dict(automaton=free, automaton_state=torch.zeros(2, dtype=torch.int64)), r"\(2,\) int32"),
        (dict(automaton=free, automaton_state=torch.tensor([0, 3], dtype=torch.int32)), "outside"),
        (dict(automaton=free, automaton_state=torch.tensor([-1, 0], dtype=torch.int32)), "outside"),
        (dict(automaton=free, banned_tokens=[2]), "state 1 is reachable and has no open token"),
    ]
    for kw, words in cases:
        for call in (m.generate, m.beam_search):
            with pytest.raises(ValueError, match=words):
                call(tok, 4, **kw)
    lb = torch.zeros(V)
    lb[1] = float("-inf")
    gen = [
        (dict(automaton=free, logit_bias=lb), "state 0 is reachable and has no open token"),
        (dict(automaton=T.forced(V, [1], 7), eos=7, min_length=3), "no open token besides eos, which min_length holds back"),
        (dict(automaton=free, no_repeat_ngram_size=2), "together with the history controls"),
        (dict(automaton=free, banned_sequences=[[1]]), "together with the history controls"),
        (dict(automaton=free, frequency_penalty=0.5), "together with the history controls"),
        (dict(automaton=free, presence_penalty=0.5), "together with the history controls"),
        (dict(automaton=free, min_p=0.1), "together with the truncation samplers"),
        (dict(automaton=free, eta_cutoff=0.1, temperature=0.0), "together with the truncation samplers"),
    ]
    for kw, words in gen:
        with pytest.raises(ValueError, match=words):
            m.generate(tok, 4, **kw)
    beam = [
        (dict(automaton=free, no_repeat_ngram_size=2), "together with no_repeat_ngram_size / banned_sequences"),
        (dict(automaton=free, banned_sequences=[[1]]), "together with no_repeat_ngram_size / banned_sequences"),
        (dict(automaton=T.forced(V, [1], 7), eos=7, min_length=3), "besides eos"),
        (dict(automaton=free, eos=7, banned_tokens=[7]), "among banned_tokens"),
    ]
    for kw, words in beam:
        with pytest.raises(ValueError, match=words):
            m.beam_search(tok, 4, **kw)
    # what passes the checks reaches the refusal of CPU tensors
    for call, kw in ((m.generate, dict(automaton=free)), (m.beam_search, dict(automaton=free, beams=2)),
                     (m.generate, dict(automaton=T.forced(V, [1], 7), eos=7, automaton_state=torch.tensor([1, 0], dtype=torch.int32)))):
        with pytest.raises(RuntimeError, match="cuda"):
            call(tok, 4, **kw)


def test_a_dead_end_is_refused_only_where_it_can_be_reached():
    from vmlmf_amd import AutomatonBeamControls, AutomatonControls
    nx = torch.tensor([[1, -1, -1], [1, 0, -1], [-1, -1, -1], [2, 2, 2]], dtype=torch.int32)        # state 2 is a dead end, from 3 only
    a = TA()(nx)
    m, tok = _model(3), torch.zeros((2, 2), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="cuda"):
        m.generate(tok, 4, automaton=a)                                      # from 0: states 0 and 1, the dead end is not reachable
    st = torch.tensor([0, 3], dtype=torch.int32)
    for call in (lambda: m.generate(tok, 4, automaton=a, automaton_state=st), lambda: m.beam_search(tok, 4, beams=2, automaton=a, automaton_state=st),
                 lambda: AutomatonControls(2, 3, "cpu", a, st), lambda: AutomatonBeamControls(2, 2, 3, "cpu", a, st)):
        with pytest.raises(ValueError, match="state 2 is reachable and has no open token"):
            call()
    # behind eos a row is finished: with the eos control the walk does not go through it
    b = TA()(torch.tensor([[0, 1, -1], [-1, -1, -1]], dtype=torch.int32))
    with pytest.raises(ValueError, match="state 1 is reachable"):
        AutomatonControls(1, 3, "cpu", b)
    assert AutomatonControls(1, 3, "cpu", b, eos=1).row_state.tolist() == [0]
    # a ban can cut a state off: state 1 is reached through token 0 only
    c = TA()(torch.tensor([[1, 0, 0], [-1, -1, -1]], dtype=torch.int32))
    assert AutomatonControls(1, 3, "cpu", c, banned_tokens=[0]).dead.tolist() == [0]


def test_the_controls_own_and_clone_their_state():
    from vmlmf_amd import AutomatonBeamControls, AutomatonControls, DecodeControls, _automaton
    a = TA().one_of(V, [[1, 2], [3]], 7)
    c = AutomatonControls(3, V, "cpu", a, torch.tensor([0, 1, 0], dtype=torch.int32), eos=7, repetition_penalty=1.2, banned_tokens=[5])
    assert isinstance(c, DecodeControls) and c.STATE == DecodeControls.STATE + ("row_state", "dead")
    assert (c.ENTRY, c.LIBRARY, c.STRUCT) == ("vmlmf_automaton_choose", _automaton.LIBRARY, _automaton.Controls)
    assert c.row_state.dtype == c.dead.dtype == torch.int32 and c.row_state.tolist() == [0, 1, 0] and c.dead.tolist() == [0, 0, 0]
    d = c.clone()
    d.row_state += 1
    d.dead += 1
    d.seen += 1
    assert c.row_state.tolist() == [0, 1, 0] and not c.dead.any() and not c.seen.any() and d.automaton is c.automaton
    s = c.struct()
    assert (s.S, s.next, s.row_state, s.dead, s.eos) == (a.S, a.next.data_ptr(), c.row_state.data_ptr(), c.dead.data_ptr(), 7)
    assert abs(s.repetition_penalty - 1.2) < 1e-6 and s.seen == c.seen.data_ptr()
    # the struct is vmlmf_decode_controls, then the table, then the two pointers
    names = [f[0] for f in _automaton.Controls._fields_]
    assert names[:8] == [f[0] for f in __import__("vmlmf_amd")._decode.Controls._fields_] and names[8:] == ["next", "S", "pad1", "row_state", "dead"]
    assert ctypes.sizeof(_automaton.Controls) == 48 + 16 + 16 and ctypes.sizeof(_automaton.Table) == 16
    bc = AutomatonBeamControls(2, 3, V, "cpu", TA().avoiding(V, [[1, 2]]), torch.tensor([0, 1], dtype=torch.int32), eos=7, min_length=2,
                               banned_tokens=[0, 5])
    assert bc.start().tolist() == [0, 0, 0, 1, 1, 1] and bc.start().dtype == torch.int32 and not bc.keeps_history and bc.clone() is bc
    assert (bc.eos, bc.min_length, bc.closed.tolist()) == (7, 2, [33])
    with pytest.raises(ValueError, match="beams"):
        AutomatonBeamControls(2, 33, V, "cpu", a)


def test_the_beam_steps_workspace_is_the_plain_steps():
    from vmlmf_amd import _automaton, _beam, decoding
    import vmlmf_amd
    assert _automaton.lib().vmlmf_automaton_workspace_bytes(3, 4, 97) == _beam.lib().vmlmf_beam_workspace_bytes(3, 4, 97) == 3 * 4 * 4 * 8
    assert _automaton.lib().vmlmf_automaton_workspace_bytes(3, 33, 97) == 0
    for name in ("TokenAutomaton", "AutomatonControls", "AutomatonBeamControls"):
        assert name in vmlmf_amd.__all__ and getattr(vmlmf_amd, name) is getattr(decoding, name)


def test_the_kernels_are_instantiated_not_copied():
    """The choice is vmlmf_select.h's on a source that wraps ControlledScores, the rows are ControlledRows', the beam step is
    vmlmf_beam_core.h's kernel under a third policy: the new file holds a copy of none of them."""
    text = open(os.path.join(CSRC, "vmlmf_automaton.hip")).read()
    for inc in ("vmlmf_select.h", "vmlmf_controlled.h", "vmlmf_beam_core.h"):
        assert '#include "%s"' % inc in text
    for fn in ("radix_select", "tie_cutoff", "best_merge", "lse_merge", "key_of", "choose_row", "pick_row", "for_quads", "write_pick", "wg_max",
               "padding", "finish"):
        assert not re.search(r"__device__[^;{]*\b%s\s*\(" % fn, text), fn
    assert not re.search(r"struct (ControlledScores|ControlledRows|BeamScratch|SelScratch)\b", text) and "__global__" in text
    assert re.search(r"\bpick_row\s*\(", text) and re.search(r"\bchoose_row\s*\(", text) and "beam_step_kernel<OfferAutomaton>" in text
    assert len(re.findall(r"__global__", text)) == 1 and "asm" not in text.replace("disassembl", "") and "atomic" not in text.replace("no float atomics", "")
    core = open(os.path.join(CSRC, "vmlmf_beam_core.h")).read()
    assert len(re.findall(r"if constexpr \(moves_states<P>::value\)", core)) == 1       # the one hook


# ---- the C ABI's refusals: all on the host, in front of any launch ----
def _choose(B=2, H=8, V=16, scores=1, inv=1.0, top_k=0, top_p=1.0, state=1, step=0, tokens=1, xn=None, embed=None,
            controls=(1.0, -1, 0, 0, None, 1, 1, 1), table=(1, 3, 0), row_state=1, dead=1, null_controls=False):
    """vmlmf_automaton_choose with fake, never dereferenced pointers (1 = some non-null address)."""
    from vmlmf_amd import _automaton
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    lib = _automaton.lib()
    c = None if null_controls else ctypes.byref(_automaton.Controls(*controls, *table, row_state, dead))
    rc = lib.vmlmf_automaton_choose(B, H, V, p(scores), None, p(embed), inv, top_k, top_p, p(state), step, c, p(tokens), None, p(xn), None, None)
    return rc, lib.vmlmf_automaton_last_error().decode()


def _beam_step(B=2, W=3, H=8, V=16, eos=-1, min_length=0, table=(1, 3, 0), state=1, state_out=2, null_table=False, scores=1, cum=1, total=2,
               embed=None, xn=None, ws=8, ws_bytes=1 << 20):
    """vmlmf_automaton_beam_step with fake, never dereferenced pointers."""
    from vmlmf_amd import _automaton
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    lib = _automaton.lib()
    t = None if null_table else ctypes.byref(_automaton.Table(*table))
    rc = lib.vmlmf_automaton_beam_step(B, W, H, V, p(scores), None, p(cum), p(1), p(1), eos, p(embed), min_length, None, t, p(state), p(state_out),
                                       p(1), p(1), p(total), p(2), p(2), p(xn), p(1), p(1), p(ws), ws_bytes, None)
    return rc, lib.vmlmf_automaton_last_error().decode()


def test_the_entry_points_refuse_on_the_host():
    from vmlmf_amd import _lib
    nan = float("nan")
    choose = [
        (dict(null_controls=True), _lib.E_BADARG, "null controls"),
        (dict(table=(None, 3, 0)), _lib.E_BADARG, "the table's next"), (dict(table=(1, 0, 0)), _lib.E_BADARG, "S >= 1"),
        (dict(table=(1, -2, 0)), _lib.E_BADARG, "S >= 1"), (dict(table=(1, 1 << 27, 0)), _lib.E_BADARG, "S V must stay below 2^31"),
        (dict(row_state=None), _lib.E_BADARG, "row_state and dead"), (dict(dead=None), _lib.E_BADARG, "row_state and dead"),
        # ... and whatever vmlmf_decode_choose refuses
        (dict(B=0), _lib.E_BADARG, "B, "), (dict(V=-3), _lib.E_BADARG, "B, "), (dict(scores=None), _lib.E_BADARG, "null"),
        (dict(tokens=None), _lib.E_BADARG, "null"), (dict(inv=-1.0), _lib.E_BADARG, "temperature"), (dict(inv=nan), _lib.E_BADARG, "temperature"),
        (dict(state=None), _lib.E_BADARG, "snapshot"), (dict(xn=1, embed=None), _lib.E_BADARG, "embedding"), (dict(step=-1), _lib.E_BADARG, "step"),
        (dict(top_k=-1), _lib.E_BADARG, "top_k"), (dict(top_p=0.0), _lib.E_BADARG, "top_p"), (dict(top_p=1.5), _lib.E_BADARG, "top_p"),
        (dict(B=1 << 16, step=1 << 16), _lib.E_UNSUPPORTED, "2^32"),
        (dict(controls=(1.0, -1, 0, 0, None, None, 1, 1)), _lib.E_BADARG, "seen"), (dict(controls=(1.0, 16, 0, 0, None, 1, 1, 1)), _lib.E_BADARG, "eos"),
        (dict(controls=(0.0, -1, 0, 0, None, 1, 1, 1)), _lib.E_BADARG, "repetition_penalty"),
        (dict(controls=(1.0, -1, 1, 0, None, 1, 1, 1)), _lib.E_BADARG, "min_length needs eos"),
    ]
    for kw, code, words in choose:
        rc, msg = _choose(**kw)
        assert rc == code and words in msg and msg.startswith("vmlmf_automaton_choose: "), (kw, rc, msg)
    beam = [
        (dict(null_table=True), _lib.E_BADARG, "null table"), (dict(table=(None, 3, 0)), _lib.E_BADARG, "the table's next"),
        (dict(table=(1, 0, 0)), _lib.E_BADARG, "S >= 1"), (dict(table=(1, 1 << 27, 0)), _lib.E_BADARG, "S V must stay below 2^31"),
        (dict(state=None), _lib.E_BADARG, "beam_state and beam_state_out"), (dict(state_out=None), _lib.E_BADARG, "beam_state and beam_state_out"),
        (dict(state=5, state_out=5), _lib.E_BADARG, "must not alias beam_state"),
        (dict(min_length=-1), _lib.E_BADARG, "min_length must be >= 0"), (dict(min_length=2), _lib.E_BADARG, "min_length needs eos"),
        # ... and whatever vmlmf_beam_step refuses
        (dict(B=0), _lib.E_BADARG, "B, H and V"), (dict(W=33), _lib.E_BADARG, r"[1, 32]"), (dict(W=3, V=2), _lib.E_BADARG, "exceed V"),
        (dict(eos=16), _lib.E_BADARG, "eos"), (dict(scores=None), _lib.E_BADARG, "null pointer"), (dict(cum=2, total=2), _lib.E_BADARG, "alias"),
        (dict(xn=1), _lib.E_BADARG, "come together"), (dict(ws=4), _lib.E_BADARG, "8-byte aligned"),
        (dict(ws_bytes=8), _lib.E_WORKSPACE, "vmlmf_automaton_workspace_bytes"),
    ]
    for kw, code, words in beam:
        rc, msg = _beam_step(**kw)
        assert rc == code and words in msg and msg.startswith("vmlmf_automaton_beam_step: "), (kw, rc, msg)
