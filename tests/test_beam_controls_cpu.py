"""The controls of Model.beam_search (min_length, banned_tokens, no_repeat_ngram_size, banned_sequences; C ABI vmlmf_beamctl_step in
libvmlmf_beamctl.so, include/vmlmf_beamctl.h): what can be checked without a GPU, beside the table test_side_libraries_cpu.py holds
every side library to - the step written once; every refusal, in Python and at the C ABI; the workspace; the
controlled fp64 search (beam_control_cases.py) against the oracle's own; and the conditions on the reference alone that the GPU tests
rely on."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import beam_control_cases as K
import vmlmf_decode_oracle as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vmlmf_amd", "csrc")


def test_the_step_is_written_once():
    """Both libraries instantiate the kernel of vmlmf_beam_core.h; neither holds a copy of it or of its parts."""
    core = open(os.path.join(CSRC, "vmlmf_beam_core.h")).read()
    parts = ("key_of", "total_of", "index_of", "row_max", "wave_max", "wg_max", "beam_step_kernel")
    for fn in parts:
        assert re.search(r"\b%s\s*\(" % fn, core), fn
    assert "struct BeamScratch" in core and "if constexpr (P::controlled)" in core
    for name, policy in (("vmlmf_beam.hip", "OfferAll"), ("vmlmf_beamctl.hip", "OfferOpen")):
        text = open(os.path.join(CSRC, name)).read()
        assert '#include "vmlmf_beam_core.h"' in text and "beam_step_kernel<%s>" % policy in text
        assert "struct BeamScratch" not in text
        for fn in parts:
            assert not re.search(r"(__device__|__global__)[^;{]*\b%s\s*\(" % fn, text), (name, fn)
    history = open(os.path.join(CSRC, "vmlmf_history.hip")).read()
    assert len(re.findall(r"__device__[^;{]*\bhistory_bans\s*\(", history)) == 1              # the ban sets are formed there alone
    assert "history_bans" not in open(os.path.join(CSRC, "vmlmf_beamctl.hip")).read().replace("vmlmf_history_bans", "")


# ---- every refusal, in Python ----
REFUSALS = [
    (dict(min_length=-1, eos=3), "min_length must be >= 0"), (dict(min_length=2), "needs eos"),
    (dict(eos=97), "eos=97 is not a token"), (dict(banned_tokens=[97]), "banned token 97"), (dict(banned_tokens=[-1]), "banned token -1"),
    (dict(banned_tokens=[3, 5], eos=3), "eos=3 is among banned_tokens"),
    (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"), (dict(no_repeat_ngram_size=1.5), "no_repeat_ngram_size"),
    (dict(no_repeat_ngram_size="two"), "no_repeat_ngram_size"),
    (dict(banned_sequences=[[1, 2], []]), "empty sequence"), (dict(banned_sequences=[[1, 97]]), "banned sequence token 97"),
    (dict(banned_sequences=[[-1]]), "banned sequence token -1"), (dict(banned_sequences=[3]), "list of lists"),
    (dict(banned_sequences=[[1] * 4097]), "more than 4096"),
]


def _model(V=97):
    from vmlmf_amd import Model
    torch.manual_seed(0)
    return Model(V, 8, 1, 0.0, 0.1, w_rank=4, u_ranks=[4], lstm_type="vmlmf")


@pytest.mark.parametrize("kw,words", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_check_beam_controls_beam_controls_and_beam_search_refuse(kw, words):
    from vmlmf_amd import BeamControls, _beamctl, _decode, _history
    with pytest.raises(ValueError, match=words):
        _beamctl.check_beam_controls(97, 4, **kw)
    with pytest.raises(ValueError, match=words):
        BeamControls(2, 4, 97, "cpu", **kw)
    with pytest.raises(ValueError, match=words):                          # before the refusal of CPU tensors
        _model().beam_search(torch.zeros((3, 2), dtype=torch.int64), 4, **kw)
    if "among banned_tokens" not in words:                                # ... and what generate's own checks say of the same arguments
        with pytest.raises(ValueError, match=words):
            ctl = {k: v for k, v in kw.items() if k in ("eos", "min_length", "banned_tokens")}
            _decode.check_controls(97, **ctl)
            _history.check_history(97, **{k: v for k, v in kw.items() if k not in ctl})


def test_the_room_for_w_candidates_and_the_widest_vocabulary():
    from vmlmf_amd import BeamControls, _beamctl
    prompt = torch.zeros((5, 2), dtype=torch.int64)
    ok = dict(no_repeat_ngram_size=2, banned_sequences=[[1, 2], [4]], banned_tokens=[7, 8], eos=3, min_length=2)
    # closed = 2 banned + eos under min_length; T0 5, steps 10, 2 sequences, W 4: 3 + 5 + 10 + 2 + 4 = 24
    assert _beamctl.check_beam_controls(24, 4, prompt_length=5, steps=10, **ok) == (3, 2, [7, 8], 2, [[1, 2], [4]])
    with pytest.raises(ValueError, match="fewer than 4 candidates.*= 24"):
        _beamctl.check_beam_controls(23, 4, prompt_length=5, steps=10, **ok)
    _beamctl.check_beam_controls(23, 3, prompt_length=5, steps=10, **ok)
    _beamctl.check_beam_controls(16, 4, **ok)                               # without `steps` the room is not looked at
    m = _model(24)
    with pytest.raises(ValueError, match="fewer than 4 candidates"):
        m.beam_search(prompt, 11, beams=4, **ok)
    with pytest.raises(RuntimeError, match="cuda"):
        m.beam_search(prompt, 10, beams=4, **ok)
    with pytest.raises(RuntimeError, match="cuda"):                          # without the arguments nothing of them is checked
        m.beam_search(prompt, 1000, beams=4, eos=3)
    with pytest.raises(ValueError, match="at most 65536"):
        _beamctl.check_beam_controls(65537, 4, no_repeat_ngram_size=2)
    with pytest.raises(ValueError, match="at most 65536"):
        _beamctl.check_beam_controls(65537, 4, banned_sequences=[[1, 2]])
    _beamctl.check_beam_controls(65537, 4, banned_tokens=[1], eos=3, min_length=2)    # closed words and min_length carry no limit
    _beamctl.check_beam_controls(65536, 4, no_repeat_ngram_size=2)
    with pytest.raises(ValueError, match="capacity"):
        BeamControls(2, 4, 97, "cpu", prompt=prompt, capacity=4, no_repeat_ngram_size=2)
    with pytest.raises(ValueError, match="prompt"):
        BeamControls(3, 4, 97, "cpu", prompt=prompt)
    with pytest.raises(ValueError, match="beams"):
        BeamControls(2, 33, 97, "cpu")
    assert not _beamctl.controls_on() and not _beamctl.controls_on(0, None, 0, None)
    assert _beamctl.controls_on(1) and _beamctl.controls_on(banned_tokens=[]) and _beamctl.controls_on(no_repeat_ngram_size=2)
    assert _beamctl.controls_on(banned_sequences=[])


def test_lm_beam_steps_signature_starts_as_it_did():
    import vmlmf_amd
    from vmlmf_amd import decoding
    assert list(inspect.signature(vmlmf_amd.lm_beam_step).parameters)[:9] == ["h", "weight", "bias", "cum", "finished", "length", "eos", "embed",
                                                                              "buffers"]
    assert "BeamControls" in vmlmf_amd.__all__ and vmlmf_amd.BeamControls is decoding.BeamControls


def test_beam_controls_owns_the_closed_words_and_the_sequences_and_starts_the_histories():
    from vmlmf_amd import BeamControls, _beamctl
    prompt = torch.tensor([[0, 5], [2, 5], [0, 96]])
    c = BeamControls(2, 3, 97, "cpu", prompt=prompt, capacity=7, min_length=2, banned_tokens=[0, 31, 32, 96], no_repeat_ngram_size=3,
                     banned_sequences=[[1, 2], (4,)], eos=3)
    assert (c.eos, c.min_length, c.no_repeat_ngram_size, c.sequences, c.capacity, c.keeps_history) == (3, 2, 3, [[1, 2], [4]], 7, True)
    assert c.closed.dtype == torch.int32 and c.closed.tolist() == [1 - (1 << 31), 1, 0, 1]     # bits 0 and 31; 32; -; 96
    assert np.array_equal(K.pack(np.isin(np.arange(97), [0, 31, 32, 96])), c.closed.numpy())
    assert c.seq_tokens.tolist() == [1, 2, 4] and c.seq_offsets.tolist() == [0, 2, 3]
    assert c.overflow.dtype == torch.int32 and c.overflow.tolist() == [0, 0]
    hist, hist_len = c.history()
    assert hist.dtype == hist_len.dtype == torch.int32 and hist_len.tolist() == [3] * 6
    assert hist.tolist() == [[0, 2, 0, 0, 0, 0, 0]] * 3 + [[5, 5, 96, 0, 0, 0, 0]] * 3        # the prompt, repeated for the W beams
    again = c.history()
    assert again[0].data_ptr() != hist.data_ptr() and torch.equal(again[0], hist)              # fresh copies: the history is carried
    d = c.clone()
    assert d.overflow.data_ptr() != c.overflow.data_ptr() and d.closed is c.closed and d.seq_tokens is c.seq_tokens
    e = BeamControls(2, 3, 97, "cpu", prompt=prompt, min_length=1, eos=3)
    assert not e.keeps_history and e.history() == (None, None) and e.closed is None and e.seq_tokens is None and e.capacity == 3 + 1024
    assert np.array_equal(K.pack(np.arange(33) == 32), _beamctl.pack_words([32], 33).numpy())    # the last mask word holds one token
    s = _beamctl.Controls(2, 7, None, None, 1, 2, 3, 4, 5)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vmlmf_beamctl.h")).read(), flags=re.S)
    body = re.search(r"typedef struct vmlmf_beamctl_controls \{(.*?)\} vmlmf_beamctl_controls;", header, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [f[0] for f in _beamctl.Controls._fields_]             # the struct is the header's
    assert (s.min_length, s.hist_capacity, s.hist, s.overflow) == (2, 7, 1, 5)
    assert ctypes.sizeof(_beamctl.Controls) == 8 + 7 * ctypes.sizeof(ctypes.c_void_p)


# ---- the entry point's refusals on the host, and the workspace ----
def _step(B=2, W=4, H=8, V=97, scores=1, cum=2, finished=3, length=4, eos=7, embed=None, controls=True, parent=5, token=6, total=7,
          finished_out=8, length_out=9, xn=None, src=10, ticket=11, ws=16, ws_bytes=1 << 20, min_length=0, cap=8, closed=None, bans=None,
          hist=None, hist_len=None, hist_out=None, hist_len_out=None, overflow=None):
    """vmlmf_beamctl_step with fake, never dereferenced pointers (small integers): refusals come before any launch."""
    from vmlmf_amd import _beamctl
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    lib = _beamctl.lib()
    c = _beamctl.Controls(min_length, cap, closed, bans, hist, hist_len, hist_out, hist_len_out, overflow)
    rc = lib.vmlmf_beamctl_step(B, W, H, V, p(scores), None, p(cum), p(finished), p(length), eos, p(embed), ctypes.byref(c) if controls else None,
                                p(parent), p(token), p(total), p(finished_out), p(length_out), p(xn), p(src), p(ticket), p(ws), ws_bytes, None)
    return rc, lib.vmlmf_beamctl_last_error().decode()


def test_the_entry_point_refuses_on_the_host():
    from vmlmf_amd import _lib
    bad = _lib.E_BADARG
    full = dict(hist=20, hist_len=21, hist_out=22, hist_len_out=23, overflow=24)
    cases = [
        # what vmlmf_beam_step refuses
        (dict(B=0), bad, "B, H and V"), (dict(H=0), bad, "B, H and V"), (dict(V=0), bad, "B, H and V"), (dict(W=0), bad, "W (beams)"),
        (dict(W=33), bad, "W (beams)"), (dict(W=4, V=3, eos=-1), bad, "must not exceed V"), (dict(W=32, V=1 << 26), bad, "2^31"),
        (dict(eos=97), bad, "eos"), (dict(eos=-2), bad, "eos"), (dict(scores=None), bad, "null pointer"), (dict(cum=None), bad, "null pointer"),
        (dict(finished=None), bad, "null pointer"), (dict(length=None), bad, "null pointer"), (dict(parent=None), bad, "null pointer"),
        (dict(token=None), bad, "null pointer"), (dict(total=None), bad, "null pointer"), (dict(finished_out=None), bad, "null pointer"),
        (dict(length_out=None), bad, "null pointer"), (dict(src=None), bad, "null pointer"), (dict(ticket=None), bad, "null pointer"),
        (dict(ws=None), bad, "null pointer"), (dict(embed=30), bad, "embed and x_next"), (dict(xn=30), bad, "embed and x_next"),
        (dict(total=2), bad, "alias"), (dict(finished_out=3), bad, "alias"), (dict(length_out=4), bad, "alias"), (dict(ws=12), bad, "8-byte aligned"),
        (dict(ws_bytes=2 * 4 * 4 * 8 - 1), _lib.E_WORKSPACE, "vmlmf_beamctl_workspace_bytes"),
        # ... and the controls' own
        (dict(controls=False), bad, "null controls"), (dict(min_length=-1), bad, "min_length must be >= 0"),
        (dict(min_length=1, eos=-1), bad, "min_length needs eos"), (dict(cap=0), bad, "hist_capacity"), (dict(cap=0, **full), bad, "hist_capacity"),
        (dict(bans=40, V=65537), bad, "VMLMF_HISTORY_MAX_V"), (dict(**{**full, "hist_out": 20}), bad, "must not alias"),
    ]
    for missing in full:                                                   # hist without one of the others
        cases.append((dict(**{**full, missing: None}), bad, "come together"))
    for only in full:                                                      # ... or one of them without the rest
        cases.append((dict(**{only: full[only]}), bad, "come together"))
    for kw, code, words in cases:
        rc, msg = _step(**kw)
        assert rc == code and words in msg and msg.startswith("vmlmf_beamctl_step: "), (kw, rc, msg)


def test_the_workspace_is_the_plain_steps():
    from vmlmf_amd import _beam, _beamctl
    ws, plain = _beamctl.lib().vmlmf_beamctl_workspace_bytes, _beam.lib().vmlmf_beam_workspace_bytes
    for B, W, V in [(1, 1, 1), (2, 4, 97), (3, 32, 10000), (32, 4, 10000), (1, 16, 12293)]:
        assert ws(B, W, V) == plain(B, W, V) == B * W * W * 8
    for B, W, V in [(0, 4, 97), (2, 0, 97), (2, 33, 97), (2, 4, 3), (2, 4, 0), (2, 32, 1 << 26)]:
        assert ws(B, W, V) == plain(B, W, V) == 0


# ---- the controlled oracle ----
@pytest.mark.parametrize("kind,B,W,seed", C.MODEL_CASES)
def test_the_controlled_search_with_neutral_controls_is_the_oracles_own(kind, B, W, seed):
    m, prompt = K.model_and_prompt(kind, B, seed)
    clear, fin, hyps, cum = C.oracle_beam_search(m, prompt, W, K.MODEL_STEPS, K.MODEL_EOS)
    mine = K.uncontrolled(kind, B, W, seed)
    assert mine[0] == clear and np.array_equal(mine[1], fin) and np.array_equal(mine[2], hyps) and np.array_equal(mine[3], cum)
    for b in range(B):                                                    # ... and the lengths it carries are the hypotheses'
        for w in range(W):
            assert mine[4][b, w] == len(K.until_eos(hyps[:, b, w], K.MODEL_EOS))


@pytest.mark.parametrize("case", K.KERNEL_SHAPES, ids=lambda c: "x".join(map(str, c)))
def test_the_neutral_kernel_oracle_is_the_plain_steps_and_the_masks_bite(case):
    B, W, H, V = case
    for mine, ref in zip(K.kernel_oracle(case, masked=False), C.kernel_oracle(case)):
        assert np.array_equal(mine[0], ref[0]) and np.array_equal(mine[1], ref[1]) and list(mine[2]) == list(ref[2]) and mine[3:] == ref[3:]
    closed, bans = K.kernel_masks(case)
    assert closed.any() and bans.any(1).all() and not closed[K.EOS] and not bans[:, K.EOS].any()
    assert np.array_equal(K.pack(bans)[:, -1] != 0, bans[:, (V - 1) // 32 * 32:].any(1))          # the last, partial word
    fin, length = C.kernel_case(*case)[4:]
    changed = 0
    for r, (masked, ref) in enumerate(zip(K.kernel_oracle(case), C.kernel_oracle(case))):
        changed += list(masked[2]) != list(ref[2])
        live = ~fin[r].numpy()
        assert (masked[1][live].sum(1) >= W).all()                        # every live beam still offers at least W candidates
        for w in np.flatnonzero(live):
            assert not masked[1][w][closed | bans[r * W + w]].any()
            assert masked[1][w, K.EOS] == (length[r, w] >= K.KERNEL_MIN_LENGTH)
    assert changed >= 1


# ---- the conditions of the GPU tests, on the reference alone ----
@pytest.mark.parametrize("case", K.KERNEL_SHAPES, ids=lambda c: "x".join(map(str, c)))
def test_every_row_of_the_masked_kernel_cases_is_clear(case):
    for r, (totals, valid, top, lo, hi) in enumerate(K.kernel_oracle(case)):
        assert lo == hi == set(top.tolist()), (case, r, sorted(lo), sorted(hi))


@pytest.mark.parametrize("name", K.SETTINGS)
@pytest.mark.parametrize("kind,B,W,seed", C.MODEL_CASES)
def test_the_controlled_model_cases_are_mostly_clear_and_the_controls_bite(kind, B, W, seed, name):
    kw = K.setting(name, kind, B, W, seed)
    n, min_length, seqs = kw["no_repeat_ngram_size"], kw.get("min_length", 0), kw.get("banned_sequences", [])
    clear, fin, hyps, cum, length = K.controlled(name, kind, B, W, seed)
    _, _, hyps0, _, length0 = K.uncontrolled(kind, B, W, seed)
    print(f"{kind} {B}x{W} {name}: clear share {np.mean(clear):.3f}, hypotheses changed {int((hyps != hyps0).any(0).sum())} of {B * W}")
    assert np.mean(clear) >= 0.9, (int(np.sum(clear)), len(clear))
    prompt = K.model_and_prompt(kind, B, seed)[1].numpy()
    whole = lambda h, b, w: list(prompt[:, b]) + K.until_eos(h[:, b, w], K.MODEL_EOS)
    rows = [(b, w) for b in range(B) for w in range(W)]
    repeats0 = sum(K.repeated_ngrams(whole(hyps0, b, w), n) for b, w in rows)
    short0 = int((length0 < min_length).sum())
    held0 = sum(K.contains(whole(hyps0, b, w), s) for b, w in rows for s in seqs)
    assert repeats0 + short0 > 0 and (not seqs or held0 > 0)               # the uncontrolled search repeats, stops early, holds the sequences
    assert sum(K.repeated_ngrams(whole(hyps, b, w), n) for b, w in rows) == 0
    assert int((length < min_length).sum()) == 0 and not any(K.contains(whole(hyps, b, w), s) for b, w in rows for s in seqs)
    assert (hyps != hyps0).any()
    assert 0 < fin.sum() < fin.size or min_length > 0                      # finished and live beams meet in the search
