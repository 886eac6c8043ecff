"""CPU: the fp64 oracle of one beam-search step (vmlmf_decode_oracle.step_sets, where the rule a GPU step is judged by is stated), the
conditions the GPU tests (tests/test_gpu_beam.py) rely on - checked on the oracle alone -, and the host side of libvmlmf_beam.so
(include/vmlmf_beam.h): the workspace size and the argument checks."""
import ctypes

import numpy as np
import pytest
import torch

from lm_util import beam_model, cpu_prompt
from vmlmf_decode_oracle import KERNEL_CASES, MODEL_CASES, MODEL_EOS, MODEL_STEPS, kernel_oracle, oracle_beam_search, step_sets
# ---- conditions on the oracle alone ----
@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_every_row_of_the_kernel_level_cases_is_clear(case):
    B, W, H, V = case
    rows = kernel_oracle(case)
    assert len(rows) == B
    for r, (totals, valid, top, lo, hi) in enumerate(rows):
        assert lo == hi == set(top.tolist()), (case, r, sorted(hi - lo))
        assert len(top) == W


def test_step_sets_orders_ties_by_flat_index_and_sees_the_margin():
    totals = np.array([[0.0, -1.0, -1.0, -5.0], [-1.0, -2.0, -1.00005, -9.0]])
    valid = np.ones((2, 4), dtype=bool)
    top, lo, hi = step_sets(totals, valid, 3, 1e-4)
    assert top.tolist() == [0, 1, 2]                    # the tie -1 = -1 = -1 over flat 1, 2, 4 goes to the lower indices
    assert lo == {0} and hi == {0, 1, 2, 4, 6}
    valid[1] = [False, False, True, False]              # a finished beam offers one token only
    top, lo, hi = step_sets(totals, valid, 3, 1e-6)
    assert top.tolist() == [0, 1, 2] and lo == hi == {0, 1, 2}
    totals[1, :] = -np.inf                              # a beam that does not exist yet loses to every finite candidate
    valid[:] = True
    top, lo, hi = step_sets(totals, valid, 4, 1e-4)
    assert top.tolist() == [0, 1, 2, 3] and lo == hi == {0, 1, 2, 3}


@pytest.mark.parametrize("kind,B,W,seed", MODEL_CASES)
def test_the_model_level_cases_are_mostly_clear_and_finish_some_beams(kind, B, W, seed):
    m = beam_model(kind)
    clear, fin, hyps, _ = oracle_beam_search(m, cpu_prompt(B, seed=seed), W, MODEL_STEPS, MODEL_EOS)
    assert len(clear) == MODEL_STEPS * B
    assert np.mean(clear) >= 0.9, (kind, B, W, int(np.sum(clear)), len(clear))
    assert 0 < fin.sum() < fin.size, (kind, B, W, int(fin.sum()))
    # a finished hypothesis is padded with eos
    for b in range(B):
        for w in range(W):
            hit = np.flatnonzero(hyps[:, b, w] == MODEL_EOS)
            assert fin[b, w] == (len(hit) > 0)
            if len(hit):
                assert (hyps[hit[0]:, b, w] == MODEL_EOS).all()


# ---- the protocol of a beam policy ----
def test_the_four_policies_share_one_protocol():
    """BeamControls, AutomatonBeamControls, GroupBeams and StochasticBeams are BeamPolicy objects: a search that starts has beam 0 of a
    row at 0 and the others at -inf (a group search: the first slot of every group), and a keyword a policy does not carry is refused."""
    import math
    from vmlmf_amd import AutomatonBeamControls, BeamControls, GroupBeams, StochasticBeams, TokenAutomaton, _beam, decoding, lm_beam_step
    B, W, V, inf = 2, 4, 97, math.inf
    prompt = torch.zeros((3, B), dtype=torch.int64)
    plain = _beam.BeamPolicy(B, W, V, "cpu")
    policies = [BeamControls(B, W, V, "cpu"), BeamControls(B, W, V, "cpu", prompt=prompt, no_repeat_ngram_size=2),
                AutomatonBeamControls(B, W, V, "cpu", TokenAutomaton.avoiding(V, [[1, 2]])), GroupBeams(B, W, V, "cpu", groups=2),
                StochasticBeams(B, W, V, "cpu")]
    zeros = torch.zeros((B, W), dtype=torch.int32)
    for p in [plain] + policies:
        assert isinstance(p, _beam.BeamPolicy) and (p.B, p.W, p.V, p.device) == (B, W, V, torch.device("cpu"))
        cum, fin, ln = p.first_beams()
        grouped = isinstance(p, GroupBeams)
        assert cum.dtype == torch.float32 and cum.tolist() == [[0.0, -inf, 0.0 if grouped else -inf, -inf]] * B, type(p).__name__
        assert fin.dtype == ln.dtype == torch.int32 and torch.equal(fin, zeros) and torch.equal(ln, zeros)
        assert fin.data_ptr() != ln.data_ptr()
        assert len(p.first_carried()) == len(p.carried) and p.keeps_history == (p.carried == ("hist", "hist_len"))
    assert [p.carried for p in [plain] + policies] == [(), (), ("hist", "hist_len"), ("beam_state",), (), ("perturbed", "draw")]
    assert policies[3].clone() is policies[3] and policies[1].clone() is not policies[1] and plain.first_carried() == []
    assert all(torch.equal(x, y) for x, y in zip(policies[3].first_beams(), policies[3].start()))
    # a keyword the controls do not carry: a TypeError that names it, before anything else is looked at
    x = torch.zeros(B * W, dtype=torch.int32)
    step = (torch.zeros(B * W, 8), torch.zeros(V, 8), None, *plain.first_beams(), None)
    for controls, kw in ((policies[3], dict(hist=x)), (policies[3], dict(beam_state=x)), (None, dict(hist=x)), (policies[2], dict(hist_len=x)),
                         (policies[0], dict(hist=x)), (policies[4], dict(beam_state=x)), (policies[1], dict(perturbed=x))):
        with pytest.raises(TypeError, match=next(iter(kw))):
            lm_beam_step(*step, controls=controls, **kw)
        with pytest.raises(TypeError, match=next(iter(kw))):
            decoding.beam_steps(None, None, [], *plain.first_beams(), 1, None, controls=controls, **kw)
        with pytest.raises(TypeError, match=next(iter(kw))):
            decoding._beam_start(controls, **kw)
    with pytest.raises(RuntimeError, match="HIP device"):                  # (a carried keyword passes on to the step's own checks)
        lm_beam_step(*step, controls=policies[2], beam_state=x)
    assert decoding._beam_start(None) == [] and decoding._beam_start(policies[3]) == []
    hist, hist_len = decoding._beam_start(policies[1])
    assert hist.shape == (B * W, policies[1].capacity) and hist_len.tolist() == [3] * (B * W)
    assert decoding._beam_start(policies[1], hist=hist, hist_len=hist_len)[0] is hist
    pert, draw = decoding._beam_start(policies[4], draw=x[:B])
    assert draw.data_ptr() == x.data_ptr() and pert.tolist() == [[0.0, -inf, -inf, -inf]] * B      # each default on its own


# ---- host-side checks ----
def test_beam_search_refuses_bad_beam_counts_before_anything_else():
    from vmlmf_amd import Model
    m = Model(97, 32, 2, 0.0, 0.1, w_rank=8, u_ranks=[8], lstm_type="vmlmf")
    prompt = torch.zeros((3, 2), dtype=torch.int64)
    for beams in (0, -1, 33, 98):
        with pytest.raises(ValueError, match="beams"):
            m.beam_search(prompt, 4, beams=beams)
    small = Model(5, 8, 1, 0.0, 0.1, w_rank=2, u_ranks=[2], lstm_type="vmlmf")
    with pytest.raises(ValueError, match="beams"):
        small.beam_search(prompt, 4, beams=6)                        # beams > V
    with pytest.raises(ValueError, match="eos"):
        m.beam_search(prompt, 4, eos=97)
    with pytest.raises(ValueError, match="chunk"):
        m.beam_search(prompt, 4, chunk=3)
    with pytest.raises(ValueError, match="length_penalty"):
        m.beam_search(prompt, 4, length_penalty=-1.0)
    with pytest.raises(RuntimeError, match="cuda"):                 # CPU tensors raise as in generate
        m.beam_search(prompt, 4)


def test_workspace_bytes():
    from vmlmf_amd import _beam
    ws = _beam.lib().vmlmf_beam_workspace_bytes
    assert ws(2, 4, 97) == 2 * 4 * 4 * 8 and ws(1, 1, 10000) == 8 and ws(32, 32, 10000) == 32 * 32 * 32 * 8
    assert ws(1, 16, 10 ** 8) == 16 * 16 * 8                         # any row length
    for bad in ((0, 4, 97), (2, 0, 97), (2, 33, 97), (2, 4, 3), (2, 4, 0), (1, 32, 2 ** 26)):
        assert ws(*bad) == 0, bad


def test_the_entry_points_refuse_bad_arguments_without_touching_the_gpu():
    from vmlmf_amd import _beam, _lib
    lib = _beam.lib()
    one = ctypes.c_void_p(16)                                        # never dereferenced: every call below is refused first
    good = dict(B=2, W=4, H=32, V=97, eos=7, ws=256)

    out = ctypes.c_void_p(32)

    def step(B=2, W=4, H=32, V=97, eos=7, ws=256, scores=one, embed=one, x_next=out, total=out, cum=one, workspace=one):
        return lib.vmlmf_beam_step(B, W, H, V, scores, one, cum, one, one, eos, embed, out, out, total, out, out, x_next, out, one,
                                   workspace, ws, None)

    for kw, word in ((dict(B=0), b">= 1"), (dict(W=0), b"beams"), (dict(W=33), b"beams"), (dict(W=4, V=3, eos=-1), b"exceed V"),
                     (dict(eos=97), b"eos"), (dict(eos=-2), b"eos"), (dict(scores=None), b"null"), (dict(embed=None), b"together"),
                     (dict(x_next=None), b"together"), (dict(total=one, cum=one), b"alias"), (dict(workspace=ctypes.c_void_p(12)), b"aligned"),
                     (dict(W=32, V=2 ** 26, eos=-1), b"2^31")):
        assert step(**kw) == _lib.E_BADARG, kw
        assert word in lib.vmlmf_beam_last_error(), (kw, lib.vmlmf_beam_last_error())
    assert step(ws=255) == _lib.E_WORKSPACE and b"workspace" in lib.vmlmf_beam_last_error()
    assert good["ws"] == lib.vmlmf_beam_workspace_bytes(2, 4, 97)
    two = (ctypes.c_void_p * 2)(16, 32)
    other = (ctypes.c_void_p * 2)(48, 64)
    for args, word in (((0, 8, 32, one, two, other, None), b"n must"), ((17, 8, 32, one, two, other, None), b"n must"),
                       ((2, 0, 32, one, two, other, None), b">= 1"), ((2, 8, 32, None, two, other, None), b"null"),
                       ((2, 8, 32, one, two, (ctypes.c_void_p * 2)(48, 16), None), b"also a source"),
                       ((2, 8, 32, one, two, (ctypes.c_void_p * 2)(48, 0), None), b"null")):
        assert lib.vmlmf_beam_gather(*args) == _lib.E_BADARG, args
        assert word in lib.vmlmf_beam_last_error(), (args, lib.vmlmf_beam_last_error())
    for args, word in (((0, 2, 4, one, one, None, one, None), b"steps"), ((3, 2, 33, one, one, None, one, None), b"beams"),
                       ((3, 2, 4, None, one, None, one, None), b"null"), ((3, 2, 4, one, one, None, None, None), b"null")):
        assert lib.vmlmf_beam_backtrack(*args) == _lib.E_BADARG, args
        assert word in lib.vmlmf_beam_last_error(), (args, lib.vmlmf_beam_last_error())
    with pytest.raises(_lib.VmlmfError) as ei:
        _beam.check(step(W=33))
    assert ei.value.code == _lib.E_BADARG and "beams" in str(ei.value)
