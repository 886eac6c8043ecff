"""Model.stochastic_beam_search and libvmlmf_sbeam.so without a GPU: the kernel-level cases of sbeam_cases.py are all clear in the fp64
reference, the reference's own properties (the largest child inherits its parent's value, no child exceeds it, the first tokens are a
sample without replacement); the refusals, from Python and from the C entry point; the workspace; what the package exports; the
signatures.  Header, SYMBOLS, exports, ABI number, Makefile and lazy loading: test_side_libraries_cpu.py's table."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import sbeam_cases as SC
from vmlmf_amd import _sbeam            # (the binding under test: without it nothing here runs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vmlmf_amd", "csrc")


# ---- the cases and the reference ----
def test_the_cases_are_the_prescribed_ones():
    assert SC.KERNEL_CASES == [(1, 4, 16, 97), (3, 6, 16, 1000), (1, 32, 8, 64), (2, 4, 8, 12293), (2, 1, 16, 97)]
    assert SC.VARIANTS == ["base", "finished", "first"] and len(SC.DRAWS) >= 2 and 0 in SC.DRAWS and any(d != 0 for d in SC.DRAWS)
    assert SC.C.KERNEL_MARGIN == 1e-4
    assert (SC.MODEL_B, SC.MODEL_W, SC.MODEL_STEPS) == (2, 4, 8) and (SC.STAT_B, SC.STAT_V) == (512, 6)
    core = open(os.path.join(CSRC, "vmlmf_beam_core.h")).read()
    lds_v = int(re.search(r"constexpr int BS_LDS_V = (\d+);", core).group(1))
    for B, W, H, V in SC.KERNEL_CASES + [(SC.STAT_B, 1, SC.STAT_H, SC.STAT_V), (SC.STAT_B, 2, SC.STAT_H, SC.STAT_V)]:
        assert _sbeam.check_sbeam(W, V) == W                                      # the binding takes every case
    assert [V > lds_v for _, _, _, V in SC.KERNEL_CASES] == [False, False, False, True, False]   # one case re-reads its scores
    assert any(W * W == 1024 for _, W, _, _ in SC.KERNEL_CASES) and any(W == 1 for _, W, _, _ in SC.KERNEL_CASES)


@pytest.mark.parametrize("draw", SC.DRAWS)
@pytest.mark.parametrize("variant", SC.VARIANTS)
@pytest.mark.parametrize("case", SC.KERNEL_CASES, ids=SC.case_id)
def test_every_row_is_clear_and_no_child_exceeds_its_parent(case, variant, draw):
    B, W, H, V = case
    h, w, b, cum, fin, length, T = SC.kernel_case(case, variant)
    if variant == "finished":
        assert fin.any() and not fin.all()
    if variant == "first":
        assert cum[:, 0].eq(0).all() and T[:, 0].eq(0).all() and torch.isinf(cum[:, 1:]).all() and torch.isinf(T[:, 1:]).all()
    rows = SC.kernel_oracle(case, variant, draw)
    assert len(rows) == B
    for r, (phi, gt, G, valid, m, top, lo, hi) in enumerate(rows):
        assert lo == hi == set(top.tolist()) and len(top) == W, (case, variant, draw, r)     # clear at every candidate's margin
        Tr = T[r].double().numpy()
        assert (m >= SC.C.KERNEL_MARGIN).all()
        for wi in range(W):
            live = valid[wi]
            assert (G[wi][live] <= Tr[wi]).all()                                        # no child exceeds its parent
            if np.isfinite(Tr[wi]) and np.isfinite(float(cum[r, wi])):
                assert G[wi][live].max() == Tr[wi]                                      # the largest child inherits it, exactly
                if not fin[r, wi]:
                    assert G[wi].argmax() == gt[wi].argmax()
            else:
                assert np.isneginf(G[wi][live]).all()
        best = G.ravel()[top]
        assert (best[:-1] >= best[1:]).all() and best[0] == Tr.max()


@pytest.mark.parametrize("draw", SC.DRAWS)
@pytest.mark.parametrize("case", SC.DEEP_CASES, ids=SC.case_id)
def test_deep_in_a_search_the_survivors_are_the_beams_largest_children(case, draw):
    """Totals 25 below the values, as after eight steps: exp(T - Z) is about e^25, every child but a beam's largest lands near its own
    gt - far below every T -, so a row's survivors are its beams' largest children at their parents' values."""
    B, W, H, V = case
    T = SC.deep_case(case)[6].double().numpy()
    clear = 0
    for r, (phi, G, valid, G_lo, G_hi, top, lo, hi) in enumerate(SC.deep_oracle(case, draw)):
        assert sorted(f // V for f in top) == list(range(W))                              # one child of every beam ...
        assert np.array_equal(G.ravel()[top], np.sort(T[r])[::-1])                        # ... at its parent's value, in order
        assert (G_lo <= G)[valid].all() and (G <= G_hi)[valid].all()
        rest = np.setdiff1d(np.flatnonzero(valid.ravel()), top)
        assert G_hi.ravel()[rest].max() < T[r].min() - 10 or lo != hi                      # the others far below, or a maximum in doubt
        clear += lo == hi
    assert clear >= B - 1


def test_another_draw_and_another_seed_give_other_noise():
    B, W, H, V = SC.BASIC
    a, b, c = SC.noise(B, W, V, 0), SC.noise(B, W, V, 5), SC.noise(B, W, V, 0, seed=SC.NOISE_SEED + 1)
    assert not np.array_equal(a, b) and not np.array_equal(a, c)
    # W = 1: the sampler's noise of (step B + b, v)
    assert np.array_equal(SC.noise(2, 1, V, 3), SC.C.gumbel_restated(SC.NOISE_SEED, SC.NOISE_OFFSET, 3, 2, V)[1].reshape(2, 1, V))
    # ... and beam w of row b at position draw B W + b W + w: the rows of a later draw continue those of the flattened batch
    wide = SC.C.gumbel_restated(SC.NOISE_SEED, SC.NOISE_OFFSET, 0, 2 * B * W, V)[1]
    assert np.array_equal(SC.noise(B, W, V, 1).reshape(B * W, V), wide[B * W:])


@pytest.mark.parametrize("W", [1, 2])
def test_the_first_tokens_are_a_sample_without_replacement(W):
    p, rows = SC.stat_oracle(W)
    assert len(rows) == SC.STAT_B and abs(p.sum() - 1) < 1e-12 and (SC.STAT_B * p).min() > 5
    tokens = []
    for phi, gt, G, valid, m, top, lo, hi in rows:
        assert lo == hi == set(top.tolist()) and SC.in_order(G, m, top)                 # what the device is compared with is clear
        assert all(f // SC.STAT_V == 0 for f in top)                                    # the first step: every survivor from beam 0
        tokens.append([int(f) % SC.STAT_V for f in top])
    tokens = np.array(tokens)
    assert all(len(set(t)) == W for t in tokens.tolist())
    stat, df = SC.stat_statistic(W, tokens)
    assert df == (SC.STAT_V - 1 if W == 1 else SC.STAT_V * (SC.STAT_V - 1) - 1)
    assert stat < SC.CHI2_999[df], (W, stat)
    # the statistic tells a wrong sampler apart: the same rows without the noise (beam search) fail it by far
    greedy = np.tile(np.argsort(-p)[:W], (SC.STAT_B, 1))
    assert SC.stat_statistic(W, greedy)[0] > 10 * SC.CHI2_999[df]


def test_the_conditional_transform_of_the_reference():
    T, Z = np.array([[0.7]]), np.array([[1.9]])
    gt = np.array([[1.9, 1.0, -3.0, -np.inf]])
    G = SC.conditional(T, Z, gt)
    assert G[0, 0] == 0.7 and np.isneginf(G[0, 3]) and (np.diff(G[0]) < 0).all()
    # -log(exp(-T) - exp(-Z) + exp(-gt)): the textbook form of the same value
    assert np.allclose(G[0, 1:3], -np.log(np.exp(-T) - np.exp(-Z) + np.exp(-gt[:, 1:3]))[0], rtol=0, atol=1e-12)
    assert np.isneginf(SC.conditional(np.array([[-np.inf]]), np.array([[-np.inf]]), np.array([[-np.inf, -np.inf]]))).all()


# ---- the refusals ----
def test_stochastic_beam_search_refuses_before_any_device_work():
    from vmlmf_amd import Model, StochasticBeams, lm_sbeam_step
    m = Model(97, 16, 2, 0.0, 0.1, w_rank=8, u_ranks=[8], lstm_type="vmlmf")
    prompt = torch.zeros((3, 2), dtype=torch.int64)
    for kw, word in ((dict(beams=0), "beams"), (dict(beams=33), "beams"), (dict(beams=98), "beams"), (dict(eos=97), "eos"),
                     (dict(eos=-1), "eos"), (dict(chunk=3), "chunk"), (dict(chunk=0), "chunk")):
        with pytest.raises(ValueError, match=word):
            m.stochastic_beam_search(prompt, 4, **kw)
    with pytest.raises(ValueError, match="steps"):
        m.stochastic_beam_search(prompt, -1)
    with pytest.raises(RuntimeError, match="cuda"):                           # CPU tensors raise as in beam_search
        m.stochastic_beam_search(prompt, 4)
    with pytest.raises(RuntimeError, match="cuda"):
        m.stochastic_beam_search(prompt, 8, 6, seed=3, eos=3, chunk=4)
    for kw in (dict(temperature=0.7), dict(min_length=2), dict(top_k=5), dict(automaton=None), dict(length_penalty=1.0)):
        with pytest.raises(TypeError):                                        # no temperature, controls or automaton here
            m.stochastic_beam_search(prompt, 4, **kw)
    with pytest.raises(TypeError):
        m.stochastic_beam_search(prompt, 4, 4, 7)                             # everything behind beams is keyword-only
    for args in ((2, 0, 97, "cpu"), (2, 33, 97, "cpu"), (2, 8, 4, "cpu"), (0, 4, 97, "cpu")):
        with pytest.raises(ValueError):
            StochasticBeams(*args)
    s = StochasticBeams(2, 4, 97, "cpu")
    assert (s.B, s.W, s.V) == (2, 4, 97)
    cum, fin, ln, pert, draw = s.start()
    assert cum.tolist() == pert.tolist() == [[0.0, -math.inf, -math.inf, -math.inf]] * 2 and cum.data_ptr() != pert.data_ptr()
    assert fin.dtype == ln.dtype == draw.dtype == torch.int32 and not fin.any() and not ln.any() and fin.shape == ln.shape == (2, 4)
    assert draw.tolist() == [0, 0]
    with pytest.raises(RuntimeError, match="HIP device"):
        lm_sbeam_step(torch.zeros(8, 16), torch.zeros(97, 16), None, cum, fin, ln, pert, draw, torch.zeros(2, dtype=torch.int64), 3)


def test_the_entry_point_refuses_bad_arguments_without_touching_the_gpu():
    from vmlmf_amd import _lib, _sbeam
    lib = _sbeam.lib()
    one, out, two, out2 = ctypes.c_void_p(16), ctypes.c_void_p(32), ctypes.c_void_p(48), ctypes.c_void_p(64)   # never dereferenced
    three, out3 = ctypes.c_void_p(80), ctypes.c_void_p(96)

    def step(B=2, W=4, H=32, V=97, eos=7, ws=2 * 4 * 4 * 12, scores=one, embed=one, x_next=out, total=out, cum=one, workspace=one,
             perturbed=two, perturbed_out=out2, draw=three, draw_out=out3, state=one):
        return lib.vmlmf_sbeam_step(B, W, H, V, scores, one, cum, one, one, eos, embed, out, out, total, out, out, x_next, out, one,
                                    workspace, ws, perturbed, perturbed_out, draw, draw_out, state, None)

    for kw, word in ((dict(B=0), b">= 1"), (dict(W=0), b"beams"), (dict(W=33), b"beams"), (dict(W=4, V=3, eos=-1), b"exceed V"),
                     (dict(eos=97), b"eos"), (dict(eos=-2), b"eos"), (dict(scores=None), b"null"), (dict(embed=None), b"together"),
                     (dict(x_next=None), b"together"), (dict(total=one, cum=one), b"alias"), (dict(workspace=ctypes.c_void_p(12)), b"aligned"),
                     (dict(W=32, V=2 ** 26, eos=-1), b"2\\^31"),
                     (dict(perturbed=None), b"null"), (dict(perturbed_out=None), b"null"), (dict(draw=None), b"null"),
                     (dict(draw_out=None), b"null"), (dict(state=None), b"null"),
                     (dict(perturbed_out=two), b"alias"), (dict(draw_out=three), b"alias"), (dict(perturbed_out=one), b"alias"),
                     (dict(total=two), b"alias"), (dict(perturbed_out=out), b"alias")):
        assert step(**kw) == _lib.E_BADARG, kw
        err = lib.vmlmf_sbeam_last_error()
        assert re.search(word, err) and err.startswith(b"vmlmf_sbeam_step: "), (kw, err)
    for ws in (2 * 4 * 4 * 12 - 1, 2 * 4 * 4 * 8, 2 * 4 * 4 * 8 - 1):          # the plain step's workspace is not enough
        assert step(ws=ws) == _lib.E_WORKSPACE and b"vmlmf_sbeam_workspace_bytes" in lib.vmlmf_sbeam_last_error()
    with pytest.raises(_lib.VmlmfError) as ei:
        _sbeam.check(step(state=None))
    assert ei.value.code == _lib.E_BADARG and "null" in str(ei.value)


def test_workspace_bytes():
    from vmlmf_amd import _beam, _sbeam
    ws = _sbeam.lib().vmlmf_sbeam_workspace_bytes
    assert ws(2, 4, 97) == 2 * 4 * 4 * 12 and ws(1, 1, 10000) == 12 and ws(32, 32, 10000) == 32 * 32 * 32 * 12
    assert ws(1, 16, 10 ** 8) == 16 * 16 * 12
    for bad in ((0, 4, 97), (2, 0, 97), (2, 33, 97), (2, 4, 3), (2, 4, 0), (1, 32, 2 ** 26)):
        assert ws(*bad) == 0, bad
    for shape in ((2, 4, 97), (3, 6, 1000), (1, 32, 64)):                     # the plain step's keys and an fp32 total beside each
        assert ws(*shape) * 8 == _beam.lib().vmlmf_beam_workspace_bytes(*shape) * 12 and ws(*shape) % 4 == 0


# ---- what the package exports ----
def test_the_package_exports_the_stochastic_beams():
    import vmlmf_amd
    from vmlmf_amd import _sbeam as b
    from vmlmf_amd import decoding
    names = ["StochasticBeams", "StochasticBeamGraph", "lm_sbeam_step"]
    at = vmlmf_amd.__all__.index("NeuralCache")
    assert vmlmf_amd.__all__[at - 3:at] == names and vmlmf_amd.__all__[-2:] == ["NeuralCache", "lm_cache_score"]
    for name in names:
        assert getattr(vmlmf_amd, name) is getattr(decoding, name)
    assert vmlmf_amd.StochasticBeams is b.StochasticBeams and vmlmf_amd.lm_sbeam_step is b.lm_sbeam_step
    assert issubclass(decoding.StochasticBeamGraph, decoding._StepGraph)
    assert callable(decoding.stochastic_beam_search) and callable(vmlmf_amd.Model.stochastic_beam_search)
    assert callable(b.check_sbeam) and b.check_sbeam(4, 97) == 4


def test_stochastic_beams_are_a_policy_of_the_one_beam_loop():
    """No second loop, graph or buffer cache: StochasticBeams goes through beam_steps / BeamGraph as the other policies do."""
    from vmlmf_amd import StochasticBeams, _beam, _sbeam as b, decoding
    assert issubclass(decoding.StochasticBeamGraph, decoding.BeamGraph) and issubclass(StochasticBeams, _beam.BeamPolicy)
    assert StochasticBeams.carried == ("perturbed", "draw")
    s = StochasticBeams(2, 4, 97, "cpu")
    first, start = s.first_carried(), s.start()
    assert len(first) == 2 and len(start) == 5 and all(torch.equal(x, y) and x.dtype == y.dtype for x, y in zip(first, start[3:]))
    assert all(torch.equal(x, y) and x.dtype == y.dtype for x, y in zip(s.first_beams(), start[:3]))
    assert not hasattr(decoding, "sbeam_steps") and not hasattr(decoding, "_sbeamed") and not hasattr(b, "_BUFFERS")
    assert s.state is None
    was = b.loaded()
    cum, fin, ln, pert, draw = start
    with pytest.raises(RuntimeError, match="state"):          # refused before any library is opened
        s.select(torch.zeros(8, 97), None, cum, fin, ln, -1, None, perturbed=pert, draw=draw)
    assert b.loaded() == was


def test_the_kernel_takes_the_selection_and_the_noise_from_the_shared_headers():
    text = open(os.path.join(CSRC, "vmlmf_sbeam.hip")).read()
    for header in ("vmlmf_beam_core.h", "vmlmf_select.h", "vmlmf_side.h", "../../include/vmlmf_sbeam.h"):
        assert '#include "%s"' % header in text, header
    for fn in ("key_of", "total_of", "index_of", "wg_max", "step_args", "step_workspace_bytes", "philox4x32_10", "gumbel_of", "sample_key"):
        assert re.search(r"\b%s\s*\(" % fn, text), fn                                     # it calls them ...
    for fn in ("key_of", "total_of", "index_of", "row_max", "wave_max", "wg_max", "step_sizes", "step_args", "philox4x32_10", "gumbel_of",
               "gumbel", "sample_key"):
        assert not re.search(r"(__device__|inline|static)[^;{]*\b%s\s*\(" % fn, text), fn   # ... and holds no copy
    assert "BeamScratch" in text and "struct BeamScratch" not in text
    assert len(re.findall(r"__global__", text)) == 1 and "asm" not in text.replace("no inline assembly", "") and "atomicAdd" not in text
    assert "VMLMF_SIDE_LIBRARY(vmlmf_sbeam, VMLMF_SBEAM_ABI_VERSION)" in text


# ---- the signatures ----
def test_the_signatures():
    from vmlmf_amd import Model, StochasticBeamGraph, StochasticBeams, _sbeam, decoding, lm_sbeam_step
    for fn, lead in ((Model.stochastic_beam_search, ["self"]), (decoding.stochastic_beam_search, ["model"])):
        ps = inspect.signature(fn).parameters
        assert list(ps) == lead + ["prompt", "steps", "beams", "seed", "states", "eos", "chunk"]
        for name in lead + ["prompt", "steps", "beams"]:
            assert ps[name].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
        for name in ("seed", "states", "eos", "chunk"):
            assert ps[name].kind is inspect.Parameter.KEYWORD_ONLY
        got = {k: p.default for k, p in ps.items() if p.default is not inspect.Parameter.empty}
        assert got == dict(beams=4, seed=None, states=None, eos=None, chunk=None)
    ps = inspect.signature(lm_sbeam_step).parameters
    assert list(ps) == ["h", "weight", "bias", "cum", "finished", "length", "perturbed", "draw", "state", "eos", "embed", "buffers"]
    assert ps["embed"].default is None and ps["buffers"].default is None and ps["eos"].default is inspect.Parameter.empty
    assert list(inspect.signature(_sbeam.check_sbeam).parameters) == ["beams", "V"]
    assert list(inspect.signature(StochasticBeams.__init__).parameters) == ["self", "B", "W", "V", "device"]
    assert list(inspect.signature(StochasticBeamGraph.__init__).parameters)[:7] == ["self", "model", "h", "states", "steps", "beams", "state"]
    assert list(inspect.signature(StochasticBeamGraph.__init__).parameters) == [
        "self", "model", "h", "states", "steps", "beams", "state", "eos", "cum", "finished", "length", "perturbed", "draw"]
    assert list(inspect.signature(StochasticBeams.select).parameters) == [
        "self", "scores", "bias", "cum", "finished", "length", "eos", "embed", "buffers", "perturbed", "draw"]
    doc = Model.stochastic_beam_search.__doc__
    for word in ("without replacement", "perturbed", "no temperature", "chunk=K", "Kool"):
        assert word in doc, word
    # the existing decoders keep theirs
    from vmlmf_amd import BeamGraph, lm_beam_step
    assert list(inspect.signature(lm_beam_step).parameters)[:9] == ["h", "weight", "bias", "cum", "finished", "length", "eos", "embed", "buffers"]
    assert list(inspect.signature(decoding.beam_steps).parameters)[:9] == ["model", "h", "states", "cum", "finished", "length", "steps", "eos", "buffers"]
    assert list(inspect.signature(BeamGraph.__init__).parameters)[:7] == ["self", "model", "h", "states", "steps", "beams", "eos"]
    assert list(inspect.signature(Model.beam_search).parameters)[:5] == ["self", "prompt", "steps", "beams", "states"]
