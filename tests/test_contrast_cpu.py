"""Model.contrastive_search and libvmlmf_contrast.so without a GPU: the kernel-level cases of contrast_cases.py are all clear in the
fp64 reference and have the properties their names promise; the refusals, from Python and from the C entry points; the workspace;
what the package exports; the signature.  Header, SYMBOLS, exports, ABI number, Makefile and lazy loading:
test_side_libraries_cpu.py's table."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import contrast_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the cases and the reference ----
def test_the_cases_are_the_prescribed_ones():
    assert CC.KERNEL_CASES == [(1, 4, 16, 5), (3, 5, 100, 63), (2, 16, 8, 64), (1, 1, 16, 65), (2, 8, 650, 257), (4, 2, 64, 1)]
    assert CC.VARIANTS == ["base", "finished", "twin", "alpha0", "alpha1"]
    assert sorted(CC.SEEDS) == sorted(CC.KERNEL_CASES)
    assert CC.bound(650) == (2 * 650 + 16) * 2.0 ** -24 and CC.margin(0.6, 16) == 2 * (0.6 * 48 + 4) * 2.0 ** -24
    for case in CC.KERNEL_CASES:
        assert CC.kernel_case(case)["Tcap"] > case[3]


@pytest.mark.parametrize("variant", CC.VARIANTS)
@pytest.mark.parametrize("case", CC.KERNEL_CASES, ids=CC.case_id)
def test_every_choice_is_clear(case, variant):
    B, k, H, t = case
    c = CC.kernel_case(case, variant)
    assert c["cand_h"].shape == (B * k, H) and c["hist_raw"].shape == (B, t, H) and c["cand_logp"].shape == c["cand_tok"].shape == (B, k)
    assert (np.diff(c["cand_logp"].astype(np.float64), axis=1) <= 0).all()            # most probable first
    assert all(len(set(row)) == k for row in c["cand_tok"].tolist())
    if variant == "finished":
        assert c["finished"][0] == 1 and (B == 1 or c["finished"][1] == 0)
    else:
        assert not c["finished"].any()
    rows = CC.kernel_oracle(case, variant)
    assert len(rows) == B
    for b, (sim, values, j, gap) in enumerate(rows):
        assert gap > CC.margin(c["alpha"], H), (case, variant, b, gap)
        assert (np.abs(sim) <= 1 + 1e-12).all() and 0 <= j < k
        assert all(values[j] > v for i, v in enumerate(values) if i != j)


@pytest.mark.parametrize("case", CC.KERNEL_CASES, ids=CC.case_id)
def test_the_reference_has_the_properties_of_its_variants(case):
    B, k, H, t = case
    for sim, values, j, gap in CC.kernel_oracle(case, "alpha0"):                     # no penalty: the most probable candidate
        assert j == 0
    for sim, values, j, gap in CC.kernel_oracle(case, "alpha1"):                     # nothing but the penalty: the least similar
        assert j == int(np.argmin(sim))
    for (sim, values, j, gap), (sim0, _, j0, _) in zip(CC.kernel_oracle(case, "twin"), CC.kernel_oracle(case, "base")):
        assert abs(sim[CC.TWIN] - 1.0) < 1e-12                                       # a history row up to scale: cosine 1
        assert (sim[1:] == sim0[1:]).all()
        if k > 1:
            assert j != CC.TWIN                                                      # ... and the penalty decides against it
    if k == 1:
        assert all(row[2] == 0 for v in CC.VARIANTS for row in CC.kernel_oracle(case, v))


def test_the_reference_choice_rule():
    assert CC.choose([0.5, 0.7, 0.7])[0] == 1                                         # equal values to the lower j
    assert CC.choose([float("nan"), -3.0])[0] == 1                                    # a NaN loses to every number
    assert CC.choose([float("nan")] * 3) == (0, np.inf)                               # all NaN: 0
    sim, values, j, gap = CC.step(np.zeros((2, 4)), np.log([0.6, 0.4]), np.ones((3, 4)), 0.5)
    assert (sim == 0).all() and j == 0                                                # a zero vector has cosine 0 with everything
    sim, values, j, gap = CC.step(np.ones((2, 4)), np.log([0.6, 0.4]), np.zeros((0, 4)), 0.5)
    assert (sim == 0).all()                                                           # an empty history: 0


# ---- the refusals ----
def _model(V=97, H=16):
    from vmlmf_amd import Model
    return Model(V, H, 2, 0.0, 0.1, w_rank=8, u_ranks=[8], lstm_type="vmlmf")


def test_contrastive_search_refuses_before_any_device_work():
    from vmlmf_amd import ContrastControls, _contrast
    m = _model()
    prompt = torch.zeros((3, 2), dtype=torch.int64)
    for kw, word in ((dict(top_k=0), "top_k"), (dict(top_k=17), "top_k"), (dict(top_k=-1), "top_k"), (dict(penalty_alpha=-0.1), "penalty_alpha"),
                     (dict(penalty_alpha=1.5), "penalty_alpha"), (dict(penalty_alpha=float("nan")), "penalty_alpha"),
                     (dict(penalty_alpha=float("inf")), "penalty_alpha"), (dict(eos=97), "eos"), (dict(eos=-1), "eos"), (dict(chunk=3), "chunk"),
                     (dict(chunk=0), "chunk")):
        with pytest.raises(ValueError, match=word):
            m.contrastive_search(prompt, 4, **kw)
    with pytest.raises(ValueError, match="top_k"):                                    # min(16, V)
        _model(V=12).contrastive_search(prompt, 4, 13)
    with pytest.raises(ValueError, match="T0 >= 1"):
        m.contrastive_search(torch.zeros((0, 2), dtype=torch.int64), 4)
    with pytest.raises(ValueError, match="steps"):
        m.contrastive_search(prompt, -1)
    with pytest.raises(ValueError, match="LDS budget"):                               # 16 * 964 > 14336
        _model(H=964).contrastive_search(prompt, 4, 16)
    with pytest.raises(RuntimeError, match="cuda"):                                   # CPU tensors raise as on the other decoders
        m.contrastive_search(prompt, 4)
    with pytest.raises(RuntimeError, match="cuda"):
        m.contrastive_search(prompt, 4, 16, 1.0, eos=3, chunk=2, return_penalties=True)
    for kw in (dict(min_length=2), dict(top_p=0.9), dict(temperature=0.5), dict(automaton=None), dict(banned_tokens=[1])):
        with pytest.raises(TypeError):                                                # no controls, filters or automata here
            m.contrastive_search(prompt, 4, **kw)
    with pytest.raises(TypeError):
        m.contrastive_search(prompt, 4, 4, 0.6, None)                                 # everything behind penalty_alpha is keyword-only
    for args, kw in (((2, 16, "cpu", 8), dict(top_k=0)), ((2, 16, "cpu", 8), dict(top_k=17)), ((2, 16, "cpu", 8), dict(penalty_alpha=2.0)),
                     ((2, 16, "cpu", 0), {}), ((0, 16, "cpu", 8), {}), ((2, 16, "cpu", 8), dict(eos=97, V=97)),
                     ((2, 16, "cpu", 8), dict(top_k=13, V=12)), ((2, 964, "cpu", 8), dict(top_k=16))):
        with pytest.raises(ValueError):
            ContrastControls(*args, **kw)
    c = ContrastControls(2, 16, "cpu", 9, top_k=5, penalty_alpha=0.25, eos=3, V=97)
    assert (c.B, c.H, c.capacity, c.k, c.alpha, c.eos) == (2, 16, 9, 5, 0.25, 3)
    assert c.hist.shape == (2, 9, 16) and c.hist.dtype == torch.float32
    for t in (c.hist_len, c.finished, c.length, c.ticket):
        assert t.dtype == torch.int32 and t.tolist() == [0, 0]
    assert c.workspace.numel() * 4 == _contrast.workspace_bytes(2) == _contrast.lib().vmlmf_contrast_workspace_bytes(2, 5, 16, 9)
    d = c.clone()
    assert d.hist.data_ptr() != c.hist.data_ptr() and d.hist_len.data_ptr() != c.hist_len.data_ptr() and (d.k, d.alpha, d.eos) == (5, 0.25, 3)
    assert ContrastControls(1, 8, "cpu", 4).eos == -1
    assert _contrast.check_contrast(16, 1.0, 97, 896) == (16, 1.0) and _contrast.check_contrast(4, 0, 10000, 650) == (4, 0.0)


def test_the_entry_points_refuse_bad_arguments_without_touching_the_gpu():
    from vmlmf_amd import _contrast, _lib
    lib = _contrast.lib()
    one, out = ctypes.c_void_p(64), ctypes.c_void_p(128)                      # never dereferenced: every call below is refused first

    def choose(B=2, k=4, H=16, Tcap=9, alpha=0.6, eos=3, ws=2 * 64 * 16 * 4, parts=0, cand_h=one, hist=out, sim=out, workspace=out):
        return lib.vmlmf_contrast_choose(B, k, H, Tcap, cand_h, one, one, alpha, eos, hist, out, out, out, out, out, out, sim, out, out, out,
                                         workspace, ws, parts, None)

    for kw, word in ((dict(B=0), b">= 1"), (dict(H=0), b">= 1"), (dict(Tcap=0), b">= 1"), (dict(k=0), b"candidates"), (dict(k=17), b"candidates"),
                     (dict(k=16, H=961), b"LDS"), (dict(k=4, H=3841), b"LDS"), (dict(alpha=-0.1), b"alpha"), (dict(alpha=1.01), b"alpha"),
                     (dict(alpha=float("nan")), b"alpha"), (dict(eos=-2), b"eos"), (dict(parts=-1), b"parts"), (dict(parts=65), b"parts"),
                     (dict(cand_h=None), b"null"), (dict(sim=None), b"null"), (dict(workspace=None), b"null"),
                     (dict(hist=ctypes.c_void_p(136)), b"16-byte"), (dict(workspace=ctypes.c_void_p(130)), b"4-byte"),
                     (dict(B=2 ** 25), b"2\\^25"), (dict(B=2 ** 20, Tcap=2 ** 11), b"2\\^31")):
        assert choose(**kw) == _lib.E_BADARG, kw
        err = lib.vmlmf_contrast_last_error()
        assert re.search(word, err) and err.startswith(b"vmlmf_contrast_choose: "), (kw, err)
    assert choose(ws=2 * 64 * 16 * 4 - 1) == _lib.E_WORKSPACE and b"vmlmf_contrast_workspace_bytes" in lib.vmlmf_contrast_last_error()

    def append(B=2, T=3, H=16, Tcap=9, h=one, hist=out, hist_len=out):
        return lib.vmlmf_contrast_append(B, T, H, h, hist, hist_len, Tcap, None)

    for kw in (dict(B=0), dict(T=0), dict(H=0), dict(Tcap=0), dict(h=None), dict(hist=None), dict(hist_len=None), dict(B=2 ** 20, Tcap=2 ** 11)):
        assert append(**kw) == _lib.E_BADARG, kw
        assert lib.vmlmf_contrast_last_error().startswith(b"vmlmf_contrast_append: ")
    with pytest.raises(_lib.VmlmfError) as ei:
        _contrast.check(choose(k=17))
    assert ei.value.code == _lib.E_BADARG and "candidates" in str(ei.value)


def test_workspace_bytes():
    from vmlmf_amd import _contrast
    ws = _contrast.lib().vmlmf_contrast_workspace_bytes
    assert ws(1, 4, 650, 200) == 64 * 16 * 4 and ws(32, 16, 650, 1000) == 32 * 64 * 16 * 4 == _contrast.workspace_bytes(32)
    for bad in ((0, 4, 16, 8), (2, 0, 16, 8), (2, 17, 16, 8), (2, 4, 0, 8), (2, 4, 16, 0), (2, 16, 961, 8)):
        assert ws(*bad) == 0, bad
    assert (_contrast.MAX_K, _contrast.MAX_PARTS, _contrast.LDS_FLOATS) == (16, 64, 14336)
    text = open(os.path.join(ROOT, "include", "vmlmf_contrast.h")).read()
    for name, value in (("MAX_K", 16), ("MAX_PARTS", 64), ("LDS_FLOATS", 14336)):   # the Python side mirrors the header's limits
        assert int(re.search(r"#define VMLMF_CONTRAST_%s (\d+)" % name, text).group(1)) == value


# ---- what the package exports ----
def test_the_package_exports_the_contrast_controls():
    import vmlmf_amd
    from vmlmf_amd import _contrast as b
    from vmlmf_amd import decoding
    for name in ("ContrastControls", "ContrastGraph", "lm_contrast_step"):
        assert name in vmlmf_amd.__all__ and getattr(vmlmf_amd, name) is getattr(decoding, name)
    assert vmlmf_amd.ContrastControls is b.ContrastControls and vmlmf_amd.lm_contrast_step is b.lm_contrast_step
    assert issubclass(vmlmf_amd.ContrastGraph, decoding._StepGraph)
    assert callable(decoding.contrastive_search) and callable(vmlmf_amd.Model.contrastive_search)


# ---- the signature ----
def test_the_signature():
    from vmlmf_amd import Model, decoding
    for fn, lead in ((Model.contrastive_search, ["self"]), (decoding.contrastive_search, ["model"])):
        ps = inspect.signature(fn).parameters
        assert list(ps) == lead + ["prompt", "steps", "top_k", "penalty_alpha", "states", "eos", "chunk", "return_penalties"]
        for name in lead + ["prompt", "steps", "top_k", "penalty_alpha"]:
            assert ps[name].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
        for name in ("states", "eos", "chunk", "return_penalties"):
            assert ps[name].kind is inspect.Parameter.KEYWORD_ONLY
        got = {k: p.default for k, p in ps.items() if p.default is not inspect.Parameter.empty}
        assert got == dict(top_k=4, penalty_alpha=0.6, states=None, eos=None, chunk=None, return_penalties=False)
    ps = inspect.signature(decoding.lm_contrast_step).parameters
    assert list(ps) == ["cand_h", "cand_tok", "cand_logp", "controls", "parts"] and ps["parts"].default == 0
