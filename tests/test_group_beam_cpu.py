"""Model.group_beam_search and libvmlmf_beamgroup.so without a GPU: the kernel-level cases of group_beam_cases.py are all clear in the
fp64 reference and the penalty decides where the groups share their inputs; the refusals, from Python and from the C entry point; the
workspace; what the package exports; the signature.  Header, SYMBOLS, exports, ABI number, Makefile and lazy loading:
test_side_libraries_cpu.py's table."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import group_beam_cases as GC


# ---- the cases ----
def test_the_cases_are_the_prescribed_ones():
    assert GC.KERNEL_CASES == [(1, 4, 2, 16, 97, 0.5), (3, 6, 3, 16, 1000, 1.0), (2, 8, 8, 16, 300, 0.7), (1, 32, 2, 8, 64, 0.5),
                               (1, 32, 32, 8, 64, 0.5), (2, 4, 2, 8, 12293, 0.5), (1, 4, 2, 16, 97, 1e4)]
    assert len(GC.SHARED) >= 4 and all(c in GC.KERNEL_CASES for c in GC.SHARED)
    assert GC.VARIANTS == ["base", "finished", "neginf"]


@pytest.mark.parametrize("variant", GC.VARIANTS)
@pytest.mark.parametrize("case", GC.KERNEL_CASES, ids=GC.case_id)
def test_every_group_of_every_row_is_clear(case, variant):
    B, W, G, H, V, lam = case
    Wg = W // G
    h, w, b, cum, fin, length = GC.kernel_case(case, variant)
    if variant == "finished":
        assert fin[:, Wg - 1].all() and not fin.all()
    if variant == "neginf" and Wg > 1:
        assert torch.isinf(cum).sum() == B * (W - G)
    if case in GC.SHARED:
        for g in range(1, G):
            assert torch.equal(h.view(B, G, Wg, H)[:, g], h.view(B, G, Wg, H)[:, 0])
            assert torch.equal(cum.view(B, G, Wg)[:, g], cum.view(B, G, Wg)[:, 0])
    rows = GC.kernel_oracle(case, variant)
    assert len(rows) == B
    for totals, groups in rows:
        assert len(groups) == G
        for g, (aug, valid, top, lo, hi) in enumerate(groups):
            assert lo == hi == set(top.tolist()) and len(top) == Wg, (case, variant, g)
            assert all(g * Wg <= f // V < (g + 1) * Wg for f in top)          # a group keeps its own beams' candidates
            assert (aug <= totals)[valid].all()
            assert GC.in_order(aug, top, GC.C.KERNEL_MARGIN), (case, variant, g)  # ... and their order is as clear as their set


@pytest.mark.parametrize("variant", ["base", "neginf"])
@pytest.mark.parametrize("case", GC.SHARED, ids=GC.case_id)
def test_the_penalty_decides_where_the_groups_share_their_inputs(case, variant):
    B, W, G, H, V, lam = case
    Wg = W // G
    with_pen, without = GC.chosen(GC.kernel_oracle(case, variant)), GC.chosen(GC.kernel_oracle(case, variant, 0.0))
    assert not np.array_equal(with_pen, without)
    # without a penalty the groups are identical: the same tokens from the same beams of each group
    local = without.reshape(B, G, Wg) - (np.arange(G) * Wg * V)[None, :, None]
    assert (local == local[:, :1]).all()
    assert np.array_equal(with_pen[:, :Wg], without[:, :Wg])                  # group 0 is never penalised
    if lam >= 1e3:                                                            # a closing penalty: no live token comes twice in a row
        for r in range(B):
            toks = (with_pen[r] % V).tolist()
            assert len(set(toks)) == W


def test_the_reference_does_not_count_a_finished_beams_eos():
    V, W, G = 12, 4, 2
    x = np.zeros((W, V))
    x[:, GC.EOS] = 5.0                                                       # eos is every live beam's best token
    x[:, 3] = 4.0
    cum = np.array([0.0, -1.0, 0.0, -1.0])
    totals, groups = GC.group_step(x, cum, np.array([True, False, False, False]), GC.EOS, W, G, 100.0, 1e-4)
    # group 0: finished beam 0's padding eos (at cum 0) and live beam 1's eos: ONE choice of eos
    assert groups[0][2].tolist() == [0 * V + GC.EOS, 1 * V + GC.EOS]
    # group 1 is penalised once for eos, not twice: aug of (2, eos) is total - 100
    assert groups[1][0][2, GC.EOS] == totals[2, GC.EOS] - 100.0
    assert groups[1][2].tolist() == [2 * V + 3, 3 * V + 3]


# ---- the refusals ----
def test_group_beam_search_refuses_before_any_device_work():
    from vmlmf_amd import GroupBeams, Model, _beamgroup
    m = Model(97, 32, 2, 0.0, 0.1, w_rank=8, u_ranks=[8], lstm_type="vmlmf")
    prompt = torch.zeros((3, 2), dtype=torch.int64)
    for kw, word in ((dict(groups=0), "groups"), (dict(groups=-2), "groups"), (dict(beams=4, groups=3), "divide"),
                     (dict(beams=6, groups=4), "divide"), (dict(diversity_penalty=-0.5), "diversity_penalty"),
                     (dict(diversity_penalty=float("inf")), "diversity_penalty"), (dict(diversity_penalty=float("nan")), "diversity_penalty"),
                     (dict(beams=0), "beams"), (dict(beams=33), "beams"), (dict(beams=98), "beams"), (dict(eos=97), "eos"),
                     (dict(chunk=3), "chunk"), (dict(length_penalty=-1.0), "length_penalty")):
        with pytest.raises(ValueError, match=word):
            m.group_beam_search(prompt, 4, **kw)
    with pytest.raises(ValueError, match="steps"):
        m.group_beam_search(prompt, -1)
    with pytest.raises(RuntimeError, match="cuda"):                           # CPU tensors raise as in beam_search
        m.group_beam_search(prompt, 4)
    with pytest.raises(TypeError):                                            # no controls, no automaton here
        m.group_beam_search(prompt, 4, min_length=2)
    with pytest.raises(TypeError):
        m.group_beam_search(prompt, 4, 4, 2)                                  # everything behind beams is keyword-only
    for args in ((2, 4, 97, "cpu", 3, 0.5), (2, 4, 97, "cpu", 0, 0.5), (2, 4, 97, "cpu", 2, -1.0), (2, 4, 97, "cpu", 2, float("nan")),
                 (2, 33, 97, "cpu", 1, 0.5), (2, 8, 4, "cpu", 2, 0.5)):
        with pytest.raises(ValueError):
            GroupBeams(*args)
    c = GroupBeams(2, 6, 97, "cpu", groups=3, diversity_penalty=1.5)
    assert (c.B, c.W, c.V, c.groups, c.diversity_penalty) == (2, 6, 97, 3, 1.5)
    assert c.carried == () and c.first_carried() == [] and c.clone() is c
    cum, fin, ln = c.start()
    assert cum.tolist() == [[0.0, -math.inf, 0.0, -math.inf, 0.0, -math.inf]] * 2
    assert fin.dtype == ln.dtype == torch.int32 and not fin.any() and not ln.any() and fin.shape == ln.shape == (2, 6)
    assert _beamgroup.group_start(1, 4, 4, "cpu")[0].tolist() == [[0.0] * 4]
    assert _beamgroup.group_start(1, 4, 1, "cpu")[0].tolist() == [[0.0, -math.inf, -math.inf, -math.inf]]   # beam_search's start


def test_the_entry_point_refuses_bad_arguments_without_touching_the_gpu():
    from vmlmf_amd import _beamgroup, _lib
    lib = _beamgroup.lib()
    one, out = ctypes.c_void_p(16), ctypes.c_void_p(32)                      # never dereferenced: every call below is refused first

    def step(B=2, W=4, H=32, V=97, eos=7, ws=256, scores=one, embed=one, x_next=out, total=out, cum=one, workspace=one, groups=2, lam=0.5):
        return lib.vmlmf_beamgroup_step(B, W, H, V, scores, one, cum, one, one, eos, embed, out, out, total, out, out, x_next, out, one,
                                        workspace, ws, groups, lam, None)

    for kw, word in ((dict(B=0), b">= 1"), (dict(W=0), b"beams"), (dict(W=33), b"beams"), (dict(W=4, V=3, eos=-1), b"exceed V"),
                     (dict(eos=97), b"eos"), (dict(eos=-2), b"eos"), (dict(scores=None), b"null"), (dict(embed=None), b"together"),
                     (dict(x_next=None), b"together"), (dict(total=one, cum=one), b"alias"), (dict(workspace=ctypes.c_void_p(12)), b"aligned"),
                     (dict(W=32, V=2 ** 26, eos=-1), b"2^31"),
                     (dict(groups=0), b"groups must be >= 1"), (dict(groups=-1), b"groups must be >= 1"), (dict(groups=3), b"divide"),
                     (dict(groups=8), b"divide"), (dict(lam=-0.25), b"diversity_penalty"), (dict(lam=float("inf")), b"diversity_penalty"),
                     (dict(lam=float("nan")), b"diversity_penalty")):
        assert step(**kw) == _lib.E_BADARG, kw
        err = lib.vmlmf_beamgroup_last_error()
        assert word in err and err.startswith(b"vmlmf_beamgroup_step: "), (kw, err)
    assert step(ws=255) == _lib.E_WORKSPACE and b"vmlmf_beamgroup_workspace_bytes" in lib.vmlmf_beamgroup_last_error()
    with pytest.raises(_lib.VmlmfError) as ei:
        _beamgroup.check(step(groups=3))
    assert ei.value.code == _lib.E_BADARG and "divide" in str(ei.value)


def test_workspace_bytes():
    from vmlmf_amd import _beam, _beamgroup
    ws = _beamgroup.lib().vmlmf_beamgroup_workspace_bytes
    assert ws(2, 4, 97) == 2 * 4 * 4 * 8 and ws(1, 1, 10000) == 8 and ws(32, 32, 10000) == 32 * 32 * 32 * 8
    assert ws(1, 16, 10 ** 8) == 16 * 16 * 8
    for bad in ((0, 4, 97), (2, 0, 97), (2, 33, 97), (2, 4, 3), (2, 4, 0), (1, 32, 2 ** 26)):
        assert ws(*bad) == 0, bad
    for shape in ((2, 4, 97), (3, 6, 1000), (1, 32, 64)):                     # the plain step's: the buffers are shared
        assert ws(*shape) == _beam.lib().vmlmf_beam_workspace_bytes(*shape)


# ---- what the package exports ----
def test_the_package_exports_the_group_beams():
    import vmlmf_amd
    from vmlmf_amd import _beamgroup as b
    from vmlmf_amd import decoding
    assert "GroupBeams" in vmlmf_amd.__all__ and vmlmf_amd.GroupBeams is decoding.GroupBeams is b.GroupBeams
    assert callable(decoding.group_beam_search) and callable(vmlmf_amd.Model.group_beam_search)


# ---- the signature ----
def test_the_signature_is_keyword_only_behind_beams():
    from vmlmf_amd import Model, decoding
    for fn, lead in ((Model.group_beam_search, ["self"]), (decoding.group_beam_search, ["model"])):
        ps = inspect.signature(fn).parameters
        assert list(ps) == lead + ["prompt", "steps", "beams", "groups", "diversity_penalty", "states", "eos", "length_penalty", "chunk"]
        for name in lead + ["prompt", "steps", "beams"]:
            assert ps[name].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
        for name in ("groups", "diversity_penalty", "states", "eos", "length_penalty", "chunk"):
            assert ps[name].kind is inspect.Parameter.KEYWORD_ONLY
        got = {k: p.default for k, p in ps.items() if p.default is not inspect.Parameter.empty}
        assert got == dict(beams=4, groups=2, diversity_penalty=0.5, states=None, eos=None, length_penalty=0.0, chunk=None)
    # the existing decoders and the step's first nine parameters are what they were
    from vmlmf_amd import lm_beam_step
    assert list(inspect.signature(lm_beam_step).parameters)[:9] == ["h", "weight", "bias", "cum", "finished", "length", "eos", "embed", "buffers"]
