"""Model.contrastive_search and libvmlmf_contrast.so without a GPU: the kernel-level cases of contrast_cases.py are all clear in the
fp64 reference and have the properties their names promise; the refusals, from Python and from the C entry points; the workspace;
header, SYMBOLS, exports and ABI number; the Makefile's `extra` target beside an unchanged `all` and `more`; lazy loading; the
signature."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import contrast_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vmlmf_amd", "csrc")
FUNCTIONS = ["vmlmf_contrast_abi_version", "vmlmf_contrast_append", "vmlmf_contrast_choose", "vmlmf_contrast_last_error",
             "vmlmf_contrast_workspace_bytes"]


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


# ---- header, SYMBOLS, exports, ABI ----
def test_every_declared_function_is_exported_and_bound():
    import vmlmf_amd
    from vmlmf_amd import _contrast as b
    from vmlmf_amd import decoding
    text = open(os.path.join(ROOT, "include", "vmlmf_contrast.h")).read()
    in_header = int(re.search(r"#define VMLMF_CONTRAST_ABI_VERSION (\d+)", text).group(1))
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(vmlmf_[a-z0-9_]+)\s*\(", code))) == sorted(b.SYMBOLS) == FUNCTIONS
    assert os.path.exists(b.LIBRARY.path), "run __graft_entry__.build() first"
    handle = ctypes.CDLL(b.LIBRARY.path)
    for name in FUNCTIONS:
        assert hasattr(handle, name), f"missing export {name}"
    from vmlmf_amd import _automaton, _beam, _beamctl, _beamgroup, _decode, _history, _lib, _score, _truncate
    for other in (_automaton, _beam, _beamctl, _beamgroup, _decode, _history, _lib, _score, _truncate):
        assert not set(other.SYMBOLS) & set(b.SYMBOLS)
        for name in other.SYMBOLS:                                                    # none of the other libraries' entry points
            assert not hasattr(handle, name), name
    assert b.LIBRARY.abi_symbol == "vmlmf_contrast_abi_version" and b.LIBRARY.error_symbol == "vmlmf_contrast_last_error"
    assert in_header == b.ABI_VERSION == b.LIBRARY.abi_version == b.lib().vmlmf_contrast_abi_version() == 1
    assert os.path.basename(b.LIBRARY.path) == "libvmlmf_contrast.so"
    assert "stock-op fallback for the contrastive-search step" in b.LIBRARY.no_fallback
    for name in ("ContrastControls", "ContrastGraph", "lm_contrast_step"):
        assert name in vmlmf_amd.__all__ and getattr(vmlmf_amd, name) is getattr(decoding, name)
    assert vmlmf_amd.ContrastControls is b.ContrastControls and vmlmf_amd.lm_contrast_step is b.lm_contrast_step
    assert issubclass(vmlmf_amd.ContrastGraph, decoding._StepGraph)
    assert callable(decoding.contrastive_search) and callable(vmlmf_amd.Model.contrastive_search)


def test_a_missing_library_is_a_clear_error(monkeypatch, tmp_path):
    from vmlmf_amd import _contrast as b
    monkeypatch.setattr(b.LIBRARY, "_handle", None)
    monkeypatch.setattr(b.LIBRARY, "path", str(tmp_path / "libvmlmf_contrast.so"))
    with pytest.raises(RuntimeError, match="libvmlmf_contrast.so is missing: build it"):
        b.lib()
    with pytest.raises(RuntimeError, match="no stock-op fallback for the contrastive-search step"):
        b.lib()
    assert not b.loaded()


# ---- the Makefile ----
def test_the_makefile_builds_it_by_a_third_target():
    r = subprocess.run(["make", "-n", "-B", "-C", CSRC, "all"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    links = [ln for ln in r.stdout.splitlines() if " -shared " in ln]
    assert len(links) == 8 and "contrast" not in r.stdout                     # `all` is what it was: the main library and seven beside it
    text = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SIDE := beam decode score history beamctl truncate automaton$", text, flags=re.M)
    assert re.search(r"^all: \$\(OUT\) \$\(SIDE_OUT\)$", text, flags=re.M)
    assert re.search(r"^MORE := beamgroup$", text, flags=re.M)
    assert re.search(r"^EXTRA := contrast$", text, flags=re.M) and re.search(r"^extra: \$\(EXTRA_OUT\)$", text, flags=re.M)
    assert re.search(r"^\.PHONY:.*\bmore\b", text, flags=re.M) and re.search(r"^\.PHONY:.*\bextra\b", text, flags=re.M)
    r = subprocess.run(["make", "-n", "-B", "-C", CSRC, "more"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "contrast" not in r.stdout
    assert len([ln for ln in r.stdout.splitlines() if " -shared " in ln]) == 1  # `more` too
    r = subprocess.run(["make", "-n", "-B", "-C", CSRC, "extra"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    links = [ln for ln in r.stdout.splitlines() if " -shared " in ln]
    assert len(links) == 1 and "-o ../lib/libvmlmf_contrast.so" in links[0]
    assert re.findall(r"\bvmlmf_\w+\.o\b", links[0]) == ["vmlmf_contrast.o"]   # linked from its own object alone
    compiles = [ln for ln in r.stdout.splitlines() if " -c " in ln]
    assert len(compiles) == 1 and "vmlmf_contrast.hip" in compiles[0] and "--offload-arch=gfx950" in compiles[0]
    side = [ln for ln in subprocess.run(["make", "-n", "-B", "-C", CSRC, "../lib/libvmlmf_beam.so"], capture_output=True,
                                        text=True, timeout=120).stdout.splitlines() if " -c " in ln or " -shared " in ln]
    strip = lambda ln: ln.replace("contrast", "beam")
    assert [strip(ln) for ln in compiles + links] == side                     # the side libraries' rule and flags
    deps = re.search(r"^vmlmf_contrast\.o:(.*)$", text, flags=re.M).group(1).split()
    source = open(os.path.join(CSRC, "vmlmf_contrast.hip")).read()
    for h in re.findall(r'#include "([^"]+)"', source):                         # rebuilt when a header it includes moves
        assert h in deps, h
    assert "vmlmf_side.h" in deps and "../../include/vmlmf_contrast.h" in deps
    r = subprocess.run(["make", "-n", "-C", CSRC, "clean"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "../lib/libvmlmf_contrast.so" in r.stdout and "vmlmf_contrast.o" in r.stdout
    assert "../lib/libvmlmf_beamgroup.so" in r.stdout and "../lib/libvmlmf_beam.so" in r.stdout
    # build() makes `all`, `more` behind it and `extra` behind that
    lib_py = open(os.path.join(ROOT, "vmlmf_amd", "_lib.py")).read()
    a = lib_py.index('["make", "-C", CSRC, f"-j{jobs}", "all"]')
    m = lib_py.index('["make", "-C", CSRC, f"-j{jobs}", "more"]')
    assert a < m < lib_py.index('["make", "-C", CSRC, f"-j{jobs}", "extra"]')
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert re.search(r"for side in \([^)]*_contrast\)", entry)                   # ... and checks its exports like the others'


# ---- lazy loading ----
WALK = """
import sys; sys.path.insert(0, %r)
import torch, vmlmf_amd
from vmlmf_amd import _contrast, _lib
_lib.lib()
def refused(call):
    try:
        call()
        raise SystemExit('no refusal')
    except RuntimeError as e:
        assert 'cuda' in str(e), e
tok = torch.zeros((3, 2), dtype=torch.int64)
m = vmlmf_amd.Model(97, 8, 1, 0.0, 0.1, w_rank=4, u_ranks=[4], lstm_type='vmlmf')
for call in (lambda: m.generate(tok, 4), lambda: m.beam_search(tok, 4), lambda: m.score(tok), lambda: m.group_beam_search(tok, 4),
             lambda: m.contrastive_search(tok, 4), lambda: m.contrastive_search(tok, 4, 8, 0.3, eos=3, chunk=2, return_penalties=True),
             lambda: m.contrastive_search(tok, 0), lambda: m.contrastive_search(tok, 4, top_k=1, penalty_alpha=0.0, states=None),
             lambda: vmlmf_amd.lm_contrast_step(torch.zeros(8, 8), torch.zeros((2, 4), dtype=torch.int64), torch.zeros(2, 4),
                                                vmlmf_amd.ContrastControls(2, 8, 'cpu', 6)),
             lambda: vmlmf_amd.ContrastControls(2, 8, 'cpu', 6).append(torch.zeros(3, 2, 8))):
    refused(call)
c = vmlmf_amd.ContrastControls(2, 8, 'cpu', 12, top_k=4, penalty_alpha=0.6, eos=3, V=97)
assert c.clone().hist.shape == (2, 12, 8) and c.hist_len.tolist() == [0, 0]
maps = open('/proc/self/maps').read()
assert 'libvmlmf_hip.so' in maps and 'libvmlmf_contrast.so' not in maps and not _contrast.loaded()
_contrast.lib()
maps = open('/proc/self/maps').read()
assert 'libvmlmf_contrast.so' in maps and _contrast.loaded()
mapped = sorted(set(ln.rsplit('/', 1)[-1] for ln in maps.splitlines() if 'libvmlmf_' in ln))
assert mapped == ['libvmlmf_contrast.so', 'libvmlmf_hip.so'], mapped
"""


def test_the_library_is_loaded_by_its_own_first_call_only():
    r = subprocess.run([sys.executable, "-c", WALK % ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


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
