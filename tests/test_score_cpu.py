"""Model.score and lm_score (C ABI vmlmf_score_rows in libvmlmf_score.so, include/vmlmf_score.h): what can be checked without a GPU -
the numpy oracle that the GPU tests (test_gpu_score.py) hold the kernel to, checked on itself; every refusal, in Python and at the C
ABI; the library, its binding, its lazy load and its place in the Makefile.

The contract, per row, on x = bias + scores in fp32: the tokens' ORDER is larger x first, equal x to the lower index;
logprob = x[y] - logsumexp(x); rank = how many tokens are ahead of y in the order; the top tokens are the order's first `top`."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def score_oracle(scores_f32, bias_f32, targets, top):
    """scores (R, V) fp32, bias (V) fp32 or None, targets (R) integers (< 0: no target) or None, top in [0, V].  x is formed by the fp32
    add, the order by np.lexsort on (x descending, index ascending), the log-probabilities in fp64 from x.  Returns (logprob (R) f64,
    rank (R) int64, top_tokens (R, top) int64, top_logprob (R, top) f64, order (R, V)); a row without a target has (0.0, -1)."""
    s = np.asarray(scores_f32, dtype=np.float32)
    x = s + (np.float32(0) if bias_f32 is None else np.asarray(bias_f32, dtype=np.float32)[None, :])
    assert x.dtype == np.float32
    R, V = x.shape
    y = np.full(R, -1, dtype=np.int64) if targets is None else np.asarray(targets, dtype=np.int64)
    x64 = x.astype(np.float64)
    m = x64.max(1)
    lse = m + np.log(np.exp(x64 - m[:, None]).sum(1))
    order = np.stack([np.lexsort((np.arange(V), -x[r])) for r in range(R)])
    place = np.empty_like(order)
    np.put_along_axis(place, order, np.broadcast_to(np.arange(V), (R, V)), 1)      # place[r, v]: how many tokens are ahead of v
    has = y >= 0
    yc = np.where(has, y, 0)
    rows = np.arange(R)
    logprob = np.where(has, x64[rows, yc] - lse, 0.0)
    rank = np.where(has, place[rows, yc], -1)
    top_tokens = order[:, :top].astype(np.int64)
    top_logprob = np.take_along_axis(x64, top_tokens, 1) - lse[:, None]
    return logprob, rank, top_tokens, top_logprob, order


# ---- the oracle on itself ----
def test_all_equal_scores_rank_by_index():
    V = 7
    lp, rank, toks, tlp, _ = score_oracle(np.full((V, V), 0.25, np.float32), None, np.arange(V), 3)
    assert rank.tolist() == list(range(V))                           # equal scores: the lower index first
    assert np.allclose(lp, -np.log(V), atol=1e-15) and np.allclose(tlp, -np.log(V), atol=1e-15)
    assert (toks == np.array([0, 1, 2])).all()


def test_a_tie_group_across_the_cut_and_tied_targets():
    x = np.array([[1, 3, 3, 3, 0, 3, 5]], np.float32).repeat(5, 0)
    y = [6, 4, 1, 5, 0]                                              # first, last, head and tail of the tie group, below it
    lp, rank, toks, tlp, order = score_oracle(x, None, y, 3)
    assert order[0].tolist() == [6, 1, 2, 3, 5, 0, 4]
    assert rank.tolist() == [0, 6, 1, 4, 5]
    assert (toks == np.array([6, 1, 2])).all()                       # the cut admits the tie group's lower indices
    lse = np.log(np.exp([1.0, 3, 3, 3, 0, 3, 5]).sum())
    assert np.allclose(lp, np.array([5.0, 0, 3, 3, 1]) - lse, atol=1e-14)
    assert np.allclose(tlp[0], np.array([5.0, 3, 3]) - lse, atol=1e-14)
    assert np.isclose(np.exp(score_oracle(x, None, None, 7)[3][0]).sum(), 1.0)


def test_the_bias_is_added_in_fp32_and_a_negative_target_is_no_target():
    s = np.array([[1.0, 1.0 + 2.0 ** -23, 0.5]], np.float32)
    b = np.array([2.0 ** -24, -(2.0 ** -24), 0.0], np.float32)     # in fp32 both sums round to a tie (to even): in fp64 they would not
    x = s + b
    assert x[0, 0] == x[0, 1]
    lp, rank, toks, _, _ = score_oracle(s.repeat(3, 0), b, [1, 0, -1], 2)
    assert rank.tolist() == [1, 0, -1] and toks[0].tolist() == [0, 1]
    assert lp[2] == 0.0 and lp[0] == lp[1] < 0
    lp, rank, toks, tlp, _ = score_oracle(s, b, None, 1)
    assert lp.tolist() == [0.0] and rank.tolist() == [-1] and toks.tolist() == [[0]]
    lp, rank, toks, tlp, _ = score_oracle(s, None, [1], 0)
    assert rank.tolist() == [0] and toks.shape == (1, 0) and tlp.shape == (1, 0)


# ---- every refusal in Python, on CPU tensors ----
def _model():
    from vmlmf_amd import Model
    torch.manual_seed(0)
    return Model(16, 8, 1, 0.0, 0.1, w_rank=4, u_ranks=[4], lstm_type="vmlmf")


_TOK = torch.zeros((5, 2), dtype=torch.int64)
REFUSALS = [
    (dict(tokens=_TOK, top=-1), "top"), (dict(tokens=_TOK, top=17), "top"), (dict(tokens=_TOK, top=33), "top"),
    (dict(tokens=_TOK, chunk_rows=0), "chunk_rows"), (dict(tokens=_TOK, chunk_rows=-4), "chunk_rows"),
    (dict(tokens=_TOK.to(torch.int32)), "int64"), (dict(tokens=_TOK.float()), "int64"), (dict(tokens=_TOK[:, 0]), "int64"),
    (dict(tokens=[[0, 1]]), "int64"),
    (dict(tokens=_TOK[:1]), "T >= 1"), (dict(tokens=_TOK[:0], targets=_TOK[:0]), "T >= 1"),
    (dict(tokens=_TOK, targets=_TOK[:4]), "targets"), (dict(tokens=_TOK, targets=_TOK.to(torch.int32)), "targets"),
    (dict(tokens=_TOK, targets=_TOK.t().contiguous()), "targets"), (dict(tokens=_TOK, targets=[0] * 5), "targets"),
    (dict(tokens=_TOK, lengths=torch.tensor([1, 2, 3])), "lengths"), (dict(tokens=_TOK, lengths=torch.tensor([[1, 2]])), "lengths"),
    (dict(tokens=_TOK, lengths=torch.tensor([1.0, 2.0])), "lengths"), (dict(tokens=_TOK, lengths=[1, 2]), "lengths"),
    (dict(tokens=_TOK, lengths=torch.tensor([True, False])), "lengths"),
]


@pytest.mark.parametrize("kw,words", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_model_score_refuses_with_a_value_error_before_the_cpu_tensors(kw, words):
    with pytest.raises(ValueError, match=words):
        _model().score(**kw)


def test_good_arguments_reach_the_refusal_of_cpu_tensors():
    m = _model()
    for kw in (dict(), dict(top=16), dict(targets=_TOK), dict(lengths=torch.tensor([5, 0])), dict(lengths=torch.tensor([5, 0], dtype=torch.int32)),
               dict(chunk_rows=1, top=3, states=m.state_init(2))):
        with pytest.raises(RuntimeError, match="cuda"):
            m.score(_TOK, **kw)
    flags = [mod.training for mod in m.modules()]
    assert all(flags) and all("_pack_cache" not in r.__dict__ for r in m.rnns)


def test_lm_score_refuses():
    from vmlmf_amd import lm_score
    h, w, b = torch.zeros(3, 8), torch.zeros(16, 8), torch.zeros(16)
    for kw, words in ((dict(top=-1), "top"), (dict(top=17), "top"), (dict(chunk_rows=0), "chunk_rows")):
        with pytest.raises(ValueError, match=words):
            lm_score(h, w, b, **kw)
    with pytest.raises(ValueError, match="top"):
        lm_score(torch.zeros(3, 8), torch.zeros(40, 8), None, top=33)
    with pytest.raises(ValueError, match="weight"):
        lm_score(h, b, None)
    with pytest.raises(RuntimeError, match="cuda"):
        lm_score(h, w, b, top=2)


# ---- the library and its binding ----
def declared_functions():
    text = open(os.path.join(ROOT, "include", "vmlmf_score.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vmlmf_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_function_is_exported_and_bound():
    from vmlmf_amd import _beam, _decode, _lib, _score
    decl = declared_functions()
    assert decl == ["vmlmf_score_abi_version", "vmlmf_score_last_error", "vmlmf_score_rows"]
    assert sorted(_score.SYMBOLS) == decl
    assert os.path.exists(_score.LIB_PATH), "run __graft_entry__.build() first"
    handle = ctypes.CDLL(_score.LIB_PATH)
    for name in decl:
        assert hasattr(handle, name), f"missing export {name}"
    header = open(os.path.join(ROOT, "include", "vmlmf_score.h")).read()
    assert int(re.search(r"#define VMLMF_SCORE_ABI_VERSION (\d+)", header).group(1)) == _score.ABI_VERSION == 1
    assert _score.lib().vmlmf_score_abi_version() == _score.ABI_VERSION
    assert int(re.search(r"#define VMLMF_SCORE_MAX_TOP (\d+)", header).group(1)) == _score.MAX_TOP == _beam.MAX_BEAMS
    assert not set(_score.SYMBOLS) & (set(_lib.SYMBOLS) | set(_beam.SYMBOLS) | set(_decode.SYMBOLS))   # the other ABIs are not touched
    for other in (_lib.LIB_PATH, _beam.LIB_PATH, _decode.LIB_PATH):
        assert not hasattr(ctypes.CDLL(other), "vmlmf_score_rows")                   # the kernel lives in the new library only


def _rows(R=2, V=16, scores=1, targets=1, top=0, logprob=1, rank=1, top_tokens=1, top_logprob=1):
    """vmlmf_score_rows with fake, never dereferenced pointers (1 = some non-null address): refusals come before any launch."""
    from vmlmf_amd import _score
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    lib = _score.lib()
    rc = lib.vmlmf_score_rows(R, V, p(scores), None, p(targets), top, p(logprob), p(rank), p(top_tokens), p(top_logprob), None)
    return rc, lib.vmlmf_score_last_error().decode()


def test_the_entry_point_refuses_on_the_host():
    from vmlmf_amd import _lib
    cases = [
        (dict(R=0), "R and V"), (dict(R=-2), "R and V"), (dict(V=0), "R and V"), (dict(V=-1), "R and V"),
        (dict(scores=None), "null pointer (scores)"),
        (dict(top=-1), "top must lie"), (dict(top=33), "top must lie"), (dict(V=5, top=6), "top must lie"), (dict(V=40, top=33), "top must lie"),
        (dict(top=1, top_tokens=None), "top > 0 needs"), (dict(V=40, top=32, top_logprob=None), "top > 0 needs"),
        (dict(logprob=None), "targets need logprob"),
    ]
    for kw, words in cases:
        rc, msg = _rows(**kw)
        assert rc == _lib.E_BADARG and words in msg and msg.startswith("vmlmf_score_rows: "), (kw, rc, msg)


def test_a_missing_library_is_a_clear_error(monkeypatch, tmp_path):
    from vmlmf_amd import _score
    monkeypatch.setattr(_score, "_handle", None)
    monkeypatch.setattr(_score, "LIB_PATH", str(tmp_path / "libvmlmf_score.so"))
    with pytest.raises(RuntimeError, match="libvmlmf_score.so is missing: build it"):
        _score.lib()
    with pytest.raises(RuntimeError, match="no stock-op fallback for Model.score"):
        _score.lib()
    assert not _score.loaded()


def test_the_library_is_loaded_by_the_first_scoring_call_only():
    """A process that imports the package, opens the main library and walks generate() and score() up to their refusals of CPU tensors
    has not opened libvmlmf_score.so."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import torch, vmlmf_amd\nfrom vmlmf_amd import _score, _lib\n_lib.lib()\n"
            "m = vmlmf_amd.Model(16, 8, 1, 0.0, 0.1, w_rank=4, u_ranks=[4], lstm_type='vmlmf')\n"
            "tok = torch.zeros((3, 2), dtype=torch.int64)\n"
            "for call in (lambda: m.generate(tok, 4), lambda: m.score(tok), lambda: m.score(tok, tok, top=4, lengths=torch.tensor([1, 2])),\n"
            "             lambda: vmlmf_amd.lm_score(torch.zeros(3, 8), torch.zeros(16, 8), None, top=2)):\n"
            "    try:\n        call()\n        raise SystemExit('no refusal')\n"
            "    except RuntimeError as e:\n        assert 'cuda' in str(e)\n"
            "maps = open('/proc/self/maps').read()\n"
            "assert 'libvmlmf_hip.so' in maps and 'libvmlmf_score.so' not in maps and not _score.loaded()\n"
            "_score.lib()\nassert 'libvmlmf_score.so' in open('/proc/self/maps').read() and _score.loaded()\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_the_makefile_builds_and_cleans_the_fourth_library():
    csrc = os.path.join(ROOT, "vmlmf_amd", "csrc")
    libs = ("libvmlmf_hip.so", "libvmlmf_beam.so", "libvmlmf_decode.so", "libvmlmf_score.so")
    r = subprocess.run(["make", "-n", "-B", "-C", csrc, "all"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and all(n in r.stdout for n in libs)
    links = [ln for ln in r.stdout.splitlines() if " -shared " in ln and "vmlmf_score.o" in ln]
    assert len(links) == 1 and "-o ../lib/libvmlmf_score.so" in links[0]                      # linked into its own library only
    assert not any(o in links[0] for o in ("vmlmf_sample.o", "vmlmf_decode.o", "vmlmf_beam.o"))
    r = subprocess.run(["make", "-n", "-C", csrc, "clean"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and all(n in r.stdout for n in libs) and "vmlmf_score.o" in r.stdout


def test_the_selection_is_still_written_once():
    """vmlmf_score.hip takes the merges, the reduction tree and the selection from vmlmf_select.h; it holds no copy of them."""
    text = open(os.path.join(ROOT, "vmlmf_amd", "csrc", "vmlmf_score.hip")).read()
    assert '#include "vmlmf_select.h"' in text
    for fn in ("best_merge", "lse_merge", "radix_select", "tie_cutoff", "choose_row", "key_of", "for_quads"):
        assert not re.search(r"__device__[^;{]*\b%s\s*\(" % fn, text), fn
    for fn in ("choose_row", "radix_select", "tie_cutoff"):
        assert re.search(r"\b%s\s*\(" % fn, text), fn                 # ... and calls them
