"""Model.cache_score and libvmlmf_ncache.so without a GPU: the fp64 reference of ncache_cases.py against the brute-force definition
and on its special cases; the cases of the GPU tests; NeuralCache's bookkeeping; the refusals, from Python and from the C entry point;
the workspace; what the package exports; the signatures.  Header, SYMBOLS, exports, ABI number, Makefile and lazy loading:
test_side_libraries_cpu.py's table."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ncache_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ----
@pytest.mark.parametrize("shape", [(2, 9, 0, 4, 5, 3, 0.7, 0.2), (1, 12, 6, 5, 8, 4, 1.3, 0.1), (3, 5, 7, 16, 2, 2, -0.5, 0.6)])
def test_the_reference_is_the_brute_force_definition(shape):
    B, T, n, window, H, V, theta, lam = shape
    g = torch.Generator().manual_seed(5)
    keys = torch.randn((B, n + T, H), generator=g)
    toks = torch.randint(0, V, (B, n + T), generator=g)
    lv_full = torch.log_softmax(torch.randn((T, B, V), generator=g, dtype=torch.float64), -1)
    full, cache_p = NC.brute_force(keys, toks, lv_full, n, window, theta, lam)
    assert torch.allclose(full.exp().sum(-1), torch.ones((T, B), dtype=torch.float64), atol=1e-12)    # a distribution over V
    y = toks[:, n:].t()
    lv = torch.gather(lv_full, 2, y[..., None])[..., 0]
    logp, lc, tol, ms, matches = NC.reference(keys, toks, lv, n, window, theta, lam)
    want = torch.gather(full, 2, y[..., None])[..., 0]
    assert torch.allclose(logp, want, atol=1e-12, rtol=0), (logp - want).abs().max()
    p = torch.gather(cache_p, 2, y[..., None])[..., 0]
    has = matches > 0
    assert torch.allclose(lc[has].exp(), p[has], atol=1e-12) and (lc[~has] == -np.inf).all() and (p[~has] == 0).all()
    assert (ms == torch.clamp(n + torch.arange(T), max=window)[:, None]).all()


def test_the_reference_special_cases():
    keys = torch.tensor([[[1.0, 0.0], [0.5, 0.5], [0.0, 2.0], [1.0, 1.0]]])
    lv = torch.tensor([[-1.0], [-2.0], [-3.0], [-0.5]])
    lam = float(np.float32(0.1))
    # an empty band: lv; afterwards the band grows by one pair per position
    logp, lc, tol, ms, matches = NC.reference(keys, torch.tensor([[0, 1, 0, 0]]), lv, 0, 8, 0.3, 0.1)
    assert ms[:, 0].tolist() == [0, 1, 2, 3] and logp[0, 0] == -1.0 and lc[0, 0] == -np.inf and tol[0, 0] == 32 * NC.U * 2
    assert matches[:, 0].tolist() == [0, 0, 1, 2]
    assert lc[1, 0] == -np.inf and logp[1, 0] == np.log1p(-lam) - 2.0                                  # no match
    s = 0.3 * np.float64(np.float32(1.0)) * np.array([0.0, 1.0])                                        # position 2 against pairs 0, 1
    assert abs(float(lc[2, 0]) - (s[0] - np.logaddexp(s[0], s[1]))) < 1e-7
    # every band token is the target: 0.0 exactly, logp = log((1 - lam) p + lam)
    logp, lc, tol, ms, matches = NC.reference(keys, torch.tensor([[2, 2, 2, 2]]), lv, 0, 8, 0.3, 0.1)
    assert (lc[1:, 0] == 0).all() and abs(float(logp[3, 0]) - np.log((1 - lam) * np.exp(-0.5) + lam)) < 1e-12
    # lam = 0: lv whatever the cache holds, lc still reported
    logp0, lc0, tol0, _, _ = NC.reference(keys, torch.tensor([[2, 2, 0, 2]]), lv, 0, 8, 0.3, 0.0)
    assert torch.equal(logp0, lv.double()) and lc0[3, 0] < 0 and np.isfinite(float(lc0[3, 0]))
    # window 1: only the pair just before
    logp, lc, tol, ms, matches = NC.reference(keys, torch.tensor([[0, 1, 1, 0]]), lv, 0, 1, 0.3, 0.1)
    assert ms[:, 0].tolist() == [0, 1, 1, 1] and lc[:, 0].tolist() == [-np.inf, -np.inf, 0.0, -np.inf]
    # carried pairs: n = 2 of the same four rows
    logp, lc, tol, ms, matches = NC.reference(keys, torch.tensor([[0, 1, 0, 0]]), lv[:2], 2, 8, 0.3, 0.1)
    assert ms[:, 0].tolist() == [2, 3] and matches[:, 0].tolist() == [1, 2]


def test_the_cases_are_the_prescribed_ones():
    assert len(set(NC.CASES)) == len(NC.CASES) == 13 and sorted(NC.SEEDS) == sorted(NC.CASES)
    col = lambda i: {c[i] for c in NC.CASES}
    assert col(0) == {1, 3} and col(1) == {1, 16, 17, 33} and col(3) == {1, 15, 16, 17, 64}
    assert {1, 3, 24, 650} <= col(4) and max(col(4)) == 2048 and col(5) <= {2, 3, 4, 5}
    rel = {(("0" if n == 0 else n - w)) for B, T, n, w, *_ in NC.CASES}
    assert {"0", -1, 0, 5} <= rel
    assert any(w < T for B, T, n, w, *_ in NC.CASES) and any(w > n + T for B, T, n, w, *_ in NC.CASES)
    assert sum(c[6] == "hot" and c[4] == 650 for c in NC.CASES) == 2
    assert NC.PARTS == (1, 2, 3, 64, 0)


@pytest.mark.parametrize("case", NC.CASES, ids=NC.case_id)
def test_the_cases_have_what_they_are_for(case):
    B, T, n, window, H, V, kind, theta, lam = case
    keys, toks, lv = NC.inputs(case)
    assert keys.shape == (B, n + T, H) and toks.shape == (B, n + T) and lv.shape == (T, B) and keys.dtype == lv.dtype == torch.float32
    logp, lc, tol, ms, matches = NC.case_reference(case)
    assert torch.isfinite(logp).all() and (tol >= 0).all()
    if n == 0:
        assert (ms[0] == 0).all() and torch.equal(logp[0], lv[0].double())                           # the first position returns lv
    k = keys.double()
    top = (abs(theta) * (k @ k.transpose(1, 2))).max().item()
    if kind == "hot":
        assert top > 120, top                                                                          # expf overflows at 88
    # an fp32 evaluation of the same rule (stock torch on the CPU) passes, well inside the bound
    got_p, got_c = NC.fp32_rule(keys, toks, lv, n, window, theta, lam)
    worst_p, worst_c = NC.assert_close(got_p, got_c, (logp, lc, tol, ms, matches), NC.case_id(case), lam)
    assert max(worst_p, worst_c) < 0.5, (worst_p, worst_c)


def test_the_table_has_matches_of_every_kind():
    none = every = some = 0
    for case in NC.CASES:
        logp, lc, tol, ms, matches = NC.case_reference(case)
        live = ms > 0
        none += int((live & (matches == 0)).sum())
        every += int((live & (matches == ms) & (ms > 1)).sum())
        some += int((live & (matches > 0) & (matches < ms)).sum())
    assert none > 20 and every >= 3 and some > 100, (none, every, some)


# ---- NeuralCache ----
def test_neural_cache_bookkeeping():
    from vmlmf_amd import NeuralCache, _ncache
    c = NeuralCache(2, 3, "cpu", 5)
    assert (c.B, c.H, c.window, c.n) == (2, 3, 5, 0) and c.keys.shape == (2, 0, 3) and c.toks.shape == (2, 0)
    assert c.keys.dtype == torch.float32 and c.toks.dtype == torch.int64
    g = torch.Generator().manual_seed(0)
    hs, ys = torch.randn((14, 2, 3), generator=g), torch.randint(0, 9, (14, 2), generator=g)
    all_k, all_t = hs.transpose(0, 1), ys.t()
    c.update(hs[:3], ys[:3])                                                  # T < window
    assert c.n == 3 and torch.equal(c.keys, all_k[:, :3]) and torch.equal(c.toks, all_t[:, :3])
    keys, toks = c.extended(hs[3:5], ys[3:5])                                 # what a call reads: carried pairs, then its own
    assert keys.shape == (2, 5, 3) and keys.is_contiguous() and toks.is_contiguous()
    assert torch.equal(keys, all_k[:, :5]) and torch.equal(toks, all_t[:, :5]) and c.n == 3
    c.keep(keys, toks)                                                        # n + T == window
    assert c.n == 5 and torch.equal(c.keys, all_k[:, :5])
    d = c.clone()
    c.update(hs[5:6], ys[5:6])                                                # slides by one
    assert c.n == 5 and torch.equal(c.keys, all_k[:, 1:6]) and torch.equal(c.toks, all_t[:, 1:6])
    assert d.n == 5 and torch.equal(d.keys, all_k[:, :5]) and d.keys.data_ptr() != c.keys.data_ptr() and d.window == 5
    c.update(hs[6:14], ys[6:14])                                              # T > window: the call's last five
    assert c.n == 5 and torch.equal(c.keys, all_k[:, 9:14]) and torch.equal(c.toks, all_t[:, 9:14])
    c.reset()
    assert c.n == 0 and c.keys.shape == (2, 0, 3) and d.n == 5
    for args in ((0, 3, "cpu", 5), (2, 0, "cpu", 5), (2, 3, "cpu", 0), (2, 2049, "cpu", 5), (2, 3, "cpu", 2.5)):
        with pytest.raises(ValueError):
            NeuralCache(*args)
    assert NeuralCache(1, 2048, "cpu").window == 500


def test_check_ncache_and_the_refusals_of_cache_score():
    from vmlmf_amd import Model, NeuralCache, _ncache, lm_cache_score
    assert _ncache.check_ncache(500, 0.3, 0.1, 650) == (500, 0.3, 0.1) and _ncache.check_ncache(1, -2, 0, 2048) == (1, -2.0, 0.0)
    for args, word in (((0, 0.3, 0.1), "window"), ((-3, 0.3, 0.1), "window"), ((1.5, 0.3, 0.1), "window"), ((5, float("inf"), 0.1), "theta"),
                       ((5, float("nan"), 0.1), "theta"), ((5, 0.3, 1.0), "lam"), ((5, 0.3, -0.01), "lam"), ((5, 0.3, float("nan")), "lam"),
                       ((5, 0.3, 0.1, 2049), "hidden size"), ((5, 0.3, 0.1, 0), "hidden size")):
        with pytest.raises(ValueError, match=word):
            _ncache.check_ncache(*args)
    m = Model(97, 16, 2, 0.0, 0.1, w_rank=8, u_ranks=[8], lstm_type="vmlmf")
    tok = torch.zeros((4, 2), dtype=torch.int64)
    for kw, word in ((dict(window=0), "window"), (dict(theta=float("inf")), "theta"), (dict(lam=1.0), "lam"), (dict(lam=-1), "lam"),
                     (dict(chunk_rows=0), "chunk_rows"), (dict(cache=NeuralCache(3, 16, "cpu", 500)), "B=3"),
                     (dict(cache=NeuralCache(2, 8, "cpu", 500)), "H=8"), (dict(cache=NeuralCache(2, 16, "cpu", 7)), "window=7"),
                     (dict(cache=NeuralCache(2, 16, "cpu", 500), window=7), "window=500"), (dict(cache="no"), "NeuralCache")):
        with pytest.raises(ValueError, match=word):
            m.cache_score(tok, **kw)
    with pytest.raises(ValueError, match="T >= 1"):
        m.cache_score(tok[:1])
    with pytest.raises(ValueError, match="int64"):
        m.cache_score(tok.int())
    with pytest.raises(ValueError, match="targets"):
        m.cache_score(tok, tok[:2])
    with pytest.raises(TypeError):
        m.cache_score(tok, None, 0.3)                                           # everything behind targets is keyword-only
    with pytest.raises(RuntimeError, match="cuda"):
        m.cache_score(tok)
    with pytest.raises(RuntimeError, match="cuda"):
        m.cache_score(tok, tok, theta=1.0, lam=0.0, window=7, cache=NeuralCache(2, 16, "cpu", 7), return_parts=True)
    c = NeuralCache(2, 16, "cpu", 7)
    h, y, lv = torch.zeros((3, 2, 16)), torch.zeros((3, 2), dtype=torch.int64), torch.zeros((3, 2))
    for kw, word in ((dict(theta=float("nan")), "theta"), (dict(lam=1.5), "lam"), (dict(parts=65), "parts"), (dict(parts=-1), "parts")):
        with pytest.raises(ValueError, match=word):
            lm_cache_score(h, y, lv, c, **kw)
    with pytest.raises(RuntimeError, match="HIP device"):
        lm_cache_score(h, y, lv, c)
    with pytest.raises(RuntimeError, match="NeuralCache"):
        lm_cache_score(h, y, lv, None)
    assert c.n == 0                                                             # a refused call moves nothing


def test_the_entry_point_refuses_bad_arguments_without_touching_the_gpu():
    from vmlmf_amd import _lib, _ncache
    lib = _ncache.lib()
    one, out = ctypes.c_void_p(64), ctypes.c_void_p(128)                      # never dereferenced: every call below is refused first
    enough = _ncache.workspace_bytes(2, 9, 5, 8)

    def score(B=2, T=9, n=5, H=16, window=8, theta=0.3, lam=0.1, ws=enough, parts=0, keys=one, toks=one, lv=one, logp=out, lc=out,
              ticket=out, workspace=out):
        return lib.vmlmf_ncache_score(B, T, n, H, window, theta, lam, keys, toks, lv, logp, lc, ticket, workspace, ws, parts, None)

    for kw, word in ((dict(B=0), b">= 1"), (dict(T=0), b">= 1"), (dict(H=0), b">= 1"), (dict(window=0), b">= 1"), (dict(n=-1), b">= 0"),
                     (dict(B=2 ** 20, n=2 ** 11), b"2\\^31"), (dict(B=2 ** 25, T=1, n=0), b"2\\^25"), (dict(H=2049), b"2048"),
                     (dict(theta=float("inf")), b"theta"), (dict(theta=float("nan")), b"theta"), (dict(lam=1.0), b"lam"),
                     (dict(lam=-0.5), b"lam"), (dict(lam=float("nan")), b"lam"), (dict(parts=-1), b"parts"), (dict(parts=65), b"parts"),
                     (dict(keys=None), b"null"), (dict(toks=None), b"null"), (dict(lv=None), b"null"), (dict(logp=None), b"null"),
                     (dict(lc=None), b"null"), (dict(ticket=None), b"null"), (dict(workspace=None), b"null"),
                     (dict(keys=ctypes.c_void_p(72)), b"16-byte"), (dict(workspace=ctypes.c_void_p(130)), b"4-byte")):
        assert score(**kw) == _lib.E_BADARG, kw
        err = lib.vmlmf_ncache_last_error()
        assert re.search(word, err) and err.startswith(b"vmlmf_ncache_score: "), (kw, err)
    assert score(ws=enough - 1) == _lib.E_WORKSPACE and b"vmlmf_ncache_workspace_bytes" in lib.vmlmf_ncache_last_error()
    with pytest.raises(_lib.VmlmfError) as ei:
        _ncache.check(score(lam=2.0))
    assert ei.value.code == _lib.E_BADARG and "lam" in str(ei.value)


def test_workspace_bytes():
    from vmlmf_amd import _ncache
    ws = _ncache.lib().vmlmf_ncache_workspace_bytes
    # (10, 35, 500, 650) with a full cache: three query tiles per row, ceil(515 / 16) = 33 key tiles, 3 x 16 numbers each
    assert ws(10, 35, 500, 650, 500) == 10 * 3 * 33 * 48 * 4 == _ncache.workspace_bytes(10, 35, 500, 500)
    assert ws(1, 1, 0, 1, 1) == 48 * 4 == _ncache.workspace_bytes(1, 1, 0, 1)                    # never below one key tile
    assert ws(3, 33, 0, 24, 64) == 3 * 3 * 3 * 48 * 4 == _ncache.workspace_bytes(3, 33, 0, 64)       # window > n + T: n + T decides
    for B, T, n, w in ((2, 17, 64, 64), (1, 70, 2000, 2000), (32, 35, 7, 500), (1, 16, 3, 2 ** 31 - 1)):
        assert ws(B, T, n, 8, w) == _ncache.workspace_bytes(B, T, n, w), (B, T, n, w)
    for bad in ((0, 9, 5, 16, 8), (2, 0, 5, 16, 8), (2, 9, -1, 16, 8), (2, 9, 5, 0, 8), (2, 9, 5, 16, 0), (2, 9, 5, 2049, 8),
                (2 ** 20, 9, 2 ** 11, 16, 8)):
        assert ws(*bad) == 0, bad
    assert (_ncache.MAX_H, _ncache.MAX_PARTS) == (2048, 64) and _ncache.MAX_H >= 1024
    text = open(os.path.join(ROOT, "include", "vmlmf_ncache.h")).read()
    for name, value in (("MAX_H", 2048), ("MAX_PARTS", 64)):                  # the Python side mirrors the header's limits
        assert int(re.search(r"#define VMLMF_NCACHE_%s (\d+)" % name, text).group(1)) == value


# ---- what the package exports ----
def test_the_package_exports_the_neural_cache():
    import vmlmf_amd
    from vmlmf_amd import _ncache as b
    from vmlmf_amd import scoring
    assert vmlmf_amd.__all__[-2:] == ["NeuralCache", "lm_cache_score"]
    assert vmlmf_amd.NeuralCache is scoring.NeuralCache is b.NeuralCache
    assert vmlmf_amd.lm_cache_score is scoring.lm_cache_score is b.lm_cache_score
    assert callable(scoring.cache_score) and callable(vmlmf_amd.Model.cache_score)


# ---- the signatures ----
def test_the_signatures():
    from vmlmf_amd import Model, NeuralCache, _ncache, scoring
    for fn, lead in ((Model.cache_score, ["self"]), (scoring.cache_score, ["model"])):
        ps = inspect.signature(fn).parameters
        assert list(ps) == lead + ["tokens", "targets", "theta", "lam", "window", "cache", "states", "return_parts", "chunk_rows"]
        for name in lead + ["tokens", "targets"]:
            assert ps[name].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
        for name in ("theta", "lam", "window", "cache", "states", "return_parts", "chunk_rows"):
            assert ps[name].kind is inspect.Parameter.KEYWORD_ONLY
        got = {k: p.default for k, p in ps.items() if p.default is not inspect.Parameter.empty}
        assert got == dict(targets=None, theta=0.3, lam=0.1, window=500, cache=None, states=None, return_parts=False, chunk_rows=2048)
    ps = inspect.signature(scoring.lm_cache_score).parameters
    assert list(ps) == ["h", "targets", "vocab_logp", "cache", "theta", "lam", "parts"]
    assert (ps["theta"].default, ps["lam"].default, ps["parts"].default) == (0.3, 0.1, 0)
    assert list(inspect.signature(_ncache.check_ncache).parameters) == ["window", "theta", "lam", "H"]
    assert list(inspect.signature(NeuralCache.__init__).parameters) == ["self", "B", "H", "device", "window"]
    assert callable(NeuralCache.clone) and callable(NeuralCache.reset)
    # generate, beam_search and score keep theirs
    assert list(inspect.signature(Model.score).parameters) == ["self", "tokens", "targets", "states", "lengths", "top", "chunk_rows"]
