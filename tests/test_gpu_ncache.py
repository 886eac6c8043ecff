"""Model.cache_score and its launch (vmlmf_ncache_score, csrc/vmlmf_ncache.hip) against the fp64 reference of ncache_cases.py, within
the tolerance derived there per position.  Kernel level: the vocabulary's log-probabilities are an input, so no GEMM error enters;
workspace and outputs start as poison.  Model level: Model(97, 24, 2), T = 9, B = 3."""
import numpy as np
import pytest
import torch

import abi_arena as A
import ncache_cases as NC
from lm_util import DEV

pytestmark = pytest.mark.gpu
CHUNK_CASE = (3, 33, 0, 16, 24, 4, "plain", 1.0, 0.1)          # an empty cache, the band sliding inside the call
ARENA_CASE = (3, 33, 16, 16, 24, 4, "plain", 1.0, 0.1)
assert ARENA_CASE in NC.CASES


def _dev():
    return torch.device(DEV, torch.cuda.current_device())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).clone()


def _launch(case, parts=0, lam=None, theta=None, bufs=None, **over):
    """One vmlmf_ncache_score launch over a case's inputs through the C ABI; returns (logp, cache_logp) (T, B) on the CPU.  bufs: a
    dict of device buffers to use (an arena's) instead of fresh poisoned ones."""
    from vmlmf_amd import _ncache
    from vmlmf_amd._lib import ptr
    B, T, n, window, H, V, kind, th, la = case
    keys, toks, lv = NC.inputs(case)
    if bufs is None:
        bufs = dict(keys=keys.to(DEV), toks=toks.to(DEV), lv=lv.to(DEV), logp=torch.full((T, B), float("nan"), device=DEV),
                    lc=torch.full((T, B), float("nan"), device=DEV), ticket=torch.zeros(B * -(-T // 16), dtype=torch.int32, device=DEV),
                    workspace=torch.full((_ncache.workspace_bytes(B, T, n, window) // 4,), float("nan"), device=DEV))
    a = dict(B=B, T=T, n=n, H=H, window=window, theta=th if theta is None else theta, lam=la if lam is None else lam,
             keys=ptr(bufs["keys"]), toks=ptr(bufs["toks"]), lv=ptr(bufs["lv"]), logp=ptr(bufs["logp"]), lc=ptr(bufs["lc"]),
             ticket=ptr(bufs["ticket"]), workspace=ptr(bufs["workspace"]), ws=bufs["workspace"].numel() * bufs["workspace"].element_size(),
             parts=parts)
    a.update(over)
    _ncache.LIBRARY.call(_dev(), "vmlmf_ncache_score", *a.values())
    torch.cuda.synchronize()
    assert not bufs["ticket"].any()                                            # every launch leaves the tickets zero
    return bufs["logp"].cpu(), bufs["lc"].cpu()


# ---- 1. the launch against the reference ----
@pytest.mark.parametrize("case", NC.CASES, ids=NC.case_id)
def test_launch_against_the_reference(case):
    B, T, n, window, H, V, kind, theta, lam = case
    logp, lc = _launch(case)
    ref = NC.case_reference(case)
    worst_p, worst_c = NC.assert_close(logp, lc, ref, NC.case_id(case), lam)   # -inf and 0.0 exactly where they are due, too
    print(NC.case_id(case), "worst |error| / tol: logp", worst_p, "cache_logp", worst_c, "largest tol", float(ref[2].max()))
    if n == 0:
        assert torch.equal(_bits(logp[0]), _bits(NC.inputs(case)[2][0]))       # the first position of every row: lv's bits
    # lam = 0 returns lv bit for bit, whatever the cache holds; cache_logp is what it was
    logp0, lc0 = _launch(case, lam=0.0)
    assert torch.equal(_bits(logp0), _bits(NC.inputs(case)[2])) and torch.equal(_bits(lc0), _bits(lc))


# ---- 2. the same bits for every `parts` and from run to run ----
@pytest.mark.parametrize("case", NC.CASES, ids=NC.case_id)
def test_same_bits_for_every_parts_and_from_two_runs(case):
    first = None
    for parts in NC.PARTS + (NC.PARTS[-1],):
        logp, lc = _launch(case, parts)
        got = (_bits(logp), _bits(lc))
        first = first or got
        assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1]), (NC.case_id(case), parts)


# ---- 3. chunk splits: the cache carried from call to call ----
def test_chunk_splits_agree_and_carry_the_same_cache():
    from vmlmf_amd import NeuralCache, lm_cache_score
    B, T, n, window, H, V, kind, theta, lam = CHUNK_CASE
    g = torch.Generator().manual_seed(7)
    h = torch.tanh(torch.randn((T, B, H), generator=g))
    y = torch.randint(0, V, (T, B), generator=g)
    lv = -5 * torch.rand((T, B), generator=g) - 0.01
    ref = NC.reference(h.transpose(0, 1).contiguous(), y.t().contiguous(), lv, 0, window, theta, lam)
    hd, yd, lvd = h.to(DEV), y.to(DEV), lv.to(DEV)
    results = []
    for split in ((33,), (16, 17), (1,) * 33):
        cache, at, outs = NeuralCache(B, H, DEV, window), 0, []
        for step in split:
            outs.append(lm_cache_score(hd[at:at + step], yd[at:at + step], lvd[at:at + step], cache, theta, lam))
            at += step
            assert cache.n == min(window, at)
        logp, lc = (torch.cat([o[i] for o in outs]).cpu() for i in (0, 1))
        NC.assert_close(logp, lc, ref, f"split {split[:2]}", lam)
        results.append((logp, lc, cache))
    tol = ref[2].float()
    for logp, lc, cache in results[1:]:
        assert ((logp - results[0][0]).abs() <= tol).all()
        both = torch.isfinite(lc) & torch.isfinite(results[0][1])
        assert torch.equal(torch.isfinite(lc), torch.isfinite(results[0][1])) and ((lc - results[0][1]).abs()[both] <= tol[both]).all()
        assert torch.equal(cache.toks, results[0][2].toks) and torch.equal(cache.keys, results[0][2].keys)
    assert torch.equal(results[0][2].keys.cpu(), h[T - window:].transpose(0, 1)) and torch.equal(results[0][2].toks.cpu(), y[T - window:].t())


# ---- 4. exactly sized, poisoned buffers ----
def _arena(fill):
    from vmlmf_amd import _ncache
    B, T, n, window, H, V, kind, theta, lam = ARENA_CASE
    keys, toks, lv = NC.inputs(ARENA_CASE)
    arena = A.Arena(_dev(), fill, capacity=1 << 22)
    bufs = dict(keys=arena.buf(keys.shape, torch.float32, init=keys, name="keys"), toks=arena.buf(toks.shape, torch.int64, init=toks, name="key_tok"),
                lv=arena.buf(lv.shape, torch.float32, init=lv, name="vocab_logp"), logp=arena.buf((T, B), torch.float32, name="logp"),
                lc=arena.buf((T, B), torch.float32, name="cache_logp"),
                ticket=arena.buf(B * -(-T // 16), torch.int32, init=0, name="ticket"),
                workspace=arena.buf(_ncache.workspace_bytes(B, T, n, window), torch.uint8, name="workspace"))
    return arena, bufs


def test_poisoned_exactly_sized_buffers():
    runs = []
    for fill in A.FILLS:
        arena, bufs = _arena(fill)
        before = {k: bufs[k].clone() for k in ("keys", "toks", "lv")}
        logp, lc = _launch(ARENA_CASE, parts=3, bufs=bufs)
        arena.check_guards()
        A.assert_written(arena, "logp", bufs["logp"])
        if fill != A.FILL_ZERO:
            assert not bool(arena.unwritten(bufs["lc"]).any())                 # (cache_logp may be -inf: written all the same)
        A.assert_zero("ticket", bufs["ticket"])
        for k, t in before.items():
            assert torch.equal(t, bufs[k]), k                                  # the inputs are read only
        NC.assert_close(logp, lc, NC.case_reference(ARENA_CASE), f"fill {fill:#x}", ARENA_CASE[8])
        runs.append((logp, lc))
    for logp, lc in runs[1:]:
        A.assert_same_bits("logp", logp, runs[0][0], "between fills")
        A.assert_same_bits("cache_logp", lc, runs[0][1], "between fills")


def test_refusals_launch_nothing():
    from vmlmf_amd import _lib, _ncache
    B, T, n, window, H, V, kind, theta, lam = ARENA_CASE
    arena, bufs = _arena(A.FILL_NAN)
    enough = bufs["workspace"].numel()
    for over, code in ((dict(B=0), _lib.E_BADARG), (dict(window=0), _lib.E_BADARG), (dict(n=-1), _lib.E_BADARG), (dict(H=2049), _lib.E_BADARG),
                       (dict(theta=float("nan")), _lib.E_BADARG), (dict(lam=1.0), _lib.E_BADARG), (dict(parts=65), _lib.E_BADARG),
                       (dict(lv=None), _lib.E_BADARG), (dict(ws=enough - 1), _lib.E_WORKSPACE)):
        with pytest.raises(_lib.VmlmfError) as ei:
            _launch(ARENA_CASE, bufs=bufs, **over)
        assert ei.value.code == code, over
    torch.cuda.synchronize()
    arena.check_guards()
    for name in ("logp", "lc", "workspace"):
        A.assert_untouched(arena, name, bufs[name])
    A.assert_zero("ticket", bufs["ticket"])


# ---- 5. the model ----
def _model():
    from vmlmf_amd import Model
    torch.manual_seed(11)
    return Model(97, 24, 2, 0.0, 0.5, w_rank=8, u_ranks=[8], lstm_type="vmlmf").to(DEV)


def test_model_cache_score():
    from vmlmf_amd import NeuralCache, decoding, lm_cache_score
    m = _model()
    T, B, window, theta, lam = 9, 3, 6, 2.0, 0.2
    g = torch.Generator().manual_seed(3)
    tokens = torch.randint(0, 5, (T + 1, B), generator=g).to(DEV)             # five tokens: matches are frequent
    m.train()
    m.rnns[1].eval()
    flags = [mod.training for mod in m.modules()]
    logp, lv, lc, states, cache = m.cache_score(tokens, theta=theta, lam=lam, window=window, return_parts=True)
    assert [mod.training for mod in m.modules()] == flags                     # every flag as the caller left it
    assert logp.shape == lv.shape == lc.shape == (T, B) and cache.n == window and (cache.B, cache.H, cache.window) == (B, 24, window)
    # bit for bit lm_cache_score over _activations' outputs and score's log-probabilities
    s_lp, s_rank, s_states = m.score(tokens)
    assert torch.equal(_bits(lv), _bits(s_lp))
    with decoding._activations(m, tokens[:-1], None) as (h, st):
        mine = NeuralCache(B, 24, DEV, window)
        want_p, want_c = lm_cache_score(h, tokens[1:], s_lp, mine, theta, lam)
        h = h.clone()
    assert torch.equal(_bits(logp), _bits(want_p)) and torch.equal(_bits(lc), _bits(want_c))
    assert torch.equal(cache.keys, mine.keys) and torch.equal(cache.toks, mine.toks)
    assert torch.equal(cache.toks, tokens[1:][T - window:].t()) and torch.equal(cache.keys, h[T - window:].transpose(0, 1))
    for (a, b), (c, d) in zip(states, s_states):
        assert torch.equal(a, c) and torch.equal(b, d)
    # ... and the reference over the same outputs
    ref = NC.reference(h.transpose(0, 1).contiguous().cpu(), tokens[1:].t().contiguous().cpu(), s_lp.cpu(), 0, window, theta, lam)
    NC.assert_close(logp.cpu(), lc.cpu(), ref, "model", lam)
    assert int((ref[4] > 0).sum()) > T and torch.isfinite(lc).any()           # the cache had its say
    # the three-tuple form; lam = 0 is score()
    short = m.cache_score(tokens, theta=theta, lam=lam, window=window)
    assert len(short) == 3 and torch.equal(_bits(short[0]), _bits(logp))
    zero = m.cache_score(tokens, theta=theta, lam=0.0, window=window)
    assert torch.equal(_bits(zero[0]), _bits(s_lp))
    # two calls with carried states and cache against one
    a = m.cache_score(tokens[:5], theta=theta, lam=lam, window=window, return_parts=True)
    b = m.cache_score(tokens[4:], theta=theta, lam=lam, window=window, cache=a[4], states=a[3], return_parts=True)
    assert b[4] is a[4] and b[4].n == window
    both_p, both_c = torch.cat([a[0], b[0]]).cpu(), torch.cat([a[2], b[2]]).cpu()
    tol = ref[2].float()
    print("two calls against one: worst |difference| / tol", float(((both_p - logp.cpu()).abs() / tol).max()))
    assert ((both_p - logp.cpu()).abs() <= tol).all()
    fin = torch.isfinite(lc.cpu())
    assert torch.equal(torch.isfinite(both_c), fin) and ((both_c - lc.cpu()).abs()[fin] <= tol[fin]).all()
    assert torch.equal(b[4].toks, cache.toks)
    with pytest.raises(ValueError, match="window"):
        m.cache_score(tokens, window=7, cache=cache)
