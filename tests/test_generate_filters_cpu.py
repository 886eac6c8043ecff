"""Top-k and nucleus (top-p) sampling (Model.generate(top_k, top_p), C ABI vmlmf_lm_sample_filtered / vmlmf_lm_choose_filtered): what
can be checked without a GPU - the new entry points' host-side refusals, the workspace size, the Python-level argument checks - and
the fp64 numpy oracle of a filtered choice (oracle/vmlmf_decode_oracle.py) that the GPU tests (test_gpu_generate_filters.py) hold the
kernels to, checked on itself.

The oracle.  The filters act on the tempered scores z = scores / tau under one total order (larger z first, equal z to the lower
index): top_k keeps the first k tokens; top_p keeps, of those, the token at sorted position j iff the mass of the tokens before it -
exp(z - z_max) over the set top-k kept, normalised by its own sum - is < p.  fp32 scores cannot order near-equal tokens, so the oracle
returns two sets per row: `lo`, the tokens kept under any admissible rounding, and `hi`, the tokens possibly kept (filtered_sets)."""
import ctypes

import numpy as np
import pytest
import torch

from vmlmf_amd import _lib
from vmlmf_decode_oracle import LDS_ROW, SETTINGS, SHAPES, TAUS, ambiguous_share, case_reference, filtered_sets, nucleus_eps, setting

# ---- the kernel-level cases of the GPU tests: seeded on the CPU, so the condition on the oracle's sets is checked here ----
@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("name", SETTINGS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_kernel_cases_are_mostly_unambiguous(shape, name, tau):
    """Condition of the GPU test: at most 10 % of a case's rows may have different argmaxes over lo and hi."""
    scores, G = case_reference(*shape)
    k, p = setting(name, shape[2])
    assert ambiguous_share(scores / tau, G, k, p, 1e-4 / tau) <= 0.10


# ---- the oracle on itself ----
@pytest.mark.parametrize("V,k,p", [(97, 10, None), (97, None, 0.9), (97, 10, 0.8), (33, 5, 0.7), (1000, 50, 0.9), (1000, None, 0.95),
                                   (97, 1, None), (97, None, 1e-6), (97, 97, 1.0), (97, 0, None)])
def test_the_exact_kept_set(V, k, p):
    rng = np.random.Generator(np.random.PCG64(V + (k or 0)))
    for _ in range(8):
        z = rng.standard_normal(V) * 2.0
        lo, hi = filtered_sets(z, k, p)
        assert np.array_equal(lo, hi)
        order = np.argsort(-z)
        n = lo.sum()
        assert lo[order[:n]].all()                              # a prefix of the order
        kk = V if not k or k >= V else k
        if p is None or p >= 1.0:
            assert n == kk                                      # exactly k kept
            continue
        assert 1 <= n <= kk
        mass = np.exp(z[order[:kk]] - z[order[0]])
        mass /= mass.sum()
        assert mass[:n].sum() >= p or n == kk                   # the kept mass reaches p ...
        assert mass[:n - 1].sum() < p                           # ... and does not without its last token


def test_equal_scores_go_to_the_lower_index():
    z = np.array([0.0, 2.0, 1.0, 1.0, 1.0, -1.0])
    lo, _ = filtered_sets(z, 2, None)
    assert np.flatnonzero(lo).tolist() == [1, 2]
    lo, _ = filtered_sets(z, 3, None)
    assert np.flatnonzero(lo).tolist() == [1, 2, 3]
    # masses e^0, e^-1 x 3, ...: the mass before token 3 is (1 + e^-1) / sum
    m = np.exp(z - 2.0)
    p = (1 + 1.5 * np.exp(-1.0)) / m.sum()                      # inside the tie group: after its first, before its second member
    lo, _ = filtered_sets(z, None, p)
    assert np.flatnonzero(lo).tolist() == [1, 2, 3]
    # with a margin every member of the group is possible, none is certain
    lo, hi = filtered_sets(z, 2, None, margin=1e-4)
    assert np.flatnonzero(lo).tolist() == [1] and np.flatnonzero(hi).tolist() == [1, 2, 3, 4]


def test_the_margin_opens_lo_and_hi_around_the_exact_set():
    rng = np.random.Generator(np.random.PCG64(5))
    z = rng.standard_normal(1000)
    for k, p in ((50, None), (None, 0.9), (50, 0.9)):
        ex, _ = filtered_sets(z, k, p)
        lo, hi = filtered_sets(z, k, p, 5e-2, nucleus_eps(p or 1.0, 5e-2, 1000))
        assert (lo <= ex).all() and (ex <= hi).all() and lo.sum() < hi.sum()


# ---- the C ABI's host side ----
def _filtered(fn, B=2, H=8, V=16, inv=1.0, top_k=0, top_p=1.0, state=1, step=0, tokens=1, xn=None, embed=None, ticket=1, ws=1,
              nbytes=1 << 20, first=1, second=1):
    """A filtered entry point with fake, never dereferenced pointers (1 = some non-null address)."""
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    lib = _lib.lib()
    if fn == "sample":
        rc = lib.vmlmf_lm_sample_filtered(B, H, V, p(first), p(second), None, p(embed), inv, top_k, top_p, p(state), step, p(tokens), None,
                                          p(xn), None, p(ticket), p(ws), nbytes, None)
    else:
        rc = lib.vmlmf_lm_choose_filtered(B, H, V, p(first), None, p(embed), inv, top_k, top_p, p(state), step, p(tokens), None, p(xn),
                                          None, None)
    return rc, lib.vmlmf_last_error().decode()


@pytest.mark.parametrize("fn", ["sample", "choose"])
def test_the_filtered_entry_points_refuse_on_the_host(fn):
    cases = [
        (dict(top_k=-1), _lib.E_BADARG, "top_k"), (dict(top_p=0.0), _lib.E_BADARG, "top_p"), (dict(top_p=-0.5), _lib.E_BADARG, "top_p"),
        (dict(top_p=1.5), _lib.E_BADARG, "top_p"), (dict(top_p=float("nan")), _lib.E_BADARG, "top_p"),
        (dict(top_p=float("inf")), _lib.E_BADARG, "top_p"),
        # ... and everything the unfiltered functions refuse, in the same way
        (dict(B=0), _lib.E_BADARG, "B, "), (dict(V=-3), _lib.E_BADARG, "B, "),
        (dict(first=None), _lib.E_BADARG, "null"), (dict(tokens=None), _lib.E_BADARG, "null"),
        (dict(inv=-1.0), _lib.E_BADARG, "temperature"), (dict(inv=float("nan")), _lib.E_BADARG, "temperature"),
        (dict(inv=float("inf")), _lib.E_BADARG, "temperature"),
        (dict(state=None), _lib.E_BADARG, "snapshot"),
        (dict(xn=1, embed=None), _lib.E_BADARG, "embedding"),
        (dict(step=-1), _lib.E_BADARG, "step"),
        (dict(B=1 << 16, step=1 << 16), _lib.E_UNSUPPORTED, "2^32"),
    ]
    if fn == "sample":
        cases += [(dict(H=0), _lib.E_BADARG, "B, H, V"), (dict(second=None), _lib.E_BADARG, "null"), (dict(ticket=None), _lib.E_BADARG, "null"),
                  (dict(ws=None), _lib.E_BADARG, "null"), (dict(nbytes=0), _lib.E_WORKSPACE, "workspace"),
                  # the unfiltered size does not hold the scores
                  (dict(nbytes=_lib.lib().vmlmf_lm_sample_workspace_bytes(2, 16)), _lib.E_WORKSPACE, "workspace")]
    for kw, code, words in cases:
        rc, msg = _filtered(fn, **kw)
        assert rc == code and words in msg, (kw, rc, msg)


def test_the_filtered_workspace_is_monotone_and_holds_the_unfiltered_one():
    lib = _lib.lib()
    f = lib.vmlmf_lm_sample_filtered_workspace_bytes
    assert f(0, 100) == 0 and f(4, 0) == 0 and f(-1, -1) == 0
    prev_v = 0
    for V in (1, 15, 16, 17, 97, 1000, 8191, 8192, 8193, 10000, LDS_ROW + 5, 50000, 262144):
        prev_b = 0
        for B in (1, 2, 4, 16, 17, 32, 256, 4096):
            n = f(B, V)
            assert n >= prev_b and n > 0
            assert n >= lib.vmlmf_lm_sample_workspace_bytes(B, V) + 4 * B * V
            prev_b = n
        n = f(32, V)
        assert n >= prev_v
        prev_v = n
    assert f(4, 10000) <= 1 << 20                       # the widths the fused form is for: 4 rows of scores and their partials


# ---- the Python layers ----
def test_generate_refuses_bad_filters_before_any_device_work():
    """The filters are checked first: a ValueError, even where the tensors would be refused next (they live on the CPU here)."""
    from vmlmf_amd import Model, lm_sample
    from vmlmf_amd.decoding import sample_filters
    torch.manual_seed(0)
    m = Model(97, 32, 2, 0.0, 0.1, w_rank=8, u_ranks=[8], lstm_type="vmlmf")
    prompt = torch.zeros((3, 2), dtype=torch.int64)
    for kw in (dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1), dict(top_p=float("nan"))):
        with pytest.raises(ValueError, match="top_k|top_p"):
            m.generate(prompt, 4, **kw)
    with pytest.raises(RuntimeError, match="cuda"):              # good filters: the existing refusal of CPU tensors
        m.generate(prompt, 4, top_k=10, top_p=0.9)
    with pytest.raises(RuntimeError, match="cuda"):
        lm_sample(torch.zeros(2, 32), m.fc.w.detach(), m.fc.b.detach(), 1.0, top_k=5)
    assert sample_filters(None, None) == (0, 1.0) and sample_filters(0, 1.0) == (0, 1.0)
    assert sample_filters(10, 0.5, 97) == (10, 0.5) and sample_filters(97, None, 97) == (0, 1.0) and sample_filters(200, None, 97) == (0, 1.0)
    with pytest.raises(ValueError, match="top_k"):
        sample_filters(-3, None)
    with pytest.raises(ValueError, match="top_p"):
        sample_filters(None, 0)
