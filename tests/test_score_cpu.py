"""Model.score and lm_score (C ABI vmlmf_score_rows in libvmlmf_score.so, include/vmlmf_score.h): what can be checked without a GPU -
the numpy oracle (oracle/vmlmf_decode_oracle.py) that the GPU tests (test_gpu_score.py) hold the kernel to, checked on itself; every
refusal, in Python and at the C ABI.

The contract, per row, on x = bias + scores in fp32: the tokens' ORDER is larger x first, equal x to the lower index;
logprob = x[y] - logsumexp(x); rank = how many tokens are ahead of y in the order; the top tokens are the order's first `top`."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from vmlmf_decode_oracle import score_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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

def test_max_top_is_the_headers_and_the_beam_limit():
    """(the exports, the ABI number, the lazy load and the Makefile: test_side_libraries_cpu.py)"""
    from vmlmf_amd import _beam, _score
    header = open(os.path.join(ROOT, "include", "vmlmf_score.h")).read()
    assert int(re.search(r"#define VMLMF_SCORE_MAX_TOP (\d+)", header).group(1)) == _score.MAX_TOP == _beam.MAX_BEAMS


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
