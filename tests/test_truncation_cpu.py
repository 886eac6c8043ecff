"""The truncation samplers of Model.generate (min_p, typical_p, epsilon_cutoff, eta_cutoff; C ABI vmlmf_truncate_choose in
libvmlmf_truncate.so, include/vmlmf_truncate.h): what can be checked without a GPU - the fp64 statement of the contract
(truncation_cases.py) on hand-made rows and against filtered_sets, the condition on its sets that the GPU tests
(test_gpu_truncation.py) rely on, every refusal in Python and at the C ABI.  (The library's exports, build rule and lazy load: its row
of test_side_libraries_cpu.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import truncation_cases as T
import vmlmf_decode_oracle as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vmlmf_amd", "csrc")


# ---- the oracle on hand-made rows ----
def _logits(p):
    return np.log(np.asarray(p, dtype=np.float64))


def test_min_p_keeps_whole_tie_groups_and_the_first_token():
    z = _logits([0.5, 0.2, 0.2, 0.05, 0.05])
    assert T.exact_set(z, min_p=0.4) == [0, 1, 2]                     # 0.2 >= 0.4 x 0.5: the tie group at the ratio is in, whole
    assert T.exact_set(z, min_p=0.41) == [0]
    assert T.exact_set(z, min_p=1.0) == [0]
    assert T.exact_set(z, min_p=0.1) == [0, 1, 2, 3, 4]
    assert T.exact_set(np.array([0.0, -np.inf, 0.0, -1.0]), min_p=1.0) == [0, 2]      # ties at the top; -inf is never kept
    # behind top-k: the ratio is to the largest probability, whatever the renormalisation
    assert T.exact_set(z, top_k=2, min_p=0.4) == [0, 1]


def test_typical_orders_by_the_deviation_from_the_entropy():
    p = np.array([0.4, 0.3, 0.2, 0.1])
    z = _logits(p)
    H = -(p * np.log(p)).sum()
    d = np.abs(-np.log(p) - H)
    assert np.argsort(d).tolist() == [1, 2, 0, 3]                     # the second token is the most typical one
    assert T.exact_set(z, typical_p=0.25) == [1]                      # a band that excludes the most probable token
    assert T.exact_set(z, typical_p=0.2999) == [1] and T.exact_set(z, typical_p=0.3001) == [1, 2]
    assert T.exact_set(z, typical_p=0.5001) == [0, 1, 2]
    assert T.exact_set(z, typical_p=0.99) == [0, 1, 2, 3]
    assert T.exact_set(z + 3.5, typical_p=0.25) == [1]                # a shift of the scores changes nothing


def test_a_tie_in_the_deviation_goes_to_the_lower_index():
    # four tokens of one score: every deviation is 0, the order is the index order, each token weighs 0.25
    z = np.zeros(4)
    assert T.exact_set(z, typical_p=0.3) == [0, 1]
    assert T.exact_set(z, typical_p=0.5) == [0, 1]
    assert T.exact_set(z, typical_p=0.51) == [0, 1, 2]
    # two tie groups, (0, 5) and (1 .. 4): whichever is nearer the entropy comes first, and inside a group the index decides
    z = np.array([np.log(4.0), 0.0, 0.0, 0.0, 0.0, np.log(4.0)])
    p = np.exp(z) / np.exp(z).sum()
    dd = np.abs(-np.log(p) + (p * np.log(p)).sum())
    assert dd[0] == dd[5] and dd[1] == dd[2] == dd[3] == dd[4] and dd[0] < dd[1]
    assert T.exact_set(z, typical_p=p[0] * 0.5) == [0] and T.exact_set(z, typical_p=p[0]) == [0]     # the mass before token 5 is p0
    assert T.exact_set(z, typical_p=p[0] * 1.5) == [0, 5]
    assert T.exact_set(z, typical_p=2 * p[0] + 1.5 * p[1]) == [0, 1, 2, 5]                            # the boundary inside the second group


def test_epsilon_and_eta_cut_by_probability_and_keep_the_top():
    p = np.array([0.6, 0.25, 0.1, 0.04, 0.01])
    z = _logits(p)
    assert T.exact_set(z, epsilon_cutoff=0.05) == [0, 1, 2]
    assert T.exact_set(z, epsilon_cutoff=0.7) == [0]                   # the most probable survivor is always kept
    assert T.exact_set(z, top_k=3, epsilon_cutoff=0.11) == [0, 1]      # renormalised over the survivors: 0.1 / 0.95 < 0.11
    assert T.exact_set(z, top_k=3, epsilon_cutoff=0.105) == [0, 1, 2]  # ... and 0.1 / 0.95 >= 0.105
    H = -(p * np.log(p)).sum()
    eta = 0.09
    thr = min(eta, np.sqrt(eta) * np.exp(-H))
    assert thr == eta and T.exact_set(z, eta_cutoff=eta) == [0, 1, 2]
    eta = 0.5
    thr = min(eta, np.sqrt(eta) * np.exp(-H))
    assert thr < eta and T.exact_set(z, eta_cutoff=eta) == np.flatnonzero(p >= thr).tolist()
    # typical first, then epsilon on what it kept: the most probable SURVIVOR stays, not the row's first token
    assert T.exact_set(_logits([0.4, 0.3, 0.2, 0.1]), typical_p=0.25, epsilon_cutoff=0.9) == [1]


def test_the_stages_run_in_order_on_the_survivors():
    rng = np.random.Generator(np.random.PCG64(3))
    z = rng.standard_normal(200) * 2
    kw = dict(min_p=0.02, typical_p=0.9, epsilon_cutoff=0.004)
    got = T.exact_set(z, top_k=50, top_p=0.95, **kw)
    keep = C.filtered_sets(z, 50, 0.95)[0]
    m = np.exp(z - z.max())
    keep &= m >= 0.02
    p = np.where(keep, m, 0) / m[keep].sum()
    c = z.max() - z
    d = np.abs(c - (p * c).sum())
    idx = np.flatnonzero(keep)
    order = idx[np.lexsort((idx, d[idx]))]
    before = np.concatenate([[0.0], np.cumsum(p[order])[:-1]])
    keep2 = np.zeros(200, bool)
    keep2[order[before < 0.9]] = True
    p2 = np.where(keep2, m, 0) / m[keep2].sum()
    keep3 = keep2 & ((p2 >= 0.004) | (z == z[keep2].max()))
    assert got == np.flatnonzero(keep3).tolist() and 1 < len(got) < 50


@pytest.mark.parametrize("k,p", [(None, None), (10, None), (None, 0.9), (20, 0.8)])
def test_everything_off_is_filtered_sets(k, p):
    rng = np.random.Generator(np.random.PCG64(5))
    for tau in (0.7, 1.0):
        z = rng.standard_normal(300) / tau
        for margin in (0.0, 1e-3):
            eps = C.nucleus_eps(p or 1.0, margin, 300) if margin else 0.0
            want = C.filtered_sets(z, k, p, margin, eps)
            for trunc in (None, {}, dict(T.OFF), dict(min_p=None, typical_p=None), dict(min_p=0, typical_p=1.0, epsilon_cutoff=0, eta_cutoff=0)):
                got = T.truncated_sets(z, k, p, trunc, margin, eps)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_the_margins_bracket_the_exact_set():
    for shape in [(3, 32, 97), (19, 40, 33)]:
        scores, _ = T.case_reference(*shape)
        for name in T.SETTINGS:
            k, p, trunc = T.setting(name, shape[2])
            for z in scores:
                ex = T.truncated_sets(z, k, p, trunc)[0]
                lo, hi = T.case_sets(z, name, 1e-4)
                assert (lo <= ex).all() and (ex <= hi).all() and lo.any()


# ---- the condition the GPU tests rely on ----
@pytest.mark.parametrize("tau", T.TAUS)
@pytest.mark.parametrize("name", T.SETTINGS)
@pytest.mark.parametrize("shape", T.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_truncation_cases_are_mostly_unambiguous(shape, name, tau):
    """At most 10 % of a case's rows may have different argmaxes over lo and hi - the cap the filter tests use -, on the plain and on the
    controlled scores; and the kept sets are neither one token nor the row."""
    scores, G = T.case_reference(*shape)
    margin = 1e-4 / tau
    share = T.ambiguous_share(scores / tau, G, name, margin)
    sizes = [int(T.case_sets(z / tau, name, margin)[0].sum()) for z in scores]
    _, c, _ = T.case_controlled(*shape)
    share_c = T.ambiguous_share(c / tau, G, name, C.z_margin(tau))
    print(f"{shape} {name} tau {tau}: ambiguous share {share:.4f} (controlled {share_c:.4f}), kept {min(sizes)} .. {max(sizes)} of {shape[2]}")
    assert share <= 0.10 and share_c <= 0.10
    assert 1 < max(sizes) and min(sizes) < shape[2]


# ---- refusals ----
BAD = [(dict(min_p=-0.1), "min_p"), (dict(min_p=1.5), "min_p"), (dict(min_p=float("nan")), "min_p"), (dict(min_p="x"), "min_p"),
       (dict(typical_p=0.0), "typical_p"), (dict(typical_p=1.2), "typical_p"), (dict(typical_p=-1), "typical_p"),
       (dict(epsilon_cutoff=-1e-3), "epsilon_cutoff"), (dict(epsilon_cutoff=1.0), "epsilon_cutoff"),
       (dict(eta_cutoff=-1e-3), "eta_cutoff"), (dict(eta_cutoff=1.0), "eta_cutoff"), (dict(eta_cutoff=float("inf")), "eta_cutoff")]


def _model(V=16):
    from vmlmf_amd import Model
    torch.manual_seed(0)
    return Model(V, 8, 1, 0.0, 0.1, w_rank=4, u_ranks=[4], lstm_type="vmlmf")


@pytest.mark.parametrize("kw,words", BAD, ids=[str(i) for i in range(len(BAD))])
def test_values_outside_their_ranges_are_refused(kw, words):
    from vmlmf_amd import Truncation
    with pytest.raises(ValueError, match=words):
        Truncation(**kw)
    with pytest.raises(ValueError, match=words):                       # ... by generate before the CPU tensors are
        _model().generate(torch.zeros((3, 2), dtype=torch.int64), 4, **kw)


def test_truncation_is_a_checked_value():
    from vmlmf_amd import Truncation
    for kw in (dict(), dict(min_p=0), dict(min_p=None, typical_p=1.0), dict(epsilon_cutoff=0, eta_cutoff=0.0)):
        assert not Truncation(**kw).on
    for kw in (dict(min_p=1.0), dict(min_p=1e-6), dict(typical_p=0.5), dict(epsilon_cutoff=3e-4), dict(eta_cutoff=0.002)):
        assert Truncation(**kw).on
    t = Truncation(min_p=0.1, typical_p=0.9, epsilon_cutoff=1e-3, eta_cutoff=2e-3)
    assert (t.min_p, t.typical_p, t.epsilon_cutoff, t.eta_cutoff) == (0.1, 0.9, 1e-3, 2e-3)
    s = t.struct()
    assert ctypes.sizeof(s) == 16 and [f[0] for f in s._fields_] == ["min_p", "typical_p", "epsilon_cutoff", "eta_cutoff"]


def test_generate_accepts_them_up_to_the_refusal_of_cpu_tensors():
    m = _model()
    prompt = torch.zeros((3, 2), dtype=torch.int64)
    for kw in (dict(min_p=0.1), dict(typical_p=0.9, eos=3), dict(epsilon_cutoff=1e-3, eta_cutoff=1e-3, top_k=5, top_p=0.9, repetition_penalty=1.2),
               dict(min_p=0.1, temperature=0.0), dict(min_p=0.0, typical_p=1.0, no_repeat_ngram_size=2)):
        with pytest.raises(RuntimeError, match="cuda"):
            m.generate(prompt, 4, **kw)


def test_history_controls_with_truncation_are_refused():
    from vmlmf_amd import DecodeGraph, HistoryControls, Truncation, lm_sample
    m = _model(64)
    prompt = torch.zeros((3, 2), dtype=torch.int64)
    for hist in (dict(no_repeat_ngram_size=2), dict(banned_sequences=[[1, 2]]), dict(frequency_penalty=0.5), dict(presence_penalty=0.5)):
        for kw in (dict(min_p=0.1), dict(typical_p=0.9), dict(epsilon_cutoff=1e-3), dict(eta_cutoff=1e-3)):
            with pytest.raises(ValueError, match="out of scope"):
                m.generate(prompt, 4, **hist, **kw)
    c = HistoryControls(2, 64, "cpu", no_repeat_ngram_size=2, prompt=prompt)
    with pytest.raises(ValueError, match="out of scope"):
        DecodeGraph(m, torch.zeros(2, 8), m.state_init(2), 4, controls=c, min_p=0.1)
    with pytest.raises(ValueError, match="min_p"):
        DecodeGraph(m, torch.zeros(2, 8), m.state_init(2), 4, min_p=2.0)
    assert "fused" in lm_sample.__doc__ and Truncation(min_p=0.1).on


def _choose(B=2, H=8, V=16, scores=1, inv=1.0, top_k=0, top_p=1.0, trunc=(0.1, 1.0, 0.0, 0.0), state=1, step=0, tokens=1, xn=None, embed=None,
            controls=None):
    """vmlmf_truncate_choose with fake, never dereferenced pointers (1 = some non-null address): refusals come before any launch."""
    from vmlmf_amd import _decode, _truncate
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    lib = _truncate.lib()
    t = None if trunc is None else ctypes.byref(_truncate.TruncationStruct(*trunc))
    c = None if controls is None else ctypes.byref(_decode.Controls(*controls))
    rc = lib.vmlmf_truncate_choose(B, H, V, p(scores), None, p(embed), inv, top_k, top_p, t, p(state), step, c, p(tokens), None, p(xn), None, None)
    return rc, lib.vmlmf_truncate_last_error().decode()


def test_the_entry_point_refuses_on_the_host():
    from vmlmf_amd import _lib
    nan = float("nan")
    cases = [
        (dict(trunc=None), _lib.E_BADARG, "null truncation"),
        (dict(trunc=(-0.1, 1.0, 0.0, 0.0)), _lib.E_BADARG, "min_p"), (dict(trunc=(1.1, 1.0, 0.0, 0.0)), _lib.E_BADARG, "min_p"),
        (dict(trunc=(nan, 1.0, 0.0, 0.0)), _lib.E_BADARG, "min_p"),
        (dict(trunc=(0.0, 0.0, 0.0, 0.0)), _lib.E_BADARG, "typical_p"), (dict(trunc=(0.0, 1.5, 0.0, 0.0)), _lib.E_BADARG, "typical_p"),
        (dict(trunc=(0.0, 1.0, -0.1, 0.0)), _lib.E_BADARG, "epsilon_cutoff"), (dict(trunc=(0.0, 1.0, 1.0, 0.0)), _lib.E_BADARG, "epsilon_cutoff"),
        (dict(trunc=(0.0, 1.0, 0.0, -0.1)), _lib.E_BADARG, "eta_cutoff"), (dict(trunc=(0.0, 1.0, 0.0, 1.0)), _lib.E_BADARG, "eta_cutoff"),
        (dict(inv=0.0, state=None), _lib.E_UNSUPPORTED, "greedy"),
        # ... everything the filtered choice refuses, in the same way
        (dict(B=0), _lib.E_BADARG, "B, "), (dict(V=-3), _lib.E_BADARG, "B, "), (dict(scores=None), _lib.E_BADARG, "null"),
        (dict(tokens=None), _lib.E_BADARG, "null"), (dict(inv=-1.0), _lib.E_BADARG, "temperature"), (dict(inv=nan), _lib.E_BADARG, "temperature"),
        (dict(state=None), _lib.E_BADARG, "snapshot"), (dict(xn=1, embed=None), _lib.E_BADARG, "embedding"), (dict(step=-1), _lib.E_BADARG, "step"),
        (dict(top_k=-1), _lib.E_BADARG, "top_k"), (dict(top_p=0.0), _lib.E_BADARG, "top_p"), (dict(top_p=1.5), _lib.E_BADARG, "top_p"),
        (dict(B=1 << 16, step=1 << 16), _lib.E_UNSUPPORTED, "2^32"),
        # ... and of the controls what the controlled choice refuses
        (dict(controls=(1.0, -1, 0, 0, None, None, 1, 1)), _lib.E_BADARG, "seen"), (dict(controls=(1.0, 16, 0, 0, None, 1, 1, 1)), _lib.E_BADARG, "eos"),
        (dict(controls=(0.0, -1, 0, 0, None, 1, 1, 1)), _lib.E_BADARG, "repetition_penalty"),
        (dict(controls=(1.0, -1, 1, 0, None, 1, 1, 1)), _lib.E_BADARG, "min_length needs eos"),
    ]
    for kw, code, words in cases:
        rc, msg = _choose(**kw)
        assert rc == code and words in msg and msg.startswith("vmlmf_truncate_choose: "), (kw, rc, msg)


def test_the_controlled_rows_are_written_once():
    """ControlledScores and the rows' state update live in vmlmf_controlled.h; both libraries include it and neither holds a copy; the
    select over a key view is the new header's, vmlmf_select.h's functions are called, not copied."""
    header = open(os.path.join(CSRC, "vmlmf_controlled.h")).read()
    assert re.search(r"struct ControlledScores\b", header) and "padding" in header and "finish" in header
    for name in ("vmlmf_decode.hip", "vmlmf_truncate.hip"):
        text = open(os.path.join(CSRC, name)).read()
        assert '#include "vmlmf_controlled.h"' in text and not re.search(r"struct ControlledScores\b", text), name
    dev = open(os.path.join(CSRC, "vmlmf_truncate.h")).read()
    assert '#include "vmlmf_select.h"' in dev
    for fn in ("radix_select", "tie_cutoff", "best_merge", "lse_merge", "key_of", "z_of", "mass_of", "for_quads", "gumbel_of", "write_pick"):
        assert not re.search(r"__device__[^;{]*\b%s\s*\(" % fn, dev), fn
    for fn in ("radix_select", "tie_cutoff", "for_quads", "mass_of", "view_select", "view_tie_cut", "sum_pass"):
        assert re.search(r"\b%s\s*\(" % fn, dev), fn
