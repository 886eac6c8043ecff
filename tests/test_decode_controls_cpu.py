"""Stopping and token controls of Model.generate (eos, min_length, repetition_penalty, logit_bias, banned_tokens; C ABI
vmlmf_decode_choose in libvmlmf_decode.so, include/vmlmf_decode.h): what can be checked without a GPU - the fp64 numpy oracle of the
controlled scores (oracle/vmlmf_decode_oracle.py) that the GPU tests (test_gpu_decode_controls.py) hold the kernel to, checked on itself; the kernel-level cases of
those tests and the condition on the oracle's sets that they rely on; every refusal, in Python and at the C ABI; the struct of the binding.

The contract (include/vmlmf_decode.h), per live row, on the fp32 scores x:
  1. repetition   r = seen[v] ? (x > 0 ? x / theta : x theta) : x
  2. bias         c = r + logit_bias[v]                       (entries finite or -inf)
  3. min length   c[eos] = -inf while length < min_length
then the existing choice (temperature, top-k, top-p, Gumbel-max; test_generate_filters_cpu.py has its oracle) runs on c."""
import ctypes

import numpy as np
import pytest
import torch

import vmlmf_decode_oracle as D


# ---- the oracle on itself ----
def test_the_sign_rule():
    x = np.array([2.0, -2.0, 0.5, -0.5])
    c = D.controlled_scores(x, [True, True, False, False], 2.0, None, None, 0, 0)
    assert c.tolist() == [1.0, -4.0, 0.5, -0.5]                    # a seen token always loses: positive scores shrink, negative grow
    c = D.controlled_scores(x, [True, True, False, False], 0.5, None, None, 0, 0)
    assert c.tolist() == [4.0, -1.0, 0.5, -0.5]                    # theta < 1 rewards repetition


def test_theta_one_is_the_identity_and_zero_stays_zero():
    rng = np.random.Generator(np.random.PCG64(1))
    x = rng.standard_normal((3, 50))
    seen = rng.random((3, 50)) < 0.5
    assert np.array_equal(D.controlled_scores(x, seen, 1.0, None, None, 0, 0), x)
    assert np.array_equal(D.controlled_scores(x, seen, 1.0, np.zeros(50), None, 0, 0), x)
    z = D.controlled_scores(np.zeros(4), [True, False, True, False], 3.0, None, None, 0, 0)
    assert (z == 0).all()
    # in fp32, as the kernel forms it: x / 1 and x * 1 are x to the bit
    x32 = x.astype(np.float32)
    assert np.array_equal(np.where(x32 > 0, x32 / np.float32(1), x32 * np.float32(1)).view(np.uint32), x32.view(np.uint32))


def test_a_ban_and_a_bias():
    x = np.array([1.0, 2.0, 3.0])
    lb = np.array([0.5, -np.inf, -1.0])
    c = D.controlled_scores(x, [False, False, True], 2.0, lb, None, 0, 0)
    assert c.tolist() == [1.5, -np.inf, 0.5]                       # the penalty first, the bias on its result
    lo, hi = D.filtered_sets(c, 2, None)
    assert np.flatnonzero(lo).tolist() == [0, 2]


def test_eos_below_the_minimum_length_and_at_it():
    x = np.array([[1.0, 5.0, 2.0], [1.0, 5.0, 2.0], [1.0, 5.0, 2.0]])
    c = D.controlled_scores(x, np.zeros((3, 3), bool), 1.0, None, 1, 2, np.array([0, 1, 2]))
    assert c[0].tolist() == [1.0, -np.inf, 2.0] and c[1].tolist() == [1.0, -np.inf, 2.0]
    assert c[2].tolist() == [1.0, 5.0, 2.0]                        # at the minimum length eos is free
    assert np.array_equal(D.controlled_scores(x, np.zeros((3, 3), bool), 1.0, None, None, 0, 0), x)
    seen, length, fin = D.next_state(np.zeros((3, 3), bool), np.array([0, 1, 2]), np.array([0, 0, 1]), [2, 1, 0], 1)
    assert seen.tolist() == [[False, False, True], [False, True, False], [False, False, False]]
    assert length.tolist() == [1, 2, 2] and fin.tolist() == [0, 1, 1]       # eos counts in the length; a finished row does not move


# ---- the kernel-level cases of the GPU tests: seeded on the CPU, so the condition on the oracle's sets is checked here ----
@pytest.mark.parametrize("tau", D.TAUS)
@pytest.mark.parametrize("name", D.CONTROL_SETTINGS)
@pytest.mark.parametrize("shape", D.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_controlled_kernel_cases_are_mostly_unambiguous(shape, name, tau):
    """Condition of the GPU test: at most 10 % of a case's rows may have different argmaxes over lo and hi."""
    _, c, G = D.case_controlled(*shape)
    k, p = D.control_setting(name, shape[2])
    share = D.ambiguous_share(c / tau, G, k, p, D.z_margin(tau))
    print(f"{shape} {name} tau {tau}: ambiguous share {share:.4f}")
    assert share <= 0.10


def test_the_cases_ban_tokens_and_hold_eos_back():
    for shape in D.SHAPES:
        seen, lb = D.case_controls(*shape)
        _, c, _ = D.case_controlled(*shape)
        assert np.isneginf(lb).any() and np.isfinite(lb).sum() > 2 and seen.any() and not seen.all()
        assert np.isneginf(c[:, D.EOS]).all() and (np.isneginf(c) == (np.isneginf(lb)[None, :] | (np.arange(shape[2]) == D.EOS)[None, :])).all()


# ---- every refusal ----
def _controls(**kw):
    from vmlmf_amd import DecodeControls
    return DecodeControls(kw.pop("B", 2), kw.pop("V", 16), "cpu", **kw)


REFUSALS = [
    (dict(repetition_penalty=0.0), "repetition_penalty"), (dict(repetition_penalty=-1.5), "repetition_penalty"),
    (dict(repetition_penalty=float("inf")), "repetition_penalty"), (dict(repetition_penalty=float("nan")), "repetition_penalty"),
    (dict(eos=3, min_length=-1), "min_length"), (dict(min_length=2), "min_length"),
    (dict(eos=16), "eos"), (dict(eos=-1), "eos"),
    (dict(banned_tokens=[3, 16]), "banned"), (dict(banned_tokens=[-1]), "banned"),
    (dict(logit_bias=torch.zeros(15)), "logit_bias"), (dict(logit_bias=torch.zeros(2, 16)), "logit_bias"),
    (dict(logit_bias=torch.zeros(16, dtype=torch.float64)), "logit_bias"), (dict(logit_bias=[0.0] * 16), "logit_bias"),
    (dict(logit_bias=torch.tensor([0.0] * 15 + [float("nan")])), "NaN"), (dict(logit_bias=torch.tensor([0.0] * 15 + [float("inf")])), "inf"),
    (dict(banned_tokens=list(range(16))), "no token"),
    (dict(logit_bias=torch.full((16,), float("-inf"))), "no token"),
    (dict(eos=3, min_length=1, banned_tokens=[v for v in range(16) if v != 3]), "besides eos"),
    (dict(eos=3, min_length=1, logit_bias=torch.tensor([float("-inf")] * 8 + [0.0] * 8), banned_tokens=[8, 9, 10, 11, 12, 13, 14, 15]), "no token"),
]


@pytest.mark.parametrize("kw,words", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_decode_controls_refuses(kw, words):
    with pytest.raises(ValueError, match=words):
        _controls(**kw)


def test_decode_controls_accepts_and_combines():
    c = _controls(eos=3, min_length=2, repetition_penalty=1.2, logit_bias=torch.tensor([0.5] * 16), banned_tokens=[1, 4],
                  prompt=torch.tensor([[0, 5], [2, 5], [0, 15]]))
    assert (c.eos, c.min_length, c.B, c.V) == (3, 2, 2, 16) and abs(c.repetition_penalty - 1.2) < 1e-12
    assert c.logit_bias.dtype == torch.float32 and torch.isneginf(c.logit_bias).nonzero()[:, 0].tolist() == [1, 4]
    assert c.logit_bias[0].item() == 0.5                                         # the bias and the bans are combined
    assert c.seen.dtype == torch.uint8 and c.seen.nonzero().tolist() == [[0, 0], [0, 2], [1, 5], [1, 15]]   # the set of the prompt's tokens
    assert c.finished.dtype == c.length.dtype == torch.int32 and not c.finished.any() and not c.length.any()
    d = c.clone()
    d.seen[0, 7] = 1
    assert c.seen[0, 7] == 0 and d.logit_bias is c.logit_bias
    # only eos left while it is free to be chosen is a valid (if dull) request
    _controls(eos=3, banned_tokens=[v for v in range(16) if v != 3])
    assert _controls().logit_bias is None and _controls(eos=2).eos == 2 and _controls().eos == -1
    with pytest.raises(ValueError, match="prompt"):
        _controls(prompt=torch.zeros((3, 5), dtype=torch.int64))


def test_generate_refuses_bad_controls_before_anything_else():
    """ValueError, even where the tensors would be refused next (they live on the CPU here); good controls reach that refusal."""
    from vmlmf_amd import Model, _decode
    torch.manual_seed(0)
    m = Model(16, 8, 1, 0.0, 0.1, w_rank=4, u_ranks=[4], lstm_type="vmlmf")
    prompt = torch.zeros((3, 2), dtype=torch.int64)
    for kw, words in REFUSALS:
        with pytest.raises(ValueError, match=words):
            m.generate(prompt, 4, **kw)
    with pytest.raises(ValueError, match="top_p"):                       # the filters' refusals are as they were
        m.generate(prompt, 4, eos=3, top_p=0.0)
    for kw in (dict(), dict(eos=3, min_length=2, repetition_penalty=1.2, banned_tokens=[1]), dict(return_lengths=True)):
        with pytest.raises(RuntimeError, match="cuda"):
            m.generate(prompt, 4, **kw)
    assert not _decode.controls_on() and not _decode.controls_on(repetition_penalty=1.0)
    assert _decode.controls_on(eos=0) and _decode.controls_on(repetition_penalty=1.1) and _decode.controls_on(banned_tokens=[])
    assert _decode.controls_on(logit_bias=torch.zeros(16))


# ---- the library and its binding ----

def test_the_controls_struct_is_the_headers():
    """(the exports, the ABI number, the lazy load and the Makefile: test_side_libraries_cpu.py)"""
    from vmlmf_amd import _decode
    # the struct the binding passes is the header's: four 32-bit scalars, then four pointers
    assert ctypes.sizeof(_decode.Controls) == 16 + 4 * ctypes.sizeof(ctypes.c_void_p)
    assert [f[0] for f in _decode.Controls._fields_] == ["repetition_penalty", "eos", "min_length", "pad", "logit_bias", "seen", "finished", "length"]


def _choose(B=2, H=8, V=16, scores=1, inv=1.0, top_k=0, top_p=1.0, state=1, step=0, tokens=1, xn=None, embed=None, controls=True,
            theta=1.0, eos=-1, min_length=0, seen=1, finished=1, length=1):
    """vmlmf_decode_choose with fake, never dereferenced pointers (1 = some non-null address): refusals come before any launch."""
    from vmlmf_amd import _decode
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    lib = _decode.lib()
    c = _decode.Controls(theta, eos, min_length, 0, None, seen, finished, length)
    rc = lib.vmlmf_decode_choose(B, H, V, p(scores), None, p(embed), inv, top_k, top_p, p(state), step, ctypes.byref(c) if controls else None,
                                 p(tokens), None, p(xn), None, None)
    return rc, lib.vmlmf_decode_last_error().decode()


def test_the_entry_point_refuses_on_the_host():
    from vmlmf_amd import _lib
    cases = [
        (dict(seen=None), _lib.E_BADARG, "seen"), (dict(finished=None), _lib.E_BADARG, "finished"), (dict(length=None), _lib.E_BADARG, "length"),
        (dict(controls=False), _lib.E_BADARG, "null controls"),
        (dict(eos=16), _lib.E_BADARG, "eos"), (dict(eos=99), _lib.E_BADARG, "eos"), (dict(eos=-2), _lib.E_BADARG, "eos"),
        (dict(theta=0.0), _lib.E_BADARG, "repetition_penalty"), (dict(theta=-1.0), _lib.E_BADARG, "repetition_penalty"),
        (dict(theta=float("nan")), _lib.E_BADARG, "repetition_penalty"), (dict(theta=float("inf")), _lib.E_BADARG, "repetition_penalty"),
        (dict(eos=3, min_length=-1), _lib.E_BADARG, "min_length"), (dict(min_length=1), _lib.E_BADARG, "min_length needs eos"),
        # ... and everything the filtered choice refuses, in the same way
        (dict(B=0), _lib.E_BADARG, "B, "), (dict(V=-3), _lib.E_BADARG, "B, "), (dict(scores=None), _lib.E_BADARG, "null"),
        (dict(tokens=None), _lib.E_BADARG, "null"), (dict(inv=-1.0), _lib.E_BADARG, "temperature"),
        (dict(inv=float("nan")), _lib.E_BADARG, "temperature"), (dict(state=None), _lib.E_BADARG, "snapshot"),
        (dict(xn=1, embed=None), _lib.E_BADARG, "embedding"), (dict(step=-1), _lib.E_BADARG, "step"),
        (dict(top_k=-1), _lib.E_BADARG, "top_k"), (dict(top_p=0.0), _lib.E_BADARG, "top_p"), (dict(top_p=1.5), _lib.E_BADARG, "top_p"),
        (dict(B=1 << 16, step=1 << 16), _lib.E_UNSUPPORTED, "2^32"),
    ]
    for kw, code, words in cases:
        rc, msg = _choose(**kw)
        assert rc == code and words in msg and msg.startswith("vmlmf_decode_choose: "), (kw, rc, msg)
