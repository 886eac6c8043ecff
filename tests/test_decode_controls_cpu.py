"""Stopping and token controls of Model.generate (eos, min_length, repetition_penalty, logit_bias, banned_tokens; C ABI
vmlmf_decode_choose in libvmlmf_decode.so, include/vmlmf_decode.h): what can be checked without a GPU - the fp64 numpy oracle of the
controlled scores that the GPU tests (test_gpu_decode_controls.py) hold the kernel to, checked on itself; the kernel-level cases of
those tests and the condition on the oracle's sets that they rely on; every refusal; the library, its binding and its lazy load.

The contract (include/vmlmf_decode.h), per live row, on the fp32 scores x:
  1. repetition   r = seen[v] ? (x > 0 ? x / theta : x theta) : x
  2. bias         c = r + logit_bias[v]                       (entries finite or -inf)
  3. min length   c[eos] = -inf while length < min_length
then the existing choice (temperature, top-k, top-p, Gumbel-max; test_generate_filters_cpu.py has its oracle) runs on c."""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_generate_filters_cpu as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def controlled_scores(x, seen, theta, logit_bias, eos, min_length, length):
    """Steps 1 - 3 in fp64.  x (..., V) raw scores; seen (..., V) bool; logit_bias (V) or None; eos a token or None; length (...) or a
    scalar: the rows' lengths so far.  Returns c (..., V)."""
    x = np.asarray(x, dtype=np.float64)
    r = np.where(np.asarray(seen, dtype=bool), np.where(x > 0, x / theta, x * theta), x)
    c = r if logit_bias is None else r + np.asarray(logit_bias, dtype=np.float64)
    c = np.array(np.broadcast_to(c, x.shape), dtype=np.float64)
    if eos is not None:
        below = np.broadcast_to(np.asarray(length) < min_length, x.shape[:-1])
        c[..., eos] = np.where(below, -np.inf, c[..., eos])
    return c


def next_state(seen, length, finished, tokens, eos):
    """Step 6 for live rows: (seen, length, finished) after `tokens` (B); finished rows are left as they are."""
    seen, length, finished = seen.copy(), length.copy(), finished.copy()
    for b, t in enumerate(tokens):
        if finished[b]:
            continue
        seen[b, t] = True
        length[b] += 1
        if eos is not None and t == eos:
            finished[b] = 1
    return seen, length, finished


# ---- the oracle on itself ----
def test_the_sign_rule():
    x = np.array([2.0, -2.0, 0.5, -0.5])
    c = controlled_scores(x, [True, True, False, False], 2.0, None, None, 0, 0)
    assert c.tolist() == [1.0, -4.0, 0.5, -0.5]                    # a seen token always loses: positive scores shrink, negative grow
    c = controlled_scores(x, [True, True, False, False], 0.5, None, None, 0, 0)
    assert c.tolist() == [4.0, -1.0, 0.5, -0.5]                    # theta < 1 rewards repetition


def test_theta_one_is_the_identity_and_zero_stays_zero():
    rng = np.random.Generator(np.random.PCG64(1))
    x = rng.standard_normal((3, 50))
    seen = rng.random((3, 50)) < 0.5
    assert np.array_equal(controlled_scores(x, seen, 1.0, None, None, 0, 0), x)
    assert np.array_equal(controlled_scores(x, seen, 1.0, np.zeros(50), None, 0, 0), x)
    z = controlled_scores(np.zeros(4), [True, False, True, False], 3.0, None, None, 0, 0)
    assert (z == 0).all()
    # in fp32, as the kernel forms it: x / 1 and x * 1 are x to the bit
    x32 = x.astype(np.float32)
    assert np.array_equal(np.where(x32 > 0, x32 / np.float32(1), x32 * np.float32(1)).view(np.uint32), x32.view(np.uint32))


def test_a_ban_and_a_bias():
    x = np.array([1.0, 2.0, 3.0])
    lb = np.array([0.5, -np.inf, -1.0])
    c = controlled_scores(x, [False, False, True], 2.0, lb, None, 0, 0)
    assert c.tolist() == [1.5, -np.inf, 0.5]                       # the penalty first, the bias on its result
    lo, hi = C.filtered_sets(c, 2, None)
    assert np.flatnonzero(lo).tolist() == [0, 2]


def test_eos_below_the_minimum_length_and_at_it():
    x = np.array([[1.0, 5.0, 2.0], [1.0, 5.0, 2.0], [1.0, 5.0, 2.0]])
    c = controlled_scores(x, np.zeros((3, 3), bool), 1.0, None, 1, 2, np.array([0, 1, 2]))
    assert c[0].tolist() == [1.0, -np.inf, 2.0] and c[1].tolist() == [1.0, -np.inf, 2.0]
    assert c[2].tolist() == [1.0, 5.0, 2.0]                        # at the minimum length eos is free
    assert np.array_equal(controlled_scores(x, np.zeros((3, 3), bool), 1.0, None, None, 0, 0), x)
    seen, length, fin = next_state(np.zeros((3, 3), bool), np.array([0, 1, 2]), np.array([0, 0, 1]), [2, 1, 0], 1)
    assert seen.tolist() == [[False, False, True], [False, True, False], [False, False, False]]
    assert length.tolist() == [1, 2, 2] and fin.tolist() == [0, 1, 1]       # eos counts in the length; a finished row does not move


# ---- the kernel-level cases of the GPU tests: seeded on the CPU, so the condition on the oracle's sets is checked here ----
SETTINGS = C.SETTINGS + ["off"]
THETA, EOS, MIN_LENGTH = 1.3, 7, 1


def setting(name, V):
    return (None, None) if name == "off" else C.setting(name, V)


def z_margin(tau, theta=THETA, base=1e-4):
    """fp32 against fp64 on the tempered controlled score: the score's own margin, scaled by what the penalty can multiply it by."""
    return base * max(theta, 1.0 / theta) / tau


@functools.lru_cache(maxsize=None)
def case_controls(B, H, V):
    """(seen (B, V) bool, logit_bias (V) fp32 with -inf entries): the draws in this order from PCG64(4242 + V).  theta = THETA,
    eos = EOS held back by min_length = MIN_LENGTH (every row's length is 0)."""
    rng = np.random.Generator(np.random.PCG64(4242 + V))
    seen = rng.random((B, V)) < 0.3
    lb = rng.standard_normal(V).astype(np.float32)
    lb[rng.random(V) < 0.1] = -np.inf
    return seen, lb


@functools.lru_cache(maxsize=None)
def case_controlled(B, H, V):
    """fp64 raw scores (B, V), controlled scores (B, V) and the sampler's noise G (B, V) of a kernel-level case."""
    scores, G = C.case_reference(B, H, V)
    seen, lb = case_controls(B, H, V)
    return scores, controlled_scores(scores, seen, THETA, lb, EOS, MIN_LENGTH, 0), G


@pytest.mark.parametrize("tau", C.TAUS)
@pytest.mark.parametrize("name", SETTINGS)
@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_controlled_kernel_cases_are_mostly_unambiguous(shape, name, tau):
    """Condition of the GPU test: at most 10 % of a case's rows may have different argmaxes over lo and hi."""
    _, c, G = case_controlled(*shape)
    k, p = setting(name, shape[2])
    share = C.ambiguous_share(c / tau, G, k, p, z_margin(tau))
    print(f"{shape} {name} tau {tau}: ambiguous share {share:.4f}")
    assert share <= 0.10


def test_the_cases_ban_tokens_and_hold_eos_back():
    for shape in C.SHAPES:
        seen, lb = case_controls(*shape)
        _, c, _ = case_controlled(*shape)
        assert np.isneginf(lb).any() and np.isfinite(lb).sum() > 2 and seen.any() and not seen.all()
        assert np.isneginf(c[:, EOS]).all() and (np.isneginf(c) == (np.isneginf(lb)[None, :] | (np.arange(shape[2]) == EOS)[None, :])).all()


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
def declared_functions():
    text = open(os.path.join(ROOT, "include", "vmlmf_decode.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vmlmf_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_function_is_exported_and_bound():
    from vmlmf_amd import _beam, _decode, _lib
    decl = declared_functions()
    assert decl == ["vmlmf_decode_abi_version", "vmlmf_decode_choose", "vmlmf_decode_last_error"]
    assert sorted(_decode.SYMBOLS) == decl
    assert os.path.exists(_decode.LIB_PATH), "run __graft_entry__.build() first"
    handle = ctypes.CDLL(_decode.LIB_PATH)
    for name in decl:
        assert hasattr(handle, name), f"missing export {name}"
    assert _decode.lib().vmlmf_decode_abi_version() == _decode.ABI_VERSION == 1
    assert not set(_decode.SYMBOLS) & (set(_lib.SYMBOLS) | set(_beam.SYMBOLS))   # the other libraries' ABIs are not touched
    main = ctypes.CDLL(_lib.LIB_PATH)
    assert not hasattr(main, "vmlmf_decode_choose")                              # the kernel lives in the new library only
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


@pytest.mark.parametrize("module, handle, name", [("_decode", "_handle", "libvmlmf_decode.so"), ("_lib", "_lib", "libvmlmf_hip.so")])
def test_a_missing_library_is_a_clear_error(monkeypatch, tmp_path, module, handle, name):
    import importlib
    binding = importlib.import_module("vmlmf_amd." + module)
    monkeypatch.setattr(binding, handle, None)
    monkeypatch.setattr(binding, "LIB_PATH", str(tmp_path / name))
    with pytest.raises(RuntimeError, match=name + " is missing: build it"):
        binding.lib()


def test_the_library_is_loaded_by_the_first_controlled_call_only():
    """A process that imports the package, opens the main library and walks a plain generate() call up to its refusal of CPU tensors
    has not opened libvmlmf_decode.so."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import torch, vmlmf_amd\nfrom vmlmf_amd import _decode, _lib\n_lib.lib()\n"
            "m = vmlmf_amd.Model(16, 8, 1, 0.0, 0.1, w_rank=4, u_ranks=[4], lstm_type='vmlmf')\n"
            "for kw in (dict(), dict(top_k=3), dict(eos=2, repetition_penalty=1.2)):\n"
            "    try:\n        m.generate(torch.zeros((3, 2), dtype=torch.int64), 4, **kw)\n"
            "    except RuntimeError as e:\n        assert 'cuda' in str(e)\n"
            "vmlmf_amd.DecodeControls(2, 16, 'cpu', eos=3)\n"
            "maps = open('/proc/self/maps').read()\n"
            "assert 'libvmlmf_hip.so' in maps and 'libvmlmf_decode.so' not in maps and not _decode.loaded()\n"
            "_decode.lib()\nassert 'libvmlmf_decode.so' in open('/proc/self/maps').read() and _decode.loaded()\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_the_makefile_builds_and_cleans_all_three_libraries():
    csrc = os.path.join(ROOT, "vmlmf_amd", "csrc")
    libs = ("libvmlmf_hip.so", "libvmlmf_beam.so", "libvmlmf_decode.so")
    r = subprocess.run(["make", "-n", "-B", "-C", csrc, "all"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and all(n in r.stdout for n in libs)
    link = [ln for ln in r.stdout.splitlines() if "-o ../lib/libvmlmf_hip.so" in ln]
    assert len(link) == 1 and "vmlmf_decode.o" not in link[0] and "vmlmf_sample.o" in link[0]    # not linked into the main library
    link = [ln for ln in r.stdout.splitlines() if "-o ../lib/libvmlmf_decode.so" in ln]
    assert len(link) == 1 and "vmlmf_decode.o" in link[0] and "vmlmf_sample.o" not in link[0]
    r = subprocess.run(["make", "-n", "-C", csrc, "clean"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and all(n in r.stdout for n in libs) and "vmlmf_decode.o" in r.stdout and "vmlmf_beam.o" in r.stdout


def test_the_selection_is_written_once():
    """Both translation units take the selection from one header; neither holds a copy of it."""
    csrc = os.path.join(ROOT, "vmlmf_amd", "csrc")
    header = open(os.path.join(csrc, "vmlmf_select.h")).read()
    for fn in ("best_merge", "lse_merge", "gumbel_of", "sample_key", "key_of", "z_of", "tempered", "radix_select", "tie_cutoff", "pick_row"):
        assert re.search(r"\b%s\s*\(" % fn, header), fn
    for name in ("vmlmf_sample.hip", "vmlmf_decode.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "vmlmf_select.h"' in text
        for fn in ("radix_select", "tie_cutoff", "best_merge", "lse_merge", "key_of"):
            assert not re.search(r"__device__[^;{]*\b%s\s*\(" % fn, text), (name, fn)
