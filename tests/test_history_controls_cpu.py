"""History controls of Model.generate (no_repeat_ngram_size, banned_sequences, frequency_penalty, presence_penalty; C ABI
vmlmf_history_choose / vmlmf_history_bans in libvmlmf_history.so, include/vmlmf_history.h): what can be checked without a GPU, beside
the table test_side_libraries_cpu.py holds every side library to - the two statements of the ban set (history_cases.py) against each
other; the condition on the reference's sets that the GPU test of the choice relies on; every
refusal, in Python and at the C ABI; the struct of the binding."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import history_cases as HC
import vmlmf_decode_oracle as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vmlmf_amd", "csrc")


def test_the_widest_vocabulary_is_the_headers():
    from vmlmf_amd import _history
    header = open(os.path.join(ROOT, "include", "vmlmf_history.h")).read()
    assert int(re.search(r"#define VMLMF_HISTORY_MAX_V (\d+)", header).group(1)) == _history.MAX_V


# ---- the two statements of the ban set ----
def test_the_two_ban_sets_agree_on_the_edges():
    for n, seqs, hists in HC.EDGES:
        for h in hists:
            a, b = HC.ban_set(h, HC.EDGE_V, n, seqs), HC.ban_set_by_dictionary(h, HC.EDGE_V, n, seqs)
            assert np.array_equal(a, b), (n, seqs, h)
    f = lambda h, n, seqs=(): np.flatnonzero(HC.ban_set(h, HC.EDGE_V, n, list(seqs))).tolist()
    assert f([], 3) == f([4], 3) == f([4, 5], 3) == f([4, 5, 4], 3) == []                      # L = 0, n - 2, n - 1; n without a match
    assert f([4, 5, 6, 4, 5], 3) == [6] and f([4, 5, 6, 4, 5, 7, 4, 5], 3) == [6, 7]
    assert f([9, 3, 9, 96], 1) == [3, 9, 96] and f([], 1) == []                                # n = 1: every token of the history
    assert f([1, 2, 3], 5) == f([1, 2, 3, 4], 5) == []                                         # n > L + 1, n = L + 1
    assert f([1, 2, 3, 4, 1, 2, 3, 4], 5) == [1] and f([1, 2, 3, 4, 9, 1, 2, 3, 4], 5) == [9]
    assert f([8, 8, 8], 2) == [8] and f([8], 2) == [] and f([8, 8], 2) == [8]                  # a a a: overlapping matches count
    seqs = ([7, 8, 9, 10], [11], [5, 6])
    assert f([7], 0, seqs) == [11] and f([7, 8, 9], 0, seqs) == [10, 11] and f([5], 0, seqs) == [6, 11] and f([], 0, seqs) == [11]


def test_the_two_ban_sets_agree_on_the_kernel_cases_and_on_random_histories():
    for shape in C.SHAPES:
        hist, count, seqs = HC.case_history(*shape)
        assert hist.shape == (shape[0], HC.HIST_LEN) and (count.sum(1) == HC.HIST_LEN - HC.PROMPT_LEN).all()
        bans = HC.case_bans(*shape)
        for r, row in enumerate(hist):
            assert np.array_equal(bans[r], HC.ban_set_by_dictionary(row, shape[2], HC.N_GRAM, seqs))
        assert bans[:, seqs[1][0]].all()                                                       # the one-token sequence, in every row
        if shape[0] > 1:
            assert (bans.sum(1) >= 2).any()                                                    # ... and an n-gram or a longer sequence
    rng = np.random.Generator(np.random.PCG64(5))
    for _ in range(300):
        n, L = int(rng.integers(0, 5)), int(rng.integers(0, 14))
        h = rng.integers(0, 4, L).tolist()
        seqs = [rng.integers(0, 4, int(rng.integers(1, 4))).tolist() for _ in range(int(rng.integers(0, 3)))]
        assert np.array_equal(HC.ban_set(h, 6, n, seqs), HC.ban_set_by_dictionary(h, 6, n, seqs)), (n, h, seqs)


def test_the_scores():
    x = np.array([2.0, -2.0, 0.5, -0.5, 1.0])
    c = HC.history_scores(x, [True, True, False, False, False], [3, 0, 1, 0, 0], 2.0, 0.25, 0.5, np.array([0.0, 0.0, 1.0, 0.0, 0.0]), 3, 1, 0,
                          [False, False, False, False, True])
    assert c.tolist() == [1.0 - 0.75 - 0.5, -4.0, 0.5 - 0.25 - 0.5 + 1.0, -np.inf, -np.inf]
    rng = np.random.Generator(np.random.PCG64(2))
    x = rng.standard_normal((3, 40))
    seen, count = rng.random((3, 40)) < 0.5, rng.integers(0, 5, (3, 40))
    lb = rng.standard_normal(40)
    assert np.array_equal(HC.history_scores(x, seen, count, 1.3, 0.0, 0.0, lb, 7, 1, 0, np.zeros((3, 40), bool)),
                          C.controlled_scores(x, seen, 1.3, lb, 7, 1, 0))                     # neutral: the controlled scores
    # in fp32, as the kernel forms it: (r - 0 * count) - 0 is r to the bit
    r32 = x.astype(np.float32)
    q32 = (r32 - np.float32(0) * count.astype(np.float32)) - np.float32(0)
    assert np.array_equal(q32.view(np.uint32), r32.view(np.uint32))
    hist, cnt = HC.next_history([[1], [2]], np.array([[0, 65535, 0], [0, 0, 7]]), [0, 1], [1, 2])
    assert hist == [[1, 1], [2]] and cnt.tolist() == [[0, 65535, 0], [0, 0, 7]]               # saturated; a finished row does not move
    words = np.array([[1 | (1 << 31), 2]], dtype=np.uint32).astype(np.int32)
    assert np.flatnonzero(HC.unpack(words, 40)[0]).tolist() == [0, 31, 33]


# ---- the condition of the GPU test of the choice, on the reference alone ----
@pytest.mark.parametrize("tau", C.TAUS)
@pytest.mark.parametrize("name", C.CONTROL_SETTINGS)
@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_history_kernel_cases_are_mostly_unambiguous(shape, name, tau):
    """At most 10 % of a case's rows may have different argmaxes over lo and hi (measured: at most 1 row of 19).  The margin is
    z_margin(tau): the penalty terms are exact to an fp32 ulp of a score of order 1 to 10, three orders below its base of 1e-4."""
    _, c, G, bans = HC.case_scores(*shape)
    k, p = C.control_setting(name, shape[2])
    share = C.ambiguous_share(c / tau, G, k, p, C.z_margin(tau))
    print(f"{shape} {name} tau {tau}: ambiguous share {share:.4f}")
    assert share <= 0.10
    assert np.isneginf(c[bans]).all() and np.isfinite(c).sum(1).min() >= 2


# ---- every refusal ----
REFUSALS = [
    (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"), (dict(no_repeat_ngram_size=1.5), "no_repeat_ngram_size"),
    (dict(no_repeat_ngram_size="two"), "no_repeat_ngram_size"),
    (dict(frequency_penalty=-0.1), "frequency_penalty"), (dict(frequency_penalty=float("inf")), "frequency_penalty"),
    (dict(frequency_penalty=float("nan")), "frequency_penalty"), (dict(frequency_penalty="x"), "frequency_penalty"),
    (dict(presence_penalty=-1.0), "presence_penalty"), (dict(presence_penalty=float("inf")), "presence_penalty"),
    (dict(presence_penalty=float("nan")), "presence_penalty"),
    (dict(banned_sequences=[[1, 2], []]), "empty sequence"), (dict(banned_sequences=[[1, 64]]), "banned sequence token 64"),
    (dict(banned_sequences=[[-1]]), "banned sequence token -1"), (dict(banned_sequences=[3]), "list of lists"),
    (dict(banned_sequences=[[1] * 4097]), "more than 4096"),
]


@pytest.mark.parametrize("kw,words", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_check_history_history_controls_and_generate_refuse(kw, words):
    from vmlmf_amd import HistoryControls, Model, _history
    with pytest.raises(ValueError, match=words):
        _history.check_history(64, **kw)
    with pytest.raises(ValueError, match=words):
        HistoryControls(2, 64, "cpu", **kw)
    torch.manual_seed(0)
    m = Model(64, 8, 1, 0.0, 0.1, w_rank=4, u_ranks=[4], lstm_type="vmlmf")
    with pytest.raises(ValueError, match=words):                          # before the refusal of CPU tensors
        m.generate(torch.zeros((3, 2), dtype=torch.int64), 4, **kw)


def test_the_room_for_a_choice_and_the_widest_vocabulary():
    from vmlmf_amd import HistoryControls, Model, _history
    ok = dict(no_repeat_ngram_size=2, banned_sequences=[[1, 2], [3]])
    assert _history.check_history(64, prompt_length=5, steps=10, closed=3, **ok) == (2, [[1, 2], [3]], 0.0, 0.0)
    _history.check_history(22, prompt_length=5, steps=10, closed=3, **ok)            # 22 > 3 + 5 + 10 + 2 + 1
    for kw in (ok, dict(no_repeat_ngram_size=1), dict(banned_sequences=[[0]])):
        need = 3 + 5 + 10 + len(kw.get("banned_sequences", [])) + 1
        with pytest.raises(ValueError, match="might leave no token to choose"):
            _history.check_history(need, prompt_length=5, steps=10, closed=3, **kw)
        _history.check_history(need + 1, prompt_length=5, steps=10, closed=3, **kw)
    _history.check_history(8, frequency_penalty=1.0, presence_penalty=1.0, prompt_length=5, steps=100)      # the penalties close nothing
    with pytest.raises(ValueError, match="at most 65536"):
        _history.check_history(65537, no_repeat_ngram_size=2)
    _history.check_history(65537, frequency_penalty=0.5)                               # ... and carry no limit
    _history.check_history(65536, no_repeat_ngram_size=2)
    torch.manual_seed(0)
    m = Model(16, 8, 1, 0.0, 0.1, w_rank=4, u_ranks=[4], lstm_type="vmlmf")
    prompt = torch.zeros((3, 2), dtype=torch.int64)
    with pytest.raises(ValueError, match="might leave no token to choose"):
        m.generate(prompt, 12, no_repeat_ngram_size=2)                                   # 16 <= 3 + 12 + 1
    with pytest.raises(ValueError, match="might leave no token to choose"):
        m.generate(prompt, 8, no_repeat_ngram_size=2, banned_tokens=[1, 2], eos=3, min_length=1, banned_sequences=[[4, 5]])
    with pytest.raises(RuntimeError, match="cuda"):
        m.generate(prompt, 11, no_repeat_ngram_size=2)
    with pytest.raises(ValueError, match="capacity"):
        HistoryControls(2, 16, "cpu", prompt=prompt, capacity=2)
    with pytest.raises(ValueError, match="repetition_penalty"):                         # DecodeControls' refusals are as they were
        HistoryControls(2, 16, "cpu", no_repeat_ngram_size=2, repetition_penalty=0.0)
    assert not _history.history_on() and not _history.history_on(0, None, 0.0, 0.0)
    assert _history.history_on(2) and _history.history_on(banned_sequences=[]) and _history.history_on(frequency_penalty=0.1)
    assert _history.history_on(presence_penalty=0.1)


def test_history_controls_is_exported_as_a_decode_controls():
    import vmlmf_amd
    assert "HistoryControls" in vmlmf_amd.__all__ and issubclass(vmlmf_amd.HistoryControls, vmlmf_amd.DecodeControls)


def test_history_controls_accepts_and_clones_all_its_state():
    from vmlmf_amd import HistoryControls
    c = HistoryControls(2, 16, "cpu", no_repeat_ngram_size=3, banned_sequences=[[1, 2], (3,)], frequency_penalty=0.5, presence_penalty=0.25,
                        eos=3, min_length=1, repetition_penalty=1.2, banned_tokens=[4], prompt=torch.tensor([[0, 5], [2, 5], [0, 15]]), capacity=7)
    assert (c.no_repeat_ngram_size, c.sequences, c.frequency_penalty, c.presence_penalty, c.capacity) == (3, [[1, 2], [3]], 0.5, 0.25, 7)
    assert c.hist.dtype == torch.int32 and c.hist.tolist() == [[0, 2, 0, 0, 0, 0, 0], [5, 5, 15, 0, 0, 0, 0]] and c.hist_len.tolist() == [3, 3]
    assert c.count.dtype == torch.uint16 and tuple(c.count.shape) == (2, 16) and not c.count.view(torch.int16).any()   # the prompt is not counted
    assert c.overflow.dtype == torch.int32 and not c.overflow.any()
    assert c.seq_tokens.tolist() == [1, 2, 3] and c.seq_offsets.tolist() == [0, 2, 3]
    assert c.seen.nonzero().tolist() == [[0, 0], [0, 2], [1, 5], [1, 15]] and c.eos == 3 and torch.isneginf(c.logit_bias[4])
    d = c.clone()
    assert type(d) is HistoryControls
    for name in HistoryControls.STATE:
        assert getattr(d, name).data_ptr() != getattr(c, name).data_ptr() and torch.equal(getattr(d, name), getattr(c, name)), name
    assert d.seq_tokens is c.seq_tokens and d.logit_bias is c.logit_bias
    e = HistoryControls(2, 16, "cpu", frequency_penalty=0.5)
    assert e.seq_tokens is None and e.capacity == 1024 and e.hist_len.tolist() == [0, 0]
    s = c.struct()
    assert (s.no_repeat_ngram_size, s.hist_capacity, s.n_sequences, s.eos, s.min_length) == (3, 7, 2, 3, 1)
    assert s.hist == c.hist.data_ptr() and s.count == c.count.data_ptr() and s.seq_offsets == c.seq_offsets.data_ptr()


# ---- the struct and the entry points' refusals on the host ----
def test_the_controls_struct_is_the_headers():
    from vmlmf_amd import _decode, _history
    names = [f[0] for f in _history.Controls._fields_]
    assert names[:8] == [f[0] for f in _decode.Controls._fields_]                       # the decode struct, field for field ...
    for f in _decode.Controls._fields_:
        assert getattr(_history.Controls, f[0]).offset == getattr(_decode.Controls, f[0]).offset
    assert names[8:] == ["no_repeat_ngram_size", "frequency_penalty", "presence_penalty", "pad1", "hist", "hist_len", "hist_capacity", "pad2",
                         "count", "overflow", "seq_tokens", "seq_offsets", "n_sequences", "pad3"]
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vmlmf_history.h")).read(), flags=re.S)
    body = re.search(r"typedef struct vmlmf_history_controls \{(.*?)\} vmlmf_history_controls;", header, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == names                                          # ... in the header's order
    vp = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_history.Controls) == ctypes.sizeof(_decode.Controls) + 16 + 2 * vp + 8 + 4 * vp + 8


def _controls(theta=1.0, eos=-1, min_length=0, seen=1, finished=1, length=1, n=0, alpha=0.0, beta=0.0, hist=1, hist_len=1, capacity=8,
              count=1, overflow=1, seq_tokens=None, seq_offsets=None, n_sequences=0):
    from vmlmf_amd import _history
    return _history.Controls(theta, eos, min_length, 0, None, seen, finished, length, n, alpha, beta, 0, hist, hist_len, capacity, 0, count,
                             overflow, seq_tokens, seq_offsets, n_sequences, 0)


def _choose(B=2, H=8, V=16, scores=1, inv=1.0, top_k=0, top_p=1.0, state=1, step=0, tokens=1, xn=None, embed=None, controls=True, **kw):
    """vmlmf_history_choose with fake, never dereferenced pointers (1 = some non-null address): refusals come before any launch."""
    from vmlmf_amd import _history
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    lib = _history.lib()
    c = _controls(**kw)
    rc = lib.vmlmf_history_choose(B, H, V, p(scores), None, p(embed), inv, top_k, top_p, p(state), step, ctypes.byref(c) if controls else None,
                                  p(tokens), None, p(xn), None, None)
    return rc, lib.vmlmf_history_last_error().decode()


def test_the_entry_points_refuse_on_the_host():
    from vmlmf_amd import _history, _lib
    bad = _lib.E_BADARG
    cases = [
        # what vmlmf_decode_choose refuses
        (dict(seen=None), bad, "seen"), (dict(finished=None), bad, "finished"), (dict(length=None), bad, "length"),
        (dict(controls=False), bad, "null controls"), (dict(eos=16), bad, "eos"), (dict(eos=-2), bad, "eos"),
        (dict(theta=0.0), bad, "repetition_penalty"), (dict(theta=float("nan")), bad, "repetition_penalty"),
        (dict(theta=float("inf")), bad, "repetition_penalty"), (dict(eos=3, min_length=-1), bad, "min_length"),
        (dict(min_length=1), bad, "min_length needs eos"), (dict(B=0), bad, "B, "), (dict(V=-3), bad, "B, "), (dict(scores=None), bad, "null"),
        (dict(tokens=None), bad, "null"), (dict(inv=-1.0), bad, "temperature"), (dict(inv=float("nan")), bad, "temperature"),
        (dict(state=None), bad, "snapshot"), (dict(xn=1, embed=None), bad, "embedding"), (dict(step=-1), bad, "step"),
        (dict(top_k=-1), bad, "top_k"), (dict(top_p=0.0), bad, "top_p"), (dict(top_p=1.5), bad, "top_p"),
        (dict(B=1 << 16, step=1 << 16), _lib.E_UNSUPPORTED, "2^32"),
        # ... and the history's own
        (dict(n=-1), bad, "no_repeat_ngram_size"), (dict(alpha=-0.5), bad, "frequency_penalty"), (dict(alpha=float("inf")), bad, "frequency_penalty"),
        (dict(alpha=float("nan")), bad, "frequency_penalty"), (dict(beta=-0.5), bad, "presence_penalty"),
        (dict(beta=float("inf")), bad, "presence_penalty"), (dict(beta=float("nan")), bad, "presence_penalty"),
        (dict(n=2, hist=None), bad, "hist"), (dict(n=2, hist_len=None), bad, "hist_len"), (dict(n=2, overflow=None), bad, "overflow"),
        (dict(n_sequences=1, seq_tokens=1, seq_offsets=1, hist=None), bad, "hist"),
        (dict(alpha=0.5, count=None), bad, "count"), (dict(beta=0.5, count=None), bad, "count"),
        (dict(capacity=0), bad, "hist_capacity"), (dict(n_sequences=-1), bad, "n_sequences"),
        (dict(n_sequences=2, seq_tokens=None, seq_offsets=1), bad, "seq_tokens"), (dict(n_sequences=2, seq_tokens=1, seq_offsets=None), bad, "seq_tokens"),
        (dict(V=65537, n=2), bad, "VMLMF_HISTORY_MAX_V"), (dict(V=65537, n_sequences=1, seq_tokens=1, seq_offsets=1), bad, "VMLMF_HISTORY_MAX_V"),
    ]
    for kw, code, words in cases:
        rc, msg = _choose(**kw)
        assert rc == code and words in msg and msg.startswith("vmlmf_history_choose: "), (kw, rc, msg)
    lib = _history.lib()
    p = ctypes.c_void_p
    for kw, B, V, out, words in [(dict(), 0, 16, 1, "B and V"), (dict(), 2, 0, 1, "B and V"), (None, 2, 16, 1, "null controls"),
                                 (dict(), 2, 16, None, "bitmap"), (dict(hist=None), 2, 16, 1, "hist"), (dict(hist_len=None), 2, 16, 1, "hist_len"),
                                 (dict(n=-1), 2, 16, 1, "no_repeat_ngram_size"), (dict(capacity=0), 2, 16, 1, "hist_capacity"),
                                 (dict(n_sequences=-1), 2, 16, 1, "n_sequences"), (dict(n_sequences=1), 2, 16, 1, "seq_tokens"),
                                 (dict(eos=16), 2, 16, 1, "eos"), (dict(n=2), 2, 65537, 1, "VMLMF_HISTORY_MAX_V")]:
        c = None if kw is None else _controls(**kw)
        rc = lib.vmlmf_history_bans(B, V, None if c is None else ctypes.byref(c), None if out is None else p(out), None)
        msg = lib.vmlmf_history_last_error().decode()
        assert rc == bad and words in msg and msg.startswith("vmlmf_history_bans: "), (kw, rc, msg)


def _static_lds(library, tools):
    """{kernel: static LDS bytes} from the metadata of a library's gfx950 code object."""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "gfx950.co")
        subprocess.run([tools[0], "--dump-section", ".hip_fatbin=" + fat, library, os.path.join(tmp, "copy.so")], check=True)
        subprocess.run([tools[1], "--unbundle", "--type=o", "--input=" + fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co],
                       check=True)
        notes = subprocess.run([tools[2], "--notes", co], check=True, capture_output=True, text=True).stdout
    lds = {}
    for block in notes.split(".args:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        lds[name] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
    return lds


def test_the_kernels_static_lds_fits_and_is_what_the_header_says():
    """The code objects' metadata: history_choose_kernel holds the selection's scratch and the bitmap of VMLMF_HISTORY_MAX_V bits in
    static LDS, at most 64 KB; history_bans_kernel the bitmap alone; libvmlmf_decode.so's one kernel, decode_choose_kernel, the scratch
    alone."""
    from vmlmf_amd import _decode, _history
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("no LLVM binary tools beside hipcc")
    lds = _static_lds(_history.LIBRARY.path, tools)
    choose = [v for k, v in lds.items() if "history_choose_kernel" in k]
    bans = [v for k, v in lds.items() if "history_bans_kernel" in k]
    assert len(lds) == 2 and len(choose) == 1 and len(bans) == 1, lds
    bitmap = _history.MAX_V // 8
    assert bans[0] == bitmap and bitmap < choose[0] <= 65536, lds
    assert choose[0] - bitmap >= 12288 * 4                                               # ... beside the keys of the longest resident row
    decode = _static_lds(_decode.LIBRARY.path, tools)
    assert len(decode) == 1 and "decode_choose_kernel" in list(decode)[0], decode
    assert list(decode.values()) == [choose[0] - bitmap], (decode, lds)                  # the decode kernel carries no bitmap
