"""CPU: the fp64 oracle of one beam-search step (step_sets), the conditions the GPU tests (tests/test_gpu_beam.py) rely on - checked on
the oracle alone -, and the host side of libvmlmf_beam.so (include/vmlmf_beam.h): exports, argument checks, the lazy load.

The rule a GPU step is judged by.  Of a batch row's candidates (flat index w V + v, fp64 total) and a margin m, step_sets returns the
exact first W of the total order (larger total first, equal totals to the lower flat index), `lo` - the candidates above the
(W + 1)-th total by more than m: whatever fp32 does, they must be kept - and `hi` - the candidates not below the W-th total by more
than m: nothing else may be kept.  A step passes when lo <= chosen <= hi and |chosen| = W; it is CLEAR when lo == hi, and then the
chosen set is the oracle's exactly."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS_KERNEL = 7
KERNEL_MARGIN = 1e-4     # the margin the filtered-sampling tests use on the same GEMM scores
KERNEL_CASES = [(3, 4, 32, 97), (5, 3, 40, 33), (2, 8, 700, 1000), (1, 16, 650, 10000), (1, 5, 16, 12293), (7, 1, 32, 97), (2, 32, 32, 97)]
MODEL_CASES = [("group", 3, 4, 11), ("plain", 3, 4, 13), ("plain", 2, 8, 11)]     # kind, B, W, prompt seed
MODEL_EOS, MODEL_STEPS = 3, 12


# ---- the oracle ----
def step_sets(totals, valid, W, m):
    """totals, valid (W, V): the fp64 totals of one batch row's candidates and which of them exist (a finished beam offers eos alone).
    Returns (top, lo, hi): top - the flat indices of the first W candidates, in order; lo, hi - sets of flat indices (see above)."""
    flat = np.flatnonzero(np.asarray(valid).ravel())
    t = np.asarray(totals, dtype=np.float64).ravel()[flat]
    assert len(flat) >= W and not np.isnan(t).any()
    order = np.lexsort((flat, -t))                       # by total, larger first; equal totals by flat index
    top = flat[order[:W]]
    t_w = t[order[W - 1]]
    t_next = t[order[W]] if len(flat) > W else -np.inf
    lo = set(flat[t > t_next + m].tolist())
    hi = set(flat[t >= t_w - m].tolist())
    assert lo <= set(top.tolist()) <= hi
    return top, lo, hi


def row_totals(x, cum, finished, eos):
    """x (W, V) fp64 scores with the bias, cum (W), finished (W) bool -> (totals (W, V), valid (W, V)) of one batch row."""
    lsm = torch.log_softmax(torch.as_tensor(x, dtype=torch.float64), -1).numpy()
    totals = np.asarray(cum, dtype=np.float64)[:, None] + lsm
    valid = np.ones(totals.shape, dtype=bool)
    for w in np.flatnonzero(np.asarray(finished)):
        if eos is not None:
            valid[w] = False
            valid[w, eos] = True
            totals[w, eos] = cum[w]
    return totals, valid


def kernel_case(B, W, H, V):
    """The prescribed fp32 inputs of a kernel-level case, and lengths of the test's own (1 .. 5)."""
    g = torch.Generator().manual_seed(1000 * B + V + W)
    h = torch.randn(B * W, H, generator=g)
    w = torch.randn(V, H, generator=g) * 0.1
    b = torch.randn(V, generator=g)
    cum = -3 * torch.rand(B, W, generator=g)
    finished = torch.rand(B, W, generator=g) < 0.25
    length = ((torch.arange(B * W) * 3) % 5 + 1).to(torch.int32).view(B, W)
    return h, w, b, cum, finished, length


_KERNEL_ORACLE = {}


def kernel_oracle(case, finished=None):
    """Per batch row (totals, valid, top, lo, hi) of a kernel-level case in fp64 (computed once per case)."""
    key = (case, None if finished is None else tuple(finished.reshape(-1).tolist()))
    if key not in _KERNEL_ORACLE:
        B, W, H, V = case
        h, w, b, cum, fin, _ = kernel_case(*case)
        fin = fin if finished is None else finished
        x = (h.double() @ w.double().t() + b.double()).view(B, W, V).numpy()
        rows = []
        for r in range(B):
            totals, valid = row_totals(x[r], cum[r].double().numpy(), fin[r].numpy(), EOS_KERNEL)
            rows.append((totals, valid) + step_sets(totals, valid, W, KERNEL_MARGIN))
        _KERNEL_ORACLE[key] = rows
    return _KERNEL_ORACLE[key]


def beam_model(kind):
    """The models of the model-level cases (CPU; winit 1.0: at the usual 0.3 the distribution is nearly uniform and the top-W boundary
    falls inside the margin), fc.b[3] raised so that eos = 3 is emitted by some beams and not by all."""
    from vmlmf_amd import Model
    if kind == "plain":
        torch.manual_seed(1)
        m = Model(97, 32, 2, 0.0, 1.0, w_rank=8, u_ranks=[8], lstm_type="vmlmf")
    else:
        torch.manual_seed(2)
        m = Model.with_group_layers(97, 32, 2, 0.0, 1.0, w_rank=8, u_ranks=[8, 8])
    with torch.no_grad():
        m.fc.b[MODEL_EOS] += 2.0
    return m


def cpu_prompt(B, T0=5, V=97, seed=0):
    """test_gpu_generate._prompt's draws, left on the CPU."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, V, (T0, B), generator=g)


def model_margin(j):
    from test_gpu_generate import LP_TOL, MARGIN
    return MARGIN + 2 * (j + 1) * LP_TOL


def oracle_last_scores(m, seqs):
    """fp64 literal forward over seqs (T, R) from zero states: the scores after the last token (R, V), and the final states."""
    from test_gpu_generate import _oracle_scores
    scores, states = _oracle_scores(m, seqs)
    return scores[-1].numpy(), states


def oracle_beam_search(m, prompt, W, steps, eos):
    """Beam search in fp64 along the oracle's own path (the literal layers over every hypothesis' whole prefix, step by step).
    Returns (clear: one bool per (step, batch row), finished (B, W) at the end, hyps (steps, B, W), cum (B, W))."""
    T0, B = prompt.shape
    hyps = np.zeros((0, B, W), dtype=np.int64)
    cum = np.full((B, W), -np.inf)
    cum[:, 0] = 0.0
    fin = np.zeros((B, W), dtype=bool)
    clear = []
    for j in range(steps):
        seqs = torch.cat([prompt[:, :, None].expand(T0, B, W), torch.from_numpy(hyps)]).reshape(T0 + j, B * W)
        x, _ = oracle_last_scores(m, seqs)
        x = x.reshape(B, W, -1)
        V = x.shape[-1]
        new_h, new_c, new_f = np.zeros((j + 1, B, W), dtype=np.int64), np.zeros((B, W)), np.zeros((B, W), dtype=bool)
        for b in range(B):
            totals, valid = row_totals(x[b], cum[b], fin[b], eos)
            top, lo, hi = step_sets(totals, valid, W, model_margin(j))
            clear.append(lo == hi)
            for r, f in enumerate(top):
                par, tok = divmod(int(f), V)
                new_h[:j, b, r], new_h[j, b, r] = hyps[:, b, par], tok
                new_c[b, r], new_f[b, r] = totals[par, tok], fin[b, par] or tok == eos
        hyps, cum, fin = new_h, new_c, new_f
    return clear, fin, hyps, cum


# ---- conditions on the oracle alone ----
@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_every_row_of_the_kernel_level_cases_is_clear(case):
    B, W, H, V = case
    rows = kernel_oracle(case)
    assert len(rows) == B
    for r, (totals, valid, top, lo, hi) in enumerate(rows):
        assert lo == hi == set(top.tolist()), (case, r, sorted(hi - lo))
        assert len(top) == W


def test_step_sets_orders_ties_by_flat_index_and_sees_the_margin():
    totals = np.array([[0.0, -1.0, -1.0, -5.0], [-1.0, -2.0, -1.00005, -9.0]])
    valid = np.ones((2, 4), dtype=bool)
    top, lo, hi = step_sets(totals, valid, 3, 1e-4)
    assert top.tolist() == [0, 1, 2]                    # the tie -1 = -1 = -1 over flat 1, 2, 4 goes to the lower indices
    assert lo == {0} and hi == {0, 1, 2, 4, 6}
    valid[1] = [False, False, True, False]              # a finished beam offers one token only
    top, lo, hi = step_sets(totals, valid, 3, 1e-6)
    assert top.tolist() == [0, 1, 2] and lo == hi == {0, 1, 2}
    totals[1, :] = -np.inf                              # a beam that does not exist yet loses to every finite candidate
    valid[:] = True
    top, lo, hi = step_sets(totals, valid, 4, 1e-4)
    assert top.tolist() == [0, 1, 2, 3] and lo == hi == {0, 1, 2, 3}


@pytest.mark.parametrize("kind,B,W,seed", MODEL_CASES)
def test_the_model_level_cases_are_mostly_clear_and_finish_some_beams(kind, B, W, seed):
    m = beam_model(kind)
    clear, fin, hyps, _ = oracle_beam_search(m, cpu_prompt(B, seed=seed), W, MODEL_STEPS, MODEL_EOS)
    assert len(clear) == MODEL_STEPS * B
    assert np.mean(clear) >= 0.9, (kind, B, W, int(np.sum(clear)), len(clear))
    assert 0 < fin.sum() < fin.size, (kind, B, W, int(fin.sum()))
    # a finished hypothesis is padded with eos
    for b in range(B):
        for w in range(W):
            hit = np.flatnonzero(hyps[:, b, w] == MODEL_EOS)
            assert fin[b, w] == (len(hit) > 0)
            if len(hit):
                assert (hyps[hit[0]:, b, w] == MODEL_EOS).all()


# ---- host-side checks ----
def test_beam_search_refuses_bad_beam_counts_before_anything_else():
    from vmlmf_amd import Model
    m = Model(97, 32, 2, 0.0, 0.1, w_rank=8, u_ranks=[8], lstm_type="vmlmf")
    prompt = torch.zeros((3, 2), dtype=torch.int64)
    for beams in (0, -1, 33, 98):
        with pytest.raises(ValueError, match="beams"):
            m.beam_search(prompt, 4, beams=beams)
    small = Model(5, 8, 1, 0.0, 0.1, w_rank=2, u_ranks=[2], lstm_type="vmlmf")
    with pytest.raises(ValueError, match="beams"):
        small.beam_search(prompt, 4, beams=6)                        # beams > V
    with pytest.raises(ValueError, match="eos"):
        m.beam_search(prompt, 4, eos=97)
    with pytest.raises(ValueError, match="chunk"):
        m.beam_search(prompt, 4, chunk=3)
    with pytest.raises(ValueError, match="length_penalty"):
        m.beam_search(prompt, 4, length_penalty=-1.0)
    with pytest.raises(RuntimeError, match="cuda"):                 # CPU tensors raise as in generate
        m.beam_search(prompt, 4)


def declared_functions():
    text = open(os.path.join(ROOT, "include", "vmlmf_beam.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vmlmf_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_function_is_exported_and_bound():
    from vmlmf_amd import _beam, _lib
    decl = declared_functions()
    assert len(decl) == 6 and all(n.startswith("vmlmf_beam_") for n in decl)
    assert sorted(_beam.SYMBOLS) == decl
    assert os.path.exists(_beam.LIB_PATH), "run __graft_entry__.build() first"
    handle = ctypes.CDLL(_beam.LIB_PATH)
    for name in decl:
        assert hasattr(handle, name), f"missing export {name}"
    assert _beam.lib().vmlmf_beam_abi_version() == _beam.ABI_VERSION == 1
    assert not set(_beam.SYMBOLS) & set(_lib.SYMBOLS)               # the main library's ABI is not touched
    main = ctypes.CDLL(_lib.LIB_PATH)
    assert not hasattr(main, "vmlmf_beam_step")                      # the kernels live in the second library only


def test_workspace_bytes():
    from vmlmf_amd import _beam
    ws = _beam.lib().vmlmf_beam_workspace_bytes
    assert ws(2, 4, 97) == 2 * 4 * 4 * 8 and ws(1, 1, 10000) == 8 and ws(32, 32, 10000) == 32 * 32 * 32 * 8
    assert ws(1, 16, 10 ** 8) == 16 * 16 * 8                         # any row length
    for bad in ((0, 4, 97), (2, 0, 97), (2, 33, 97), (2, 4, 3), (2, 4, 0), (1, 32, 2 ** 26)):
        assert ws(*bad) == 0, bad


def test_the_entry_points_refuse_bad_arguments_without_touching_the_gpu():
    from vmlmf_amd import _beam, _lib
    lib = _beam.lib()
    one = ctypes.c_void_p(16)                                        # never dereferenced: every call below is refused first
    good = dict(B=2, W=4, H=32, V=97, eos=7, ws=256)

    out = ctypes.c_void_p(32)

    def step(B=2, W=4, H=32, V=97, eos=7, ws=256, scores=one, embed=one, x_next=out, total=out, cum=one, workspace=one):
        return lib.vmlmf_beam_step(B, W, H, V, scores, one, cum, one, one, eos, embed, out, out, total, out, out, x_next, out, one,
                                   workspace, ws, None)

    for kw, word in ((dict(B=0), b">= 1"), (dict(W=0), b"beams"), (dict(W=33), b"beams"), (dict(W=4, V=3, eos=-1), b"exceed V"),
                     (dict(eos=97), b"eos"), (dict(eos=-2), b"eos"), (dict(scores=None), b"null"), (dict(embed=None), b"together"),
                     (dict(x_next=None), b"together"), (dict(total=one, cum=one), b"alias"), (dict(workspace=ctypes.c_void_p(12)), b"aligned"),
                     (dict(W=32, V=2 ** 26, eos=-1), b"2^31")):
        assert step(**kw) == _lib.E_BADARG, kw
        assert word in lib.vmlmf_beam_last_error(), (kw, lib.vmlmf_beam_last_error())
    assert step(ws=255) == _lib.E_WORKSPACE and b"workspace" in lib.vmlmf_beam_last_error()
    assert good["ws"] == lib.vmlmf_beam_workspace_bytes(2, 4, 97)
    two = (ctypes.c_void_p * 2)(16, 32)
    other = (ctypes.c_void_p * 2)(48, 64)
    for args, word in (((0, 8, 32, one, two, other, None), b"n must"), ((17, 8, 32, one, two, other, None), b"n must"),
                       ((2, 0, 32, one, two, other, None), b">= 1"), ((2, 8, 32, None, two, other, None), b"null"),
                       ((2, 8, 32, one, two, (ctypes.c_void_p * 2)(48, 16), None), b"also a source"),
                       ((2, 8, 32, one, two, (ctypes.c_void_p * 2)(48, 0), None), b"null")):
        assert lib.vmlmf_beam_gather(*args) == _lib.E_BADARG, args
        assert word in lib.vmlmf_beam_last_error(), (args, lib.vmlmf_beam_last_error())
    for args, word in (((0, 2, 4, one, one, None, one, None), b"steps"), ((3, 2, 33, one, one, None, one, None), b"beams"),
                       ((3, 2, 4, None, one, None, one, None), b"null"), ((3, 2, 4, one, one, None, None, None), b"null")):
        assert lib.vmlmf_beam_backtrack(*args) == _lib.E_BADARG, args
        assert word in lib.vmlmf_beam_last_error(), (args, lib.vmlmf_beam_last_error())
    with pytest.raises(_lib.VmlmfError) as ei:
        _beam.check(step(W=33))
    assert ei.value.code == _lib.E_BADARG and "beams" in str(ei.value)


def test_a_missing_library_is_a_clear_error(monkeypatch, tmp_path):
    from vmlmf_amd import _beam
    monkeypatch.setattr(_beam, "_handle", None)
    monkeypatch.setattr(_beam, "LIB_PATH", str(tmp_path / "libvmlmf_beam.so"))
    with pytest.raises(RuntimeError, match="libvmlmf_beam.so is missing: build it"):
        _beam.lib()


def test_the_library_is_loaded_by_the_first_beam_call_only():
    """A process that imports the package and opens the main library has not opened libvmlmf_beam.so."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import vmlmf_amd\nfrom vmlmf_amd import _beam, _lib\n_lib.lib()\n"
            "maps = open('/proc/self/maps').read()\n"
            "assert 'libvmlmf_hip.so' in maps and 'libvmlmf_beam.so' not in maps and not _beam.loaded()\n"
            "_beam.lib()\nassert 'libvmlmf_beam.so' in open('/proc/self/maps').read() and _beam.loaded()\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_the_makefile_builds_and_cleans_both_libraries():
    csrc = os.path.join(ROOT, "vmlmf_amd", "csrc")
    r = subprocess.run(["make", "-n", "-B", "-C", csrc, "all"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "libvmlmf_hip.so" in r.stdout and "libvmlmf_beam.so" in r.stdout
    link = [ln for ln in r.stdout.splitlines() if "-o ../lib/libvmlmf_hip.so" in ln]
    assert len(link) == 1 and "vmlmf_beam.o" not in link[0] and "vmlmf_sample.o" in link[0]      # not linked into the main library
    r = subprocess.run(["make", "-n", "-C", csrc, "clean"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "libvmlmf_hip.so" in r.stdout and "libvmlmf_beam.so" in r.stdout and "vmlmf_beam.o" in r.stdout
