"""The decoder's side libraries - libvmlmf_<name>.so for the eleven names of the Makefile's SIDE and of _lib.SIDE, each with a header, an
ABI version and a binding of its own (vmlmf_amd/_<name>.py: one _lib.Library each) - held to one table: what the header declares is
bound and exported, and by that library alone; a missing file is a clear error; a library is opened by its own first call only; the
Makefile links each from its own object, by one rule, and cleans all of them; the selection is written once, in vmlmf_select.h.
What is specific to one library (its struct, its limits, its refusals) is in that library's own test file."""
import ctypes
import importlib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vmlmf_amd", "csrc")


def side(name, functions, no_fallback, deps=()):
    """A row: functions - what the header declares, sorted; deps - what the Makefile's line of the object names, besides vmlmf_side.h
    and the library's own header (which every row is held to)."""
    return dict(name=name, header="vmlmf_%s.h" % name, module="_" + name, file="libvmlmf_%s.so" % name, obj="vmlmf_%s.o" % name,
                abi_macro="VMLMF_%s_ABI_VERSION" % name.upper(), functions=["vmlmf_%s_%s" % (name, f) for f in functions],
                no_fallback="no stock-op fallback for " + no_fallback, deps=list(deps))


SIDE = [
    side("beam", ["abi_version", "backtrack", "gather", "last_error", "step", "workspace_bytes"], "the beam-search step"),
    side("decode", ["abi_version", "choose", "last_error"], "the controlled choice of Model.generate",
         ["vmlmf_controlled.h"]),           # the controlled rows are written once, for the decode, truncate and automaton libraries
    side("score", ["abi_version", "last_error", "rows"], "Model.score"),
    side("history", ["abi_version", "bans", "choose", "last_error"], "the history controls of Model.generate"),
    side("beamctl", ["abi_version", "last_error", "step", "workspace_bytes"], "the controlled beam-search step"),
    side("truncate", ["abi_version", "choose", "last_error"], "the truncation samplers of Model.generate",
         ["vmlmf_refusals.h", "vmlmf_select.h", "vmlmf_controlled.h", "vmlmf_truncate.h", "vmlmf_dropout.h", "../../include/vmlmf_decode.h"]),
    side("automaton", ["abi_version", "beam_step", "choose", "last_error", "workspace_bytes"], "decoding under a token automaton",
         ["vmlmf_refusals.h", "vmlmf_select.h", "vmlmf_controlled.h", "vmlmf_beam_core.h", "vmlmf_dropout.h", "../../include/vmlmf_beam.h",
          "../../include/vmlmf_decode.h"]),
    side("beamgroup", ["abi_version", "last_error", "step", "workspace_bytes"], "the group beam-search step",
         ["vmlmf_beam_core.h", "../../include/vmlmf_beam.h"]),
    side("contrast", ["abi_version", "append", "choose", "last_error", "workspace_bytes"], "the contrastive-search step"),
    side("ncache", ["abi_version", "last_error", "score", "workspace_bytes"], "the continuous-cache scoring"),
    side("sbeam", ["abi_version", "last_error", "step", "workspace_bytes"], "the stochastic beam-search step",
         ["vmlmf_beam_core.h", "vmlmf_select.h", "vmlmf_dropout.h", "../../include/vmlmf_beam.h"]),
]
MAIN = dict(module="_lib", file="libvmlmf_hip.so", no_fallback="no CPU / PyTorch fallback for the hot path")
IDS = [row["module"] for row in SIDE]
MAKEFILE = open(os.path.join(CSRC, "Makefile")).read()


def binding(row):
    return importlib.import_module("vmlmf_amd." + row["module"])


def path_of(row):
    b = binding(row)
    return b.LIB_PATH if row is MAIN else b.LIBRARY.path


def declared_functions(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vmlmf_[a-z0-9_]+)\s*\(", text)))


# ---- a. declarations, exports and ABI numbers ----
@pytest.mark.parametrize("row", SIDE, ids=IDS)
def test_every_declared_function_is_exported_and_bound(row):
    b = binding(row)
    prefix = row["file"][len("lib"):-len(".so")] + "_"
    assert declared_functions(row["header"]) == sorted(b.SYMBOLS) == row["functions"]
    assert len(row["functions"]) >= 3 and all(n.startswith(prefix) for n in row["functions"])
    assert os.path.exists(path_of(row)), "run __graft_entry__.build() first"
    handle = ctypes.CDLL(path_of(row))
    for name in row["functions"]:
        assert hasattr(handle, name), f"missing export {name}"
    header = open(os.path.join(ROOT, "include", row["header"])).read()
    in_header = int(re.search(r"#define %s (\d+)" % row["abi_macro"], header).group(1))
    assert b.LIBRARY.abi_symbol == prefix + "abi_version" and b.LIBRARY.error_symbol == prefix + "last_error"
    assert in_header == b.ABI_VERSION == b.LIBRARY.abi_version == getattr(b.lib(), b.LIBRARY.abi_symbol)() == 1
    assert os.path.basename(b.LIBRARY.path) == row["file"] and "no " + b.LIBRARY.no_fallback == row["no_fallback"]
    source = open(os.path.join(CSRC, row["obj"][:-2] + ".hip")).read()       # the scaffold of vmlmf_side.h: ABI number and last error
    assert "VMLMF_SIDE_LIBRARY(vmlmf_%s, %s)" % (row["name"], row["abi_macro"]) in source


def test_the_makefile_the_package_and_this_table_name_the_same_libraries():
    from vmlmf_amd import _lib
    in_makefile = re.search(r"^SIDE := (.*)$", MAKEFILE, flags=re.M).group(1).split()
    assert in_makefile == list(_lib.SIDE) == [row["name"] for row in SIDE] and len(set(in_makefile)) == len(SIDE) == 11


def test_the_abis_are_disjoint_and_no_library_exports_anothers_entry_points():
    rows = [MAIN] + SIDE
    symbols = {row["module"]: set(binding(row).SYMBOLS) for row in rows}
    for i, a in enumerate(rows):
        for b in rows[i + 1:]:
            assert not symbols[a["module"]] & symbols[b["module"]], (a["module"], b["module"])
    for row in rows:                                                     # a kernel lives in its own library only
        handle = ctypes.CDLL(path_of(row))
        for other in rows:
            if other is not row:
                for name in sorted(symbols[other["module"]]):
                    assert not hasattr(handle, name), (row["file"], name)


# ---- b. a missing file ----
@pytest.mark.parametrize("row", SIDE + [MAIN], ids=IDS + ["_lib"])
def test_a_missing_library_is_a_clear_error(monkeypatch, tmp_path, row):
    b = binding(row)
    missing = str(tmp_path / row["file"])
    if row is MAIN:
        monkeypatch.setattr(b, "_lib", None)
        monkeypatch.setattr(b, "LIB_PATH", missing)
    else:
        monkeypatch.setattr(b.LIBRARY, "_handle", None)
        monkeypatch.setattr(b.LIBRARY, "path", missing)
    with pytest.raises(RuntimeError, match=row["file"] + " is missing: build it"):
        b.lib()
    with pytest.raises(RuntimeError, match=row["no_fallback"]):
        b.lib()
    if row is not MAIN:
        assert not b.loaded()


# ---- c. lazy loading ----
WALK = """
import sys; sys.path.insert(0, %r)
import importlib, math, torch, vmlmf_amd
from vmlmf_amd import _lib
_lib.lib()
def refused(call):
    try:
        call()
        raise SystemExit('no refusal')
    except RuntimeError as e:
        assert 'cuda' in str(e) or 'HIP device' in str(e), e
tok = torch.zeros((3, 2), dtype=torch.int64)
m = vmlmf_amd.Model(16, 8, 1, 0.0, 0.1, w_rank=4, u_ranks=[4], lstm_type='vmlmf')
off = dict(min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None, automaton=None, automaton_state=None)
for call in (lambda: m.generate(tok, 4), lambda: m.generate(tok, 4, top_k=3), lambda: m.generate(tok, 4, eos=2, repetition_penalty=1.2),
             lambda: m.generate(tok, 4, **off), lambda: m.beam_search(tok, 4, automaton=None, automaton_state=None),
             lambda: m.generate(tok, 4, min_p=0.1), lambda: m.generate(tok, 4, typical_p=0.9, eos=3),
             lambda: m.generate(tok, 4, epsilon_cutoff=0.01, eta_cutoff=0.01, top_k=4),
             lambda: m.score(tok), lambda: m.score(tok, tok, top=4, lengths=torch.tensor([1, 2])),
             lambda: vmlmf_amd.lm_score(torch.zeros(3, 8), torch.zeros(16, 8), None, top=2)):
    refused(call)
vmlmf_amd.DecodeControls(2, 16, 'cpu', eos=3)
t = vmlmf_amd.Truncation(min_p=0.1, typical_p=0.9, epsilon_cutoff=0.01, eta_cutoff=0.01)
assert t.on and t.struct().min_p > 0
m = vmlmf_amd.Model(64, 8, 1, 0.0, 0.1, w_rank=4, u_ranks=[4], lstm_type='vmlmf')
c = vmlmf_amd.HistoryControls(2, 64, 'cpu', no_repeat_ngram_size=2, banned_sequences=[[1, 2]], frequency_penalty=0.5, prompt=tok)
assert c.hist_len.tolist() == [3, 3] and c.count.dtype == torch.uint16
refused(lambda: m.generate(tok, 4, no_repeat_ngram_size=2))
m = vmlmf_amd.Model(97, 8, 1, 0.0, 0.1, w_rank=4, u_ranks=[4], lstm_type='vmlmf')
for kw in (dict(), dict(eos=3), dict(eos=3, min_length=2), dict(banned_tokens=[5]), dict(eos=3, min_length=2, banned_tokens=[5]), dict(no_repeat_ngram_size=2),
           dict(banned_sequences=[[1, 2]]), dict(eos=3, min_length=2, banned_tokens=[5], no_repeat_ngram_size=3, banned_sequences=[[1, 2]])):
    refused(lambda: m.beam_search(tok, 4, **kw))
c = vmlmf_amd.BeamControls(2, 4, 97, 'cpu', prompt=tok, no_repeat_ngram_size=2, banned_sequences=[[1, 2]], banned_tokens=[5], eos=3, min_length=1)
assert c.history()[1].tolist() == [3] * 8
for kw in (dict(), dict(top_k=3), dict(seed=3, top_k=5), dict(eos=2, repetition_penalty=1.2), dict(no_repeat_ngram_size=2),
           dict(banned_sequences=[[1, 2]]), dict(min_p=0.1), dict(typical_p=0.9, eos=3)):
    refused(lambda: m.generate(tok, 4, **kw))
refused(lambda: m.score(tok))
A = vmlmf_amd.TokenAutomaton.avoiding(97, [[1, 2], [3]])
assert A.advance(tok).tolist() == [0, 0] and A.accepts([1, 1, 4])
for B in (vmlmf_amd.TokenAutomaton.forced(97, [4, 5], 3), vmlmf_amd.TokenAutomaton.one_of(97, [[4], [5, 6]]),
          vmlmf_amd.TokenAutomaton.template(97, [[1, 2], 3])):
    assert B.S >= 3
c = vmlmf_amd.AutomatonControls(2, 97, 'cpu', A, eos=3, banned_tokens=[5], prompt=tok)
assert c.row_state.tolist() == [0, 0] and c.clone().struct().S == A.S
b = vmlmf_amd.AutomatonBeamControls(2, 4, 97, 'cpu', A, eos=3, min_length=1)
assert b.start().tolist() == [0] * 8
refused(lambda: m.generate(tok, 4, automaton=A, eos=3))
refused(lambda: m.beam_search(tok, 4, automaton=A, eos=3, min_length=2))
n = vmlmf_amd.NeuralCache(2, 8, 'cpu', 12)
for call in (lambda: m.group_beam_search(tok, 4),
             lambda: m.group_beam_search(tok, 4, beams=6, groups=3, diversity_penalty=1.0, eos=3, length_penalty=1.0),
             lambda: m.contrastive_search(tok, 4), lambda: m.contrastive_search(tok, 4, 8, 0.3, eos=3, chunk=2, return_penalties=True),
             lambda: m.contrastive_search(tok, 0), lambda: m.contrastive_search(tok, 4, top_k=1, penalty_alpha=0.0, states=None),
             lambda: vmlmf_amd.lm_contrast_step(torch.zeros(8, 8), torch.zeros((2, 4), dtype=torch.int64), torch.zeros(2, 4),
                                                vmlmf_amd.ContrastControls(2, 8, 'cpu', 6)),
             lambda: vmlmf_amd.ContrastControls(2, 8, 'cpu', 6).append(torch.zeros(3, 2, 8)),
             lambda: m.cache_score(tok), lambda: m.cache_score(tok, tok, cache=n, window=12),
             lambda: m.cache_score(tok, tok, theta=1.0, lam=0.5, window=12, cache=n, return_parts=True),
             lambda: vmlmf_amd.lm_cache_score(torch.zeros(3, 2, 8), tok, torch.zeros(3, 2), n),
             lambda: m.stochastic_beam_search(tok, 4), lambda: m.stochastic_beam_search(tok, 4, 6, seed=5, eos=3, chunk=2)):
    refused(call)
g = vmlmf_amd.GroupBeams(2, 4, 97, 'cpu', groups=2, diversity_penalty=0.5)
assert g.start()[0].shape == (2, 4) and g.start()[0].tolist() == [[0.0, -math.inf, 0.0, -math.inf]] * 2
c = vmlmf_amd.ContrastControls(2, 8, 'cpu', 12, top_k=4, penalty_alpha=0.6, eos=3, V=97)
assert c.clone().hist.shape == (2, 12, 8) and c.hist_len.tolist() == [0, 0]
n.update(torch.zeros(3, 2, 8), tok)
assert n.n == 3 and n.clone().keys.shape == (2, 3, 8)
s = vmlmf_amd.StochasticBeams(2, 4, 97, 'cpu')
assert s.start()[3].shape == (2, 4) and s.start()[4].shape == (2,)
side = {importlib.import_module('vmlmf_amd._' + name): 'libvmlmf_%%s.so' %% name for name in _lib.SIDE}
assert len(side) == %d
def mapped():
    return {ln.rsplit('/', 1)[-1] for ln in open('/proc/self/maps').read().splitlines() if 'libvmlmf_' in ln}
assert mapped() == {'libvmlmf_hip.so'} and not any(binding.loaded() for binding in side), mapped()
mine = getattr(vmlmf_amd, %r)
mine.lib()
assert mapped() == {'libvmlmf_hip.so', side[mine]}, mapped()
for binding in side:
    assert binding.loaded() == (binding is mine), side[binding]
"""


@pytest.mark.parametrize("row", SIDE, ids=IDS)
def test_a_side_library_is_loaded_by_its_own_first_call_only(row):
    """A process that imports the package, opens the main library and walks every decoder entry point - generate(), beam_search(),
    group_beam_search(), contrastive_search(), stochastic_beam_search(), score(), cache_score() and the lm_* steps, with and without
    every control, truncation sampler, automaton and cache, and with every keyword-only argument given as None - up to their refusals
    of CPU tensors, and builds every controls class on the CPU, has mapped libvmlmf_hip.so alone; then the row's own opens alone."""
    r = subprocess.run([sys.executable, "-c", WALK % (ROOT, len(SIDE), row["module"])], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


# ---- d. the Makefile ----
def make(*args):
    r = subprocess.run(["make", "-n", *args, "-C", CSRC], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def test_the_makefile_builds_and_cleans_every_library():
    libs = [MAIN["file"]] + [row["file"] for row in SIDE]
    objs = [row["obj"] for row in SIDE]
    links = [ln for ln in make("-B", "all") if " -shared " in ln]
    assert len(links) == 1 + len(SIDE) == 12                                                  # the main library and eleven beside it
    assert re.search(r"^SIDE := beam decode score history beamctl truncate automaton beamgroup contrast ncache sbeam$", MAKEFILE, flags=re.M)
    assert re.search(r"^all: \$\(OUT\) \$\(SIDE_OUT\)$", MAKEFILE, flags=re.M)
    main = [ln for ln in links if "-o ../lib/libvmlmf_hip.so" in ln]
    assert len(main) == 1 and "vmlmf_sample.o" in main[0] and not any(o in main[0] for o in objs)   # not linked into the main library
    steps = lambda lines: [ln for ln in lines if " -c " in ln or " -shared " in ln]
    rule = steps(make("-B", "../lib/libvmlmf_beam.so"))                                         # one rule and one set of flags for all
    assert len(rule) == 2 and "--offload-arch=gfx950" in rule[0] and " -c vmlmf_beam.hip " in rule[0] and rule[1] in links
    for row in SIDE:
        mine = [ln for ln in links if "-o ../lib/" + row["file"] in ln]
        assert len(mine) == 1 and [ln for ln in links if row["obj"] in ln] == mine                 # linked once, into its own library
        assert re.findall(r"\bvmlmf_\w+\.o\b", mine[0]) == [row["obj"]]                          # ... which holds nothing else
        own = steps(make("-B", "../lib/" + row["file"]))                                        # one compile and one link: the rule's
        assert own[1:] == mine and [ln.replace(row["name"], "beam") for ln in own] == rule, row["name"]
        deps = re.search(r"^%s:(.*)$" % re.escape(row["obj"]), MAKEFILE, flags=re.M).group(1).split()
        included = re.findall(r'#include "([^"]+)"', open(os.path.join(CSRC, row["obj"][:-2] + ".hip")).read())
        assert "vmlmf_side.h" in included and "../../include/" + row["header"] in included
        for h in included + row["deps"]:                        # rebuilt when a header it includes moves, or one that those include
            assert h in deps, (row["obj"], h)
    cleaned = "\n".join(make("clean"))
    assert all(n in cleaned for n in libs + objs)
    # build() makes all of it with one command - no target but `all`, `clean` and `torch` -, and the README shows the same command
    lib_py = open(os.path.join(ROOT, "vmlmf_amd", "_lib.py")).read()
    assert lib_py.count('["make", "-C", CSRC, f"-j{jobs}", "all"]') == 1
    assert re.findall(r'\["make", [^\]]*"(\w+)"\]', lib_py) == ["clean", "all", "torch"] and lib_py.count('"make"') == 3
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()                               # ... and checks every library of SIDE
    assert re.search(r'for name in _lib\.SIDE:\n +side = importlib\.import_module\("vmlmf_amd\._" \+ name\)', entry)
    assert not re.search(r"\b_(%s)\b" % "|".join(row["name"] for row in SIDE), entry)              # ... none of them by hand
    shown = re.search(r"^make -C vmlmf_amd/csrc -j8 ([^#\n]*)", open(os.path.join(ROOT, "README.md")).read(), flags=re.M)
    assert shown.group(1).split() == ["all"]
    assert re.findall(r"^(\w+):", MAKEFILE, flags=re.M) == ["all", "torch", "clean"]                # one target builds every library
    assert re.search(r"^\.PHONY: all clean torch$", MAKEFILE, flags=re.M)


# ---- e. the selection is written once ----
def test_the_selection_is_written_once():
    """The sampler, the controlled choices and the scoring take the merges, the reduction tree and the selection from one header;
    none of them holds a copy."""
    header = open(os.path.join(CSRC, "vmlmf_select.h")).read()
    for fn in ("best_merge", "lse_merge", "gumbel_of", "sample_key", "key_of", "z_of", "tempered", "radix_select", "tie_cutoff", "pick_row"):
        assert re.search(r"\b%s\s*\(" % fn, header), fn
    for name in ("vmlmf_sample.hip", "vmlmf_decode.hip", "vmlmf_score.hip", "vmlmf_history.hip"):
        text = open(os.path.join(CSRC, name)).read()
        assert '#include "vmlmf_select.h"' in text
        for fn in ("radix_select", "tie_cutoff", "best_merge", "lse_merge", "key_of", "choose_row", "pick_row", "for_quads"):
            assert not re.search(r"__device__[^;{]*\b%s\s*\(" % fn, text), (name, fn)
    text = open(os.path.join(CSRC, "vmlmf_score.hip")).read()
    for fn in ("choose_row", "radix_select", "tie_cutoff"):
        assert re.search(r"\b%s\s*\(" % fn, text), fn                 # ... and the scoring calls them


def test_the_history_choice_takes_the_selection_and_writes_phase_0_once():
    text = open(os.path.join(CSRC, "vmlmf_history.hip")).read()
    assert re.search(r"\bpick_row\s*\(", text) and re.search(r"\bchoose_row\s*\(", text)
    assert len(re.findall(r"__device__[^;{]*\bhistory_bans\s*\(", text)) == 1             # phase 0 is written once, for both kernels
    assert len(re.findall(r"\bhistory_bans\s*\(", text)) == 3
