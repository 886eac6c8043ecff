"""The decoder's side libraries - libvmlmf_beam.so, libvmlmf_decode.so, libvmlmf_score.so, libvmlmf_history.so, libvmlmf_beamctl.so,
libvmlmf_truncate.so, libvmlmf_automaton.so, each with a header, an ABI version and a binding of its own (vmlmf_amd/_<name>.py: one
_lib.Library each) - held to one table: what the header declares is bound and exported, and by that library alone; a missing file is a
clear error; a library is opened by its own first call only; the Makefile links each from its own object and cleans all of them; the
selection is written once, in vmlmf_select.h.
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

SIDE = [
    dict(header="vmlmf_beam.h", module="_beam", file="libvmlmf_beam.so", abi_macro="VMLMF_BEAM_ABI_VERSION", obj="vmlmf_beam.o",
         functions=["vmlmf_beam_abi_version", "vmlmf_beam_backtrack", "vmlmf_beam_gather", "vmlmf_beam_last_error", "vmlmf_beam_step",
                    "vmlmf_beam_workspace_bytes"],
         no_fallback="no stock-op fallback for the beam-search step"),
    dict(header="vmlmf_decode.h", module="_decode", file="libvmlmf_decode.so", abi_macro="VMLMF_DECODE_ABI_VERSION", obj="vmlmf_decode.o",
         functions=["vmlmf_decode_abi_version", "vmlmf_decode_choose", "vmlmf_decode_last_error"],
         no_fallback="no stock-op fallback for the controlled choice of Model.generate"),
    dict(header="vmlmf_score.h", module="_score", file="libvmlmf_score.so", abi_macro="VMLMF_SCORE_ABI_VERSION", obj="vmlmf_score.o",
         functions=["vmlmf_score_abi_version", "vmlmf_score_last_error", "vmlmf_score_rows"],
         no_fallback="no stock-op fallback for Model.score"),
    dict(header="vmlmf_history.h", module="_history", file="libvmlmf_history.so", abi_macro="VMLMF_HISTORY_ABI_VERSION", obj="vmlmf_history.o",
         functions=["vmlmf_history_abi_version", "vmlmf_history_bans", "vmlmf_history_choose", "vmlmf_history_last_error"],
         no_fallback="no stock-op fallback for the history controls of Model.generate"),
    dict(header="vmlmf_beamctl.h", module="_beamctl", file="libvmlmf_beamctl.so", abi_macro="VMLMF_BEAMCTL_ABI_VERSION", obj="vmlmf_beamctl.o",
         functions=["vmlmf_beamctl_abi_version", "vmlmf_beamctl_last_error", "vmlmf_beamctl_step", "vmlmf_beamctl_workspace_bytes"],
         no_fallback="no stock-op fallback for the controlled beam-search step"),
    dict(header="vmlmf_truncate.h", module="_truncate", file="libvmlmf_truncate.so", abi_macro="VMLMF_TRUNCATE_ABI_VERSION", obj="vmlmf_truncate.o",
         functions=["vmlmf_truncate_abi_version", "vmlmf_truncate_choose", "vmlmf_truncate_last_error"],
         no_fallback="no stock-op fallback for the truncation samplers of Model.generate",
         deps=["vmlmf_side.h", "vmlmf_refusals.h", "vmlmf_select.h", "vmlmf_controlled.h", "vmlmf_truncate.h", "vmlmf_dropout.h",
               "../../include/vmlmf_decode.h", "../../include/vmlmf_truncate.h"]),
    dict(header="vmlmf_automaton.h", module="_automaton", file="libvmlmf_automaton.so", abi_macro="VMLMF_AUTOMATON_ABI_VERSION",
         obj="vmlmf_automaton.o",
         functions=["vmlmf_automaton_abi_version", "vmlmf_automaton_beam_step", "vmlmf_automaton_choose", "vmlmf_automaton_last_error",
                    "vmlmf_automaton_workspace_bytes"],
         no_fallback="no stock-op fallback for decoding under a token automaton",
         deps=["vmlmf_side.h", "vmlmf_refusals.h", "vmlmf_select.h", "vmlmf_controlled.h", "vmlmf_beam_core.h", "vmlmf_dropout.h",
               "../../include/vmlmf_beam.h", "../../include/vmlmf_decode.h", "../../include/vmlmf_automaton.h"]),
]
SIDE[1]["deps"] = ["vmlmf_controlled.h"]        # the controlled rows are written once, for the decode, truncate and automaton libraries
MAIN = dict(module="_lib", file="libvmlmf_hip.so", no_fallback="no CPU / PyTorch fallback for the hot path")
IDS = [row["module"] for row in SIDE]


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
    assert os.path.basename(b.LIBRARY.path) == row["file"] and b.LIBRARY.no_fallback in row["no_fallback"]


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
import torch, vmlmf_amd
from vmlmf_amd import _automaton, _beam, _beamctl, _decode, _history, _score, _truncate, _lib
_lib.lib()
def refused(call):
    try:
        call()
        raise SystemExit('no refusal')
    except RuntimeError as e:
        assert 'cuda' in str(e)
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
for kw in (dict(), dict(top_k=3), dict(eos=2, repetition_penalty=1.2), dict(no_repeat_ngram_size=2), dict(banned_sequences=[[1, 2]]),
           dict(min_p=0.1), dict(typical_p=0.9, eos=3)):
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
side = {_beam: 'libvmlmf_beam.so', _decode: 'libvmlmf_decode.so', _score: 'libvmlmf_score.so', _history: 'libvmlmf_history.so',
        _beamctl: 'libvmlmf_beamctl.so', _truncate: 'libvmlmf_truncate.so', _automaton: 'libvmlmf_automaton.so'}
assert len(side) == %d
maps = open('/proc/self/maps').read()
assert 'libvmlmf_hip.so' in maps
for binding, name in side.items():
    assert name not in maps and not binding.loaded(), name
mine = getattr(vmlmf_amd, %r)
mine.lib()
maps = open('/proc/self/maps').read()
for binding, name in side.items():
    assert (name in maps) == binding.loaded() == (binding is mine), name
"""


@pytest.mark.parametrize("row", SIDE, ids=IDS)
def test_a_side_library_is_loaded_by_its_own_first_call_only(row):
    """A process that imports the package, opens the main library and walks generate(), beam_search(), score() and lm_score - with and
    without every control, truncation sampler and automaton, and with every keyword-only argument given as None - up to their refusals of
    CPU tensors, and builds DecodeControls, HistoryControls, BeamControls, Truncation, TokenAutomaton, AutomatonControls and
    AutomatonBeamControls on the CPU, has opened none of the seven; then the row's own opens alone."""
    r = subprocess.run([sys.executable, "-c", WALK % (ROOT, len(SIDE), row["module"])], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


# ---- d. the Makefile ----
def test_the_makefile_builds_and_cleans_every_library():
    libs = [MAIN["file"]] + [row["file"] for row in SIDE]
    objs = [row["obj"] for row in SIDE]
    r = subprocess.run(["make", "-n", "-B", "-C", CSRC, "all"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and all(n in r.stdout for n in libs)
    links = [ln for ln in r.stdout.splitlines() if " -shared " in ln]
    assert len(links) == 1 + len(SIDE) == 8                                                   # the main library and seven beside it
    text = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SIDE := beam decode score history beamctl truncate automaton$", text, flags=re.M)
    main = [ln for ln in links if "-o ../lib/libvmlmf_hip.so" in ln]
    assert len(main) == 1 and "vmlmf_sample.o" in main[0] and not any(o in main[0] for o in objs)   # not linked into the main library
    for row in SIDE:
        mine = [ln for ln in links if "-o ../lib/" + row["file"] in ln]
        assert len(mine) == 1 and [ln for ln in links if row["obj"] in ln] == mine                 # linked once, into its own library
        assert re.findall(r"\bvmlmf_\w+\.o\b", mine[0]) == [row["obj"]]                          # ... which holds nothing else
        deps = re.search(r"^%s:(.*)$" % re.escape(row["obj"]), text, flags=re.M).group(1).split()
        for h in row.get("deps", []) + ["vmlmf_side.h", "../../include/" + row["header"]]:      # rebuilt when a header it includes moves
            assert h in deps, (row["obj"], h)
    r = subprocess.run(["make", "-n", "-C", CSRC, "clean"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and all(n in r.stdout for n in libs + objs)
    # build() builds all of it, and the README shows the same command
    assert re.search(r'\["make", "-C", CSRC, f"-j\{jobs\}", "all"\]', open(os.path.join(ROOT, "vmlmf_amd", "_lib.py")).read())
    assert re.search(r"^make -C vmlmf_amd/csrc -j8 ", open(os.path.join(ROOT, "README.md")).read(), flags=re.M)


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
