"""The decoder's side libraries - libvmlmf_beam.so, libvmlmf_decode.so, libvmlmf_score.so, each with a header, an ABI version and a
binding of its own (vmlmf_amd/_beam.py, _decode.py, _score.py: one _lib.Library each) - held to one table: what the header declares is
bound and exported, and by that library alone; a missing file is a clear error; a library is opened by its own first call only; the
Makefile links each from its own object and cleans all of them; the selection is written once, in vmlmf_select.h.
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
]
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
def test_a_side_library_is_loaded_by_its_own_first_call_only():
    """A process that imports the package, opens the main library and walks generate(), DecodeControls, score() and lm_score up to
    their refusals of CPU tensors has opened none of the three; then each opens alone."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import torch, vmlmf_amd\nfrom vmlmf_amd import _beam, _decode, _score, _lib\n_lib.lib()\n"
            "m = vmlmf_amd.Model(16, 8, 1, 0.0, 0.1, w_rank=4, u_ranks=[4], lstm_type='vmlmf')\n"
            "tok = torch.zeros((3, 2), dtype=torch.int64)\n"
            "for call in (lambda: m.generate(tok, 4), lambda: m.generate(tok, 4, top_k=3), lambda: m.generate(tok, 4, eos=2, repetition_penalty=1.2),\n"
            "             lambda: m.score(tok), lambda: m.score(tok, tok, top=4, lengths=torch.tensor([1, 2])),\n"
            "             lambda: vmlmf_amd.lm_score(torch.zeros(3, 8), torch.zeros(16, 8), None, top=2)):\n"
            "    try:\n        call()\n        raise SystemExit('no refusal')\n"
            "    except RuntimeError as e:\n        assert 'cuda' in str(e)\n"
            "vmlmf_amd.DecodeControls(2, 16, 'cpu', eos=3)\n"
            "side = [(_beam, 'libvmlmf_beam.so'), (_decode, 'libvmlmf_decode.so'), (_score, 'libvmlmf_score.so')]\n"
            "maps = open('/proc/self/maps').read()\n"
            "assert 'libvmlmf_hip.so' in maps\n"
            "for i, (binding, name) in enumerate(side):\n"
            "    maps = open('/proc/self/maps').read()\n"
            "    for later, later_name in side[i:]:\n"
            "        assert later_name not in maps and not later.loaded(), (name, later_name)\n"
            "    binding.lib()\n"
            "    assert name in open('/proc/self/maps').read() and binding.loaded(), name\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


# ---- d. the Makefile ----
def test_the_makefile_builds_and_cleans_every_library():
    libs = [MAIN["file"]] + [row["file"] for row in SIDE]
    objs = [row["obj"] for row in SIDE]
    r = subprocess.run(["make", "-n", "-B", "-C", CSRC, "all"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and all(n in r.stdout for n in libs)
    links = [ln for ln in r.stdout.splitlines() if " -shared " in ln]
    main = [ln for ln in links if "-o ../lib/libvmlmf_hip.so" in ln]
    assert len(main) == 1 and "vmlmf_sample.o" in main[0] and not any(o in main[0] for o in objs)   # not linked into the main library
    for row in SIDE:
        mine = [ln for ln in links if "-o ../lib/" + row["file"] in ln]
        assert len(mine) == 1 and [ln for ln in links if row["obj"] in ln] == mine                 # linked once, into its own library
        assert re.findall(r"\bvmlmf_\w+\.o\b", mine[0]) == [row["obj"]]                          # ... which holds nothing else
    r = subprocess.run(["make", "-n", "-C", CSRC, "clean"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and all(n in r.stdout for n in libs + objs)


# ---- e. the selection is written once ----
def test_the_selection_is_written_once():
    """The sampler, the controlled choice and the scoring take the merges, the reduction tree and the selection from one header;
    none of them holds a copy."""
    header = open(os.path.join(CSRC, "vmlmf_select.h")).read()
    for fn in ("best_merge", "lse_merge", "gumbel_of", "sample_key", "key_of", "z_of", "tempered", "radix_select", "tie_cutoff", "pick_row"):
        assert re.search(r"\b%s\s*\(" % fn, header), fn
    for name in ("vmlmf_sample.hip", "vmlmf_decode.hip", "vmlmf_score.hip"):
        text = open(os.path.join(CSRC, name)).read()
        assert '#include "vmlmf_select.h"' in text
        for fn in ("radix_select", "tie_cutoff", "best_merge", "lse_merge", "key_of", "choose_row", "for_quads"):
            assert not re.search(r"__device__[^;{]*\b%s\s*\(" % fn, text), (name, fn)
    text = open(os.path.join(CSRC, "vmlmf_score.hip")).read()
    for fn in ("choose_row", "radix_select", "tie_cutoff"):
        assert re.search(r"\b%s\s*\(" % fn, text), fn                 # ... and the scoring calls them
