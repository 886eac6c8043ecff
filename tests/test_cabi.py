"""CPU: the C-ABI shared library loads without a GPU and exports every symbol include/vmlmf_hip.h declares;
vmlmf_query (host-only) validates descriptors the way the reference's shapes demand."""
import ctypes
import os
import re

import pytest

from vmlmf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    text = open(os.path.join(ROOT, "include", "vmlmf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"\b(vmlmf_[a-z0-9_]+)\s*\(", text)
    return sorted(set(names))


def test_header_and_binding_agree():
    decl = declared_functions()
    assert decl, "no functions parsed from the header"
    assert sorted(_lib.SYMBOLS) == decl


def test_library_loads_and_exports_every_symbol():
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared_functions():
        assert hasattr(handle, name), f"missing export {name}"
    lib = _lib.lib()
    assert lib.vmlmf_abi_version() == _lib.ABI_VERSION == 13
    assert b"gfx950" in lib.vmlmf_build_info()
    assert [lib.vmlmf_kernel_name(k).decode() for k in range(_lib.NKERNELS)] == [
        "pack_kernel", "xproj_kernel", "rec_fwd_kernel", "rec_bwd_kernel", "dqx_dx_kernel", "wgrad_mfma_kernel", "reduce_cg_kernel",
        "finish_kernel", "head_fwd_kernel", "head_bwd_kernel", "ce_fwd_kernel", "ce_bwd_kernel", "finish2_kernel"]


def test_query_headline_geometry():
    s = _lib.query(_lib.make_desc(_lib.V1_CELL, 64, 128, 9, 180, 16, [16]))
    assert (s.rows_per_wg, s.threads_per_wg, s.workgroups, s.kx, s.kh) == (1, 192, 64, 16, 16)
    assert s.reserve_bytes > 64 * 128 * 180 * 5 * 4          # gates + c tape
    s = _lib.query(_lib.make_desc(_lib.V2_GROUP_CELL, 512, 128, 9, 180, 16, [16, 16], g=2))
    assert (s.rows_per_wg, s.threads_per_wg, s.workgroups, s.kh) == (1, 256, 512, 32)   # 2 groups x 2 waves
    s = _lib.query(_lib.make_desc(_lib.V1_CELL, 1024, 8, 9, 180, 16, [16]))
    assert (s.rows_per_wg, s.workgroups) == (1, 1024)                                   # one row per workgroup at any batch
    s = _lib.query(_lib.make_desc(_lib.V2_GROUP_CELL, 81, 24, 77, 180, 8, [2, 4], g=2))  # demo.sh:10
    assert (s.kx, s.kh) == (8, 16)
    # BASELINE config E (PTB group layer): too large for the register-resident kernels -> step-wise path
    s = _lib.query(_lib.make_desc(_lib.V4_LM_GROUP, 256, 35, 650, 650, 32, [32, 32], g=2, time_major=True))
    # ... now on the clustered row-block MFMA kernels: 16 row blocks x 16 workgroups, 4 compute waves each
    assert (s.kx, s.kh, s.threads_per_wg, s.rows_per_wg, s.workgroups) == (32, 64, 256, 16, 256)
    # the cells without vm share the geometry of their vm counterparts
    s = _lib.query(_lib.make_desc(_lib.V5_LMF_CELL, 64, 128, 9, 180, 16, [16]))
    assert (s.rows_per_wg, s.threads_per_wg, s.workgroups, s.kx, s.kh) == (1, 192, 64, 16, 16)
    s = _lib.query(_lib.make_desc(_lib.V6_GROUP_NOVM, 64, 128, 9, 180, 16, [16, 16], g=2))
    assert (s.threads_per_wg, s.kh) == (256, 32)
    # ... and, unlike them, accept more inputs than hidden units (as the reference does for these two cells)
    s = _lib.query(_lib.make_desc(_lib.V5_LMF_CELL, 4, 3, 10, 8, 3, [3]))
    assert s.workspace_bytes > 0


@pytest.mark.parametrize("desc,code", [
    (dict(variant=_lib.V1_CELL, B=4, T=3, I=10, H=8, w_rank=3, u_ranks=[3]), _lib.E_SHAPE),        # vmlmf.py:94
    (dict(variant=_lib.V3_LM, B=4, T=3, I=6, H=8, w_rank=3, u_ranks=[3]), _lib.E_SHAPE),          # vmlmf_lm.py:243
    (dict(variant=_lib.V2_GROUP_CELL, B=4, T=3, I=4, H=9, w_rank=3, u_ranks=[2, 2], g=2), _lib.E_SHAPE),
    (dict(variant=7, B=4, T=3, I=4, H=8, w_rank=3, u_ranks=[3]), _lib.E_BADARG),
    (dict(variant=_lib.V6_GROUP_NOVM, B=4, T=3, I=4, H=9, w_rank=3, u_ranks=[2, 2], g=2), _lib.E_SHAPE),
    (dict(variant=_lib.V1_CELL, B=0, T=3, I=4, H=8, w_rank=3, u_ranks=[3]), _lib.E_BADARG),
    (dict(variant=_lib.V1_CELL, B=4, T=3, I=4, H=8, w_rank=3, u_ranks=[0]), _lib.E_BADARG),
    (dict(variant=_lib.V2_GROUP_CELL, B=4, T=3, I=4, H=12, w_rank=3, u_ranks=[2, 2, 2], g=3), _lib.E_UNSUPPORTED),
    (dict(variant=_lib.V1_CELL, B=4, T=3, I=4, H=64, w_rank=40, u_ranks=[8]), _lib.E_UNSUPPORTED),
    (dict(variant=_lib.V2_GROUP_CELL, B=4, T=3, I=4, H=64, w_rank=4, u_ranks=[72, 72], g=2), _lib.E_UNSUPPORTED),
])
def test_query_rejects_what_it_must(desc, code):
    with pytest.raises(_lib.VmlmfError) as ei:
        _lib.query(_lib.make_desc(**desc))
    assert ei.value.code == code
    assert len(str(ei.value)) > 20          # carries an explanation, like the reference's RuntimeError


def test_forward_refuses_null_buffers_without_touching_the_gpu():
    lib = _lib.lib()
    d = _lib.make_desc(_lib.V1_CELL, 4, 3, 4, 8, 3, [3])
    p = _lib.Params()
    rc = lib.vmlmf_seq_forward(ctypes.byref(d), ctypes.byref(p), None, None, None, None, None, None, None, None,
                               0, None)
    assert rc == _lib.E_BADARG
    assert b"null" in lib.vmlmf_last_error()
    d5 = _lib.make_desc(_lib.V5_LMF_CELL, 4, 3, 4, 8, 3, [3])
    rc = lib.vmlmf_seq_forward(ctypes.byref(d5), ctypes.byref(p), None, None, None, None, None, None, None, None,
                               0, None)
    assert rc == _lib.E_BADARG and b"null pointer in params" in lib.vmlmf_last_error()


def test_driver_build_entry_point_runs():
    """__graft_entry__.build() is what the driver calls on the CPU box: make (a no-op when the library is current),
    import, ABI check."""
    import importlib
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    entry = importlib.import_module("__graft_entry__")
    entry.build()


def test_comm_entry_points_validate_arguments_without_a_gpu():
    """The RCCL entry points are bound at run time: bad arguments are refused before RCCL is touched, and a missing RCCL
    is VMLMF_E_UNSUPPORTED with a reason, never a crash (no collective is run here)."""
    lib = _lib.lib()
    rc = lib.vmlmf_flat_allreduce(None, 0, _lib.SUM, None, None)
    assert rc in (_lib.E_BADARG, _lib.E_UNSUPPORTED) and lib.vmlmf_last_error()
    rc = lib.vmlmf_flat_allreduce(None, 0, 7, ctypes.c_void_p(1), None)
    assert rc in (_lib.E_BADARG, _lib.E_UNSUPPORTED)
    h = ctypes.c_void_p()
    rc = lib.vmlmf_comm_init(ctypes.byref(h), 2, 5, (ctypes.c_ubyte * 128)())
    assert rc in (_lib.E_BADARG, _lib.E_UNSUPPORTED) and not h


def test_stack_query_host_logic():
    """vmlmf_stack_query (ABI 7) is pure host logic: sizes for a covered stack, VMLMF_E_UNSUPPORTED / VMLMF_E_SHAPE for
    stacks the wavefront kernels do not take (the caller then chains the per-layer calls).  No GPU call."""
    import ctypes
    from vmlmf_amd import _lib
    lib = _lib.lib()

    def query(L, B, T, I, H, rw, ru, variant=_lib.V1_CELL, g=1, H_upper=None, I_upper=None):
        layers = (_lib.StackLayer * L)()
        for l in range(L):
            h = H if (l == 0 or H_upper is None) else H_upper
            i = I if l == 0 else (H if I_upper is None else I_upper)
            layers[l].desc = _lib.make_desc(variant, B, T, i, h, rw, [ru] * g, g=g, time_major=False, training=True)
        rb = (ctypes.c_size_t * L)()
        wb = ctypes.c_size_t()
        rc = lib.vmlmf_stack_query(L, ctypes.addressof(layers), ctypes.addressof(rb), ctypes.addressof(wb))
        return rc, [int(v) for v in rb], int(wb.value)

    rc, rb, wb = query(2, 128, 24, 77, 256, 24, 24)            # BASELINE configs[2]
    assert rc == 0 and all(v > 0 for v in rb) and wb > 0
    single = _lib.query(_lib.make_desc(_lib.V1_CELL, 128, 24, 256, 256, 24, [24], training=True))
    assert rb[1] > single.reserve_bytes                          # the stack's reserve also holds the rotated images
    assert rb[0] - rb[1] != 0                                    # layer 0: other input width, plus the backward's progress words
    assert query(1, 64, 128, 9, 180, 16, 16)[0] == 0
    assert query(4, 8, 5, 20, 64, 8, 8)[0] == 0
    assert query(5, 8, 5, 20, 64, 8, 8)[0] == _lib.E_UNSUPPORTED                      # more than four layers
    assert query(2, 8, 5, 20, 64, 8, 16)[0] == 0                                      # padded w_rank != padded u_rank: the wider of the two
    assert query(2, 8, 5, 20, 256, 8, 32)[0] == _lib.E_UNSUPPORTED                    # ... which must still fit
    assert query(2, 8, 5, 20, 320, 16, 16)[0] == _lib.E_UNSUPPORTED                   # more than four waves of units
    assert query(2, 8, 5, 20, 256, 32, 32)[0] == _lib.E_UNSUPPORTED                   # rank 32 with four waves: register budget
    assert query(2, 8, 5, 20, 64, 8, 8, variant=_lib.V2_GROUP_CELL, g=2)[0] == 0                    # group cells: two rank blocks
    assert query(2, 8, 5, 20, 360, 8, 8, variant=_lib.V2_GROUP_CELL, g=2)[0] == _lib.E_UNSUPPORTED   # ... within four waves of units
    assert query(2, 8, 5, 64, 64, 8, 8, variant=_lib.V4_LM_GROUP, g=2)[0] in (_lib.E_UNSUPPORTED, _lib.E_SHAPE)   # the flat LM layout: not covered
    assert query(2, 8, 5, 20, 64, 8, 8, H_upper=72, I_upper=64)[0] == 0               # unequal hidden sizes (round 6): the widest layer's geometry
    assert query(2, 8, 5, 20, 64, 8, 8, H_upper=320, I_upper=64)[0] == _lib.E_UNSUPPORTED           # ... which must fit four waves of units
    assert query(2, 8, 5, 20, 64, 8, 16, H_upper=72, I_upper=64)[0] == _lib.E_UNSUPPORTED           # ... one padded rank on both sides
    assert query(2, 8, 5, 20, 64, 8, 8, variant=_lib.V2_GROUP_CELL, g=2, H_upper=72, I_upper=64)[0] == _lib.E_UNSUPPORTED   # ... one group
    assert query(2, 8, 5, 20, 64, 8, 8, I_upper=48)[0] == _lib.E_SHAPE                # layer 1 does not read layer 0's width
    assert b"stack" in lib.vmlmf_last_error()


def test_p2p_entry_points_validate_their_arguments():
    """vmlmf_p2p_* (ABI 13; host-only part): rank / world / size limits are refused before anything touches a device, and the
    entry points that take a handle refuse NULL."""
    lib = _lib.lib()
    h = ctypes.c_void_p()
    buf = (ctypes.c_ubyte * _lib.P2P_HANDLE_BYTES)()
    assert lib.vmlmf_p2p_create(ctypes.byref(h), 0, _lib.P2P_MAX_RANKS + 1, 1000, buf) == _lib.E_BADARG
    assert lib.vmlmf_p2p_create(ctypes.byref(h), 2, 2, 1000, buf) == _lib.E_BADARG            # rank >= world
    assert lib.vmlmf_p2p_create(ctypes.byref(h), 0, 2, 0, buf) == _lib.E_UNSUPPORTED
    assert lib.vmlmf_p2p_create(ctypes.byref(h), 0, 2, (1 << 22) + 1, buf) == _lib.E_UNSUPPORTED   # RCCL's job
    assert b"small" in lib.vmlmf_last_error()
    assert lib.vmlmf_p2p_create(None, 0, 2, 1000, buf) == _lib.E_BADARG
    assert lib.vmlmf_p2p_connect(None, buf) == _lib.E_BADARG
    assert lib.vmlmf_p2p_allreduce(None, None, 4, _lib.SUM, None) == _lib.E_BADARG
    assert lib.vmlmf_p2p_destroy(None) == 0


def test_every_documented_kernel_switch_is_accepted():
    """The keys the header documents for vmlmf_tune are the keys the library takes (host-only: the switches are plain
    process-wide settings), each call moves the generation GraphedTrainStep watches, an unknown key is VMLMF_E_BADARG."""
    text = open(os.path.join(ROOT, "include", "vmlmf_hip.h")).read()
    block = text[text.index("Kernel-selection switches"):text.index("int vmlmf_tune(")]
    keys = re.findall(r'^ \*   "([a-z0-9_]+)"', block, flags=re.M)
    assert {"rb", "wride", "inrow", "wring", "adam_guard"} <= set(keys), keys
    defaults = {"rb": -1, "rb_min_batch": 0, "rb_cluster": 0, "rb_rows": 0, "rec3": 6, "wride": 1, "inrow": -1, "adam_guard": 1,
                "clear_health": 0, "wring": -1, "test_wride_spin": 0, "direct": 1, "finish2": 1, "rbx": 1, "ffb": 0}
    lib = _lib.lib()
    import ctypes
    for k in keys:
        assert k in defaults, f"header documents {k}: add its default here"
        g0 = lib.vmlmf_tune_generation()
        was = ctypes.c_int(0)
        readable = lib.vmlmf_tune_get(k.encode(), ctypes.byref(was)) == 0
        assert lib.vmlmf_tune(k.encode(), defaults[k]) == 0, (k, lib.vmlmf_last_error())
        assert lib.vmlmf_tune_generation() == g0 + 1
        if readable:      # leave the process as it was (rb_min_batch's 0 means 1: the next test's plans would change)
            assert lib.vmlmf_tune(k.encode(), was.value) == 0
    assert lib.vmlmf_tune(b"no_such_switch", 1) == _lib.E_BADARG
    # the measured-no-gain forms of round 4 left the product library (tools/experiments/*.patch): their switches are gone with them
    for k in (b"inrow_rows", b"rb_wgrad", b"rb_xfold"):
        assert lib.vmlmf_tune(k, 0) == _lib.E_BADARG, k
    # ABI 11: the switches read back (a benchmark reports whether the riding workers were armed)
    assert lib.vmlmf_tune(b"wride", 0) == 0 and _lib.tune_get("wride") == 0
    assert lib.vmlmf_tune(b"wride", 1) == 0 and _lib.tune_get("wride") == (0 if os.environ.get("VMLMF_WRIDE") == "0" else 1)
    assert lib.vmlmf_tune(b"rec3", 7) == 0 and _lib.tune_get("rec3") == 7 and lib.vmlmf_tune(b"rec3", 6) == 0
    assert lib.vmlmf_tune_get(b"no_such_switch", ctypes.byref(ctypes.c_int(0))) == _lib.E_BADARG


def test_a_switch_flipped_through_the_raw_symbol_reaches_the_descriptor_cache():
    """functional's host caches carry vmlmf_tune_generation() in their keys, so a switch that did not go through _lib.tune() - the
    raw symbol, as above, or the library's own switch after a riding worker gave up - is seen by the next descriptor lookup:
    the cached entry before the call, a freshly queried one after it (host-only: vmlmf_query)."""
    from vmlmf_amd import functional as F
    lib = _lib.lib()
    shape = ((_lib.V1_CELL, 1, 16, (16,), False, _lib.DT_F32), 64, 128, 9, 180, True)
    first = F._desc_for(*shape)
    assert F._desc_for(*shape) is first
    was = _lib.tune_get("rec3")
    try:
        assert lib.vmlmf_tune(b"rec3", 6 if was == 7 else 7) == 0
        fresh = F._desc_for(*shape)
        assert fresh is not first and fresh[0] is not first[0]
        now = _lib.query(fresh[0])
        assert all(getattr(fresh[1], f) == getattr(now, f) for f, _ in _lib.Sizes._fields_)
        assert F._desc_for(*shape) is fresh
    finally:
        assert lib.vmlmf_tune(b"rec3", was) == 0


def test_the_product_library_stays_pruned():
    """Verdict r4 item 6: no probe-only / unreachable instantiations in the shipped library - under 9 MB, and none of the ablation
    template parameters' names in its kernel symbols."""
    import subprocess
    size = os.path.getsize(_lib.LIB_PATH)
    # (round 5: 8.92 MB; round 6 adds the clustered-stack kernels - rbx_fwd / rbx_bwd for the PTB group and plain layers, the stack-wide
    #  pack and zero launches: + 0.2 MB of product code; wgrad4_stack_kernel's two instantiations and the one-launch finish: + 0.15 MB)
    assert size < 9_400_000, f"libvmlmf_hip.so is {size / 1e6:.2f} MB"
    out = subprocess.run(["strings", "-n", "12", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "VMLMF_R4_ABL" not in out and "VMLMF_WRIDE_DRY" not in out


def _stack_layers(variant, L, B, T, H, rw, ru, g):
    layers = (_lib.StackLayer * L)()
    for l in range(L):
        layers[l].desc = _lib.make_desc(variant, B, T, H, H, rw, ru, g=g, time_major=True, training=True)
    return layers


def test_clustered_stacks_are_planned_where_all_clusters_are_co_resident():
    """Round 6 (vmlmf_stack_*, ABI 12; host-only): PTB-sized layers (vmlmf_lm.py:53-174 / 178-280) are stacked into one launch per direction
    while L x ceil(B / rows) x 16 workgroups fit the device (256 CUs assumed without a GPU): two layers up to 128 rows, three up to 80;
    beyond that - and for a single layer - VMLMF_E_UNSUPPORTED (the caller chains the layers); such stacks take dropout inside."""
    lib = _lib.lib()
    rb = (ctypes.c_size_t * 4)()
    wb = ctypes.c_size_t()

    def query(variant, L, B, ru, g, H=650):
        layers = _stack_layers(variant, L, B, 35, H, 32, ru, g)
        rc = lib.vmlmf_stack_query(L, ctypes.addressof(layers), ctypes.addressof(rb), ctypes.addressof(wb))
        return rc, lib.vmlmf_stack_dropout_fused(L, ctypes.addressof(layers))

    for B in (7, 32, 64, 128):
        assert query(_lib.V4_LM_GROUP, 2, B, [32, 32], 2) == (0, 1), B
        assert query(_lib.V3_LM, 2, B, [32], 1) == (0, 1), B
    assert query(_lib.V4_LM_GROUP, 2, 256, [32, 32], 2)[0] == _lib.E_UNSUPPORTED
    assert query(_lib.V4_LM_GROUP, 3, 128, [32, 32], 2)[0] == _lib.E_UNSUPPORTED
    assert query(_lib.V3_LM, 3, 80, [32], 1) == (0, 1)
    assert query(_lib.V3_LM, 1, 32, [32], 1)[0] == _lib.E_UNSUPPORTED
    assert rb[0] > 0 and wb.value > 0
    # small layers: the wavefront form; one-group stacks take dropout inside its launches too, two-group stacks do not
    assert query(_lib.V3_LM, 2, 32, [16], 1, H=128)[1] == 1
    layers = (_lib.StackLayer * 2)()
    for l in range(2):
        layers[l].desc = _lib.make_desc(_lib.V2_GROUP_CELL, 16, 8, 64, 64, 8, [8, 8], g=2, training=True)
    assert lib.vmlmf_stack_query(2, ctypes.addressof(layers), ctypes.addressof(rb), ctypes.addressof(wb)) == 0
    assert lib.vmlmf_stack_dropout_fused(2, ctypes.addressof(layers)) == 0
    # the switch that keeps clustered layers chained
    _lib.tune("rbx", 0)
    try:
        assert query(_lib.V4_LM_GROUP, 2, 32, [32, 32], 2)[0] == _lib.E_UNSUPPORTED
    finally:
        _lib.tune("rbx", 1)
    assert query(_lib.V4_LM_GROUP, 2, 32, [32, 32], 2)[0] == 0


def test_the_run_time_switches_follow_the_environment():
    """Round 6: the switches defined inside the extern "C" block came up with other switches' defaults (mangled lambda names shared with the
    top-of-file block).  A fresh process must see what the environment says: every key vmlmf_tune_get answers, set from its environment
    variable, read back; the defaults with no VMLMF_* set; and the parse rules (on unless it starts with 0, integer, positive or the
    default)."""
    import subprocess
    import sys
    # key: (environment variable, default, a value that is not the default)
    switches = {"rbx": ("VMLMF_RBX", 1, 7), "ffb": ("VMLMF_FFB", 0, -1), "rb": ("VMLMF_RB", -1, 0), "inrow": ("VMLMF_INROW", -1, 1),
                "rec3": ("VMLMF_REC3", 6, 5), "adam_guard": ("VMLMF_ADAM_GUARD", 1, 2), "wring": ("VMLMF_WRING", -1, 1),
                "direct": ("VMLMF_DIRECT", 1, 0), "finish2": ("VMLMF_FINISH2", 1, 0), "wride": ("VMLMF_WRIDE", 1, 0),
                "rb_min_batch": ("VMLMF_RB_MINB", 0, 96), "rb_cluster": ("VMLMF_RB_S", 0, 8), "rb_rows": ("VMLMF_RB_ROWS", 0, 4)}
    code = ("import ctypes; from vmlmf_amd import _lib; l = _lib.lib(); v = ctypes.c_int(); out = []\n"
            f"for k in {[k.encode() for k in switches]!r}:\n"
            "    assert l.vmlmf_tune_get(k, ctypes.byref(v)) == 0, k; out.append(v.value)\n"
            "print(out)")
    base = {k: v for k, v in os.environ.items() if not k.startswith("VMLMF_")}
    base["PYTHONPATH"] = ROOT

    def read(extra):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(base, **extra), timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return dict(zip(switches, eval(r.stdout.strip().splitlines()[-1])))

    assert read({e: str(v) for e, _, v in switches.values()}) == {k: v for k, (_, _, v) in switches.items()}
    assert read({}) == {k: d for k, (_, d, _) in switches.items()}
    got = read({"VMLMF_WRIDE": "-1", "VMLMF_DIRECT": "00", "VMLMF_RB_MINB": "-5", "VMLMF_RB_S": "x", "VMLMF_REC3": "3abc"})
    assert (got["wride"], got["direct"], got["rb_min_batch"], got["rb_cluster"], got["rec3"]) == (1, 0, 0, 0, 3), got
    assert read({"VMLMF_WRIDE": "0x"})["wride"] == 0
