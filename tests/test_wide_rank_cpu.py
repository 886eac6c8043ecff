"""CPU: the admission rule for wide-rank layers (padded w_rank > 32 or padded hidden rank summed over groups > 128) in vmlmf_query
and vmlmf_stack_query - pure host logic of the built library, no GPU call - and the wide-rank golden fixtures against the oracle."""
import ctypes
import os
import sys

import numpy as np
import pytest

from vmlmf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ACCEPTED = [
    # (variant, B, T, I, H, w_rank, u_ranks, g, time_major)
    (_lib.V3_LM, 20, 35, 650, 650, 300, [300], 1, True),             # the reference LM layer at lm_test.py's defaults
    (_lib.V4_LM_GROUP, 20, 35, 650, 650, 300, [300, 300], 2, True),  # its group form
    (_lib.V1_CELL, 81, 24, 77, 180, 64, [64], 1, False),             # OPP cell, --wRank 64 --uRanks 64
    (_lib.V2_GROUP_CELL, 8, 10, 64, 180, 40, [48, 40], 2, False),
    (_lib.V5_LMF_CELL, 8, 10, 100, 180, 64, [150], 1, False),
    (_lib.V6_GROUP_NOVM, 8, 10, 100, 180, 64, [60, 60], 2, False),
    (_lib.V1_CELL, 8, 10, 64, 180, 37, [40], 1, False),              # odd w_rank
    (_lib.V5_LMF_CELL, 4, 6, 700, 160, 600, [40], 1, True),          # more inputs than units, KX 600
]


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("case", ACCEPTED, ids=lambda c: f"v{c[0]}_I{c[3]}_H{c[4]}_w{c[5]}_u{'x'.join(map(str, c[6]))}")
def test_query_accepts_wide_ranks(case, training):
    variant, B, T, I, H, rw, ru, g, tm = case
    s = _lib.query(_lib.make_desc(variant, B, T, I, H, rw, ru, g=g, time_major=tm, training=training))
    assert s.workspace_bytes > 0 and s.reserve_bytes > 0
    assert s.kx == (rw + 7) // 8 * 8
    assert s.kh == sum((r + 7) // 8 * 8 for r in ru)


REFUSED = [
    # (desc, start of the message)
    (dict(variant=_lib.V1_CELL, B=4, T=3, I=48, H=180, w_rank=64, u_ranks=[64]), "wide ranks: w_rank larger than input_size"),
    (dict(variant=_lib.V1_CELL, B=4, T=3, I=77, H=180, w_rank=64, u_ranks=[200]), "wide ranks: a u_rank larger"),
    (dict(variant=_lib.V2_GROUP_CELL, B=4, T=3, I=64, H=180, w_rank=8, u_ranks=[100, 40], g=2), "wide ranks: a u_rank larger"),
    # a wide x side on a register-resident layer
    (dict(variant=_lib.V1_CELL, B=81, T=24, I=77, H=180, w_rank=64, u_ranks=[16]), "padded w_rank > 32"),
    # past the caps
    (dict(variant=_lib.V3_LM, B=4, T=3, I=2000, H=2000, w_rank=1030, u_ranks=[300], time_major=True), "wide ranks: padded w_rank"),
    (dict(variant=_lib.V3_LM, B=4, T=3, I=2000, H=2000, w_rank=300, u_ranks=[1100], time_major=True), "wide ranks: padded w_rank"),
    # bf16 at wide ranks
    (dict(variant=_lib.V3_LM, B=20, T=35, I=650, H=650, w_rank=300, u_ranks=[300], time_major=True, dtype=1), "wide ranks: dtype bf16"),
]


@pytest.mark.parametrize("desc,start", REFUSED, ids=lambda v: str(v)[:40] if isinstance(v, str) else None)
def test_query_refuses_outside_the_wide_envelope(desc, start):
    with pytest.raises(_lib.VmlmfError) as ei:
        _lib.query(_lib.make_desc(**desc))
    assert ei.value.code == _lib.E_UNSUPPORTED
    assert str(ei.value).startswith(f"vmlmf_hip error {_lib.E_UNSUPPORTED}: {start}"), str(ei.value)


# ---- the caps exactly: padded 1024 accepted, the next padded width (1025 -> 1032) refused ----------------------------------------
AT_CAP = [
    # (variant, I, H, w_rank, u_ranks, g)
    (_lib.V3_LM, 1024, 1024, 1024, [1024], 1),              # both caps on one layer
    (_lib.V1_CELL, 1024, 1024, 1017, [40], 1),              # w_rank 1017 pads to 1024
    (_lib.V4_LM_GROUP, 1024, 1024, 64, [512, 512], 2),      # the hidden rank summed over the two shifts: 512 + 512
    (_lib.V2_GROUP_CELL, 64, 1040, 16, [505, 512], 2),      # 505 pads to 512: summed 1024
    (_lib.V5_LMF_CELL, 1100, 160, 1020, [40], 1),           # more inputs than units, w_rank pads to 1024
]


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("case", AT_CAP, ids=lambda c: f"v{c[0]}_I{c[1]}_H{c[2]}_w{c[3]}_u{'x'.join(map(str, c[4]))}")
def test_query_accepts_exactly_the_caps(case, training):
    variant, I, H, rw, ru, g = case
    s = _lib.query(_lib.make_desc(variant, 2, 3, I, H, rw, ru, g=g, time_major=True, training=training))
    assert s.workspace_bytes > 0 and (s.reserve_bytes > 0 or not training)
    assert s.kx == (rw + 7) // 8 * 8 and s.kx <= 1024
    assert s.kh == sum((r + 7) // 8 * 8 for r in ru) and s.kh <= 1024
    assert max(s.kx, s.kh) == 1024


PAST_CAP = [
    dict(variant=_lib.V3_LM, I=1032, H=1032, w_rank=1025, u_ranks=[40]),             # padded w_rank 1032
    dict(variant=_lib.V5_LMF_CELL, I=1100, H=160, w_rank=1025, u_ranks=[40]),        # ... with I > H
    dict(variant=_lib.V1_CELL, I=64, H=1100, w_rank=16, u_ranks=[1025]),             # padded u_rank 1032
    dict(variant=_lib.V4_LM_GROUP, I=1040, H=1040, w_rank=64, u_ranks=[512, 513], g=2),   # summed 512 + 520
    dict(variant=_lib.V2_GROUP_CELL, I=64, H=1040, w_rank=16, u_ranks=[513, 512], g=2),   # summed 520 + 512
]


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("desc", PAST_CAP, ids=lambda d: f"v{d['variant']}_w{d['w_rank']}_u{'x'.join(map(str, d['u_ranks']))}")
def test_query_refuses_one_past_the_caps(desc, training):
    with pytest.raises(_lib.VmlmfError) as ei:
        _lib.query(_lib.make_desc(B=2, T=3, time_major=True, training=training, **desc))
    assert ei.value.code == _lib.E_UNSUPPORTED
    assert str(ei.value).startswith(f"vmlmf_hip error {_lib.E_UNSUPPORTED}: wide ranks: padded w_rank"), str(ei.value)


# ---- large hidden sizes on the step-wise path (not wide): the 12-stage skinny forms of Q (H >= 1536) and dQ (H >= 705) --------
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("H", [705, 1536])
def test_query_accepts_large_one_group_layers(H, training):
    s = _lib.query(_lib.make_desc(_lib.V1_CELL, 3, 3, 64, H, 16, [40], training=training))
    assert (s.kx, s.kh) == (16, 40)
    # the step-wise path: one batch row per workgroup, every thread slot of the layer in it (NT = 64 per 64 units)
    assert (s.rows_per_wg, s.threads_per_wg, s.workgroups) == (1, (H + 63) // 64 * 64, 3)


def test_stack_of_wide_layers_is_refused():
    """The stack entry points do not take wide layers: MyLSTM / Model chain them through the per-layer calls."""
    lib = _lib.lib()
    for variant, I, H, rw, ru, g, tm in ((_lib.V3_LM, 650, 650, 300, [300], 1, True), (_lib.V1_CELL, 64, 128, 48, [56], 1, False)):
        L = 2
        layers = (_lib.StackLayer * L)()
        for l in range(L):
            layers[l].desc = _lib.make_desc(variant, 20, 35, I if l == 0 else H, H, rw, ru, g=g, time_major=tm, training=True)
        rb = (ctypes.c_size_t * L)()
        wb = ctypes.c_size_t()
        rc = lib.vmlmf_stack_query(L, ctypes.addressof(layers), ctypes.addressof(rb), ctypes.addressof(wb))
        assert rc == _lib.E_UNSUPPORTED


# ---- the wide-rank golden fixtures (tools/make_golden_wide_rank.py) agree with the fp64 oracle -------------------------------------
@pytest.mark.parametrize("name", ["wide_cell_v1", "wide_seq_v1", "wide_seq_v2", "wide_seq_v5", "wide_seq_v6", "wide_lm_v3",
                                  "wide_lm_v4"])
def test_wide_goldens_agree_with_the_oracle(name):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vmlmf_oracle as O
    from conftest import load_golden
    from hip_util import run_literal, assert_out, assert_grad
    d = load_golden(name)
    variant, B, T = (int(v) for v in d["meta"][:3])
    if name.startswith("wide_cell"):
        ref = run_literal(variant, d["P"], d["x"][:, None, :], d["h0"], d["c0"], None, d["dh"], d["dc"])
        assert_out(ref["hT"], d["h1"], "h1")
        assert_out(ref["cT"], d["c1"], "c1")
        assert_grad(ref["dx"][:, 0, :], d["dx"], "dx")
        assert_grad(ref["dh0"], d["dh0"], "dh0")
    elif name.startswith("wide_seq"):
        ref = run_literal(variant, d["P"], d["x"], None, None, d["dy"], d["dhT"], None)
        assert_out(ref["y"], d["y"], "y")
        assert_grad(ref["dx"], d["dx"], "dx")
    else:
        ref = run_literal(variant, d["P"], d["x"], d["h0"], d["c0"], d["dy"], d["dhT"], d["dcT"], time_major=True)
        assert_out(ref["y"], d["y"], "y")
        assert_grad(ref["dx"], d["dx"], "dx")
        assert_grad(ref["dc0"], d["dc0"], "dc0")
    for k, v in d["G"].items():
        assert_grad(ref["G"][k], v, "G." + k)
    assert O.V1 <= variant <= O.V6
