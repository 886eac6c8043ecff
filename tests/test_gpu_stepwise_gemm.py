"""GPU: the GEMM dispatch of the step-wise family (vmlmf_generic.hip) at every selection boundary, against the fp64 oracle.

Each timestep of a step-wise layer runs its products through gemm(), launch_dq_split and launch_dhrec, which pick one of about ten
kernel instantiations from M, N and K; a wide layer adds the x-side GEMMs, four transposed-A weight-gradient products (gemm_at) and
the chunked column sums.  Every row of CASES sits on one side of one of those rules, named in its comment as the dispatcher writes
it, and lists the instantiation(s) it is there to reach; test_kernel_map checks that the launches really include them, so that a
change to the dispatcher cannot move a case off its branch unnoticed.

Notation: GK = G * KH (the padded hidden rank summed over groups), NT = thread slots (64 per 64-unit wave of a group),
TB = T * B, tiles = ceil(M / 64) * ceil(N / 64).  S8 / S12 = gemm_skinny_kernel<8,0,8,1> / <8,0,12,1>.
The products: Q = H_{t-1} Ud (M = B, N = GK, K = H), P = Q Vd with the gate epilogue (gemm_tile_kernel<1>), dQ = dpre VdT in two
K-halves (launch_dq_split, K = 4 NT), dH_rec = dQ UdT (launch_dhrec: gemm_rows16_kernel<2,2>, <0,2> at t = 0); narrow x side
qx = X U_x (generic_qx, K = I) and dqx = dpre VxT (quad image, gemm_skinny_kernel<8,2,12,*>); wide x side qx, gx = qx VXD,
dqx = dpre VxT (K = 4 NT), dxs = dqx U_x^T (K = KX) and the gemm_at products (K = TB); wide_colsum_kernel in WIDE_NCH = 64 chunks.

Not reachable with the default switches, and so not listed: gemm_rows16_kernel<2,1> / <0,1> and gates_fwd_kernel (only with
VMLMF_DQ_SPLIT=0 or VMLMF_FUSE_GATES=0/3, read once when the library loads); a skinny dxs (it needs N = I <= 128 with K = KX >= 256,
but a wide layer has w_rank <= I).  The non-wide one-group layers at KH = 32 are taken by the clustered family by default, so the
non-wide cases below use u_rank 40 (KH = 40), which the default plan keeps on the step-wise path.

Tolerances: tests/hip_util.py, plus assert_edges below (the last partial 16- and 64-row and -column blocks of every gradient)."""
import numpy as np
import pytest
import torch

import vmlmf_oracle as O
from hip_util import ORDER, run_hip, run_literal, compare_all, assert_grad
from vmlmf_amd import _lib, vmlmf_sequence

pytestmark = pytest.mark.gpu
DEV = "cuda"
GROUPED = (O.V2, O.V4, O.V6)

S8, S12 = "gemm_skinny_kernel<8,0,8,1>", "gemm_skinny_kernel<8,0,12,1>"
QUAD1, QUAD2 = "gemm_skinny_kernel<8,2,12,1>", "gemm_skinny_kernel<8,2,12,2>"
TILE0, TILE1 = "gemm_tile_kernel<0>", "gemm_tile_kernel<1>"
R16E, R16 = "gemm_rows16_kernel<2,2>", "gemm_rows16_kernel<0,2>"
COLSUM, CG = "wide_colsum_kernel", "wide_cg_kernel"

# name: (variant, B, T, I, H, w_rank, u_ranks, time_major, with_state, need_dx, kernels that must launch, kernels that must not)
CASES = {
    # ---- Q product of a non-wide one-group layer: gemm() takes the skinny kernel when N <= 128 && K >= 256, and its 12-stage
    # form when K >= 1536 (K = H).  (dQ: NT = 1536, K / DQ_ZS = 3072 >= 1536: S12 in launch_dq_split for both.)
    "q_H1535_s8": (O.V1, 3, 3, 64, 1535, 16, [40], False, True, True, [S8, S12, R16E, R16, TILE1, QUAD1], []),
    "q_H1536_s12": (O.V1, 3, 3, 64, 1536, 16, [40], False, True, True, [S12, R16E, R16, TILE1, QUAD1], []),
    # ---- dQ = dpre VdT (launch_dq_split): K / DQ_ZS >= 1536 picks S12, i.e. NT >= 768 (H >= 705 for one group).  B = 19: a ragged
    # 16-row tile in both halves and in gemm_rows16_kernel; H % 64 != 0 (720, 705): a ragged 64-column tile of dH_rec
    "dq_v1_H704_s8": (O.V1, 19, 3, 64, 704, 16, [40], False, True, True, [S8, R16E, R16, TILE1, QUAD1], [S12]),
    "dq_v1_H720_s12": (O.V1, 19, 3, 64, 720, 16, [40], False, True, True, [S12, R16E, R16], []),
    # (V3, time-major: qx = X U_x with K = I = 704 >= 256 and N = KX = 16 is S8 as well)
    "dq_v3_H704_s8": (O.V3, 19, 3, 704, 704, 16, [40], True, True, True, [S8, R16E, R16, QUAD1], [S12]),
    "dq_v3_H705_s12": (O.V3, 19, 3, 705, 705, 16, [40], True, True, False, [S12, R16E, R16, QUAD1], []),
    # ---- dqx of a narrow layer on the quad image: gemm_skinny_kernel<8,2,12,2> when N % 32 == 0 && t16 >= 1024
    # (t16 = ceil(TB / 16) * ceil(KX / 16): KX = 32 and TB = 8192)
    "dqx_quad_two_subtiles": (O.V1, 128, 64, 48, 64, 32, [40], True, False, True, [QUAD2, R16E, R16, TILE1], [CG]),
    # ---- split-K tile path (wide layers, Q: N = GK > 128): gemm_tile_kernel<0> with nz > 1 when tiles < 64 && K >= 256,
    # nz = min(ceil(K / 128), GEMM_MAX_SPLIT = 8)
    "splitk_nz2_B960_tiles60": (O.V1, 960, 2, 64, 256, 16, [200], False, False, True, [TILE0, TILE1, CG], []),   # 15 * 4 tiles, nz 2
    "splitk_off_B1008_tiles64": (O.V1, 1008, 2, 64, 256, 16, [200], False, False, True, [TILE0, TILE1, CG], []),  # 16 * 4 tiles, nz 1
    "splitk_nz8_H1100": (O.V1, 3, 3, 64, 1100, 16, [150], False, True, True, [TILE0, TILE1, S12, CG], []),  # ceil(1100/128) = 9 -> 8
    "splitk_group_v2": (O.V2, 5, 4, 64, 512, 16, [72, 64], False, True, True, [TILE0, TILE1, S8, CG], []),   # GK 272, K 512: nz 4
    # (flat V4; qx: N = KX = 40 <= 128, K = I = 384 >= 256: S8)
    "splitk_group_v4": (O.V4, 6, 3, 384, 384, 40, [100, 60], True, True, True, [TILE0, TILE1, S8, CG], []),   # GK 336, nz 3
    # ---- wide ranks beyond 300.  KX > 128: qx, dqx and dxs are tile products (N > 128), whole K in one workgroup
    "wide_v5_kx600_I_gt_H": (O.V5, 4, 6, 700, 160, 600, [40], True, True, True, [TILE0, TILE1, COLSUM, CG], []),
    # both caps: KX = KH = 1024; Q: 16 tiles, K = 1024 -> nz 8; dQ: NT = 1024 -> S12 with N = 1024
    "wide_v3_caps_1024": (O.V3, 2, 2, 1024, 1024, 1024, [1024], True, True, True, [TILE0, TILE1, S12, COLSUM, CG], []),
    # w_rank 1017 pads to 1024; Q: N = GK = 40, K = 1024: S8
    "wide_v1_rw1017": (O.V1, 2, 3, 1024, 1024, 1017, [40], False, True, True, [TILE0, TILE1, S8, S12, CG], []),
    # ---- the narrow / wide switch: wide = KX > 32 || GK > 128, on otherwise equal layers.  Narrow: generic_qx and the quad dqx;
    # wide: wide_gx_kernel, the dense dqx (N = KX = 40 <= 128, K = 4 NT = 768: S8) and the canonical-gradient kernels
    "switch_rw32_narrow": (O.V1, 5, 4, 64, 180, 32, [40], False, True, True, [QUAD1, R16E, R16], [CG, COLSUM]),
    "switch_rw33_wide": (O.V1, 5, 4, 64, 180, 33, [40], False, True, True, [S8, COLSUM, CG, "wide_gx_kernel"], [QUAD1]),
    "switch_gk128_narrow": (O.V1, 5, 4, 64, 180, 16, [128], False, True, True, [QUAD1], [CG, COLSUM]),
    "switch_gk136_wide": (O.V1, 5, 4, 64, 180, 16, [129], False, True, True, [COLSUM, CG, "wide_dx_kernel"], [QUAD1]),
    # ---- wide layers with many rows: wide_colsum_kernel cuts TB rows into nch = min(TB, WIDE_NCH) chunks of ceil(TB / nch);
    # gemm_at runs K = TB in one workgroup per tile
    "rows_TB63": (O.V1, 9, 7, 48, 64, 40, [40], False, True, True, [COLSUM, CG, "wide_rows_kernel"], []),
    "rows_TB64": (O.V1, 8, 8, 48, 64, 40, [40], True, True, True, [COLSUM, CG], []),
    "rows_TB65": (O.V1, 13, 5, 48, 64, 40, [40], False, False, True, [COLSUM, CG], []),   # 2 rows a chunk, the last 31 empty
    # TB = 16384, batch-first: x and h_{t-1} through wide_rows_kernel (the reorder and the one-step shift)
    "rows_16k_batch_first": (O.V1, 128, 128, 48, 64, 40, [40], False, True, True, [COLSUM, CG, "wide_rows_kernel"], []),
    "rows_16k_time_major_v2": (O.V2, 256, 64, 48, 64, 40, [32, 24], True, True, False, [COLSUM, CG], []),
}
SPLITK = ["splitk_nz2_B960_tiles60", "splitk_nz8_H1100", "splitk_group_v2", "splitk_group_v4", "wide_v3_caps_1024"]


def _scale(I, H, rw, ru):
    """Parameter scale: 0.1, or 1 / sqrt(fan-in) once a contraction is longer than 100.  At 0.1 the pre-activations of a layer with
    K ~ 1000 reach ~10 and the fp32 rounding of the products alone exceeds the outputs' absolute tolerance (1e-5): the same layer
    evaluated in fp32 on the host missed it too, so such a failure says nothing about the kernels."""
    return min(0.1, 1.0 / np.sqrt(max(I, H, rw, sum(ru))))


def _io(name):
    variant, B, T, I, H, rw, ru, tm, with_state = CASES[name][:9]
    rng = np.random.Generator(np.random.PCG64(sum(map(ord, name)) + 31 * H))
    P = O.make_params(variant, I, H, rw, ru if variant in GROUPED else ru[0], seed=H + rw + B, scale=_scale(I, H, rw, ru))
    shp = (T, B, I) if tm else (B, T, I)
    x = rng.standard_normal(shp).astype(np.float32)
    h0 = (0.4 * rng.standard_normal((B, H))).astype(np.float32) if with_state else None
    c0 = (0.4 * rng.standard_normal((B, H))).astype(np.float32) if with_state else None
    dy = rng.standard_normal(shp[:2] + (H,)).astype(np.float32)
    dhT = rng.standard_normal((B, H)).astype(np.float32)
    dcT = rng.standard_normal((B, H)).astype(np.float32)
    return P, x, h0, c0, dy, dhT, dcT


def _hip(name):
    variant, tm, need_dx = CASES[name][0], CASES[name][7], CASES[name][9]
    P, x, h0, c0, dy, dhT, dcT = _io(name)
    return run_hip(variant, P, x, h0, c0, dy, dhT, dcT, time_major=tm, need_dx=need_dx)


# ---- B. the edge-tile gradient check ------------------------------------------------------------------------------------------
EDGE_FLOOR = 0.01   # a block's scale is at least this share of the whole gradient's largest value


def _edge_blocks(R, C):
    """The last (partial, where the size is not a multiple) 16- and 64-row blocks and 16- and 64-column blocks of an R x C array."""
    out = []
    for n in (16, 64):
        r0, c0 = (R - 1) // n * n, (C - 1) // n * n
        out.append((f"rows[{r0}:{R}]", np.s_[r0:R, :]))
        out.append((f"cols[{c0}:{C}]", np.s_[:, c0:C]))
    return out


def assert_edges(a, b, what, rel=1e-4):
    """assert_grad on the whole gradient, then on each edge block S of it viewed as 2-D (leading dimensions x last):
    max|a_S - b_S| <= rel * max(max|b_S|, EDGE_FLOOR * max|b|) + 1e-6.  A masked edge tile whose values are small next to the
    array's maximum is invisible to the whole-array bound; here it is held to its own scale."""
    assert_grad(a, b, what, rel=rel)
    a2 = np.asarray(a, np.float64).reshape(-1, np.shape(a)[-1])
    b2 = np.asarray(b, np.float64).reshape(a2.shape)
    full = np.abs(b2).max()
    for tag, s in _edge_blocks(*a2.shape):
        aS, bS = a2[s], b2[s]
        err, scale = np.abs(aS - bS).max(), max(np.abs(bS).max(), EDGE_FLOOR * full)
        assert err <= rel * scale + 1e-6, f"{what} {tag}: max err {err:.3e} vs block scale {scale:.3e} (whole array {full:.3e})"


def compare_strict(got, ref, tag):
    compare_all(got, ref, tag)
    problems = []
    grads = [(k, got[k], ref[k]) for k in ("dx", "dh0", "dc0") if k in got and k in ref]
    grads += [("G." + k, got["G"][k], ref["G"][k]) for k in ref["G"]]
    for k, a, b in grads:
        try:
            assert_edges(a, b, f"{tag}.{k}")
        except AssertionError as e:
            problems.append(str(e))
    assert not problems, "\n".join(problems)


# ---- A. every case against the fp64 oracle ---------------------------------------------------------------------------------------
def _is_stepwise(name):
    variant, B, T, I, H, rw, ru, tm = CASES[name][:8]
    g = 2 if variant in GROUPED else 1
    s = _lib.query(_lib.make_desc(variant, B, T, I, H, rw, ru, g=g, time_major=tm, training=True))
    KH, NT = s.kh, g * ((H // g + 63) // 64) * 64
    return s.rows_per_wg == 1 and (KH > 32 or NT > 512 or I > H)


@pytest.mark.parametrize("name", list(CASES))
def test_case_vs_oracle(name):
    assert _is_stepwise(name), f"{name} is not on the step-wise path"
    variant, tm = CASES[name][0], CASES[name][7]
    P, x, h0, c0, dy, dhT, dcT = _io(name)
    got = _hip(name)
    ref = run_literal(variant, P, x, h0, c0, dy, dhT, dcT, time_major=tm)
    compare_strict(got, ref, name)


def _launched(fn):
    """Names of the GPU kernels fn launches (torch.profiler, device activity), spaces removed."""
    from torch.profiler import profile, ProfilerActivity
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.name.replace(" ", "") for e in prof.events()}


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_map(name):
    want, absent = CASES[name][10], CASES[name][11]
    names = _launched(lambda: _hip(name))
    seen = lambda k: any(k in n for n in names)   # noqa: E731
    assert any("gemm_" in n for n in names), f"the profiler reported none of the library's kernels: {sorted(names)[:20]}"
    missing = [k for k in want if not seen(k)]
    extra = [k for k in absent if seen(k)]
    lib_names = sorted(n for n in names if "kernel" in n)
    assert not missing and not extra, f"{name}: missing {missing}, unexpected {extra}; launched {lib_names}"


@pytest.mark.parametrize("name,want,absent", [("q_H1535_s8", S8, S12), ("q_H1536_s12", S12, S8)])
def test_q_product_switch_in_the_forward(name, want, absent):
    """The forward alone has one skinny product (Q), so the 8 / 12-stage switch at K = H = 1536 is seen without dQ's launches."""
    variant, tm = CASES[name][0], CASES[name][7]
    P, x, h0, c0, *_ = _io(name)
    params = [torch.tensor(np.asarray(P[k]), device=DEV) for k in ORDER[variant]]
    xt, h0t, c0t = (torch.tensor(a, device=DEV) for a in (x, h0, c0))
    rw, ru = CASES[name][5], CASES[name][6]
    with torch.no_grad():
        names = _launched(lambda: vmlmf_sequence(variant, xt, h0t, c0t, params, rw, ru, time_major=tm))
    assert any(want in n for n in names) and not any(absent in n for n in names), sorted(n for n in names if "kernel" in n)


# ---- determinism and the split-K tickets --------------------------------------------------------------------------------------
def _assert_same(a, b, tag):
    for k in ("y", "hT", "cT", "dx", "dh0", "dc0"):
        if k in a:
            assert np.array_equal(a[k], b[k]), f"{tag}: {k} differs"
    for k in a["G"]:
        assert np.array_equal(a["G"][k], b["G"][k]), f"{tag}: G.{k} differs"


@pytest.mark.parametrize("name", SPLITK)
def test_split_k_call_is_bit_identical_run_to_run(name):
    _assert_same(_hip(name), _hip(name), name)


def test_split_k_tickets_are_back_at_zero_for_the_next_layer():
    """Split-K call, a different split-K layer, the first again: the library promises no float atomics and tickets that are zero
    on entry and on exit, so the third call reproduces the first bit for bit."""
    a = _hip("splitk_nz8_H1100")
    _hip("splitk_group_v2")
    _assert_same(a, _hip("splitk_nz8_H1100"), "after another split-K layer")
    b = _hip("splitk_nz2_B960_tiles60")
    _hip("wide_v3_caps_1024")
    _assert_same(b, _hip("splitk_nz2_B960_tiles60"), "after the caps layer")
