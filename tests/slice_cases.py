"""The inputs and case tables of the slice-wise and structural tests of the recurrent kernels (docs/design/slice_tolerances.md): the rows of
tests/hot_cases.py's tables - the smallest shapes that select each kernel family - with ordinary values (O.make_params at the suite's
scale, x ~ N(0, 1)) and the two upstream-gradient patterns the whole-tensor rule of tests/hip_util.py is blind to.  Read by
tests/test_slice_compare_cpu.py (the inputs' conditions, CPU), tests/test_gpu_slices.py and tests/test_gpu_structure.py (the kernels, GPU).
Helpers only: no test lives here."""
import numpy as np
import torch

import hot_cases as HC
import vmlmf_oracle as O
from hip_util import compare_slices, run_literal

V1, V2, V3, V4, V5, V6 = O.V1, O.V2, O.V3, O.V4, O.V5, O.V6
PATTERNS = ("last", "rows")
# last: dy = None, dense dhT (and dcT where the case has states): the classifier's case, dx decays by orders of magnitude towards t = 0
# rows: dense dy, dhT, dcT, row b multiplied by 10 ** (-6 b / (B - 1)): rows of very different loss weight


def _g(variant):
    return 2 if variant in HC.GROUPED else 1


def layout(variant, H, time_major):
    """The layout compare_all(..., slices=) and compare_slices take."""
    return {"variant": variant, "H": H, "g": _g(variant), "time_major": time_major}


def row_weights(B):
    return (10.0 ** (-6.0 * np.arange(B) / (B - 1))).astype(np.float32)


def _scale_rows(a, w, time_major):
    return a * (w[None, :, None] if time_major else w[:, None, None])


def ordinary_inputs(row, pattern="dense"):
    """P, x, h0, c0, dy, dhT, dcT (numpy) of one layer row with ordinary values.  One PCG64 stream per row: x, h0, c0, dy, dhT, dcT."""
    v, B, T, I, H, rw, ru, tm, st = row[:9]
    seed = HC.case_seed(v, B, T, I, H, rw) + 424243
    rng = np.random.Generator(np.random.PCG64(seed))
    P = O.make_params(v, I, H, rw, list(ru) if v in HC.GROUPED else ru[0], seed=seed + 1, scale=HC.param_scale(H))
    shp = (T, B, I) if tm else (B, T, I)
    x = rng.standard_normal(shp).astype(np.float32)
    h0 = (0.5 * rng.standard_normal((B, H))).astype(np.float32)
    c0 = (0.5 * rng.standard_normal((B, H))).astype(np.float32)
    dy = rng.standard_normal(shp[:2] + (H,)).astype(np.float32)
    dhT = rng.standard_normal((B, H)).astype(np.float32)
    dcT = rng.standard_normal((B, H)).astype(np.float32)
    if not st:
        h0 = c0 = None
    if pattern == "last":
        dy = None
        if not st:
            dcT = None
    elif pattern == "rows":
        w = row_weights(B)
        dy, dhT, dcT = _scale_rows(dy, w, tm), dhT * w[:, None], dcT * w[:, None]
    else:
        assert pattern == "dense", pattern
    return P, x, h0, c0, dy, dhT, dcT


def ordinary_stack_inputs(variant, B, T, I, Hs, rw, ru, time_major, with_state, pattern="dense"):
    """A stack's inputs with ordinary values: Ps (list), x, h0, c0 (lists of (B, H_l), or None), dy, dhT, dcT (lists)."""
    seed = HC.case_seed(variant, B, T, I, Hs[-1], len(Hs)) + 424243
    rng = np.random.Generator(np.random.PCG64(seed))
    Ps = [O.make_params(variant, I if l == 0 else Hs[l - 1], H, rw, list(ru) if variant in HC.GROUPED else ru[0], seed=seed + 1 + l,
                        scale=HC.param_scale(H)) for l, H in enumerate(Hs)]
    shp = (T, B, I) if time_major else (B, T, I)
    x = rng.standard_normal(shp).astype(np.float32)
    h0 = [(0.5 * rng.standard_normal((B, H))).astype(np.float32) for H in Hs]
    c0 = [(0.5 * rng.standard_normal((B, H))).astype(np.float32) for H in Hs]
    dy = rng.standard_normal(shp[:2] + (Hs[-1],)).astype(np.float32)
    dhT = [rng.standard_normal((B, H)).astype(np.float32) for H in Hs]
    dcT = [rng.standard_normal((B, H)).astype(np.float32) for H in Hs]
    if not with_state:
        h0 = c0 = None
    if pattern == "last":
        dy = None
    elif pattern == "rows":
        w = row_weights(B)
        dy, dhT, dcT = _scale_rows(dy, w, time_major), [a * w[:, None] for a in dhT], [a * w[:, None] for a in dcT]
    else:
        assert pattern == "dense", pattern
    return Ps, x, h0, c0, dy, dhT, dcT


# ---- the case tables ---------------------------------------------------------------------------------------------------------------------
# a layer case: (family, row of tests/hot_cases.py's layout, switches held while it runs); a stack case: (family, stack row)
# stack rows here: (variant, B, T, I, hidden sizes, w_rank, u_ranks, time_major, with_state)
SIXTEEN = {"rb": 1, "rb_cluster": 16, "rb_rows": 16}


def _rbx(row):
    v, L, B, T = row[:4]
    return (v, B, T, HC.RBX_H, [HC.RBX_H] * L, HC.RBX_RW, HC.rbx_ranks(v), True, True)


def _wave(row):
    v, B, T, I, Hs, rw, ru, st = row[:8]
    return (v, B, T, I, list(Hs), rw, ru, False, st)


LAYER_ROWS = [("valu", row, {}) for row in HC.VALU] + \
             [("valu.rec3=%d" % mask, row, {"rec3": mask}) for row in HC.VALU[:HC.VALU_REC3_ROWS] for mask in (0, 7)] + \
             [("headline", row, {}) for row in HC.HEADLINE] + \
             [("rb", row, {"rb": 1}) for row in HC.RB] + [("rb_cluster", row, {"rb": 1}) for row in HC.RB_CLUSTER] + \
             [("rb_cluster16", HC.RB_CLUSTER16, SIXTEEN)] + [("stepwise", row[:10], row[10]) for row in HC.STEPWISE]
STACK_ROWS = [("rbx", _rbx(row)) for row in HC.RBX] + [("wave", _wave(row)) for row in HC.WAVE]

# the last-step-only pattern: per family the table's row with the largest T and, where the table has no long row, one more row of T = 24 at
# the family's smallest B and a shape of its table (so that the same family is planned)
LONG = {
    "rb": (V1, 2, 24, 30, 200, 16, [24], False, True, HC.HOT),
    "rb_cluster": (V1, 5, 24, 20, 600, 8, [8], False, True, HC.HOT),
    "stepwise": (V1, 3, 24, 12, 40, 6, [40], False, True, HC.HOT),
}
LAST_LAYERS = [("valu", HC.VALU[1], {}), ("valu", HC.VALU[9], {}), ("headline", HC.HEADLINE[1], {}),
               ("rb", HC.RB[0], {"rb": 1}), ("rb", LONG["rb"], {"rb": 1}),
               ("rb_cluster", HC.RB_CLUSTER[1], {"rb": 1}), ("rb_cluster", LONG["rb_cluster"], {"rb": 1}),
               ("rb_cluster16", HC.RB_CLUSTER16, SIXTEEN),
               ("stepwise", HC.STEPWISE[6][:10], HC.STEPWISE[6][10]), ("stepwise", LONG["stepwise"], {})]
LAST_STACKS = [("rbx", _rbx(HC.RBX[0])), ("rbx", (V4, 7, 24, HC.RBX_H, [HC.RBX_H] * 2, HC.RBX_RW, [32, 32], True, True)),
               ("wave", _wave(HC.WAVE[0])), ("wave", (V1, 4, 24, 12, [40, 40, 40], 8, [8], False, True))]
ROWS_LAYERS = [c for c in LAYER_ROWS if c[1][1] >= 2]
ROWS_STACKS = [c for c in STACK_ROWS if c[1][1] >= 2]

GPU_LAYER_CASES = [(c, "last") for c in LAST_LAYERS] + [(c, "rows") for c in ROWS_LAYERS]
GPU_STACK_CASES = [(c, "last") for c in LAST_STACKS] + [(c, "rows") for c in ROWS_STACKS]


def stack_id(row):
    v, B, T, I, Hs, rw, ru, tm, st = row
    return "v%d_B%d_T%d_I%d_H%s_r%d_%s_%s%s" % (v, B, T, I, "x".join(map(str, Hs)), rw, "x".join(map(str, ru)), "tm_" if tm else "", "st" if st else "z")


def case_id(v):
    if isinstance(v, tuple) and len(v) == 2 and isinstance(v[0], tuple):      # (case, pattern)
        return case_id(v[0]) + "-" + v[1]
    if isinstance(v, tuple) and isinstance(v[0], str):
        return v[0] + "-" + (stack_id(v[1]) if isinstance(v[1][4], list) else HC.row_id(v[1]))
    return str(v)


# ---- one fp64 reference per (case, pattern), shared by every test that runs the case ------------------------------------------------------
_REF = {}


def layer_case(row, pattern):
    key = (HC.row_id(row), pattern)
    if key not in _REF:
        inp = ordinary_inputs(row, pattern)
        _REF[key] = (inp, run_literal(row[0], *inp, time_major=row[7]))
    return _REF[key]


def stack_case(row, pattern):
    key = (stack_id(row), pattern)
    if key not in _REF:
        v, B, T, I, Hs, rw, ru, tm, st = row
        inp = ordinary_stack_inputs(v, B, T, I, Hs, rw, ru, tm, st, pattern)
        _REF[key] = (inp, HC.run_stack_literal(v, *inp, tm))
    return _REF[key]


def fp32_slice_report(case, pattern):
    """The fp32 literal oracle against the fp64 one, slice by slice: compare_slices' report (which fails beyond the slice tolerance)."""
    row = case[1]
    if isinstance(row[4], list):
        inp, ref = stack_case(row, pattern)
        got = HC.run_stack_literal(row[0], *inp, row[7], dtype=torch.float32)
    else:
        inp, ref = layer_case(row, pattern)
        got = run_literal(row[0], *inp, time_major=row[7], dtype=torch.float32)
    return compare_slices(got, ref, case_id(case), layout(row[0], row[4], row[7]))
