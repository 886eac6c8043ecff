"""The conditions that make tests/test_gpu_hot_regime.py meaningful, checked without a GPU on every row of tests/hot_cases.py's tables:
the gates are saturated (hot tier) or on the rails, past the point where exp leaves fp32 (rail tier); the cell state is large; and plain
fp32 arithmetic - the literal oracle in fp32 against itself in fp64 - stays within a third of the suite's tolerance, so a kernel that
misses the tolerance there is wrong, not unlucky.  Also: the seeded hot runs of tools/fuzz_parity.py stay within their redraw cap, and the
suite's standard draw saturates nothing (the gap this regime closes, in executable form).  docs/design/value_regimes.md has the numbers."""
import os
import sys

import numpy as np
import pytest

import vmlmf_oracle as O
import hot_cases as HC

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_draw  # noqa: E402

CPU_ROWS_CAP = 2_000_000        # B T H beyond this: the conditions are checked at B = 8, same T


def c_floor(T, with_state):
    """The cell state a hot row must reach.  From c0 = 4 N(0, 1) it is 8.  A row without initial states starts at c = 0 and
    |c_t| <= |c_(t-1)| + 1 (every gate lies in [0, 1], |tanh| <= 1), so before step 8 it cannot be there whatever the kernel does: such a
    row must come within a tenth of that ceiling instead, which the units with forget gate, input gate and candidate all on their
    rails do."""
    return 8.0 if with_state else min(8.0, 0.9 * T)


def check_conditions(tier, st, name, share, tag, T, with_state):
    line = (f"{tag} {tier}: |pre| > 4 {st['gt4']:.3f}, > 16 {st['gt16']:.3f}, > 88.7 {st['gt88']:.4f}, max |pre| {st['max_pre']:.1f}, "
            f"max |c| {st['max_c']:.1f}, fp32 oracle worst {name} {share:.3f} x tolerance")
    print("\n" + line)
    if tier == "hot":
        assert st["gt4"] >= 0.30 and st["max_c"] >= c_floor(T, with_state), line
    else:
        assert st["gt16"] >= 0.5 and st["gt88"] >= 0.01, line
        assert st["og_low"].any(), line + ": no unit's output gate stays below -88.7 (the rail assertions on y would check nothing)"
    assert share <= HC.FP32_SHARE, line


LAYER_ROWS = [(fam, row, tier) for fam, rows in HC.LAYER_TABLES.items() for row in rows for tier in row[9]]


@pytest.mark.parametrize("fam,row,tier", LAYER_ROWS, ids=lambda v: HC.row_id(v) if isinstance(v, tuple) else str(v))
def test_layer_rows_are_in_the_regime_and_within_reach_of_fp32(fam, row, tier):
    v, B, T, I, H = row[:5]
    Bc = 8 if B * T * H > CPU_ROWS_CAP else None
    P, x, h0, c0, dy, dhT, dcT = HC.row_inputs(row, tier, B=Bc)
    st = HC.gate_stats(v, P, x, h0, c0, row[7])
    name, share = HC.fp32_oracle_share(v, P, x, h0, c0, dy, dhT, dcT, row[7])
    check_conditions(tier, st, name, share, f"{fam} {HC.row_id(row)}", T, row[8])


STACK_ROWS = [("rbx", row, tier) for row in HC.RBX for tier in row[4]] + [("wave", row, tier) for row in HC.WAVE for tier in row[8]]


@pytest.mark.parametrize("fam,row,tier", STACK_ROWS, ids=lambda v: "_".join(str(e) for e in v[:5]).replace(" ", "") if isinstance(v, tuple) else str(v))
def test_stack_rows_are_in_the_regime_and_within_reach_of_fp32(fam, row, tier):
    if fam == "rbx":
        Ps, x, h0, c0, dy, dhT, dcT = HC.rbx_inputs(row, tier, B=8 if row[2] * row[3] * HC.RBX_H > CPU_ROWS_CAP else None)
        tm = True
    else:
        Ps, x, h0, c0, dy, dhT, dcT = HC.wave_inputs(row, tier)
        tm = False
    st = HC.stack_gate_stats(row[0], Ps, x, h0, c0, tm)
    name, share = HC.fp32_stack_share(row[0], Ps, x, h0, c0, dy, dhT, dcT, tm)
    check_conditions(tier, st, name, share, f"{fam} {row[:5]}", x.shape[0 if tm else 1], h0 is not None)


def test_gate_stats_leaves_the_oracle_as_it_found_it():
    plain = O._lstm_tail
    P, x, h0, c0, *_ = HC.row_inputs(HC.VALU[0], "rail")
    with pytest.raises(KeyError):
        HC.gate_stats(O.V1, {k: v for k, v in P.items() if k != "b_h"}, x, h0, c0)
    assert O._lstm_tail is plain
    st = HC.gate_stats(O.V1, P, x, h0, c0)
    assert O._lstm_tail is plain and st["og_low"].shape == h0.shape


def test_the_standard_draw_saturates_nothing():
    """The regression note: test_seeded_shapes_vs_oracle's first three cases, drawn as the cold-regime suite draws them (make_params'
    default scale, x ~ N(0, 1), states at 0.4 N(0, 1)), have no pre-activation beyond 4 at all."""
    for variant, B, T, I, H, rw, ru, tm, with_state in [(O.V1, 3, 5, 4, 16, 2, [3], False, False), (O.V1, 7, 9, 16, 64, 8, [8], False, True),
                                                        (O.V1, 5, 4, 9, 65, 5, [11], True, True)]:
        rng = np.random.Generator(np.random.PCG64(1000 + B + 7 * T + 13 * H))
        P = O.make_params(variant, I, H, rw, ru[0], seed=H + rw)
        x = rng.standard_normal((T, B, I) if tm else (B, T, I)).astype(np.float32)
        h0 = (0.4 * rng.standard_normal((B, H))).astype(np.float32) if with_state else None
        c0 = (0.4 * rng.standard_normal((B, H))).astype(np.float32) if with_state else None
        st = HC.gate_stats(variant, P, x, h0, c0, tm)
        assert st["gt4"] == 0 and st["max_c"] < 2, st


@pytest.mark.parametrize("mode,cases,seed", [("seq", 40, 21), ("rb", 25, 22), ("stack", 25, 23)])
def test_seeded_hot_fuzz_draws_stay_within_the_redraw_cap(mode, cases, seed):
    """The draws of tests/test_gpu_fuzz.py's hot runs and their fp32-against-fp64 check need no GPU: replayed here."""
    redrawn = fuzz_draw.hot_redraws(mode, cases, seed)
    print(f"\nfuzz {mode} hot seed {seed}: {cases} cases, {redrawn} redrawn (fp32 oracle)")
    assert redrawn <= fuzz_draw.REDRAW_CAP * cases
