"""Golden vectors of wide-rank layers (padded w_rank > 32 or padded hidden rank > 128: the step-wise path's rank-agnostic x side
and weight gradients), captured from the imported reference through oracle/make_golden.py's case helpers under fixture names of
their own.  Build container only (needs the reference checkout that make_golden.py imports); the .npz files travel.

    python tools/make_golden_wide_rank.py            # every fixture below
    python tools/make_golden_wide_rank.py NAME...    # only the named ones

Sizes stay moderate (all fixtures together well under 2 MB): the full-size LM layer is checked against the fp64 oracle instead
(tests/test_gpu_wide_rank.py).  MyVMLSTMGroup runs at B = 40 only (its scratch rows are hard-coded in the reference)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))

import make_golden as MG   # noqa: E402  (imports the reference modules)
import vmlmf_oracle as O   # noqa: E402

CASES = {
    # bare cell (T = 1): w_rank 40 (padded 40 > 32), u_rank 64
    "wide_cell_v1": lambda n: MG.case_bare_cell(n, O.V1, 5, 48, 96, 40, 64, 61),
    # one layer through MyLSTM, batch-first, zero initial state
    "wide_seq_v1": lambda n: MG.case_har_seq(n, O.V1, 3, 5, 40, 48, 36, [40], 62),
    "wide_seq_v2": lambda n: MG.case_har_seq(n, O.V2, 3, 5, 40, 48, 36, [20, 20], 63),
    "wide_seq_v5": lambda n: MG.case_har_seq(n, O.V5, 3, 5, 40, 48, 36, [40], 64),
    "wide_seq_v6": lambda n: MG.case_har_seq(n, O.V6, 3, 5, 40, 48, 37, [20, 18], 65),
    # LM layers, time-major, non-zero initial state and dhT / dcT
    "wide_lm_v3": lambda n: MG.case_lm_seq(n, O.V3, 4, 5, 48, 40, 44, 66),
    "wide_lm_v4": lambda n: MG.case_lm_seq(n, O.V4, 40, 3, 48, 36, [20, 20], 67),
}


def main(argv):
    os.makedirs(MG.OUT, exist_ok=True)
    for name in (argv or list(CASES)):
        CASES[name](name)


if __name__ == "__main__":
    main(sys.argv[1:])
