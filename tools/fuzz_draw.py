"""The draws of tools/fuzz_parity.py: shapes, ranks and variants from one seeded stream, and - for the saturated-gate regime
(tests/hot_cases.py, docs/design/value_regimes.md) - the values of a drawn case and the check that plain fp32 arithmetic can meet the
suite's tolerance on it.  Nothing here touches the HIP library: tests/test_hot_regime_cpu.py replays the seeded draws on the CPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np
import vmlmf_oracle as O

VARIANTS = [O.V1, O.V2, O.V3, O.V4, O.V5, O.V6]
HOT_MODES = ("seq", "rb", "stack")
HOT_T_CAP = 48
RAIL_SHARE = 0.25           # of the hot cases
REDRAW_CAP = 0.10           # of the cases: more redraws than this fail a hot run
rng = None
MODE = "seq"


def init(seed, mode):
    global rng, MODE
    rng = np.random.Generator(np.random.PCG64(seed))
    MODE = mode
    return rng


def pick(lo, hi, small=0.5):
    """mostly small values, sometimes up to hi"""
    if rng.random() < small:
        return int(rng.integers(lo, min(hi, lo + 12) + 1))
    return int(rng.integers(lo, hi + 1))


def draw():
    v = VARIANTS[int(rng.integers(0, len(VARIANTS)))]
    group = v in (O.V2, O.V4, O.V6)
    H = pick(2, 300, 0.3)
    if group and H % 2:
        H += 1
    novm = v in (O.V5, O.V6)
    lm = v in (O.V3, O.V4)            # the LM layers need input_size == hidden_size (vmlmf_lm.py:243)
    if lm:
        H = min(H, 160)
    I = H if lm else pick(2, 150 if novm else min(H, 150), 0.4)   # (I = 1: the reference's own squeeze() breaks the literal oracle)
    rw = pick(1, 32, 0.3)             # narrow ranks (padded <= 32 / hidden <= 128 summed): every kernel family; wider: MODE "wide"
    ru = [pick(1, 32, 0.3), pick(1, 32, 0.3)] if group else pick(1, 32, 0.3)
    B, T = pick(1, 200, 0.4), pick(1, 40, 0.4)
    if MODE == "big":
        B, T = int(rng.integers(64, 1101)), int(rng.integers(16, 201))
        H = int(rng.integers(32, 701)) + (0 if not group else 0)
        if group and H % 2:
            H += 1
        if lm:
            H = min(H, 660)
            I = H
        else:
            I = int(rng.integers(2, (150 if novm else min(H, 150)) + 1))
        while B * T * H > 24_000_000:      # keeps the float64 oracle of a case within seconds
            T = max(8, T // 2)
    if v == O.V4 and B == 1:
        B = 2                         # (B = 1: the reference's squeeze() in vmlmf_lm.py:257 drops the batch dimension and the layer raises)
    return dict(v=v, B=B, T=T, I=I, H=H, rw=rw, ru=ru, states=bool(rng.random() < 0.5), tm=bool(rng.random() < 0.3),
                dy=bool(rng.random() < 0.8), dh=bool(rng.random() < 0.5), dc=bool(rng.random() < 0.4), seed=int(rng.integers(0, 2**31)))


def draw_stack():
    c = draw()
    while c["v"] == O.V4:             # (the flat V4 layout is not on the wavefront kernels)
        c = draw()
    c["L"] = int(rng.integers(2, 5))
    c["H"] = min(c["H"], 256)
    if c["v"] in (O.V2, O.V6) and c["H"] % 2:
        c["H"] += 1
    if c["v"] == O.V3:
        c["I"] = c["H"]
    elif c["v"] == O.V5 or c["v"] == O.V6:
        pass
    else:
        c["I"] = min(c["I"], c["H"])
    c["B"], c["T"] = min(c["B"], 128), min(c["T"], 30)
    if c["v"] in (O.V1, O.V5) and rng.random() < 0.35:      # growing hidden sizes (a VMLMF cell needs input_size <= hidden_size)
        hs = sorted(int(min(256, max(c["I"] if c["v"] == O.V1 else 2, pick(2, 256, 0.2)))) for _ in range(c["L"]))
        c["Hs"], c["H"] = hs, hs[0]
        if c["v"] == O.V1:
            c["I"] = min(c["I"], hs[0])
    return c


# ---- the saturated-gate regime -----------------------------------------------------------------------------------------------------------
def _ranks(c):
    return list(c["ru"]) if isinstance(c["ru"], (list, tuple)) else [c["ru"]]


def hot_values(c):
    """The values of a drawn case by hot_inputs' rule: a layer's (P, x, h0, c0, dy, dhT, dcT) - upstream gradients the case did not
    draw are None - or a stack's (Ps, x, h0, c0, dy, dhT, None), the hot draw per layer."""
    import hot_cases as HC
    if "L" in c:
        Hs = c.get("Hs") or [c["H"]] * c["L"]
        states = c["states"] and len(set(Hs)) == 1
        Ps, x, h0, c0, dy, dhT, _ = HC.hot_stack_inputs(c["v"], c["B"], c["T"], c["I"], Hs, c["rw"], _ranks(c), c["tier"], c["tm"], states, seed=c["seed"])
        return Ps, x, h0, c0, dy, dhT, None
    P, x, h0, c0, dy, dhT, dcT = HC.hot_inputs(c["v"], c["B"], c["T"], c["I"], c["H"], c["rw"], _ranks(c), c["tier"], c["tm"], c["states"], seed=c["seed"])
    dy, dcT = (dy if c["dy"] else None), (dcT if c["dc"] else None)
    if not c["dh"] and (dy is not None or dcT is not None):
        dhT = None
    return P, x, h0, c0, dy, dhT, dcT


def fp32_share(c, vals):
    """Worst share of the suite's tolerance that the fp32 literal oracle uses against the fp64 one on these values."""
    import hot_cases as HC
    fn = HC.fp32_stack_share if "L" in c else HC.fp32_oracle_share
    return fn(c["v"], *vals, c["tm"])[1]


def draw_hot():
    """One case of the current mode in the regime: drawn as ever (T capped), the tier rail one time in four, drawn again while
    plain fp32 cannot meet a third of the tolerance on it.  Returns (case, values, redraws)."""
    import hot_cases as HC
    redraws = 0
    while True:
        c = draw_stack() if MODE == "stack" else draw()
        c["T"] = min(c["T"], HOT_T_CAP)
        c["tier"] = "rail" if rng.random() < RAIL_SHARE else "hot"
        vals = hot_values(c)
        if fp32_share(c, vals) <= HC.FP32_SHARE:
            return c, vals, redraws
        redraws += 1


def hot_redraws(mode, cases, seed):
    """The redraw count of `fuzz_parity.py cases seed mode hot`, replayed without a GPU."""
    init(seed, mode)
    return sum(draw_hot()[2] for _ in range(cases))
