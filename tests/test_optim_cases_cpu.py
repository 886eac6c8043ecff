"""The bounds of tests/optim_cases.py (docs/design/optimizer_bounds.md) hold and discriminate, without a GPU: an fp32 emulation of each
kernel's operation order stays inside them on every case - product-sums as separate roundings and as fused multiply-adds -, and every
known-wrong variant breaks them on at least one case."""
import numpy as np
import pytest

import optim_cases as C

CASES = [(layout, hyper, start) for layout in C.LAYOUTS for hyper in C.HYPERS for start in C.STARTS]


def seed_of(layout, hyper, start):
    return 100 + 31 * list(C.LAYOUTS).index(layout) + 7 * list(C.HYPERS).index(hyper) + list(C.STARTS).index(start)


def emulated_ratios(fx, hyper, fused, mutate=None):
    want = C.adam_oracle(fx["p"], fx["g"], fx["m"], fx["v"], fx["starts"], **hyper)
    got_p, mf, vf = C.adam_emulate(fx["p"], fx["g"], fx["m_flat"], fx["v_flat"], fx["steps"] + np.float32(1), fx["offsets"], fx["sidx"],
                                   fused=fused, mutate=mutate, **hyper)
    got_m = [mf[o:o + n] for o, n in zip(fx["offsets"], fx["numels"])]
    got_v = [vf[o:o + n] for o, n in zip(fx["offsets"], fx["numels"])]
    return C.adam_ratios(got_p, got_m, got_v, want)


@pytest.mark.parametrize("layout", list(C.LAYOUTS))
def test_the_adam_emulations_stay_inside_the_bounds(layout):
    worst = np.zeros(3)
    for _, hyper, start in (c for c in CASES if c[0] == layout):
        fx = C.adam_fixture(layout, start, seed_of(layout, hyper, start))
        for fused in (False, True):
            r = emulated_ratios(fx, C.HYPERS[hyper], fused)
            assert max(r) <= 1.0, (layout, hyper, start, fused, r)
            worst = np.maximum(worst, r)
    assert worst.min() > 0.0                      # (the emulation does round: the bound is not met by being the oracle)
    print(f"adam emulation {layout}: worst error / bound p {worst[0]:.3f}, m {worst[1]:.3f}, v {worst[2]:.3f}")


def test_the_cases_hold_what_the_bounds_need_to_see():
    """Exact zeros, sqrt(v') at or below eps on a first step and away from it, different step counts inside one list."""
    fx = C.adam_fixture("padded", "mixed", 5)
    assert len(set(fx["starts"])) > 2
    _, _, vn, _ = C.adam_oracle(fx["p"], fx["g"], fx["m"], fx["v"], fx["starts"], **C.HYPERS["defaults"])
    for gi, vi, s in zip(fx["g"][4:], vn[4:], fx["starts"][4:]):
        assert (gi == 0).any() and ((np.sqrt(vi) < 1e-8) & (gi != 0)).any() and (np.sqrt(vi) > 1e-4).any(), s


@pytest.mark.parametrize("mutate", C.ADAM_MUTATIONS)
def test_a_wrong_adam_breaks_the_bounds(mutate):
    """Over the small layouts: the variant exceeds a bound on at least one case (and the cases it needs exist: weight decay for the
    decoupled form, different counters in one list for the neighbour's, eps = 1e-3 on early steps for its placement)."""
    broken = []
    for layout, hyper, start in CASES:
        if layout == "million":
            continue
        fx = C.adam_fixture(layout, start, seed_of(layout, hyper, start))
        r = emulated_ratios(fx, C.HYPERS[hyper], True, mutate)
        if not max(r) <= 1.0:
            broken.append((layout, hyper, start))
    assert broken, f"{mutate} stays inside the bounds on every case"
    print(f"{mutate}: outside the bounds on {len(broken)} of {len(CASES)} cases, first {broken[0]}")


# ---- clip + SGD ----
def norm32(g):
    """An fp32 norm as sqsum_kernel + norm_kernel may leave it: fp32 partial sums per tensor, summed in fp32."""
    with np.errstate(over="ignore"):
        parts = [np.float32((a.astype(np.float32) ** 2).sum(dtype=np.float32)) for a in g]
        return np.sqrt(np.float32(sum(parts, np.float32(0))))


def sgd_ratios(p, g, got, want, lr):
    wp, wg, _, c = want
    worst = [0.0, 0.0]
    for pi, gp, gg, a, b in zip(p, got[0], got[1], wp, wg):
        for k, (x, ref, bound) in enumerate(zip((gp, gg), (a, b), C.sgd_bounds(pi, b, lr=lr, c=c))):
            err = np.abs(x.astype(np.float64) - ref)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(err == 0, 0.0, err / bound)
            if ratio.size:
                worst[k] = max(worst[k], float(np.nan_to_num(ratio, nan=np.inf).max()))
    return worst


def sgd_cases():
    """(p, g, lr, max_norm): every layout at the three clips, and one list whose norm is 1e-4, where the 1e-6 is a percent of it."""
    for li, layout in enumerate(C.LAYOUTS):
        p, g = C.sgd_case(C.LAYOUTS[layout]["numels"], 300 + li)
        _, _, norm, _ = C.sgd_clip_oracle(p, g, lr=0.5, max_norm=0.0)
        for factor in C.CLIPS.values():
            yield p, g, 0.5, factor * norm
    p, g = C.sgd_case(C.SIZES, 399, scale=1e-6)
    _, _, norm, _ = C.sgd_clip_oracle(p, g, lr=0.5, max_norm=0.0)
    assert 5e-5 < norm < 2e-4
    yield p, g, 0.5, 0.25 * norm


def test_the_sgd_emulations_stay_inside_the_bounds():
    worst = np.zeros(2)
    for p, g, lr, max_norm in sgd_cases():
        want = C.sgd_clip_oracle(p, g, lr=lr, max_norm=max_norm)
        n32 = norm32(g)
        assert abs(float(n32) - want[2]) <= C.NORM_RTOL * want[2]
        for fused in (False, True):
            got = C.sgd_emulate(p, g, n32, lr=lr, max_norm=max_norm, fused=fused)
            r = sgd_ratios(p, g, got, want, lr)
            assert max(r) <= 1.0, (max_norm, fused, r)
            if want[3] == 1.0:
                assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got[1], g))
            worst = np.maximum(worst, r)
    print(f"clip + SGD emulation: worst error / bound p {worst[0]:.3f}, g {worst[1]:.3f}")


@pytest.mark.parametrize("mutate", C.SGD_MUTATIONS)
def test_a_wrong_clip_breaks_the_bounds(mutate):
    broken = 0
    for p, g, lr, max_norm in sgd_cases():
        want = C.sgd_clip_oracle(p, g, lr=lr, max_norm=max_norm)
        got = C.sgd_emulate(p, g, norm32(g), lr=lr, max_norm=max_norm, fused=True, mutate=mutate)
        broken += not max(sgd_ratios(p, g, got, want, lr)) <= 1.0
    assert broken, f"{mutate} stays inside the bounds on every case"


def test_a_norm_that_is_not_finite_changes_nothing():
    """Finite gradients whose sum of squares passes the largest float, and a NaN: the oracle and the emulation keep every bit."""
    p, g = C.sgd_case(C.SIZES, 398)
    big = [a.copy() for a in g]
    big[3][:] = 3e19
    nan = [a.copy() for a in g]
    nan[7][-1] = np.nan
    for bad in (big, nan):
        wp, wg, norm, _ = C.sgd_clip_oracle(p, bad, lr=0.5, max_norm=0.25)
        assert not np.isfinite(norm) and not np.isfinite(norm32(bad))
        got = C.sgd_emulate(p, bad, norm32(bad), lr=0.5, max_norm=0.25, fused=False)
        for a, b, c, d, pi, gi in zip(got[0], got[1], wp, wg, p, bad):
            assert np.array_equal(a.view(np.uint32), pi.view(np.uint32)) and np.array_equal(b.view(np.uint32), gi.view(np.uint32))
            assert np.array_equal(c, pi.astype(np.float64)) and np.array_equal(d, gi.astype(np.float64), equal_nan=True)
