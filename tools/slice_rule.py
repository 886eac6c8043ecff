"""The slice-wise gradient rule (docs/design/slice_tolerances.md): for every slice s of a gradient, max|a_s - b_s| <= rel * max|b_s|, with no
absolute floor, and the map from a tensor's name to its slices - time steps and rows of dx, rows of dh0 / dc0, the gate blocks of every
stacked-gate parameter, the groups and gate blocks of the grouped factors.  numpy only.  It lives beside tools/fuzz_parity.py, which applies
it to its draws, so that the sweep needs nothing of the test helpers but what they have always had; the tests reach it through
tests/hip_util.py (assert_grad_slices, compare_slices, compare_all(..., slices=))."""
import numpy as np

import vmlmf_oracle as O

GREL = 1e-4                 # the suite's gradient tolerance (tests/hip_util.py), here of each slice's own maximum
TINY = 2.0 ** -100          # a slice whose reference stays below this is skipped: flush-to-zero of denormal products is no error


def _slice_maxima(err, ref, cut):
    """(labels, max err, max |ref|) of every slice of one cut.  A cut is an int or a tuple of ints - the axes to cut along, one slice per
    index along them - or a list of (label, index) blocks, index being what numpy takes between brackets."""
    if isinstance(cut, (int, tuple)):
        axes = (cut,) if isinstance(cut, int) else tuple(cut)
        rest = tuple(ax for ax in range(err.ndim) if ax not in axes)
        e, r = err.max(axis=rest), ref.max(axis=rest)
        labels = ["axes %s index %s" % (axes, idx) for idx in np.ndindex(e.shape)]
        return labels, e.reshape(-1), r.reshape(-1)
    return [lab for lab, _ in cut], np.array([err[idx].max() for _, idx in cut]), np.array([ref[idx].max() for _, idx in cut])


def slice_report(a, b, slices, rel=GREL):
    """(label of the worst slice, its max error as a share of rel * its own max |ref|, slices skipped as below TINY) over every cut."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err, ref = np.abs(a - b), np.abs(b)
    err = np.where(np.isfinite(err), err, np.inf)
    worst, skipped = ("none", 0.0), 0
    for cut in slices:
        labels, e, r = _slice_maxima(err, ref, cut)
        live = r >= TINY
        skipped += int((~live).sum())
        if live.any():
            share = np.where(live, e / np.where(live, rel * r, 1.0), -1.0)
            i = int(share.argmax())
            if share[i] >= worst[1]:
                worst = (labels[i], float(share[i]))
    return worst[0], worst[1], skipped


def assert_grad_slices(a, b, what, slices, rel=GREL):
    """The gradient rule slice by slice: for every slice s of every cut in slices, max|a_s - b_s| <= rel * max|b_s|, with no absolute
    floor.  Slices whose reference lies below TINY are skipped; their number is returned."""
    assert np.shape(a) == np.shape(b), (what, np.shape(a), np.shape(b))
    assert np.all(np.isfinite(a)), what + ": non-finite values"
    label, share, skipped = slice_report(a, b, slices, rel)
    assert share <= 1.0, f"{what}: worst slice {label} uses {share:.3g} x its tolerance ({rel:g} of the slice's own max |ref|)"
    return skipped


def _gate_blocks(shape, axis, n=4):
    w = shape[axis] // n
    pre = (slice(None),) * axis
    return [("gate block %d (axis %d, %d:%d)" % (k, axis, k * w, (k + 1) * w), pre + (slice(k * w, (k + 1) * w),)) for k in range(n)]


def slice_cuts(name, shape, variant, H, g=1, time_major=False):
    """The cuts of one gradient tensor, or None where the whole-tensor rule stays (dia_*, u_x, u_h, w, u, V5's per-gate tensors).  The
    boundaries are those of oracle/vmlmf_oracle.py::literal_step: the stacked axis of length 4H is split by chunk(4, 1) and by
    _strip_diag's range(0, 4H, H) into four blocks of H; V2 / V6 chunk the grouped product (B, g, 4H/g) along its last axis into four
    blocks of H/g; V4 flattens it to (B, 4H) before chunk(4, 1), so gate k owns the flat columns kH:(k+1)H of (group, column)."""
    if name == "dx":
        return [0, 1]                                   # per time step and per row, whichever of the two leading axes is which
    if name in ("dh0", "dc0"):
        return [0]
    if variant == O.V5:
        return None
    if name in ("v_x", "v_h", "w_x", "w_h", "b_x", "b_h", "bias_x", "bias_h"):
        axis = [ax for ax, n in enumerate(shape) if n == 4 * H]
        assert len(axis) == 1, (name, shape, H)
        return [_gate_blocks(shape, axis[0])]
    if name[:4] in ("u_h_", "v_h_", "u_h.", "v_h.") and len(shape) == 3:
        Hg = H // g
        assert shape[0] == g, (name, shape, g)
        cuts = [0]
        if shape[2] == 4 * Hg:
            blocks = []
            for q in range(g):
                if variant == O.V4:
                    for k in range(4):
                        lo, hi = max(0, k * H - q * 4 * Hg), min(4 * Hg, (k + 1) * H - q * 4 * Hg)
                        if lo < hi:
                            blocks.append(("group %d gate block %d (columns %d:%d)" % (q, k, lo, hi), (q, slice(None), slice(lo, hi))))
                else:
                    blocks += [("group %d %s" % (q, lab), (q,) + idx[1:]) for lab, idx in _gate_blocks(shape, 2)]
            cuts.append(blocks)
        return cuts
    return None


def _grad_items(res):
    """(name, parameter name or None, layer, array) of every gradient of a layer's or a stack's result."""
    for k in ("dx", "dh0", "dc0"):
        v = res.get(k)
        if isinstance(v, list):
            for l, a in enumerate(v):
                yield f"{k}[{l}]", k, l, a
        elif v is not None:
            yield k, k, None, v
    G = res.get("G")
    if isinstance(G, dict):
        for k, a in G.items():
            yield "G." + k, k, None, a
    elif G is not None:
        for l, Gl in enumerate(G):
            for k, a in Gl.items():
                yield f"G[{l}].{k}", k, l, a


def compare_slices(got, ref, tag, slices, rel=GREL):
    """assert_grad_slices on every gradient of a layer's or a stack's result that got holds, by the cuts of slice_cuts.  slices: the
    layout, a dict of variant, H (a list for a stack whose layers differ), g and time_major.  Returns {"skipped": slices below TINY,
    "worst": (quantity and slice, share of the slice tolerance)}."""
    have = {name: a for name, _, _, a in _grad_items(got)}
    problems, skipped, worst = [], 0, ("none", 0.0)
    for name, key, layer, b in _grad_items(ref):
        if name not in have:
            continue
        H = slices["H"][layer or 0] if isinstance(slices["H"], (list, tuple)) else slices["H"]       # (a stack's dx has no layer: no H either)
        cuts = slice_cuts(key, np.shape(b), slices["variant"], H, slices.get("g", 1), slices.get("time_major", False))
        if cuts is None:
            continue
        label, share, skip = slice_report(have[name], b, cuts, rel)
        skipped += skip
        if share >= worst[1]:
            worst = (f"{name} {label}", share)
        try:
            assert_grad_slices(have[name], b, f"{tag}.{name}", cuts, rel)
        except AssertionError as e:
            problems.append(str(e))
    assert not problems, "\n".join(problems)
    return {"skipped": skipped, "worst": worst}
