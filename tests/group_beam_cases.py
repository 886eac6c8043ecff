"""Diverse (group) beam search (Model.group_beam_search; C ABI vmlmf_beamgroup_step in libvmlmf_beamgroup.so,
include/vmlmf_beamgroup.h) stated in numpy and fp64, with the seeded cases that test_group_beam_cpu.py and test_gpu_group_beam.py share.
The step's own contract - totals, the order, lo / hi - is oracle/vmlmf_decode_oracle.py's: row_totals gives a batch row's raw totals,
and every group is judged by step_sets on its own beams' candidates under aug = total - lambda n at KERNEL_MARGIN.  The groups are
walked in order; n counts the reference's own survivors of the groups before (token v, live parent).  Test-side code: nothing here
imports the package."""
import functools

import numpy as np
import torch

import vmlmf_decode_oracle as C

EOS = C.EOS_KERNEL

# (B, W, G, H, V, lambda)
BASIC = (1, 4, 2, 16, 97, 0.5)            # the basic two-group step
ODD = (3, 6, 3, 16, 1000, 1.0)            # W not a power of two; a ticket per row
SINGLES = (2, 8, 8, 16, 300, 0.7)         # Wg = 1
WIDE = (1, 32, 2, 8, 64, 0.5)             # a merge of 1024 threads
BOUNDARY = (1, 32, 32, 8, 64, 0.5)        # the lemma's boundary: up to 31 penalised tokens among a beam's 32
LONG = (2, 4, 2, 8, 12293, 0.5)           # rows beyond BS_LDS_V, which re-read their scores
CLOSING = (1, 4, 2, 16, 97, 1e4)          # a penalty that closes every repeated token
KERNEL_CASES = [BASIC, ODD, SINGLES, WIDE, BOUNDARY, LONG, CLOSING]
# in these every group holds group 0's h rows and cum, as at the first step of a search: the penalty decides
SHARED = [BASIC, ODD, SINGLES, BOUNDARY, CLOSING]
# base: every beam live at a total of its own; finished: about a quarter of the beams finished, the last beam of group 0 among them;
# neginf: every slot of a group but its first at -inf - the first step of a search.  (Where Wg = 1 a group is one beam and the third
# variant has no beam at -inf: a whole group at -inf has nothing a margin could separate - all its totals are -inf and the flat index
# decides exactly -, which test_gpu_group_beam.py checks on its own.)
VARIANTS = ["base", "finished", "neginf"]
# chosen so that every group of every row of every variant is clear at C.KERNEL_MARGIN in the fp64 reference (test_group_beam_cpu.py
# asserts it) and, in the shared cases, the penalty changes the choice
SEEDS = {BASIC: 1, ODD: 1, SINGLES: 1, WIDE: 1, BOUNDARY: 1, LONG: 1, CLOSING: 1}


def case_id(case):
    return "x".join(str(v) for v in case)


@functools.lru_cache(maxsize=None)
def kernel_case(case, variant="base"):
    """The fp32 inputs of a kernel-level case: h (B W, H), w (V, H), bias (V), cum (B, W), finished (B, W) bool, length (B, W) int32 -
    CPU tensors drawn in this order from torch.Generator().manual_seed(SEEDS[case])."""
    B, W, G, H, V, _ = case
    Wg = W // G
    g = torch.Generator().manual_seed(SEEDS[case])
    h = torch.randn(B * W, H, generator=g)
    w = torch.randn(V, H, generator=g) * 0.1
    b = torch.randn(V, generator=g)
    cum = -3 * torch.rand(B, W, generator=g)
    fin = torch.rand(B, W, generator=g) < 0.25
    length = ((torch.arange(B * W) * 3) % 5 + 1).to(torch.int32).view(B, W)
    if variant == "finished":
        fin[:, Wg - 1] = True
    else:
        fin = torch.zeros((B, W), dtype=torch.bool)
    if variant == "neginf":
        dead = torch.ones(W, dtype=torch.bool)
        dead[::Wg] = False
        cum[:, dead] = float("-inf")
    if case in SHARED:
        h = h.view(B, G, Wg, H)[:, :1].expand(B, G, Wg, H).reshape(B * W, H).contiguous()
        cum = cum.view(B, G, Wg)[:, :1].expand(B, G, Wg).reshape(B, W).contiguous()
    return h, w, b, cum, fin, length


def group_step(x, cum, finished, eos, W, G, lam, margin, forced=None):
    """One batch row in fp64.  x (W, V) scores with the bias, cum (W), finished (W) bool.  Returns (totals (W, V) - the RAW totals -,
    groups): per group g (aug (W, V), valid (W, V) - the group's own beams' candidates -, top, lo, hi) of step_sets(aug, valid, Wg),
    flat indices w V + v over the whole row.  The counts the next group is penalised with are those of `top` - or, teacher-forced,
    those of forced[g], the flat indices a step under test chose for group g."""
    totals, valid = C.row_totals(x, cum, finished, eos)
    Wn, V = totals.shape
    assert Wn == W and W % G == 0
    Wg = W // G
    fin = np.asarray(finished, dtype=bool) & (eos is not None)
    counts = np.zeros(V)
    groups = []
    for g in range(G):
        mine = slice(g * Wg, (g + 1) * Wg)
        vg = np.zeros_like(valid)
        vg[mine] = valid[mine]
        aug = totals.copy()
        for w in range(g * Wg, (g + 1) * Wg):
            if not fin[w]:                                  # a finished beam's candidate is not penalised
                aug[w] = totals[w] - lam * counts
        top, lo, hi = C.step_sets(aug, vg, Wg, margin)
        groups.append((aug, vg, top, lo, hi))
        for f in (top if forced is None else forced[g]):
            par, tok = divmod(int(f), V)
            if not fin[par]:                                # a finished beam's padding eos is not a choice
                counts[tok] += 1
    return totals, groups


def scores64(case, variant="base"):
    B, W, G, H, V, _ = case
    h, w, b = kernel_case(case, variant)[:3]
    return (h.double() @ w.double().t() + b.double()).view(B, W, V).numpy()


@functools.lru_cache(maxsize=None)
def kernel_oracle(case, variant="base", lam=None):
    """Per batch row (totals, groups) of group_step for a kernel-level case at C.KERNEL_MARGIN (lam: another penalty than the case's)."""
    B, W, G, H, V, lam0 = case
    _, _, _, cum, fin, _ = kernel_case(case, variant)
    x = scores64(case, variant)
    return [group_step(x[r], cum[r].double().numpy(), fin[r].numpy(), EOS, W, G, lam0 if lam is None else lam, C.KERNEL_MARGIN)
            for r in range(B)]


def in_order(aug, top, margin):
    """Whether the order of a group's survivors is beyond fp32's reach too: consecutive aug more than the margin apart."""
    a = aug.ravel()[top]
    return bool((a[:-1] - a[1:] > margin).all())


def chosen(rows):
    """The reference's survivors of kernel_oracle's rows as flat indices, (B, W), group-major in order."""
    return np.array([[int(f) for (_, _, top, _, _) in groups for f in top] for _, groups in rows])


# ---- model level ----
MODEL_CASES = [("plain", 2, 4, 2, 0.5, 13), ("group", 2, 6, 3, 1.0, 11)]       # kind, B, W, G, lambda, prompt seed
MODEL_STEPS, MODEL_EOS = 8, C.MODEL_EOS
