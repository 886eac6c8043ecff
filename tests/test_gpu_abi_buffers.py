"""The C ABI (include/vmlmf_hip.h and the three side libraries) on poisoned, exactly sized buffers with guard bands, straight
through ctypes (tests/abi_arena.py; the design and the audit behind the table: docs/design/buffer_contract.md).

Every parity test of the suite takes its buffers from torch.empty: fresh device memory is zero, allocations are rounded up, and an
output nobody writes keeps a plausible previous occupant.  Here every buffer of a call - inputs, outputs, reserve, workspaces,
scratch - is a view of ONE allocation filled with a 32-bit pattern, exactly sized, between guard bands.  The header says which
words a caller must zero (the CE ticket, the sampler and beam tickets, the Adam guard block); everything else may hold anything.
No float atomics exist in the library and the summation orders are fixed, so the demand is exact.  Per case, the call sequence
(forward, then backward with a SECOND, freshly poisoned workspace, as the header allows) runs once per fill - 0x00000000 (the
de-facto condition), 0x7FC07FC0 (NaN as fp32 and in both bf16 halves, a huge counter), 0xFFFFFFFF (negative NaN, -1) - and

  a. every call returns 0 and vmlmf_check_status() is clean after the synchronisation,
  b. no guard byte of any buffer changed,
  c. no output element still holds the pattern (asked under the two non-zero fills: a written zero is the zero pattern) and every
     floating output is finite,
  d. every output has the same bits under the three fills,
  e. every word the header says a launch leaves zero is zero,
  f. layer and stack cases: the zero-fill run matches the fp64 oracle at hip_util's tolerances (bf16 cases: tests/test_gpu_bf16.py
     owns that bound), so a mis-wired case cannot pass by being consistently wrong,

and each layer and stack case asserts that the kernel family it is meant for ran (vmlmf_query's geometry, vmlmf_stack_query's return,
tune_get - "wring_launches" counts wgrad_ring_kernel itself -, the per-kernel launch counts of vmlmf_profile_*).  The flat kernels
other than the classifier head and the criterion, and the side libraries, have no slot in vmlmf_profile_*: their rows are tied to
their entry point by name and checked against a reference of the same operation.  No output element is excluded from (c) or (d): the header declares none
unspecified.

Out of scope: vmlmf_comm_* and vmlmf_p2p_* (they need several processes), and the A/B forms chosen by environment variables at
load time (a process each; test_measurement_switches_compute_the_same_thing keeps their parity).  A score row without a target is
not in the table either: its rank is -1 by contract, which is the 0xFFFFFFFF pattern.  A two-group layer of padded hidden rank 24
has no row-block instantiation (the library keeps it on the register-resident kernels): the V2 rows of that family use ranks 16 and 32.
"""
import ctypes

import numpy as np
import pytest
import torch

import vmlmf_oracle as O
from abi_arena import ALIGN, FILL_ZERO, FILLS, GUARD, Arena, assert_same_bits, assert_untouched, assert_written, assert_zero
from hip_util import ORDER, assert_grad, assert_out

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, I64, I32, U8 = torch.float32, torch.int64, torch.int32, torch.uint8
GROUPED = (O.V2, O.V4, O.V6)


# ---- plumbing ---------------------------------------------------------------------------------------------------------------
class Plan:
    """The buffers of one call, asked for before the arena exists (its size is their sum): add() records, alloc() carves."""

    def __init__(self):
        self.items, self.out, self.zero = [], [], []

    def add(self, name, shape, dtype=F32, init=None, out=False, zero_after=False):
        self.items.append((name, shape, dtype, init))
        if out:
            self.out.append(name)
        if zero_after:
            self.zero.append(name)
        return name

    def alloc(self, fill):
        need = GUARD + 2 * ALIGN
        for _, shape, dtype, _ in self.items:
            n = int(np.prod(shape, dtype=np.int64)) if not isinstance(shape, (int, np.integer)) else int(shape)
            need += n * torch.empty((), dtype=dtype).element_size() + GUARD + 2 * ALIGN
        arena = Arena(DEV, fill, capacity=need)
        return arena, {name: arena.buf(shape, dtype, init=init, name=name) for name, shape, dtype, init in self.items}


def _lib():
    from vmlmf_amd import _lib as L
    return L


def stream():
    return _lib().raw_stream(device())


def device():
    return torch.device("cuda", torch.cuda.current_device())


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def ok(rc, what=""):
    assert rc == 0, f"{what}: rc {rc}: {_lib().lib().vmlmf_last_error().decode()}"


class counted:
    """Launch counts of the library's internal kernels inside the block (vmlmf_profile_*), by kernel name, in .counts."""

    def __enter__(self):
        L = _lib()
        L.lib().vmlmf_profile_read(None, None, 1)
        L.lib().vmlmf_profile_enable((1 << L.NKERNELS) - 1)
        self.counts = {}
        return self

    def __exit__(self, *exc):
        L = _lib()
        try:
            if exc[0] is None:
                torch.cuda.synchronize()
                cnt = (ctypes.c_int32 * L.NKERNELS)()
                L.lib().vmlmf_profile_read(None, cnt, 1)
                self.counts.update({L.lib().vmlmf_kernel_name(k).decode(): cnt[k] for k in range(L.NKERNELS)})
        finally:
            L.lib().vmlmf_profile_enable(0)
        return False


class tuned:
    """vmlmf_tune switches for the block; every one restored, and the gradient-health word cleared, on the way out."""

    def __init__(self, switches):
        self.switches = dict(switches)

    def __enter__(self):
        L = _lib()
        self.before = {k: L.tune_get(k) for k in self.switches}
        for k, v in self.switches.items():
            L.tune(k, v)
            assert L.tune_get(k) == v, (k, v, L.tune_get(k))
        return self

    def __exit__(self, *exc):
        L = _lib()
        try:
            torch.cuda.synchronize()
        finally:
            for k, v in self.before.items():
                L.tune(k, v)
            L.tune("clear_health", 0)
        return False


def settle(arena, bufs, plan):
    """(a) the status word, (b) the guards, (c) the outputs, (e) the zero words of one finished call; the outputs, cloned."""
    torch.cuda.synchronize()
    _lib().check_status()
    arena.check_guards()
    for name in plan.out:
        assert_written(arena, name, bufs[name])
    for name in plan.zero:
        assert_zero(name, bufs[name])
    return {name: bufs[name].clone() for name in plan.out}


def same_under_every_fill(runs):
    """(d): every output of the fills' runs against the zero fill's, bit for bit."""
    for fill, run in zip(FILLS[1:], runs[1:]):
        assert run.keys() == runs[0].keys()
        for name in runs[0]:
            assert_same_bits(name, runs[0][name], run[name], f"between the fills 0x{FILL_ZERO:08x} and 0x{fill:08x}")


def expect_counts(counts, want, tag):
    for name, n in want.items():
        assert counts[name] == n, f"{tag}: {name} launched {counts[name]} times, the case is meant for {n}: {counts}"


def params_struct(variant, tensors):
    from vmlmf_amd.functional import _params_struct
    return _params_struct(tensors, 2 if variant in GROUPED else 1, variant)


def rng_for(name):
    return np.random.Generator(np.random.PCG64(sum(map(ord, name))))


def lib_factors(desc, R, H, prob, state, site):
    """The dropout factors the library applies for (state, site), (R, H), as layer `desc`'s kernels map the columns."""
    L = _lib()
    out = torch.empty((R, H), device=DEV, dtype=F32)
    st = state.clone()
    ok(L.lib().vmlmf_dropout_factors(None if desc is None else ctypes.byref(desc), R, H, float(prob), p(st), int(site), p(out), stream()),
       "dropout_factors")
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64)


# ---- one layer: vmlmf_seq_forward_ex / vmlmf_seq_backward_ex ------------------------------------------------------------------
def lc(id, variant, B, T, I, H, rw, ru, tm=False, st=True, dst=True, dx=True, dtype="f32", tune=None, head=False, ce=False,
       drop=False, packed=False, geo=None, fwd=None, bwd=None, scale=0.1, ring=0):
    return dict(id=id, variant=variant, B=B, T=T, I=I, H=H, rw=rw, ru=ru, tm=tm, st=st, dst=dst, dx=dx, dtype=dtype, tune=tune or {},
                head=head, ce=ce, drop=drop, packed=packed, geo=geo or {}, fwd=fwd or {}, bwd=bwd or {}, scale=scale, ring=ring)


RIDE = dict(B=21, T=13, I=9, H=65, rw=16, ru=[16])     # the fewest rows (T B = 273) at which four weight-gradient workers ride
SMALL = dict(B=5, T=3, I=9, H=65)                      # eleven dead rows of a block, a wave with one unit, I % 4 != 0, odd T
BIG = dict(I=650, H=650, T=3, tm=True, scale=0.03)     # beyond one CU: clusters of workgroups, or the step-wise family
VALU1 = dict(rows_per_wg=1)

LAYER_CASES = [
    # register-resident one-row kernels: every variant, padded hidden ranks 8 / 16 / 24 / 32 from ranks off the padding grid
    lc("valu-v1-kh8", O.V1, rw=5, ru=[5], **SMALL, geo=dict(rows_per_wg=1, kh=8, kx=8), fwd=dict(rec_fwd_kernel=1, xproj_kernel=0)),
    lc("valu-v3-kh16-tm", O.V3, B=5, T=3, I=65, H=65, rw=11, ru=[11], tm=True, geo=dict(rows_per_wg=1, kh=16, kx=16),
       fwd=dict(xproj_kernel=1, rec_fwd_kernel=1), bwd=dict(rec_bwd_kernel=1, dqx_dx_kernel=1, wgrad_mfma_kernel=1)),
    lc("valu-v2-kh24", O.V2, B=5, T=3, I=9, H=130, rw=5, ru=[5, 11], geo=dict(rows_per_wg=1, kh=24), fwd=dict(rec_fwd_kernel=1)),
    lc("valu-v5-kh32", O.V5, B=5, T=3, I=9, H=65, rw=9, ru=[27], geo=dict(rows_per_wg=1, kh=32, kx=16), fwd=dict(rec_fwd_kernel=1)),
    lc("valu-v6-kh16-nostates", O.V6, B=21, T=3, I=9, H=130, rw=5, ru=[5, 5], st=False, dst=False, geo=dict(rows_per_wg=1, kh=16)),
    lc("valu-v1-kh24-nodx", O.V1, rw=11, ru=[20], dx=False, **SMALL, geo=dict(rows_per_wg=1, kh=24, kx=16), bwd=dict(dqx_dx_kernel=0)),
    # old and new forward / backward recurrences (layers of the x-projection wave with the x-fold)
    lc("valu-rec3=0", O.V1, rw=11, ru=[11], tune=dict(rec3=0), **SMALL, geo=VALU1, fwd=dict(xproj_kernel=0, rec_fwd_kernel=1)),
    lc("valu-rec3=6", O.V1, rw=11, ru=[11], tune=dict(rec3=6), **SMALL, geo=VALU1, fwd=dict(xproj_kernel=0, rec_fwd_kernel=1)),
    lc("valu-rec3=7", O.V1, rw=11, ru=[11], tune=dict(rec3=7), **SMALL, geo=VALU1, fwd=dict(xproj_kernel=0, rec_fwd_kernel=1)),
    # register images built in the kernels' prologues, or by pack_kernel
    lc("valu-direct=1", O.V1, rw=16, ru=[16], tune=dict(direct=1), **SMALL, geo=VALU1, fwd=dict(pack_kernel=0), bwd=dict(pack_kernel=1)),
    lc("valu-direct=0", O.V1, rw=16, ru=[16], tune=dict(direct=0), **SMALL, geo=VALU1, fwd=dict(pack_kernel=1), bwd=dict(pack_kernel=0)),
    # weight-gradient workers riding on the backward launch, and the launches that finish behind them
    lc("valu-wride=1-finish2=1", O.V1, **RIDE, dx=False, tune=dict(wride=1, finish2=1), geo=VALU1,
       fwd=dict(pack_kernel=0), bwd=dict(pack_kernel=0, wgrad_mfma_kernel=0, finish2_kernel=1, reduce_cg_kernel=0, finish_kernel=0)),
    lc("valu-wride=1-finish2=0", O.V1, **RIDE, tune=dict(wride=1, finish2=0), geo=VALU1,
       bwd=dict(wgrad_mfma_kernel=0, finish2_kernel=0, reduce_cg_kernel=1, finish_kernel=1, dqx_dx_kernel=1)),
    lc("valu-wride=0", O.V1, **RIDE, tune=dict(wride=0), geo=VALU1,
       bwd=dict(wgrad_mfma_kernel=1, finish2_kernel=0, reduce_cg_kernel=1, finish_kernel=1)),
    lc("valu-wride=1-v3-tm-nostates", O.V3, B=21, T=13, I=16, H=16, rw=16, ru=[16], tm=True, st=False, dx=False, tune=dict(wride=1),
       geo=VALU1, bwd=dict(wgrad_mfma_kernel=0, finish2_kernel=1)),
    # weight gradients formed in the rows' workgroups (x-fold layer, dx NULL)
    lc("valu-inrow=1", O.V1, rw=16, ru=[16], dx=False, tune=dict(inrow=1), **SMALL, geo=VALU1,
       bwd=dict(rec_bwd_kernel=1, wgrad_mfma_kernel=0, dqx_dx_kernel=0, reduce_cg_kernel=1, finish_kernel=1)),
    # kept parameter images: the packed buffer poisoned before vmlmf_pack_params
    lc("valu-packed", O.V1, rw=11, ru=[11], packed=True, **SMALL, geo=VALU1, fwd=dict(pack_kernel=0), bwd=dict(pack_kernel=0)),
    lc("rb-packed", O.V1, rw=5, ru=[5], packed=True, tune=dict(rb=1), B=21, T=3, I=9, H=65, geo=dict(threads_per_wg=256),
       fwd=dict(pack_kernel=0), bwd=dict(pack_kernel=0)),
    # classifier and criterion riding on the launch
    lc("valu-head-ce", O.V1, rw=16, ru=[16], head=True, ce=True, **SMALL, geo=VALU1,
       fwd=dict(head_fwd_kernel=0, ce_fwd_kernel=0), bwd=dict(head_bwd_kernel=0)),
    lc("valu-head-ce-ride", O.V1, **RIDE, dx=False, head=True, ce=True, tune=dict(wride=1, finish2=1), geo=VALU1,
       fwd=dict(head_fwd_kernel=0, ce_fwd_kernel=0), bwd=dict(head_bwd_kernel=0, finish2_kernel=1)),
    # row-block kernels within one CU
    lc("rb-v1-rows4", O.V1, B=21, T=3, I=9, H=65, rw=5, ru=[5], tune=dict(rb=1, rb_rows=4), geo=dict(rows_per_wg=4, threads_per_wg=256, workgroups=6)),
    lc("rb-v1-rows8", O.V1, B=21, T=3, I=9, H=65, rw=5, ru=[5], tune=dict(rb=1, rb_rows=8), geo=dict(rows_per_wg=8, threads_per_wg=256, workgroups=3)),
    lc("rb-v2-kh16-nostates", O.V2, B=21, T=3, I=9, H=130, rw=5, ru=[5, 5], st=False, dst=False, tune=dict(rb=1),
       geo=dict(threads_per_wg=256, kh=16), bwd=dict(dqx_dx_kernel=1, wgrad_mfma_kernel=1)),
    lc("rb-v2-kh32-rows8", O.V2, B=21, T=3, I=9, H=130, rw=5, ru=[11, 11], tune=dict(rb=1, rb_rows=8),
       geo=dict(rows_per_wg=8, threads_per_wg=256, workgroups=3, kh=32)),
    lc("rb-v1-rows16-tm", O.V1, B=21, T=3, I=9, H=65, rw=11, ru=[11], tm=True, tune=dict(rb=1, rb_rows=16),
       geo=dict(rows_per_wg=16, threads_per_wg=256, workgroups=2)),
    lc("rb-v1-B5-nostates", O.V1, rw=5, ru=[5], st=False, dst=False, tune=dict(rb=1), **SMALL, geo=dict(threads_per_wg=256)),
    lc("rb-bf16-v1", O.V1, B=21, T=3, I=9, H=65, rw=5, ru=[5], dtype="bf16", geo=dict(threads_per_wg=256)),
    lc("rb-bf16-v3-tm", O.V3, B=5, T=3, I=65, H=65, rw=11, ru=[11], tm=True, dtype="bf16", geo=dict(threads_per_wg=256)),
    lc("rb-bf16-v5", O.V5, B=21, T=3, I=9, H=65, rw=9, ru=[11], dtype="bf16", geo=dict(threads_per_wg=256)),
    lc("rb-head-ce", O.V1, B=21, T=3, I=9, H=65, rw=5, ru=[5], head=True, ce=True, dst=False, tune=dict(rb=1), geo=dict(threads_per_wg=256),
       fwd=dict(head_fwd_kernel=1, ce_fwd_kernel=1), bwd=dict(head_bwd_kernel=1)),
    lc("rb-dropout-fused", O.V3, B=21, T=3, I=65, H=65, rw=11, ru=[11], tm=True, drop=True, tune=dict(rb=1), geo=dict(threads_per_wg=256)),
    # clustered row-block layers
    lc("cluster-v3-B5", O.V3, B=5, rw=32, ru=[32], **BIG, geo=dict(threads_per_wg=256), bwd=dict(wgrad_mfma_kernel=1)),
    lc("cluster-v4-B21-S4", O.V4, B=21, rw=32, ru=[32, 32], **BIG, tune=dict(rb_cluster=4, rb_rows=16), geo=dict(threads_per_wg=256, workgroups=8)),
    lc("cluster-v3-B21-wring=1", O.V3, B=21, rw=32, ru=[32], **BIG, tune=dict(wring=1), ring=1, geo=dict(threads_per_wg=256), bwd=dict(wgrad_mfma_kernel=1)),
    lc("cluster-v4-B5-wring=0-nostates", O.V4, B=5, rw=32, ru=[32, 32], st=False, dst=False, **BIG, tune=dict(wring=0), geo=dict(threads_per_wg=256)),
    lc("cluster-v3-head-ce", O.V3, B=5, rw=32, ru=[32], head=True, ce=True, dst=False, **BIG, geo=dict(threads_per_wg=256),
       fwd=dict(head_fwd_kernel=1, ce_fwd_kernel=1), bwd=dict(head_bwd_kernel=1)),
    # the step-wise family
    lc("step-v3-B5", O.V3, B=5, rw=32, ru=[32], **BIG, tune=dict(rb=0), geo=dict(rows_per_wg=1, workgroups=5), fwd=dict(xproj_kernel=1)),
    lc("step-v4-B21-wring=1", O.V4, B=21, rw=32, ru=[32, 32], **BIG, tune=dict(rb=0, wring=1), ring=1, geo=dict(rows_per_wg=1, workgroups=21)),
    lc("step-v5-I>H", O.V5, B=5, T=3, I=80, H=65, rw=9, ru=[11], tune=dict(rb=0), geo=dict(rows_per_wg=1), fwd=dict(xproj_kernel=1)),
    lc("step-wide-v3-tm", O.V3, B=5, T=3, I=96, H=96, rw=40, ru=[40], tm=True, geo=dict(rows_per_wg=1, kx=40, kh=40), fwd=dict(xproj_kernel=1)),
    lc("step-wide-v3-batch-first", O.V3, B=5, T=3, I=96, H=96, rw=40, ru=[40], tm=False, geo=dict(rows_per_wg=1, kx=40, kh=40),
       fwd=dict(xproj_kernel=1)),
    lc("step-head-ce", O.V3, B=5, rw=32, ru=[32], head=True, ce=True, dst=False, **BIG, tune=dict(rb=0), geo=dict(rows_per_wg=1),
       fwd=dict(head_fwd_kernel=1, ce_fwd_kernel=1), bwd=dict(head_bwd_kernel=1)),
]
CLASSES, DROP_P = 18, 0.3


def layer_inputs(c):
    """numpy inputs of a layer case (the same for every fill)."""
    rng = rng_for(c["id"])
    B, T, I, H = c["B"], c["T"], c["I"], c["H"]
    P = O.make_params(c["variant"], I, H, c["rw"], c["ru"] if c["variant"] in GROUPED else c["ru"][0], seed=2, scale=c["scale"])
    sh = (T, B) if c["tm"] else (B, T)
    d = dict(P=P, x=(0.5 * rng.standard_normal(sh + (I,))).astype(np.float32), dy=rng.standard_normal(sh + (H,)).astype(np.float32))
    d["h0"] = (0.4 * rng.standard_normal((B, H))).astype(np.float32) if c["st"] else None
    d["c0"] = (0.4 * rng.standard_normal((B, H))).astype(np.float32) if c["st"] else None
    d["dhT"] = rng.standard_normal((B, H)).astype(np.float32) if c["dst"] else None
    d["dcT"] = rng.standard_normal((B, H)).astype(np.float32) if c["dst"] else None
    if c["head"]:
        d["hw"] = (0.1 * rng.standard_normal((CLASSES, H))).astype(np.float32)
        d["hb"] = (0.1 * rng.standard_normal(CLASSES)).astype(np.float32)
        d["dlogits"] = rng.standard_normal((B, CLASSES)).astype(np.float32)
        d["target"] = rng.integers(0, CLASSES, B).astype(np.int64)
        d["target"][1] = -100       # an ignored row
    return d


def run_layer(c, d, fill):
    """Forward, then backward with a second workspace, of one layer case under one fill.  Returns (outputs, sizes, launch counts of
    the forward, of the backward, the descriptor)."""
    L = _lib()
    lib = L.lib()
    variant, B, T, I, H = c["variant"], c["B"], c["T"], c["I"], c["H"]
    desc = L.make_desc(variant, B, T, I, H, c["rw"], c["ru"], g=2 if variant in GROUPED else 1, time_major=c["tm"], training=True, dtype=c["dtype"])
    sz = L.query(desc)
    sh = (T, B) if c["tm"] else (B, T)
    names = ORDER[variant]
    pl = Plan()
    for k in names:
        pl.add("p." + k, d["P"][k].shape, init=d["P"][k])
        pl.add("g." + k, d["P"][k].shape, out=True)
    pl.add("x", sh + (I,), init=d["x"])
    pl.add("dy", sh + (H,), init=d["dy"])
    for k in ("h0", "c0", "dhT", "dcT"):
        if d[k] is not None:
            pl.add(k, (B, H), init=d[k])
    for k in ("y",):
        pl.add(k, sh + (H,), out=True)
    pl.add("hT", (B, H), out=True), pl.add("cT", (B, H), out=True)
    if c["dx"]:
        pl.add("dx", sh + (I,), out=True)
    if c["st"]:
        pl.add("dh0", (B, H), out=True), pl.add("dc0", (B, H), out=True)
    pl.add("reserve", sz.reserve_bytes, U8)
    pl.add("ws.forward", sz.workspace_bytes, U8)
    pl.add("ws.backward", sz.workspace_bytes, U8)
    if c["head"]:
        pl.add("head.weight", (CLASSES, H), init=d["hw"]), pl.add("head.bias", CLASSES, init=d["hb"])
        pl.add("head.dlogits", (B, CLASSES), init=d["dlogits"])
        pl.add("logits", (B, CLASSES), out=True), pl.add("dweight", (CLASSES, H), out=True), pl.add("dbias", CLASSES, out=True)
    if c["ce"]:
        pl.add("ce.target", B, I64, init=d["target"])
        pl.add("loss", 1, out=True), pl.add("nvalid", 1, out=True), pl.add("lse", B, out=True)
        pl.add("dlogits_unit", (B, CLASSES), out=True)
        pl.add("ce.ticket", 2, I64, init=0, zero_after=True)
    if c["drop"]:
        pl.add("drop.state", 2, I64, init=np.array([1234567, 3], np.int64))
        pl.add("y_dropped", sh + (H,), out=True)
    nbytes = ctypes.c_size_t(0)
    if c["packed"]:
        ok(lib.vmlmf_pack_bytes(ctypes.byref(desc), ctypes.byref(nbytes)), "pack_bytes")
        pl.add("packed", nbytes.value, U8)
    arena, b = pl.alloc(fill)
    ps = params_struct(variant, [b["p." + k] for k in names])
    gs = params_struct(variant, [b["g." + k] for k in names])
    s = stream()
    if c["packed"]:
        ok(lib.vmlmf_pack_params(ctypes.byref(desc), ctypes.byref(ps), p(b["packed"]), s), "pack_params")
    hd = L.Head()
    if c["head"]:
        hd.classes, hd.weight, hd.bias, hd.logits = CLASSES, b["head.weight"].data_ptr(), b["head.bias"].data_ptr(), b["logits"].data_ptr()
        hd.dlogits, hd.dweight, hd.dbias = b["head.dlogits"].data_ptr(), b["dweight"].data_ptr(), b["dbias"].data_ptr()
    ce = L.Ce()
    if c["ce"]:
        ce.target, ce.ignore_index, ce.loss, ce.nvalid = b["ce.target"].data_ptr(), -100, b["loss"].data_ptr(), b["nvalid"].data_ptr()
        ce.lse, ce.dlogits_unit, ce.ticket = b["lse"].data_ptr(), b["dlogits_unit"].data_ptr(), b["ce.ticket"].data_ptr()
    dr = L.Dropout()
    if c["drop"]:
        assert lib.vmlmf_dropout_fused(ctypes.byref(desc)) == 1
        dr.p, dr.site, dr.state, dr.y_dropped = DROP_P, 1, b["drop.state"].data_ptr(), b["y_dropped"].data_ptr()
    ex = L.Extra()
    ex.packed = b["packed"].data_ptr() if c["packed"] else None
    ex.head = ctypes.pointer(hd) if c["head"] else None
    ex.ce = ctypes.pointer(ce) if c["ce"] else None
    ex.drop = ctypes.pointer(dr) if c["drop"] else None
    fargs = (ctypes.byref(desc), ctypes.byref(ps), p(b["x"]), p(b.get("h0")), p(b.get("c0")), p(b["y"]), p(b["hT"]), p(b["cT"]), p(b["reserve"]),
             p(b["ws.forward"]), sz.workspace_bytes, s)
    with counted() as fwd:
        if c["packed"]:      # the kept-image entry points themselves
            ok(lib.vmlmf_seq_forward_packed(*fargs, p(b["packed"])), "forward_packed")
        else:
            ok(lib.vmlmf_seq_forward_ex(*fargs, ctypes.byref(ex)), "forward")
    ex.ce = None
    bargs = (ctypes.byref(desc), ctypes.byref(ps), p(b["x"]), p(b.get("h0")), p(b.get("c0")), p(b["y"]), p(b["reserve"]), p(b["dy"]), p(b.get("dhT")),
             p(b.get("dcT")), p(b.get("dx")), p(b.get("dh0")), p(b.get("dc0")), ctypes.byref(gs), p(b["ws.backward"]), sz.workspace_bytes, s)
    with counted() as bwd:
        if c["packed"]:
            ok(lib.vmlmf_seq_backward_packed(*bargs, p(b["packed"])), "backward_packed")
        else:
            ok(lib.vmlmf_seq_backward_ex(*bargs, ctypes.byref(ex)), "backward")
    return settle(arena, b, pl), sz, fwd.counts, bwd.counts, desc


def layer_oracle(c, d, got, desc):
    """(f): the zero-fill run against run_literal in fp64 (hip_util's tolerances)."""
    from hip_util import run_literal
    tag = c["id"]
    g = {k: v.cpu().numpy() for k, v in got.items()}
    dy = d["dy"].astype(np.float64)
    if c["drop"]:
        f = lib_factors(desc, c["T"] * c["B"], c["H"], DROP_P, torch.tensor([1234567, 3], device=DEV), 1).reshape(dy.shape)
        assert 0.1 < (f == 0).mean() < 0.5 and len(np.unique(f)) == 2
        assert_out(g["y_dropped"], g["y"].astype(np.float64) * f, tag + ".y_dropped", atol=1e-7, rtol=1e-6)
        dy = dy * f
    dhT = None if d["dhT"] is None else d["dhT"].astype(np.float64)
    if c["head"]:
        dhT = (0.0 if dhT is None else dhT) + d["dlogits"].astype(np.float64) @ d["hw"].astype(np.float64)
    ref = run_literal(c["variant"], d["P"], d["x"], d["h0"], d["c0"], dy, dhT, d["dcT"], time_major=c["tm"])
    for k in ("y", "hT", "cT"):
        assert_out(g[k], ref[k], f"{tag}.{k}")
    for k in ("dx", "dh0", "dc0"):
        if k in g:
            assert_grad(g[k], ref[k], f"{tag}.{k}")
    for k in ORDER[c["variant"]]:
        assert_grad(g["g." + k], ref["G"][k], f"{tag}.grad.{k}")
    if c["head"]:
        hT = ref["hT"]
        assert_grad(g["logits"], hT @ d["hw"].astype(np.float64).T + d["hb"], tag + ".logits")
        assert_grad(g["dweight"], d["dlogits"].astype(np.float64).T @ hT, tag + ".dweight")
        assert_grad(g["dbias"], d["dlogits"].astype(np.float64).sum(0), tag + ".dbias")
    if c["ce"]:
        z, t = torch.tensor(g["logits"], dtype=torch.float64, requires_grad=True), torch.tensor(d["target"])
        loss = torch.nn.functional.cross_entropy(z, t, ignore_index=-100)
        loss.backward()
        assert abs(float(g["loss"][0]) - float(loss)) <= 2e-6 * max(1.0, abs(float(loss))), (float(g["loss"][0]), float(loss))
        assert float(g["nvalid"][0]) == float((d["target"] != -100).sum())
        assert_out(g["lse"], torch.logsumexp(z.detach(), 1).numpy(), tag + ".lse")
        assert_grad(g["dlogits_unit"], z.grad.numpy(), tag + ".dlogits_unit")


@pytest.mark.parametrize("c", LAYER_CASES, ids=[c["id"] for c in LAYER_CASES])
def test_layer_calls_on_poisoned_buffers(c):
    L = _lib()
    d = layer_inputs(c)
    with tuned(c["tune"]):
        runs = []
        for fill in FILLS:
            rings = L.tune_get("wring_launches")
            out, sz, fwd, bwd, desc = run_layer(c, d, fill)
            rings = L.tune_get("wring_launches") - rings
            # "wring" says what was asked for, the counter what ran: wgrad_ring_kernel itself, not the stand-alone fallback in its slot
            assert rings == c["ring"], f"{c['id']}: wgrad_ring_kernel was launched {rings} times, the case is meant for {c['ring']}"
            print(f"{c['id']} fill 0x{fill:08x}: rows_per_wg {sz.rows_per_wg} threads {sz.threads_per_wg} workgroups {sz.workgroups} kx {sz.kx} "
                  f"kh {sz.kh} ws {sz.workspace_bytes} reserve {sz.reserve_bytes}\n  forward {fwd}\n  backward {bwd}")
            for k, v in c["geo"].items():
                assert getattr(sz, k) == v, f"{c['id']}: vmlmf_query says {k} = {getattr(sz, k)}, the case is meant for {v}"
            if c["id"].startswith("cluster"):
                assert sz.workgroups >= 2 * -(-c["B"] // sz.rows_per_wg), "not a cluster of workgroups per row block"
            if c["id"].startswith("step"):
                assert sz.threads_per_wg != 256 or sz.rows_per_wg == 1
            expect_counts(fwd, {"rec_fwd_kernel": 1, **c["fwd"]}, c["id"] + " forward")
            expect_counts(bwd, {"finish_kernel": 0 if c["bwd"].get("finish2_kernel") else 1, **c["bwd"]}, c["id"] + " backward")
            for k, v in c["tune"].items():
                assert L.tune_get(k) == v, f"{c['id']}: switch {k} moved to {L.tune_get(k)} during the call"
            runs.append(out)
        same_under_every_fill(runs)
        if c["dtype"] == "f32":
            layer_oracle(c, d, runs[0], desc)


# ---- vmlmf_stack_* -------------------------------------------------------------------------------------------------------------
def sc(id, variant, B, T, I, Hs, rw, ru, tm=False, head=False, drop=False, st=False, tune=None, fwd=None, bwd=None, scale=0.1, clustered=False, ring=0):
    return dict(ring=ring, id=id, variant=variant, B=B, T=T, I=I, Hs=Hs, rw=rw, ru=ru, tm=tm, head=head, drop=drop, st=st, tune=tune or {}, fwd=fwd or {},
                bwd=bwd or {}, scale=scale, clustered=clustered)


WAVE = dict(fwd=dict(pack_kernel=1, rec_fwd_kernel=1), bwd=dict(rec_bwd_kernel=1, wgrad_mfma_kernel=1))
STACK_CASES = [
    sc("wave-2xv1-h24-h40", O.V1, 5, 3, 9, [24, 40], 16, [16], **WAVE),
    sc("wave-2xv2-states", O.V2, 21, 3, 9, [66, 66], 5, [5, 11], st=True, **WAVE),
    sc("wave-3xv3-h64-dropout", O.V3, 5, 3, 64, [64, 64, 64], 11, [11], tm=True, drop=True, **WAVE),
    sc("wave-2xv1-head", O.V1, 21, 3, 9, [65, 65], 11, [11], head=True, **WAVE),
    sc("rbx-2xv3-dropout", O.V3, 5, 3, 650, [650, 650], 32, [32], tm=True, drop=True, scale=0.03, clustered=True, tune=dict(rbx=1),
       fwd=dict(pack_kernel=1, rec_fwd_kernel=1), bwd=dict(rec_bwd_kernel=1, wgrad_mfma_kernel=2)),
    sc("rbx-2xv4-dropout-ffb=0", O.V4, 5, 3, 650, [650, 650], 32, [32, 32], tm=True, drop=True, scale=0.03, clustered=True,
       tune=dict(rbx=1, wring=1, ffb=0), ring=2, fwd=dict(rec_fwd_kernel=1), bwd=dict(rec_bwd_kernel=1, wgrad_mfma_kernel=2)),
    sc("rbx-2xv3-states-ffb=1", O.V3, 5, 3, 650, [650, 650], 32, [32], tm=True, st=True, scale=0.03, clustered=True,
       tune=dict(rbx=1, wring=1, ffb=1), ring=2, fwd=dict(rec_fwd_kernel=1), bwd=dict(rec_bwd_kernel=1, wgrad_mfma_kernel=2)),
]


def stack_inputs(c):
    rng = rng_for(c["id"])
    B, T, Hs = c["B"], c["T"], c["Hs"]
    sh = (T, B) if c["tm"] else (B, T)
    d = dict(P=[], x=(0.5 * rng.standard_normal(sh + (c["I"],))).astype(np.float32), dy=rng.standard_normal(sh + (Hs[-1],)).astype(np.float32))
    for l, H in enumerate(Hs):
        Il = c["I"] if l == 0 else Hs[l - 1]
        d["P"].append(O.make_params(c["variant"], Il, H, c["rw"], c["ru"] if c["variant"] in GROUPED else c["ru"][0], seed=30 + l, scale=c["scale"]))
    d["h0"] = [(0.4 * rng.standard_normal((B, H))).astype(np.float32) for H in Hs] if c["st"] else None
    d["c0"] = [(0.4 * rng.standard_normal((B, H))).astype(np.float32) for H in Hs] if c["st"] else None
    d["dhT"] = [rng.standard_normal((B, H)).astype(np.float32) for H in Hs]
    d["dcT"] = [rng.standard_normal((B, H)).astype(np.float32) for H in Hs]
    if c["head"]:
        d["hw"] = (0.1 * rng.standard_normal((CLASSES, Hs[-1]))).astype(np.float32)
        d["hb"] = (0.1 * rng.standard_normal(CLASSES)).astype(np.float32)
        d["dlogits"] = rng.standard_normal((B, CLASSES)).astype(np.float32)
    return d


def stack_descs(c):
    L = _lib()
    return [L.make_desc(c["variant"], c["B"], c["T"], c["I"] if l == 0 else c["Hs"][l - 1], H, c["rw"], c["ru"], g=2 if c["variant"] in GROUPED else 1,
                        time_major=c["tm"], training=True) for l, H in enumerate(c["Hs"])]


def stack_query(descs):
    L = _lib()
    n = len(descs)
    layers = (L.StackLayer * n)()
    for l in range(n):
        layers[l].desc = descs[l]
    rb, wb = (ctypes.c_size_t * n)(), ctypes.c_size_t()
    ok(L.lib().vmlmf_stack_query(n, ctypes.addressof(layers), ctypes.addressof(rb), ctypes.addressof(wb)), "stack_query")
    return [int(v) for v in rb], int(wb.value)


def run_stack(c, d, fill, short_workspace=False):
    L = _lib()
    lib = L.lib()
    variant, B, T, Hs = c["variant"], c["B"], c["T"], c["Hs"]
    n = len(Hs)
    names = ORDER[variant]
    descs = stack_descs(c)
    rbytes, wbytes = stack_query(descs)
    sh = (T, B) if c["tm"] else (B, T)
    pl = Plan()
    pl.add("x", sh + (c["I"],), init=d["x"]), pl.add("dy", sh + (Hs[-1],), init=d["dy"]), pl.add("dx", sh + (c["I"],), out=True)
    for l, H in enumerate(Hs):
        for k in names:
            pl.add(f"p{l}.{k}", d["P"][l][k].shape, init=d["P"][l][k])
            pl.add(f"g{l}.{k}", d["P"][l][k].shape, out=True)
        pl.add(f"y{l}", sh + (H,), out=True), pl.add(f"hT{l}", (B, H), out=True), pl.add(f"cT{l}", (B, H), out=True)
        pl.add(f"dhT{l}", (B, H), init=d["dhT"][l]), pl.add(f"dcT{l}", (B, H), init=d["dcT"][l])
        if c["st"]:
            pl.add(f"h0{l}", (B, H), init=d["h0"][l]), pl.add(f"c0{l}", (B, H), init=d["c0"][l])
            pl.add(f"dh0{l}", (B, H), out=True), pl.add(f"dc0{l}", (B, H), out=True)
        pl.add(f"reserve{l}", rbytes[l], U8)
        if c["drop"]:
            pl.add(f"y_dropped{l}", sh + (H,), out=True)
    if c["drop"]:
        pl.add("drop.state", 2, I64, init=np.array([987654321, 5], np.int64))
    pl.add("ws.forward", wbytes, U8), pl.add("ws.backward", wbytes, U8)
    if c["head"]:
        pl.add("head.weight", (CLASSES, Hs[-1]), init=d["hw"]), pl.add("head.bias", CLASSES, init=d["hb"])
        pl.add("head.dlogits", (B, CLASSES), init=d["dlogits"])
        pl.add("logits", (B, CLASSES), out=True), pl.add("dweight", (CLASSES, Hs[-1]), out=True), pl.add("dbias", CLASSES, out=True)
    arena, b = pl.alloc(fill)
    layers = (L.StackLayer * n)()
    keep = []
    for l in range(n):
        ps = params_struct(variant, [b[f"p{l}.{k}"] for k in names])
        gs = params_struct(variant, [b[f"g{l}.{k}"] for k in names])
        keep += [ps, gs]
        ly = layers[l]
        ly.desc, ly.params, ly.grads = descs[l], ctypes.pointer(ps), ctypes.pointer(gs)
        ly.y, ly.hT, ly.cT, ly.reserve = b[f"y{l}"].data_ptr(), b[f"hT{l}"].data_ptr(), b[f"cT{l}"].data_ptr(), b[f"reserve{l}"].data_ptr()
        ly.dhT, ly.dcT = b[f"dhT{l}"].data_ptr(), b[f"dcT{l}"].data_ptr()
        if c["st"]:
            ly.h0, ly.c0, ly.dh0, ly.dc0 = (b[f"{k}{l}"].data_ptr() for k in ("h0", "c0", "dh0", "dc0"))
        if c["drop"]:
            dr = L.Dropout(DROP_P, l + 1, b["drop.state"].data_ptr(), b[f"y_dropped{l}"].data_ptr())
            keep.append(dr)
            ly.drop = ctypes.pointer(dr)
    if c["drop"]:
        assert lib.vmlmf_stack_dropout_fused(n, ctypes.addressof(layers)) == 1
    hd = L.Head()
    if c["head"]:
        hd.classes, hd.weight, hd.bias, hd.logits = CLASSES, b["head.weight"].data_ptr(), b["head.bias"].data_ptr(), b["logits"].data_ptr()
        hd.dlogits, hd.dweight, hd.dbias = b["head.dlogits"].data_ptr(), b["dweight"].data_ptr(), b["dbias"].data_ptr()
    hp = ctypes.addressof(hd) if c["head"] else None
    s = stream()
    if short_workspace:
        rc = lib.vmlmf_stack_forward(n, ctypes.addressof(layers), p(b["x"]), hp, p(b["ws.forward"]), wbytes - 1, s)
        rc2 = lib.vmlmf_stack_backward(n, ctypes.addressof(layers), p(b["x"]), p(b["dy"]), p(b["dx"]), hp, p(b["ws.backward"]), wbytes - 1, s)
        return arena, b, pl, rc, rc2
    with counted() as fwd:
        ok(lib.vmlmf_stack_forward(n, ctypes.addressof(layers), p(b["x"]), hp, p(b["ws.forward"]), wbytes, s), "stack_forward")
    with counted() as bwd:
        ok(lib.vmlmf_stack_backward(n, ctypes.addressof(layers), p(b["x"]), p(b["dy"]), p(b["dx"]), hp, p(b["ws.backward"]), wbytes, s),
           "stack_backward")
    return settle(arena, b, pl), fwd.counts, bwd.counts, descs


def stack_oracle(c, d, got, descs):
    """(f): the layers chained through the literal restatement in fp64 (autograd), the dropout between them by the library's factors."""
    tag, n, variant = c["id"], len(c["Hs"]), c["variant"]
    g = {k: v.cpu().numpy() for k, v in got.items()}
    f64 = torch.float64
    Pt = [O.to_torch(P, dtype=f64, requires_grad=True) for P in d["P"]]
    xt = torch.tensor(d["x"], dtype=f64, requires_grad=True)
    h0 = [None] * n if d["h0"] is None else [torch.tensor(v, dtype=f64, requires_grad=True) for v in d["h0"]]
    c0 = [None] * n if d["c0"] is None else [torch.tensor(v, dtype=f64, requires_grad=True) for v in d["c0"]]
    cur, ys, hs, cs, loss = xt, [], [], [], 0.0
    for l in range(n):
        y, h, cc = O.literal_sequence(variant, Pt[l], cur, h0[l], c0[l], time_major=c["tm"], v4_scratch_rows=c["B"])
        ys.append(y), hs.append(h), cs.append(cc)
        loss = loss + (h * torch.tensor(d["dhT"][l], dtype=f64)).sum() + (cc * torch.tensor(d["dcT"][l], dtype=f64)).sum()
        cur = y
        if c["drop"]:
            f = lib_factors(descs[l], c["T"] * c["B"], c["Hs"][l], DROP_P, torch.tensor([987654321, 5], device=DEV), l + 1).reshape(tuple(y.shape))
            assert 0.1 < (f == 0).mean() < 0.5
            cur = y * torch.tensor(f)
            assert_out(g[f"y_dropped{l}"], g[f"y{l}"].astype(np.float64) * f, f"{tag}.y_dropped{l}", atol=1e-7, rtol=1e-6)
    loss = loss + (cur * torch.tensor(d["dy"], dtype=f64)).sum()
    if c["head"]:
        logits = hs[-1] @ torch.tensor(d["hw"], dtype=f64).T + torch.tensor(d["hb"], dtype=f64)
        loss = loss + (logits * torch.tensor(d["dlogits"], dtype=f64)).sum()
        assert_grad(g["logits"], logits.detach().numpy(), tag + ".logits")
        assert_grad(g["dweight"], d["dlogits"].astype(np.float64).T @ hs[-1].detach().numpy(), tag + ".dweight")
        assert_grad(g["dbias"], d["dlogits"].astype(np.float64).sum(0), tag + ".dbias")
    loss.backward()
    for l in range(n):
        assert_out(g[f"y{l}"], ys[l].detach().numpy(), f"{tag}.y{l}")
        assert_out(g[f"hT{l}"], hs[l].detach().numpy(), f"{tag}.hT{l}")
        assert_out(g[f"cT{l}"], cs[l].detach().numpy(), f"{tag}.cT{l}")
        if c["st"]:
            assert_grad(g[f"dh0{l}"], h0[l].grad.numpy(), f"{tag}.dh0{l}")
            assert_grad(g[f"dc0{l}"], c0[l].grad.numpy(), f"{tag}.dc0{l}")
        for k in ORDER[variant]:
            assert_grad(g[f"g{l}.{k}"], Pt[l][k].grad.numpy(), f"{tag}.grad{l}.{k}")
    assert_grad(g["dx"], xt.grad.numpy(), tag + ".dx")


@pytest.mark.parametrize("c", STACK_CASES, ids=[c["id"] for c in STACK_CASES])
def test_stack_calls_on_poisoned_buffers(c):
    L = _lib()
    d = stack_inputs(c)
    with tuned(c["tune"]):
        q0 = L.query(stack_descs(c)[0])
        if c["clustered"]:     # every layer on clusters of workgroups: the family vmlmf_stack_* runs in one launch per direction
            assert q0.threads_per_wg == 256 and q0.workgroups >= 2 * -(-c["B"] // q0.rows_per_wg), (q0.threads_per_wg, q0.workgroups)
        else:
            assert q0.rows_per_wg == 1 and q0.workgroups == c["B"]
        runs = []
        for fill in FILLS:
            rings = L.tune_get("wring_launches")
            out, fwd, bwd, descs = run_stack(c, d, fill)
            rings = L.tune_get("wring_launches") - rings
            assert rings == c["ring"], f"{c['id']}: wgrad_ring_kernel was launched {rings} times, the case is meant for {c['ring']}"
            print(f"{c['id']} fill 0x{fill:08x}:\n  forward {fwd}\n  backward {bwd}")
            expect_counts(fwd, {"xproj_kernel": 0, **c["fwd"]}, c["id"] + " forward")       # every layer's x side inside the launch
            expect_counts(bwd, {"dqx_dx_kernel": 0, **c["bwd"]}, c["id"] + " backward")
            assert bwd["finish_kernel"] >= 1
            if "ffb" in c["tune"]:
                assert bwd["reduce_cg_kernel"] == 0 if c["tune"]["ffb"] else bwd["reduce_cg_kernel"] <= 1
            runs.append(out)
        same_under_every_fill(runs)
        stack_oracle(c, d, runs[0], descs)


# ---- a workspace one byte short: VMLMF_E_WORKSPACE, and nothing launched --------------------------------------------------------
def test_a_short_workspace_is_refused_and_nothing_is_written():
    L = _lib()
    lib = L.lib()
    c = LAYER_CASES[0]
    d = layer_inputs(c)
    for fill in FILLS[1:]:
        desc = L.make_desc(c["variant"], c["B"], c["T"], c["I"], c["H"], c["rw"], c["ru"], time_major=c["tm"], training=True)
        sz = L.query(desc)
        names = ORDER[c["variant"]]
        pl = Plan()
        for k in names:
            pl.add("p." + k, d["P"][k].shape, init=d["P"][k]), pl.add("g." + k, d["P"][k].shape, out=True)
        B, T, I, H = c["B"], c["T"], c["I"], c["H"]
        pl.add("x", (B, T, I), init=d["x"]), pl.add("dy", (B, T, H), init=d["dy"])
        for k, shape in (("y", (B, T, H)), ("hT", (B, H)), ("cT", (B, H)), ("dx", (B, T, I)), ("dh0", (B, H)), ("dc0", (B, H))):
            pl.add(k, shape, out=True)
        pl.add("reserve", sz.reserve_bytes, U8, out=True), pl.add("ws", sz.workspace_bytes, U8, out=True)
        arena, b = pl.alloc(fill)
        ps = params_struct(c["variant"], [b["p." + k] for k in names])
        gs = params_struct(c["variant"], [b["g." + k] for k in names])
        s = stream()
        with counted() as n:
            rc = lib.vmlmf_seq_forward(ctypes.byref(desc), ctypes.byref(ps), p(b["x"]), None, None, p(b["y"]), p(b["hT"]), p(b["cT"]), p(b["reserve"]),
                                       p(b["ws"]), sz.workspace_bytes - 1, s)
            assert rc == L.E_WORKSPACE, rc
            rc = lib.vmlmf_seq_backward(ctypes.byref(desc), ctypes.byref(ps), p(b["x"]), None, None, p(b["y"]), p(b["reserve"]), p(b["dy"]), None, None,
                                        p(b["dx"]), p(b["dh0"]), p(b["dc0"]), ctypes.byref(gs), p(b["ws"]), sz.workspace_bytes - 1, s)
            assert rc == L.E_WORKSPACE, rc
        assert sum(n.counts.values()) == 0, n.counts
        torch.cuda.synchronize()
        arena.check_guards()
        for name in pl.out:
            assert_untouched(arena, name, b[name])
        # the stack entry points
        sc_ = STACK_CASES[0]
        arena, b, pl, rc, rc2 = run_stack(sc_, stack_inputs(sc_), fill, short_workspace=True)
        assert (rc, rc2) == (L.E_WORKSPACE, L.E_WORKSPACE), (rc, rc2)
        torch.cuda.synchronize()
        arena.check_guards()
        for name in pl.out + [k for k in b if k.startswith(("reserve", "ws."))]:
            assert_untouched(arena, name, b[name])


# ---- flat kernels ----------------------------------------------------------------------------------------------------------------
def flat(make):
    """make(fill) -> (arena, buffers, plan) after launching; settles every fill, compares them, returns the zero fill's outputs."""
    runs = []
    for fill in FILLS:
        arena, b, pl = make(fill)
        runs.append(settle(arena, b, pl))
    same_under_every_fill(runs)
    return {k: v.cpu() for k, v in runs[0].items()}


def test_flat_head_forward_backward_strided():
    """h is the last-timestep slice of a (B, T, H) output: row stride ldh = T H; the rows between are poison."""
    B, T, H, C = 21, 3, 65, 18
    r = rng_for("head")
    y, w, bias, dl = (r.standard_normal(s).astype(np.float32) for s in ((B, T, H), (C, H), (C,), (B, C)))

    def make(fill):
        pl = Plan()
        pl.add("y", (B, T, H)), pl.add("w", (C, H), init=w), pl.add("bias", C, init=bias), pl.add("dlogits", (B, C), init=dl)
        for k, s in (("logits", (B, C)), ("dh", (B, H)), ("dweight", (C, H)), ("dbias", (C,))):
            pl.add(k, s, out=True)
        arena, b = pl.alloc(fill)
        b["y"][:, T - 1, :] = torch.tensor(y[:, T - 1, :], device=DEV)     # only the slice the call may read holds values
        h = ctypes.c_void_p(b["y"].data_ptr() + 4 * (T - 1) * H)
        with counted() as n:
            ok(_lib().lib().vmlmf_head_forward(B, H, C, h, T * H, p(b["w"]), p(b["bias"]), p(b["logits"]), stream()), "head_forward")
            ok(_lib().lib().vmlmf_head_backward(B, H, C, h, T * H, p(b["w"]), p(b["dlogits"]), p(b["dh"]), p(b["dweight"]), p(b["dbias"]), stream()),
               "head_backward")
        expect_counts(n.counts, dict(head_fwd_kernel=1, head_bwd_kernel=1), "head")
        return arena, b, pl
    got = flat(make)
    hl = y[:, T - 1, :].astype(np.float64)
    assert_grad(got["logits"].numpy(), hl @ w.T.astype(np.float64) + bias, "logits")
    assert_grad(got["dh"].numpy(), dl.astype(np.float64) @ w, "dh")
    assert_grad(got["dweight"].numpy(), dl.T.astype(np.float64) @ hl, "dweight")
    assert_grad(got["dbias"].numpy(), dl.astype(np.float64).sum(0), "dbias")


def test_flat_ce_forward_backward_with_ignored_rows():
    B, C = 21, 18
    r = rng_for("ce")
    z = r.standard_normal((B, C)).astype(np.float32)
    t = r.integers(0, C, B).astype(np.int64)
    t[[0, 7, 20]] = -100

    def make(fill):
        pl = Plan()
        pl.add("logits", (B, C), init=z), pl.add("target", B, I64, init=t), pl.add("dloss", 1, init=np.array([1.5], np.float32))
        for k, s in (("loss", 1), ("lse", B), ("nvalid", 1), ("dlogits_unit", (B, C)), ("dlogits", (B, C))):
            pl.add(k, s, out=True)
        arena, b = pl.alloc(fill)
        with counted() as n:
            ok(_lib().lib().vmlmf_ce_forward(B, C, p(b["logits"]), p(b["target"]), -100, p(b["loss"]), p(b["lse"]), p(b["nvalid"]),
                                             p(b["dlogits_unit"]), stream()), "ce_forward")
            ok(_lib().lib().vmlmf_ce_backward(B, C, p(b["logits"]), p(b["target"]), -100, p(b["lse"]), p(b["nvalid"]), p(b["dloss"]),
                                              p(b["dlogits"]), stream()), "ce_backward")
        expect_counts(n.counts, dict(ce_fwd_kernel=1, ce_bwd_kernel=1), "ce")
        return arena, b, pl
    got = flat(make)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    ref = torch.nn.functional.cross_entropy(zt, torch.tensor(t), ignore_index=-100)
    ref.backward()
    assert abs(float(got["loss"]) - float(ref)) <= 2e-6 * abs(float(ref)) and float(got["nvalid"]) == B - 3
    assert_grad(got["dlogits_unit"].numpy(), zt.grad.numpy(), "dlogits_unit")
    assert_grad(got["dlogits"].numpy(), 1.5 * zt.grad.numpy(), "dlogits")


@pytest.mark.parametrize("R,V", [(15, 1000), (7, 12288), (5, 12293)], ids=["V1000", "V12288", "V12293"])
def test_flat_nll_forward_backward_and_the_one_pass_form(R, V):
    r = rng_for("nll%d" % V)
    z = r.standard_normal((R, V)).astype(np.float32)
    bias = (0.1 * r.standard_normal(V)).astype(np.float32)
    yv = r.integers(0, V, R).astype(np.int64)
    scale = 0.25
    lib = _lib().lib()
    fused = V % 4 == 0 and V <= 12288

    def make(fill):
        pl = Plan()
        pl.add("scores", (R, V), init=z + bias), pl.add("y", R, I64, init=yv), pl.add("dloss", 1, init=np.array([1.0], np.float32))
        for k, s in (("loss", 1), ("lse", R), ("rowloss", R), ("dscores", (R, V))):
            pl.add(k, s, out=True)
        if fused:
            pl.add("scores.inplace", (R, V), init=z, out=True), pl.add("bias", V, init=bias)
            pl.add("loss2", 1, out=True), pl.add("rowloss2", R, out=True), pl.add("dbias", V, out=True)
            pl.add("scratch", int(lib.vmlmf_nll_grad_scratch_floats(R, V)))
        arena, b = pl.alloc(fill)
        ok(lib.vmlmf_nll_forward(R, V, p(b["scores"]), p(b["y"]), scale, p(b["loss"]), p(b["lse"]), p(b["rowloss"]), stream()), "nll_forward")
        ok(lib.vmlmf_nll_backward(R, V, p(b["scores"]), p(b["y"]), scale, p(b["lse"]), p(b["dloss"]), p(b["dscores"]), stream()), "nll_backward")
        if fused:
            ok(lib.vmlmf_nll_forward_grad(R, V, p(b["scores.inplace"]), p(b["bias"]), p(b["y"]), scale, p(b["loss2"]), p(b["rowloss2"]), p(b["dbias"]),
                                          p(b["scratch"]), stream()), "nll_forward_grad")
        return arena, b, pl
    got = flat(make)
    zt = torch.tensor((z + bias).astype(np.float64), requires_grad=True)
    ref = scale * torch.nn.functional.cross_entropy(zt, torch.tensor(yv), reduction="sum")
    ref.backward()
    assert abs(float(got["loss"]) - float(ref)) <= 1e-5 * abs(float(ref))
    assert_grad(got["dscores"].numpy(), zt.grad.numpy(), "dscores")
    if fused:
        assert abs(float(got["loss2"]) - float(ref)) <= 1e-5 * abs(float(ref))
        assert_grad(got["scores.inplace"].numpy(), zt.grad.numpy(), "dscores in place")
        assert_grad(got["dbias"].numpy(), zt.grad.numpy().sum(0), "dbias")


def test_flat_embedding_gradients_with_repeated_and_unselected_rows():
    R, H, V = 45, 65, 37
    r = rng_for("embed")
    tok = r.integers(0, 11, R).astype(np.int64)          # tokens repeat; vocabulary rows 11 .. 36 are selected by nobody
    tok[3] = V - 1
    dyv, w = r.standard_normal((R, H)).astype(np.float32), r.standard_normal((V, H)).astype(np.float32)
    lib = _lib().lib()
    nb = int(lib.vmlmf_embed_backward_scratch_bytes(R, V))

    def make(fill):
        pl = Plan()
        pl.add("tokens", R, I64, init=tok), pl.add("dy", (R, H), init=dyv), pl.add("weight", (V, H), init=w)
        pl.add("state", 2, I64, init=np.array([42, 7], np.int64))
        pl.add("dweight", (V, H), out=True), pl.add("scratch", nb, U8)
        pl.add("out", (R, H), out=True), pl.add("dweight.drop", (V, H), out=True), pl.add("scratch.drop", nb, U8)
        arena, b = pl.alloc(fill)
        s = stream()
        ok(lib.vmlmf_embed_backward(R, H, V, p(b["tokens"]), p(b["dy"]), p(b["dweight"]), p(b["scratch"]), nb, s), "embed_backward")
        ok(lib.vmlmf_embed_dropout_forward(R, H, V, p(b["tokens"]), p(b["weight"]), p(b["out"]), DROP_P, p(b["state"]), 0, s), "embed_dropout_forward")
        ok(lib.vmlmf_embed_dropout_backward(R, H, V, p(b["tokens"]), p(b["dy"]), p(b["dweight.drop"]), p(b["scratch.drop"]), nb, DROP_P, p(b["state"]),
                                            0, s), "embed_dropout_backward")
        return arena, b, pl
    got = flat(make)
    f = lib_factors(None, R, H, DROP_P, torch.tensor([42, 7], device=DEV), 0)
    ref = np.zeros((V, H)), np.zeros((V, H))
    for i in range(R):
        ref[0][tok[i]] += dyv[i]
        ref[1][tok[i]] += dyv[i].astype(np.float64) * f[i]
    assert_grad(got["dweight"].numpy(), ref[0], "dweight")
    assert_grad(got["dweight.drop"].numpy(), ref[1], "dweight under dropout")
    assert_out(got["out"].numpy(), w[tok].astype(np.float64) * f, "embed_dropout_forward", atol=1e-7, rtol=1e-6)
    assert not got["dweight"][11:V - 1].any()


def test_flat_dropout_apply_factors_and_transpose():
    R, H = 45, 65
    rows, cols = 37, 129
    r = rng_for("dropout")
    xv, m = r.standard_normal((R, H)).astype(np.float32), r.standard_normal((rows, cols)).astype(np.float32)
    lib = _lib().lib()

    def make(fill):
        pl = Plan()
        pl.add("x", (R, H), init=xv), pl.add("state", 2, I64, init=np.array([42, 7], np.int64)), pl.add("src", (rows, cols), init=m)
        pl.add("y", (R, H), out=True), pl.add("factors", (R, H), out=True), pl.add("dst", (cols, rows), out=True)
        arena, b = pl.alloc(fill)
        s = stream()
        ok(lib.vmlmf_dropout_apply(R, H, p(b["x"]), p(b["y"]), DROP_P, p(b["state"]), 2, s), "dropout_apply")
        ok(lib.vmlmf_dropout_factors(None, R, H, DROP_P, p(b["state"]), 2, p(b["factors"]), s), "dropout_factors")
        ok(lib.vmlmf_transpose(rows, cols, p(b["src"]), p(b["dst"]), s), "transpose")
        return arena, b, pl
    got = flat(make)
    assert torch.equal(got["dst"], torch.tensor(m).t().contiguous())
    assert torch.equal(got["y"], torch.tensor(xv) * got["factors"])
    assert 0.15 < float((got["factors"] == 0).float().mean()) < 0.45


@pytest.mark.parametrize("form", ["plain", "guarded", "ex"])
def test_flat_adam_steps(form):
    """plain / guarded: one tensor above 2^20 elements, the size from which the header says a guarded list takes a tick launch and an update
    launch; ex: a list of small tensors, which the header says takes one launch.  (The optimizers have no slot in vmlmf_profile_*: which
    form ran is not observable here, the results are - the guard's verdict and ticket words, and every element against fp64.)"""
    L = _lib()
    lib = L.lib()
    sizes = [(1 << 20) + 13, 650, 37] if form != "ex" else [650, 37]
    r = rng_for("adam")
    pv = [r.standard_normal(n).astype(np.float32) for n in sizes]
    gv = [r.standard_normal(n).astype(np.float32) for n in sizes]
    total = sum(sizes)
    mv, vv = (0.1 * r.standard_normal(total)).astype(np.float32), (0.01 * r.standard_normal(total) ** 2).astype(np.float32)
    L.tune("clear_health", 0)

    def make(fill):
        pl = Plan()
        for i, n in enumerate(sizes):
            pl.add(f"param{i}", n, init=pv[i], out=True), pl.add(f"grad{i}", n, init=gv[i])
        pl.add("exp_avg", total, init=mv, out=True), pl.add("exp_avg_sq", total, init=vv, out=True)
        pl.add("steps", len(sizes), init=np.full(len(sizes), 3.0, np.float32), out=True)
        if form != "plain":
            pl.add("guard", L.GUARD_WORDS, I32, init=0, out=True)
        arena, b = pl.alloc(fill)
        tl = L.TensorList()
        o = 0
        for i, n in enumerate(sizes):
            tl.param[i], tl.grad[i], tl.numel[i], tl.state_offset[i], tl.step_index[i] = b[f"param{i}"].data_ptr(), b[f"grad{i}"].data_ptr(), n, o, i
            o += n
        tl.count = len(sizes)
        args = (ctypes.byref(tl), p(b["exp_avg"]), p(b["exp_avg_sq"]), p(b["steps"]), 1e-3, 0.9, 0.999, 1e-8, 0.01)
        if form == "plain":
            ok(lib.vmlmf_adam_step(*args, stream()), "adam_step")
        elif form == "guarded":
            ok(lib.vmlmf_adam_step_guarded(*args, p(b["guard"]), stream()), "adam_step_guarded")
        else:
            ok(lib.vmlmf_adam_step_ex(*args, p(b["guard"]), L.ADAM_FIRST | L.ADAM_LAST, stream()), "adam_step_ex")
        return arena, b, pl
    got = flat(make)
    if form != "plain":
        gw = got["guard"]
        assert int(gw[L.GUARD_GO]) == 1 and int(gw[L.GUARD_SKIPPED]) == 0 and int(gw[:L.GUARD_GO].abs().sum()) == 0 and int(gw[65]) == 0, gw
    assert got["steps"].tolist() == [4.0] * len(sizes)
    o = 0
    for i, n in enumerate(sizes):
        w, g_ = torch.tensor(pv[i], dtype=torch.float64), torch.tensor(gv[i], dtype=torch.float64)
        g_ = g_ + 0.01 * w
        m1 = 0.9 * torch.tensor(mv[o:o + n], dtype=torch.float64) + 0.1 * g_
        v1 = 0.999 * torch.tensor(vv[o:o + n], dtype=torch.float64) + 0.001 * g_ * g_
        ref = w - 1e-3 / (1 - 0.9 ** 4) * m1 / ((v1 / (1 - 0.999 ** 4)).sqrt() + 1e-8)
        assert_out(got[f"param{i}"].numpy(), ref.numpy(), f"param{i}", atol=1e-6, rtol=1e-5)
        assert_out(got["exp_avg"][o:o + n].numpy(), m1.numpy(), f"exp_avg{i}", atol=1e-7, rtol=1e-5)
        o += n


def test_flat_sgd_clip_step():
    L = _lib()
    lib = L.lib()
    sizes = [70001, 650, 37]
    r = rng_for("sgd")
    pv = [r.standard_normal(n).astype(np.float32) for n in sizes]
    gv = [r.standard_normal(n).astype(np.float32) for n in sizes]

    def make(fill):
        pl = Plan()
        for i, n in enumerate(sizes):
            pl.add(f"param{i}", n, init=pv[i], out=True), pl.add(f"grad{i}", n, init=gv[i], out=True)
        pl.add("norm", 1, out=True), pl.add("scratch", L.MAX_TENSORS * 64)
        arena, b = pl.alloc(fill)
        tl = L.TensorList()
        for i, n in enumerate(sizes):
            tl.param[i], tl.grad[i], tl.numel[i], tl.state_offset[i], tl.step_index[i] = b[f"param{i}"].data_ptr(), b[f"grad{i}"].data_ptr(), n, 0, i
        tl.count = len(sizes)
        ok(lib.vmlmf_sgd_clip_step(ctypes.byref(tl), 0.5, 0.25, p(b["norm"]), p(b["scratch"]), stream()), "sgd_clip_step")
        return arena, b, pl
    got = flat(make)
    norm = float(np.sqrt(sum((g.astype(np.float64) ** 2).sum() for g in gv)))
    assert abs(float(got["norm"]) - norm) <= 1e-5 * norm
    k = 0.25 / (norm + 1e-6)
    for i in range(len(sizes)):
        assert_out(got[f"grad{i}"].numpy(), k * gv[i].astype(np.float64), f"grad{i}", atol=1e-7, rtol=1e-4)
        assert_out(got[f"param{i}"].numpy(), pv[i] - 0.5 * k * gv[i].astype(np.float64), f"param{i}", atol=1e-6, rtol=1e-4)


@pytest.mark.parametrize("V", [97, 12293])
@pytest.mark.parametrize("form", ["sample", "sample_filtered", "choose", "choose_filtered"])
def test_flat_lm_sample_and_choose(form, V):
    """V = 12293: past the row the filtered sampler keeps in LDS, and no multiple of four."""
    lib = _lib().lib()
    B, H = 5, 33
    r = rng_for("sample")
    h, w = r.standard_normal((B, H)).astype(np.float32), (0.3 * r.standard_normal((V, H))).astype(np.float32)
    bias, emb = (0.1 * r.standard_normal(V)).astype(np.float32), r.standard_normal((V, H)).astype(np.float32)
    scores = (h.astype(np.float64) @ w.T.astype(np.float64)).astype(np.float32)
    filtered, fused = form.endswith("filtered"), form.startswith("sample")
    nws = int((lib.vmlmf_lm_sample_filtered_workspace_bytes if filtered else lib.vmlmf_lm_sample_workspace_bytes)(B, V))

    def make(fill):
        pl = Plan()
        pl.add("bias", V, init=bias), pl.add("embed", (V, H), init=emb), pl.add("state", 2, I64, init=np.array([99, 4], np.int64))
        if fused:
            pl.add("h", (B, H), init=h), pl.add("weight", (V, H), init=w), pl.add("ticket", 1, I64, init=0, zero_after=True), pl.add("workspace", nws, U8)
        else:
            pl.add("scores", (B, V), init=scores)
        pl.add("tokens", B, I64, out=True), pl.add("logprob", B, out=True), pl.add("x_next", (B, H), out=True)
        if filtered:
            pl.add("kept", B, I32, out=True)
        arena, b = pl.alloc(fill)
        tail = (p(b["state"]), 3, p(b["tokens"]), p(b["logprob"]), p(b["x_next"]))
        if form == "sample":
            rc = lib.vmlmf_lm_sample(B, H, V, p(b["h"]), p(b["weight"]), p(b["bias"]), p(b["embed"]), 0.8, *tail, p(b["ticket"]), p(b["workspace"]), nws, stream())
        elif form == "sample_filtered":
            rc = lib.vmlmf_lm_sample_filtered(B, H, V, p(b["h"]), p(b["weight"]), p(b["bias"]), p(b["embed"]), 0.8, 40, 0.9, *tail, p(b["kept"]),
                                              p(b["ticket"]), p(b["workspace"]), nws, stream())
        elif form == "choose":
            rc = lib.vmlmf_lm_choose(B, H, V, p(b["scores"]), p(b["bias"]), p(b["embed"]), 0.8, *tail, stream())
        else:
            rc = lib.vmlmf_lm_choose_filtered(B, H, V, p(b["scores"]), p(b["bias"]), p(b["embed"]), 0.8, 40, 0.9, *tail, p(b["kept"]), stream())
        ok(rc, form)
        return arena, b, pl
    got = flat(make)
    tok = got["tokens"].numpy()
    assert ((0 <= tok) & (tok < V)).all()
    ls = torch.log_softmax(torch.tensor(scores.astype(np.float64) + bias), 1).numpy()
    assert_out(got["logprob"].numpy(), ls[np.arange(B), tok], form + ".logprob", atol=2e-5, rtol=1e-4)
    assert torch.equal(got["x_next"], torch.tensor(emb[tok]))
    if filtered:
        assert ((1 <= got["kept"].numpy()) & (got["kept"].numpy() <= 40)).all()


# ---- the three side libraries -----------------------------------------------------------------------------------------------------
def test_side_library_controlled_choice():
    from vmlmf_amd import _decode
    B, H, V = 5, 33, 97
    r = rng_for("decode")
    scores, bias, emb = r.standard_normal((B, V)).astype(np.float32), (0.1 * r.standard_normal(V)).astype(np.float32), r.standard_normal((V, H)).astype(np.float32)
    lb = np.zeros(V, np.float32)
    lb[[3, 50]] = -np.inf
    seen = (r.random((B, V)) < 0.1).astype(np.uint8)

    def make(fill):
        pl = Plan()
        pl.add("scores", (B, V), init=scores), pl.add("bias", V, init=bias), pl.add("embed", (V, H), init=emb)
        pl.add("state", 2, I64, init=np.array([99, 4], np.int64)), pl.add("logit_bias", V, init=lb)
        pl.add("seen", (B, V), U8, init=seen, out=True), pl.add("finished", B, I32, init=np.array([0, 1, 0, 0, 0], np.int32), out=True)
        pl.add("length", B, I32, init=np.array([2, 4, 0, 1, 9], np.int32), out=True)
        pl.add("tokens", B, I64, out=True), pl.add("logprob", B, out=True), pl.add("x_next", (B, H), out=True), pl.add("kept", B, I32, out=True)
        arena, b = pl.alloc(fill)
        c = _decode.Controls(1.3, 7, 3, 0, b["logit_bias"].data_ptr(), b["seen"].data_ptr(), b["finished"].data_ptr(), b["length"].data_ptr())
        _decode.LIBRARY.call(device(), "vmlmf_decode_choose", B, H, V, p(b["scores"]), p(b["bias"]), p(b["embed"]), 0.8, 20, 0.9,
                             p(b["state"]), 2, ctypes.byref(c), p(b["tokens"]), p(b["logprob"]), p(b["x_next"]), p(b["kept"]))
        return arena, b, pl
    got = flat(make)
    tok = got["tokens"].numpy()
    assert tok[1] == 7 and float(got["logprob"][1]) == 0.0            # a finished row emits eos at log-probability 0
    assert not np.isin(tok[[0, 2, 3, 4]], [3, 50]).any() and tok[2] != 7 and tok[3] != 7      # bans; eos held back below min_length
    assert torch.equal(got["x_next"], torch.tensor(emb[tok]))
    live = np.array([0, 2, 3, 4])
    assert got["seen"][live, tok[live]].all()                              # a live row has now held its token


def test_side_library_beam_step_gather_backtrack():
    from vmlmf_amd import _beam
    B, W, H, V = 3, 5, 33, 97
    r = rng_for("beam")
    scores, bias, emb = r.standard_normal((B * W, V)).astype(np.float32), (0.1 * r.standard_normal(V)).astype(np.float32), r.standard_normal((V, H)).astype(np.float32)
    cum = -np.abs(r.standard_normal((B, W))).astype(np.float32)
    fin, ln = np.zeros((B, W), np.int32), np.full((B, W), 2, np.int32)
    fin[1, 2] = 1
    state = r.standard_normal((B * W, H)).astype(np.float32)
    nws = int(_beam.lib().vmlmf_beam_workspace_bytes(B, W, V))
    dev = device()

    def make(fill):
        pl = Plan()
        pl.add("scores", (B * W, V), init=scores), pl.add("bias", V, init=bias), pl.add("embed", (V, H), init=emb), pl.add("cum", (B, W), init=cum)
        pl.add("finished", (B, W), I32, init=fin), pl.add("length", (B, W), I32, init=ln), pl.add("state.h", (B * W, H), init=state)
        pl.add("parent", (1, B, W), I32, out=True), pl.add("token", (1, B, W), I64, out=True), pl.add("total", (B, W), out=True)
        pl.add("finished_out", (B, W), I32, out=True), pl.add("length_out", (B, W), I32, out=True), pl.add("x_next", (B * W, H), out=True)
        pl.add("src_row", B * W, I32, out=True), pl.add("ticket", B, I32, init=0, zero_after=True), pl.add("workspace", nws, U8)
        pl.add("state.gathered", (B * W, H), out=True), pl.add("hypotheses", (1, B, W), I64, out=True)
        arena, b = pl.alloc(fill)
        _beam.LIBRARY.call(dev, "vmlmf_beam_step", B, W, H, V, p(b["scores"]), p(b["bias"]), p(b["cum"]), p(b["finished"]), p(b["length"]), 7, p(b["embed"]),
                           p(b["parent"]), p(b["token"]), p(b["total"]), p(b["finished_out"]), p(b["length_out"]), p(b["x_next"]), p(b["src_row"]),
                           p(b["ticket"]), p(b["workspace"]), nws)
        vp = ctypes.c_void_p
        _beam.LIBRARY.call(dev, "vmlmf_beam_gather", 1, B * W, H, p(b["src_row"]), (vp * 1)(b["state.h"].data_ptr()), (vp * 1)(b["state.gathered"].data_ptr()))
        _beam.LIBRARY.call(dev, "vmlmf_beam_backtrack", 1, B, W, p(b["parent"]), p(b["token"]), None, p(b["hypotheses"]))
        return arena, b, pl
    got = flat(make)
    ls = torch.log_softmax(torch.tensor(scores.astype(np.float64) + bias), 1).reshape(B, W, V) + torch.tensor(cum.astype(np.float64))[:, :, None]
    ls[1, 2] = -np.inf
    ls[1, 2, 7] = float(cum[1, 2])                                      # a finished beam offers eos alone, at its total so far
    best = ls.reshape(B, W * V).topk(W, dim=1)
    assert_out(got["total"].numpy(), best.values.numpy(), "beam.total", atol=2e-5, rtol=1e-4)
    assert torch.equal(got["parent"][0].long() * V + got["token"][0], best.indices)
    assert torch.equal(got["src_row"].view(B, W).long(), torch.arange(B)[:, None] * W + got["parent"][0].long())
    assert torch.equal(got["state.gathered"], torch.tensor(state)[got["src_row"].long()])
    assert torch.equal(got["hypotheses"], got["token"]) and torch.equal(got["x_next"], torch.tensor(emb)[got["token"].reshape(-1)])


def test_side_library_score_rows_top8():
    from vmlmf_amd import _score
    R, V, top = 7, 12293, 8
    r = rng_for("score")
    scores, bias = r.standard_normal((R, V)).astype(np.float32), (0.1 * r.standard_normal(V)).astype(np.float32)
    tg = r.integers(0, V, R).astype(np.int64)

    def make(fill):
        pl = Plan()
        pl.add("scores", (R, V), init=scores), pl.add("bias", V, init=bias), pl.add("targets", R, I64, init=tg)
        pl.add("logprob", R, out=True), pl.add("rank", R, I32, out=True), pl.add("top_tokens", (R, top), I64, out=True)
        pl.add("top_logprob", (R, top), out=True)
        arena, b = pl.alloc(fill)
        _score.LIBRARY.call(device(), "vmlmf_score_rows", R, V, p(b["scores"]), p(b["bias"]), p(b["targets"]), top, p(b["logprob"]),
                            p(b["rank"]), p(b["top_tokens"]), p(b["top_logprob"]))
        return arena, b, pl
    got = flat(make)
    xs = torch.tensor(scores) + torch.tensor(bias)
    ls = torch.log_softmax(xs.double(), 1)
    assert_out(got["logprob"].numpy(), ls[torch.arange(R), torch.tensor(tg)].numpy(), "score.logprob", atol=2e-5, rtol=1e-4)
    assert torch.equal(got["top_tokens"], xs.topk(top, dim=1).indices)
    assert torch.equal(got["rank"].long(), (xs > xs[torch.arange(R), torch.tensor(tg)][:, None]).sum(1))
