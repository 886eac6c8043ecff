"""Host-only sweep of the C ABI: every entry point that decides something on the host (geometry, layouts, stack plans, argument
checks, the switch table) is called over a grid of descriptors and bad arguments, and return code, outputs and vmlmf_last_error()
text are written as JSON lines.  Every case is refused in front of the first launch (its pointers are fakes), so the sweep needs no
GPU (the CU-count lookup then falls back to 256) - and must not have one: the worker refuses to start where a device is visible, and
a case that comes back with a HIP error code, i.e. reached a launch, fails the run.

    python tools/host_sweep.py --worker OUT.jsonl          # the library VMLMF_LIB names (default: the in-tree build)
    python tools/host_sweep.py --compare A.so B.so OUT     # one process per library; OUT: a header line (cases, differences),
                                                           # a line per entry point, the error texts reached
"""
import ctypes
import hashlib
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# refusals of make_geo and of the stack plans that no argument reaches (every other one is among the cases)
UNREACHABLE = {
    "padded hidden rank (summed over groups) > 128 is not covered on a register-resident layer":
        "a register-resident layer has a padded rank of at most 32 per group and at most two groups",
    "stack: at most four clustered layers": "vmlmf_stack_* refuse more than four layers before they look at the form",
}
FAKE = 0x10000   # a non-null pointer no case lets the library dereference or hand to a launch


def worker(out_path):
    import torch
    if torch.cuda.is_available():
        sys.exit("host_sweep: a GPU is visible; the cases pass fake pointers and must never reach one (hide it: HIP_VISIBLE_DEVICES=-1)")
    from vmlmf_amd import _lib as L
    lib = L.lib()
    out = open(out_path, "w")
    n = [0]

    def rec(call, args, rc, **outs):
        r = {"call": call, "args": args, "rc": rc}
        r.update(outs)
        if rc > 0 and not call.split(".")[0].endswith("fused"):
            sys.exit("host_sweep: case %s %s got as far as a launch (HIP error %d): fix the case" % (call, args, rc))
        if rc != 0 and not call.split(".")[0].endswith("fused"):
            r["err"] = lib.vmlmf_last_error().decode()
        out.write(json.dumps(r) + "\n")
        n[0] += 1

    def desc_of(a):
        v, B, T, I, H, rw, ru, g, tm, tr, dt = a
        return L.make_desc(v, B, T, I, H, rw, ru, g=g, time_major=tm, training=tr, dtype=dt)

    def layer_calls(a, tag=""):
        d = desc_of(a)
        s = L.Sizes()
        rc = lib.vmlmf_query(ctypes.byref(d), ctypes.byref(s))
        rec("query" + tag, a, rc, out=[getattr(s, f) for f, _ in L.Sizes._fields_] if rc == 0 else None)
        nb = ctypes.c_size_t(0)
        rc = lib.vmlmf_pack_bytes(ctypes.byref(d), ctypes.byref(nb))
        rec("pack_bytes" + tag, a, rc, out=nb.value if rc == 0 else None)
        rec("dropout_fused" + tag, a, lib.vmlmf_dropout_fused(ctypes.byref(d)))

    # ---- layers: (B, T, I, H, w_rank, u_rank) on each side of every family boundary of make_geo
    shapes = [
        (32, 16, 9, 180, 16, 16),      # register-resident, x-fold
        (96, 16, 9, 180, 16, 16),      # ... beyond the riding workers' batch
        (32, 16, 180, 180, 16, 16),    # ... I == H (the LM variants)
        (32, 8, 64, 512, 32, 32),      # 512 thread slots: the last register-resident size
        (32, 8, 64, 576, 32, 32),      # ... one wave more: step-wise / clustered
        (32, 8, 650, 650, 32, 32),     # clustered H = 650
        (32, 8, 650, 650, 32, 40),     # padded u_rank > 32
        (32, 8, 200, 64, 16, 16),      # I > H
        (32, 8, 180, 180, 40, 16),     # padded w_rank > 32 on a register-resident layer
        (16, 4, 650, 650, 300, 300),   # wide (the LM's default ranks)
        (8, 2, 1100, 1100, 1024, 64),  # wide, at the cap
        (8, 2, 1100, 1100, 1025, 64),  # ... one beyond
        (8, 2, 650, 650, 700, 32),     # wide: w_rank > input_size
        (8, 2, 650, 650, 300, 700),    # wide: u_rank > units
        (4096, 4096, 9, 180, 16, 16),  # 32-bit offsets
    ]
    for v, sh, tm, dt, tr in itertools.product(range(1, 7), shapes, (0, 1), (0, 1), (0, 1)):
        grouped = v in (2, 4, 6)
        B, T, I, H, rw, ru = sh
        layer_calls([v, B, T, I, H, rw, [ru // 2, ru // 2] if grouped else [ru], 2 if grouped else 1, tm, tr, dt])
    bad = [
        [0, 8, 8, 9, 180, 16, [16], 1, 0, 1, 0], [7, 8, 8, 9, 180, 16, [16], 1, 0, 1, 0], [1, 8, 8, 9, 180, 16, [16], 1, 0, 1, 2],
        [1, 0, 8, 9, 180, 16, [16], 1, 0, 1, 0], [1, 8, 8, 9, 180, 0, [16], 1, 0, 1, 0], [1, 8, 8, 9, 180, 16, [0], 1, 0, 1, 0],
        [2, 8, 8, 9, 180, 16, [8, 0], 2, 0, 1, 0], [2, 8, 8, 9, 180, 16, [8, 8], 0, 0, 1, 0], [2, 8, 8, 9, 180, 16, [8, 8], 3, 0, 1, 0],
        [2, 8, 8, 9, 181, 16, [8, 8], 2, 0, 1, 0], [3, 8, 8, 9, 180, 16, [16], 1, 0, 1, 0], [1, 8, 8, 181, 180, 16, [16], 1, 0, 1, 0],
    ]
    for a in bad:
        layer_calls(a, ".bad")
    rec("query.null", None, lib.vmlmf_query(None, ctypes.byref(L.Sizes())))
    rec("query.null_out", None, lib.vmlmf_query(ctypes.byref(desc_of(bad[0])), None))
    rec("pack_bytes.null_out", None, lib.vmlmf_pack_bytes(ctypes.byref(desc_of(bad[0])), None))
    rec("dropout_fused.null", None, lib.vmlmf_dropout_fused(None))

    # ---- the switch table: every key, one unknown key; the family switches move the grid above
    def tune_get(k):
        v = ctypes.c_int(-12345)
        rc = lib.vmlmf_tune_get(k, ctypes.byref(v))
        rec("tune_get", k.decode() if k else None, rc, out=v.value)
        return v.value
    keys = [b"adam_guard", b"rb", b"rb_min_batch", b"rb_cluster", b"rb_rows", b"rec3", b"inrow", b"wring", b"direct", b"finish2", b"rbx",
            b"ffb", b"wride", b"test_wride_spin", b"clear_health", b"no_such_key", None]
    for k in keys:
        before = tune_get(k)
        for val in (-1, 0, 1, 7):
            rec("tune", [k.decode() if k else None, val], lib.vmlmf_tune(k, val), gen=lib.vmlmf_tune_generation())
            tune_get(k)
        if k not in (b"test_wride_spin", b"clear_health", b"no_such_key", None):
            lib.vmlmf_tune(k, 1 if k == b"wride" else before)
    lib.vmlmf_tune(b"test_wride_spin", 0)
    rec("tune_get.null_out", None, lib.vmlmf_tune_get(b"rb", None))
    sub = [(32, 16, 9, 180, 16, 16), (32, 8, 64, 576, 32, 32), (32, 8, 650, 650, 32, 32), (256, 8, 650, 650, 32, 32)]
    for key, val in ((b"rb", 1), (b"rb", 0), (b"rb_min_batch", 32), (b"rb_cluster", 4), (b"rb_rows", 8)):
        before = ctypes.c_int(0)
        lib.vmlmf_tune_get(key, ctypes.byref(before))
        lib.vmlmf_tune(key, val)
        for v, sh, tm in itertools.product(range(1, 7), sub, (0, 1)):
            grouped = v in (2, 4, 6)
            B, T, I, H, rw, ru = sh
            layer_calls([v, B, T, I, H, rw, [ru // 2, ru // 2] if grouped else [ru], 2 if grouped else 1, tm, 1, 0], ".%s=%d" % (key.decode(), val))
        lib.vmlmf_tune(key, before.value)

    # ---- stacks
    def fake_params():
        p = L.Params()
        for f, t in L.Params._fields_:
            if t is ctypes.c_void_p:
                setattr(p, f, FAKE)
            else:
                for i in range(len(getattr(p, f))):
                    getattr(p, f)[i] = FAKE
        return p

    def stack_of(layers, fill=False, drop=None):
        arr = (L.StackLayer * max(len(layers), 1))()
        keep = []
        for l, a in enumerate(layers):
            arr[l].desc = desc_of(a)
            if fill:
                p, gr = fake_params(), fake_params()
                keep += [p, gr]
                arr[l].params, arr[l].grads = ctypes.pointer(p), ctypes.pointer(gr)
                arr[l].y = arr[l].reserve = FAKE
            if drop is not None and drop[0] == l:
                dr = L.Dropout(drop[1], l, FAKE, FAKE)
                keep.append(dr)
                arr[l].drop = ctypes.pointer(dr)
        return arr, keep

    def stack_calls(name, layers):
        n_l = len(layers)
        arr, keep = stack_of(layers)
        res = (ctypes.c_size_t * 8)()
        wsb = ctypes.c_size_t(0)
        rc = lib.vmlmf_stack_query(n_l, arr, res, ctypes.byref(wsb))
        rec("stack_query", [name, layers], rc, out=[list(res)[:n_l], wsb.value] if rc == 0 else None)
        rec("stack_dropout_fused", [name, n_l], lib.vmlmf_stack_dropout_fused(n_l, arr))
        big = 1 << 40
        for what, head, x, ws, nbytes, fill, drop in (
                ("null_x", None, None, FAKE, big, True, None), ("small_ws", None, FAKE, FAKE, 64, True, None),
                ("null_params", None, FAKE, FAKE, big, False, None), ("bad_p", None, FAKE, FAKE, big, True, (n_l - 1, 1.5)),
                ("bad_head", L.Head(40, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE), FAKE, FAKE, big, True, None),
                ("head_null_ptr", L.Head(4, None, None, None, None, None, None), FAKE, FAKE, big, True, None)):
            arr2, keep2 = stack_of(layers, fill, drop)
            hp = ctypes.byref(head) if head is not None else None
            rec("stack_forward." + what, name, lib.vmlmf_stack_forward(n_l, arr2, x, hp, ws, nbytes, None))
            rec("stack_backward." + what, name, lib.vmlmf_stack_backward(n_l, arr2, x, FAKE, None, hp, ws, nbytes, None))

    def wf(l, B=32, H=64, I0=20, v=1, r=16, tm=0, tr=1, dt=0, g=1):
        return [v, B, 12, I0 if l == 0 else H, H, r, [r // g] * g, g, tm, tr, dt]

    def cl(B=32, v=3, tm=1, tr=1, H=650, g=1):
        return [v, B, 8, H, H, 32, [32] * g, g, tm, tr, 0]
    for n_l in range(1, 6):
        stack_calls("wavefront", [wf(l) for l in range(n_l)])
        stack_calls("wavefront.inference", [wf(l, tr=0) for l in range(n_l)])
        stack_calls("wavefront.group", [wf(l, v=2, g=2) for l in range(n_l)])
        stack_calls("wavefront.bf16_tape", [wf(l, dt=1) for l in range(n_l)])
        stack_calls("clustered", [cl() for _ in range(n_l)])
        stack_calls("clustered.group", [cl(v=4, g=2) for _ in range(n_l)])
        stack_calls("clustered.B256", [cl(B=256) for _ in range(n_l)])
    stack_calls("mixed_sizes", [wf(0, H=64), [1, 32, 12, 64, 128, 16, [16], 1, 0, 1, 0], [1, 32, 12, 128, 128, 16, [16], 1, 0, 1, 0]])
    stack_calls("mixed_sizes.group", [wf(0, v=2, g=2), [2, 32, 12, 64, 128, 16, [8, 8], 2, 0, 1, 0]])
    stack_calls("mixed_sizes.ranks_differ", [[1, 32, 12, 20, 64, 8, [16], 1, 0, 1, 0], [1, 32, 12, 64, 128, 8, [16], 1, 0, 1, 0]])
    stack_calls("refused.B_differs", [wf(0), wf(1, B=16)])
    stack_calls("refused.input_size", [wf(0), [1, 32, 12, 48, 64, 16, [16], 1, 0, 1, 0]])
    stack_calls("refused.variant_v4", [wf(0, v=4, g=2, I0=64), wf(1, v=4, g=2)])
    stack_calls("refused.rank_32_four_waves", [wf(0, H=256, r=32), wf(1, H=256, r=32)])
    stack_calls("refused.bf16_rank_8", [wf(0, dt=1, r=8), wf(1, dt=1, r=8)])
    stack_calls("refused.bf16_4096_rows", [wf(0, dt=1, B=4096), wf(1, dt=1, B=4096)])
    stack_calls("refused.bf16_one_layer_only", [wf(0, dt=1), wf(1)])
    stack_calls("refused.bad_layer", [wf(0), [1, 32, 12, 64, 64, 0, [16], 1, 0, 1, 0]])
    stack_calls("refused.clustered_batch_major", [cl(tm=0), cl(tm=0)])
    stack_calls("refused.clustered_differ", [cl(), cl(tr=0)])
    stack_calls("refused.clustered_v1", [cl(v=1), cl(v=1)])
    stack_calls("refused.clustered_not_coresident", [cl(B=2048), cl(B=2048)])
    stack_calls("refused.clustered_bad_layer", [cl(), [3, 32, 8, 650, 650, 0, [32], 1, 1, 1, 0]])
    for val in (0, 2):
        lib.vmlmf_tune(b"rbx", val)
        for n_l in (1, 2):
            stack_calls("clustered.rbx=%d" % val, [cl() for _ in range(n_l)])
    lib.vmlmf_tune(b"rbx", 1)
    rec("stack_query.null", None, lib.vmlmf_stack_query(2, None, None, None))
    rec("stack_dropout_fused.null", None, lib.vmlmf_stack_dropout_fused(2, None))
    rec("stack_forward.null_layers", None, lib.vmlmf_stack_forward(2, None, FAKE, None, FAKE, 1 << 40, None))
    rec("stack_backward.null_layers", None, lib.vmlmf_stack_backward(2, None, FAKE, FAKE, None, None, FAKE, 1 << 40, None))

    # ---- one layer's entry points: every refusal in front of the first launch
    big = 1 << 40
    valu, rb, gen = desc_of([1, 32, 16, 9, 180, 16, [16], 1, 0, 1, 0]), desc_of([1, 32, 16, 9, 180, 16, [16], 1, 1, 1, 1]), desc_of(
        [3, 32, 8, 650, 650, 32, [32], 1, 1, 1, 0])
    P, G = fake_params(), fake_params()
    Pn = L.Params()
    P2 = fake_params()
    P2.u_h[1] = None
    gd = desc_of([2, 32, 16, 9, 180, 16, [8, 8], 2, 0, 1, 0])

    def fwd(name, d, p, x, y, res, ws, nbytes, ex=None, hT=FAKE):
        rec("seq_forward_ex." + name, None, lib.vmlmf_seq_forward_ex(ctypes.byref(d), p, x, None, None, y, hT, None, res, ws, nbytes, None, ex))

    def bwd(name, d, p, gr, x, y, res, ws, nbytes, ex=None, dhT=None):
        rec("seq_backward_ex." + name, None,
            lib.vmlmf_seq_backward_ex(ctypes.byref(d), p, x, None, None, y, res, FAKE, dhT, None, None, None, None, gr, ws, nbytes, None, ex))
    pp, gp = ctypes.byref(P), ctypes.byref(G)
    fwd("null_params", valu, None, FAKE, FAKE, FAKE, FAKE, big)
    fwd("null_pointer_in_params", valu, ctypes.byref(Pn), FAKE, FAKE, FAKE, FAKE, big)
    fwd("group_needs_u_h1", gd, ctypes.byref(P2), FAKE, FAKE, FAKE, FAKE, big)
    fwd("null_x", valu, pp, None, FAKE, FAKE, FAKE, big)
    fwd("null_reserve", valu, pp, FAKE, FAKE, None, FAKE, big)
    fwd("small_ws", valu, pp, FAKE, FAKE, FAKE, FAKE, 64)
    bwd("null_grads", valu, pp, None, FAKE, FAKE, FAKE, FAKE, big)
    bwd("null_pointer_in_grads", valu, pp, ctypes.byref(Pn), FAKE, FAKE, FAKE, FAKE, big)
    bwd("null_x", valu, pp, gp, None, FAKE, FAKE, FAKE, big)
    bwd("small_ws", valu, pp, gp, FAKE, FAKE, FAKE, FAKE, 64)
    for name, d in (("valu", valu), ("rb", rb), ("clustered", gen)):
        for hname, hd in (("40_classes", L.Head(40, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE)), ("null_ptr", L.Head(4, None, None, None, None, None, None))):
            ex = L.Extra(None, ctypes.pointer(hd), None, None)
            fwd("head_%s.%s" % (hname, name), d, pp, FAKE, FAKE, FAKE, FAKE, big, ctypes.byref(ex))
            bwd("head_%s.%s" % (hname, name), d, pp, gp, FAKE, FAKE, FAKE, FAKE, big, ctypes.byref(ex))
        hd = L.Head(4, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE)
        ex = L.Extra(None, ctypes.pointer(hd), None, None)
        if name != "valu":   # (the VALU kernels carry the classifier: accepted there, the calls would launch)
            fwd("head_needs_hT." + name, d, pp, FAKE, FAKE, FAKE, FAKE, big, ctypes.byref(ex), hT=None)
            bwd("head_with_dhT." + name, d, pp, gp, FAKE, FAKE, FAKE, FAKE, big, ctypes.byref(ex), dhT=FAKE)
        ce = L.Ce(FAKE, -100, FAKE, FAKE, FAKE, FAKE, FAKE)
        fwd("ce_without_head." + name, d, pp, FAKE, FAKE, FAKE, FAKE, big, ctypes.byref(L.Extra(None, None, ctypes.pointer(ce), None)))
        fwd("ce_null_ptr." + name, d, pp, FAKE, FAKE, FAKE, FAKE, big,
            ctypes.byref(L.Extra(None, ctypes.pointer(hd), ctypes.pointer(L.Ce(None, -100, FAKE, FAKE, FAKE, FAKE, FAKE)), None)))
        for dname, dr in (("p", L.Dropout(1.0, 0, FAKE, FAKE)), ("null_state", L.Dropout(0.5, 0, None, FAKE)),
                          ("null_y_dropped", L.Dropout(0.5, 0, FAKE, None)), ("family", L.Dropout(0.5, 0, FAKE, FAKE))):
            if dname == "family" and name != "valu":
                continue   # (the row-block layers, clustered ones included, take it: the call would launch)
            ex = L.Extra(None, None, None, ctypes.pointer(dr))
            fwd("drop_%s.%s" % (dname, name), d, pp, FAKE, FAKE, FAKE, FAKE, big, ctypes.byref(ex))
            if dname != "null_y_dropped" or name == "valu":   # (a backward needs no y_dropped: accepted on the row-block layers)
                bwd("drop_%s.%s" % (dname, name), d, pp, gp, FAKE, FAKE, FAKE, FAKE, big, ctypes.byref(ex))
        ex = L.Extra(FAKE, None, None, None)   # a kept image nobody packed
        fwd("packed_unknown." + name, d, pp, FAKE, FAKE, FAKE, FAKE, big, ctypes.byref(ex))
        bwd("packed_unknown." + name, d, pp, gp, FAKE, FAKE, FAKE, FAKE, big, ctypes.byref(ex))
        rec("pack_params.null_packed." + name, None, lib.vmlmf_pack_params(ctypes.byref(d), pp, None, None))
        rec("pack_params.null_params." + name, None, lib.vmlmf_pack_params(ctypes.byref(d), None, FAKE, None))
    rec("pack_params.clustered", None, lib.vmlmf_pack_params(ctypes.byref(gen), pp, FAKE, None))
    rec("seq_forward.null_x", None, lib.vmlmf_seq_forward(ctypes.byref(valu), pp, None, None, None, FAKE, None, None, FAKE, FAKE, big, None))
    rec("seq_backward.null_x", None,
        lib.vmlmf_seq_backward(ctypes.byref(valu), pp, None, None, None, FAKE, FAKE, FAKE, None, None, None, None, None, gp, FAKE, big, None))
    rec("seq_forward_packed.unknown", None,
        lib.vmlmf_seq_forward_packed(ctypes.byref(valu), pp, FAKE, None, None, FAKE, None, None, FAKE, FAKE, big, None, FAKE))
    rec("seq_backward_packed.unknown", None, lib.vmlmf_seq_backward_packed(ctypes.byref(valu), pp, FAKE, None, None, FAKE, FAKE, FAKE, None, None,
                                                                           None, None, None, gp, FAKE, big, None, FAKE))

    def profile_counts():   # (no launch ran: every slot is empty)
        us, cnt = (ctypes.c_float * L.NKERNELS)(), (ctypes.c_int32 * L.NKERNELS)()
        return [lib.vmlmf_profile_read(us, cnt, 0), list(us), list(cnt)]

    # ---- the thin entry points, each with an out-of-range and a null argument
    f = ctypes.c_float
    for name, call in (
            ("head_forward.range", lambda: lib.vmlmf_head_forward(0, 8, 4, FAKE, 8, FAKE, FAKE, FAKE, None)),
            ("head_forward.ldh", lambda: lib.vmlmf_head_forward(4, 8, 4, FAKE, 7, FAKE, FAKE, FAKE, None)),
            ("head_forward.classes", lambda: lib.vmlmf_head_forward(4, 8, 33, FAKE, 8, FAKE, FAKE, FAKE, None)),
            ("head_forward.null", lambda: lib.vmlmf_head_forward(4, 8, 4, None, 8, FAKE, FAKE, FAKE, None)),
            ("head_backward.range", lambda: lib.vmlmf_head_backward(4, 0, 4, FAKE, 8, FAKE, FAKE, FAKE, FAKE, FAKE, None)),
            ("head_backward.classes", lambda: lib.vmlmf_head_backward(4, 8, 33, FAKE, 8, FAKE, FAKE, FAKE, FAKE, FAKE, None)),
            ("head_backward.null", lambda: lib.vmlmf_head_backward(4, 8, 4, FAKE, 8, FAKE, None, FAKE, FAKE, FAKE, None)),
            ("ce_forward.range", lambda: lib.vmlmf_ce_forward(0, 4, FAKE, FAKE, -100, FAKE, FAKE, FAKE, FAKE, None)),
            ("ce_forward.null", lambda: lib.vmlmf_ce_forward(4, 4, FAKE, None, -100, FAKE, FAKE, FAKE, FAKE, None)),
            ("ce_backward.range", lambda: lib.vmlmf_ce_backward(4, 0, FAKE, FAKE, -100, FAKE, FAKE, FAKE, FAKE, None)),
            ("ce_backward.null", lambda: lib.vmlmf_ce_backward(4, 4, FAKE, FAKE, -100, FAKE, FAKE, None, FAKE, None)),
            ("nll_forward.range", lambda: lib.vmlmf_nll_forward(0, 4, FAKE, FAKE, f(1), FAKE, FAKE, FAKE, None)),
            ("nll_forward.null", lambda: lib.vmlmf_nll_forward(4, 4, None, FAKE, f(1), FAKE, FAKE, FAKE, None)),
            ("nll_backward.range", lambda: lib.vmlmf_nll_backward(4, 0, FAKE, FAKE, f(1), FAKE, FAKE, FAKE, None)),
            ("nll_backward.null", lambda: lib.vmlmf_nll_backward(4, 4, FAKE, FAKE, f(1), FAKE, FAKE, None, None)),
            ("nll_forward_grad.range", lambda: lib.vmlmf_nll_forward_grad(0, 4, FAKE, FAKE, FAKE, f(1), FAKE, FAKE, FAKE, FAKE, None)),
            ("nll_forward_grad.null", lambda: lib.vmlmf_nll_forward_grad(4, 4, FAKE, FAKE, FAKE, f(1), FAKE, FAKE, FAKE, None, None)),
            ("embed_backward.range", lambda: lib.vmlmf_embed_backward(4, 0, 9, FAKE, FAKE, FAKE, FAKE, 64, None)),
            ("embed_backward.null", lambda: lib.vmlmf_embed_backward(4, 8, 9, None, FAKE, FAKE, FAKE, 64, None)),
            ("dropout_advance.null", lambda: lib.vmlmf_dropout_advance(None, FAKE, None)),
            ("dropout_advance.same", lambda: lib.vmlmf_dropout_advance(FAKE, FAKE, None)),
            ("dropout_apply.range", lambda: lib.vmlmf_dropout_apply(-1, 8, FAKE, FAKE, f(0.5), FAKE, 0, None)),
            ("dropout_apply.p", lambda: lib.vmlmf_dropout_apply(4, 8, FAKE, FAKE, f(1.0), FAKE, 0, None)),
            ("dropout_apply.p_nan", lambda: lib.vmlmf_dropout_apply(4, 8, FAKE, FAKE, f(float("nan")), FAKE, 0, None)),
            ("dropout_apply.null", lambda: lib.vmlmf_dropout_apply(4, 8, None, FAKE, f(0.5), FAKE, 0, None)),
            ("dropout_apply.null_state", lambda: lib.vmlmf_dropout_apply(4, 8, FAKE, FAKE, f(0.5), None, 0, None)),
            ("dropout_apply.2^32", lambda: lib.vmlmf_dropout_apply(1 << 32, 8, FAKE, FAKE, f(0.5), FAKE, 0, None)),
            ("dropout_factors.bad_desc", lambda: lib.vmlmf_dropout_factors(ctypes.byref(desc_of(bad[0])), 4, 180, f(0.5), FAKE, 0, FAKE, None)),
            ("dropout_factors.H", lambda: lib.vmlmf_dropout_factors(ctypes.byref(valu), 4, 64, f(0.5), FAKE, 0, FAKE, None)),
            ("dropout_factors.p", lambda: lib.vmlmf_dropout_factors(ctypes.byref(rb), 4, 180, f(-0.5), FAKE, 0, FAKE, None)),
            ("dropout_factors.null", lambda: lib.vmlmf_dropout_factors(None, 4, 180, f(0.5), FAKE, 0, None, None)),
            ("embed_dropout_forward.V", lambda: lib.vmlmf_embed_dropout_forward(4, 8, 0, FAKE, FAKE, FAKE, f(0.5), FAKE, 0, None)),
            ("embed_dropout_forward.p", lambda: lib.vmlmf_embed_dropout_forward(4, 8, 9, FAKE, FAKE, FAKE, f(2.0), FAKE, 0, None)),
            ("embed_dropout_forward.null", lambda: lib.vmlmf_embed_dropout_forward(4, 8, 9, None, FAKE, FAKE, f(0.5), FAKE, 0, None)),
            ("embed_dropout_backward.range", lambda: lib.vmlmf_embed_dropout_backward(0, 8, 9, FAKE, FAKE, FAKE, FAKE, 64, f(0.5), FAKE, 0, None)),
            ("embed_dropout_backward.null", lambda: lib.vmlmf_embed_dropout_backward(4, 8, 9, FAKE, FAKE, FAKE, FAKE, 64, f(0.5), None, 0, None)),
            ("embed_dropout_backward.p", lambda: lib.vmlmf_embed_dropout_backward(4, 8, 9, FAKE, FAKE, FAKE, FAKE, 64, f(-0.1), FAKE, 0, None)),
            ("lm_sample.range", lambda: lib.vmlmf_lm_sample(0, 8, 9, FAKE, FAKE, FAKE, FAKE, f(1), FAKE, 0, FAKE, FAKE, FAKE, FAKE, FAKE, big, None)),
            ("lm_sample.null", lambda: lib.vmlmf_lm_sample(4, 8, 9, None, FAKE, FAKE, FAKE, f(1), FAKE, 0, FAKE, FAKE, FAKE, FAKE, FAKE, big, None)),
            ("lm_sample.temperature", lambda: lib.vmlmf_lm_sample(4, 8, 9, FAKE, FAKE, FAKE, FAKE, f(-1), FAKE, 0, FAKE, FAKE, FAKE, FAKE, FAKE, big, None)),
            ("lm_sample.state", lambda: lib.vmlmf_lm_sample(4, 8, 9, FAKE, FAKE, FAKE, FAKE, f(1), None, 0, FAKE, FAKE, FAKE, FAKE, FAKE, big, None)),
            ("lm_sample.embed", lambda: lib.vmlmf_lm_sample(4, 8, 9, FAKE, FAKE, FAKE, None, f(1), FAKE, 0, FAKE, FAKE, FAKE, FAKE, FAKE, big, None)),
            ("lm_sample.step", lambda: lib.vmlmf_lm_sample(4, 8, 9, FAKE, FAKE, FAKE, FAKE, f(1), FAKE, -1, FAKE, FAKE, FAKE, FAKE, FAKE, big, None)),
            ("lm_sample.2^32", lambda: lib.vmlmf_lm_sample(1 << 20, 8, 9, FAKE, FAKE, FAKE, FAKE, f(1), FAKE, 1 << 13, FAKE, FAKE, FAKE, FAKE, FAKE, big, None)),
            ("lm_sample.small_ws", lambda: lib.vmlmf_lm_sample(4, 8, 9, FAKE, FAKE, FAKE, FAKE, f(1), FAKE, 0, FAKE, FAKE, FAKE, FAKE, FAKE, 1, None)),
            ("lm_choose.range", lambda: lib.vmlmf_lm_choose(4, 8, 0, FAKE, FAKE, FAKE, f(1), FAKE, 0, FAKE, FAKE, FAKE, None)),
            ("lm_choose.null", lambda: lib.vmlmf_lm_choose(4, 8, 9, None, FAKE, FAKE, f(1), FAKE, 0, FAKE, FAKE, FAKE, None)),
            ("lm_choose.temperature", lambda: lib.vmlmf_lm_choose(4, 8, 9, FAKE, FAKE, FAKE, f(float("inf")), FAKE, 0, FAKE, FAKE, FAKE, None)),
            ("lm_choose.state", lambda: lib.vmlmf_lm_choose(4, 8, 9, FAKE, FAKE, FAKE, f(1), None, 0, FAKE, FAKE, FAKE, None)),
            ("lm_choose.embed", lambda: lib.vmlmf_lm_choose(4, 8, 9, FAKE, FAKE, None, f(1), FAKE, 0, FAKE, FAKE, FAKE, None)),
            ("lm_choose.step", lambda: lib.vmlmf_lm_choose(4, 8, 9, FAKE, FAKE, FAKE, f(1), FAKE, -1, FAKE, FAKE, FAKE, None)),
            ("lm_choose.2^32", lambda: lib.vmlmf_lm_choose(1 << 20, 8, 9, FAKE, FAKE, FAKE, f(1), FAKE, 1 << 13, FAKE, FAKE, FAKE, None)),
            ("transpose.range", lambda: lib.vmlmf_transpose(0, 8, FAKE, FAKE + 64, None)),
            ("transpose.same", lambda: lib.vmlmf_transpose(8, 8, FAKE, FAKE, None)),
            ("check_status", lambda: lib.vmlmf_check_status()),
            ("profile_read.null", lambda: lib.vmlmf_profile_read(None, None, 1)),
            ("profile_enable", lambda: lib.vmlmf_profile_enable(0))):
        rec(name, None, call())
    for name, val in (("abi_version", lib.vmlmf_abi_version()), ("build_info", lib.vmlmf_build_info().decode()),
                      ("nll_grad_scratch_floats", [lib.vmlmf_nll_grad_scratch_floats(r, v) for r, v in ((0, 0), (7, 33), (4096, 10000))]),
                      ("embed_backward_scratch_bytes", [lib.vmlmf_embed_backward_scratch_bytes(r, v) for r, v in ((0, 0), (7, 33), (4096, 10000))]),
                      ("lm_sample_workspace_bytes", [lib.vmlmf_lm_sample_workspace_bytes(b, v) for b, v in ((0, 9), (4, 0), (32, 10000))]),
                      ("profile_read", profile_counts()),
                      ("kernel_name", [lib.vmlmf_kernel_name(k).decode() for k in range(-1, 15)])):
        rec(name, None, 0, out=val)
    out.close()
    print("%d cases -> %s" % (n[0], out_path))


def compare(lib_a, lib_b, out_path):
    runs = []
    for tag, path in (("a", lib_a), ("b", lib_b)):
        tmp = "%s.%s.tmp" % (out_path, tag)
        env = dict(os.environ, VMLMF_LIB=os.path.abspath(path))
        subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", tmp], check=True, env=env)
        runs.append(open(tmp).read().splitlines())
        os.remove(tmp)
    a, b = runs
    diffs = [i for i in range(max(len(a), len(b))) if i >= len(a) or i >= len(b) or a[i] != b[i]]
    for i in diffs[:20]:
        print("DIFF\n  a:", a[i] if i < len(a) else None, "\n  b:", b[i] if i < len(b) else None)
    errs = sorted({json.loads(r).get("err") for r in b} - {None})
    groups = {}   # entry point -> [cases, differences, {return code: cases}, digest of A's records, of B's]
    for i in range(max(len(a), len(b))):
        ra, rb = (a[i] if i < len(a) else ""), (b[i] if i < len(b) else "")
        r = json.loads(rb or ra)
        g = groups.setdefault(r["call"].split(".")[0], [0, 0, {}, hashlib.sha256(), hashlib.sha256()])
        g[0] += 1
        g[1] += ra != rb
        g[2][str(r["rc"])] = g[2].get(str(r["rc"]), 0) + 1
        g[3].update(ra.encode())
        g[4].update(rb.encode())
    with open(out_path, "w") as f:
        f.write(json.dumps({"what": "host-only sweep of the C ABI (tools/host_sweep.py: the grid of cases is defined there), the parent commit's "
                                    "library against this tree's, one process each: return code, every output field and the vmlmf_last_error() "
                                    "text of every case; below, per entry point: cases, differing cases, cases per return code, sha256 over "
                                    "the records of either library; then every distinct error text reached",
                            "cases": len(b), "differences": len(diffs), "distinct_error_texts": len(errs),
                            "refusals_no_descriptor_reaches": UNREACHABLE}) + "\n")
        for name, g in groups.items():
            f.write(json.dumps({"entry": name, "cases": g[0], "differences": g[1], "rc": g[2], "sha256_parent": g[3].hexdigest()[:16],
                                "sha256_new": g[4].hexdigest()[:16]}) + "\n")
        f.write(json.dumps({"error_texts": errs}) + "\n")
    print("%d cases, %d differences, %d distinct error texts -> %s" % (len(b), len(diffs), len(errs), out_path))
    return 1 if diffs else 0


if __name__ == "__main__":
    if sys.argv[1] == "--worker":
        worker(sys.argv[2])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[4]))
