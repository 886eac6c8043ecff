"""torch.autograd bridge over the C ABI: one call = one layer over the whole sequence.

PyTorch supplies device memory (caching allocator), the current HIP stream and autograd bookkeeping; all
arithmetic of the hot path happens in libvmlmf_hip.so.  Tensors must live on a HIP device.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import ptr as _ptr

# order in which parameter tensors are passed to VmlmfSeqFn (and gradients come back)
#   V1-V4: dia_x dia_h u_x v_x b_x b_h u_h[0] v_h[0] (u_h[1] v_h[1])
#   V6:    u_x v_x b_x b_h u_h[0] v_h[0] u_h[1] v_h[1]                       (no vm vectors)
#   V5:    w u w1 w2 w3 w4 u1 u2 u3 u4 bias_i bias_f bias_o bias_c          (gate order of the kernels: i, f, o, c~)
N_FIXED = 6


# ---- C++ binding (csrc/torch_binding.cpp: TORCH_LIBRARY "vmlmf" with C++ autograd functions over the same C ABI) --------
# Loaded when vmlmf_amd/lib/libvmlmf_torch.so has been built (`make -C vmlmf_amd/csrc torch`, done by
# __graft_entry__.build()).  Same kernels, same results; it only takes the per-call bookkeeping out of Python (eager
# steps of the unchanged reference loop are host-bound at the UCI-HAR shape).  VMLMF_PYBIND=ctypes keeps the classes below.
_OPS = None


def torch_ops():
    """torch.ops.vmlmf, or None when the C++ binding is not built / disabled."""
    global _OPS
    if _OPS is None:
        _OPS = False
        import os
        path = os.path.join(os.path.dirname(_lib.LIB_PATH), "libvmlmf_torch.so")
        if os.environ.get("VMLMF_PYBIND", "") != "ctypes" and os.path.exists(path) and "VMLMF_LIB" not in os.environ:
            _lib.lib()                       # libvmlmf_hip.so first (the binding links against it)
            try:
                torch.ops.load_library(path)
                _OPS = torch.ops.vmlmf
            except OSError:
                _OPS = False
    return _OPS or None


def _params_struct(tensors, g, variant=_lib.V1_CELL):
    p = _lib.Params()
    if variant == _lib.V5_LMF_CELL:
        p.u_x, p.u_h[0] = tensors[0].data_ptr(), tensors[1].data_ptr()
        for k in range(4):
            p.w_gate[k] = tensors[2 + k].data_ptr()
            p.u_gate[k] = tensors[6 + k].data_ptr()
            p.b_gate[k] = tensors[10 + k].data_ptr()
        return p
    names = ["dia_x", "dia_h", "u_x", "v_x", "b_x", "b_h"]
    if variant == _lib.V6_GROUP_NOVM:
        names = names[2:]
    for name, t in zip(names, tensors[:len(names)]):
        setattr(p, name, t.data_ptr())
    for s in range(g):
        p.u_h[s] = tensors[len(names) + 2 * s].data_ptr()
        p.v_h[s] = tensors[len(names) + 2 * s + 1].data_ptr()
    return p


def _hidden_size(variant, params):
    if variant == _lib.V5_LMF_CELL:
        return params[1].shape[0]              # u (H, ru)
    if variant == _lib.V6_GROUP_NOVM:
        return params[2].shape[-1] // 4        # bias_x (1, 4H)
    return params[1].shape[-1]                 # dia_h (1, H)


def _layer_cfg(variant, g, w_rank, u_ranks, time_major, dtype):
    """The configuration of a layer call as the 6-tuple (variant, g, w_rank, u_ranks, time_major, dtype) that the autograd classes
    take and every host cache below keys on."""
    ur = tuple(u_ranks) if isinstance(u_ranks, (list, tuple)) else (int(u_ranks),)
    return (variant, g, int(w_rank), ur, bool(time_major), _lib.DTYPES[dtype] if isinstance(dtype, str) else int(dtype))


def _tbi(x, time_major):
    """(T, B, I) of a layer's input."""
    return (x.shape[0], x.shape[1], x.shape[2]) if time_major else (x.shape[1], x.shape[0], x.shape[2])


def _needs_tape(x, params, h0=None, c0=None, head=None):
    """Will this call run in training mode (tape kept, reserve buffer allocated)?  Asked of exactly the tensors that reach
    Function.apply as differentiable inputs - input, parameters, initial states, the classifier's weight and bias - so it is what
    any(ctx.needs_input_grad) says inside VmlmfSeqFn / VmlmfStackFn.forward (False under torch.no_grad(): inference kernels)."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, h0, c0, *params, *(head or ())))


# The host caches (_DESC_CACHE, _STACK_CACHE, PackCache) all carry the library's switch generation (vmlmf_tune_generation) in their
# keys: whoever flips a switch - _lib.tune(), a raw vmlmf_tune call, the library itself after a riding worker gave up - is seen
# by the next lookup.
# cfg + (B, T, I, H, training, generation) -> (Desc, Sizes): host-side descriptor cache
_DESC_CACHE = {}
# grow-only scratch buffers, one per (kind, device, stream): the contents never outlive the call that fills them and all calls
# on a stream are serialised.  Kinds stay distinct objects ("layer": workspaces; "embed"; "sample": the two may be live in one
# captured region)
_WORKSPACE = {}


def _desc_for(cfg, B, T, I, H, training):
    key = cfg + (B, T, I, H, training, _lib.lib().vmlmf_tune_generation())
    hit = _DESC_CACHE.get(key)
    if hit is None:
        variant, g, w_rank, u_ranks, time_major, dtype = cfg
        desc = _lib.make_desc(variant, B, T, I, H, w_rank, u_ranks, g=g, time_major=time_major, training=training, dtype=dtype)
        hit = (desc, _lib.query(desc))
        _DESC_CACHE[key] = hit
    return hit


def _workspace(dev, nbytes, kind="layer"):
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(nbytes, device=dev, dtype=torch.uint8)      # graph-private pool
    key = (kind, dev.index, _lib.raw_stream(dev).value)
    buf = _WORKSPACE.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _WORKSPACE[key] = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    return buf


def _head_forward(head_w, head_b, B, dev):
    """A classifier riding on a launch's final hidden state (Net.lin), forward side: (weight, bias, logits, _lib.Head) with weight
    and bias contiguous and the (B, C) logits allocated - or (None, None, an empty tensor, None) without a classifier."""
    if head_w is None:
        return None, None, torch.empty((0,), device=dev, dtype=torch.float32), None
    hw = head_w.contiguous()
    hb = None if head_b is None else head_b.contiguous()
    _require_hip(hw, "head weight")
    logits = torch.empty((B, hw.shape[0]), device=dev, dtype=torch.float32)
    hd = _lib.Head()
    hd.classes, hd.weight, hd.logits = hw.shape[0], hw.data_ptr(), logits.data_ptr()
    hd.bias = None if hb is None else hb.data_ptr()
    return hw, hb, logits, hd


def _flat_grads(params, hw, has_head_b, dlogits):
    """The gradient buffer of a layer or stack backward: (flat, grads, dW, db, _lib.Head or None).

    THE LAYOUT CONTRACT (vmlmf_amd/dp.py reduces `flat` in place; csrc/torch_binding.cpp: flat_grads lays out the same bytes):
    ONE fp32 allocation holds the gradients of `params` in call order, each dense in its parameter's shape, followed - whenever
    the classifier takes part, i.e. there is a head weight `hw` AND a gradient `dlogits` (contiguous) for its logits - by
    dW (C, H), then db (C).  The tail is C * H + C floats with or without a bias; db is a view of it only with one.  grads, dW
    and db are views, so one all-reduce of `flat` exchanges everything the launch produced."""
    total = sum(p.numel() for p in params)
    use_head = hw is not None and dlogits is not None
    flat = torch.empty(total + (hw.numel() + hw.shape[0] if use_head else 0), device=params[0].device, dtype=torch.float32)
    grads, o = [], 0
    for p in params:
        grads.append(flat[o:o + p.numel()].view(p.shape))
        o += p.numel()
    if not use_head:
        return flat, tuple(grads), None, None, None
    C, H = hw.shape
    dW = flat[total:total + C * H].view(C, H)
    db = flat[total + C * H:] if has_head_b else None
    hd = _lib.Head()
    hd.classes, hd.weight, hd.dlogits, hd.dweight = C, hw.data_ptr(), dlogits.data_ptr(), dW.data_ptr()
    hd.dbias = None if db is None else db.data_ptr()
    return flat, tuple(grads), dW, db, hd


class PackCache:
    """Kept parameter images of one layer (C ABI: vmlmf_pack_params / vmlmf_seq_*_packed), opt-in through
    vmlmf_amd.cache_packed_parameters(module).  The library packs the reference-layout parameters into the kernels' register
    images on every forward (6 us of the 185 us headline step); while the parameters are unchanged the images can be
    reused - inference, evaluation, gradient accumulation, a loop without an optimizer step.  "Unchanged" is judged by
    (data_ptr, _version) of every parameter tensor: in-place updates under torch.no_grad() (torch.optim, the reference's
    `param -= lr * grad`, vmlmf_amd.optim) are seen; writes through `param.data` are NOT (they do not bump the version) -
    that is why the cache is opt-in.  During a stream capture the cache is only read, never filled."""
    __slots__ = ("key", "packed", "hits", "fills")

    def __init__(self):
        self.key, self.packed, self.hits, self.fills = None, None, 0, 0

    def get(self, cfg, params, x, B, T, I, H):
        if self.key == "unsupported":
            return None
        key = (cfg, B, I, H, x.device.index, _lib.lib().vmlmf_tune_generation(),
               tuple((p.data_ptr(), p._version) for p in params))
        if key == self.key:
            self.hits += 1
            return self.packed
        if torch.cuda.is_current_stream_capturing():
            return None                       # packed inside the captured call, as without a cache
        variant, g, w_rank, u_ranks, time_major, dtype = cfg
        desc = _lib.make_desc(variant, B, T, I, H, w_rank, u_ranks, g=g, time_major=time_major, training=True, dtype=dtype)
        n = ctypes.c_size_t()
        rc = _lib.lib().vmlmf_pack_bytes(ctypes.byref(desc), ctypes.byref(n))
        if rc == _lib.E_UNSUPPORTED:          # step-wise / clustered layers keep per-call state in their image
            self.key, self.packed = "unsupported", None
            return None
        _lib.check(rc)
        packed = torch.empty(n.value, device=x.device, dtype=torch.uint8)   # a NEW buffer: an earlier forward's backward may still need the old one
        ps = _params_struct(params, g, variant)
        with _lib.on_device(x.device):
            _lib.check(_lib.lib().vmlmf_pack_params(ctypes.byref(desc), ctypes.byref(ps), _ptr(packed), _lib.raw_stream(x.device)))
        self.key, self.packed = key, packed
        self.fills += 1
        return packed


def cache_packed_parameters(module, enable=True):
    """Let every VMLMF layer under `module` keep its packed parameter images between forward calls while its parameters are
    unchanged (see PackCache for what "unchanged" can and cannot see).  Returns the number of layers switched."""
    n = 0
    for m in module.modules():
        if hasattr(m, "kernel_params"):
            m._pack_cache = PackCache() if enable else None
            n += 1
    return n


def _require_hip(t, what):
    if not t.is_cuda:
        raise RuntimeError(
            f"vmlmf_amd: {what} is on {t.device}; the VMLMF hot path runs only as HIP kernels on an MI355X "
            "(no CPU fallback). Move the module and inputs to 'cuda'.")
    if t.dtype != torch.float32:
        raise RuntimeError(f"vmlmf_amd: {what} must be float32, got {t.dtype}")


_TICKET = {}
_TICKET_CAPTURE_SLOTS = 16


def ce_ticket(device):
    """The ticket words of the criterion that rides on the forward launch (include/vmlmf_hip.h: vmlmf_ce.ticket): two zeroed
    int64; every launch leaves them zero.  Launches that share a ticket must be ordered on ONE stream, so the pair is kept per
    (device, stream).  Nothing is allocated inside a stream capture (the allocation would land in the graph's private pool and a
    memset node in the graph): a captured forward takes the next pair of a block of 16 that the first call outside a capture set
    aside for the device, so different graphs - replayed on whatever streams - do not meet on one pair either.  Only a process whose
    very first forward is captured pays a zeroing node in that graph (the pair is then the graph's own and is not kept here)."""
    return _stream_ticket(device, "ce")


def sample_ticket(device):
    """The ticket of the token sampler (vmlmf_lm_sample: the last workgroup to finish merges the others' partials and puts the
    word back to zero), kept by ce_ticket's rules: per (device, stream), nothing allocated inside a stream capture."""
    return _stream_ticket(device, "sample")


def _stream_ticket(device, kind):
    device = torch.device(device)
    capturing = torch.cuda.is_current_stream_capturing()
    block = _TICKET.get((kind, device.index, "capture"))
    if block is None and not capturing:
        block = _TICKET[(kind, device.index, "capture")] = [torch.zeros(2 * _TICKET_CAPTURE_SLOTS, device=device, dtype=torch.int64), 0]
    if capturing:
        if block is None:
            return torch.zeros(2, device=device, dtype=torch.int64)
        i = block[1] % _TICKET_CAPTURE_SLOTS
        block[1] += 1
        return block[0][2 * i:2 * i + 2]
    key = (kind, device.index, _lib.raw_stream(device).value)
    t = _TICKET.get(key)
    if t is None:
        t = _TICKET[key] = torch.zeros(2, device=device, dtype=torch.int64)
    return t


class VmlmfSeqFn(torch.autograd.Function):
    """y, hT, cT, logits, loss = f(x, h0, c0, *params) for one layer.  cfg = (variant, g, w_rank, u_ranks, time_major, dtype).
    target (with a head): mean cross-entropy of the logits against it as the fifth output (vmlmf_ce: inside the same launch)."""

    @staticmethod
    def forward(ctx, cfg, packed, x, h0, c0, head_w, head_b, target, ignore_index, drop, *params):
        variant, g, w_rank, u_ranks, time_major, _ = cfg
        ctx.set_materialize_grads(False)
        _require_hip(x, "input")
        for p in params:
            _require_hip(p, "parameter")
        x = x.contiguous()
        params = tuple(p.contiguous() for p in params)
        T, B, I = _tbi(x, time_major)
        H = _hidden_size(variant, params)
        training = bool(any(ctx.needs_input_grad))   # (what _needs_tape says of this call's tensors)
        ctx.packed = packed                           # kept parameter images (PackCache) or None
        desc, sizes = _desc_for(cfg, B, T, I, H, training)
        dev = x.device
        y = torch.empty((T, B, H) if time_major else (B, T, H), device=dev, dtype=torch.float32)
        hT = torch.empty((B, H), device=dev, dtype=torch.float32)
        cT = torch.empty((B, H), device=dev, dtype=torch.float32)
        ws = _workspace(dev, sizes.workspace_bytes)
        reserve = torch.empty(sizes.reserve_bytes, device=dev, dtype=torch.uint8) if training else None
        h0c = None if h0 is None else h0.contiguous()
        c0c = None if c0 is None else c0.contiguous()
        ps = _params_struct(params, g, variant)
        stream = _lib.raw_stream(dev)
        hw, hb, logits, hd = _head_forward(head_w, head_b, B, dev)   # the riding classifier's logits are the 4th output
        ex = _lib.Extra()
        ex.packed = None if packed is None else packed.data_ptr()
        ex.head = ctypes.pointer(hd) if hd is not None else None
        # the criterion on those logits: loss | nvalid | lse[B] in one allocation, the unit gradient of the logits beside it
        stats = dz_unit = None
        ce = _lib.Ce()
        if target is not None:
            if hw is None:
                raise RuntimeError("vmlmf_amd: a criterion rides on the classifier's logits (head)")
            tg = target.contiguous()
            stats = torch.empty(2 + B, device=dev, dtype=torch.float32)
            dz_unit = torch.empty_like(logits) if training else None
            base = stats.data_ptr()
            ce.target, ce.ignore_index = tg.data_ptr(), int(ignore_index)
            ce.loss, ce.nvalid, ce.lse = base, base + 4, base + 8
            ce.dlogits_unit = None if dz_unit is None else dz_unit.data_ptr()
            ce.ticket = ce_ticket(dev).data_ptr()
            ex.ce = ctypes.pointer(ce)
        # dropout of the layer's output inside its launches (vmlmf_dropout, ABI 11): drop = (p, snapshot, site); the first output is
        # then the DROPPED copy, y itself stays with the backward
        yd = dr = None
        if drop is not None:
            yd = torch.empty_like(y)
            dr = _lib.Dropout(float(drop[0]), site_word(drop), drop[1].data_ptr(), yd.data_ptr())
            ex.drop = ctypes.pointer(dr)
        with _lib.on_device(dev):
            _lib.check(_lib.lib().vmlmf_seq_forward_ex(
                ctypes.byref(desc), ctypes.byref(ps), _ptr(x), _ptr(h0c), _ptr(c0c), _ptr(y), _ptr(hT),
                _ptr(cT), _ptr(reserve), _ptr(ws), sizes.workspace_bytes, stream, ctypes.byref(ex)))
        if training:
            ctx.cfg, ctx.desc, ctx.sizes = cfg, desc, sizes
            ctx.has_h0, ctx.has_c0 = h0 is not None, c0 is not None
            ctx.has_head, ctx.has_head_b = hw is not None, hb is not None
            ctx.has_ce = dz_unit is not None
            ctx.drop = None if drop is None else (float(drop[0]), site_word(drop))
            ctx.save_for_backward(x, y, reserve, *params, *([h0c] if h0 is not None else []),
                                  *([c0c] if c0 is not None else []), *([hw] if hw is not None else []),
                                  *([dz_unit] if dz_unit is not None else []), *([drop[1]] if drop is not None else []))
            ctx.nparams = len(params)
        loss = stats[0] if stats is not None else torch.empty((0,), device=dev, dtype=torch.float32)
        return (y if yd is None else yd), hT, cT, logits, loss

    @staticmethod
    def backward(ctx, dy, dhT, dcT, dlogits, dloss):
        variant, g, w_rank, u_ranks, time_major, _ = ctx.cfg
        saved = ctx.saved_tensors
        x, y, reserve = saved[0], saved[1], saved[2]
        params = saved[3:3 + ctx.nparams]
        rest = list(saved[3 + ctx.nparams:])
        h0 = rest.pop(0) if ctx.has_h0 else None
        c0 = rest.pop(0) if ctx.has_c0 else None
        hw = rest.pop(0) if ctx.has_head else None
        dz = rest.pop(0) if ctx.has_ce else None   # (popped whether or not the loss takes part: what follows it is the dropout snapshot)
        if dz is not None and dloss is not None:
            # the criterion's share of d(logits): what the forward launch wrote for d(loss) = 1 - as it is when the incoming
            # gradient IS the package's constant one (vmlmf_amd.unit_gradient), scaled otherwise
            if not _is_unit(dloss):
                dz = dz * dloss
            dlogits = dz if dlogits is None else dlogits + dz
        snap = rest.pop(0) if ctx.drop is not None else None
        dev = x.device
        desc, sizes = ctx.desc, ctx.sizes
        dy = None if dy is None else dy.contiguous()
        dhT = None if dhT is None else dhT.contiguous()
        dcT = None if dcT is None else dcT.contiguous()
        dlogits = None if dlogits is None else dlogits.contiguous()
        need_dx = ctx.needs_input_grad[2]   # (cfg, packed, x, h0, c0, head_w, head_b, target, ignore_index, drop, *params)
        dx = torch.empty_like(x) if need_dx else None
        B, H = y.shape[1 if time_major else 0], y.shape[2]
        dh0 = torch.empty((B, H), device=dev, dtype=torch.float32) if ctx.has_h0 else None
        dc0 = torch.empty((B, H), device=dev, dtype=torch.float32) if ctx.has_c0 else None
        flat, grads, dW, db, hd = _flat_grads(params, hw, ctx.has_head_b, dlogits)
        ws = _workspace(dev, sizes.workspace_bytes)
        ps = _params_struct(params, g, variant)
        gs = _params_struct(grads, g, variant)
        stream = _lib.raw_stream(dev)
        ex = _lib.Extra()
        ex.packed = None if ctx.packed is None else ctx.packed.data_ptr()
        ex.head = ctypes.pointer(hd) if hd is not None else None
        if snap is not None:   # dy is the gradient of the dropped copy: the launch regenerates the forward's factors
            dr = _lib.Dropout(ctx.drop[0], ctx.drop[1], snap.data_ptr(), None)
            ex.drop = ctypes.pointer(dr)
        with _lib.on_device(dev):
            _lib.check(_lib.lib().vmlmf_seq_backward_ex(
                ctypes.byref(desc), ctypes.byref(ps), _ptr(x), _ptr(h0), _ptr(c0), _ptr(y), _ptr(reserve),
                _ptr(dy), _ptr(dhT), _ptr(dcT), _ptr(dx), _ptr(dh0), _ptr(dc0), ctypes.byref(gs),
                _ptr(ws), sizes.workspace_bytes, stream, ctypes.byref(ex)))
        return (None, None, dx, dh0, dc0, dW, db, None, None, None) + grads


def vmlmf_sequence(variant, x, h0, c0, params, w_rank, u_ranks, g=1, time_major=False, dtype="f32", pack_cache=None,
                   head=None, target=None, ignore_index=-100, drop=None):
    """Run one VMLMF layer over a whole sequence on the GPU.

    params: tensors in the order dia_x, dia_h, u_x, v_x, b_x, b_h, u_h[0], v_h[0] (, u_h[1], v_h[1]),
    each in the reference's layout (the cells without vm: see the table at the top of this file).
    dtype: "f32" (the reference's arithmetic) or "bf16" (bf16 MFMA with fp32 accumulation and state, bf16 tapes; all
    tensors stay float32 - include/vmlmf_hip.h: vmlmf_desc.dtype).  Returns (y, hT, cT).
    head: (weight (C, H), bias (C) or None) of a classifier on the layer's final hidden state (Net.lin); the call then
    returns (y, hT, cT, logits) and neither the logits nor their backward cost a launch of their own on the VALU kernels.
    target (with head): (B,) int64 class indices - the mean cross-entropy of the logits against them (nn.CrossEntropyLoss() with
    default arguments, train.py:58-65) comes back as a fifth element, formed inside the same forward launch.
    drop: (p, snapshot, site) - nn.Dropout(p) behind the layer (vmlmf_lm.py:438-439) without a mask tensor: the returned y is the
    dropped activation; inside the layer's own launches where the library takes it (vmlmf_dropout_fused: the row-block kernels,
    time-major), one launch of the package's otherwise (dropout()).  Not together with a head.  (p, snapshot, site, True): the
    LOCKED form of that dropout - one (B, H) mask for every time step (docs/design/lm_locked.md) - in the same launches.
    """
    cfg = _layer_cfg(variant, g, w_rank, u_ranks, time_major, dtype)
    hw, hb = (None, None) if head is None else head
    if drop is not None and head is not None:
        raise RuntimeError("vmlmf_amd: dropout behind a layer and a classifier riding on it do not combine")
    if x.is_cuda and (drop is not None or pack_cache is not None):
        (T, B, I), H = _tbi(x, cfg[4]), _hidden_size(variant, params)
    if drop is not None and x.is_cuda:      # in-launch dropout: the ctypes class, where the library takes it
        desc, _ = _desc_for(cfg, B, T, I, H, _needs_tape(x, params, h0, c0))
        if _lib.lib().vmlmf_dropout_fused(ctypes.byref(desc)) == 1:
            return VmlmfSeqFn.apply(cfg, None, x, h0, c0, None, None, None, ignore_index, tuple(drop), *params)[:3]
    packed = pack_cache.get(cfg, params, x, B, T, I, H) if pack_cache is not None and x.is_cuda else None
    ops = torch_ops()
    if ops is None:
        out = VmlmfSeqFn.apply(cfg, packed, x, h0, c0, hw, hb, target, ignore_index, None, *params)
    elif target is not None:
        out = ops.sequence_loss(x, h0, c0, list(params), variant, g, cfg[2], list(cfg[3]), cfg[4], cfg[5], packed, hw, hb, target,
                                int(ignore_index), unit_gradient(x.device), ce_ticket(x.device))
    else:
        out = ops.sequence(x, h0, c0, list(params), variant, g, cfg[2], list(cfg[3]), cfg[4], cfg[5], packed, hw, hb)
    if drop is not None:                    # ... and as one launch of the package's behind the layer otherwise
        if drop_locked(drop) and not cfg[4]:                            # (a locked mask is laid over time-major rows)
            return dropout(out[0].transpose(0, 1), drop[0], drop[1], drop[2], locked=True).transpose(0, 1), out[1], out[2]
        return dropout(out[0], drop[0], drop[1], drop[2], locked=drop_locked(drop)), out[1], out[2]
    return out[:3 if head is None else 4 if target is None else 5]


def locked_site(site):
    """`site` with VMLMF_SITE_LOCKED (bit 31) set: the locked (variational) dropout of that site - one (B, H) mask shared by every
    time step (docs/design/lm_locked.md) - for activation_regularizer(site=), the one place of this module that takes the flag in
    the site itself as the C ABI does; dropout(), embedding_dropout() and the layers' drop tuples say `locked`."""
    return int(site) | (1 << 31)


def drop_locked(drop):
    """Is a layer's drop tuple - (p, snapshot, site) or (p, snapshot, site, locked) - the locked form?"""
    return len(drop) > 3 and bool(drop[3])


def site_word(drop):
    """The site of a drop tuple as the C ABI's vmlmf_dropout.site takes it: VMLMF_SITE_LOCKED (bit 31) set for the locked form."""
    return int(drop[2]) + (_lib.SITE_LOCKED if drop_locked(drop) else 0)


# ---- stacked layers: one wavefront launch per direction (C ABI 7: vmlmf_stack_*) ----------------------------------------
# (cfg, L, B, T, I, H, training) -> None (not covered: chain the per-layer calls) or (descs, reserve bytes, workspace bytes)
_STACK_CACHE = {}


def _stack_plan(cfg, L, B, T, I, H, training):
    """H: the layers' hidden size, or one per layer (round 6: MyLSTM builds any hidden_layer_sizes, vmlmf.py:283-292)."""
    Hs = tuple(H) if isinstance(H, (list, tuple)) else (int(H),) * L
    key = (cfg, L, B, T, I, Hs, training, _lib.lib().vmlmf_tune_generation())
    if key in _STACK_CACHE:
        return _STACK_CACHE[key]
    variant, g, w_rank, u_ranks, time_major, dtype = cfg
    plan = None
    if 1 <= L <= _lib.STACK_MAX and g in (1, 2) and dtype in (_lib.DT_F32, _lib.DT_BF16):
        layers = (_lib.StackLayer * L)()
        descs = []
        for l in range(L):
            d = _lib.make_desc(variant, B, T, I if l == 0 else Hs[l - 1], Hs[l], w_rank, u_ranks, g=g, time_major=time_major,
                               training=training, dtype=dtype)
            layers[l].desc = d
            descs.append(d)
        rb = (ctypes.c_size_t * L)()
        wb = ctypes.c_size_t()
        rc = _lib.lib().vmlmf_stack_query(L, ctypes.addressof(layers), ctypes.addressof(rb), ctypes.addressof(wb))
        if rc == 0:
            plan = (descs, [int(v) for v in rb], int(wb.value))
        elif rc not in (_lib.E_UNSUPPORTED, _lib.E_SHAPE):
            _lib.check(rc)
    _STACK_CACHE[key] = plan
    return plan


def stack_takes_dropout(cfg, L, B, T, I, H, training):
    """Does the stack run in the clustered form (include/vmlmf_hip.h: vmlmf_stack_dropout_fused), whose launches apply the dropout
    between the layers themselves?"""
    plan = _stack_plan(cfg, L, B, T, I, H, training)
    if plan is None:
        return False
    layers = (_lib.StackLayer * L)()
    for l in range(L):
        layers[l].desc = plan[0][l]
    return _lib.lib().vmlmf_stack_dropout_fused(L, ctypes.addressof(layers)) == 1


class VmlmfStackFn(torch.autograd.Function):
    """y_top, hT_0 .. hT_{L-1}, cT_0 .. cT_{L-1} = f(x, params of layer 0, ..., params of layer L-1): every layer of a stack in
    one launch per direction (include/vmlmf_hip.h: vmlmf_stack_forward / vmlmf_stack_backward).  Initial states are zero
    (MyLSTM.forward, vmlmf.py:296-298)."""

    @staticmethod
    def forward(ctx, cfg, L, x, head_w, head_b, h0, c0, drops, *params):
        # drops: None, or one entry per layer - None / (p, snapshot, site): nn.Dropout(p) behind that layer inside the stack's launches
        # (the clustered form only: vmlmf_stack_dropout_fused); the first output is then the top layer's DROPPED copy
        variant, g, w_rank, u_ranks, time_major, _ = cfg
        ctx.set_materialize_grads(False)
        _require_hip(x, "input")
        x = x.contiguous()
        params = tuple(p.contiguous() for p in params)
        nper = len(params) // L
        T, B, I = _tbi(x, time_major)
        Hs = tuple(_hidden_size(variant, params[l * nper:(l + 1) * nper]) for l in range(L))
        training = bool(any(ctx.needs_input_grad))   # (what _needs_tape said when vmlmf_stack looked the plan up)
        plan = _stack_plan(cfg, L, B, T, I, Hs, training)
        if plan is None:
            raise RuntimeError("vmlmf_amd: this stack is not covered by the wavefront kernels (vmlmf_stack_supported)")
        descs, rbytes, wbytes = plan
        dev = x.device
        ys = [torch.empty((T, B, Hs[l]) if time_major else (B, T, Hs[l]), device=dev, dtype=torch.float32) for l in range(L)]
        # final states of every layer: one allocation when the layers are alike (what the LM carries), one per layer otherwise
        hc = [torch.empty((2, B, Hs[l]), device=dev, dtype=torch.float32) for l in range(L)] if len(set(Hs)) > 1 else \
            list(torch.empty((L, 2, B, Hs[0]), device=dev, dtype=torch.float32).unbind(0))
        reserves = [torch.empty(rbytes[l], device=dev, dtype=torch.uint8) if training else None for l in range(L)]
        ws = _workspace(dev, wbytes)
        h0c = None if h0 is None else h0.contiguous()      # initial states of every layer, (L, B, H), or None = zeros
        c0c = None if c0 is None else c0.contiguous()
        layers = (_lib.StackLayer * L)()
        keep = []
        yds = [None] * L
        for l in range(L):
            ps = _params_struct(params[l * nper:(l + 1) * nper], g, variant)
            keep.append(ps)
            ly = layers[l]
            ly.desc, ly.params = descs[l], ctypes.pointer(ps)
            if drops is not None and drops[l] is not None:
                yds[l] = torch.empty_like(ys[l])
                dr = _lib.Dropout(float(drops[l][0]), site_word(drops[l]), drops[l][1].data_ptr(), yds[l].data_ptr())
                keep.append(dr)
                ly.drop = ctypes.pointer(dr)
            ly.y, ly.hT, ly.cT = ys[l].data_ptr(), hc[l][0].data_ptr(), hc[l][1].data_ptr()
            ly.reserve = None if reserves[l] is None else reserves[l].data_ptr()
            ly.h0 = None if h0c is None else h0c[l].data_ptr()
            ly.c0 = None if c0c is None else c0c[l].data_ptr()
        hw, hb, logits, hd = _head_forward(head_w, head_b, B, dev)   # riding on the top layer: its logits are the last output
        with _lib.on_device(dev):
            _lib.check(_lib.lib().vmlmf_stack_forward(L, ctypes.addressof(layers), x.data_ptr(),
                                                      None if hd is None else ctypes.addressof(hd), ws.data_ptr(), wbytes,
                                                      _lib.raw_stream(dev)))
        if training:
            ctx.cfg, ctx.L, ctx.nper, ctx.plan = cfg, L, nper, plan
            ctx.has_head, ctx.has_head_b = hw is not None, hb is not None
            ctx.has_h0, ctx.has_c0 = h0c is not None, c0c is not None
            ctx.drops = None if drops is None else [None if d is None else (float(d[0]), site_word(d)) for d in drops]
            dsaved = [] if drops is None else [t for l in range(L) if drops[l] is not None for t in (yds[l], drops[l][1])]
            ctx.save_for_backward(x, *ys, *reserves, *params, *([hw] if hw is not None else []),
                                  *([h0c] if h0c is not None else []), *([c0c] if c0c is not None else []), *dsaved)
        top = ys[-1] if yds[-1] is None else yds[-1]
        return (top,) + tuple(hc[l][0] for l in range(L)) + tuple(hc[l][1] for l in range(L)) + (logits,)

    @staticmethod
    def backward(ctx, dy, *dstates):
        variant, g, w_rank, u_ranks, time_major, _ = ctx.cfg
        L, nper = ctx.L, ctx.nper
        descs, rbytes, wbytes = ctx.plan
        saved = ctx.saved_tensors
        x, ys, reserves, params = saved[0], saved[1:1 + L], saved[1 + L:1 + 2 * L], list(saved[1 + 2 * L:])
        dsaved = {}
        if ctx.drops is not None:     # (dropped copy, snapshot) of every layer with a dropout, saved behind everything else
            for l in reversed(range(L)):
                if ctx.drops[l] is not None:
                    snap = params.pop()
                    yd = params.pop()
                    dsaved[l] = (yd, snap)
        c0 = params.pop() if ctx.has_c0 else None
        h0 = params.pop() if ctx.has_h0 else None
        hw = params.pop() if ctx.has_head else None
        dlogits = None if dstates[2 * L] is None else dstates[2 * L].contiguous()
        dev = x.device
        dy = None if dy is None else dy.contiguous()
        dhT = [None if d is None else d.contiguous() for d in dstates[:L]]
        dcT = [None if d is None else d.contiguous() for d in dstates[L:2 * L]]
        need_dx = ctx.needs_input_grad[2]
        dx = torch.empty_like(x) if need_dx else None
        flat, grads, dW, db, hd = _flat_grads(params, hw, ctx.has_head_b, dlogits)   # the whole stack's and the classifier's
        ws = _workspace(dev, wbytes)
        B, H = ys[0].shape[1 if time_major else 0], ys[0].shape[2]
        dh0 = torch.empty((L, B, H), device=dev, dtype=torch.float32) if ctx.has_h0 else None
        dc0 = torch.empty((L, B, H), device=dev, dtype=torch.float32) if ctx.has_c0 else None
        layers = (_lib.StackLayer * L)()
        keep = []
        for l in range(L):
            ps = _params_struct(params[l * nper:(l + 1) * nper], g, variant)
            gs = _params_struct(grads[l * nper:(l + 1) * nper], g, variant)
            keep += [ps, gs]
            ly = layers[l]
            ly.desc, ly.params, ly.grads = descs[l], ctypes.pointer(ps), ctypes.pointer(gs)
            if l in dsaved:   # the launch regenerates the forward's factors; the layer above's weight gradients read the dropped copy
                dr = _lib.Dropout(ctx.drops[l][0], ctx.drops[l][1], dsaved[l][1].data_ptr(), dsaved[l][0].data_ptr())
                keep.append(dr)
                ly.drop = ctypes.pointer(dr)
            ly.y, ly.reserve = ys[l].data_ptr(), reserves[l].data_ptr()
            ly.h0 = None if h0 is None else h0[l].data_ptr()
            ly.c0 = None if c0 is None else c0[l].data_ptr()
            ly.dh0 = None if dh0 is None else dh0[l].data_ptr()
            ly.dc0 = None if dc0 is None else dc0[l].data_ptr()
            ly.dhT = None if dhT[l] is None else dhT[l].data_ptr()
            ly.dcT = None if dcT[l] is None else dcT[l].data_ptr()
        with _lib.on_device(dev):
            _lib.check(_lib.lib().vmlmf_stack_backward(L, ctypes.addressof(layers), x.data_ptr(), _ptr(dy), _ptr(dx),
                                                       None if hd is None else ctypes.addressof(hd), ws.data_ptr(), wbytes,
                                                       _lib.raw_stream(dev)))
        return (None, None, dx, dW, db, dh0, dc0, None) + grads


def stack_mode():
    """VMLMF_STACK: "auto" (default: every covered stack of two or more layers - measured faster than the chained kernels
    from B = 64 to 2048, profiles/r02_stack_vs_chained_over_batch.txt; a single layer only when its input is wider than 16,
    i.e. when its x-projection would otherwise be a launch of its own, and T <= 96), "0" (never: chain the per-layer
    calls), "1" (whenever the wavefront kernels cover the stack)."""
    import os
    return os.environ.get("VMLMF_STACK", "auto")


def vmlmf_stack(variant, x, layer_params, w_rank, u_ranks, g=1, time_major=False, dtype="f32", head=None, h0=None, c0=None, drops=None):
    """Run a stack of VMLMF layers (zero initial states) in one wavefront launch per direction.  layer_params: one parameter
    tuple per layer, in vmlmf_sequence's order.  Returns (y of the top layer, [hT per layer], [cT per layer]) or None when
    the stack is not covered / not worth it (the caller then chains vmlmf_sequence calls).  head: (weight (C, H), bias or
    None) of a classifier on the top layer's final hidden state (<= 32 classes): a fourth element, its logits, is returned.
    h0 / c0: initial states of every layer as (L, B, H) tensors (None = zeros, MyLSTM.forward; the LM network carries them
    from batch to batch, vmlmf_lm.py:421-439)."""
    mode = stack_mode()
    L = len(layer_params)
    if mode == "0" or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 3:
        return None
    cfg = _layer_cfg(variant, g, w_rank, u_ranks, time_major, dtype)
    T, B, I = _tbi(x, cfg[4])
    Hs = tuple(_hidden_size(variant, ps) for ps in layer_params)
    H = Hs[0]
    if len(set(Hs)) > 1:
        if h0 is not None or c0 is not None or drops is not None:
            return None     # (carried states / dropout: the LM's stacks, whose layers are alike)
        H = Hs
    xwave = I <= 16 and Hs[0] <= 192 and g == 1       # (vg_xwave_ok of the C side: <= 3 waves of units, one group)
    if mode != "1" and L == 1 and (xwave or T > 96):
        return None          # (a single layer with a narrow input already forms its x side inside the recurrent kernel; with a wide
                             #  one the x-team's per-step cost overtakes the two launches it saves at T ~ 128:
                             #  profiles/r02_stack_vs_chained_over_T.txt)
    # (the classifier's weight and bias count: with a frozen RNN under a trainable head the launch runs in training mode, and the
    #  coverage check must be made for that mode - otherwise an uncovered stack raised instead of falling back to chained layers)
    flat = [p for ps in layer_params for p in ps]
    training = _needs_tape(x, flat, h0, c0, head)
    if _stack_plan(cfg, L, B, T, I, H, training) is None:
        return None
    if drops is not None and any(d is not None for d in drops):
        # drops: per layer None / (p, snapshot, site) - only the clustered form applies dropout inside its launches
        if not stack_takes_dropout(cfg, L, B, T, I, H, training):
            return None
    else:
        drops = None
    hw, hb = (None, None) if head is None else head
    ops = torch_ops()
    if ops is not None and h0 is None and c0 is None and cfg[5] == _lib.DT_F32 and drops is None and len(set(Hs)) == 1:      # (initial states, the bf16 tape, dropout, unequal sizes: the ctypes form below)
        y, hT, cT, logits = ops.stack(x, flat, L, variant, cfg[2], list(cfg[3]), int(g), cfg[4], hw, hb)
        out = (y, list(hT.unbind(0)), list(cT.unbind(0)))
        return out + (logits,) if head is not None else out
    res = VmlmfStackFn.apply(cfg, L, x, hw, hb, h0, c0, drops, *flat)
    out = (res[0], list(res[1:1 + L]), list(res[1 + L:1 + 2 * L]))
    return out + (res[1 + 2 * L],) if head is not None else out


class HeadLinearFn(torch.autograd.Function):
    """logits = h @ W^T + bias for the classifier on the last timestep (Net.lin, V/src/models/vmlmf.py:345,
    353-355): two latency-sized kernels instead of three library GEMM launches and a bias-gradient reduction."""

    @staticmethod
    def forward(ctx, h, weight, bias):
        ctx.set_materialize_grads(False)
        _require_hip(h, "head input")
        _require_hip(weight, "head weight")
        if h.stride(-1) != 1:
            h = h.contiguous()
        weight = weight.contiguous()
        bias_c = None if bias is None else bias.contiguous()
        B, H = h.shape
        C = weight.shape[0]
        out = torch.empty((B, C), device=h.device, dtype=torch.float32)
        stream = _lib.raw_stream(h.device)
        with _lib.on_device(h.device):
            _lib.check(_lib.lib().vmlmf_head_forward(B, H, C, _ptr(h), h.stride(0), _ptr(weight), _ptr(bias_c),
                                                     _ptr(out), stream))
        ctx.save_for_backward(h, weight)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, dl):
        if dl is None:
            return None, None, None
        h, weight = ctx.saved_tensors
        dl = dl.contiguous()
        B, H = h.shape
        C = weight.shape[0]
        need_h, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        dh = torch.empty((B, H), device=h.device, dtype=torch.float32) if need_h else None
        # weight and bias gradients share one allocation (contiguous for the data-parallel all-reduce)
        flat = torch.empty(C * H + C, device=h.device, dtype=torch.float32) if (need_w or need_b) else None
        dW = flat[:C * H].view(C, H) if need_w else None
        db = flat[C * H:] if need_b else None
        stream = _lib.raw_stream(h.device)
        with _lib.on_device(h.device):
            _lib.check(_lib.lib().vmlmf_head_backward(B, H, C, _ptr(h), h.stride(0), _ptr(weight), _ptr(dl),
                                                      _ptr(dh), _ptr(dW), _ptr(db), stream))
        return dh, dW, db


def set_compute_dtype(module, dtype):
    """Select the arithmetic of every VMLMF layer under `module`: "f32" (default, the reference's) or "bf16" (bf16 MFMA in
    the recurrence with fp32 accumulation and state, bf16 tapes; BASELINE configs[2]).  Parameters, inputs, outputs and
    gradients stay float32 tensors either way; a layer the bf16 kernels do not cover raises when it is run."""
    if dtype not in _lib.DTYPES:
        raise ValueError(f"dtype must be one of {sorted(_lib.DTYPES)}")
    n = 0
    for m in module.modules():
        if hasattr(m, "kernel_params"):
            m.compute_dtype = dtype
            n += 1
    return n


def head_linear(h, weight, bias):
    """nn.Linear on (B, H) rows through the head kernels when they apply (HIP fp32, <= 32 classes); the stock
    library op otherwise (it is not part of the VMLMF path and has no CPU restriction of its own)."""
    if (h.is_cuda and h.dim() == 2 and h.dtype == torch.float32 and weight.dtype == torch.float32
            and weight.shape[0] <= _lib.HEAD_MAX_CLASSES):
        ops = torch_ops()
        if ops is not None:
            return ops.head_linear(h, weight, bias)
        return HeadLinearFn.apply(h, weight, bias)
    return torch.nn.functional.linear(h, weight, bias)


_UNIT = {}


def _is_unit(dloss):
    """Is this incoming gradient the package's constant one (unit_gradient) - the very tensor, not an equal value?"""
    unit = _UNIT.get(dloss.device)
    return unit is not None and dloss.data_ptr() == unit.data_ptr()


def unit_gradient(device):
    """The constant 1.0 as a 0-d fp32 tensor on `device`, one object per device, never written.  `loss.backward()` makes
    autograd fill a fresh ones_like(loss) in every step; `loss.backward(vmlmf_amd.unit_gradient(loss.device))` is the
    same gradient without that launch, and the fused criteria recognise this very tensor as "scale 1" and return
    the gradient their forward kernel already wrote instead of launching a backward kernel."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    t = _UNIT.get(device)
    if t is None:
        t = torch.ones((), device=device, dtype=torch.float32)
        _UNIT[device] = t
    return t


class CrossEntropyFn(torch.autograd.Function):
    """Mean cross-entropy of (B, C) logits against int64 targets, forward and backward in one launch each (and no
    backward launch at all when the incoming gradient is unit_gradient(device))."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index):
        _require_hip(logits, "logits")
        logits = logits.contiguous()
        target = target.contiguous()
        B, C = logits.shape
        dev = logits.device
        stats = torch.empty(B + 2, device=dev, dtype=torch.float32)     # loss | nvalid | lse[B]
        dz_unit = torch.empty_like(logits) if ctx.needs_input_grad[0] else None
        stream = _lib.raw_stream(dev)
        with _lib.on_device(dev):
            _lib.check(_lib.lib().vmlmf_ce_forward(B, C, _ptr(logits), _ptr(target), int(ignore_index),
                                                   stats.data_ptr(), stats.data_ptr() + 8, stats.data_ptr() + 4,
                                                   _ptr(dz_unit), stream))
        ctx.save_for_backward(logits, target, stats, *([dz_unit] if dz_unit is not None else []))
        ctx.ignore_index = int(ignore_index)
        ctx.leaf_logits = logits.grad_fn is None
        return stats[0]

    @staticmethod
    def backward(ctx, dloss):
        logits, target, stats = ctx.saved_tensors[:3]
        if _is_unit(dloss) and len(ctx.saved_tensors) == 4:
            # d(loss) is the package's constant one: forward wrote this.  Logits produced by another node (the classifier
            # head) just pass it on.  When the logits are a LEAF, AccumulateGrad adopts what it is handed as .grad (views
            # included), and in-place work on that gradient (zero_grad(set_to_none=False), clip_grad_norm_, a further
            # backward through a retained graph) would then write into the saved buffer: such callers get a copy.
            dz = ctx.saved_tensors[3]
            return (dz.clone() if ctx.leaf_logits else dz), None, None
        B, C = logits.shape
        dloss = dloss.contiguous()
        dz = torch.empty_like(logits)
        stream = _lib.raw_stream(logits.device)
        with _lib.on_device(logits.device):
            _lib.check(_lib.lib().vmlmf_ce_backward(B, C, _ptr(logits), _ptr(target), ctx.ignore_index,
                                                    stats.data_ptr() + 8, stats.data_ptr() + 4, _ptr(dloss),
                                                    _ptr(dz), stream))
        return dz, None, None


def cross_entropy(input, target, ignore_index=-100):
    """Drop-in for torch.nn.functional.cross_entropy(input, target) with the default arguments (mean reduction,
    class-index targets, no weights, no label smoothing) — the criterion of the reference's training loop
    (V/src/train_test/train.py:58-65).  Classifier-sized (B, C) fp32 logits on a HIP device take the fused
    kernels; anything else goes to the library op."""
    if (input.is_cuda and input.dim() == 2 and input.dtype == torch.float32 and target.dtype == torch.int64
            and target.dim() == 1 and input.numel() <= 65536):
        ops = torch_ops()
        if ops is not None:
            return ops.cross_entropy(input, target, int(ignore_index), unit_gradient(input.device))
        return CrossEntropyFn.apply(input, target, ignore_index)
    return torch.nn.functional.cross_entropy(input, target, ignore_index=ignore_index)


class CrossEntropyLoss(torch.nn.Module):
    """nn.CrossEntropyLoss() with default arguments, on the fused kernels (see cross_entropy)."""

    def __init__(self, ignore_index=-100):
        super().__init__()
        self.ignore_index = ignore_index

    def forward(self, input, target):
        return cross_entropy(input, target, self.ignore_index)


class NllLossFn(torch.autograd.Function):
    """loss = mean over rows of -log softmax(scores)[row, y[row]] * batch_size (lm_test.py:140-153), one read of
    `scores` forward, one read and one write backward."""

    @staticmethod
    def forward(ctx, scores, y, batch_size):
        ctx.set_materialize_grads(False)
        _require_hip(scores, "scores")
        scores = scores.contiguous()
        yrow = y.reshape(-1).contiguous()
        R, V = scores.shape
        scale = float(batch_size) / float(R)
        stats = torch.empty(1 + 2 * R, device=scores.device, dtype=torch.float32)   # loss | lse | rowloss
        stream = _lib.raw_stream(scores.device)
        base = stats.data_ptr()
        with _lib.on_device(scores.device):
            _lib.check(_lib.lib().vmlmf_nll_forward(R, V, _ptr(scores), _ptr(yrow), scale, base, base + 4,
                                                    base + 4 * (1 + R), stream))
        ctx.save_for_backward(scores, yrow, stats)
        ctx.scale = scale
        return stats[0]

    @staticmethod
    def backward(ctx, dloss):
        if dloss is None:
            return None, None, None
        scores, yrow, stats = ctx.saved_tensors
        R, V = scores.shape
        dloss = dloss.contiguous()
        dz = torch.empty_like(scores)
        stream = _lib.raw_stream(scores.device)
        with _lib.on_device(scores.device):
            _lib.check(_lib.lib().vmlmf_nll_backward(R, V, _ptr(scores), _ptr(yrow), ctx.scale, stats.data_ptr() + 4,
                                                     _ptr(dloss), _ptr(dz), stream))
        return dz, None, None


def nll_loss(scores, y):
    """Drop-in for the reference's language-model loss `nll_loss(scores, y)` (V/src/train_test/lm_test.py:140-153):
    scores (T*B, V) fp32, y (T, B) int64 -> scalar, scaled by batch_size as there.  On a HIP device the fused
    kernels run (stable around the row maximum: where the reference's plain exp overflows, this does not);
    CPU tensors take the reference's own formulation in stock ops."""
    batch_size = y.size(1)
    if scores.is_cuda and scores.dim() == 2 and scores.dtype == torch.float32 and y.dtype == torch.int64:
        return NllLossFn.apply(scores, y, batch_size)
    expscores = scores.exp()
    probabilities = expscores / expscores.sum(1, keepdim=True)
    answerprobs = probabilities[range(len(y.reshape(-1))), y.reshape(-1)]
    return torch.mean(-torch.log(answerprobs) * batch_size)


class LinearNllFn(torch.autograd.Function):
    """Vocabulary projection + log-softmax + NLL of the LM loop (Linear, vmlmf_lm.py:355-358; nll_loss, lm_test.py:140-153)
    WITHOUT the (T*B, V) score tensor in HBM: the rows are cut into chunks whose scores (chunk x V) live in one reused buffer
    that stays in the memory-side cache; every chunk is one library GEMM + the fused NLL kernel.  The backward recomputes a
    chunk's scores (a fourth GEMM-sized product) before it forms dscores, dh and accumulates dW, db.
    Measured at config E's shape (tools/bench_lm_head.py, profiles/r03_lm_head_fusion.jsonl): the forward alone is faster than
    GEMM + loss over the full tensor; forward + backward is slower (the recomputed product costs more than the three round
    trips of 358 MB it saves) - so vmlmf_amd.linear_nll takes this path only when no gradient is needed."""

    @staticmethod
    def forward(ctx, h, w, b, y, chunk_rows):
        _require_hip(h, "h")
        h2 = h.reshape(-1, h.shape[-1]).contiguous()
        R, V = h2.shape[0], w.shape[0]
        batch_size = y.size(1)
        yrow = y.reshape(-1).contiguous()
        scale = float(batch_size) / float(R)
        C = min(int(chunk_rows), R)
        buf = torch.empty((C, V), device=h.device, dtype=torch.float32)
        stats = torch.empty(1 + 2 * R, device=h.device, dtype=torch.float32)       # (chunk loss) | lse | rowloss
        losses = torch.empty((R + C - 1) // C, device=h.device, dtype=torch.float32)
        stream = _lib.raw_stream(h.device)
        lib = _lib.lib()
        with _lib.on_device(h.device):
            for ci, r0 in enumerate(range(0, R, C)):
                n = min(C, R - r0)
                sc = buf[:n]
                torch.addmm(b, h2[r0:r0 + n], w.t(), out=sc)
                _lib.check(lib.vmlmf_nll_forward(n, V, _ptr(sc), yrow.data_ptr() + 8 * r0, scale, losses.data_ptr() + 4 * ci,
                                                 stats.data_ptr() + 4 * (1 + r0), stats.data_ptr() + 4 * (1 + R + r0), stream))
        ctx.save_for_backward(h2, w, b, yrow, stats)
        ctx.scale, ctx.C, ctx.hshape = scale, C, h.shape
        return losses.sum()

    @staticmethod
    def backward(ctx, dloss):
        h2, w, b, yrow, stats = ctx.saved_tensors
        R, V, C = h2.shape[0], w.shape[0], ctx.C
        dloss = dloss.contiguous()
        buf = torch.empty((C, V), device=h2.device, dtype=torch.float32)
        dzb = torch.empty((C, V), device=h2.device, dtype=torch.float32)
        dh = torch.empty_like(h2)
        dw = torch.zeros_like(w)
        db = torch.zeros_like(b)
        stream = _lib.raw_stream(h2.device)
        lib = _lib.lib()
        with _lib.on_device(h2.device):
            for r0 in range(0, R, C):
                n = min(C, R - r0)
                sc, dz = buf[:n], dzb[:n]
                torch.addmm(b, h2[r0:r0 + n], w.t(), out=sc)                     # the scores again
                _lib.check(lib.vmlmf_nll_backward(n, V, _ptr(sc), yrow.data_ptr() + 8 * r0, ctx.scale,
                                                  stats.data_ptr() + 4 * (1 + r0), _ptr(dloss), _ptr(dz), stream))
                torch.mm(dz, w, out=dh[r0:r0 + n])
                dw.addmm_(dz.t(), h2[r0:r0 + n])
                db.add_(dz.sum(0))
        return dh.view(ctx.hshape), dw, db, None, None


# ---- the LM head for TRAINING: projection + loss with the gradient of the scores formed in place -------------------------------
# (verdict r3 item 5.)  scores = h W^T is one library GEMM (fp32: rocBLAS / hipBLASLt run it at 120-140 TFLOP/s, 0.77-0.9 of the
# fp32 matrix peak - profiles/r03_lm_head_fusion.jsonl: a hand-written kernel would have to match that to pay); everything
# between the three GEMMs is this package's: vmlmf_nll_forward_grad adds the bias, takes the loss and overwrites the scores
# with their own gradient in ONE pass (the bias gradient falls out as column sums), so the backward's two GEMMs read the
# gradient where the forward left it - no second 358 MB matrix, no separate bias reduction, no backward loss kernel.
# Which library and which operand layout serves each of the three products best differs by 10-25 % (tools/experiments/
# gemm_probe.py: dW as dz^T h runs at 96-104 TFLOP/s, as (h^T dz)^T at 119 on rocBLAS); the forms are timed once per shape on the
# device and the fastest is kept (VMLMF_HEAD_TUNE=0: the first form of each list).
_HEAD_FORMS = {}


def _blas_libs():
    libs = [None]
    if hasattr(torch.backends.cuda, "preferred_blas_library"):
        libs += ["hipblaslt", "cublas"]          # ("cublas" is rocBLAS on ROCm)
    return libs


class _with_blas:
    def __init__(self, lib):
        self.lib, self.prev = lib, None

    def __enter__(self):
        if self.lib is not None:
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                self.prev = torch.backends.cuda.preferred_blas_library()
                torch.backends.cuda.preferred_blas_library(self.lib)

    def __exit__(self, *exc):
        if self.prev is not None:
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                torch.backends.cuda.preferred_blas_library(self.prev)
        return False


def transposed(m):
    """m^T as a dense tensor (vmlmf_transpose: LDS tiles; torch's strided copy takes 43 us for the 26 MB of the PTB head's dW)."""
    if not (m.is_cuda and m.dtype == torch.float32 and m.dim() == 2 and m.is_contiguous()):
        return m.t().contiguous()
    out = torch.empty((m.shape[1], m.shape[0]), device=m.device, dtype=torch.float32)
    with _lib.on_device(m.device):
        _lib.check(_lib.lib().vmlmf_transpose(m.shape[0], m.shape[1], _ptr(m), _ptr(out), _lib.raw_stream(m.device)))
    return out


def _head_products():
    """name -> [(label, fn)] candidate forms; every fn returns a contiguous result."""
    return {
        "fwd": [("mm(h, W^T)", lambda h, w: torch.mm(h, w.t()))],
        "dh": [("mm(dz, W)", lambda dz, w: torch.mm(dz, w))],
        "dw": [("mm(dz^T, h)", lambda dz, h: torch.mm(dz.t(), h)),
               ("mm(h^T, dz)^T", lambda dz, h: transposed(torch.mm(h.t(), dz)))],
    }


def head_forms(R, H, V, device):
    """The (library, form) chosen for each of the LM head's three GEMMs at this shape; timed on first use."""
    import os
    key = (R, H, V, device.index)
    hit = _HEAD_FORMS.get(key)
    if hit is not None:
        return hit
    prods = _head_products()
    tune = os.environ.get("VMLMF_HEAD_TUNE", "1") != "0" and not torch.cuda.is_current_stream_capturing()
    chosen = {k: (None, v[0][0], v[0][1], None) for k, v in prods.items()}
    if tune:
        # with the user's TunableOp on (PYTORCH_TUNABLEOP_ENABLED=1) the solutions of both libraries are candidates of every call:
        # no preferred-library switch, under which the other library's tuned solutions are not found again
        tunable = getattr(torch.cuda, "tunable", None)
        libs = [None] if (tunable is not None and tunable.is_enabled()) else _blas_libs()
        with torch.no_grad():
            a = {"fwd": (torch.randn(R, H, device=device), torch.randn(V, H, device=device)),
                 "dh": (torch.randn(R, V, device=device), torch.randn(V, H, device=device)),
                 "dw": (torch.randn(R, V, device=device), torch.randn(R, H, device=device))}
            for name, forms in prods.items():
                best = None
                for lib in libs:
                    for label, fn in forms:
                        try:
                            with _with_blas(lib):
                                fn(*a[name])
                                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                                e0.record()
                                for _ in range(3):
                                    fn(*a[name])
                                e1.record()
                            e1.synchronize()
                            ms = e0.elapsed_time(e1) / 3
                        except RuntimeError:
                            continue
                        if best is None or ms < best[3]:
                            best = (lib, label, fn, ms)
                if best is not None:
                    chosen[name] = best
            del a
    if tune or not torch.cuda.is_current_stream_capturing():
        _HEAD_FORMS[key] = chosen
    return chosen


def _run_form(form, *args):
    lib, _, fn, _ = form
    with _with_blas(lib):
        return fn(*args)


def _head_loss_forward(ctx, h, w, b, y, stats_floats, launch):
    """The forward of the LM head's training losses, written once: the projection in its tuned form, then `launch(lib, R, V, scores,
    bias, yrow, scale, stats, dbias, stream)` - the one thing the losses differ in - takes the loss into `stats`
    (stats_floats(R) floats) and overwrites the scores with their own gradient, which is what is saved for _head_loss_backward."""
    _require_hip(h, "h")
    _require_hip(w, "fc.w")
    H = h.shape[-1]
    h2 = h.reshape(-1, H).contiguous()
    w = w.contiguous()
    R, V = h2.shape[0], w.shape[0]
    forms = head_forms(R, H, V, h.device)
    scores = _run_form(forms["fwd"], h2, w)                       # (R, V), no bias
    yrow = y.reshape(-1).contiguous()
    scale = float(y.size(1)) / float(R)
    stats = torch.empty(stats_floats(R), device=h.device, dtype=torch.float32)
    dbias = torch.empty(V, device=h.device, dtype=torch.float32) if b is not None else None
    lib = _lib.lib()
    with _lib.on_device(h.device):
        launch(lib, R, V, scores, None if b is None else b.contiguous(), yrow, scale, stats, dbias, _lib.raw_stream(h.device))
    ctx.save_for_backward(h2, w, scores, *([dbias] if dbias is not None else []))
    ctx.hshape, ctx.forms, ctx.has_b = h.shape, forms, b is not None
    return stats


class TiedGradient:
    """The holder of ONE (V, H) gradient of a table that is both the embedding and the vocabulary projection (Model.tie_weights;
    docs/design/lm_tied.md): it carries the head's dW from the head's backward to the embedding's backward of the SAME call, which
    adds its rows into that tensor in place (vmlmf_embed_backward_ex, accumulate=1) and returns it as the table's one gradient.
    The head takes the table detached, so autograd has no edge - and forms no table-wide sum - of its own.  Make a fresh holder
    per loss call and hand it to both ends (lm_head_loss(..., grad_to=) and embedding(..., grad_from=))."""
    __slots__ = ("dw",)

    def __init__(self):
        self.dw = None

    def put(self, dw):
        self.dw = dw

    def take(self):
        dw, self.dw = self.dw, None
        return dw


def tied_gradient(weight, tokens):
    """A fresh TiedGradient where both ends of a tied table take it - the table requires grad under autograd, the package's
    embedding backward covers it (_embed_covered) and the fused head loss covers its width - else None: autograd's own accumulation
    of the two gradients, which is always correct."""
    V = weight.shape[0]
    if (torch.is_grad_enabled() and weight.requires_grad and _embed_covered(weight, tokens) and tokens.numel() > 0
            and V % 4 == 0 and V <= 12288):
        return TiedGradient()
    return None


def _head_loss_backward(ctx, dloss):
    """(dh, dw, db) of the LM head's training losses: the two GEMMs read the scores' gradient where the forward left it.  A head that
    was handed a TiedGradient (ctx.tied; its weight came in detached) forms dw all the same, puts it into the holder and returns
    None for the weight: the embedding's backward of this call finishes it."""
    h2, w, dz = ctx.saved_tensors[:3]
    dbias = ctx.saved_tensors[3] if ctx.has_b else None
    tied = getattr(ctx, "tied", None)
    scaled = not _is_unit(dloss)
    dh = _run_form(ctx.forms["dh"], dz, w) if ctx.needs_input_grad[0] else None
    dw = _run_form(ctx.forms["dw"], dz, h2) if (ctx.needs_input_grad[1] or tied is not None) else None
    db = dbias if (ctx.has_b and ctx.needs_input_grad[2]) else None
    if scaled:                                   # d(loss) is not the package's constant one: the stored gradient is for 1
        dh = None if dh is None else dh.mul_(dloss)
        dw = None if dw is None else dw.mul_(dloss)
        db = None if db is None else db * dloss
    if tied is not None:
        tied.put(dw)
        dw = None
    return (None if dh is None else dh.view(ctx.hshape)), dw, db


def _nll_launch(lib, R, V, scores, bias, yrow, scale, stats, dbias, stream):
    scratch = _workspace(scores.device, 4 * lib.vmlmf_nll_grad_scratch_floats(R, V))
    _lib.check(lib.vmlmf_nll_forward_grad(R, V, _ptr(scores), _ptr(bias), _ptr(yrow), scale, stats.data_ptr(), stats.data_ptr() + 4,
                                          _ptr(dbias), scratch.data_ptr(), stream))


class LmHeadLossFn(torch.autograd.Function):
    """loss = nll_loss(Linear(h), y) (vmlmf_lm.py:355-358 + lm_test.py:140-153) for training; see the block comment above."""

    @staticmethod
    def forward(ctx, h, w, b, y, rows=False, tied=None):
        ctx.tied = tied
        stats = _head_loss_forward(ctx, h, w, b, y, lambda R: 1 + R, _nll_launch)            # loss | rowloss
        if not rows:
            return stats[0]
        rowloss = stats[1:]
        ctx.mark_non_differentiable(rowloss)
        return stats[0], rowloss

    @staticmethod
    def backward(ctx, dloss, *_):
        return (*_head_loss_backward(ctx, dloss), None, None, None)


def lm_head_loss(h, weight, bias, y, return_rows=False, grad_to=None):
    """Training form of nll_loss(Linear(h), y): h (T, B, H), weight (V, H), bias (V), y (T, B) int64 -> scalar loss whose
    backward reads the scores' gradient where the forward left it.  Call loss.backward(vmlmf_amd.unit_gradient(device)) to spare
    the three scalings a foreign d(loss) tensor costs.  Vocabulary widths the in-register loss does not cover (not a multiple
    of four, beyond 12288) and CPU tensors take projection + nll_loss.
    return_rows=True: (loss, rows) - rows (T B) fp32 is what each position is charged, logsumexp(z_r) - z_r[y_r], unscaled and not
    differentiable: the row output the loss launch writes anyway (the stock path forms it in stock ops).
    grad_to: a TiedGradient (tied_gradient()) when `weight` is also the embedding table of the same call - the fused path then takes
    the weight detached and leaves its dW in the holder for embedding(..., grad_from=) (the other paths leave the holder empty and
    autograd adds the two gradients up)."""
    V = weight.shape[0]
    if h.is_cuda and h.dtype == torch.float32 and y.dtype == torch.int64 and V % 4 == 0 and V <= 12288:
        if grad_to is not None:
            return LmHeadLossFn.apply(h, weight.detach(), bias, y, bool(return_rows), grad_to)
        return LmHeadLossFn.apply(h, weight, bias, y, True) if return_rows else LmHeadLossFn.apply(h, weight, bias, y)
    scores = torch.addmm(bias, h.reshape(-1, h.shape[-1]), weight.t())
    if not return_rows:
        return nll_loss(scores, y)
    with torch.no_grad():
        rows = scores.logsumexp(1) - scores.gather(1, y.reshape(-1, 1)).squeeze(1)
    return nll_loss(scores, y), rows


# ---- knowledge distillation at the LM head (C ABI vmlmf_distill_forward_grad; csrc/vmlmf_distill.hip; docs/design/lm_distill.md) ----
# loss = scale sum_r ((1 - alpha) hard_r + alpha soft_r) against a teacher's distribution P: hard_r is lm_head_loss's row term,
# soft_r = tau^2 KL(P_r || softmax(z_r / tau)) (Hinton, Vinyals, Dean).  The same three GEMMs as lm_head_loss; between them ONE
# pass over the scores takes both losses and leaves the gradient of their mix in place.
DISTILL_MAX_TOP = 32


def check_distill(alpha, temperature, top=0):
    """ValueError for an alpha outside [0, 1], a temperature that is not finite and positive, a top outside [0, 32]."""
    import math
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0.0 <= alpha <= 1.0:
        raise ValueError(f"vmlmf_amd: distillation's alpha must lie in [0, 1], got {alpha!r}")
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not (math.isfinite(temperature) and temperature > 0):
        raise ValueError(f"vmlmf_amd: distillation's temperature must be finite and positive, got {temperature!r}")
    if isinstance(top, bool) or not isinstance(top, int) or not 0 <= top <= DISTILL_MAX_TOP:
        raise ValueError(f"vmlmf_amd: distillation's top must lie in [0, {DISTILL_MAX_TOP}], got {top!r}")


def distill_teacher(teacher, R, V, dtype=torch.float32):
    """A teacher in one of its two forms, checked against the student's R rows of V scores of type `dtype` and flattened to rows:
    (scores (R, V), None, None) for a (T, B, V) or (R, V) tensor; (None, top_tokens (R, k) int64, top_scores (R, k)) for a pair of
    (T, B, k) or (R, k) tensors, 1 <= k <= min(32, V).  ValueError for another shape or type; no value is looked at."""
    if isinstance(teacher, torch.Tensor):
        if teacher.dtype != dtype or teacher.dim() not in (2, 3) or teacher.shape[-1] != V or teacher.numel() != R * V:
            raise ValueError(f"vmlmf_amd: a dense teacher is (T, B, V) or (R, V) {dtype} scores for {R} rows of {V}, "
                             f"got {tuple(teacher.shape)} {teacher.dtype}")
        return teacher.reshape(R, V), None, None
    if not (isinstance(teacher, (tuple, list)) and len(teacher) == 2 and all(isinstance(t, torch.Tensor) for t in teacher)):
        raise ValueError("vmlmf_amd: a teacher is a score tensor or a pair (top_tokens, top_scores)")
    tok, sc = teacher
    k = tok.shape[-1] if tok.dim() in (2, 3) else 0
    if (tok.dtype != torch.int64 or sc.dtype != dtype or tok.shape != sc.shape or not 1 <= k <= min(DISTILL_MAX_TOP, V)
            or tok.numel() != R * k):
        raise ValueError(f"vmlmf_amd: a top-k teacher is top_tokens int64 and top_scores {dtype}, both (T, B, k) or (R, k) with "
                         f"1 <= k <= {min(DISTILL_MAX_TOP, V)} for {R} rows, got {tuple(tok.shape)} {tok.dtype} and {tuple(sc.shape)} {sc.dtype}")
    return None, tok.reshape(R, k), sc.reshape(R, k)


def distill_loss_stock(scores, y, teacher, alpha, temperature):
    """The distillation loss in stock ops under autograd - the path of CPU tensors, of widths and types the kernel does not
    cover, and the baseline tools/bench_distill.py measures the kernel against.  scores (R, V) with the bias in them, y (T, B),
    teacher as distill_teacher() takes it.  Returns (loss, hard, soft), hard and soft scaled as nll_loss scales."""
    R, V = scores.shape
    dense, tok, tsc = distill_teacher(teacher, R, V, scores.dtype)
    scale, tau = float(y.size(1)) / float(R), float(temperature)
    hard = torch.nn.functional.cross_entropy(scores, y.reshape(-1), reduction="sum") * scale
    logq = torch.log_softmax(scores / tau, dim=1)
    if dense is not None:
        logp = torch.log_softmax(dense.detach() / tau, dim=1)
    else:
        logp, logq = torch.log_softmax(tsc.detach() / tau, dim=1), logq.gather(1, tok)
    soft = torch.nn.functional.kl_div(logq, logp, reduction="sum", log_target=True) * (tau * tau * scale)
    return (1.0 - alpha) * hard + alpha * soft, hard, soft


class LmHeadDistillFn(torch.autograd.Function):
    """(loss, hard, soft) of lm_head_distill_loss; the forward product, the tuned forms and the backward are lm_head_loss's, the
    loss launch is vmlmf_distill_forward_grad.  hard and soft are reported, not differentiable."""

    @staticmethod
    def forward(ctx, h, w, b, y, dense, tok, tsc, alpha, tau, tied=None):
        ctx.tied = tied
        kd = _lib.Distill(alpha=alpha, temperature=tau, teacher=None if dense is None else dense.data_ptr(),
                          top_tokens=None if tok is None else tok.data_ptr(), top_scores=None if tsc is None else tsc.data_ptr(),
                          top=0 if tok is None else tok.shape[1])

        def launch(lib, R, V, scores, bias, yrow, scale, stats, dbias, stream):
            scratch = _workspace(scores.device, 4 * lib.vmlmf_distill_scratch_floats(R, V))
            _lib.check(lib.vmlmf_distill_forward_grad(R, V, _ptr(scores), _ptr(bias), _ptr(yrow), scale, ctypes.byref(kd), stats.data_ptr(),
                                                      stats.data_ptr() + 12, _ptr(dbias), scratch.data_ptr(), stream))

        stats = _head_loss_forward(ctx, h, w, b, y, lambda R: 3 + 2 * R, launch)             # total, hard, soft | rowloss (2, R)
        hard, soft = stats[1], stats[2]
        ctx.mark_non_differentiable(hard, soft)
        return stats[0], hard, soft

    @staticmethod
    def backward(ctx, dloss, dhard, dsoft):
        return (*_head_loss_backward(ctx, dloss), None, None, None, None, None, None, None)


def lm_head_distill_loss(h, weight, bias, y, teacher, *, alpha=0.5, temperature=2.0, return_parts=False, grad_to=None):
    """lm_head_loss with a soft-target term (knowledge distillation): h (T, B, H), weight (V, H), bias (V) or None, y (T, B) int64.
    With z = Linear(h), tau = temperature, Q = softmax(z / tau) and the teacher's distribution P, per row
        hard = logsumexp(z) - z[y]        soft = tau^2 KL(P || Q)        loss = scale sum ((1 - alpha) hard + alpha soft)
    scaled as nll_loss scales (scale = B / (T B)).  teacher: (T, B, V) or (R, V) fp32 scores, the teacher's bias in them -
    P = softmax(teacher / tau) -, or a pair (top_tokens (T, B, k) int64, top_scores (T, B, k) fp32), 1 <= k <= 32, as
    Model.score(top=k) returns them - P = softmax(top_scores / tau) on those tokens and zero elsewhere (scores or log-probabilities:
    a constant per row changes nothing).  The teacher is a constant: no gradient flows into it.  Returns the scalar loss; with
    return_parts=True (loss, hard, soft), the parts detached and scaled like the loss.
    On a HIP device one pass over the scores takes both terms and leaves the gradient of the mix in place for the two backward
    GEMMs (vmlmf_distill_forward_grad); alpha == 0 IS lm_head_loss, launch for launch, and does not read the teacher (soft is then
    reported as zero).  CPU tensors, other types and widths the kernel does not cover (not a multiple of four, beyond 12288) take
    distill_loss_stock under autograd.  ValueError, before any device work, for alpha outside [0, 1], a temperature that is not
    finite and positive and teacher tensors of the wrong shape or type.  That the top tokens of a row are distinct and in [0, V) is
    the caller's responsibility: the call never reads a value back from the device, so it does not look."""
    check_distill(alpha, temperature)
    V = weight.shape[0]
    R = h.numel() // h.shape[-1]
    dense, tok, tsc = distill_teacher(teacher, R, V, h.dtype)
    alpha, tau = float(alpha), float(temperature)
    fused = h.is_cuda and h.dtype == torch.float32 and y.dtype == torch.int64 and V % 4 == 0 and V <= 12288
    if fused and alpha == 0.0:
        loss = LmHeadLossFn.apply(h, weight, bias, y) if grad_to is None else LmHeadLossFn.apply(h, weight.detach(), bias, y, False, grad_to)
        return (loss, loss.detach(), torch.zeros_like(loss)) if return_parts else loss
    if fused:
        given = [t.detach().contiguous() for t in (dense, tok, tsc) if t is not None]
        if any(t.device != h.device for t in given):
            raise ValueError(f"vmlmf_amd: the teacher's tensors must be on the student's device {h.device}")
        dense, tok, tsc = (given[0], None, None) if dense is not None else (None, given[0], given[1])
        if grad_to is not None:                  # a tied table (lm_head_loss's grad_to)
            loss, hard, soft = LmHeadDistillFn.apply(h, weight.detach(), bias, y, dense, tok, tsc, alpha, tau, grad_to)
        else:
            loss, hard, soft = LmHeadDistillFn.apply(h, weight, bias, y, dense, tok, tsc, alpha, tau)
    else:
        h2 = h.reshape(-1, h.shape[-1])
        scores = torch.mm(h2, weight.t()) if bias is None else torch.addmm(bias, h2, weight.t())
        loss, hard, soft = distill_loss_stock(scores, y, teacher, alpha, tau)
        hard, soft = hard.detach(), soft.detach()
    return (loss, hard, soft) if return_parts else loss


# ---- the general training objective at the LM head (C ABI vmlmf_objective_forward_grad; docs/design/lm_objective.md) ----
# A padding mask, label smoothing (eps), z-loss (zeta) and token-level unlikelihood (alpha; Welleck et al., "Neural Text Generation
# with Unlikelihood Training") as terms of lm_head_loss's one pass.  With p = softmax(z_r), lse_r = logsumexp(z_r), per row
#   nll = lse - z[y]    sm = lse - mean z    zl = lse^2    ul = sum over the row's negative set of -log(max(1 - p_c, 1e-5))
#   loss = scale sum over the unmasked rows of ((1 - eps) nll + eps sm + zeta zl + alpha ul)
OBJECTIVE_MAX_K = 256
UNLIKELIHOOD_FLOOR = 1e-5


def check_objective(label_smoothing, z_loss, unlikelihood, normalize):
    """ValueError for a label_smoothing outside [0, 1), a negative or non-finite z_loss or unlikelihood, a normalize that is
    neither "rows" nor "tokens"."""
    import math

    def number(v):
        return not isinstance(v, bool) and isinstance(v, (int, float)) and math.isfinite(v)
    if not (number(label_smoothing) and 0.0 <= label_smoothing < 1.0):
        raise ValueError(f"vmlmf_amd: label_smoothing must lie in [0, 1), got {label_smoothing!r}")
    if not (number(z_loss) and z_loss >= 0.0):
        raise ValueError(f"vmlmf_amd: z_loss must be finite and >= 0, got {z_loss!r}")
    if not (number(unlikelihood) and unlikelihood >= 0.0):
        raise ValueError(f"vmlmf_amd: unlikelihood must be finite and >= 0, got {unlikelihood!r}")
    if normalize not in ("rows", "tokens"):
        raise ValueError(f"vmlmf_amd: normalize is \"rows\" or \"tokens\", got {normalize!r}")


def check_lengths(lengths, B, who):
    """The contract Model.score and Model.loss share for lengths: None or an integer tensor of shape (B,)."""
    if lengths is not None and not (isinstance(lengths, torch.Tensor) and tuple(lengths.shape) == (B,) and not lengths.is_floating_point()
                                    and not lengths.is_complex() and lengths.dtype != torch.bool):
        raise ValueError(f"vmlmf_amd: {who}: lengths must be an integer tensor of shape ({B},), one per row")


def objective_negatives(negatives, R):
    """The rows' negative candidates flattened to (R, K): a (T, B, K) or (R, K) int64 tensor, 1 <= K <= 256.  ValueError for
    another type or shape; no value is looked at (entries outside [0, V) are padding)."""
    if not (isinstance(negatives, torch.Tensor) and negatives.dtype == torch.int64 and negatives.dim() in (2, 3)
            and 1 <= negatives.shape[-1] <= OBJECTIVE_MAX_K and negatives.numel() == R * negatives.shape[-1]):
        got = (tuple(negatives.shape), negatives.dtype) if isinstance(negatives, torch.Tensor) else type(negatives).__name__
        raise ValueError(f"vmlmf_amd: negatives are a (T, B, K) or (R, K) int64 tensor with 1 <= K <= {OBJECTIVE_MAX_K} for {R} rows, got {got}")
    return negatives.reshape(R, negatives.shape[-1])


def context_negatives(x):
    """The token-level unlikelihood candidates of the paper within a minibatch: for input tokens x (T, B) int64, a (T, B, T) int64
    tensor whose row (t, b) holds x[0 .. t, b] - every input token of the row up to and including position t - and -1 (padding)
    behind them.  The loss takes them as a set and drops the position's own target.  Stock ops on x's device, no read-back."""
    if not (isinstance(x, torch.Tensor) and x.dim() == 2 and x.dtype == torch.int64):
        raise ValueError("vmlmf_amd: context_negatives takes (T, B) int64 tokens")
    T = x.shape[0]
    steps = torch.arange(T, device=x.device)
    return x.t().unsqueeze(0).expand(T, -1, -1).masked_fill(steps[None, None, :] > steps[:, None, None], -1)


def _mask_targets(y, lengths):
    """y (T, B) with -1 at the positions t >= lengths[b], as Model.score masks them."""
    if lengths is None:
        return y
    return y.masked_fill(torch.arange(y.shape[0], device=y.device)[:, None] >= lengths.to(y.device)[None, :], -1)


def _valid_count(lengths, T, dtype):
    """max(number of positions t < lengths[b], 1) as a device scalar of `dtype`."""
    return lengths.clamp(0, T).sum().clamp(min=1).to(dtype)


def objective_loss_stock(scores, y, *, lengths=None, label_smoothing=0.0, z_loss=0.0, unlikelihood=0.0, negatives=None, normalize="rows"):
    """The general objective in stock ops under autograd - the path of CPU tensors, of widths and types the kernel does not cover,
    and the baseline tools/bench_objective.py measures the kernel against.  scores (R, V) with the bias in them, y (T, B) int64 (-1:
    masked), the keywords as lm_head_objective_loss takes them.  Returns (loss, nll, smooth, z, unlikelihood), the parts scaled like
    the loss and not by their weights; smooth and unlikelihood are zero where their weight is."""
    R, V = scores.shape
    T, B = y.shape
    eps, zeta, alpha = float(label_smoothing), float(z_loss), float(unlikelihood)
    yrow = _mask_targets(y, lengths).reshape(-1)
    live = yrow != -1
    scale = float(B) / float(R)
    if normalize == "tokens" and lengths is not None:
        scale = float(B) / _valid_count(lengths.to(scores.device), T, scores.dtype)
    inr = (yrow >= 0) & (yrow < V)
    lse = torch.logsumexp(scores, dim=1)
    zt = scores.gather(1, yrow.clamp(0, V - 1)[:, None])[:, 0]
    nll = lse - torch.where(inr | ~live, zt, torch.full_like(zt, float("nan")))   # a target outside [0, V) that is not the mask
    zero = torch.zeros_like(lse)
    smooth = lse - scores.mean(dim=1) if eps > 0 else zero
    zl = lse * lse
    ul = zero
    if alpha > 0:
        if negatives is None:
            raise ValueError("vmlmf_amd: unlikelihood > 0 takes negatives (Model.loss builds context_negatives(x) by default)")
        neg = objective_negatives(negatives, R).to(scores.device)
        member = torch.zeros(R, V + 1, dtype=torch.bool, device=scores.device)
        member.scatter_(1, torch.where((neg >= 0) & (neg < V), neg, torch.full_like(neg, V)), True)       # a set: duplicates once
        member = member[:, :V] & ~(torch.arange(V, device=scores.device)[None, :] == yrow[:, None])       # ... without the target
        p = torch.softmax(scores, dim=1)
        ul = -(torch.log(torch.clamp(1.0 - p, min=UNLIKELIHOOD_FLOOR)) * member).sum(dim=1)

    def total(rows):
        return scale * torch.where(live, rows, zero).sum()
    parts = [total(nll), total(smooth), total(zl), total(ul)]
    loss = (1.0 - eps) * parts[0] + eps * parts[1] + zeta * parts[2] + alpha * parts[3]
    return (loss, *parts)


class LmHeadObjectiveFn(torch.autograd.Function):
    """(loss, nll, smooth, z, unlikelihood) of lm_head_objective_loss; the forward product, the tuned forms and the backward are
    lm_head_loss's, the loss launch is vmlmf_objective_forward_grad.  The parts are reported, not differentiable."""

    @staticmethod
    def forward(ctx, h, w, b, y, negatives, scale_dev, eps, zeta, alpha, tied=None):
        ctx.tied = tied
        obj = _lib.Objective(label_smoothing=eps, z_loss=zeta, unlikelihood=alpha, negatives=None if negatives is None else negatives.data_ptr(),
                             k=0 if negatives is None else negatives.shape[1], scale_dev=None if scale_dev is None else scale_dev.data_ptr())

        def launch(lib, R, V, scores, bias, yrow, scale, stats, dbias, stream):
            scratch = _workspace(scores.device, 4 * lib.vmlmf_objective_scratch_floats(R, V))
            _lib.check(lib.vmlmf_objective_forward_grad(R, V, _ptr(scores), _ptr(bias), _ptr(yrow), scale, ctypes.byref(obj), stats.data_ptr(),
                                                        stats.data_ptr() + 20, _ptr(dbias), scratch.data_ptr(), stream))

        stats = _head_loss_forward(ctx, h, w, b, y, lambda R: 5 + 4 * R, launch)             # total and four parts | rowloss (4, R)
        parts = tuple(stats[i] for i in range(1, 5))
        ctx.mark_non_differentiable(*parts)
        return (stats[0], *parts)

    @staticmethod
    def backward(ctx, dloss, *dparts):
        return (*_head_loss_backward(ctx, dloss), None, None, None, None, None, None, None)


def lm_head_objective_loss(h, weight, bias, y, *, lengths=None, label_smoothing=0.0, z_loss=0.0, unlikelihood=0.0, negatives=None,
                           normalize="rows", return_parts=False, grad_to=None):
    """lm_head_loss with a padding mask, label smoothing, z-loss and token-level unlikelihood: h (T, B, H), weight (V, H), bias (V)
    or None, y (T, B) int64.  With z = Linear(h), p = softmax(z), eps = label_smoothing, zeta = z_loss, alpha = unlikelihood, per row
        nll = lse - z[y]    sm = lse - mean z    zl = lse^2    ul = sum over c in C of -log(max(1 - p_c, 1e-5))
        loss = scale sum over the unmasked rows of ((1 - eps) nll + eps sm + zeta zl + alpha ul)
    lengths (B) integers: position (t, b) counts iff t < lengths[b] (its target is set to -1, the mask: the row adds nothing and
    its gradient is zero); any other target outside [0, V) makes the loss NaN.  normalize "rows": scale = B / (T B), lm_head_loss's;
    "tokens": scale = B / max(number of valid positions, 1), formed on the device from lengths ("tokens" without lengths is "rows").
    negatives (T, B, K) or (T B, K) int64, 1 <= K <= 256: the row's candidate SET C - entries outside [0, V) are padding,
    duplicates count once, the row's own target is ignored; required when unlikelihood > 0, not read when it is 0.
    Returns the scalar loss; with return_parts=True (loss, nll, smooth, z, unlikelihood), the parts detached, scaled like the loss
    and not multiplied by their weights (smooth and unlikelihood are reported as zero where their weight is zero).
    On a HIP device (fp32, V a multiple of four, at most 12288) one pass over the scores takes all terms and leaves the gradient in
    place for the two backward GEMMs (vmlmf_objective_forward_grad); with everything off and no parts asked for the call IS
    lm_head_loss, launch for launch.  CPU tensors, other types and widths take objective_loss_stock under autograd.  ValueError,
    before any device work, for arguments out of range, lengths that are not (B) integers and negatives of the wrong type or shape.
    The call never reads a value back from the device."""
    check_objective(label_smoothing, z_loss, unlikelihood, normalize)
    if not (isinstance(y, torch.Tensor) and y.dim() == 2):
        raise ValueError("vmlmf_amd: lm_head_objective_loss takes targets y of shape (T, B)")
    check_lengths(lengths, y.shape[1], "lm_head_objective_loss")
    eps, zeta, alpha = float(label_smoothing), float(z_loss), float(unlikelihood)
    V, R = weight.shape[0], h.numel() // h.shape[-1]
    if alpha > 0 and negatives is None:
        raise ValueError("vmlmf_amd: unlikelihood > 0 takes negatives (Model.loss builds context_negatives(x) by default)")
    neg = objective_negatives(negatives, R) if alpha > 0 else None
    fused = h.is_cuda and h.dtype == torch.float32 and y.dtype == torch.int64 and V % 4 == 0 and V <= 12288
    if lengths is None and eps == 0.0 and zeta == 0.0 and alpha == 0.0 and not return_parts:
        return lm_head_loss(h, weight, bias, y, grad_to=grad_to)
    if fused:
        if neg is not None and neg.device != h.device:
            raise ValueError(f"vmlmf_amd: negatives must be on the scores' device {h.device}")
        scale_dev = None
        if normalize == "tokens" and lengths is not None:
            scale_dev = float(R) / _valid_count(lengths.to(h.device), y.shape[0], torch.float32)
        args = (_mask_targets(y, lengths), None if neg is None else neg.contiguous(), scale_dev, eps, zeta, alpha)
        if grad_to is not None:                  # a tied table (lm_head_loss's grad_to)
            out = LmHeadObjectiveFn.apply(h, weight.detach(), bias, *args, grad_to)
        else:
            out = LmHeadObjectiveFn.apply(h, weight, bias, *args)
    else:
        h2 = h.reshape(-1, h.shape[-1])
        scores = torch.mm(h2, weight.t()) if bias is None else torch.addmm(bias, h2, weight.t())
        out = objective_loss_stock(scores, y, lengths=lengths, label_smoothing=eps, z_loss=zeta, unlikelihood=alpha, negatives=neg,
                                   normalize=normalize)
        out = (out[0], *(t.detach() for t in out[1:]))
    return out if return_parts else out[0]


class EmbedFn(torch.autograd.Function):
    """x = w[tokens] (Embed, vmlmf_lm.py:46-48) whose backward is the package's deterministic scatter-add (vmlmf_embed_backward:
    every row of the table's gradient summed in position order, no float atomics, the zero fill in the same pass)."""

    @staticmethod
    def forward(ctx, w, tokens):
        ctx.save_for_backward(tokens)
        ctx.wshape = w.shape
        return torch.nn.functional.embedding(tokens, w)

    @staticmethod
    def backward(ctx, dy):
        (tokens,) = ctx.saved_tensors
        V, H = ctx.wshape
        dy2 = dy.reshape(-1, H).contiguous()
        R = dy2.shape[0]
        tok = tokens.reshape(-1).contiguous()
        dw = torch.empty((V, H), device=dy.device, dtype=torch.float32)
        lib = _lib.lib()
        nbytes = lib.vmlmf_embed_backward_scratch_bytes(R, V)
        scratch = _workspace(dy.device, nbytes, "embed")
        with _lib.on_device(dy.device):
            _lib.check(lib.vmlmf_embed_backward(R, H, V, _ptr(tok), _ptr(dy2), _ptr(dw), scratch.data_ptr(), nbytes,
                                                _lib.raw_stream(dy.device)))
        return dw, None


# ---- dropout of the LM network without mask tensors (C ABI 11: vmlmf_dropout_*; csrc/vmlmf_dropout.h) --------------------------
def dropout_state(device, seed=None):
    """{seed, offset} of the package's dropout generator on `device` (int64[2]).  seed=None: drawn from torch's CPU generator, so
    torch.manual_seed() makes the masks repeatable."""
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        # data-parallel replicas seeded alike (torch.manual_seed(s) on every rank) still draw different masks for their shards
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            seed = (seed + torch.distributed.get_rank() * 0x9E3779B97F4A7C15) & (2 ** 62 - 1)
    return torch.tensor([int(seed), 0], dtype=torch.int64, device=device)


def dropout_advance(state):
    """This forward's snapshot of `state`; the state moves on by one (one tiny launch: a node of a captured step, so every replay
    draws fresh factors)."""
    if not state.is_cuda or state.dtype != torch.int64 or state.numel() != 2:
        raise RuntimeError("vmlmf_amd: the dropout state is two int64 words on a HIP device (dropout_state())")
    snap = torch.empty_like(state)
    with _lib.on_device(state.device):
        _lib.check(_lib.lib().vmlmf_dropout_advance(state.data_ptr(), snap.data_ptr(), _lib.raw_stream(state.device)))
    return snap


class DropoutFn(torch.autograd.Function):
    """y = x * factor(snapshot, site) over the rows of x (..., H): nn.Dropout(p) in one launch per direction, the factors
    regenerated in the backward (no mask is kept)."""

    @staticmethod
    def forward(ctx, x, p, snap, site, locked_batch=0):
        _require_hip(x, "input")
        x = x.contiguous()
        y = torch.empty_like(x)
        ctx.save_for_backward(snap)
        ctx.p, ctx.site, ctx.locked_batch = float(p), int(site), int(locked_batch)
        DropoutFn.launch(ctx, snap, x, y)
        return y

    @staticmethod
    def launch(ctx, snap, x, y):
        """y = x * factor: the forward, and on the upstream gradient the backward; locked_batch = B > 0: x is (T, B, H) and the
        factors are those of the batch row (vmlmf_dropout_apply_locked)."""
        H = x.shape[-1]
        lib, stream = _lib.lib(), _lib.raw_stream(x.device)
        with _lib.on_device(x.device):
            if ctx.locked_batch:
                _lib.check(lib.vmlmf_dropout_apply_locked(x.numel() // H, ctx.locked_batch, H, _ptr(x), _ptr(y), ctx.p, snap.data_ptr(),
                                                          ctx.site, stream))
            else:
                _lib.check(lib.vmlmf_dropout_apply(x.numel() // H, H, _ptr(x), _ptr(y), ctx.p, snap.data_ptr(), ctx.site, stream))

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        DropoutFn.launch(ctx, ctx.saved_tensors[0], dy, dx)
        return dx, None, None, None, None


def locked_dropout_stock(x, p, training=True):
    """AWD-LSTM's LockedDropout in stock ops: one (1, B, H) mask of x (T, B, H), drawn from torch's generator, for every time step -
    the form of CPU tensors and of Model.stock_dropout."""
    if not training or p <= 0.0:
        return x
    return x * (x.new_empty(1, x.shape[1], x.shape[2]).bernoulli_(1 - p) / (1 - p))


def dropout(x, p, snap, site, locked=False):
    """nn.Dropout(p)(x) in training mode with the package's generator: x (..., H) float32 on a HIP device.  locked=True: locked
    (variational) dropout of x (T, B, H) - ONE (B, H) mask for every time step (AWD-LSTM's LockedDropout; the factors of
    dropout_factors(..., locked_batch=B)), in the same single launch per direction."""
    if locked and x.dim() != 3:
        raise ValueError("vmlmf_amd.dropout: a locked mask takes activations of shape (T, B, H)")
    if p <= 0.0:
        return x
    if x.dtype != torch.float32:
        raise RuntimeError("vmlmf_amd.dropout: float32 activations")
    return DropoutFn.apply(x, p, snap, site, x.shape[1] if locked else 0)


def dropout_factors(rows, H, p, snap, site, layer_desc=None, locked_batch=None):
    """The (rows, H) factors (0 or 1/(1-p)) the kernels apply for (snapshot, site) - for a layer whose launches apply them
    themselves pass its descriptor (vmlmf_dropout_factors).  The parity tests multiply a CPU restatement by this tensor.
    locked_batch=B: the locked factors of rows = T B time-major positions (vmlmf_dropout_factors_locked): row r has batch row r % B's."""
    out = torch.empty((rows, H), device=snap.device, dtype=torch.float32)
    desc = None if layer_desc is None else ctypes.byref(layer_desc)
    with _lib.on_device(snap.device):
        if locked_batch is None:
            _lib.check(_lib.lib().vmlmf_dropout_factors(desc, rows, H, float(p), snap.data_ptr(), int(site), out.data_ptr(),
                                                         _lib.raw_stream(snap.device)))
        else:
            _lib.check(_lib.lib().vmlmf_dropout_factors_locked(desc, rows, int(locked_batch), H, float(p), snap.data_ptr(), int(site),
                                                                out.data_ptr(), _lib.raw_stream(snap.device)))
    return out


# ---- activation regularisation of the LM's top layer (C ABI vmlmf_actreg_*; csrc/vmlmf_dropout.hip; docs/design/lm_actreg.md) ----
# AR and TAR of AWD-LSTM (Merity, Keskar, Socher, "Regularizing and Optimizing LSTM Language Models"): with raw (T, B, H) the top
# layer's output, f that site's dropout factors, yd = raw f and m[t,b] = (t < lengths[b]),
#   AR = sum m yd^2 / max(N_ar, 1)   TAR = sum m[t] m[t+1] (raw[t+1] - raw[t])^2 / max(N_tar, 1)   penalty = B (ar AR + tar TAR)
# N_ar = H #valid positions, N_tar = H #valid pairs of neighbouring steps.
def check_actreg(ar, tar):
    """ValueError for an ar or tar that is negative, not finite, a bool or no number."""
    import math
    for name, v in (("ar", ar), ("tar", tar)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"vmlmf_amd: {name} must be finite and >= 0, got {v!r}")


def activation_regularizer_stock(raw, *, ar, tar, factors=None, lengths=None, batch_scale=None):
    """activation_regularizer's rule in stock ops under autograd, the dropout factors of the site given as a tensor (None: all ones) -
    the path of CPU tensors, of types other than fp32 and of Model.stock_dropout, the baseline tools/bench_actreg.py measures the
    kernels against and the GPU tests' second opinion.  Returns (yd, penalty, (ar_part, tar_part)) as activation_regularizer does.
    (torch's mean over no element is NaN; here a term without a valid element is 0: T == 1, or lengths that leave no pair.)"""
    check_actreg(ar, tar)
    T, B, H = raw.shape
    check_lengths(lengths, B, "activation_regularizer_stock")
    scale = float(B if batch_scale is None else batch_scale)
    yd = raw if factors is None else raw * factors
    zero = torch.zeros((), device=raw.device, dtype=raw.dtype)
    live, n_ar, n_tar = None, float(max(T * B * H, 1)), float(max((T - 1) * B * H, 1))
    if lengths is not None:
        n = lengths.to(raw.device).clamp(0, T)
        live = (torch.arange(T, device=raw.device)[:, None] < n[None, :])[:, :, None]
        n_ar = (n.sum() * H).clamp(min=1).to(raw.dtype)
        n_tar = ((n - 1).clamp(min=0).sum() * H).clamp(min=1).to(raw.dtype)
    ar_part = tar_part = zero
    if ar > 0:
        sq = yd * yd
        ar_part = scale * ((sq if live is None else torch.where(live, sq, zero)).sum() / n_ar)
    if tar > 0 and T > 1:
        d = raw[1:] - raw[:-1]
        sq = d * d
        tar_part = scale * ((sq if live is None else torch.where(live[1:] & live[:-1], sq, zero)).sum() / n_tar)
    return yd, ar * ar_part + tar * tar_part, (ar_part.detach(), tar_part.detach())


class ActRegFn(torch.autograd.Function):
    """(yd, penalty, ar_part, tar_part) of activation_regularizer: vmlmf_actreg_forward, and vmlmf_actreg_backward for the gradient of
    raw from those of yd and the penalty - one launch each, the factors regenerated, nothing kept but raw and eight floats."""

    @staticmethod
    def forward(ctx, raw, lengths, snap, ar, tar, p, site, layer_desc, batch_scale):
        _require_hip(raw, "raw")
        raw = raw.contiguous()
        T, B, H = raw.shape
        dev, lib = raw.device, _lib.lib()
        yd = torch.empty_like(raw) if p > 0 else None
        stats = torch.empty(_lib.ACTREG_STATS, device=dev, dtype=torch.float32)
        scratch = _workspace(dev, 4 * lib.vmlmf_actreg_scratch_floats(T, B, H), "actreg")
        ticket = _stream_ticket(dev, "actreg")
        desc = None if layer_desc is None else ctypes.byref(layer_desc)
        with _lib.on_device(dev):
            _lib.check(lib.vmlmf_actreg_forward(T, B, H, _ptr(raw), _ptr(yd), _ptr(lengths), ar, tar, batch_scale, p, _ptr(snap), site, desc,
                                                stats.data_ptr(), scratch.data_ptr(), ticket.data_ptr(), _lib.raw_stream(dev)))
        ctx.save_for_backward(raw, stats, *(t for t in (lengths, snap) if t is not None))
        ctx.has_lengths, ctx.args, ctx.layer_desc = lengths is not None, (ar, tar, p, site), layer_desc
        parts = (stats[1], stats[2])
        ctx.mark_non_differentiable(*parts)
        return (raw.view_as(raw) if yd is None else yd, stats[0], *parts)      # (p == 0: yd IS raw, nothing was written)

    @staticmethod
    def backward(ctx, g, dpenalty, *_):
        raw, stats, *rest = ctx.saved_tensors
        lengths = rest.pop(0) if ctx.has_lengths else None
        snap = rest.pop(0) if rest else None
        ar, tar, p, site = ctx.args
        T, B, H = raw.shape
        g = g.contiguous()
        draw = torch.empty_like(raw)
        scaled = None if _is_unit(dpenalty) else dpenalty.to(torch.float32).contiguous()
        desc = None if ctx.layer_desc is None else ctypes.byref(ctx.layer_desc)
        with _lib.on_device(raw.device):
            _lib.check(_lib.lib().vmlmf_actreg_backward(T, B, H, _ptr(raw), _ptr(g), _ptr(draw), _ptr(lengths), ar, tar, p, _ptr(snap), site, desc,
                                                        stats.data_ptr(), _ptr(scaled), _lib.raw_stream(raw.device)))
        return draw, None, None, None, None, None, None, None, None


def activation_regularizer(raw, *, ar, tar, p=0.0, snap=None, site=0, lengths=None, layer_desc=None, batch_scale=None):
    """AWD-LSTM's activation regularisation (AR, weight `ar`: its --alpha) and temporal activation regularisation (TAR, weight `tar`:
    its --beta) of a recurrent layer's output raw (T, B, H), with the dropout behind that layer applied in the same pass.  With f the
    factors of (snap, site, p) - 0 or 1 / (1 - p); all ones at p == 0 -, yd = raw f, and m[t,b] = 1 iff t < lengths[b] (lengths (B)
    integers, Model.score's contract; None: every position):
        AR = sum m yd^2 / max(N_ar, 1),  N_ar = H #{m[t,b]}          TAR = sum m[t] m[t+1] (raw[t+1] - raw[t])^2 / max(N_tar, 1),
        N_tar = H #{t + 1 < T: m[t,b] m[t+1,b]}                      penalty = batch_scale (ar AR + tar TAR)
    AR is taken on the dropped copy, TAR on the raw one, as AWD-LSTM's main.py takes them; batch_scale (default B) is the factor
    Model.loss carries over the mean NLL.  At T == 1, or when the lengths leave no pair, TAR is 0 (torch's mean over no element would
    be NaN).  Returns (yd, penalty, (ar_part, tar_part)): yd for the head - every position's, masked ones included; at p == 0 it is
    raw itself -, the differentiable penalty, and batch_scale AR and batch_scale TAR, detached and not multiplied by their weights; a
    term whose weight is 0 is not formed and reported as 0.
    The factors are the ones dropout(raw, p, snap, site) applies - with layer_desc, the descriptor of a layer whose own launches
    apply its dropout (vmlmf_dropout_fused), the ones that layer would have applied (dropout_factors(..., layer_desc)).
    fp32 on a HIP device: ONE launch forward and ONE backward (vmlmf_actreg_forward / _backward): raw is read once per direction,
    the sums are reduced in a fixed order (the same bits from run to run), the counts are formed on the device from lengths, no
    value is read back - a step with it captures; an upstream gradient of the penalty other than unit_gradient()'s scales its share
    inside the backward launch.  CPU tensors and other types take activation_regularizer_stock (with p > 0 on the CPU the factors
    come from torch's generator: snap and site are not looked at).  ValueError, before any device work, for an ar or tar that is
    negative, not finite or a bool, p outside [0, 1), p > 0 without a snapshot on a HIP device, a raw that is not (T, B, H) and
    lengths that are not (B) integers.
    site=locked_site(i): the site's dropout is the LOCKED one (dropout(..., locked=True): one (B, H) mask for every step) - the
    flag rides in the site word as it does in the C ABI, whose entries that know B take it; a thread of either launch then draws
    once for its four time steps."""
    check_actreg(ar, tar)
    if not (isinstance(raw, torch.Tensor) and raw.dim() == 3 and raw.numel() > 0 and raw.is_floating_point()):
        raise ValueError("vmlmf_amd: activation_regularizer takes activations raw of shape (T, B, H)")
    T, B, H = raw.shape
    check_lengths(lengths, B, "activation_regularizer")
    locked, site = bool(int(site) & (1 << 31)), int(site) & 0x7FFFFFFF
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"vmlmf_amd: p must lie in [0, 1), got {p!r}")
    if p > 0 and raw.is_cuda and not (isinstance(snap, torch.Tensor) and snap.is_cuda and snap.dtype == torch.int64 and snap.numel() == 2):
        raise ValueError("vmlmf_amd: p > 0 takes the snapshot of dropout_advance()")
    scale = float(B if batch_scale is None else batch_scale)
    if raw.is_cuda and raw.dtype == torch.float32:
        n = None if lengths is None else lengths.to(device=raw.device, dtype=torch.int64).contiguous()
        word = int(site) + (_lib.SITE_LOCKED if locked else 0)      # (these entries know B: the flag asks for the locked factors)
        yd, penalty, ar_part, tar_part = ActRegFn.apply(raw, n, snap if p > 0 else None, float(ar), float(tar), p, word, layer_desc, scale)
        return yd, penalty, (ar_part, tar_part)
    factors = None
    if p > 0 and raw.is_cuda:
        factors = dropout_factors(T * B, H, p, snap, site, layer_desc, B if locked else None).view(T, B, H).to(raw.dtype)
    elif p > 0 and locked:
        factors = locked_dropout_stock(torch.ones_like(raw[:1]), p)
    elif p > 0:
        factors = torch.nn.functional.dropout(torch.ones_like(raw), p, True)
    return activation_regularizer_stock(raw, ar=ar, tar=tar, factors=factors, lengths=lengths, batch_scale=scale)


class EmbedDropFn(torch.autograd.Function):
    """dropout(w[tokens]) of vmlmf_lm.py:434-435 as one gather launch; backward: EmbedFn's scatter-add with the factors regenerated
    on the fly."""

    @staticmethod
    def forward(ctx, w, tokens, p, snap, site):
        V, H = w.shape
        tok = tokens.reshape(-1).contiguous()
        out = torch.empty(tuple(tokens.shape) + (H,), device=w.device, dtype=torch.float32)
        with _lib.on_device(w.device):
            _lib.check(_lib.lib().vmlmf_embed_dropout_forward(tok.numel(), H, V, _ptr(tok), _ptr(w), _ptr(out), float(p), snap.data_ptr(),
                                                              int(site), _lib.raw_stream(w.device)))
        ctx.save_for_backward(tok, snap)
        ctx.wshape, ctx.p, ctx.site = w.shape, float(p), int(site)
        return out

    @staticmethod
    def backward(ctx, dy):
        tok, snap = ctx.saved_tensors
        V, H = ctx.wshape
        dy2 = dy.reshape(-1, H).contiguous()
        R = dy2.shape[0]
        dw = torch.empty((V, H), device=dy.device, dtype=torch.float32)
        lib = _lib.lib()
        nbytes = lib.vmlmf_embed_backward_scratch_bytes(R, V)
        scratch = _workspace(dy.device, nbytes, "embed")
        with _lib.on_device(dy.device):
            _lib.check(lib.vmlmf_embed_dropout_backward(R, H, V, _ptr(tok), _ptr(dy2), _ptr(dw), scratch.data_ptr(), nbytes, ctx.p,
                                                        snap.data_ptr(), ctx.site, _lib.raw_stream(dy.device)))
        return dw, None, None, None, None


def _embed_covered(weight, tokens):
    return (weight.is_cuda and weight.dtype == torch.float32 and weight.dim() == 2 and weight.shape[1] <= 1024 and tokens.dtype == torch.int64
            and weight.is_contiguous() and weight.shape[0] * ((tokens.numel() + 31) // 32) * 4 <= (64 << 20))


def check_word_dropout(word_p, who="embed_dropout"):
    """ValueError for a word-dropout probability that is a bool, not a number or outside [0, 1)."""
    if isinstance(word_p, bool) or not isinstance(word_p, (int, float)) or not 0.0 <= word_p < 1.0:
        raise ValueError(f"vmlmf_amd: {who} must be a number in [0, 1), got {word_p!r}")


class EmbedExFn(torch.autograd.Function):
    """(w[tokens] * fw[tokens]) * f - the gather under AWD-LSTM's word dropout (fw: one factor per vocabulary row) and the element
    dropout (f) - and / or the embedding end of a tied table (docs/design/lm_tied.md): vmlmf_embed_dropout_forward_ex and
    vmlmf_embed_backward_ex, one launch sequence per direction.  With a TiedGradient that the head's backward filled the backward
    adds its rows INTO the head's dW (accumulate=1: rows no token hit are neither read nor written) and returns that tensor as
    the table's one gradient; with an empty holder, or none, it returns its own (accumulate=0).
    The order is safe: this function's output feeds the layers, which feed the head, so within a backward pass autograd runs the
    head's backward - which fills the holder - before this one.  This is the one place that relies on it."""

    @staticmethod
    def forward(ctx, w, tokens, p, word_p, snap, site, holder, locked_batch=0):
        V, H = w.shape
        tok = tokens.reshape(-1).contiguous()
        if p > 0.0 or word_p > 0.0:
            out = torch.empty(tuple(tokens.shape) + (H,), device=w.device, dtype=torch.float32)
            lib, stream = _lib.lib(), _lib.raw_stream(w.device)
            with _lib.on_device(w.device):
                if locked_batch:       # tokens (T, B): the element factors of a position are its batch row's (the _lk entries)
                    _lib.check(lib.vmlmf_embed_dropout_forward_lk(tok.numel(), int(locked_batch), H, V, _ptr(tok), _ptr(w), _ptr(out), float(p),
                                                                  float(word_p), snap.data_ptr(), int(site), stream))
                else:
                    _lib.check(lib.vmlmf_embed_dropout_forward_ex(tok.numel(), H, V, _ptr(tok), _ptr(w), _ptr(out), float(p), float(word_p),
                                                                  snap.data_ptr(), int(site), stream))
            ctx.save_for_backward(tok, snap)
        else:
            out = torch.nn.functional.embedding(tokens, w)
            ctx.save_for_backward(tok)
        ctx.wshape, ctx.p, ctx.word_p, ctx.site, ctx.holder = w.shape, float(p), float(word_p), int(site), holder
        ctx.locked_batch = int(locked_batch) if p > 0.0 else 0
        return out

    @staticmethod
    def backward(ctx, dy):
        tok = ctx.saved_tensors[0]
        snap = ctx.saved_tensors[1] if len(ctx.saved_tensors) > 1 else None
        V, H = ctx.wshape
        dy2 = dy.reshape(-1, H).contiguous()
        R = dy2.shape[0]
        dw = ctx.holder.take() if ctx.holder is not None else None     # the head's dW of this backward pass, or nothing
        accumulate = dw is not None
        if not accumulate:
            dw = torch.empty((V, H), device=dy.device, dtype=torch.float32)
        lib = _lib.lib()
        nbytes = lib.vmlmf_embed_backward_scratch_bytes(R, V)
        scratch = _workspace(dy.device, nbytes, "embed")
        state, stream = None if snap is None else snap.data_ptr(), _lib.raw_stream(dy.device)
        with _lib.on_device(dy.device):
            if ctx.locked_batch:
                _lib.check(lib.vmlmf_embed_backward_lk(R, ctx.locked_batch, H, V, _ptr(tok), _ptr(dy2), _ptr(dw), int(accumulate),
                                                       scratch.data_ptr(), nbytes, ctx.p, ctx.word_p, state, ctx.site, stream))
            else:
                _lib.check(lib.vmlmf_embed_backward_ex(R, H, V, _ptr(tok), _ptr(dy2), _ptr(dw), int(accumulate), scratch.data_ptr(), nbytes, ctx.p,
                                                       ctx.word_p, state, ctx.site, stream))
        return dw, None, None, None, None, None, None, None


def _embed_ex(weight, tokens, p, word_p, snap, site, grad_from, locked_batch=0):
    if not _embed_covered(weight, tokens):
        raise RuntimeError("vmlmf_amd: word dropout and a tied table's gradient take a contiguous fp32 table on a HIP device, up to 1024 "
                           "wide and 64 MB of position bits, and int64 tokens (embedding_dropout_stock is the form in stock ops)")
    if (p > 0.0 or word_p > 0.0) and snap is None:
        raise ValueError("vmlmf_amd: dropout takes a snapshot of the generator (dropout_advance())")
    return EmbedExFn.apply(weight, tokens, float(p), float(word_p), snap, site, grad_from, locked_batch)


def embedding_dropout(weight, tokens, p, snap, site=0, *, word_p=0.0, grad_from=None, locked=False):
    """dropout(weight[tokens]) - the first two lines of Model.forward (vmlmf_lm.py:434-435) - as one launch per direction on HIP fp32
    tables up to 1024 wide; embedding() followed by dropout() otherwise.
    word_p in [0, 1): AWD-LSTM's embedding dropout (--dropoute) in the same launches - whole WORDS are dropped, one factor per
    vocabulary row (0, or 1 / (1 - word_p)) shared by every position that holds the word, applied before the element dropout:
    (weight[tokens] * fw[tokens]) * f; word_dropout_factors() shows fw.  grad_from: a TiedGradient when `weight` is also the
    head's weight of the same call (EmbedExFn).  With both at their defaults the call is what it was without them.
    locked=True: tokens are (T, B) and the element dropout is the locked one - a position's factors are its batch row's, the same
    at every time step (dropout(..., locked=True)) - in the same launches; it composes with word_p and grad_from."""
    check_word_dropout(word_p, "word_p")
    if locked:
        if tokens.dim() != 2:
            raise ValueError("vmlmf_amd.embedding_dropout: a locked mask takes tokens of shape (T, B)")
        if p > 0.0 and word_p == 0.0 and grad_from is None and not _embed_covered(weight, tokens):
            return dropout(embedding(weight, tokens), p, snap, site, locked=True)
        if p > 0.0:
            return _embed_ex(weight, tokens, float(p), word_p, snap, site, grad_from, tokens.shape[1])
    if word_p == 0.0 and grad_from is None:
        if p <= 0.0:
            return embedding(weight, tokens)
        if _embed_covered(weight, tokens):
            return EmbedDropFn.apply(weight, tokens, p, snap, site)
        return dropout(embedding(weight, tokens), p, snap, site)
    return _embed_ex(weight, tokens, max(float(p), 0.0), word_p, snap, site, grad_from)


def embedding_dropout_stock(weight, tokens, p, word_p, training=True):
    """The same rule in stock ops under autograd, literally AWD-LSTM's embedded_dropout followed by the input dropout - for CPU
    tensors and Model.stock_dropout: F.dropout(F.embedding(tokens, weight * F.dropout(ones(V, 1), word_p)), p), masks from torch's
    generator."""
    F = torch.nn.functional
    check_word_dropout(word_p, "word_p")
    if training and word_p > 0.0:
        weight = weight * F.dropout(torch.ones((weight.shape[0], 1), device=weight.device, dtype=weight.dtype), word_p, True)
    return F.dropout(F.embedding(tokens, weight), p, training)


def word_dropout_factors(V, word_p, snap):
    """The (V) fp32 word factors fw (0 or 1 / (1 - word_p)) that embedding_dropout(..., word_p=) applies under the snapshot `snap`:
    formed by the gather itself on a (V, 4) table of ones.  For tests, and for users who want to see the mask."""
    check_word_dropout(word_p, "word_p")
    if not (isinstance(snap, torch.Tensor) and snap.is_cuda and snap.dtype == torch.int64 and snap.numel() == 2):
        raise RuntimeError("vmlmf_amd: the snapshot is two int64 words on a HIP device (dropout_advance())")
    ones = torch.ones((int(V), 4), device=snap.device, dtype=torch.float32)
    out = torch.empty_like(ones)
    tok = torch.arange(int(V), device=snap.device, dtype=torch.int64)
    with _lib.on_device(snap.device):
        _lib.check(_lib.lib().vmlmf_embed_dropout_forward_ex(int(V), 4, int(V), _ptr(tok), _ptr(ones), _ptr(out), 0.0, float(word_p),
                                                             snap.data_ptr(), 0, _lib.raw_stream(snap.device)))
    return out[:, 0].contiguous()


def embedding(weight, tokens, grad_from=None):
    """weight[tokens] with the package's backward on HIP fp32 tables up to 1024 wide and 64 MB of position bits; the stock op otherwise.
    grad_from: a TiedGradient when `weight` is also the head's weight of the same call (EmbedExFn)."""
    if grad_from is not None:
        return _embed_ex(weight, tokens, 0.0, 0.0, None, 0, grad_from)
    if _embed_covered(weight, tokens):
        return EmbedFn.apply(weight, tokens)
    return weight[tokens]


def linear_nll(h, weight, bias, y, chunk_rows=2048, fused=None):
    """loss = nll_loss(Linear(h), y) of the LM loop (vmlmf_lm.py:355-358 + lm_test.py:140-153): h (T, B, H), weight (V, H), bias
    (V), y (T, B) int64.  fused=None: the chunked form without the score tensor when no gradient is needed (evaluation,
    perplexity), GEMM + loss over the full tensor when one is (measured: LinearNllFn's docstring); True / False force one."""
    need_grad = torch.is_grad_enabled() and (h.requires_grad or weight.requires_grad or bias.requires_grad)
    use = (not need_grad) if fused is None else bool(fused)
    if use and h.is_cuda:
        return LinearNllFn.apply(h, weight, bias, y, chunk_rows)
    return nll_loss(torch.addmm(bias, h.reshape(-1, h.shape[-1]), weight.t()), y)
