"""Optimizer steps of the reference's two training loops as single launches over all parameter tensors.

  Adam            drop-in for torch.optim.Adam(model.parameters(), lr=...)      V/src/train_test/train.py:47,65
  clip_sgd_step   clip_grad_norm_(params, max_norm) + `param -= lr * param.grad` V/src/train_test/lm_test.py:203-209
  ASGD            NT-ASGD for the language model: clip_sgd_step with L2 weight decay and, once switched on, the average of the
                  iterates (clip_grad_norm_ + torch.optim.ASGD(lambd=0)); asgd_step / asgd_step_stock underneath, the latter the
                  one form here that also takes CPU tensors.  docs/design/lm_asgd.md

The models are 10-20 small tensors: the stock optimizer costs ~2 ms of dispatcher time per step at the headline
shape, ten times the forward + backward it follows.  Here one kernel walks every tensor (pointers travel in the
kernel arguments); the step counters live on the device, so a whole training step can sit in one hipGraph.
SURVEY.md section 8f ("next" row).  HIP tensors only; anything else raises (no CPU path).
"""
from __future__ import annotations

import contextlib
import ctypes
import math

import torch

from . import _lib


def _tensor_lists(pairs, offsets, step_index=None):
    """[(param, grad)] -> ctypes TensorList structs of at most MAX_TENSORS entries each."""
    out = []
    for lo in range(0, len(pairs), _lib.MAX_TENSORS):
        tl = _lib.TensorList()
        chunk = pairs[lo:lo + _lib.MAX_TENSORS]
        for i, (p, g) in enumerate(chunk):
            tl.param[i], tl.grad[i] = p.data_ptr(), g.data_ptr()
            tl.numel[i], tl.state_offset[i] = p.numel(), offsets[lo + i]
            tl.step_index[i] = 0 if step_index is None else step_index[lo + i]
        tl.count = len(chunk)
        out.append(tl)
    return out


def _check(p, g):
    if not (p.is_cuda and g.is_cuda):
        raise RuntimeError("vmlmf_amd.optim: parameters and gradients must live on a HIP device (no CPU path)")
    if p.dtype != torch.float32 or g.dtype != torch.float32 or not p.is_contiguous():
        raise RuntimeError("vmlmf_amd.optim: dense float32 parameters only")


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam semantics (betas, eps, L2 weight_decay; no amsgrad / maximize), one launch per step and
    parameter group.  state[p] holds 'step', 'exp_avg', 'exp_avg_sq' like the stock optimizer (the moments are
    views of two flat buffers per group).
    Non-finite gradients of the VMLMF layers never reach the parameters: the library's backward marks a per-device health word
    when it writes an Inf / NaN parameter gradient (a launch that gave up a bounded wait, VMLMF_E_PROTOCOL, leaves NaN gradients, and
    a replayed hipGraph cannot ask the host), this optimizer's tick launch reads it and skips the whole step; skipped_steps()
    counts.  vmlmf_amd._lib.tune("adam_guard", 2) scans every gradient instead (any source, one more launch); guard=False: the
    unguarded launch."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, guard=True):
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._guarded = bool(guard)

    def skipped_steps(self):
        """Optimizer steps the device-side gate refused because a gradient was not finite (synchronises)."""
        g = getattr(self, "_guard", None)
        return 0 if g is None else int(g[_lib.GUARD_SKIPPED].item())

    def _group_state(self, gi, group):
        """Flat moment buffers covering every parameter of the group (allocated at the first step; kept out of
        param_groups so that state_dict() stays what torch.optim.Adam's is)."""
        if not hasattr(self, "_flat"):
            self._flat = {}
        gs = self._flat.get(gi)
        if gs is None:
            self._step_cache = None   # (new moment buffers: the remembered argument blocks point at the old ones)
            ps = group["params"]
            dev = ps[0].device
            total, offs, sidx = 0, {}, {}
            for k, p in enumerate(ps):
                offs[p], sidx[p] = total, k
                total += p.numel()
            gs = dict(m=torch.zeros(total, device=dev), v=torch.zeros(total, device=dev),
                      steps=torch.zeros(len(ps), device=dev), offs=offs, sidx=sidx)
            # ONE guard block for the whole optimizer: the verdict on a step's gradients is taken once, by the first launch of the
            # step, and holds for every tensor list and parameter group of that step
            if getattr(self, "_guarded", True) and getattr(self, "_guard", None) is None:
                self._guard = torch.zeros(_lib.GUARD_WORDS, device=dev, dtype=torch.int32)
            self._flat[gi] = gs
            for p in ps:
                self._adopt(gs, p, fresh=True)
        return gs

    @torch.no_grad()
    def _adopt(self, gs, p, fresh=False):
        """state[p] becomes p's views of the group's flat buffers, holding what state[p] held before: the moments and step count of a
        loaded checkpoint (also one written by torch.optim.Adam), zeros where it held none - where a fresh optimizer starts (`fresh`:
        the buffers are new zeros already)."""
        o, n = gs["offs"][p], p.numel()
        new = dict(step=gs["steps"][gs["sidx"][p]], exp_avg=gs["m"][o:o + n].view_as(p), exp_avg_sq=gs["v"][o:o + n].view_as(p))
        old = self.state.get(p) or {}
        for k in ("exp_avg", "exp_avg_sq"):
            if k in old:
                new[k].copy_(old[k].to(device=new[k].device, dtype=torch.float32).view_as(p))
            elif not fresh:
                new[k].zero_()
        if "step" in old:
            new["step"].fill_(float(old["step"]))
        elif not fresh:
            new["step"].zero_()
        self.state[p] = new

    def load_state_dict(self, state_dict):
        """As torch.optim.Optimizer.load_state_dict.  A group whose flat buffers exist gets the loaded moments and step counts
        copied INTO them, and zeros for parameters without loaded state (an empty state_dict() resets to a fresh optimizer): the
        buffers keep their addresses, so the argument blocks step() remembers and a GraphedTrainStep's captured graph stay valid.
        A group without buffers yet gets them now when it has loaded state."""
        super().load_state_dict(state_dict)
        # converted NOW, not at the next step(): torch hands the checkpoint's own tensors through when device and dtype
        # already match, so a lazily read state would follow whatever the checkpoint's owner does to them meanwhile
        flat = self.__dict__.get("_flat") or {}
        self._flat = {}
        for gi, group in enumerate(self.param_groups):
            gs, ps = flat.get(gi), group["params"]
            if gs is not None and len(gs["offs"]) == len(ps) and all(a is b for a, b in zip(gs["offs"], ps)):
                self._flat[gi] = gs
                for p in ps:
                    self._adopt(gs, p)
                continue
            if gs is not None:
                self._step_cache = None   # (the group's old buffers are dropped: no remembered argument block may point at them)
            if any(self.state.get(p) for p in ps):
                self._group_state(gi, group)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.lib()
        # The step's launches are a pure function of the addresses involved and the groups' hyper-parameters: when neither has changed
        # since the last step (the usual case: backward hands the same allocator blocks back, step after step) the argument blocks
        # built then are used again - the Python below costs 2-3x the launch it prepares (host path: tools/probes/host_path.py).
        key = []
        for group in self.param_groups:
            key.append((group["lr"], group["betas"], group["eps"], group["weight_decay"]))
            for p in group["params"]:
                g = p.grad
                key.append(None if g is None else (p.data_ptr(), g.data_ptr(), g.is_contiguous()))
        key = tuple(key)
        cached = self.__dict__.get("_step_cache")
        if cached is not None and cached[0] == key and all(k[2] for k in key if k is not None and len(k) == 3):
            for args, live in cached[1]:
                with _lib.on_device(live[0].device):
                    _lib.check(lib.vmlmf_adam_step_ex(*args[:-1], _lib.raw_stream(live[0].device)))
                _bump_versions(live)
            return loss
        # every launch of the step first (tensor lists of every group), then FIRST on the first and LAST on the last of them: one
        # verdict on the step's gradients for all of them (include/vmlmf_hip.h: vmlmf_adam_step_ex)
        calls = []
        for gi, group in enumerate(self.param_groups):
            live = [p for p in group["params"] if p.grad is not None]
            if not live:
                continue
            gs = self._group_state(gi, group)
            pairs = []
            for p in live:
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                _check(p, g)
                pairs.append((p, g))
            for tl in _tensor_lists(pairs, [gs["offs"][p] for p in live], [gs["sidx"][p] for p in live]):
                calls.append((tl, gs, group, live, pairs))   # pairs: the .contiguous() copies live until their launch is issued
        guard = getattr(self, "_guard", None)
        kept = []
        for ci, (tl, gs, group, live, _keep) in enumerate(calls):
            dev = live[0].device
            b1, b2 = group["betas"]
            flags = (_lib.ADAM_FIRST if ci == 0 else 0) | (_lib.ADAM_LAST if ci == len(calls) - 1 else 0)
            args = (ctypes.byref(tl), gs["m"].data_ptr(), gs["v"].data_ptr(), gs["steps"].data_ptr(), float(group["lr"]), float(b1),
                    float(b2), float(group["eps"]), float(group["weight_decay"]), None if guard is None else guard.data_ptr(), flags,
                    _lib.raw_stream(dev))
            with _lib.on_device(dev):
                _lib.check(lib.vmlmf_adam_step_ex(*args))
            _bump_versions(live)
            kept.append((args + (tl,), live))   # (tl keeps the struct byref points at alive; the stream is taken anew at every step)
        # (only steps whose gradients were all contiguous are remembered: a .contiguous() copy has a new address every step anyway)
        self._step_cache = (key, [(a[:-1], live) for a, live in kept], [a[-1] for a, _ in kept])
        return loss


def _bump_versions(params):
    """The kernels write parameters through raw pointers: tell autograd's version counters (kept parameter images,
    functional.PackCache, and any saved-tensor check key on them) that the tensors changed in place."""
    for p in params:
        torch.autograd.graph.increment_version(p)


class _Scratch:
    bufs = {}

    @classmethod
    def get(cls, dev):
        b = cls.bufs.get(dev)
        if b is None:
            b = cls.bufs[dev] = torch.empty(_lib.MAX_TENSORS * 64 + 1, device=dev)
        return b


@torch.no_grad()
def clip_sgd_step(parameters, lr, max_norm):
    """The LM loop's update (lm_test.py:203-209): norm = clip_grad_norm_(parameters, max_norm); p -= lr * p.grad.
    Returns the total gradient norm before clipping as a 0-d device tensor (what clip_grad_norm_ returns).
    A norm that is not finite (NaN gradients of a launch that gave up a bounded wait; an overflow) skips the step on the device:
    parameters and gradients keep their values and the returned norm says so."""
    live = [p for p in parameters if p.grad is not None]
    if not live:
        return torch.zeros(())
    if len(live) > _lib.MAX_TENSORS:
        raise RuntimeError(f"clip_sgd_step: at most {_lib.MAX_TENSORS} tensors (the norm spans all of them)")
    for p in live:
        _check(p, p.grad)
        if not p.grad.is_contiguous():
            raise RuntimeError("clip_sgd_step scales the gradients in place: they must be contiguous")
    dev = live[0].device
    scratch = _Scratch.get(dev)
    norm = torch.empty((), device=dev)
    tl = _tensor_lists([(p, p.grad) for p in live], [0] * len(live))[0]
    stream = _lib.raw_stream(dev)
    with _lib.on_device(dev):
        _lib.check(_lib.lib().vmlmf_sgd_clip_step(ctypes.byref(tl), float(lr), float(max_norm), norm.data_ptr(),
                                                  scratch.data_ptr(), stream))
    _bump_versions(live)
    return norm


# ---- NT-ASGD (Merity, Keskar, Socher, "Regularizing and Optimizing LSTM Language Models"; docs/design/lm_asgd.md) ----
#   c   = 1 if max_norm <= 0 else min(1, max_norm / (|g|_2 + 1e-6))      |g|_2 over every gradient of the step (clip_sgd_step's)
#   g'  = c g                         written back into the gradient when c < 1
#   p'  = p - lr (g' + wd p)
#   n   = k - 1 - t0                  k: this applied step (1-based, counted on the device), t0: the count at start_averaging()
#   ax' = ax while averaging is off | p' (a copy) when n <= 1 | ax + (p' - ax) (1 / n) when n >= 2
# torch.optim.ASGD(lambd=0, t0=t0, weight_decay=wd) behind clip_grad_norm_, its fp32 mu included.  A norm that is not finite skips
# the step on the device: p, g, ax and the step count keep their bits and the returned norm says so.
def _check_asgd_hyper(lr, weight_decay, max_norm):
    for name, v in (("lr", lr), ("weight_decay", weight_decay), ("max_norm", max_norm)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"vmlmf_amd.optim.ASGD: {name} must be a finite number >= 0 (max_norm 0: no clipping), got {v!r}")


def new_asgd_state(device):
    """vmlmf_asgd_step's state block (include/vmlmf_hip.h) of a fresh optimizer: no step applied, averaging off."""
    words = [0] * _lib.ASGD_WORDS
    words[_lib.ASGD_T0] = _lib.ASGD_T0_OFF
    return torch.tensor(words, dtype=torch.int32, device=device)


def _check_asgd_lists(params, grads, ax, state, offsets):
    if not 1 <= len(params) <= _lib.MAX_TENSORS:
        raise ValueError(f"vmlmf_amd.optim.asgd_step: 1 .. {_lib.MAX_TENSORS} tensors per call (the norm spans all of them), got {len(params)}")
    if len(params) != len(grads) or len(params) != len(offsets) or any(p.numel() != g.numel() for p, g in zip(params, grads)):
        raise ValueError("vmlmf_amd.optim.asgd_step: one gradient of its parameter's size and one offset per parameter")
    if ax.dtype != torch.float32 or ax.dim() != 1 or not ax.is_contiguous():
        raise RuntimeError("vmlmf_amd.optim.asgd_step: ax is one flat dense float32 buffer")
    if state.dtype != torch.int32 or state.dim() != 1 or state.numel() < _lib.ASGD_WORDS or not state.is_contiguous():
        raise RuntimeError(f"vmlmf_amd.optim.asgd_step: the state block is {_lib.ASGD_WORDS} dense int32 words")
    for o, p in zip(offsets, params):            # the kernel addresses ax through the offsets unchecked
        if o < 0 or o + p.numel() > ax.numel():
            raise ValueError(f"vmlmf_amd.optim.asgd_step: offset {o} + {p.numel()} elements lies outside a buffer of {ax.numel()}")


@torch.no_grad()
def asgd_step(params, grads, ax, state, offsets, *, lr, weight_decay=0.0, max_norm=0.0, norm=None):
    """The rule above on params[i] and grads[i] (both written in place), the flat buffer ax (tensor i at offsets[i]) and the state
    block (new_asgd_state): vmlmf_asgd_step's three launches, no host read, so it captures.  Returns |g|_2 before clipping as a
    0-d device tensor (`norm` where given: a captured step writes the same one at every replay)."""
    params, grads, offsets = list(params), list(grads), list(offsets)
    _check_asgd_hyper(lr, weight_decay, max_norm)
    _check_asgd_lists(params, grads, ax, state, offsets)
    for p, g in zip(params, grads):
        _check(p, g)
        if not g.is_contiguous():
            raise RuntimeError("vmlmf_amd.optim.asgd_step scales the gradients in place: they must be contiguous")
    dev = params[0].device
    if not (ax.is_cuda and state.is_cuda):
        raise RuntimeError("vmlmf_amd.optim.asgd_step: ax and the state block live on the parameters' HIP device (CPU: asgd_step_stock)")
    if norm is None:
        norm = torch.empty((), device=dev, dtype=torch.float32)
    tl = _tensor_lists(list(zip(params, grads)), offsets)[0]
    with _lib.on_device(dev):
        _lib.check(_lib.lib().vmlmf_asgd_step(ctypes.byref(tl), ax.data_ptr(), state.data_ptr(), float(lr), float(weight_decay),
                                              float(max_norm), norm.data_ptr(), _Scratch.get(dev).data_ptr(), _lib.raw_stream(dev)))
    _bump_versions(params)
    return norm


@torch.no_grad()
def asgd_step_stock(params, grads, ax, state, offsets, *, lr, weight_decay=0.0, max_norm=0.0, norm=None):
    """asgd_step in stock ops, on whatever device the tensors live on: what CPU tensors take and the benchmark's baseline.  Every
    decision - the non-finite guard, the clip, off / copy / average - is a select on the device, so this form reads no value back
    either (unlike the kernel it rewrites unchanged values with their own bits)."""
    params, grads, offsets = list(params), list(grads), list(offsets)
    _check_asgd_hyper(lr, weight_decay, max_norm)
    _check_asgd_lists(params, grads, ax, state, offsets)
    total = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads]))
    ok = torch.isfinite(total)
    c = torch.clamp(max_norm / (total + 1e-6), max=1.0) if max_norm > 0 else torch.ones_like(total)
    k, t0 = state[_lib.ASGD_STEP] + 1, state[_lib.ASGD_T0]
    n = k - 1 - t0
    on, average = t0 >= 0, (t0 >= 0) & (n >= 2)
    mu = torch.where(average, 1.0 / n.clamp(min=1).to(torch.float32), torch.ones_like(total))
    for p, g, o in zip(params, grads, offsets):
        a = ax[o:o + p.numel()].view_as(p)
        gc = g.view_as(p) * c
        pn = p - lr * (gc + weight_decay * p)
        an = torch.where(average, a + (pn - a) * mu, pn)
        g.copy_(torch.where(ok, gc, g.view_as(p)).view_as(g))       # (c == 1: the same bits)
        a.copy_(torch.where(ok & on, an, a))
        p.copy_(torch.where(ok, pn, p))
    # the block's words as device tensors throughout (a Python number assigned into a device tensor is a host copy: not capturable)
    scalars = torch.stack([c, mu]).to(torch.float32).view(torch.int32)
    new, skipped = list(state.unbind()), list(state.unbind())
    new[_lib.ASGD_STEP], new[_lib.ASGD_COEF], new[_lib.ASGD_MU] = k, scalars[0], scalars[1]
    new[_lib.ASGD_GO] = torch.ones_like(k)
    new[_lib.ASGD_MODE] = on.to(torch.int32) + average.to(torch.int32)         # ASGD_MODE_OFF / _COPY / _AVERAGE = 0 / 1 / 2
    skipped[_lib.ASGD_GO] = torch.zeros_like(k)
    state.copy_(torch.where(ok, torch.stack(new), torch.stack(skipped)))
    if norm is None:
        return total
    norm.copy_(total)
    return norm


class ASGD(torch.optim.Optimizer):
    """NT-ASGD for a language model (the rule above): SGD with gradient clipping and L2 weight decay that, once the validation metric
    has stopped improving, also keeps the average of the iterates - the parameters that are evaluated and saved.

        opt = vmlmf_amd.optim.ASGD(model.parameters(), lr=30.0, weight_decay=1.2e-6, max_norm=0.25, nonmono=5)
        ... loss.backward(); opt.step() ...                      # one fused step: clip, decay, SGD, average (three launches)
        with opt.averaged():                                     # the parameters hold the average in here (before averaging
            val = validate(model)                                # has started: evaluate the plain model instead)
        opt.observe(val)                                         # the non-monotone trigger; start_averaging() switches by hand

    One parameter group; the gradient norm spans every tensor.  lr, weight_decay and max_norm are read from param_groups[0] at every
    step.  ValueError, before any device work, for a negative or non-finite lr, weight_decay or max_norm, nonmono < 1, more than
    _lib.MAX_TENSORS tensors, parameters that are not dense float32 on one device, or more than one group.  ax and the state block are
    created here and never reallocated, and the step reads nothing back: a captured step goes on working across start_averaging()
    and load_state_dict(), which write those device buffers (lr, weight_decay and max_norm are launch arguments: a captured step
    keeps the values it was captured with).
    HIP parameters take the fused launches, CPU parameters the stock ops (`stock = True` forces those on a HIP device)."""

    def __init__(self, params, lr, weight_decay=0.0, max_norm=0.0, nonmono=5):
        _check_asgd_hyper(lr, weight_decay, max_norm)
        if isinstance(nonmono, bool) or not isinstance(nonmono, int) or nonmono < 1:
            raise ValueError(f"vmlmf_amd.optim.ASGD: nonmono must be an integer >= 1, got {nonmono!r}")
        params = list(params)
        if any(not isinstance(p, torch.Tensor) for p in params):
            raise ValueError("vmlmf_amd.optim.ASGD takes one group of parameter tensors (the norm spans all of them)")
        if not 1 <= len(params) <= _lib.MAX_TENSORS:
            raise ValueError(f"vmlmf_amd.optim.ASGD: 1 .. {_lib.MAX_TENSORS} parameter tensors (the gradient norm spans all of them), "
                             f"got {len(params)}")
        dev = params[0].device
        if any(p.device != dev or p.dtype != torch.float32 or p.is_sparse or not p.is_contiguous() for p in params):
            raise ValueError("vmlmf_amd.optim.ASGD: dense float32 parameters on one device")
        super().__init__(params, dict(lr=lr, weight_decay=weight_decay, max_norm=max_norm))
        self.nonmono, self.history, self.averaging = nonmono, [], False
        self.stock = dev.type != "cuda"
        # every tensor's slice of ax starts on a 16-byte boundary: the update's wide accesses apply to all of them
        self._params, self._offsets, total = params, [], 0
        for p in params:
            self._offsets.append(total)
            total += (p.numel() + 3) // 4 * 4
        self.ax = torch.zeros(total, device=dev)
        self._words = new_asgd_state(dev)
        self.last_norm = torch.zeros((), device=dev)
        if not self.stock:
            _Scratch.get(dev)            # (allocated now, not inside somebody's graph capture)

    def add_param_group(self, param_group):
        if self.param_groups:
            raise ValueError("vmlmf_amd.optim.ASGD has one parameter group: the norm, ax and the step count span all its tensors")
        super().add_param_group(param_group)

    def ax_views(self):
        """The average of each parameter: views of the flat buffer, in the parameters' order and shapes."""
        return [self.ax[o:o + p.numel()].view_as(p) for o, p in zip(self._offsets, self._params)]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self.param_groups[0]
        lr, wd, max_norm = group["lr"], group["weight_decay"], group["max_norm"]
        _check_asgd_hyper(lr, wd, max_norm)
        live = [i for i, p in enumerate(self._params) if p.grad is not None]       # parameters without a gradient are skipped
        if not live:
            return loss
        params, grads = [self._params[i] for i in live], [self._params[i].grad for i in live]
        for p, g in zip(params, grads):
            if g.dtype != torch.float32 or g.device != p.device or g.is_sparse or not g.is_contiguous():
                raise RuntimeError("vmlmf_amd.optim.ASGD scales the gradients in place: contiguous dense float32 on the parameters' device")
        fn = asgd_step_stock if self.stock else asgd_step
        fn(params, grads, self.ax, self._words, [self._offsets[i] for i in live], lr=lr, weight_decay=wd, max_norm=max_norm,
           norm=self.last_norm)       # (asgd_step bumps the versions behind its raw-pointer writes; the stock ops bump their own)
        return loss

    def clip_step(self, parameters, lr, max_norm):
        """LmDataParallel's update_fn: clip_sgd_step's signature.  Sets the two values and steps (`parameters` are the optimizer's own);
        returns the norm."""
        self.param_groups[0]["lr"], self.param_groups[0]["max_norm"] = lr, max_norm
        self.step()
        return self.last_norm

    @torch.no_grad()
    def start_averaging(self):
        """From the next step on ax follows the parameters: t0 <- the device's step word (device to device, nothing is read back - a
        captured step goes on working), ax <- the parameters."""
        self._words[_lib.ASGD_T0:_lib.ASGD_T0 + 1].copy_(self._words[_lib.ASGD_STEP:_lib.ASGD_STEP + 1])
        for a, p in zip(self.ax_views(), self._params):
            a.copy_(p)
        self.averaging = True

    def observe(self, metric):
        """The non-monotone trigger as AWD-LSTM writes it: call with each validation metric (lower is better).  Returns whether
        averaging is on."""
        if not self.averaging and len(self.history) > self.nonmono and metric > min(self.history[:-self.nonmono]):
            self.start_averaging()
        self.history.append(float(metric))
        return self.averaging

    @torch.no_grad()
    def _exchange(self):
        for a, p in zip(self.ax_views(), self._params):
            held = p.detach().clone()
            p.copy_(a)
            a.copy_(held)
        _bump_versions(self._params)

    @contextlib.contextmanager
    def averaged(self):
        """Inside, the parameters hold ax and ax holds the parameters (an exchange: no third copy is kept); on the way out they are
        exchanged back, bit for bit, whatever is raised.  Versions are bumped both ways.  RuntimeError before start_averaging()."""
        if not self.averaging:
            raise RuntimeError("vmlmf_amd.optim.ASGD.averaged: averaging has not started (start_averaging(), or observe())")
        self._exchange()
        try:
            yield self
        finally:
            self._exchange()

    def state_dict(self):
        """ax per parameter, the step count, t0 (-1: off), the trigger's history and flag, the group's values (one host read)."""
        words = self._words.tolist()
        return {"ax": [a.clone() for a in self.ax_views()], "step": words[_lib.ASGD_STEP], "t0": words[_lib.ASGD_T0],
                "history": list(self.history), "averaging": self.averaging, "nonmono": self.nonmono,
                "param_groups": [{k: v for k, v in self.param_groups[0].items() if k != "params"}]}

    @torch.no_grad()
    def load_state_dict(self, d):
        """Copies INTO the existing buffers (a captured graph sees the loaded state).  ValueError unless d is another ASGD's
        state_dict() for parameters of the same shapes."""
        if len(d["ax"]) != len(self._params) or any(tuple(t.shape) != tuple(p.shape) for t, p in zip(d["ax"], self._params)):
            raise ValueError("vmlmf_amd.optim.ASGD.load_state_dict: 'ax' does not match the parameters' shapes")
        for dst, src in zip(self.ax_views(), d["ax"]):
            dst.copy_(src)
        words = self._words.tolist()
        words[_lib.ASGD_STEP], words[_lib.ASGD_T0] = int(d["step"]), int(d["t0"])
        self._words.copy_(torch.tensor(words, dtype=torch.int32))
        self.history, self.averaging, self.nonmono = [float(v) for v in d["history"]], bool(d["averaging"]), int(d["nonmono"])
        for k, v in d["param_groups"][0].items():
            self.param_groups[0][k] = v
