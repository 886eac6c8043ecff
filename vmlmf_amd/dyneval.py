"""Dynamic evaluation (Krause, Kahembwe, Murray, Renals, "Dynamic Evaluation of Neural Sequence Models", 2018): while the language
model (lm.Model) walks a text it takes a small gradient step on every segment it has just predicted, pulled back towards the trained
parameters.  docs/design/lm_dyneval.md has the contract, the kernel and the numbers.

  statistics   ms += g * g behind each of N training minibatches (dropout off), r = sqrt(ms / N) elementwise, m = the mean over the
               parameter tensors of each tensor's mean of r
  step         c    = 1 if max_norm <= 0 else min(1, max_norm / (|g|_2 + 1e-6))        |g|_2 over every gradient of the step
               ld_i = min(decay r_i / m, 1)
               theta_i <- theta_i + ld_i (theta0_i - theta_i) - lr c g_i / (r_i + eps)
               a norm that is not finite skips the step (the parameters keep their bits, the returned norm says so); the gradients
               are never written

  dyneval_accumulate, dyneval_step              the C ABI's vmlmf_dyneval_accumulate / vmlmf_dyneval_step (csrc/vmlmf_optim.hip): one
                                                launch over all tensors, and the norm's two launches plus one update launch
  dyneval_accumulate_stock, dyneval_step_stock  the same formulas in stock ops, on any device: what CPU tensors take, the benchmark's
                                                baseline, the tests' second opinion
  DynamicEval                                   the statistics, the loop over a text and the way back to theta0
"""
from __future__ import annotations

import ctypes
import math

import torch
from torch import nn

from . import _lib
from .optim import _Scratch, _bump_versions, _tensor_lists


def _check_hyper(lr, decay, eps, max_norm):
    ok = all(isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) for v in (lr, decay, eps, max_norm))
    if not ok or lr < 0 or decay < 0 or eps <= 0:
        raise ValueError(f"vmlmf_amd.dyneval: lr >= 0, decay >= 0, eps > 0 and a finite max_norm (<= 0: no clipping); got lr={lr}, "
                         f"decay={decay}, eps={eps}, max_norm={max_norm}")


def _check_fused(tensors, what):
    if len(tensors) < 1 or len(tensors) > _lib.MAX_TENSORS:
        raise ValueError(f"vmlmf_amd.dyneval: 1 .. {_lib.MAX_TENSORS} tensors per call (the norm spans all of them), got {len(tensors)}")
    for t in tensors:
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError(f"vmlmf_amd.dyneval: {what} must be dense float32 tensors on a HIP device (CPU tensors: the _stock form)")


def _check_state(offsets, numels, *flat):
    """The flat buffers must hold [offset, offset + numel) of every tensor: the kernels address them through the offsets unchecked."""
    for f in flat:
        if not (f.is_cuda and f.dtype == torch.float32 and f.is_contiguous() and f.dim() == 1):
            raise RuntimeError("vmlmf_amd.dyneval: the statistics are flat dense float32 buffers on the HIP device")
        for o, n in zip(offsets, numels):
            if o < 0 or o + n > f.numel():
                raise ValueError(f"vmlmf_amd.dyneval: offset {o} + {n} elements lies outside a buffer of {f.numel()}")


@torch.no_grad()
def dyneval_accumulate(grads, ms, offsets):
    """ms[offsets[i] : offsets[i] + grads[i].numel()] += grads[i] ** 2 for every listed gradient, one launch."""
    grads = list(grads)
    _check_fused(grads, "gradients")
    _check_state(offsets, [g.numel() for g in grads], ms)
    dev = grads[0].device
    tl = _tensor_lists([(g, g) for g in grads], list(offsets))[0]      # (the parameter slot is not touched by this launch)
    with _lib.on_device(dev):
        _lib.check(_lib.lib().vmlmf_dyneval_accumulate(ctypes.byref(tl), ms.data_ptr(), _lib.raw_stream(dev)))
    return ms


@torch.no_grad()
def dyneval_step(params, grads, theta0, rms, offsets, *, lr, decay, inv_mean_rms, eps=1e-5, max_norm=0.0, norm=None):
    """The update rule above on params[i] (written in place) from grads[i] (only read) and the flat buffers theta0 and rms, tensor i
    at offsets[i]; inv_mean_rms = 1 / m.  Three launches, no host read: capturable.  Returns |g|_2 as a 0-d device tensor (`norm`
    where given: a captured step writes the same one at every replay)."""
    params, grads = list(params), list(grads)
    _check_hyper(lr, decay, eps, max_norm)
    _check_fused(params, "parameters")
    _check_fused(grads, "gradients")
    if len(params) != len(grads) or any(p.numel() != g.numel() for p, g in zip(params, grads)):
        raise ValueError("vmlmf_amd.dyneval: one gradient of its parameter's size per parameter")
    _check_state(offsets, [p.numel() for p in params], theta0, rms)
    dev = params[0].device
    if norm is None:
        norm = torch.empty((), device=dev, dtype=torch.float32)
    tl = _tensor_lists(list(zip(params, grads)), list(offsets))[0]
    with _lib.on_device(dev):
        _lib.check(_lib.lib().vmlmf_dyneval_step(ctypes.byref(tl), theta0.data_ptr(), rms.data_ptr(), float(lr), float(decay),
                                                 float(inv_mean_rms), float(eps), float(max_norm), norm.data_ptr(),
                                                 _Scratch.get(dev).data_ptr(), _lib.raw_stream(dev)))
    _bump_versions(params)
    return norm


@torch.no_grad()
def dyneval_accumulate_stock(grads, ms):
    """ms[i] += grads[i] ** 2 in stock ops; ms: one tensor per gradient (views of a flat buffer will do)."""
    for g, m in zip(grads, ms):
        m.addcmul_(g.reshape(m.shape), g.reshape(m.shape))
    return ms


@torch.no_grad()
def dyneval_step_stock(params, grads, theta0, rms, *, lr, decay, inv_mean_rms, eps=1e-5, max_norm=0.0):
    """The update rule in stock ops, on whatever device the tensors live on; theta0, rms: one tensor per parameter.  The non-finite
    guard is a select on the device, so this form reads no value back either.  Returns |g|_2 (0-d)."""
    params, grads = list(params), list(grads)
    _check_hyper(lr, decay, eps, max_norm)
    norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads]))
    ok = torch.isfinite(norm)
    s = lr * torch.clamp(max_norm / (norm + 1e-6), max=1.0) if max_norm > 0 else lr
    dm = decay * inv_mean_rms
    for p, g, p0, r in zip(params, grads, theta0, rms):
        p0, r, g = p0.view_as(p), r.view_as(p), g.view_as(p)
        ld = torch.clamp(dm * r, max=1.0)
        p.copy_(torch.where(ok, p + ld * (p0 - p) - s * (g / (r + eps)), p))
    return norm


class DynamicEval:
    """Test-time adaptation of a Model (module docstring: the rule).  lr and decay have no defaults: they are tuned per model.

        de = DynamicEval(model, lr=..., decay=...)      # theta0 = the parameters as they are now
        for x, y in training minibatches: states = de.accumulate(x, y, states)
        de.finalize()                                   # or de.load_state_dict(saved statistics)
        with de:                                        # theta <- theta0 on the way out, whatever is raised
            logprobs, states = de.score(tokens)

    ValueError for lr < 0, decay < 0, eps <= 0, a max_norm that is not finite, segment < 1, more than _lib.MAX_TENSORS parameters (the
    norm spans all of them), parameters that are not dense float32 on one device, and a model with nn.LSTM layers (their backward
    needs train mode; the package's own layers and lstm_type="custom" are covered).  HIP parameters take the fused launches, CPU
    parameters the stock ops (`stock = True` forces those on a HIP device: the benchmark's baseline)."""

    def __init__(self, model, *, lr, decay, eps=1e-5, max_norm=0.0, segment=5):
        _check_hyper(lr, decay, eps, max_norm)
        if isinstance(segment, bool) or not isinstance(segment, int) or segment < 1:
            raise ValueError(f"vmlmf_amd.DynamicEval: segment must be an integer >= 1, got {segment}")
        if any(isinstance(m, nn.LSTM) for m in model.modules()):
            raise ValueError("vmlmf_amd.DynamicEval: nn.LSTM layers run their backward in train mode only; build the Model with the "
                             "package's layers (lstm_type='vmlmf', with_group_layers) or lstm_type='custom'")
        params = list(model.parameters())
        if not 1 <= len(params) <= _lib.MAX_TENSORS:
            raise ValueError(f"vmlmf_amd.DynamicEval: 1 .. {_lib.MAX_TENSORS} parameter tensors (the gradient norm spans all of them), "
                             f"got {len(params)}")
        dev = params[0].device
        if any(p.device != dev or p.dtype != torch.float32 or not p.is_contiguous() for p in params):
            raise ValueError("vmlmf_amd.DynamicEval: dense float32 parameters on one device")
        self.model, self.params = model, params
        self.lr, self.decay, self.eps, self.max_norm, self.segment = float(lr), float(decay), float(eps), float(max_norm), segment
        self.stock = not dev.type == "cuda"
        # every tensor's slice of the flat buffers starts on a 16-byte boundary: the update's wide accesses apply to all of them
        self.offsets, total = [], 0
        for p in params:
            self.offsets.append(total)
            total += (p.numel() + 3) // 4 * 4
        with torch.no_grad():
            self.theta0 = torch.zeros(total, device=dev)
            for p0, p in zip(self._views(self.theta0), params):
                p0.copy_(p)
        self.ms = torch.zeros(total, device=dev)
        self.rms, self.mean_rms, self.minibatches = None, None, 0

    def _views(self, flat):
        return [flat[o:o + p.numel()].view_as(p) for o, p in zip(self.offsets, self.params)]

    # ---- the model under adaptation: eval mode, gradients on, everything put back ----
    class _Adapting:
        def __init__(self, de):
            self.de = de

        def __enter__(self):
            de = self.de
            self.modes = [(m, m.training) for m in de.model.modules()]
            self.req = [p.requires_grad for p in de.params]
            self.grad = torch.is_grad_enabled()
            de.model.train(False)                      # dropout off throughout
            for p in de.params:
                p.requires_grad_(True)
            torch.set_grad_enabled(True)

        def __exit__(self, *exc):
            torch.set_grad_enabled(self.grad)
            for p, was in zip(self.de.params, self.req):
                p.requires_grad_(was)
            for m, was in self.modes:
                m.training = was
            return False

    def _segment(self, x, y, states):
        """One minibatch or segment: gradients freed, Model.loss at its defaults with the loss launch's own rows, backward.  Returns
        (rows, detached states)."""
        from .functional import lm_head_loss, unit_gradient
        model = self.model
        for p in self.params:
            p.grad = None
        states = [(hh.detach(), cc.detach()) for hh, cc in states]
        tied = model._tied_gradient(x) if hasattr(model, "_tied_gradient") else None     # a tied table: one gradient, no table-wide add
        h, states = model.features(x, states) if tied is None else model._features(x, states, grad_from=tied)[:2]
        loss, rows = lm_head_loss(h, model.fc.w, model.fc.b, y, return_rows=True, grad_to=tied)
        loss.backward(unit_gradient(loss.device))
        return rows, model.detach(states)

    def _check_text(self, x, y, who):
        if not (isinstance(x, torch.Tensor) and x.dim() == 2 and x.dtype == torch.int64 and x.shape[0] >= 1
                and isinstance(y, torch.Tensor) and y.dtype == torch.int64 and y.shape == x.shape):
            raise ValueError(f"vmlmf_amd.DynamicEval.{who}: (T, B) int64 inputs and targets of one shape, time-major, T >= 1")
        if x.device != self.theta0.device or y.device != x.device:
            raise RuntimeError(f"vmlmf_amd.DynamicEval.{who}: the text must live on the model's device {self.theta0.device}")

    # ---- statistics ----
    def accumulate(self, x, y, states=None):
        """One training minibatch (x, y (T, B) int64 as lm_test.minibatch hands them out): Model.loss at its defaults with dropout
        off, backward, ms += g * g.  Returns the detached states for the next minibatch.  RuntimeError after finalize()."""
        if self.rms is not None:
            raise RuntimeError("vmlmf_amd.DynamicEval.accumulate: the statistics are final (finalize() or load_state_dict())")
        self._check_text(x, y, "accumulate")
        states = self.model.state_init(x.shape[1]) if states is None else list(states)
        with self._Adapting(self):
            _, states = self._segment(x, y, states)
        grads = self._grads()
        if self.stock:
            dyneval_accumulate_stock([g for _, g in grads], [self._views(self.ms)[i] for i, _ in grads])
        else:
            dyneval_accumulate([g for _, g in grads], self.ms, [self.offsets[i] for i, _ in grads])
        self.minibatches += 1
        return states

    @torch.no_grad()
    def finalize(self):
        """r = sqrt(ms / N) and m (one host read, once per model); accumulate() afterwards raises."""
        if self.rms is not None:
            return
        if self.minibatches < 1:
            raise RuntimeError("vmlmf_amd.DynamicEval.finalize: no minibatch has been accumulated")
        rms = torch.sqrt(self.ms / float(self.minibatches))
        mean = float(torch.stack([r.mean() for r in self._views(rms)]).mean())
        if not (math.isfinite(mean) and mean > 0):
            raise RuntimeError(f"vmlmf_amd.DynamicEval.finalize: the mean RMS gradient is {mean}: nothing to scale the decay by")
        self.rms, self.mean_rms = rms, mean

    def state_dict(self):
        """The statistics (not theta0, not the hyper-parameters): collected once per checkpoint."""
        return {"minibatches": self.minibatches, "ms": [m.clone() for m in self._views(self.ms)],
                "rms": None if self.rms is None else [r.clone() for r in self._views(self.rms)], "mean_rms": self.mean_rms}

    @torch.no_grad()
    def load_state_dict(self, d):
        """ValueError unless d is another DynamicEval's state_dict() for a model of the same parameter shapes."""
        for key in ("ms", "rms"):
            if d[key] is not None and (len(d[key]) != len(self.params)
                                       or any(tuple(t.shape) != tuple(p.shape) for t, p in zip(d[key], self.params))):
                raise ValueError(f"vmlmf_amd.DynamicEval.load_state_dict: '{key}' does not match the model's parameter shapes")
        if (d["rms"] is None) != (d["mean_rms"] is None):
            raise ValueError("vmlmf_amd.DynamicEval.load_state_dict: rms and mean_rms come together")
        for dst, src in zip(self._views(self.ms), d["ms"]):
            dst.copy_(src)
        self.minibatches = int(d["minibatches"])
        self.rms, self.mean_rms = None, None
        if d["rms"] is not None:
            self.rms = torch.zeros_like(self.ms)
            for dst, src in zip(self._views(self.rms), d["rms"]):
                dst.copy_(src)
            self.mean_rms = float(d["mean_rms"])

    # ---- the update ----
    def _grads(self):
        """[(index, contiguous gradient)] of the parameters that have one."""
        out = []
        for i, p in enumerate(self.params):
            if p.grad is not None:
                if p.grad.dtype != torch.float32 or p.grad.device != p.device:
                    raise RuntimeError("vmlmf_amd.DynamicEval: float32 gradients on the parameters' device")
                out.append((i, p.grad if p.grad.is_contiguous() else p.grad.contiguous()))
        return out

    @torch.no_grad()
    def step(self):
        """The update from the parameters' current .grad (parameters without one are left alone, and out of the norm): what score()
        calls behind every segment.  Returns |g|_2 before clipping as a 0-d tensor on the device; nothing is read back."""
        if self.rms is None:
            raise RuntimeError("vmlmf_amd.DynamicEval.step: no statistics yet (accumulate() ... finalize(), or load_state_dict())")
        grads = self._grads()
        dev = self.theta0.device
        if not grads:
            return torch.zeros((), device=dev)
        hyper = dict(lr=self.lr, decay=self.decay, inv_mean_rms=1.0 / self.mean_rms, eps=self.eps, max_norm=self.max_norm)
        live = [self.params[i] for i, _ in grads]
        if self.stock:
            theta0, rms = self._views(self.theta0), self._views(self.rms)
            return dyneval_step_stock(live, [g for _, g in grads], [theta0[i] for i, _ in grads], [rms[i] for i, _ in grads], **hyper)
        return dyneval_step(live, [g for _, g in grads], self.theta0, self.rms, [self.offsets[i] for i, _ in grads], **hyper)

    def score(self, tokens, targets=None, states=None):
        """Model.score's text contract: targets=None takes (T + 1, B) int64 tokens, time-major (inputs tokens[:-1], targets
        tokens[1:]); otherwise tokens and targets are both (T, B).  Returns (logprobs (T, B) fp32, states).  The text is walked in
        segments of `segment` positions (the last may be shorter): each is scored with the CURRENT parameters - logprobs are the
        predictions before the adaptation they cause, the negated rows of the head-loss launch -, then backward and step().  The
        step follows every segment, the last included, so calls on consecutive chunks (states handed on) compose to the call on the
        whole text.  Dropout is off; every module's train / eval flag, every requires_grad and the autograd mode are as the caller
        left them afterwards, whatever is raised.  The parameters stay adapted: restore() or `with de:` takes them back.  No value
        is read back from the device."""
        if not (isinstance(tokens, torch.Tensor) and tokens.dim() == 2 and tokens.dtype == torch.int64):
            raise ValueError("vmlmf_amd.DynamicEval.score takes (T, B) int64 tokens, time-major")
        if targets is None:
            if tokens.shape[0] < 2:
                raise ValueError(f"vmlmf_amd.DynamicEval.score without targets takes (T + 1, B) tokens, T >= 1; got {tuple(tokens.shape)}")
            x, y = tokens[:-1], tokens[1:]
        else:
            x, y = tokens, targets
        self._check_text(x, y, "score")
        if self.rms is None:
            raise RuntimeError("vmlmf_amd.DynamicEval.score: no statistics yet (accumulate() ... finalize(), or load_state_dict())")
        T, B = x.shape
        states = self.model.state_init(B) if states is None else list(states)
        logprobs = torch.empty((T, B), device=x.device, dtype=torch.float32)
        with self._Adapting(self):
            for lo in range(0, T, self.segment):
                hi = min(lo + self.segment, T)
                rows, states = self._segment(x[lo:hi], y[lo:hi].contiguous(), states)
                torch.neg(rows.view(hi - lo, B), out=logprobs[lo:hi])
                self.step()
        for p in self.params:
            p.grad = None
        return logprobs, states

    @torch.no_grad()
    def restore(self):
        """theta <- theta0, bit for bit."""
        for p, p0 in zip(self.params, self._views(self.theta0)):
            p.copy_(p0)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.restore()
        return False
