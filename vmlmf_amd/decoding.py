"""Decoding the language model (lm.Model): what stands behind Model.generate, Model.beam_search, Model.group_beam_search and Model.contrastive_search.  The reference has no decoder;
lm.py holds its layers, this module everything that continues a prompt with them.

  lm_sample, sample_filters                  the head and the choice of the next token in one launch (C ABI: vmlmf_lm_sample ...)
  lm_beam_step, beam_gather, beam_backtrack  the beam step, the state reorder and the read-back (_beam.py, a library of its own)
  decode_steps, beam_steps                   the step loops: a choice, then the layers at T = 1 - no host synchronisation
  DecodeGraph, BeamGraph                     those loops captured into a hipGraph
  (a beam step that differs from the plain one is a _beam.BeamPolicy - BeamControls, AutomatonBeamControls, GroupBeams,
   StochasticBeams -: beam_steps and BeamGraph are written once, against that protocol)
  generate, beam_search, group_beam_search   the calls behind Model's methods of the same names, where the contract is written down
  lm_contrast_step, contrast_steps, ContrastGraph, contrastive_search    contrastive search: the step's one launch (_contrast.py, a
                                             library of its own), its loop, the loop captured, the call behind Model.contrastive_search
  lm_sbeam_step, StochasticBeams, StochasticBeamGraph, stochastic_beam_search    stochastic beam search - sequences sampled without
                                             replacement: the step's one launch (_sbeam.py, a library of its own), the policy that
                                             puts it into beam_steps, a BeamGraph under that policy, the call behind
                                             Model.stochastic_beam_search
(scoring.py - Model.score - runs on this module's session too.)
"""
from __future__ import annotations

import contextlib

import torch

from . import _automaton, _beam, _beamctl, _beamgroup, _contrast, _decode, _history, _lib, _sbeam, _truncate
from ._automaton import AutomatonBeamControls, AutomatonControls, TokenAutomaton  # noqa: F401
from ._beam import lm_beam_step, beam_gather, beam_backtrack  # noqa: F401
from ._beamctl import BeamControls
from ._beamgroup import GroupBeams
from ._contrast import ContrastControls, lm_contrast_step
from ._decode import DecodeControls
from ._history import HistoryControls
from ._sbeam import StochasticBeams, lm_sbeam_step
from ._lib import ptr
from ._truncate import Truncation
from .functional import PackCache, _require_hip, _workspace, dropout_advance, sample_ticket
from .lm import stack_layers


# ---- head + token choice in one launch per token (C ABI: vmlmf_lm_sample; csrc/vmlmf_sample.hip) ---------------------------------
def _sample_workspace(dev, nbytes):
    return _workspace(dev, nbytes, "sample")


SAMPLE_FUSED_MAX_ROWS = 4   # measured at the PTB size: fused 25.6 us against 37.2 at 1 row, 40.5 against 37.8 at 8 (lm_sampling.md)
# ... with a filter on (top_k / top_p) the fused launch's last workgroup selects and chooses its rows one after the other, 256 threads
# a row; the choice launch behind the GEMM gives every row 1024.  Measured at the PTB size, top_k 40 / top_p 0.9 / both: fused 87.5 /
# 105.9 / 125.6 us at 1 row against 47.4 / 56.7 / 65.4 for GEMM + choice (291 / 364 / 445 against 47.9 / 57.3 / 66.1 at 4 rows): the GEMM
# form at every width; form="fused" still reaches the one-launch form (lm_sampling.md)
SAMPLE_FILTERED_FUSED_MAX_ROWS = 0


def sample_filters(top_k, top_p, V=None):
    """(top_k, top_p) as the C ABI takes them: (0, 1.0) is off.  ValueError for top_k < 0 and for top_p outside (0, 1]."""
    k = 0 if top_k is None else int(top_k)
    p = 1.0 if top_p is None else float(top_p)
    if k < 0:
        raise ValueError(f"vmlmf_amd: top_k must be >= 0 (None / 0: off), got {top_k}")
    if not (0.0 < p <= 1.0):
        raise ValueError(f"vmlmf_amd: top_p must lie in (0, 1] (None / 1: off), got {top_p}")
    if V is not None and k >= V:
        k = 0
    return k, p


def lm_sample(h, weight, bias, temperature, state=None, step=0, embed=None, form=None, top_k=None, top_p=None, return_kept=False,
              controls=None, truncation=None):
    """The next token of every row of h (B, H) - the top layer's output - under Linear(weight (V, H), bias (V)), in ONE launch that
    never writes the (B, V) scores.  temperature 0: greedy (argmax, ties to the lowest index); tau > 0: a draw from softmax(scores / tau)
    by Gumbel-max, its noise from Philox4x32-10 at (state = a {seed, offset} snapshot of dropout_advance(), position step * B + b,
    vocabulary row, the sampler's own site _lib.SITE_SAMPLE).  Returns (tokens (B) int64, logprobs (B)) - logprobs are the untempered
    log-softmax of the chosen tokens, what nll_loss charges for them - and, with embed (V, H), x_next = embed[tokens] (B, H).
    form: "fused" (vmlmf_lm_sample: head and choice in one launch, no score tensor), "gemm" (the library GEMM's (B, V) scores, then
    vmlmf_lm_choose: one workgroup per row), None: fused up to SAMPLE_FUSED_MAX_ROWS rows, gemm beyond (docs/design/lm_sampling.md).
    Both forms draw the same noise; their scores differ in fp32 rounding only.
    top_k / top_p (None: off; 0, k >= V and 1.0 too): the draw is restricted to the first k tokens of the order (larger score first,
    equal scores to the lower index) and, of those, to the shortest prefix whose renormalised mass under softmax(scores / tau) reaches
    top_p (vmlmf_lm_sample_filtered / vmlmf_lm_choose_filtered; include/vmlmf_hip.h has the contract).  The noise and the
    log-probabilities are those of the unfiltered call; greedy decoding is unchanged by any filter.  With a filter on form=None is
    fused up to SAMPLE_FILTERED_FUSED_MAX_ROWS rows (0: measured, the GEMM form is faster at every width).  return_kept: a last result, kept (B) int32 - how many tokens survived per row
    (V where no selection ran: filters off, or greedy).
    controls: a DecodeControls (eos, min_length, repetition_penalty, logit_bias / bans and the rows' seen / finished / length state):
    the choice runs on the controlled scores in ONE launch of its own library behind the head's GEMM (vmlmf_decode_choose,
    include/vmlmf_decode.h has the contract; form "gemm" only), which updates the controls' state in place; the noise and the
    log-probabilities stay those of the plain call, a finished row gives (eos, 0.0, kept 0), kept never counts a token at -inf.
    A HistoryControls (those, and no_repeat_ngram_size, banned_sequences, frequency_penalty, presence_penalty with the rows' hist /
    hist_len / count / overflow state) goes to ONE launch of vmlmf_history_choose instead (include/vmlmf_history.h has the contract),
    whatever of its controls is on: with none of the history's on, the results and the shared state are vmlmf_decode_choose's to the bit.
    truncation: a Truncation (min_p, typical_p, epsilon_cutoff, eta_cutoff).  With one of them on and temperature > 0 the choice is
    ONE launch of a library of its own behind the head's GEMM (vmlmf_truncate_choose, include/vmlmf_truncate.h has the contract; form
    "gemm" only), which runs top_k and top_p too and, under a DecodeControls, chooses on the controlled scores and moves their state on
    as vmlmf_decode_choose does; the noise and the log-probabilities stay those of the plain call, kept counts the survivors.  Greedy
    decoding ignores it, and None or a Truncation with nothing on is the call above, launch for launch.  ValueError with form="fused"
    and with a HistoryControls.
    An AutomatonControls (a DecodeControls, a TokenAutomaton and the rows' row_state / dead) goes to ONE launch of
    vmlmf_automaton_choose (include/vmlmf_automaton.h has the contract): a row's state closes the tokens its table row does not offer
    and moves on with the chosen token.  ValueError together with a truncation that is on."""
    for t, what in ((h, "h"), (weight, "weight")):
        _require_hip(t, what)
    if bias is not None:
        _require_hip(bias, "bias")
    if embed is not None:
        _require_hip(embed, "embedding table")
    temperature = float(temperature)
    if not temperature >= 0.0:
        raise ValueError(f"vmlmf_amd.lm_sample: temperature must be >= 0, got {temperature}")
    inv = 0.0 if temperature == 0.0 else 1.0 / temperature
    if inv > 0.0 and (state is None or not state.is_cuda or state.dtype != torch.int64 or state.numel() != 2):
        raise RuntimeError("vmlmf_amd.lm_sample: sampling (temperature > 0) needs a {seed, offset} snapshot: two int64 on the device")
    h2 = h.reshape(-1, h.shape[-1]).contiguous()
    B, H = h2.shape
    w = weight.contiguous()
    V = w.shape[0]
    if w.shape[1] != H or (bias is not None and bias.numel() != V) or (embed is not None and tuple(embed.shape) != (V, H)):
        raise RuntimeError(f"vmlmf_amd.lm_sample: h {tuple(h.shape)}, weight {tuple(weight.shape)}, bias / embed must be (V) / (V, H)")
    k, p = sample_filters(top_k, top_p, V)
    filtered = inv > 0.0 and (k > 0 or p < 1.0)      # greedy: the argmax is always kept, the existing kernels run
    if truncation is not None and not isinstance(truncation, Truncation):
        raise ValueError(f"vmlmf_amd.lm_sample: truncation must be a vmlmf_amd.Truncation or None, got {type(truncation).__name__}")
    truncated = truncation is not None and truncation.on
    if truncated and form not in (None, "gemm"):
        raise ValueError(f"vmlmf_amd.lm_sample: the truncation samplers have no fused-head form (form must be 'gemm' or None, got {form!r})")
    if truncated and getattr(controls, "TRUNCATION_REFUSAL", None) is not None:      # (a HistoryControls', an AutomatonControls')
        raise ValueError(controls.TRUNCATION_REFUSAL)
    truncated = truncated and inv > 0.0
    dev = h2.device
    lib = _lib.lib()
    tokens = torch.empty(B, device=dev, dtype=torch.int64)
    logp = torch.empty(B, device=dev, dtype=torch.float32)
    xn = torch.empty((B, H), device=dev, dtype=torch.float32) if embed is not None else None
    if not return_kept:
        kept = None
    elif filtered or truncated or controls is not None:
        kept = torch.empty(B, device=dev, dtype=torch.int32)
    else:
        kept = torch.full((B,), V, device=dev, dtype=torch.int32)
    if controls is not None and form not in (None, "gemm"):
        raise ValueError(f"vmlmf_amd.lm_sample: the controlled choice has no fused-head form (form must be 'gemm' or None, got {form!r})")
    if form is None:
        form = "fused" if B <= (SAMPLE_FILTERED_FUSED_MAX_ROWS if filtered else SAMPLE_FUSED_MAX_ROWS) else "gemm"
    outs = lambda: tuple(t for t in (tokens, logp, xn, kept) if t is not None)
    state_p = None if inv == 0.0 else ptr(state)
    bias_c, embed_c = None if bias is None else bias.contiguous(), None if embed is None else embed.contiguous()
    bias_p, embed_p = ptr(bias_c), ptr(embed_c)
    if truncated:
        _truncate.truncate_choose(torch.mm(h2, w.t()), bias_c, embed_c, inv, k, p, truncation, state, step, controls, tokens, logp, xn, kept)
        return outs()
    if controls is not None:
        _decode.decode_choose(torch.mm(h2, w.t()), bias_c, embed_c, inv, k, p, None if inv == 0.0 else state, step, controls, tokens, logp,
                              xn, kept)      # (the controls' class has the library and the entry point)
        return outs()
    if form == "gemm":
        scores = torch.mm(h2, w.t())
        with _lib.on_device(dev):
            if filtered:
                _lib.check(lib.vmlmf_lm_choose_filtered(B, H, V, ptr(scores), bias_p, embed_p, inv, k, p, state_p, int(step), ptr(tokens),
                                                        ptr(logp), ptr(xn), ptr(kept), _lib.raw_stream(dev)))
            else:
                _lib.check(lib.vmlmf_lm_choose(B, H, V, ptr(scores), bias_p, embed_p, inv, state_p, int(step), ptr(tokens), ptr(logp),
                                               ptr(xn), _lib.raw_stream(dev)))
        return outs()
    if form != "fused":
        raise ValueError(f"vmlmf_amd.lm_sample: form must be 'fused', 'gemm' or None, got {form!r}")
    nbytes = (lib.vmlmf_lm_sample_filtered_workspace_bytes if filtered else lib.vmlmf_lm_sample_workspace_bytes)(B, V)
    ws = _sample_workspace(dev, nbytes)
    with _lib.on_device(dev):
        if filtered:
            _lib.check(lib.vmlmf_lm_sample_filtered(B, H, V, ptr(h2), ptr(w), bias_p, embed_p, inv, k, p, state_p, int(step),
                                                    ptr(tokens), ptr(logp), ptr(xn), ptr(kept), ptr(sample_ticket(dev)), ptr(ws),
                                                    nbytes, _lib.raw_stream(dev)))
        else:
            _lib.check(lib.vmlmf_lm_sample(B, H, V, ptr(h2), ptr(w), bias_p, embed_p, inv, state_p, int(step), ptr(tokens),
                                           ptr(logp), ptr(xn), ptr(sample_ticket(dev)), ptr(ws), nbytes, _lib.raw_stream(dev)))
    return outs()


# ---- the step loops ----------------------------------------------------------------------------------------------------------------
def decode_layers(model, x, states, layer_path):
    """The layers at T = 1: x (1, B, H) -> (y (1, B, H), states).  layer_path "stack": stack_layers' one launch where it covers the
    layers (it packs the parameters on every call); otherwise a call per layer - VMLMF layers reuse kept images (_KeptImages)."""
    if layer_path == "stack":
        stacked = stack_layers(model.rnns, x, states)
        if stacked is not None:
            return stacked[0], list(stacked[1])
    states = list(states)
    for i, rnn in enumerate(model.rnns):
        x, states[i] = rnn(x, states[i])
    return x, states


def decode_steps(model, h, states, steps, temperature, snap, layer_path, top_k=None, top_p=None, controls=None, min_p=None, typical_p=None,
                 epsilon_cutoff=None, eta_cutoff=None):
    """`steps` tokens from the top layer's output h (B, H): per step one vmlmf_lm_sample launch (head, choice, log-probability and
    the next input row; with top_k / top_p its filtered form), then the layers at T = 1 on that row.  No host synchronisation:
    capturable (DecodeGraph).  controls: a DecodeControls - the choice is then the controlled launch behind the head's GEMM
    (vmlmf_decode_choose; a HistoryControls: vmlmf_history_choose), which moves the controls' state on in place.  min_p, typical_p,
    epsilon_cutoff, eta_cutoff: the truncation samplers of Model.generate - with one of them on the choice is vmlmf_truncate_choose."""
    toks, lps = [], []
    trunc = _truncate.truncation(min_p, typical_p, epsilon_cutoff, eta_cutoff, isinstance(controls, HistoryControls))
    for j in range(steps):
        tok, lp, x = lm_sample(h, model.fc.w, model.fc.b, temperature, snap, j, embed=model.embed.w, top_k=top_k, top_p=top_p,
                               controls=controls, truncation=trunc)
        toks.append(tok)
        lps.append(lp)
        y, states = decode_layers(model, x.unsqueeze(0), states, layer_path)
        h = y[-1]
    return torch.stack(toks), torch.stack(lps), h, states


def beam_steps(model, h, states, cum, finished, length, steps, eos, buffers=None, controls=None, **carried):
    """`steps` steps of beam search from the beams' top-layer outputs h (B W, H): per step the head's GEMM and ONE selection launch
    (lm_beam_step: totals, the W survivors of each batch row in order, their next input rows), ONE launch that makes the
    2 L state tensors follow their hypotheses (beam_gather), then the layers at T = 1 on the B W rows.  No host
    synchronisation: capturable (BeamGraph).  Returns (parents, tokens (steps, B, W), h, states, cum, finished, length).
    controls: a BeamPolicy - the selection is its select(), and the tensors it carries from step to step (controls.carried) are taken as
    keywords **carried (default: controls.first_carried(), a search that starts; TypeError for a keyword it does not carry) and follow
    the seven results as they stand after the steps.  A BeamControls: the controlled launch (vmlmf_beamctl_step) and, where the controls
    keep a history, the vmlmf_history_bans launch in front of it on hist / hist_len, the beams' histories.  An AutomatonBeamControls:
    vmlmf_automaton_beam_step on beam_state (B W) int32, the beams' states.  A GroupBeams: vmlmf_beamgroup_step, nothing carried.  A
    StochasticBeams: vmlmf_sbeam_step on perturbed (B, W) and draw (B), drawing from controls.state."""
    parents, toks = [], []
    # what the controls carry from step to step behind cum, finished and length (lm_beam_step takes it by these names)
    names = _beam_extras(controls)
    extra = _beam_start(controls, **carried)
    for _ in range(steps):
        par, tok, cum, finished, length, x, src, *rest = lm_beam_step(h, model.fc.w, model.fc.b, cum, finished, length, eos, model.embed.w,
                                                                      buffers=buffers, controls=controls, **dict(zip(names, extra)))
        extra = rest[:len(names)]
        parents.append(par)
        toks.append(tok)
        flat = beam_gather([t for st in states for t in st], src)
        states = [(flat[2 * i], flat[2 * i + 1]) for i in range(len(states))]
        y, states = decode_layers(model, x.unsqueeze(0), states, "layers")
        h = y[-1]
    return (torch.stack(parents), torch.stack(toks), h, states, cum, finished, length, *extra)


# What a decode carries from step to step, as one flat list: [h, h_0, c_0, ... h_L-1, c_L-1] and, for beams, cum, finished and length
# behind them - and behind those, under BeamControls that keep a history, the beams' hist and hist_len; under AutomatonBeamControls, the
# beams' states.  The two forms below are the step loops above on such a list: carried -> (outputs, carried after the steps).
def _pairs(flat):
    return [(flat[i], flat[i + 1]) for i in range(0, len(flat), 2)]


def _sampled(model, gen, carried, steps, temperature, layer_path, top_k, top_p, controls, **truncation):
    """decode_steps, the generator `gen` (None: greedy) snapshotted and advanced in front."""
    snap = dropout_advance(gen) if gen is not None else None
    toks, lps, h, states = decode_steps(model, carried[0], _pairs(carried[1:]), steps, temperature, snap, layer_path, top_k, top_p, controls,
                                        **truncation)
    return (toks, lps), [h, *(t for st in states for t in st)]


def _join_beams(h, states, cum, finished, length, history):
    return [h, *(t for st in states for t in st), cum, finished, length, *history]


def _beam_extras(controls):                 # the names of what the controls carry behind cum, finished and length (beam_steps' keywords)
    return () if controls is None else controls.carried


def _beam_start(controls, **carried):       # those tensors: the given ones (hist=, hist_len= / beam_state= ...), or a search that starts
    _beam.check_carried(controls, carried)
    given = [carried.get(name) for name in _beam_extras(controls)]
    if any(t is None for t in given):
        given = [first if t is None else t for t, first in zip(given, controls.first_carried())]
    return given


def _split_beams(carried, controls):        # _join_beams' arguments back; history: [hist, hist_len] / [beam_state] where the controls carry them
    n = len(_beam_extras(controls))
    history = list(carried[-n:]) if n else []
    h, *flat, cum, finished, length = carried[:len(carried) - len(history)]
    return h, _pairs(flat), cum, finished, length, history


def _beamed(model, carried, steps, eos, buffers=None, controls=None):
    h, states, cum, finished, length, history = _split_beams(carried, controls)
    par, tok, h, states, cum, finished, length, *history = beam_steps(model, h, states, cum, finished, length, steps, eos, buffers, controls,
                                                                      **dict(zip(_beam_extras(controls), history)))
    return (par, tok), _join_beams(h, states, cum, finished, length, history)


# ---- the step loops as captured graphs ---------------------------------------------------------------------------------------------
class _KeptImages:
    """`with _KeptImages(model[, caches]):` every VMLMF layer of the model keeps its packed parameter images for the duration
    (functional.cache_packed_parameters) - a layer that already keeps them keeps its own cache -, and the caller's setting comes back
    afterwards.  caches: the PackCache of each such layer, in order (a captured graph holds its own: the graph reads their buffers)."""

    def __init__(self, model, caches=None):
        self.layers = [m for m in model.modules() if hasattr(m, "kernel_params")]
        self.caches = caches

    def __enter__(self):
        self.saved = [m.__dict__.get("_pack_cache", _UNSET) for m in self.layers]
        for i, (m, was) in enumerate(zip(self.layers, self.saved)):
            if self.caches is not None:
                m._pack_cache = self.caches[i]
            elif was is _UNSET or was is None:
                m._pack_cache = PackCache()
        return self

    def __exit__(self, *exc):
        for m, was in zip(self.layers, self.saved):
            if was is _UNSET:
                m.__dict__.pop("_pack_cache", None)
            else:
                m._pack_cache = was
        return False


_UNSET = object()


class _StepGraph:
    """What DecodeGraph and BeamGraph share: steps of a model captured once into a hipGraph - linear, on one stream - over buffers
    this object owns, so that a replay continues where the previous one stopped."""

    def _capture(self, model, carried, step, warm_up=None):
        """carried: the tensors a step reads and hands on, cloned into `self.carried`; step(carried) -> (outputs, carried after it).
        One PackCache per VMLMF layer (`self.caches`: the graph reads their buffers); a warm-up outside the capture, on a side stream
        and on copies - warm_up(copies), default step - packs the images, loads the libraries and creates tickets and workspaces;
        then the capture on the owned buffers, the copy-back of every carried tensor its last work."""
        self.carried = [t.detach().clone() for t in carried]
        self.caches = [PackCache() for m in model.modules() if hasattr(m, "kernel_params")]
        dev = self.carried[0].device
        with torch.no_grad(), _KeptImages(model, self.caches):
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                (warm_up or step)([t.clone() for t in self.carried])
            torch.cuda.current_stream(dev).wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.outputs, after = step(self.carried)
                for t, new in zip(self.carried, after):
                    t.copy_(new)

    def replay(self):
        self.graph.replay()
        return tuple(t.clone() for t in self.outputs)


class DecodeGraph(_StepGraph):
    """`steps` decode steps of a Model (decode_steps: per step the vmlmf_lm_sample launch and the layers at T = 1) captured once into
    a hipGraph - linear, on one stream.  replay() continues from where the previous replay stopped (the top layer's output and the
    layers' states live in this object's buffers, h / states) and returns (tokens (steps, B), logprobs (steps, B)); with temperature > 0
    the first node snapshots and advances the model's sampler_state(), so every replay draws fresh tokens and a new capture from the same
    seed and inputs repeats the first replay.  The generator is the sampler_state() tensor of construction time: re-seeding the model
    (sampler_state(seed)) puts a new tensor in its place, which this graph does not see - build a new DecodeGraph after re-seeding, as
    after the parameters change (the layers read kept parameter images packed at construction).  Replay DecodeGraphs one after
    another, never two at once on different streams: the sampler's ticket words are taken from a ring of 16 per device (as the
    criterion's, functional.ce_ticket), so two graphs can share them, and concurrent replays would break the last-arrival count.
    top_k / top_p: the filters of Model.generate, fixed at construction.
    controls: a DecodeControls (eos, bans, repetition penalty ...).  The captured launches read and write ITS buffers - seen, finished,
    length, and a HistoryControls' hist, hist_len, count, overflow -, so replays continue one decode: finished rows stay finished, seen
    and the history accumulate (the warm-up runs on a clone of all of them).  An AutomatonControls' row_state and dead are among them:
    a replay continues the rows' walk through the automaton.
    min_p, typical_p, epsilon_cutoff, eta_cutoff: the truncation samplers of Model.generate, fixed at construction."""

    def __init__(self, model, h, states, steps, temperature=1.0, layer_path="layers", top_k=None, top_p=None, controls=None, min_p=None,
                 typical_p=None, epsilon_cutoff=None, eta_cutoff=None):
        self.model, self.steps, self.temperature, self.layer_path = model, int(steps), float(temperature), layer_path
        sample_filters(top_k, top_p)
        self.top_k, self.top_p, self.controls = top_k, top_p, controls
        self.truncation = dict(min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff)
        _truncate.truncation(**self.truncation, history=isinstance(controls, HistoryControls))
        self.gen = model.sampler_state() if self.temperature > 0 else None

        def step(carried, controls=controls):
            return _sampled(model, self.gen, carried, self.steps, self.temperature, layer_path, top_k, top_p, controls, **self.truncation)

        def warm_up(carried):           # on a clone of the controls; the generator is put back
            saved = None if self.gen is None else self.gen.clone()
            step(carried, None if controls is None else controls.clone())
            if saved is not None:
                self.gen.copy_(saved)
        self._capture(model, [h, *(t for st in states for t in st)], step, warm_up)
        self.h, *flat = self.carried
        self.states, (self.tokens, self.logprobs) = _pairs(flat), self.outputs


class BeamGraph(_StepGraph):
    """`steps` steps of Model.beam_search (beam_steps: per step the head's GEMM, the vmlmf_beam_step launch, the vmlmf_beam_gather
    launch and the layers at T = 1) captured once into a hipGraph - linear, on one stream.  h (B W, H) and states are the beams' (row
    b W + w) of `beams` = W beams per batch row; cum / finished / length (B, W) default to a fresh search (beam 0 at 0, the others at
    -inf; the controls' first_beams()).  replay() continues from where the previous replay stopped - h, states, cum, finished and length
    live in this object's buffers - and returns (parents, tokens), both (steps, B, W), for beam_backtrack.  The ticket words and the
    workspace of the selection are this graph's own (`buffers`: the controls' new_buffers(), sized for THEIR step), so graphs may be
    replayed on whatever streams; the layers read parameter images packed at construction: build a new BeamGraph after the parameters
    change.
    controls: a BeamPolicy.  What it carries (controls.carried, given as keywords **carried - default: controls.first_carried(), a
    search that starts) is carried with cum, finished and length - in this object's buffers, one attribute per name, so a replay
    continues the hypotheses of the last one; the warm-up runs on controls.clone().  A BeamControls that keeps a history: hist /
    hist_len; the captured launches set the controls' own `overflow`.  An AutomatonBeamControls: beam_state.  A StochasticBeams:
    perturbed and draw (StochasticBeamGraph)."""

    def __init__(self, model, h, states, steps, beams, eos=None, cum=None, finished=None, length=None, controls=None, **carried):
        self.model, self.steps, self.eos, self.controls = model, int(steps), eos, controls
        W = _beam.check_beams(beams, model.vocab_size)
        policy = controls if controls is not None else _beam.BeamPolicy(h.shape[0] // W, W, model.vocab_size, h.device)
        cum, finished, length = (new if t is None else t for t, new in zip((cum, finished, length), policy.first_beams()))
        self.buffers = policy.new_buffers()
        history = _beam_start(controls, **carried)
        step = lambda carried, controls=controls: _beamed(model, carried, self.steps, eos, self.buffers, controls)
        self._capture(model, _join_beams(h, states, cum, finished.to(torch.int32), length.to(torch.int32), history), step,
                      None if controls is None else lambda carried: step(carried, controls.clone()))
        self.h, self.states, self.cum, self.finished, self.length, history = _split_beams(self.carried, controls)
        for name, t in zip(_beam_extras(controls), history):
            setattr(self, name, t)
        self.parents, self.tokens = self.outputs


class StochasticBeamGraph(BeamGraph):
    """`steps` steps of Model.stochastic_beam_search captured once into a hipGraph: a BeamGraph under a StochasticBeams (`beams`) of its
    own - per step the head's GEMM, the vmlmf_sbeam_step launch, the vmlmf_beam_gather launch and the layers at T = 1.  cum / finished /
    length / perturbed / draw default to a search that starts (StochasticBeams.start()).  state: a {seed, offset} snapshot
    (dropout_advance()); the graph draws from its own copy, `self.state` - copy another snapshot into it for another sample.  replay()
    continues from where the previous replay stopped - perturbed and draw live in this object's buffers with BeamGraph's, so the noise of
    a replay is that of the eager steps at the same count."""

    def __init__(self, model, h, states, steps, beams, state, eos=None, cum=None, finished=None, length=None, perturbed=None, draw=None):
        W = _sbeam.check_sbeam(beams, model.vocab_size)
        self.beams = StochasticBeams(h.shape[0] // W, W, model.vocab_size, h.device)
        self.beams.state = self.state = state.detach().clone()
        super().__init__(model, h, states, steps, W, eos, cum, finished, length, self.beams, perturbed=perturbed, draw=draw)


# ---- one call: the checks, the prompt, the steps -----------------------------------------------------------------------------------
def _check_call(model, prompt, method, kernel):
    """RuntimeError unless the model and the prompt live on a HIP device and the prompt is (T0, B) int64."""
    if not (isinstance(prompt, torch.Tensor) and prompt.is_cuda and model.embed.w.is_cuda):
        raise RuntimeError(f"vmlmf_amd: Model.{method} runs on the HIP {kernel} only: move the model and the prompt to 'cuda' "
                           "(no CPU fallback)")
    if prompt.dim() != 2 or prompt.dtype != torch.int64:
        raise RuntimeError(f"vmlmf_amd: Model.{method} takes a (T0, B) int64 prompt")


def _check_chunk(method, chunk, steps):
    if chunk is not None and (int(chunk) < 1 or steps % int(chunk) != 0):
        raise ValueError(f"vmlmf_amd: Model.{method}: chunk={chunk} must divide steps={steps}")


def _check_search(method, V, **given):
    """ValueError for what a search call cannot take of eos= (None or one of the V tokens), length_penalty= (>= 0) and steps= (an int
    >= 0), looked at in the order given."""
    for name, value in given.items():
        if name == "eos" and value is not None and not 0 <= int(value) < V:
            raise ValueError(f"vmlmf_amd: Model.{method}: eos={value} is not a token of the vocabulary ({V})")
        if name == "length_penalty" and not float(value) >= 0.0:
            raise ValueError(f"vmlmf_amd: Model.{method}: length_penalty must be >= 0, got {value}")
        if name == "steps" and value < 0:
            raise ValueError(f"vmlmf_amd: Model.{method}: steps must be >= 0, got {value}")


def _widen(states, W):
    """The layers' states with every batch row W times over (row b W + w)."""
    return [tuple(t.repeat_interleave(W, t.dim() - 2) for t in st) for st in states]


def _ranked(parents, toks, cum, length, states, alpha, groups=1):
    """The end of a beam search: (hypotheses (steps, B, W) behind the last step's slots, cum, length, states), for alpha > 0 re-sorted
    (stable) by cum / length ** alpha within each of the `groups` groups of a row - no hypothesis leaves its group."""
    B, W = cum.shape
    order = None
    if alpha > 0.0 and len(parents):                # (no step: the start values as they are)
        key = cum / length.to(torch.float32) ** alpha
        if groups == 1:
            order = torch.sort(key, dim=1, descending=True, stable=True).indices
        else:
            order = torch.sort(key.view(B, groups, W // groups), dim=2, descending=True, stable=True).indices
            order = (order + torch.arange(groups, device=cum.device)[None, :, None] * (W // groups)).view(B, W)
        cum, length = cum.gather(1, order), length.gather(1, order)
        rows = (torch.arange(B, device=cum.device)[:, None] * W + order).reshape(-1).to(torch.int32)
        states = _pairs(beam_gather([t for st in states for t in st], rows))
        order = order.to(torch.int32)
    return beam_backtrack(parents, toks, order), cum, length, states


@contextlib.contextmanager
def _activations(model, tokens, states):
    """`with _activations(model, tokens, states) as (h, states):` the model in eval mode, without autograd and on kept parameter images
    for the duration; h (T, B, H) are features()'s activations - the top layer's output behind every token -, states (default:
    state_init) have taken the tokens in.  Every module's train / eval flag is as the caller left it afterwards, whatever was raised."""
    states = model.state_init(tokens.shape[1]) if states is None else list(states)
    modes = [(mod, mod.training) for mod in model.modules()]
    model.train(False)
    try:
        with torch.no_grad(), _KeptImages(model):
            h, states = model.features(tokens, list(states))
            yield h, states
    finally:
        for mod, was in modes:
            mod.training = was


@contextlib.contextmanager
def _session(model, prompt, states):
    """_activations for a decode: h (B, H) is the top layer's output behind the prompt's last token."""
    with _activations(model, prompt, states) as (h, states):
        yield h[-1], states


def _run(steps, chunk, eager, graph):
    """The steps of one call, as (outputs, carried after them): eager(), or - chunk=K - graph()'s K captured steps replayed
    steps / K times: the replays' outputs concatenated, the carried tensors cloned out of the graph's buffers."""
    if chunk is None:
        return eager()
    g = graph()
    outs = [g.replay() for _ in range(steps // int(chunk))]
    return tuple(torch.cat(o) for o in zip(*outs)), [t.clone() for t in g.carried]


def generate(model, prompt, steps, states=None, temperature=1.0, seed=None, chunk=None, layer_path="layers", top_k=None, top_p=None,
             eos=None, min_length=0, repetition_penalty=1.0, logit_bias=None, banned_tokens=None, return_lengths=False,
             no_repeat_ngram_size=0, banned_sequences=None, frequency_penalty=0.0, presence_penalty=0.0, *, min_p=None, typical_p=None,
             epsilon_cutoff=None, eta_cutoff=None, automaton=None, automaton_state=None):
    """Model.generate (lm.py has the contract)."""
    sample_filters(top_k, top_p)
    trunc_args = dict(min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff)
    hist_args = dict(no_repeat_ngram_size=no_repeat_ngram_size, banned_sequences=banned_sequences, frequency_penalty=frequency_penalty,
                     presence_penalty=presence_penalty)
    history = _history.history_on(**hist_args)
    trunc = _truncate.truncation(**trunc_args, history=history)
    if automaton is None and automaton_state is not None:
        raise ValueError("vmlmf_amd: automaton_state needs automaton")
    if automaton is not None and history:
        raise ValueError(_automaton.GENERATE_REFUSAL.format(
            what="the history controls (no_repeat_ngram_size, banned_sequences, frequency_penalty, presence_penalty)"))
    if automaton is not None and trunc is not None:
        raise ValueError(_automaton.GENERATE_REFUSAL.format(what="the truncation samplers (min_p, typical_p, epsilon_cutoff, eta_cutoff)"))
    ctl_args = dict(eos=eos, min_length=min_length, repetition_penalty=repetition_penalty, logit_bias=logit_bias,
                    banned_tokens=banned_tokens)
    eos_c, min_c, _, banned = _decode.check_controls(model.vocab_size, **ctl_args)
    controlled = _decode.controls_on(eos, repetition_penalty, logit_bias, banned_tokens)
    if controlled or history or automaton is not None:
        closed = _decode.check_bias(model.vocab_size, logit_bias, banned, eos_c, min_c)
    if automaton is not None:
        rows = prompt.shape[1] if isinstance(prompt, torch.Tensor) and prompt.dim() == 2 else 0
        start = _automaton.check_automaton(automaton, model.vocab_size, rows, automaton_state)
        automaton.check_reachable(start, _automaton.closed_tokens(model.vocab_size, logit_bias, banned), eos_c, min_c)
    if history:
        T0 = prompt.shape[0] if isinstance(prompt, torch.Tensor) and prompt.dim() == 2 else 0
        _history.check_history(model.vocab_size, prompt_length=T0, steps=int(steps), closed=closed, **hist_args)
    _check_call(model, prompt, "generate", "sampler kernel (vmlmf_lm_sample)")
    steps, temperature = int(steps), float(temperature)
    _check_chunk("generate", chunk, steps)
    B, dev = prompt.shape[1], prompt.device
    gen = model.sampler_state(seed) if temperature > 0 else None
    with _session(model, prompt, states) as (h, states):
        if automaton is not None:
            controls = AutomatonControls(B, model.vocab_size, dev, automaton, automaton_state, prompt=prompt, _checked=True, **ctl_args)
        elif history:   # capacity: the prompt and every step - the history never overflows
            controls = HistoryControls(B, model.vocab_size, dev, capacity=max(prompt.shape[0] + steps, 1), prompt=prompt, _checked=True,
                                       **hist_args, **ctl_args)
        else:
            controls = DecodeControls(B, model.vocab_size, dev, prompt=prompt, _checked=True, **ctl_args) if controlled else None
        if steps == 0:
            tokens, logprobs = torch.empty((0, B), dtype=torch.int64, device=dev), torch.empty((0, B), device=dev)
        else:
            (tokens, logprobs), (_, *flat) = _run(
                steps, chunk,
                lambda: _sampled(model, gen, [h, *(t for st in states for t in st)], steps, temperature, layer_path, top_k, top_p, controls,
                                 **trunc_args),
                lambda: DecodeGraph(model, h, states, int(chunk), temperature, layer_path, top_k, top_p, controls, **trunc_args))
            states = _pairs(flat)
        if not return_lengths:
            return tokens, logprobs, states
        lengths = controls.length.clone() if controls is not None else torch.full((B,), steps, dtype=torch.int32, device=dev)
        return tokens, logprobs, lengths, states


def _search(model, prompt, states, steps, chunk, W, eos, controls):
    """What beam_search, group_beam_search and stochastic_beam_search share behind their checks: the session on the prompt, h and the
    states W times over, the start of a search (the controls' first_beams() and first_carried(); controls None: the plain step), the
    steps - eager, or chunk=K: a BeamGraph of K steps replayed - and the carried list taken apart.  Returns ((parents, tokens), each
    (steps, B, W), states, cum, finished, length, [what the controls carry]); steps == 0: the start values."""
    B, dev = prompt.shape[1], prompt.device
    policy = controls if controls is not None else _beam.BeamPolicy(B, W, model.vocab_size, dev)
    with _session(model, prompt, states) as (h, states):
        h, states = h.repeat_interleave(W, 0), _widen(states, W)
        (cum, finished, length), history = policy.first_beams(), policy.first_carried()
        if steps == 0:
            none = torch.empty((0, B, W), dtype=torch.int32, device=dev)
            return (none, none.to(torch.int64)), states, cum, finished, length, history
        outs, carried = _run(
            steps, chunk,
            lambda: _beamed(model, _join_beams(h, states, cum, finished, length, history), steps, eos, None, controls),
            lambda: BeamGraph(model, h, states, int(chunk), W, eos, cum, finished, length, controls,
                              **dict(zip(policy.carried, history))))
        return (outs, *_split_beams(carried, controls)[1:])


def beam_search(model, prompt, steps, beams=4, states=None, eos=None, length_penalty=0.0, chunk=None, min_length=0, banned_tokens=None,
                no_repeat_ngram_size=0, banned_sequences=None, *, automaton=None, automaton_state=None):
    """Model.beam_search (lm.py has the contract)."""
    W = _beam.check_beams(beams, model.vocab_size)
    steps, alpha = int(steps), float(length_penalty)
    _check_search("beam_search", model.vocab_size, eos=eos, length_penalty=length_penalty, steps=steps)
    ctl_args = dict(eos=eos, min_length=min_length, banned_tokens=banned_tokens, no_repeat_ngram_size=no_repeat_ngram_size,
                    banned_sequences=banned_sequences)
    controlled = _beamctl.controls_on(min_length, banned_tokens, no_repeat_ngram_size, banned_sequences)
    T0 = prompt.shape[0] if isinstance(prompt, torch.Tensor) and prompt.dim() == 2 else 0
    if automaton is None and automaton_state is not None:
        raise ValueError("vmlmf_amd: automaton_state needs automaton")
    if automaton is not None:
        if no_repeat_ngram_size != 0 or banned_sequences is not None:
            raise ValueError(_automaton.BEAM_REFUSAL.format(what="no_repeat_ngram_size / banned_sequences"))
        controlled = False
        eos_c, min_c, banned, _, _ = _beamctl.check_beam_controls(model.vocab_size, 1, eos, min_length, banned_tokens)
        rows = prompt.shape[1] if isinstance(prompt, torch.Tensor) and prompt.dim() == 2 else 0
        start = _automaton.check_automaton(automaton, model.vocab_size, rows, automaton_state)
        automaton.check_reachable(start, _automaton.closed_tokens(model.vocab_size, None, banned), eos_c, min_c)
    if controlled:      # (without them nothing of the controls is looked at: the call is what it was)
        _beamctl.check_beam_controls(model.vocab_size, W, prompt_length=T0, steps=steps, **ctl_args)
    _check_chunk("beam_search", chunk, steps)
    _check_call(model, prompt, "beam_search", "beam-step kernel (vmlmf_beam_step)")
    B, dev = prompt.shape[1], prompt.device
    # capacity: the prompt and every step - the history never overflows
    controls = BeamControls(B, W, model.vocab_size, dev, prompt=prompt, capacity=max(T0 + steps, 1), **ctl_args) if controlled else None
    if automaton is not None:
        controls = AutomatonBeamControls(B, W, model.vocab_size, dev, automaton, automaton_state, eos=eos, min_length=min_length,
                                         banned_tokens=banned_tokens, _checked=True)
    (parents, toks), states, cum, _, length, _ = _search(model, prompt, states, steps, chunk, W, eos, controls)
    return _ranked(parents, toks, cum, length, states, alpha)


def group_beam_search(model, prompt, steps, beams=4, *, groups=2, diversity_penalty=0.5, states=None, eos=None, length_penalty=0.0,
                      chunk=None):
    """Model.group_beam_search (lm.py has the contract)."""
    W, G, lam = _beamgroup.check_groups(beams, groups, diversity_penalty, model.vocab_size)
    steps, alpha = int(steps), float(length_penalty)
    _check_search("group_beam_search", model.vocab_size, eos=eos, length_penalty=length_penalty, steps=steps)
    _check_chunk("group_beam_search", chunk, steps)
    _check_call(model, prompt, "group_beam_search", "group beam-step kernel (vmlmf_beamgroup_step)")
    controls = GroupBeams(prompt.shape[1], W, model.vocab_size, prompt.device, G, lam)
    (parents, toks), states, cum, _, length, _ = _search(model, prompt, states, steps, chunk, W, eos, controls)
    return _ranked(parents, toks, cum, length, states, alpha, G)


# ---- contrastive search ------------------------------------------------------------------------------------------------------------
def _block_heads(t, k):
    """Row b k of every block of k rows (the rows of a block are equal): (..., B k, H) -> (..., B, H)."""
    return t.index_select(t.dim() - 2, torch.arange(0, t.shape[-2], k, device=t.device))


def contrast_steps(model, h, states, controls, steps, return_penalties=False):
    """`steps` steps of contrastive search from the top layer's output h (B, H) and the layers' states on B k rows (row b k + j: the
    rows of a block equal): per step the head's GEMM and the vmlmf_score_rows launch that names the k candidates (scoring.lm_score,
    top=k: the project's one selection), the embedding, the layers at T = 1 on the B k candidate rows, ONE vmlmf_contrast_choose launch
    (lm_contrast_step) and ONE vmlmf_beam_gather launch that makes every state row of a block follow the chosen candidate.  No host
    synchronisation: capturable (ContrastGraph).  Returns (tokens, logprobs[, penalties] (steps, B), h, states, before): `before` are
    the states in front of the last step's layers - they have taken in everything but the last token."""
    from .scoring import lm_score
    toks, lps, pens = [], [], []
    before = states
    for _ in range(steps):
        _, _, cand_tok, cand_logp = lm_score(h, model.fc.w, model.fc.b, None, controls.k)
        x = model.embed(cand_tok.reshape(-1))
        y, after = decode_layers(model, x.unsqueeze(0), states, "layers")
        tok, lp, chosen, sim, h, src = lm_contrast_step(y[-1], cand_tok, cand_logp, controls)
        toks.append(tok)
        lps.append(lp)
        if return_penalties:
            pens.append(sim.gather(1, chosen.to(torch.int64)[:, None])[:, 0])
        before = states
        states = _pairs(beam_gather([t for st in after for t in st], src))
    outs = (torch.stack(toks), torch.stack(lps)) + ((torch.stack(pens),) if return_penalties else ())
    return (*outs, h, states, before)


def _contrasted(model, carried, controls, steps, return_penalties):
    """contrast_steps on a flat list [h, before ..., states ...] -> (outputs, that list after the steps).  `before` stands in front of
    the states: after one step it IS the incoming states, and a graph's copy-back (_StepGraph._capture) writes its buffers in list
    order - the states' buffers must still hold the old states when `before` is copied out of them."""
    n = (len(carried) - 1) // 2
    *outs, h, states, before = contrast_steps(model, carried[0], _pairs(carried[1 + n:]), controls, steps, return_penalties)
    return tuple(outs), [h, *(t for st in before for t in st), *(t for st in states for t in st)]


class ContrastGraph(_StepGraph):
    """`steps` steps of Model.contrastive_search (contrast_steps) captured once into a hipGraph - linear, on one stream.  h (B, H) and
    states (B k rows) are those of contrast_steps; replay() continues from where the previous replay stopped - h and the states live in
    this object's buffers, the history, its length on the device, finished and length in `controls`, which the captured launches read
    and write in place (the warm-up runs on a clone) - and returns (tokens, logprobs[, penalties]), each (steps, B).  The ticket and
    the workspace are the controls' own; the layers read parameter images packed at construction: build a new graph after the
    parameters change.  The controls' capacity must cover every replay."""

    def __init__(self, model, h, states, steps, controls, return_penalties=False):
        self.model, self.steps, self.controls = model, int(steps), controls
        flat = [t for st in states for t in st]
        step = lambda carried, controls=controls: _contrasted(model, carried, controls, self.steps, return_penalties)
        self._capture(model, [h, *flat, *flat], step, lambda carried: step(carried, controls.clone()))
        n = len(flat)
        self.h, self.before, self.states = self.carried[0], _pairs(self.carried[1:1 + n]), _pairs(self.carried[1 + n:])
        self.tokens, self.logprobs = self.outputs[:2]


def contrastive_search(model, prompt, steps, top_k=4, penalty_alpha=0.6, *, states=None, eos=None, chunk=None, return_penalties=False):
    """Model.contrastive_search (lm.py has the contract)."""
    k, alpha = _contrast.check_contrast(top_k, penalty_alpha, model.vocab_size, model.hidden_size)
    steps = int(steps)
    _check_search("contrastive_search", model.vocab_size, steps=steps, eos=eos)
    if isinstance(prompt, torch.Tensor) and prompt.dim() == 2 and prompt.shape[0] < 1:
        raise ValueError("vmlmf_amd: Model.contrastive_search: the prompt needs T0 >= 1 tokens: the first step compares with the history behind them")
    _check_chunk("contrastive_search", chunk, steps)
    _check_call(model, prompt, "contrastive_search", "contrastive-step kernel (vmlmf_contrast_choose)")
    T0, B = prompt.shape
    dev = prompt.device
    with _activations(model, prompt, states) as (hs, states):
        controls = ContrastControls(B, model.hidden_size, dev, T0 + max(steps, 1), k, alpha, eos, model.vocab_size)
        controls.append(hs)
        if steps == 0:
            empty = torch.empty((0, B), device=dev)
            return (empty.to(torch.int64), empty, controls.length, *((empty.clone(),) if return_penalties else ()), states)
        wide = _widen(states, k)
        flat = [t for st in wide for t in st]
        outs, carried = _run(steps, chunk, lambda: _contrasted(model, [hs[-1], *flat, *flat], controls, steps, return_penalties),
                             lambda: ContrastGraph(model, hs[-1], wide, int(chunk), controls, return_penalties))
        before = _pairs([_block_heads(t, k) for t in carried[1:1 + len(flat)]])
        return (outs[0], outs[1], controls.length.clone(), *outs[2:], before)


# ---- stochastic beam search --------------------------------------------------------------------------------------------------------
def stochastic_beam_search(model, prompt, steps, beams=4, *, seed=None, states=None, eos=None, chunk=None):
    """Model.stochastic_beam_search (lm.py has the contract)."""
    W = _sbeam.check_sbeam(beams, model.vocab_size)
    steps = int(steps)
    _check_search("stochastic_beam_search", model.vocab_size, eos=eos, steps=steps)
    _check_chunk("stochastic_beam_search", chunk, steps)
    _check_call(model, prompt, "stochastic_beam_search", "stochastic beam-step kernel (vmlmf_sbeam_step)")
    controls = StochasticBeams(prompt.shape[1], W, model.vocab_size, prompt.device)
    controls.state = dropout_advance(model.sampler_state(seed))      # once per call: the steps differ by `draw`, on the device
    (parents, toks), states, cum, _, length, (perturbed, _) = _search(model, prompt, states, steps, chunk, W, eos, controls)
    return beam_backtrack(parents, toks), cum, perturbed, length, states
