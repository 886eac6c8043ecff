"""Scoring given text with the language model (lm.Model): what stands behind Model.score.  Where decoding.py continues a prompt, this
module says how probable a text is, token by token.

  lm_score    the head's GEMM and ONE launch per chunk of rows (C ABI: vmlmf_score_rows, a library of its own; _score.py): a target
              token's log-probability and rank, and the row's most probable tokens
  score       the call behind Model.score, where the contract is written down
  lm_cache_score  ONE launch per call (C ABI: vmlmf_ncache_score, a library of its own; _ncache.py): the positions' log-probabilities
              under the model mixed with a continuous cache of the last `window` outputs and the tokens that followed them
  cache_score the call behind Model.cache_score, where the contract is written down
"""
from __future__ import annotations

import torch

from . import _ncache, _score
from ._ncache import NeuralCache, lm_cache_score  # noqa: F401 (the package's exports)
from .functional import _require_hip, check_lengths


def _check_chunk_rows(chunk_rows, who):
    if int(chunk_rows) < 1:
        raise ValueError(f"vmlmf_amd.{who}: chunk_rows must be >= 1, got {chunk_rows}")
    return int(chunk_rows)


def lm_score(h, weight, bias, targets=None, top=0, chunk_rows=2048):
    """Score the R rows of h (..., H) - the top layer's outputs - under Linear(weight (V, H), bias (V) or None).  Per chunk of at most
    chunk_rows rows: the library GEMM's (rows, V) scores, then ONE vmlmf_score_rows launch, a workgroup per row (include/vmlmf_score.h
    has the contract), so the score buffer never exceeds chunk_rows x V (the default is linear_nll's).
    targets (R) int64 on the device, or None: the token each row is asked about; an entry < 0 is a row without a target.
    Returns (logprobs (R), ranks (R) int32): the untempered log-softmax of the target (bias included; what nll_loss charges for it;
    for the greedy token, on the same GEMM scores, what vmlmf_lm_choose - lm_sample's form "gemm" - reports, to the bit; lm_sample's
    fused form builds its scores differently and agrees in rounding only) and the number of tokens ahead of it in the project's one total
    order - larger score first, equal scores to the lower index -, 0 where greedy decoding would have chosen it.  A row without a
    target gives (0.0, -1).  top in [1, min(32, V)] adds (top_tokens (R, top) int64, top_logprobs (R, top)): the first `top` tokens of
    that order, in order, and their log-probabilities.
    A target >= V is the caller's error: it is not looked for (that would be a host synchronisation), nothing outside the row is
    read for it, and its row gives (NaN, -1).  No autograd, no host synchronisation: capturable."""
    if not (isinstance(weight, torch.Tensor) and weight.dim() == 2):
        raise ValueError("vmlmf_amd.lm_score: weight must be a (V, H) tensor")
    V = weight.shape[0]
    k = _score.check_top(top, V)
    chunk_rows = _check_chunk_rows(chunk_rows, "lm_score")
    for t, what in ((h, "h"), (weight, "weight")):
        _require_hip(t, what)
    if bias is not None:
        _require_hip(bias, "bias")
    h2 = h.detach().reshape(-1, h.shape[-1]).contiguous()
    R, H = h2.shape
    w = weight.detach().contiguous()
    if w.shape[1] != H or (bias is not None and tuple(bias.shape) != (V,)):
        raise RuntimeError(f"vmlmf_amd.lm_score: h {tuple(h.shape)}, weight {tuple(weight.shape)}, bias must be (V)")
    if targets is not None and not (isinstance(targets, torch.Tensor) and targets.is_cuda and targets.dtype == torch.int64
                                    and targets.numel() == R):
        raise RuntimeError(f"vmlmf_amd.lm_score: targets must be {R} int64 on the device, one per row of h")
    dev = h2.device
    y = None if targets is None else targets.reshape(-1).contiguous()
    b = None if bias is None else bias.detach().contiguous()
    logp = torch.empty(R, device=dev, dtype=torch.float32)
    rank = torch.empty(R, device=dev, dtype=torch.int32)
    toks = torch.empty((R, k), device=dev, dtype=torch.int64) if k > 0 else None
    tlp = torch.empty((R, k), device=dev, dtype=torch.float32) if k > 0 else None
    if R > 0:
        with torch.no_grad():
            buf = torch.empty((min(chunk_rows, R), V), device=dev, dtype=torch.float32)
            wt = w.t()
            for lo in range(0, R, chunk_rows):
                hi = min(lo + chunk_rows, R)
                scores = torch.mm(h2[lo:hi], wt, out=buf[:hi - lo])
                _score.score_rows(scores, b, None if y is None else y[lo:hi], k, logp[lo:hi], rank[lo:hi],
                                  None if k == 0 else toks[lo:hi], None if k == 0 else tlp[lo:hi])
    return (logp, rank) if k == 0 else (logp, rank, toks, tlp)


def score(model, tokens, targets=None, states=None, lengths=None, top=0, chunk_rows=2048):
    """Model.score (lm.py has the contract)."""
    from . import decoding
    k = _score.check_top(top, model.vocab_size, "Model.score")
    chunk_rows = _check_chunk_rows(chunk_rows, "Model.score")
    if not (isinstance(tokens, torch.Tensor) and tokens.dim() == 2 and tokens.dtype == torch.int64):
        raise ValueError("vmlmf_amd: Model.score takes (T, B) int64 tokens, time-major")
    if targets is None:
        if tokens.shape[0] < 2:
            raise ValueError(f"vmlmf_amd: Model.score without targets takes (T + 1, B) tokens, T >= 1; got {tuple(tokens.shape)}")
    elif not (isinstance(targets, torch.Tensor) and targets.dtype == torch.int64 and targets.shape == tokens.shape and tokens.shape[0] >= 1):
        raise ValueError(f"vmlmf_amd: Model.score takes int64 targets of the tokens' shape {tuple(tokens.shape)}, T >= 1")
    B = tokens.shape[1]
    check_lengths(lengths, B, "Model.score")
    decoding._check_call(model, tokens, "score", "scoring kernel (vmlmf_score_rows)")
    if targets is not None:
        decoding._check_call(model, targets, "score", "scoring kernel (vmlmf_score_rows)")
    inputs, y = (tokens[:-1], tokens[1:]) if targets is None else (tokens, targets)
    T, dev = inputs.shape[0], tokens.device
    if lengths is not None:
        y = y.masked_fill(torch.arange(T, device=dev)[:, None] >= lengths.to(dev)[None, :], -1)
    with decoding._activations(model, inputs, states) as (h, states):
        out = lm_score(h, model.fc.w, model.fc.b, y.reshape(-1), k, chunk_rows)
    return (*(t.view(T, B, *t.shape[1:]) for t in out), states)


def cache_score(model, tokens, targets=None, *, theta=0.3, lam=0.1, window=500, cache=None, states=None, return_parts=False,
                chunk_rows=2048):
    """Model.cache_score (lm.py has the contract)."""
    from . import decoding
    H = model.hidden_size
    window, theta, lam = _ncache.check_ncache(window, theta, lam, H)
    chunk_rows = _check_chunk_rows(chunk_rows, "Model.cache_score")
    if not (isinstance(tokens, torch.Tensor) and tokens.dim() == 2 and tokens.dtype == torch.int64):
        raise ValueError("vmlmf_amd: Model.cache_score takes (T, B) int64 tokens, time-major")
    if targets is None:
        if tokens.shape[0] < 2:
            raise ValueError(f"vmlmf_amd: Model.cache_score without targets takes (T + 1, B) tokens, T >= 1; got {tuple(tokens.shape)}")
    elif not (isinstance(targets, torch.Tensor) and targets.dtype == torch.int64 and targets.shape == tokens.shape and tokens.shape[0] >= 1):
        raise ValueError(f"vmlmf_amd: Model.cache_score takes int64 targets of the tokens' shape {tuple(tokens.shape)}, T >= 1")
    B = tokens.shape[1]
    if cache is not None:
        if not isinstance(cache, NeuralCache):
            raise ValueError(f"vmlmf_amd: Model.cache_score: cache must be a NeuralCache, got {type(cache).__name__}")
        if (cache.B, cache.H, cache.window) != (B, H, window):
            raise ValueError(f"vmlmf_amd: Model.cache_score: the cache is one of B={cache.B}, H={cache.H}, window={cache.window}; the call "
                             f"needs B={B}, H={H}, window={window}")
    decoding._check_call(model, tokens, "cache_score", "cache-scoring kernel (vmlmf_ncache_score)")
    if targets is not None:
        decoding._check_call(model, targets, "cache_score", "cache-scoring kernel (vmlmf_ncache_score)")
    inputs, y = (tokens[:-1], tokens[1:]) if targets is None else (tokens, targets)
    T = inputs.shape[0]
    if cache is None:
        cache = NeuralCache(B, H, tokens.device, window)
    with decoding._activations(model, inputs, states) as (h, states):
        lv = lm_score(h, model.fc.w, model.fc.b, y.reshape(-1), 0, chunk_rows)[0].view(T, B)
        logp, lc = lm_cache_score(h, y, lv, cache, theta, lam)
    return (logp, lv, lc, states, cache) if return_parts else (logp, states, cache)
