"""Decoding the LM (Model.generate, C ABI vmlmf_lm_sample): what can be checked without a GPU - the entry points' argument checks
(host only: they refuse before anything reaches a device), the workspace size, and the numpy restatement of the sampler's draw that
the GPU tests hold the kernel to (vmlmf_decode_oracle.gumbel_restated), checked on itself."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from vmlmf_amd import _lib
from vmlmf_decode_oracle import SITE_SAMPLE, gumbel_restated

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "vmlmf_hip.h")


def _sample(B=2, H=8, V=16, h=1, w=1, bias=None, embed=None, inv=0.0, state=None, step=0, tokens=1, logp=None, xn=None,
            ticket=1, ws=1, nbytes=1 << 20):
    """vmlmf_lm_sample with fake, never dereferenced pointers (1 = some non-null address)."""
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    lib = _lib.lib()
    rc = lib.vmlmf_lm_sample(B, H, V, p(h), p(w), p(bias), p(embed), inv, p(state), step, p(tokens), p(logp), p(xn), p(ticket), p(ws),
                             nbytes, None)
    return rc, lib.vmlmf_last_error().decode()


def test_the_sampler_refuses_bad_arguments_on_the_host():
    cases = [
        (dict(B=0), _lib.E_BADARG, "B, H, V"), (dict(H=0), _lib.E_BADARG, "B, H, V"), (dict(V=-3), _lib.E_BADARG, "B, H, V"),
        (dict(h=None), _lib.E_BADARG, "null"), (dict(w=None), _lib.E_BADARG, "null"), (dict(tokens=None), _lib.E_BADARG, "null"),
        (dict(ticket=None), _lib.E_BADARG, "null"), (dict(ws=None), _lib.E_BADARG, "null"),
        (dict(inv=-1.0), _lib.E_BADARG, "temperature"), (dict(inv=float("nan")), _lib.E_BADARG, "temperature"),
        (dict(inv=float("inf")), _lib.E_BADARG, "temperature"),
        (dict(inv=1.0, state=None), _lib.E_BADARG, "snapshot"),
        (dict(xn=1, embed=None), _lib.E_BADARG, "embedding"),
        (dict(step=-1), _lib.E_BADARG, "step"),
        (dict(B=1 << 16, step=1 << 16), _lib.E_UNSUPPORTED, "2^32"),
        (dict(nbytes=0), _lib.E_WORKSPACE, "workspace"),
    ]
    for kw, code, words in cases:
        rc, msg = _sample(**kw)
        assert rc == code and words in msg, (kw, rc, msg)


def test_workspace_size_is_monotone_in_rows_and_vocabulary():
    lib = _lib.lib()
    assert lib.vmlmf_lm_sample_workspace_bytes(0, 100) == 0 and lib.vmlmf_lm_sample_workspace_bytes(4, 0) == 0
    prev_v = 0
    for V in (1, 15, 16, 17, 97, 1000, 8191, 8192, 8193, 10000, 50000, 262144):
        prev_b = 0
        for B in (1, 2, 16, 17, 32, 256, 4096):
            n = lib.vmlmf_lm_sample_workspace_bytes(B, V)
            assert n >= prev_b and n > 0
            prev_b = n
        n = lib.vmlmf_lm_sample_workspace_bytes(32, V)
        assert n >= prev_v
        prev_v = n
    # at the PTB size one step holds (B rows x strips) partials of 32 bytes: 2 MB at B = 256
    assert lib.vmlmf_lm_sample_workspace_bytes(256, 10000) <= 4 << 20


def test_the_restated_draw_stays_inside_the_unit_interval_on_a_site_of_its_own():
    u, g = gumbel_restated(0x1234_5678_9ABC_DEF, 3, 5, 64, 1000)
    assert (u > 0).all() and (u < 1).all() and np.isfinite(g).all()
    assert ((0x00 + 0.5) * 2.0 ** -24) > 0 and ((0xFFFFFF + 0.5) * 2.0 ** -24) < 1   # the extreme words
    assert abs(u.mean() - 0.5) < 5 * np.sqrt(1 / 12 / u.size)
    assert abs(g.mean() - np.euler_gamma) < 5 * np.sqrt(np.pi ** 2 / 6 / g.size)      # Gumbel(0, 1): mean = Euler's gamma
    # the header and the binding name the same site, and no dropout site (0 = the embedding, l + 1 = layer l) can be it
    m = re.search(r"#define VMLMF_SITE_SAMPLE (0x[0-9A-Fa-f]+)", open(HEADER).read())
    assert m and int(m.group(1), 16) == _lib.SITE_SAMPLE == SITE_SAMPLE
    assert _lib.SITE_SAMPLE > 1 << 16
    # a different step, row, seed or offset is a different stream of words
    for args in ((0x1234_5678_9ABC_DEF, 3, 6), (0x1234_5678_9ABC_DEF, 4, 5), (7, 3, 5)):
        u2, _ = gumbel_restated(*args, 64, 1000)
        assert not np.array_equal(u, u2)


def test_generate_refuses_cpu_tensors():
    from vmlmf_amd import Model
    torch.manual_seed(0)
    m = Model(97, 32, 2, 0.0, 0.1, w_rank=8, u_ranks=[8], lstm_type="vmlmf")
    with pytest.raises(RuntimeError, match="cuda"):
        m.generate(torch.zeros((3, 2), dtype=torch.int64), 4)
    from vmlmf_amd import lm_sample
    with pytest.raises(RuntimeError, match="cuda"):
        lm_sample(torch.zeros(2, 32), m.fc.w.detach(), m.fc.b.detach(), 0.0)


GENERATE = ["prompt", "steps", "states", "temperature", "seed", "chunk", "layer_path", "top_k", "top_p", "eos", "min_length",
            "repetition_penalty", "logit_bias", "banned_tokens", "return_lengths", "no_repeat_ngram_size", "banned_sequences",
            "frequency_penalty", "presence_penalty"]
BEAM_SEARCH = ["prompt", "steps", "beams", "states", "eos", "length_penalty", "chunk", "min_length", "banned_tokens", "no_repeat_ngram_size",
               "banned_sequences"]


def test_the_decoders_signatures():
    """Model.generate / Model.beam_search and decoding's functions behind them: the positional parameters are what they have been, in
    their order; what came later - the truncation samplers, the automaton - is keyword-only and None by default."""
    from vmlmf_amd import Model, TokenAutomaton, decoding
    table = [(Model.generate, decoding.generate, GENERATE, "generate", {"no_repeat_ngram_size": 0, "banned_sequences": None,
                                                                        "frequency_penalty": 0.0, "presence_penalty": 0.0},
              ["min_p", "typical_p", "epsilon_cutoff", "eta_cutoff", "automaton", "automaton_state"]),
             (Model.beam_search, decoding.beam_search, BEAM_SEARCH, "beam_search", {"min_length": 0, "banned_tokens": None,
                                                                                    "no_repeat_ngram_size": 0, "banned_sequences": None},
              ["automaton", "automaton_state"])]
    for method, function, positional, name, defaults, keywords in table:
        for fn, first in ((method, "self"), (function, "model")):
            params = inspect.signature(fn).parameters
            assert [n for n, p in params.items() if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD] == [first] + positional
            assert list(params) == [first] + positional + keywords                  # ... and nothing of another kind
            assert {n: params[n].default for n in defaults} == defaults
            assert all(params[n].kind is inspect.Parameter.KEYWORD_ONLY and params[n].default is None for n in keywords)
            assert fn.__name__ == name
        assert "keyword-only" in method.__doc__ and "automaton" in method.__doc__
    torch.manual_seed(0)
    m, tok = Model(8, 8, 1, 0.0, 0.1, w_rank=4, u_ranks=[4], lstm_type="vmlmf"), torch.zeros((3, 2), dtype=torch.int64)
    a = TokenAutomaton.forced(8, [1])
    for call in (m.generate, m.beam_search):
        with pytest.raises(RuntimeError, match="cuda"):                      # accepted as keywords ...
            call(tok, 4, automaton=a, automaton_state=None)
        with pytest.raises(RuntimeError, match="cuda"):                      # ... and None is "not given": the call it was
            call(tok, 4, automaton=None, automaton_state=None)
        with pytest.raises(TypeError):
            call(tok, 4, automatons=a)
    with pytest.raises(RuntimeError, match="cuda"):
        m.generate(tok, 4, min_p=0.1, typical_p=None, epsilon_cutoff=None, eta_cutoff=None)
    with pytest.raises(TypeError):
        m.generate(tok, 4, min_ps=0.1)
    with pytest.raises(TypeError):
        m.generate(tok, 4, None, 1.0, None, None, "layers", None, None, None, 0, 1.0, None, None, False, 0, None, 0.0, 0.0, a)   # keyword-only
    with pytest.raises(TypeError):
        m.beam_search(tok, 4, 4, None, None, 0.0, None, 0, None, 0, None, a)
