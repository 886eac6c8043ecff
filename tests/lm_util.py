"""What the decoder's GPU tests share (test_gpu_generate*.py, test_gpu_decode_controls.py, test_gpu_beam.py, test_gpu_score.py and the
CPU tests of their cases): the small 97-token models, prompts, the teacher-forced oracle run and the kernel-level cases on the device.
The contracts themselves are oracle/vmlmf_decode_oracle.py's.  Importing this touches no device."""
import functools

import numpy as np
import torch

from vmlmf_decode_oracle import LP_TOL, MARGIN, MODEL_EOS, SEED, _oracle_scores, case_inputs  # noqa: F401 (LP_TOL, MARGIN: for the tests)

DEV = "cuda"


def _small(kind):
    from vmlmf_amd import Model
    torch.manual_seed({"plain": 1, "group": 2, "wide": 3, "wide300": 4}[kind])
    if kind == "plain":
        m = Model(97, 32, 2, 0.0, 0.3, w_rank=8, u_ranks=[8], lstm_type="vmlmf")
    elif kind == "group":
        m = Model.with_group_layers(97, 32, 2, 0.0, 0.3, w_rank=8, u_ranks=[8, 8])
    elif kind == "wide":   # padded u_rank 48 > 32: the step-wise wide-rank layers
        m = Model(97, 64, 2, 0.0, 0.2, w_rank=40, u_ranks=[48], lstm_type="vmlmf")
    else:                  # the LM default's hidden rank, u_ranks = 300
        m = Model(97, 320, 2, 0.0, 0.05, w_rank=32, u_ranks=[300], lstm_type="vmlmf")
    return m.to(DEV)


def beam_model(kind):
    """The models of the model-level cases (CPU; winit 1.0: at the usual 0.3 the distribution is nearly uniform and the top-W boundary
    falls inside the margin), fc.b[3] raised so that eos = 3 is emitted by some beams and not by all."""
    from vmlmf_amd import Model
    if kind == "plain":
        torch.manual_seed(1)
        m = Model(97, 32, 2, 0.0, 1.0, w_rank=8, u_ranks=[8], lstm_type="vmlmf")
    else:
        torch.manual_seed(2)
        m = Model.with_group_layers(97, 32, 2, 0.0, 1.0, w_rank=8, u_ranks=[8, 8])
    with torch.no_grad():
        m.fc.b[MODEL_EOS] += 2.0
    return m


def _check_choices(z, tokens, margin, what):
    """z (steps, B, V) fp64 criterion; tokens (steps, B): argmax, or within `margin` of it."""
    z = z.numpy()
    t = tokens.cpu().numpy()
    best = z.max(-1)
    picked = np.take_along_axis(z, t[..., None], -1)[..., 0]
    exact = (t == z.argmax(-1))
    assert (best - picked <= margin).all(), (what, np.argwhere(best - picked > margin)[:5])
    assert exact.mean() > 0.9, (what, exact.mean())


def _prompt(B, T0=5, V=97, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, V, (T0, B), generator=g).to(DEV)


def cpu_prompt(B, T0=5, V=97, seed=0):
    """_prompt's draws, left on the CPU."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, V, (T0, B), generator=g)


def _teacher_forced(m, prompt, tokens):
    T0 = prompt.shape[0]
    seq = torch.cat([prompt.cpu(), tokens.cpu()])
    scores, states = _oracle_scores(m, seq)
    return scores[T0 - 1:T0 - 1 + tokens.shape[0]], states


def _snap(seed=SEED):
    from vmlmf_amd import dropout_advance, dropout_state
    return dropout_advance(dropout_state(DEV, seed))


@functools.lru_cache(maxsize=None)
def _on_device(B, H, V):
    return tuple(t.to(DEV) for t in case_inputs(B, H, V))


def _tied_row():
    """h (16), w (97, 16), bias (97) whose scores are exact in fp32 in any order of summation (small dyadic numbers): token 40 scores
    2.5, tokens 5, 20 and 60 carry identical rows and the second-highest score 2.0, every other token stays below 1."""
    g = torch.Generator().manual_seed(4)
    h = torch.randint(0, 2, (16,), generator=g).float() * 2 - 1            # +-1
    w = torch.randint(-8, 9, (97, 16), generator=g).float() / 128           # |score| <= 1
    bias = torch.zeros(97)
    for v in (5, 20, 60):
        w[v] = h / 8
    w[40] = h * 5 / 32
    return h, w, bias
