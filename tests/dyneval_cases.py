"""Dynamic evaluation (vmlmf_amd.dyneval; docs/design/lm_dyneval.md): the fp64 oracle of the two formulas and of the whole loop, and the
fixtures the CPU and GPU tests share.  numpy / torch fp64 only: nothing here touches the code under test."""
import numpy as np
import torch

U = 2.0 ** -24            # unit roundoff of fp32, round to nearest
# roundings in the update kernel's operation order (docs/design/lm_dyneval.md, "Rounding"): 1/m to fp32, decay * (1/m), * r, theta0 - theta,
# ld * d (5); norm + 1e-6, max_norm / ., lr * c, r + eps, g / ., s * q (6); theta + pull, - update (2)
K_ROUNDINGS = 13
NORM_RTOL = 1e-5          # the norm against fp64: what test_clip_sgd_step_matches_the_lm_loop holds sqsum_kernel + norm_kernel to

# hyper-parameters that are fp32 numbers, so that the oracle and the kernel start from the same values
LR, DECAY, EPS = 2.0 ** -10, 0.5, 2.0 ** -17


def step_oracle(theta, theta0, r, g, *, lr, decay, m, eps, max_norm):
    """The update rule in fp64 on lists of arrays.  Returns (new, norm, scale, clamped): per tensor the updated parameters, the bound's
    magnitude |theta| + |ld (theta0 - theta)| + |lr c g / (r + eps)|, and where decay r / m > 1 (the clamp binds).  A norm that is
    not finite: new = theta."""
    theta, theta0, r, g = ([np.asarray(a, np.float64) for a in seq] for seq in (theta, theta0, r, g))
    with np.errstate(invalid="ignore", over="ignore"):
        norm = np.sqrt(sum(float((a * a).sum()) for a in g))
    if not np.isfinite(norm):
        return [a.copy() for a in theta], norm, [np.abs(a) for a in theta], [decay * a / m > 1 for a in r]
    c = 1.0 if max_norm <= 0 else min(1.0, max_norm / (norm + 1e-6))
    new, scale, clamped = [], [], []
    for p, p0, ri, gi in zip(theta, theta0, r, g):
        raw = decay * ri / m
        pull = np.minimum(raw, 1.0) * (p0 - p)
        upd = lr * c * gi / (ri + eps)
        new.append(p + pull - upd)
        scale.append(np.abs(p) + np.abs(pull) + np.abs(upd))
        clamped.append(raw > 1)
    return new, norm, scale, clamped


def update_term(r, g, *, lr, eps, max_norm, norm):
    """|lr c g / (r + eps)| per tensor in fp64: what an error of the norm (through c) is multiplied into."""
    c = 1.0 if max_norm <= 0 else min(1.0, max_norm / (norm + 1e-6))
    return [np.abs(lr * c * np.asarray(gi, np.float64) / (np.asarray(ri, np.float64) + eps)) for ri, gi in zip(r, g)]


def accumulate_oracle(ms, grads):
    return [np.asarray(m, np.float64) + np.asarray(g, np.float64) ** 2 for m, g in zip(ms, grads)]


def mean_rms(r):
    """m: the mean over the tensors of each tensor's mean of r."""
    return float(np.mean([np.asarray(a, np.float64).mean() for a in r]))


# ---- tensor lists that reach every path of the kernels ----
# numels: every n % 4, below / at / above one workgroup's 1024 elements, several workgroups.  pad: state offsets rounded up to
# multiples of four (all four streams 16-byte aligned: the wide path) or packed (offsets 1, 4, 8, 13, ...: the scalar loop under an
# aligned parameter).  misalign: {index: "param" | "grad"} - that tensor is a one-float-offset view of a larger allocation.
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 4099]
STEP_CASES = {
    "padded": dict(numels=SIZES, pad=True, misalign={}),
    "packed_offsets": dict(numels=SIZES, pad=False, misalign={}),
    "misaligned_views": dict(numels=SIZES, pad=True, misalign={6: "param", 7: "grad", 2: "param"}),
    "count_1": dict(numels=[4099], pad=True, misalign={}),
    "count_48": dict(numels=[SIZES[i % 8] if i % 8 < 7 else 7 for i in range(48)], pad=False, misalign={}),
    "million": dict(numels=[5, 2 ** 20 + 3, 1025], pad=True, misalign={}),     # sqsum_kernel on 1024-thread workgroups
}


def offsets_of(numels, pad):
    out, total = [], 0
    for n in numels:
        out.append(total)
        total += (n + 3) // 4 * 4 if pad else n
    return out, total


def step_case(numels, seed):
    """fp32 arrays (theta, theta0, r, g) per tensor.  r is log-uniform over two decades, so that decay r / m passes 1 on part of the
    elements at DECAY = 0.5 and stays below on the rest."""
    rng = np.random.Generator(np.random.PCG64(seed))
    theta = [rng.standard_normal(n).astype(np.float32) * 0.1 for n in numels]
    theta0 = [(t + 0.02 * rng.standard_normal(t.size)).astype(np.float32) for t in theta]
    r = [(10.0 ** rng.uniform(-3.0, -1.0, n)).astype(np.float32) for n in numels]
    g = [(ri * rng.standard_normal(ri.size)).astype(np.float32) for ri in r]
    return theta, theta0, r, g


def flat_state(per_tensor, offsets, total):
    flat = np.zeros(total, np.float32)
    for a, o in zip(per_tensor, offsets):
        flat[o:o + a.size] = a
    return flat


def butterfly_sum(rows):
    """The sum of at most 64 fp32 row losses in the order the head loss's finish launch takes it (one row per lane, a wave-wide
    xor butterfly 32, 16, 8, 4, 2, 1; the other three waves add zeros): Model.loss = scale * this, to the bit."""
    v = torch.zeros(64, dtype=torch.float32)
    v[:rows.numel()] = rows.detach().reshape(-1).cpu()
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[lane ^ o]
    return v[0]


# ---- the whole loop in fp64 ----
def rows_and_loss(scores, y):
    """(rows, loss) of Model.loss at its defaults from (T B, V) scores: rows = logsumexp - target score, loss = B / (T B) * sum."""
    rows = scores.logsumexp(1) - scores.gather(1, y.reshape(-1, 1)).squeeze(1)
    return rows, rows.sum() * (float(y.shape[1]) / float(rows.numel()))


def loop_oracle(forward, params, r, m, x, y, states, *, segment, lr, decay, eps, max_norm):
    """Dynamic evaluation of a model given as a callable, in fp64: forward(params, x, states) -> ((T B, V) scores, states) under
    autograd on `params` (a list of fp64 leaf tensors, adapted in place); r: one array per parameter.  theta0 is params on entry.
    Returns (logprobs (T, B) fp64 numpy, states)."""
    theta0 = [p.detach().numpy().copy() for p in params]
    T, B = x.shape
    out = np.zeros((T, B))
    for lo in range(0, T, segment):
        hi = min(lo + segment, T)
        for p in params:
            p.grad = None
        scores, states = forward(params, x[lo:hi], states)
        rows, loss = rows_and_loss(scores, y[lo:hi])
        loss.backward()
        out[lo:hi] = -rows.detach().numpy().reshape(hi - lo, B)
        new, _, _, _ = step_oracle([p.detach().numpy() for p in params], theta0, r, [p.grad.numpy() for p in params],
                                   lr=lr, decay=decay, m=m, eps=eps, max_norm=max_norm)
        with torch.no_grad():
            for p, a in zip(params, new):
                p.copy_(torch.from_numpy(a.reshape(p.shape)))
        states = [(h.detach(), c.detach()) for h, c in states]
    return out, states


def module_forward(model64):
    """forward for loop_oracle from a Model in fp64 stock ops (lstm_type="custom"): the parameters ARE the module's."""
    def forward(params, x, states):
        h, states = model64.features(x, list(states))
        return torch.addmm(model64.fc.b, h.reshape(-1, h.shape[-1]), model64.fc.w.t()), states
    return forward


def literal_forward(names, layer_num):
    """forward for loop_oracle on the oracle's literal VMLMF language model (vmlmf_oracle.literal_lm_forward)."""
    import vmlmf_oracle as O

    def forward(params, x, states):
        return O.literal_lm_forward(dict(zip(names, params)), x, states, layer_num)
    return forward
