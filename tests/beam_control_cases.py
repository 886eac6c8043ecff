"""The controls of Model.beam_search (min_length, banned_tokens, no_repeat_ngram_size, banned_sequences; C ABI vmlmf_beamctl_step in
libvmlmf_beamctl.so, include/vmlmf_beamctl.h) stated in numpy and fp64, with the seeded cases that test_beam_controls_cpu.py and
test_gpu_beam_controls.py share.  The step's own contract - totals, the order, lo / hi - is oracle/vmlmf_decode_oracle.py's (row_totals
and step_sets take an arbitrary `valid` mask), a row's ban set is history_cases.ban_set.  A control only takes candidates out of
`valid`: a closed candidate is not offered, no total changes.  Test-side code: nothing here imports the package."""
import functools

import numpy as np
import torch

import history_cases as HC
import vmlmf_decode_oracle as C

EOS = C.EOS_KERNEL

# ---- kernel level: a step under seeded masks ----
# (B, W, H, V): the plain step's small case; 33 tokens - the last mask word holds one; a row that does not fit LDS (12 288); W at its
# limit; the PTB size
KERNEL_SHAPES = [(3, 4, 32, 97), (5, 3, 40, 33), (1, 5, 16, 12293), (2, 32, 32, 97), (1, 16, 650, 10000)]
MASK_SEED = 3            # chosen so that every row of every masked case is clear at C.KERNEL_MARGIN (test_beam_controls_cpu.py asserts it)
MASK_SHARE = 0.125       # of the tokens in `closed`, and again in every beam's own bans
KERNEL_MIN_LENGTH = 3    # kernel_case's lengths run 1 .. 5: some live beams are below it


@functools.lru_cache(maxsize=None)
def kernel_masks(case):
    """(closed (V) bool, bans (B W, V) bool) of a kernel-level case, drawn in this order from PCG64(MASK_SEED + 1000 B + V + W); eos is
    left to min_length (it is in neither)."""
    B, W, H, V = case
    rng = np.random.Generator(np.random.PCG64(MASK_SEED + 1000 * B + V + W))
    closed = rng.random(V) < MASK_SHARE
    bans = rng.random((B * W, V)) < MASK_SHARE
    closed[EOS] = False
    bans[:, EOS] = False
    return closed, bans


def pack(mask):
    """(..., V) bool -> (..., ceil(V / 32)) int32 words in vmlmf_history_bans' layout (bit v & 31 of word v >> 5)."""
    mask = np.asarray(mask, dtype=bool)
    V = mask.shape[-1]
    pad = np.zeros(mask.shape[:-1] + ((-V) % 32,), dtype=bool)
    bits = np.concatenate([mask, pad], -1)
    return np.ascontiguousarray(np.packbits(bits, axis=-1, bitorder="little")).view(np.int32)


def controlled_valid(valid, finished, length, eos, closed=None, bans=None, min_length=0):
    """`valid` (W, V) of row_totals with what the controls close taken out, for the LIVE beams of one batch row: closed (V) bool, bans
    (W, V) bool, eos while length[w] < min_length.  A finished beam keeps its eos whatever is closed."""
    valid = valid.copy()
    for w in range(valid.shape[0]):
        if eos is not None and finished[w]:
            continue
        if closed is not None:
            valid[w] &= ~np.asarray(closed, dtype=bool)
        if bans is not None:
            valid[w] &= ~np.asarray(bans[w], dtype=bool)
        if eos is not None and length[w] < min_length:
            valid[w, eos] = False
    return valid


def controlled_step(x, cum, finished, length, eos, W, margin, closed=None, bans=None, min_length=0):
    """One batch row: (totals, valid, top, lo, hi) of step_sets under the controls.  x (W, V) fp64 scores with the bias."""
    totals, valid = C.row_totals(x, cum, finished, eos)
    valid = controlled_valid(valid, finished, length, eos, closed, bans, min_length)
    return (totals, valid) + C.step_sets(totals, valid, W, margin)


@functools.lru_cache(maxsize=None)
def kernel_oracle(case, masked=True):
    """Per batch row (totals, valid, top, lo, hi) of a kernel-level case in fp64: under kernel_masks and KERNEL_MIN_LENGTH, or
    (masked=False) under neutral controls."""
    B, W, H, V = case
    h, w, b, cum, fin, length = C.kernel_case(*case)
    x = (h.double() @ w.double().t() + b.double()).view(B, W, V).numpy()
    closed, bans = kernel_masks(case) if masked else (None, None)
    rows = []
    for r in range(B):
        rows.append(controlled_step(x[r], cum[r].double().numpy(), fin[r].numpy(), length[r].numpy(), EOS, W, C.KERNEL_MARGIN, closed,
                                    None if bans is None else bans[r * W:(r + 1) * W], KERNEL_MIN_LENGTH if masked else 0))
    return rows


def next_histories(hist, hist_len, cap, parent, token, finished):
    """The step's history rule restated: hist (B W, cap), hist_len (B W), parent / token (B, W), finished (B, W) of the step's INPUT ->
    (hist_out as a list of lists: the defined prefix of every slot, hist_len_out, overflow (B))."""
    B, W = parent.shape
    out, lens, over = [], [], [0] * B
    for b in range(B):
        for r in range(W):
            prow = b * W + int(parent[b, r])
            L = int(hist_len[prow])
            row = [int(t) for t in hist[prow][:L]]
            if finished[b, int(parent[b, r])]:
                pass
            elif L < cap:
                row.append(int(token[b, r]))
            else:
                over[b] = 1
            out.append(row)
            lens.append(len(row))
    return out, lens, over


# ---- model level: the oracle's search under controls ----
MODEL_STEPS, MODEL_EOS = C.MODEL_STEPS, C.MODEL_EOS
assert (MODEL_STEPS, MODEL_EOS) == (12, 3)
SETTINGS = ["n2", "n2_min6", "n3_min6_seqs"]


def oracle_beam_search(m, prompt, W, steps, eos, n=0, seqs=(), banned=(), min_length=0):
    """C.oracle_beam_search with the controls: valid[w] &= ~(ban_set(prompt + hypothesis) | closed) for live beams, eos cleared below
    min_length, lengths carried.  Returns (clear: one bool per (step, batch row), finished (B, W), hyps (steps, B, W), cum (B, W),
    length (B, W))."""
    T0, B = prompt.shape
    hyps = np.zeros((0, B, W), dtype=np.int64)
    cum = np.full((B, W), -np.inf)
    cum[:, 0] = 0.0
    fin = np.zeros((B, W), dtype=bool)
    length = np.zeros((B, W), dtype=np.int64)
    clear = []
    pr = prompt.numpy()
    for j in range(steps):
        seqs_in = torch.cat([prompt[:, :, None].expand(T0, B, W), torch.from_numpy(hyps)]).reshape(T0 + j, B * W)
        x, _ = C.oracle_last_scores(m, seqs_in)
        x = x.reshape(B, W, -1)
        V = x.shape[-1]
        closed = np.zeros(V, dtype=bool)
        closed[list(banned)] = True
        new_h, new_c = np.zeros((j + 1, B, W), dtype=np.int64), np.zeros((B, W))
        new_f, new_l = np.zeros((B, W), dtype=bool), np.zeros((B, W), dtype=np.int64)
        for b in range(B):
            bans = np.stack([HC.ban_set(list(pr[:, b]) + list(hyps[:, b, w]), V, n, list(seqs)) for w in range(W)])
            totals, valid, top, lo, hi = controlled_step(x[b], cum[b], fin[b], length[b], eos, W, C.model_margin(j), closed, bans, min_length)
            clear.append(lo == hi)
            for r, f in enumerate(top):
                par, tok = divmod(int(f), V)
                new_h[:j, b, r], new_h[j, b, r] = hyps[:, b, par], tok
                new_c[b, r], new_f[b, r] = totals[par, tok], fin[b, par] or tok == eos
                new_l[b, r] = length[b, par] + (0 if fin[b, par] else 1)
        hyps, cum, fin, length = new_h, new_c, new_f, new_l
    return clear, fin, hyps, cum, length


def model_and_prompt(kind, B, seed):
    from lm_util import beam_model, cpu_prompt
    return beam_model(kind), cpu_prompt(B, seed=seed)


@functools.lru_cache(maxsize=None)
def uncontrolled(kind, B, W, seed):
    m, prompt = model_and_prompt(kind, B, seed)
    return oracle_beam_search(m, prompt, W, MODEL_STEPS, MODEL_EOS)


def _first_tokens(hyps, b, k, eos):
    """The first k tokens of batch row b's first hypothesis (in the search's final order) that holds no eos among them."""
    for w in range(hyps.shape[2]):
        s = [int(t) for t in hyps[:k, b, w]]
        if eos not in s:
            return s
    raise AssertionError("every hypothesis of the row starts with eos")


@functools.lru_cache(maxsize=None)
def setting(name, kind, B, W, seed):
    """The controls of a model case as keyword arguments of Model.beam_search (eos aside).  The two banned sequences of the third
    setting are the first 2 tokens of batch row 0's and the first 3 of row B - 1's best eos-free hypothesis of the UNCONTROLLED fp64
    search."""
    if name == "n2":
        return dict(no_repeat_ngram_size=2)
    if name == "n2_min6":
        return dict(no_repeat_ngram_size=2, min_length=6)
    assert name == "n3_min6_seqs"
    hyps = uncontrolled(kind, B, W, seed)[2]
    return dict(no_repeat_ngram_size=3, min_length=6,
                banned_sequences=[_first_tokens(hyps, 0, 2, MODEL_EOS), _first_tokens(hyps, B - 1, 3, MODEL_EOS)])


@functools.lru_cache(maxsize=None)
def controlled(name, kind, B, W, seed):
    m, prompt = model_and_prompt(kind, B, seed)
    kw = setting(name, kind, B, W, seed)
    return oracle_beam_search(m, prompt, W, MODEL_STEPS, MODEL_EOS, n=kw.get("no_repeat_ngram_size", 0),
                              seqs=tuple(tuple(s) for s in kw.get("banned_sequences", ())), min_length=kw.get("min_length", 0))


def repeated_ngrams(seq, n):
    """How many n-grams of seq come a second (third ...) time."""
    grams = [tuple(seq[i:i + n]) for i in range(len(seq) - n + 1)]
    return len(grams) - len(set(grams))


def until_eos(tokens, eos):
    """The hypothesis up to and including its first eos."""
    tokens = [int(t) for t in tokens]
    return tokens[:tokens.index(eos) + 1] if eos in tokens else tokens


def contains(seq, sub):
    sub = list(sub)
    return any(list(seq[i:i + len(sub)]) == sub for i in range(len(seq) - len(sub) + 1))
