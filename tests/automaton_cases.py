"""Decoding under a token automaton (vmlmf_amd.TokenAutomaton; C ABI vmlmf_automaton_choose / vmlmf_automaton_beam_step in
libvmlmf_automaton.so, include/vmlmf_automaton.h) stated in numpy, with the seeded cases that test_automaton_cpu.py and
test_gpu_automaton.py share.  A table only CLOSES tokens: the kernel tests compare with the project's own kernels under an equivalent
-inf bias (vmlmf_decode_choose) or ban bitmap (vmlmf_beamctl_step), bit for bit - no tolerance appears here.  Test-side code: nothing
here imports the package."""
import itertools

import numpy as np

import beam_control_cases as K  # noqa: F401 (pack: a ban set's words)
import history_cases as HC      # noqa: F401 (ban_set: the rule of banned_sequences)

EOS = 7


# ---- the rule ----
def closes(nxt, s):
    """(V) bool: what state s of the (S, V) table does not offer; everything for a state outside [0, S)."""
    S, V = nxt.shape
    return np.ones(V, dtype=bool) if not 0 <= int(s) < S else nxt[int(s)] < 0


def step_state(nxt, s, token, finished_before=False, dead=False):
    """A row's state behind its choice: unchanged for a finished row and for one that had nothing to choose."""
    return int(s) if finished_before or dead else int(nxt[int(s), int(token)])


def walk(nxt, start, tokens, eos=None):
    """The state behind `tokens` from `start`, or None where a transition is closed; with eos, the walk ends behind the first eos."""
    s = int(start)
    for t in tokens:
        if not 0 <= s < nxt.shape[0] or nxt[s, int(t)] < 0:
            return None
        s = int(nxt[s, int(t)])
        if eos is not None and int(t) == eos:
            break
    return s


def language(nxt, start, V, length):
    """Every sequence of exactly `length` tokens the automaton can emit from `start`, by brute force over V ** length sequences."""
    return {seq for seq in itertools.product(range(V), repeat=length) if walk(nxt, start, seq) is not None}


def survivor_states(nxt, beam_state, parent, token, total, finished):
    """beam_state_out (B W) of a beam step: beam_state (B W), parent / token / total (B, W) of the step's output, finished (B, W) of its
    INPUT.  A finished parent's state is copied; a slot without a candidate (NaN total) gets -1."""
    B, W = parent.shape
    out = np.full(B * W, -1, dtype=np.int32)
    for b in range(B):
        for r in range(W):
            if np.isnan(total[b, r]):
                continue
            prow = b * W + int(parent[b, r])
            out[b * W + r] = beam_state[prow] if finished[b, int(parent[b, r])] else nxt[beam_state[prow], int(token[b, r])]
    return out


# ---- seeded tables ----
def random_table(S, V, seed, share=0.5, keep_open=()):
    """(S, V) int32: every transition open with probability `share`, to a uniformly drawn state; the tokens of keep_open are open
    everywhere.  From PCG64(seed + 1000 S + V)."""
    rng = np.random.Generator(np.random.PCG64(seed + 1000 * S + V))
    nxt = rng.integers(0, S, size=(S, V)).astype(np.int32)
    nxt[rng.random((S, V)) >= share] = -1
    for t in keep_open:
        nxt[nxt[:, t] < 0, t] = 0
    return nxt


def neutral_table(V):
    return np.zeros((1, V), dtype=np.int32)


# ---- kernel level: the choice ----
CHOICE_V = [97, 4096, 12288, 12289]      # not a multiple of 32; the last resident length; the first re-reading length
CHOICE_B = [1, 3]
CHOICE_S = [1, 5]
CHOICE_MODES = {"greedy": (0.0, 0, 1.0), "sample": (0.9, 0, 1.0), "k7p0.8": (0.9, 7, 0.8)}      # temperature, top_k, top_p
CHOICE_STEP, CHOICE_H, THETA, MIN_LENGTH = 3, 16, 1.3, 4


def choice_case(B, S, V):
    """The inputs of a K1 case: scores (B, V) - a seeded randn scaled by 3: no ties -, bias (V), embed (V, H), the controls (a finite
    logit bias with one ban, seen, finished, length) and the table with the rows' states.  With B = 3 row 1 is finished, the rows sit in
    different states, and rows 0 and 2 lie below and above MIN_LENGTH."""
    rng = np.random.Generator(np.random.PCG64(11 + 100 * B + 10 * S + V))
    scores = (3.0 * rng.standard_normal((B, V))).astype(np.float32)
    bias = rng.standard_normal(V).astype(np.float32)
    embed = rng.standard_normal((V, CHOICE_H)).astype(np.float32)
    lb = (0.5 * rng.standard_normal(V)).astype(np.float32)
    lb[5] = -np.inf
    seen = (rng.random((B, V)) < 0.3).astype(np.uint8)
    finished = np.zeros(B, dtype=np.int32)
    length = np.array([2, 9, 6][:B], dtype=np.int32)
    if B == 3:
        finished[1] = 1
    nxt = random_table(S, V, 5, keep_open=(EOS,))
    state = np.array([(2 * b + 1) % S for b in range(B)], dtype=np.int32)
    return dict(scores=scores, bias=bias, embed=embed, logit_bias=lb, seen=seen, finished=finished, length=length, next=nxt, state=state)


# ---- kernel level: the beam step ----
BEAM_SHAPES = [(1, 1), (1, 4), (3, 5), (2, 32)]
BEAM_V = [97, 12288, 12289]
BEAM_H, BEAM_S, BEAM_MIN_LENGTH = 16, 5, 3


def beam_case(B, W, V, first_step=False):
    """The inputs of a B1 case: scores (B W, V), bias, embed, cum (B, W), finished, length, the shared closed mask, the table and the
    beams' states (all different where S allows).  One beam per batch row is finished (W > 1); first_step: a search that starts - cum 0,
    -inf, ..., nothing finished, length 0, every beam in state 0."""
    rng = np.random.Generator(np.random.PCG64(23 + 1000 * B + 10 * W + V))
    scores = (3.0 * rng.standard_normal((B * W, V))).astype(np.float32)
    bias = rng.standard_normal(V).astype(np.float32)
    embed = rng.standard_normal((V, BEAM_H)).astype(np.float32)
    closed = rng.random(V) < 0.125
    closed[EOS] = False
    nxt = random_table(BEAM_S, V, 9, keep_open=(EOS,))
    if first_step:
        cum = np.full((B, W), -np.inf, dtype=np.float32)
        cum[:, 0] = 0.0
        finished = np.zeros((B, W), dtype=np.int32)
        length = np.zeros((B, W), dtype=np.int32)
        state = np.zeros(B * W, dtype=np.int32)
    else:
        cum = (-3.0 * rng.random((B, W))).astype(np.float32)
        finished = np.zeros((B, W), dtype=np.int32)
        if W > 1:
            finished[:, W - 1] = 1
        length = ((np.arange(B * W) * 3) % 5 + 1).astype(np.int32).reshape(B, W)
        state = ((np.arange(B * W) * 2 + 1) % BEAM_S).astype(np.int32)
    return dict(scores=scores, bias=bias, embed=embed, cum=cum, finished=finished, length=length, closed=closed, next=nxt, state=state)


def beam_bans(nxt, state):
    """(B W, V) bool: per beam, what its state closes - the `bans` of the equivalent vmlmf_beamctl_step call."""
    return np.stack([closes(nxt, s) for s in state])


# ---- the sequence sets of `avoiding` ----
AVOID_V = 6
AVOID_SETS = [
    [[1, 2]],
    [[1, 2], [2, 3]],
    [[1, 2, 3], [2, 3]],            # one a suffix of another
    [[1, 2], [1, 2, 3]],            # one a prefix of another
    [[4], [1, 2, 1]],               # a single token; a sequence that overlaps itself
    [[0, 0], [0, 0, 0], [5]],
    [[1, 1, 2], [1, 2, 1], [3, 1, 1]],
]


def contains_any(h, seqs):
    return any(list(h[i:i + len(s)]) == list(s) for s in seqs for i in range(len(h) - len(s) + 1))


def avoid_histories(seqs, count, seed):
    """`count` random histories over AVOID_V tokens (lengths 0 .. 9) that contain none of the sequences."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    while len(out) < count:
        h = rng.integers(0, AVOID_V, size=int(rng.integers(0, 10))).tolist()
        if not contains_any(h, seqs):
            out.append(h)
    return out
