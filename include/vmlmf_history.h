/* C ABI of libvmlmf_history.so: the choice of the LM decoder under controls that need a row's SEQUENCE of tokens (Model.generate with
 * no_repeat_ngram_size / banned_sequences / frequency_penalty / presence_penalty, vmlmf_amd/lm.py) for the AMD Instinct MI355X
 * (gfx950).  A library of its own beside libvmlmf_hip.so (include/vmlmf_hip.h) and libvmlmf_decode.so (include/vmlmf_decode.h, whose
 * controls it applies too), loaded on the first call that needs it: a generate() without these arguments never opens it.
 *
 * Conventions are vmlmf_hip.h's: every pointer is a device pointer unless it says "host", every launch goes to `stream` (a hipStream_t
 * passed as void*), nothing synchronises.  Return value: 0 = ok, <0 = VMLMF_E_* (the values of vmlmf_hip.h), >0 = hipError_t; the
 * text of the last failure of THIS library is vmlmf_history_last_error() (thread-local).
 */
#ifndef VMLMF_HISTORY_H
#define VMLMF_HISTORY_H

#include <stddef.h>
#include <stdint.h>

#include "vmlmf_hip.h" /* VMLMF_E_* */

#ifdef __cplusplus
extern "C" {
#endif

#define VMLMF_HISTORY_ABI_VERSION 1

/* The largest vocabulary for which history BANS (n-grams, sequences) are accepted.  A row's ban set is a bitmap of ceil(V / 32) words
 * in the workgroup's LDS beside the selection's scratch (55 824 bytes: 12 288 keys, the radix histogram, the reduction and tie-count
 * arrays); a kernel's static LDS ends at 65 536 bytes, which leaves 9 712 - room for 77 696 tokens.  The limit is the largest power of
 * two below that: 65 536 tokens, an 8 192-byte bitmap, 64 016 bytes in all.  The penalties carry no such limit. */
#define VMLMF_HISTORY_MAX_V 65536

int vmlmf_history_abi_version(void);
const char *vmlmf_history_last_error(void);

/* The controls of one decode and its per-row state.  A HOST struct of scalars and device pointers, copied into the launch's arguments.
 * The first eight fields are struct vmlmf_decode_controls, field for field (vmlmf_decode.h: theta, eos, min_length, logit_bias, seen,
 * finished, length).  Beside them:
 *   hist (B, hist_capacity)  int32, row-major: the row's tokens so far, PROMPT INCLUDED, oldest first
 *   hist_len (B)             int32: tokens in hist[b]
 *   count (B, V)             uint16: how often the row has GENERATED the token (the prompt is not counted); saturates at 65535
 *   overflow (B)             int32: set to 1, and never cleared, by a launch that found hist[b] full (see step 7)
 *   seq_tokens, seq_offsets  the banned sequences, flat: sequence s is seq_tokens[seq_offsets[s] .. seq_offsets[s + 1]), tokens in [0, V)
 * The launch updates seen, finished, length, hist, hist_len, count and overflow IN PLACE. */
typedef struct vmlmf_history_controls {
  float repetition_penalty; /* theta > 0, finite; 1: the identity to the bit                         */
  int32_t eos;              /* the end-of-sentence token in [0, V), or -1: no row ever finishes      */
  int32_t min_length;       /* >= 0; > 0 needs eos: eos cannot be chosen while length < min_length   */
  int32_t pad;
  const float *logit_bias;  /* (V) fp32 shared by the rows, entries finite or -inf (a ban); or NULL  */
  uint8_t *seen;
  int32_t *finished;
  int32_t *length;
  int32_t no_repeat_ngram_size; /* n >= 0; 0: off                                                    */
  float frequency_penalty;      /* alpha >= 0, finite; 0: off                                        */
  float presence_penalty;       /* beta >= 0, finite; 0: off                                         */
  int32_t pad1;
  int32_t *hist;                /* required with a ban on (n >= 1 or n_sequences >= 1); else may be NULL: no history is kept */
  int32_t *hist_len;            /* as hist                                                           */
  int32_t hist_capacity;        /* >= 1                                                              */
  int32_t pad2;
  uint16_t *count;              /* required with a penalty on; else may be NULL: nothing is counted  */
  int32_t *overflow;            /* as hist                                                           */
  const int32_t *seq_tokens;
  const int32_t *seq_offsets;   /* (n_sequences + 1) int32, non-decreasing from 0                    */
  int32_t n_sequences;          /* >= 0                                                              */
  int32_t pad3;
} vmlmf_history_controls;

/* One decode step's choice for all B rows behind the head's GEMM, ONE launch, a workgroup per row.  The arguments are
 * vmlmf_decode_choose's (vmlmf_decode.h), the controls aside.  Let x[v] = bias[v] + scores[b][v] in fp32.
 * A FINISHED row (eos >= 0 and finished[b] != 0):  token = eos, logprob = 0.0 exactly, kept = 0, x_next = embed[eos];  nothing of the
 * row's state moves.
 * A LIVE row, in this order:
 *   1. repetition   r = seen[b][v] ? (x > 0 ? x / theta : x * theta) : x
 *   2. frequency / presence   q = (r - alpha * float(count[b][v])) - (count[b][v] > 0 ? beta : 0)
 *                   one rounded product and two rounded subtractions, never contracted; alpha = beta = 0: q == r to the bit
 *   3. bias         c = q + logit_bias[v]                                            (NULL: c = q + 0)
 *   4. min length   if eos >= 0 and length[b] < min_length:  c[eos] = -inf
 *   5. history bans c[v] = -inf for every v of the row's ban set.  With L = hist_len[b], h = hist[b]:
 *        n-grams (n = no_repeat_ngram_size >= 1): for every i in [0, L - n] with h[i .. i + n - 1) == h[L - n + 1 .. L), ban
 *          h[i + n - 1].  No ban while L + 1 < n; n = 1 bans every token of the history; overlapping matches count.  (The rule of
 *          Hugging Face's NoRepeatNGramLogitsProcessor.)
 *        sequences: a sequence s of m tokens: m = 1: s[0] is always banned; m > 1: s[m - 1] is banned when L >= m - 1 and
 *          h[L - m + 1 .. L) == s[0 .. m - 1).
 *   6. choice on c, exactly as vmlmf_decode_choose chooses on its c: the noise, the filters, the total order and the tie rule are the
 *      same, logprob = x[token] - logsumexp_v x[v] (raw, untempered), kept never counts a token at -inf; if nothing is open the token
 *      is 0.
 *   7. state, plain stores from one thread behind a workgroup barrier that every read of the row's state precedes:
 *      seen[b][token] = 1;  length[b] += 1;  if token == eos: finished[b] = 1;  count[b][token] += 1, saturating at 65535;
 *      if L < hist_capacity: hist[b][L] = token, hist_len[b] = L + 1;  else overflow[b] = 1 and hist, hist_len stay as they are - a
 *      full history is never written past.
 * NEUTRAL history controls (n = 0, n_sequences = 0, alpha = beta = 0): tokens, logprob, x_next, kept, seen, finished and length are
 * vmlmf_decode_choose's to the bit, whatever count holds.
 * The workgroup has 1024 threads when a filter is on and 256 when none is, as vmlmf_decode_choose's.  With a ban on, the row's ban set
 * is formed first, as a bitmap in LDS: threads stride over the match positions i and over the sequences, a match sets its bit with an
 * LDS atomic OR (the result does not depend on the order of arrival), one barrier follows; the selection then reads the bit beside
 * logit_bias, seen and count.  No pass over the scores and no launch is added.  Bit-identical from run to run.
 * Refused (VMLMF_E_BADARG, nothing launched): whatever vmlmf_decode_choose refuses; n < 0; alpha or beta negative or not finite; a
 * null hist, hist_len or overflow with a ban on; a null count with a penalty on; hist_capacity < 1; n_sequences < 0, or > 0 with a null
 * seq_tokens or seq_offsets; a ban on with V > VMLMF_HISTORY_MAX_V. */
int vmlmf_history_choose(int B, int H, int V, const float *scores, const float *bias, const float *embed, float inv_temperature,
                         int top_k, float top_p, const int64_t *state, int step, const vmlmf_history_controls *c, int64_t *tokens,
                         float *logprob, float *x_next, int32_t *kept, void *stream);

/* Step 5 alone, ONE launch, a workgroup per row: bitmap (B, ceil(V / 32)) uint32, row-major - bit (v & 31) of word v >> 5 is set when
 * v is in row b's ban set.  A finished row (eos >= 0, finished non-null and finished[b] != 0) gets zeros.  Nothing is chosen and no
 * state moves.  Of the controls it reads n, the sequences, hist, hist_len, hist_capacity, eos and finished.
 * Refused (VMLMF_E_BADARG): B, V < 1; a null controls, bitmap, hist or hist_len; n < 0; hist_capacity < 1; n_sequences < 0, or > 0
 * with a null array; eos outside [-1, V); V > VMLMF_HISTORY_MAX_V. */
int vmlmf_history_bans(int B, int V, const vmlmf_history_controls *c, uint32_t *bitmap, void *stream);

#ifdef __cplusplus
}
#endif
#endif
