/* C ABI of libvmlmf_decode.so: the controlled choice of the LM decoder (Model.generate with eos / min_length / repetition_penalty /
 * logit_bias / banned_tokens, vmlmf_amd/lm.py) for the AMD Instinct MI355X (gfx950).  A library of its own beside libvmlmf_hip.so
 * (include/vmlmf_hip.h), loaded on the first controlled call only: a plain generate() never opens it.
 *
 * Conventions are vmlmf_hip.h's: every pointer is a device pointer unless it says "host", every launch goes to `stream` (a hipStream_t
 * passed as void*), nothing synchronises.  Return value: 0 = ok, <0 = VMLMF_E_* (the values of vmlmf_hip.h), >0 = hipError_t; the
 * text of the last failure of THIS library is vmlmf_decode_last_error() (thread-local).
 */
#ifndef VMLMF_DECODE_H
#define VMLMF_DECODE_H

#include <stddef.h>
#include <stdint.h>

#include "vmlmf_hip.h" /* VMLMF_E_* */

#ifdef __cplusplus
extern "C" {
#endif

#define VMLMF_DECODE_ABI_VERSION 1

int vmlmf_decode_abi_version(void);
const char *vmlmf_decode_last_error(void);

/* The controls of one decode and its per-row state.  A HOST struct of scalars and device pointers, copied into the launch's arguments.
 *   seen (B, V)      uint8, ONE BYTE per (row, token), row-major: non-zero = the row has held the token (prompt included)
 *   finished (B)     int32, non-zero: the row has emitted eos (looked at only when eos >= 0)
 *   length (B)       int32, tokens the row has emitted, eos included
 * The launch updates all three IN PLACE. */
typedef struct vmlmf_decode_controls {
  float repetition_penalty; /* theta > 0, finite; 1: the identity to the bit                         */
  int32_t eos;              /* the end-of-sentence token in [0, V), or -1: no row ever finishes      */
  int32_t min_length;       /* >= 0; > 0 needs eos: eos cannot be chosen while length < min_length   */
  int32_t pad;
  const float *logit_bias;  /* (V) fp32 shared by the rows, entries finite or -inf (a ban); or NULL  */
  uint8_t *seen;
  int32_t *finished;
  int32_t *length;
} vmlmf_decode_controls;

/* One decode step's choice for all B rows behind the head's GEMM, ONE launch, a workgroup per row.
 *   scores (B, V)    h fc.w^T WITHOUT the bias (a library GEMM);  bias (V) fc.b or NULL;  embed (V, H) or NULL together with x_next
 *   inv_temperature  1 / tau, or 0: greedy;  top_k in [0, ..) (0 and >= V: off);  top_p in (0, 1] (1: off)
 *   state            the {seed, offset} snapshot of the sampler's generator (two uint64; NULL when greedy);  step: the decode step j
 * Let x[v] = bias[v] + scores[b][v] in fp32.
 * A FINISHED row (eos >= 0 and finished[b] != 0):  token = eos, logprob = 0.0 exactly, kept = 0, x_next = embed[eos];  seen, length
 * and finished are left as they are.
 * A LIVE row, in this order:
 *   1. repetition   r = seen[b][v] ? (x > 0 ? x / theta : x * theta) : x            (IEEE division; theta = 1: r == x to the bit)
 *   2. bias         c = r + logit_bias[v]                                            (NULL: c = r + 0)
 *   3. min length   if eos >= 0 and length[b] < min_length:  c[eos] = -inf
 *   4. choice on c, exactly as vmlmf_lm_choose / vmlmf_lm_choose_filtered choose on x (include/vmlmf_hip.h): greedy = argmax c, ties
 *      to the lower index; sampling: z = c * inv_temperature, top-k, then top-p under the one total order (larger z first, equal z to
 *      the lower index), token = argmax over the kept set of z + G, G the very noise those entry points draw for (step B + b, v).  A
 *      token at c = -inf is never chosen and is not counted in kept.  With theta = 1, logit_bias NULL or zero, eos = -1 and seen all
 *      zero the results are those entry points' results to the bit.
 *   5. logprob = x[token] - logsumexp_v x[v]: the unprocessed, untempered log-softmax (what nll_loss charges)
 *   6. state        seen[b][token] = 1;  length[b] += 1;  if token == eos: finished[b] = 1  - plain stores from one thread of the
 *      row's workgroup, behind a workgroup barrier that every read of the row's state precedes.
 *   kept (B) int32 or NULL: how many tokens the choice ran over (filters on: the kept set; off or greedy: the tokens with c > -inf).
 * The workgroup has 1024 threads when a filter is on (sampling with top_k or top_p: the selection of vmlmf_lm_choose_filtered, on c)
 * and 256 when none is (greedy, unfiltered sampling: the single pass and the reduction tree of vmlmf_lm_choose, on c) - the sizes at
 * which those kernels form (max, sum exp), so that the log-probabilities agree to the bit.  Rows longer than 12288 tokens re-read
 * their scores and re-apply the controls in every pass of the selection.  Bit-identical from run to run.
 * Refused (VMLMF_E_BADARG, nothing launched): B, V < 1 (H < 1 with x_next); a null scores, tokens, controls, seen, finished or
 * length; eos outside [-1, V); repetition_penalty <= 0 or not finite; min_length < 0, or > 0 without eos; x_next without embed; and
 * whatever vmlmf_lm_choose_filtered refuses of inv_temperature, top_k, top_p, state and step. */
int vmlmf_decode_choose(int B, int H, int V, const float *scores, const float *bias, const float *embed, float inv_temperature,
                        int top_k, float top_p, const int64_t *state, int step, const vmlmf_decode_controls *c, int64_t *tokens,
                        float *logprob, float *x_next, int32_t *kept, void *stream);

#ifdef __cplusplus
}
#endif
#endif
