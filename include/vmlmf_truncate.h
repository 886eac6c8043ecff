/* C ABI of libvmlmf_truncate.so: the truncation samplers of the LM decoder (Model.generate with min_p / typical_p / epsilon_cutoff /
 * eta_cutoff, vmlmf_amd/lm.py) for the AMD Instinct MI355X (gfx950).  A library of its own beside libvmlmf_hip.so
 * (include/vmlmf_hip.h), loaded on the first truncated call only: every other generate() never opens it.
 *
 * Conventions are vmlmf_hip.h's: every pointer is a device pointer unless it says "host", every launch goes to `stream` (a hipStream_t
 * passed as void*), nothing synchronises.  Return value: 0 = ok, <0 = VMLMF_E_* (the values of vmlmf_hip.h), >0 = hipError_t; the
 * text of the last failure of THIS library is vmlmf_truncate_last_error() (thread-local).
 */
#ifndef VMLMF_TRUNCATE_H
#define VMLMF_TRUNCATE_H

#include <stddef.h>
#include <stdint.h>

#include "vmlmf_decode.h" /* vmlmf_decode_controls */
#include "vmlmf_hip.h"    /* VMLMF_E_* */

#ifdef __cplusplus
extern "C" {
#endif

#define VMLMF_TRUNCATE_ABI_VERSION 1

int vmlmf_truncate_abi_version(void);
const char *vmlmf_truncate_last_error(void);

/* The four samplers, a HOST struct.  min_p in [0, 1] (0: off), typical_p in (0, 1] (1: off), epsilon_cutoff and eta_cutoff in [0, 1)
 * (0: off). */
typedef struct vmlmf_truncation {
  float min_p, typical_p, epsilon_cutoff, eta_cutoff; /* 0, 1, 0, 0: off */
} vmlmf_truncation;

/* One decode step's truncated choice for all B rows behind the head's GEMM: ONE launch, a workgroup of 1024 threads per row.
 * scores, bias, embed, inv_temperature (> 0: this entry point samples), top_k, top_p, state, step, tokens, logprob, x_next, kept and
 * stream are vmlmf_lm_choose_filtered's (include/vmlmf_hip.h); controls (a host struct, or NULL: none) are vmlmf_decode_choose's
 * (include/vmlmf_decode.h), with their finished rows, their state update and their refusals.
 * Let x[v] = bias[v] + scores[b][v], c = x (controls NULL) or the controlled score of vmlmf_decode.h, z = c * inv_temperature + 0 in
 * fp32, z_max the row's largest z.  A token with z = -inf is never kept and never counted.
 *   ORDER   larger z first, equal z to the lower index.  mass_v = round(exp(z_v - z_max) 2^40), a 64-bit integer.
 *   STAGES  in this order, each on the survivors of the stages before it, each keeping at least its own first token:
 *     top_k, top_p      as vmlmf_lm_choose_filtered: the first k of the order; of those the shortest prefix whose mass reaches
 *                       ceil(top_p x their mass), a tie group at the boundary cut by index
 *     min_p = a         keep v iff fl(z_v - z_max) >= fl32(log a): log a is formed once on the host in fp64 and rounded to fp32, the
 *                       difference is one correctly rounded fp32 subtraction.  Every token of a tie group is in or out together.
 *     typical_p = m     over the survivors S = sum mass, cbar = fl32(sum mass (z_max - z) / S) - the entropy minus log S -,
 *                       d_v = |fl(fl(z_max - z_v) - cbar)|.  In the order "smaller d first, equal d to the lower index" keep the
 *                       token at position j iff the mass before it is < ceil(m S): Hugging Face's TypicalLogitsWarper with the
 *                       boundary's ties cut by index.  The band need not hold the most probable token.
 *     epsilon_cutoff    keep v iff mass_v >= ceil(epsilon S), S over the survivors; the survivors with the largest z stay anyway
 *     eta_cutoff        with H = log(S 2^-40) + sum mass (z_max - z) / S, the entropy of the survivors, in fp64: keep v iff
 *                       mass_v >= ceil(min(eta, sqrt(eta) exp(-H)) S); the survivors with the largest z stay anyway
 *   S is an exact integer sum.  sum mass (z_max - z) is an fp64 sum through a fixed tree (a thread's tokens in a fixed order, a
 *   64-lane butterfly, the 16 waves in order).  cbar, H and every threshold are rounded once per row.
 *   CHOICE  token = argmax over the kept set of z + G, G exactly the noise vmlmf_lm_choose draws for (step B + b, v); Philox runs
 *   only for the groups of four tokens that hold a kept one.  logprob = x[token] - logsumexp x, the untempered, unfiltered
 *   log-softmax, its (max, sum exp) formed by vmlmf_lm_choose's reduction tree: a truncation that keeps every token gives that entry
 *   point's logprob to the bit.  kept (B) int32 or NULL: the survivors.  x_next (B, H) or NULL: embed[token].
 * Rows longer than 12288 tokens re-read their scores (and re-apply the controls) in every pass.  Bit-identical from run to run.
 * Refused (nothing launched): what vmlmf_lm_choose_filtered refuses; a null `t`, or a field of it outside its range
 * (VMLMF_E_BADARG); inv_temperature == 0 (VMLMF_E_UNSUPPORTED: greedy decoding ignores truncation - run vmlmf_lm_choose or
 * vmlmf_decode_choose); with controls, what vmlmf_decode_choose refuses of them. */
int vmlmf_truncate_choose(int B, int H, int V, const float *scores, const float *bias, const float *embed, float inv_temperature,
                          int top_k, float top_p, const vmlmf_truncation *t, const int64_t *state, int step,
                          const vmlmf_decode_controls *controls, int64_t *tokens, float *logprob, float *x_next, int32_t *kept,
                          void *stream);

#ifdef __cplusplus
}
#endif
#endif
