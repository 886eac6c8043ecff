/* C ABI of libvmlmf_score.so: scoring given text with the LM's head (Model.score, vmlmf_amd.lm_score; vmlmf_amd/scoring.py) for
 * the AMD Instinct MI355X (gfx950) - the log-probability and the rank of a target token per row of scores, and the row's most probable
 * tokens.  A library of its own beside libvmlmf_hip.so (include/vmlmf_hip.h), loaded on the first scoring call only: a training or a
 * generating process never opens it.
 *
 * Conventions are vmlmf_hip.h's: every pointer is a device pointer, every launch goes to `stream` (a hipStream_t passed as void*),
 * nothing synchronises.  Return value: 0 = ok, <0 = VMLMF_E_* (the values of vmlmf_hip.h), >0 = hipError_t; the text of the last
 * failure of THIS library is vmlmf_score_last_error() (thread-local).
 */
#ifndef VMLMF_SCORE_H
#define VMLMF_SCORE_H

#include <stddef.h>
#include <stdint.h>

#include "vmlmf_hip.h" /* VMLMF_E_* */

#ifdef __cplusplus
extern "C" {
#endif

#define VMLMF_SCORE_ABI_VERSION 1
#define VMLMF_SCORE_MAX_TOP 32 /* as VMLMF_BEAM_MAX_BEAMS */

int vmlmf_score_abi_version(void);
const char *vmlmf_score_last_error(void);

/* R rows of V scores behind the head's GEMM, ONE launch, a workgroup of 256 threads per row.
 *   scores (R, V)    h fc.w^T WITHOUT the bias (a library GEMM);  bias (V) fc.b or NULL
 *   targets (R)      int64, the token each row is asked about; < 0: the row has no target.  NULL: no row has one
 *   top              in [0, min(32, V)]: how many of the row's most probable tokens to report
 * Let x[v] = bias[v] + scores[r][v] in fp32 (bias NULL: 0 + scores[r][v]), and (m, s) = (max, sum exp(x - max)) of the row, formed
 * exactly as vmlmf_lm_choose forms them (include/vmlmf_hip.h: 256 threads, four neighbouring tokens per thread per trip, the 64-lane
 * butterfly, then the four waves in order - the kernels share the code).  The ORDER of a row's tokens is the project's one total
 * order: larger x first, equal x (-0 and +0 are equal) to the lower index.
 *   logprob (R)            x[y] - (m + logf(s)), y = targets[r]: for the greedy token what vmlmf_lm_choose reports, to the bit
 *   rank (R) int32 / NULL  the number of tokens ahead of y in the order; 0: greedy decoding would have chosen y
 *   top_tokens (R, top)    int64: the first `top` tokens of the order, in order
 *   top_logprob (R, top)   x[token] - (m + logf(s)), the same (m, s)
 * A row WITHOUT a target: logprob = 0.0 exactly, rank = -1; its top outputs are those of any row.  With targets NULL logprob and rank
 * may be NULL.  A target >= V is the caller's error: nothing outside the row is read for it, logprob = NaN and rank = -1.
 * A row that holds a NaN: logprob and every top_logprob are NaN; rank and top_tokens follow the order of the scores' bit patterns
 * (a NaN with the sign bit clear ahead of +inf, one with it set behind -inf), so every index written lies in [0, V).
 * The row is read from memory once where it fits LDS (V <= 12288): that pass forms (m, s), counts the rank and leaves the row's
 * keys in LDS, where the selection of the top tokens runs (a radix select over counts, the tie group cut at the lower indices, then
 * the <= 32 survivors ordered).  A longer row is read again by each of the selection's six passes; with top = 0 every row is read
 * exactly once.  No atomics on floats, no atomics on global memory: bit-identical from run to run.
 * Refused (VMLMF_E_BADARG, nothing launched): R, V < 1; a null scores; top outside [0, min(32, V)]; top > 0 with a null top_tokens or
 * top_logprob; targets without logprob. */
int vmlmf_score_rows(int R, int V, const float *scores, const float *bias, const int64_t *targets, int top, float *logprob,
                     int32_t *rank, int64_t *top_tokens, float *top_logprob, void *stream);

#ifdef __cplusplus
}
#endif
#endif
