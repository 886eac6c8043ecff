/* C ABI of libvmlmf_contrast.so: the step of CONTRASTIVE SEARCH of the LM decoder (Model.contrastive_search, vmlmf_amd/lm.py; Su et
 * al., "A Contrastive Framework for Neural Text Generation") for the AMD Instinct MI355X (gfx950).  A library of its own, loaded on the
 * first contrastive call only; one of the Makefile's SIDE.
 *
 * Conventions are vmlmf_beamgroup.h's: every pointer is a device pointer, every launch goes to `stream` (a hipStream_t passed as
 * void*), nothing synchronises.  Return value: 0 = ok, <0 = VMLMF_E_*, >0 = hipError_t; the text of the last failure of THIS library
 * is vmlmf_contrast_last_error() (thread-local).
 *
 * The history.  hist (B, Tcap, H) fp32 holds, per batch row b, hist_len[b] UNIT vectors: the top layer's output behind every token of
 * the row so far, each divided by its Euclidean norm (the zero vector stays zero; so does a vector whose sum of squares is not a
 * positive finite number).  The rule is written once, as a device function both entry points call: a row's sum of squares is taken by
 * one 64-lane wave - lane l sums the elements l, l + 64, ... in rising order by fused multiply-adds, then a butterfly over the lanes -,
 * inv = 1 / sqrt(sum), element e becomes x[e] * inv.  Rows at and beyond hist_len[b] are unspecified and never read.
 */
#ifndef VMLMF_CONTRAST_H
#define VMLMF_CONTRAST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VMLMF_CONTRAST_ABI_VERSION 1
#define VMLMF_CONTRAST_MAX_K 16
/* how many workgroups may share one row's history */
#define VMLMF_CONTRAST_MAX_PARTS 64
/* the k unit candidates of a row wait in LDS, each padded to a multiple of four floats: k * 4 * ceil(H / 4) <= this many floats
 * (56 KiB) - H <= 896 at k = 16, H <= 3584 at k = 4 */
#define VMLMF_CONTRAST_LDS_FLOATS 14336

#ifndef VMLMF_E_BADARG
#define VMLMF_E_BADARG (-1)
#define VMLMF_E_WORKSPACE (-4)
#endif

int vmlmf_contrast_abi_version(void);
const char *vmlmf_contrast_last_error(void);

/* Host only.  Bytes of the workspace vmlmf_contrast_choose needs: the partial maxima of VMLMF_CONTRAST_MAX_PARTS workgroups per row,
 * B * VMLMF_CONTRAST_MAX_PARTS * VMLMF_CONTRAST_MAX_K * 4.  0 for sizes vmlmf_contrast_choose would refuse. */
size_t vmlmf_contrast_workspace_bytes(int B, int k, int H, int Tcap);

/* Append the T rows h[t][b] (h is (T, B, H) fp32) to every row's history as unit vectors: hist[b][hist_len[b] + t] = unit(h[t][b]),
 * t = 0 .. T - 1, then hist_len[b] += T (two launches: the rows, then the lengths).  This is how a prompt enters.  A row that would
 * land at or beyond Tcap is not written and hist_len[b] stops at Tcap: the caller sizes Tcap so that this never happens.
 * Refused with VMLMF_E_BADARG, nothing launched: B, T, H, Tcap < 1, B Tcap >= 2^31, null pointers. */
int vmlmf_contrast_append(int B, int T, int H, const float *h, float *hist, int32_t *hist_len, int Tcap, void *stream);

/* One step of contrastive search over B rows of k candidates, ONE launch.
 * In:  cand_h (B k, H) fp32, the top layer's output behind candidate j of row b at row b k + j; cand_tok (B, k) int64 and cand_logp
 *      (B, k) fp32, the candidates' tokens and log-probabilities under the whole distribution; alpha in [0, 1]; eos a token or -1;
 *      hist / hist_len as above; finished (B) int32, length (B) int32.
 * Per live row b (finished[b] == 0, or eos < 0), with t = hist_len[b] clamped to [0, Tcap]:
 *   sim[b][j] = max over i < t of dot(unit(cand_h[b k + j]), hist[b][i])      0 for t = 0
 *   value_j   = fsub_rn(fmul_rn(1 - alpha, expf(cand_logp[b][j])), fmul_rn(alpha, sim[b][j]))      fp32, each operation rounded once
 *   j*        = the j of the largest value, equal values to the lower j; a NaN value loses to every number; all NaN: j* = 0
 *   token[b] = cand_tok[b][j*], logprob[b] = cand_logp[b][j*], chosen[b] = j*, h_next[b] = cand_h[b k + j*] (raw, not unit),
 *   src_row[b k + j] = b k + j* for every j; hist[b][t] = unit(cand_h[b k + j*]) and hist_len[b] = t + 1 where t < Tcap (a full
 *   history is never written past: the append is skipped); length[b] += 1; finished[b] = 1 where eos >= 0 and token[b] == eos.
 * A finished row (eos >= 0 and finished[b] != 0) reports token eos, logprob 0.0, chosen 0, sim 0.0, h_next = cand_h[b k],
 * src_row = b k; its hist, hist_len, finished and length stay untouched and its history is not read.
 * Every dot product is summed whole by one wave in an order that depends on H alone (lane l takes the 16-byte - H % 4 == 0 -, 8-byte
 * - H % 2 == 0 - or 4-byte pieces l, l + 64, ... of the row in rising order, fused multiply-adds, then a butterfly over the lanes);
 * the maximum is exact and a NaN dot product makes the maximum NaN whatever the order.  parts workgroups share a row's history
 * (0: chosen from B and Tcap; 1 .. VMLMF_CONTRAST_MAX_PARTS: forced); each leaves its maxima in the workspace and takes the row's
 * ticket with an agent-scope release, the last to arrive acquires, merges and chooses and puts the ticket back to zero (ticket: (B)
 * uint32, zero before the first launch).  Nobody waits for anybody; no floating-point atomics: every output is the same bits for
 * every `parts` and from run to run.  Nothing at or beyond hist_len[b] is read; of hist only the appended row is written.
 * Refused with VMLMF_E_BADARG, nothing launched: B, H, Tcap < 1; B k or B Tcap >= 2^31; k outside [1, VMLMF_CONTRAST_MAX_K];
 * k * 4 * ceil(H / 4) > VMLMF_CONTRAST_LDS_FLOATS; alpha outside [0, 1] or NaN; eos < -1; parts outside [0, VMLMF_CONTRAST_MAX_PARTS];
 * null pointers; B >= 2^25; hist not 16-byte aligned; workspace not 4-byte aligned.  VMLMF_E_WORKSPACE: workspace_bytes smaller
 * than vmlmf_contrast_workspace_bytes(B, k, H, Tcap). */
int vmlmf_contrast_choose(int B, int k, int H, int Tcap, const float *cand_h, const int64_t *cand_tok, const float *cand_logp,
                          float alpha, int eos, float *hist, int32_t *hist_len, int32_t *finished, int32_t *length, int64_t *token,
                          float *logprob, int32_t *chosen, float *sim, float *h_next, int32_t *src_row, uint32_t *ticket,
                          void *workspace, size_t workspace_bytes, int parts, void *stream);

#ifdef __cplusplus
}
#endif
#endif
