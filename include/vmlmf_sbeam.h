/* C ABI of libvmlmf_sbeam.so: the step of STOCHASTIC beam search of the LM decoder (Model.stochastic_beam_search, vmlmf_amd/lm.py) for
 * the AMD Instinct MI355X (gfx950).  A library of its own beside libvmlmf_beam.so (include/vmlmf_beam.h), loaded on the first
 * stochastic-beam call only; one of the Makefile's SIDE.
 *
 * Conventions are vmlmf_hip.h's: every pointer is a device pointer, every launch goes to `stream` (a hipStream_t passed as void*),
 * nothing synchronises.  Return value: 0 = ok, <0 = VMLMF_E_*, >0 = hipError_t; the text of the last failure of THIS library is
 * vmlmf_sbeam_last_error() (thread-local).
 */
#ifndef VMLMF_SBEAM_H
#define VMLMF_SBEAM_H

#include <stddef.h>
#include <stdint.h>

#include "vmlmf_beam.h" /* VMLMF_BEAM_MAX_BEAMS, VMLMF_E_* */

#ifdef __cplusplus
extern "C" {
#endif

#define VMLMF_SBEAM_ABI_VERSION 1

int vmlmf_sbeam_abi_version(void);
const char *vmlmf_sbeam_last_error(void);

/* Host only.  Bytes of the workspace vmlmf_sbeam_step needs: the W first candidates of each of the B x W rows as a 64-bit key
 * (perturbed value, flat index) and an fp32 total - B W W (8 + 4).  0 for sizes vmlmf_sbeam_step would refuse. */
size_t vmlmf_sbeam_workspace_bytes(int B, int W, int V);

/* One step of stochastic beam search (Kool, van Hoof and Welling, "Stochastic Beams and Where to Find Them") over B batch rows of W
 * beams, ONE launch: beam search over Gumbel-perturbed totals whose perturbation is drawn top-down, so a child's perturbed value never
 * exceeds its parent's.  Every argument up to workspace_bytes is vmlmf_beam_step's (include/vmlmf_beam.h), and so are the outputs
 * parent, token, total, finished_out, length_out, x_next and src_row; behind them
 *   perturbed (B, W)      fp32 in: each beam's perturbed value T.  A search that starts has 0 for beam 0 and -inf for the others
 *   perturbed_out (B, W)  the survivors' perturbed values G, non-increasing along W
 *   draw (B)              int32 in: how many steps this search has taken
 *   draw_out (B)          draw + 1
 *   state                 the sampler's two int64 {seed, offset}, as vmlmf_lm_choose takes them
 * Candidates.  A live beam w of batch row b, T = perturbed[b, w], offers every v with
 *   phi = cum[w] + ((bias[v] + scores[w][v]) - lse)        vmlmf_beam_step's three operations and its fixed-tree lse: its bits
 *   gt  = phi + gumbel(key(state), position, v)            the sampler's noise (vmlmf_lm_choose: Philox4x32-10 at (position, v >> 2,
 *                                                          VMLMF_SITE_SAMPLE, offset)), position = draw[b] B W + b W + w in uint32
 *                                                          arithmetic - with W = 1 the sampler's noise of (step B + b, v)
 *   Z   = max_v gt                                         exact (NaN is skipped)
 *   G   = T                                                where gt == Z, exactly; otherwise, each operation rounded to fp32 in
 *                                                          this order,
 *         u = (T - gt) + log1pf(-expf(gt - Z))
 *         G = (T - fmaxf(u, 0)) - log1pf(expf(-fabsf(u)))
 *   G   = -inf where T, cum[w] or gt is -inf; a NaN score is no candidate.
 * A finished beam offers (w, eos) alone, at total cum[w] and G = T: a finished hypothesis keeps its value.
 * Order.  Larger G first, equal G to the lower flat index w V + v - within a beam and in the merge.  The selection runs on G itself
 * (the fp32 transform need not be monotone in gt to the bit).  The first W candidates of a batch row go to slots b W + r in that
 * order: parent, token, total = phi, perturbed_out = G, finished_out, length_out, src_row, x_next = embed[token], as vmlmf_beam_step
 * writes them.  perturbed_out[b][0] is max_w perturbed[b][w] to the bit, and no survivor's G exceeds its parent's T.
 * The outputs must not alias the inputs.  Exact and bit-identical from run to run; a workgroup per beam, a ticket per batch row, the
 * row's last workgroup merges W x W candidates in W rounds and puts the ticket back to zero; nobody waits for anybody.
 *   workspace        vmlmf_sbeam_workspace_bytes(B, W, V) bytes, 8-byte aligned
 * Refused (nothing launched): whatever vmlmf_beam_step refuses; VMLMF_E_BADARG for a null perturbed, perturbed_out, draw, draw_out or
 * state and for perturbed_out == perturbed, perturbed_out == cum, perturbed_out == total, total == perturbed or draw_out == draw.
 * If fewer than W candidates can be ordered (NaN scores) the remaining slots get parent 0, token 0 and NaN total and perturbed_out. */
int vmlmf_sbeam_step(int B, int W, int H, int V, const float *scores, const float *bias, const float *cum, const int32_t *finished,
                     const int32_t *length, int eos, const float *embed, int32_t *parent, int64_t *token, float *total,
                     int32_t *finished_out, int32_t *length_out, float *x_next, int32_t *src_row, uint32_t *ticket, void *workspace,
                     size_t workspace_bytes, const float *perturbed, float *perturbed_out, const int32_t *draw, int32_t *draw_out,
                     const void *state, void *stream);

#ifdef __cplusplus
}
#endif
#endif
