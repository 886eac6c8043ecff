/* C ABI of libvmlmf_beamgroup.so: the step of DIVERSE (group) beam search of the LM decoder (Model.group_beam_search, vmlmf_amd/lm.py)
 * for the AMD Instinct MI355X (gfx950).  A library of its own beside libvmlmf_beam.so (include/vmlmf_beam.h), loaded on the first
 * group-beam call only; one of the Makefile's SIDE.
 *
 * Conventions are vmlmf_hip.h's: every pointer is a device pointer, every launch goes to `stream` (a hipStream_t passed as void*),
 * nothing synchronises.  Return value: 0 = ok, <0 = VMLMF_E_*, >0 = hipError_t; the text of the last failure of THIS library is
 * vmlmf_beamgroup_last_error() (thread-local).
 */
#ifndef VMLMF_BEAMGROUP_H
#define VMLMF_BEAMGROUP_H

#include <stddef.h>
#include <stdint.h>

#include "vmlmf_beam.h" /* VMLMF_BEAM_MAX_BEAMS, VMLMF_E_* */

#ifdef __cplusplus
extern "C" {
#endif

#define VMLMF_BEAMGROUP_ABI_VERSION 1

int vmlmf_beamgroup_abi_version(void);
const char *vmlmf_beamgroup_last_error(void);

/* Host only.  Bytes of the workspace vmlmf_beamgroup_step needs (vmlmf_beam_step's: the W best candidates of each of the B x W rows).
 * 0 for sizes vmlmf_beamgroup_step would refuse. */
size_t vmlmf_beamgroup_workspace_bytes(int B, int W, int V);

/* One step of diverse beam search (Vijayakumar et al., "Diverse Beam Search") over B batch rows of W beams in G = groups groups, ONE
 * launch.  Every argument up to workspace_bytes is vmlmf_beam_step's (include/vmlmf_beam.h), and so is every output; only which
 * candidates survive differs.
 * Groups.  G divides W, Wg = W / G.  Group g owns slots g Wg .. g Wg + Wg - 1 of a batch row, as beams on the way in and as survivors
 * on the way out: groups never exchange beams.
 * Candidates.  vmlmf_beam_step's, formed by the same operations in the same fixed tree: a live beam w offers every v with
 * total = cum[w] + (x[v] - lse); a finished beam offers (w, eos) alone, at cum[w].
 * Order.  The groups are processed in order g = 0 .. G - 1.  A live beam's candidate (w, v) of group g is ranked by
 *   aug = total - lambda n        lambda = diversity_penalty; n = how many survivors the groups 0 .. g - 1 of this batch row chose IN
 *                                 THIS STEP with token v and a live parent (a finished beam's padding eos is no choice: not counted)
 * formed in fp32 as two separately rounded operations, aug = fsub_rn(total, fmul_rn(lambda, (float)n)) - no fused multiply-add, so a
 * host reproduces it bit for bit; for n = 0 it is `total`.  A finished beam's candidate is not penalised.  Within a group: larger aug
 * first, equal aug to the lower flat index w V + v (w the beam's index in the whole row, 0 .. W - 1).  The first Wg candidates of group
 * g go to slots g Wg + r, r = 0 .. Wg - 1, in that order.
 * Outputs.  total is the RAW total - the penalty steers the step's choice and is never accumulated (the paper's objective), so totals
 * stay sums of plain log-probabilities -; parent is the beam's index in the whole row, 0 .. W - 1; token, finished_out, length_out,
 * x_next and src_row = b W + parent are vmlmf_beam_step's.
 * groups = 1 is vmlmf_beam_step bit for bit; diversity_penalty = 0 is vmlmf_beam_step called on B G rows of Wg beams (parent + g Wg).
 * Exact and bit-identical from run to run; one launch; nobody waits for anybody; the ticket protocol is vmlmf_beam_step's.
 * Refused (nothing launched): whatever vmlmf_beam_step refuses, and VMLMF_E_BADARG for groups < 1, W % groups != 0 and a
 * diversity_penalty that is negative or not finite. */
int vmlmf_beamgroup_step(int B, int W, int H, int V, const float *scores, const float *bias, const float *cum, const int32_t *finished,
                         const int32_t *length, int eos, const float *embed, int32_t *parent, int64_t *token, float *total,
                         int32_t *finished_out, int32_t *length_out, float *x_next, int32_t *src_row, uint32_t *ticket, void *workspace,
                         size_t workspace_bytes, int groups, float diversity_penalty, void *stream);

#ifdef __cplusplus
}
#endif
#endif
