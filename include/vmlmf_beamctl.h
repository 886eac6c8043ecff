/* C ABI of libvmlmf_beamctl.so: the beam-search step of the LM decoder UNDER CONTROLS (Model.beam_search with min_length, banned_tokens,
 * no_repeat_ngram_size or banned_sequences, vmlmf_amd/lm.py) for the AMD Instinct MI355X (gfx950).  A library of its own beside
 * libvmlmf_hip.so (include/vmlmf_hip.h) and libvmlmf_beam.so (include/vmlmf_beam.h, whose step it extends), loaded on the first
 * controlled beam call only: a beam_search() without these arguments never opens it.
 *
 * Conventions are vmlmf_hip.h's: every pointer is a device pointer unless it says "host", every launch goes to `stream` (a hipStream_t
 * passed as void*), nothing synchronises.  Return value: 0 = ok, <0 = VMLMF_E_* (the values of vmlmf_hip.h), >0 = hipError_t; the
 * text of the last failure of THIS library is vmlmf_beamctl_last_error() (thread-local).
 */
#ifndef VMLMF_BEAMCTL_H
#define VMLMF_BEAMCTL_H

#include <stddef.h>
#include <stdint.h>

#include "vmlmf_beam.h"    /* VMLMF_BEAM_MAX_BEAMS, the plain step's contract */
#include "vmlmf_history.h" /* VMLMF_HISTORY_MAX_V, the layout of a ban set    */

#ifdef __cplusplus
extern "C" {
#endif

#define VMLMF_BEAMCTL_ABI_VERSION 1

int vmlmf_beamctl_abi_version(void);
const char *vmlmf_beamctl_last_error(void);

/* The controls of one step.  A HOST struct of scalars and device pointers, copied into the launch's arguments.  The controls only
 * CLOSE candidates - a candidate is offered or it is not -, they never change a total.
 *   min_length               >= 0; > 0 needs eos: a live beam with length[b, w] < min_length does not offer eos
 *   closed                   ceil(V / 32) uint32 words shared by all beams, bit (v & 31) of word v >> 5 set: no live beam offers v; or NULL
 *   bans                     (B W, ceil(V / 32)) uint32: row b W + w is beam w's own ban set, exactly as vmlmf_history_bans
 *                            (vmlmf_history.h) writes it when called on B W rows; or NULL
 *   hist (B W, hist_capacity), hist_len (B W)   int32: each beam's tokens so far, PROMPT INCLUDED, oldest first; or both NULL: no
 *                            history is kept, and hist_out, hist_len_out and overflow are NULL too
 *   hist_out (B W, hist_capacity), hist_len_out (B W)   int32: the survivors' histories, written by this launch; hist_out must not be hist
 *   overflow (B)             int32: set to 1, and never cleared, by a launch in which a live parent's history was full */
typedef struct vmlmf_beamctl_controls {
  int32_t min_length;
  int32_t hist_capacity; /* >= 1 */
  const uint32_t *closed;
  const uint32_t *bans;
  const int32_t *hist;
  const int32_t *hist_len;
  int32_t *hist_out;
  int32_t *hist_len_out;
  int32_t *overflow;
} vmlmf_beamctl_controls;

/* Host only.  Bytes of the workspace vmlmf_beamctl_step needs (those of vmlmf_beam_step: the W best candidates of each of the B x W
 * rows).  0 for sizes vmlmf_beamctl_step would refuse. */
size_t vmlmf_beamctl_workspace_bytes(int B, int W, int V);

/* One step of beam search over B batch rows of W beams under controls, ONE launch.  Every argument in front of `c` is
 * vmlmf_beam_step's (vmlmf_beam.h), and so is the contract, word for word: the candidates' totals cum[w] + ((bias[v] + scores[w][v])
 * - lse) with lse over the RAW row, formed by the same operations in the same fixed tree; the order (larger total first, equal totals
 * to the lower flat index w V + v); the outputs, written in that order to slot b W + r; the ticket and the workspace.  Beside it:
 * Closed candidates.  A live beam w does not offer v when v's bit is set in `closed` or in bans[b W + w], or when v == eos and
 *   length[b, w] < min_length.  A closed candidate is not offered AT ALL - it is not a candidate at -inf: a beam that does not exist
 *   yet (cum = -inf) already offers real candidates at -inf, and they come before nothing.
 * Finished beams.  A finished beam offers (w, eos) alone at its total, whatever is closed.
 * Too few candidates.  A beam with fewer than W open tokens offers those it has.  If a batch row has fewer than W candidates in all,
 *   the remaining slots get parent 0, token 0 and a NaN total (as vmlmf_beam_step's slots that cannot be ordered).
 * History (with hist).  Slot b W + r gets hist[b W + parent][0 .. L), L = hist_len[b W + parent] (clamped to [0, hist_capacity]),
 *   followed by its token, and hist_len_out = L + 1.  If the parent was finished the history and its length are copied unchanged.  If
 *   L == hist_capacity for a live parent, the history is copied, nothing is written past its end, hist_len_out = L and overflow[b] is
 *   set to 1.  (A slot without a candidate - NaN total - is treated as its parent 0 and token 0 say.)  What lies behind hist_len_out
 *   in a row of hist_out is not written.
 * NEUTRAL controls (min_length 0, closed, bans and hist NULL): every output equals vmlmf_beam_step's to the bit.
 * The kernel is vmlmf_beam_step's (csrc/vmlmf_beam_core.h: a workgroup per beam, a ticket per batch row, 64-bit keys, nobody waits for
 * anybody, no float atomics, bit-identical from run to run).  A closed candidate of a row that stays in LDS is a NaN in place of its
 * total, which the selection rounds skip as they skip NaN scores; the last workgroup of a batch row, which writes the outputs, also
 * copies the W histories.
 * Refused (VMLMF_E_BADARG, nothing launched): whatever vmlmf_beam_step refuses; a null c; min_length < 0, or > 0 with eos == -1; hist
 * without hist_len, hist_out, hist_len_out and overflow, or any of those without hist; hist_out == hist; hist_capacity < 1; bans with
 * V > VMLMF_HISTORY_MAX_V.  VMLMF_E_WORKSPACE: workspace too small. */
int vmlmf_beamctl_step(int B, int W, int H, int V, const float *scores, const float *bias, const float *cum, const int32_t *finished,
                       const int32_t *length, int eos, const float *embed, const vmlmf_beamctl_controls *c, int32_t *parent,
                       int64_t *token, float *total, int32_t *finished_out, int32_t *length_out, float *x_next, int32_t *src_row,
                       uint32_t *ticket, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
