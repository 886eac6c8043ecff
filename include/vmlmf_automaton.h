/* C ABI of libvmlmf_automaton.so: decoding under a TOKEN AUTOMATON (Model.generate and Model.beam_search with automaton=,
 * vmlmf_amd/lm.py) for the AMD Instinct MI355X (gfx950).  A library of its own beside libvmlmf_hip.so (include/vmlmf_hip.h),
 * libvmlmf_decode.so (include/vmlmf_decode.h, whose choice it extends) and libvmlmf_beam.so (include/vmlmf_beam.h, whose step it
 * extends), loaded on the first constrained call only: a generate() or beam_search() without automaton= never opens it.
 *
 * Conventions are vmlmf_hip.h's: every pointer is a device pointer unless it says "host", every launch goes to `stream` (a hipStream_t
 * passed as void*), nothing synchronises.  Return value: 0 = ok, <0 = VMLMF_E_* (the values of vmlmf_hip.h), >0 = hipError_t; the
 * text of the last failure of THIS library is vmlmf_automaton_last_error() (thread-local).
 */
#ifndef VMLMF_AUTOMATON_H
#define VMLMF_AUTOMATON_H

#include <stddef.h>
#include <stdint.h>

#include "vmlmf_decode.h" /* vmlmf_decode_controls, VMLMF_E_* */

#ifdef __cplusplus
extern "C" {
#endif

#define VMLMF_AUTOMATON_ABI_VERSION 1

int vmlmf_automaton_abi_version(void);
const char *vmlmf_automaton_last_error(void);

/* A finite automaton over tokens: a dense table next (S, V) int32, row-major, on the device.  A HOST struct.
 *   next[s][v] >= 0   in state s token v is OPEN and leads to that state (the caller keeps it below S)
 *   next[s][v] <  0   s does not offer v
 * eos is a token like any other: a state is accepting iff it offers eos.  A state outside [0, S) offers nothing - no address is ever
 * formed from it.  Every row of a decode (every beam of a search) carries one state. */
typedef struct vmlmf_token_automaton {
  const int32_t *next;
  int32_t S; /* >= 1, S V < 2^31 */
  int32_t pad;
} vmlmf_token_automaton;

/* The controls of one constrained decode and its per-row state: vmlmf_decode_controls, then the table and
 *   row_state (B)   int32: each row's state; moved on IN PLACE by the launch
 *   dead (B)        int32: set to 1 by a launch in which the row had nothing to choose; never cleared by a launch */
typedef struct vmlmf_automaton_controls {
  vmlmf_decode_controls decode;
  vmlmf_token_automaton table;
  int32_t *row_state;
  int32_t *dead;
} vmlmf_automaton_controls;

/* One decode step's choice for all B rows behind the head's GEMM under the automaton, ONE launch, a workgroup per row.  Every argument
 * but `c` is vmlmf_decode_choose's (vmlmf_decode.h), and the contract is that entry point's steps 1 - 6 word for word, with two additions:
 *   3a. (behind step 3) with s = row_state[b]: if s is outside [0, S) or next[s][v] < 0, c[v] = -inf.  The -inf REPLACES the value
 *       formed by the bias add: an open token's c is exactly vmlmf_decode_choose's, and the row's results are those of
 *       vmlmf_decode_choose under a logit_bias that also holds -inf at the tokens s closes, to the bit.
 *   6.  also writes row_state[b] = next[s][token] - by the same thread, behind the same workgroup barrier.
 * Nothing to choose (no token has c > -inf): tokens, logprob, kept, x_next and the row's seen / length / finished are whatever
 *   vmlmf_decode_choose writes for a row whose every c is -inf (token 0, a NaN log-probability, kept 0); row_state[b] is left
 *   unchanged and dead[b] = 1.
 * A FINISHED row writes its padding and touches neither row_state nor dead.
 * Unchanged from the plain call: logprob is the RAW row's log-softmax; kept never counts a closed token; the noise is the plain
 * call's; the workgroup has 1024 threads when a filter is on and 256 when none is; rows longer than 12288 tokens re-read their
 * scores and re-apply the controls, step 3a among them, in every pass.  The table costs a pass one more 4-byte coalesced load per
 * token, beside logit_bias[v] and seen[b][v] in the same eight-deep batch; no pass over the scores and no launch is added.
 * Refused (VMLMF_E_BADARG, nothing launched): whatever vmlmf_decode_choose refuses; a null c, next, row_state or dead; S < 1;
 * S V >= 2^31. */
int vmlmf_automaton_choose(int B, int H, int V, const float *scores, const float *bias, const float *embed, float inv_temperature,
                           int top_k, float top_p, const int64_t *state, int step, const vmlmf_automaton_controls *c, int64_t *tokens,
                           float *logprob, float *x_next, int32_t *kept, void *stream);

/* Host only.  Bytes of the workspace vmlmf_automaton_beam_step needs (those of vmlmf_beam_step).  0 for sizes it would refuse. */
size_t vmlmf_automaton_workspace_bytes(int B, int W, int V);

/* One step of beam search over B batch rows of W beams under the automaton, ONE launch.  The contract is vmlmf_beamctl_step's
 * (vmlmf_beamctl.h; every argument it shares with vmlmf_beam_step is that entry point's); in place of the per-beam bans and the
 * histories it takes
 *   min_length               >= 0; > 0 needs eos
 *   closed                   ceil(V / 32) uint32 words shared by all beams (bit v & 31 of word v >> 5), or NULL
 *   table                    the automaton (host struct)
 *   beam_state (B W)         int32: the state of beam w of batch row b at b W + w
 *   beam_state_out (B W)     int32: the survivors' states, written by this launch; must not be beam_state
 * Closed candidates.  A live beam with state s does not offer v when `closed` holds v, when v == eos and length[b, w] < min_length,
 *   when s is outside [0, S), or when next[s][v] < 0.  A closed candidate is not offered AT ALL (in a row that stays in LDS it is a
 *   NaN in its total's place); every offered candidate's total is vmlmf_beam_step's to the bit.
 * Finished beams.  A finished beam offers (w, eos) alone at its total, whatever is closed.
 * States.  Survivor slot b W + r gets beam_state_out = beam_state[parent row] if the parent was finished, else
 *   next[beam_state[parent row]][token]; a slot without a candidate (NaN total, parent 0, token 0) gets -1.  Written by the W threads
 *   of the batch row's last workgroup that write the other outputs.
 * NEUTRAL (a one-state, all-open table, min_length 0, closed NULL): every output equals vmlmf_beam_step's to the bit.
 * The kernel is vmlmf_beam_step's (csrc/vmlmf_beam_core.h) under a third offer policy.
 * Refused (VMLMF_E_BADARG, nothing launched): whatever vmlmf_beam_step refuses; min_length < 0, or > 0 with eos == -1; a null table,
 * next, beam_state or beam_state_out; beam_state_out == beam_state; S < 1; S V >= 2^31.  VMLMF_E_WORKSPACE: workspace too small. */
int vmlmf_automaton_beam_step(int B, int W, int H, int V, const float *scores, const float *bias, const float *cum,
                              const int32_t *finished, const int32_t *length, int eos, const float *embed, int min_length,
                              const uint32_t *closed, const vmlmf_token_automaton *table, const int32_t *beam_state,
                              int32_t *beam_state_out, int32_t *parent, int64_t *token, float *total, int32_t *finished_out,
                              int32_t *length_out, float *x_next, int32_t *src_row, uint32_t *ticket, void *workspace,
                              size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
