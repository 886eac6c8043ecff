/* C ABI of libvmlmf_beam.so: the beam-search step of the LM decoder (Model.beam_search, vmlmf_amd/lm.py) for the AMD Instinct
 * MI355X (gfx950).  A library of its own beside libvmlmf_hip.so (include/vmlmf_hip.h), loaded on the first beam call only.
 *
 * Conventions are vmlmf_hip.h's: every pointer is a device pointer unless it says "host", every launch goes to `stream` (a hipStream_t
 * passed as void*), nothing synchronises.  Return value: 0 = ok, <0 = VMLMF_E_* (the values of vmlmf_hip.h), >0 = hipError_t; the
 * text of the last failure of THIS library is vmlmf_beam_last_error() (thread-local).
 */
#ifndef VMLMF_BEAM_H
#define VMLMF_BEAM_H

#include <stddef.h>
#include <stdint.h>

#include "vmlmf_hip.h" /* VMLMF_E_* */

#ifdef __cplusplus
extern "C" {
#endif

#define VMLMF_BEAM_ABI_VERSION 1
#define VMLMF_BEAM_MAX_BEAMS 32   /* W: the merge holds the W x W candidates of a batch row one per thread of a workgroup */
#define VMLMF_BEAM_MAX_TENSORS 16 /* state tensors one vmlmf_beam_gather launch reorders (2 per layer)                    */

int vmlmf_beam_abi_version(void);
const char *vmlmf_beam_last_error(void);

/* Host only.  Bytes of the workspace vmlmf_beam_step needs: the W best candidates (total, flat index) of each of the B x W rows.
 * 0 for arguments vmlmf_beam_step would refuse. */
size_t vmlmf_beam_workspace_bytes(int B, int W, int V);

/* One step of beam search over B batch rows of W beams, ONE launch.
 *   scores (B W, V)  h fc.w^T of the beams' top-layer outputs, WITHOUT the bias (a library GEMM); row b W + w is beam w of batch row b
 *   bias (V)         fc.b, or NULL
 *   cum (B, W)       the beams' totals so far (fp32; -inf: a beam that does not exist yet)
 *   finished (B, W)  int32, non-zero: the beam has emitted eos (looked at only when eos >= 0)
 *   length (B, W)    int32, tokens emitted up to and including eos
 *   eos              the end-of-sentence token in [0, V), or -1: no beam ever finishes
 *   embed (V, H)     the embedding table, or NULL together with x_next
 * Candidates.  A live beam w offers (w, v) for every v with total cum[w] + (x[v] - lse), x[v] = bias[v] + scores[w][v] and
 * lse = log sum_v exp x[v], all fp32 in a fixed order.  A finished beam offers (w, eos) alone, with total cum[w].
 * Order.  Larger total first, equal totals to the lower flat index w V + v.  The step keeps the first W candidates of a batch row
 * and writes them IN THAT ORDER to slot b W + r, r = 0 .. W - 1:
 *   parent int32 (the beam w it extends), token int64, total fp32, finished_out int32 (parent finished, or token == eos),
 *   length_out int32 (the parent's, + 1 unless the parent was finished), x_next (B W, H) = embed[token], src_row int32 = b W + parent.
 * The outputs must not alias the inputs.  Exact and bit-identical from run to run: no float atomics, nothing depends on the order in
 * which workgroups arrive.  A workgroup per beam forms that beam's own first W candidates (a survivor of the row is always among
 * them), leaves them in the workspace and takes the row's ticket; the last of a row's W workgroups to arrive merges the W x W
 * candidates, writes the outputs and puts the ticket back to zero.  Nobody waits for anybody.
 *   ticket           B uint32, zero before the first launch; every launch leaves them zero.  Launches that share them must be
 *                    ordered on one stream.
 *   workspace        vmlmf_beam_workspace_bytes(B, W, V) bytes, 8-byte aligned
 * Refused (VMLMF_E_BADARG, nothing launched): B, H, V < 1, W outside [1, VMLMF_BEAM_MAX_BEAMS], W > V, W V >= 2^31, eos outside
 * [-1, V), a null pointer among the required ones, embed without x_next or the other way round; VMLMF_E_WORKSPACE: workspace too small.
 * If fewer than W candidates can be ordered (NaN scores) the remaining slots get parent 0, token 0 and a NaN total. */
int vmlmf_beam_step(int B, int W, int H, int V, const float *scores, const float *bias, const float *cum, const int32_t *finished,
                    const int32_t *length, int eos, const float *embed, int32_t *parent, int64_t *token, float *total,
                    int32_t *finished_out, int32_t *length_out, float *x_next, int32_t *src_row, uint32_t *ticket, void *workspace,
                    size_t workspace_bytes, void *stream);

/* dst[i][r][:] = src[i][src_row[r]][:] for the n tensors of a pointer table, each (rows, H) fp32, in ONE launch: the layers' (h, c)
 * follow their hypotheses.  src / dst: HOST arrays of n device pointers (copied into the launch's arguments); every dst must be a
 * buffer distinct from every src.  A src_row outside [0, rows) copies row r itself.  Refused: n outside [1, VMLMF_BEAM_MAX_TENSORS],
 * rows or H < 1, null pointers, a dst that is also a src. */
int vmlmf_beam_gather(int n, int rows, int H, const int32_t *src_row, const void *const *src, void *const *dst, void *stream);

/* out[j][b][w] = the j-th token of the hypothesis that ends in slot order[b][w] (order NULL: slot w) of the last step, read back
 * through the parent pointers: parent, token (steps, B, W) as vmlmf_beam_step wrote them step by step; order (B, W) int32 or NULL;
 * out (steps, B, W) int64.  One thread per (b, w) walks backwards.  Refused: steps, B < 1, W outside [1, VMLMF_BEAM_MAX_BEAMS], null. */
int vmlmf_beam_backtrack(int steps, int B, int W, const int32_t *parent, const int64_t *token, const int32_t *order, int64_t *out,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif
