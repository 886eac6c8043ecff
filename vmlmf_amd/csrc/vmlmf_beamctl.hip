// The beam-search step under controls (Model.beam_search with min_length, banned_tokens, no_repeat_ngram_size or banned_sequences):
// libvmlmf_beamctl.so, a library of its own beside libvmlmf_beam.so (include/vmlmf_beamctl.h has the contract).  One launch:
//   beam_step_kernel<OfferOpen>   vmlmf_beam_step's selection (csrc/vmlmf_beam_core.h - the kernel is written once, this file instantiates
//                          it with the policy below) in which a live beam withholds the tokens of the shared `closed` words, of its own ban
//                          words and - below min_length - eos, and whose last workgroup of a batch row copies the survivors' histories
// The mask words are read from global memory in pass 2, where the totals are formed: the 64 lanes of a wave look at two words of each
// set, and a row that stays in LDS keeps a NaN in a closed candidate's place, which every later scan skips.  Pass 1 and the
// (max, sum exp) tree are the plain step's: lse is taken over the raw row.  The per-beam ban words come from a vmlmf_history_bans
// launch on B W rows in front of this one (libvmlmf_history.so).  docs/design/lm_beam_controls.md has the numbers.
// Plain HIP C++ for wave64, no inline assembly.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vmlmf_beamctl.h"
#include "vmlmf_beam_core.h"
#include "vmlmf_side.h"

namespace {

using namespace vmlmf_beam_core;

// the controlled offer policy (vmlmf_beam_core.h says what a policy is)
struct OfferOpen {
  static constexpr bool controlled = true;
  int min_length, eos, words, cap;
  const uint32_t *closed, *bans;
  const int32_t *length, *hist, *hist_len;
  int32_t *hist_out, *hist_len_out, *overflow;
  struct Row {
    const uint32_t *closed, *bans;   // the shared words; this beam's own
    int held;                        // eos while the beam is below min_length, else -1
    __device__ __forceinline__ bool closes(int v) const {
      unsigned m = closed != nullptr ? closed[v >> 5] : 0u;
      if (bans != nullptr) m |= bans[v >> 5];
      return ((m >> (v & 31)) & 1u) != 0u || v == held;
    }
  };
  __device__ __forceinline__ Row row(int r) const {
    return Row{closed, bans != nullptr ? bans + (size_t)r * words : nullptr, (eos >= 0 && length[r] < min_length) ? eos : -1};
  }
  __device__ __forceinline__ bool keeps_history() const { return hist != nullptr; }
};

using vmlmf_side::fail;

}  // namespace

VMLMF_SIDE_LIBRARY(vmlmf_beamctl, VMLMF_BEAMCTL_ABI_VERSION)

extern "C" {

size_t vmlmf_beamctl_workspace_bytes(int B, int W, int V) { return step_workspace_bytes(B, W, V); }

int vmlmf_beamctl_step(int B, int W, int H, int V, const float* scores, const float* bias, const float* cum, const int32_t* finished,
                       const int32_t* length, int eos, const float* embed, const vmlmf_beamctl_controls* c, int32_t* parent,
                       int64_t* token, float* total, int32_t* finished_out, int32_t* length_out, float* x_next, int32_t* src_row,
                       uint32_t* ticket, void* workspace, size_t workspace_bytes, void* stream) {
  const std::string name = "vmlmf_beamctl_step: ";
  std::string why;
  BeamStepArgs a;
  if (const int rc = step_args(a, &why, B, W, H, V, scores, bias, cum, finished, length, eos, embed, parent, token, total, finished_out,
                               length_out, x_next, src_row, ticket, workspace, workspace_bytes, "vmlmf_beamctl_workspace_bytes"))
    return fail(rc, name + why);
  if (!c) return fail(VMLMF_E_BADARG, name + "null controls");
  if (c->min_length < 0) return fail(VMLMF_E_BADARG, name + "min_length must be >= 0");
  if (c->min_length > 0 && eos < 0) return fail(VMLMF_E_BADARG, name + "min_length needs eos (the token it holds back)");
  const bool some = c->hist || c->hist_len || c->hist_out || c->hist_len_out || c->overflow;
  const bool all = c->hist && c->hist_len && c->hist_out && c->hist_len_out && c->overflow;
  if (some && !all)
    return fail(VMLMF_E_BADARG, name + "hist, hist_len, hist_out, hist_len_out and overflow come together (all, or all null)");
  if (c->hist_capacity < 1) return fail(VMLMF_E_BADARG, name + "hist_capacity must be >= 1");
  if (all && (c->hist == c->hist_out || c->hist_len == c->hist_len_out))
    return fail(VMLMF_E_BADARG, name + "hist_out must not alias hist (the merge reads other slots' histories)");
  if (c->bans && V > VMLMF_HISTORY_MAX_V)
    return fail(VMLMF_E_BADARG, name + "per-beam bans need V <= VMLMF_HISTORY_MAX_V (65536): vmlmf_history_bans writes them");
  OfferOpen p;
  p.min_length = c->min_length, p.eos = eos, p.words = (V + 31) / 32, p.cap = c->hist_capacity;
  p.closed = c->closed, p.bans = c->bans, p.length = length, p.hist = c->hist, p.hist_len = c->hist_len;
  p.hist_out = c->hist_out, p.hist_len_out = c->hist_len_out, p.overflow = c->overflow;
  hipLaunchKernelGGL(beam_step_kernel<OfferOpen>, dim3(B * W), dim3(BS_NT), 0, static_cast<hipStream_t>(stream), a, p);
  return vmlmf_side::launch_tail("vmlmf_beamctl_step");
}

}  // extern "C"
