// The beam-search step of the LM decoder (Model.beam_search, vmlmf_amd/lm.py): libvmlmf_beam.so, a library of its own beside
// libvmlmf_hip.so (include/vmlmf_beam.h has the contract).  Three launches:
//   beam_step_kernel       one step's selection over the (B W, V) scores of the head's GEMM: per beam (max, sum exp), the candidate
//                          totals cum[w] + (x[v] - lse), the first W candidates of each batch row under the total order (larger total
//                          first, equal totals to the lower flat index w V + v - the sampler's tie rule over beams), and per survivor
//                          parent, token, total, finished flag, length, the next input row embed[token] and the source state row
//   beam_gather_kernel     the 2 L state tensors reordered by the source rows, all in one launch over a pointer table passed by value
//   beam_backtrack_kernel  the (steps, B, W) parent / token arrays read back into hypotheses, one thread per (b, w)
// The selection itself - the candidate key, the workgroup maximum, the step body - is csrc/vmlmf_beam_core.h, shared with
// libvmlmf_beamctl.so (the step under controls); this file instantiates it with every candidate offered.
// docs/design/lm_beam_search.md has the numbers.  Plain HIP C++ for wave64, no inline assembly.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vmlmf_beam.h"
#include "vmlmf_beam_core.h"
#include "vmlmf_side.h"

namespace {

using namespace vmlmf_beam_core;

struct BeamGatherArgs {
  const float* src[VMLMF_BEAM_MAX_TENSORS];
  float* dst[VMLMF_BEAM_MAX_TENSORS];
  const int32_t* src_row;
  int rows, H;
};
// grid (rows, n): workgroup (r, i) copies row src_row[r] of tensor i
__global__ __launch_bounds__(256) void beam_gather_kernel(BeamGatherArgs a) {
  const int r = blockIdx.x, i = blockIdx.y;
  int sr = a.src_row[r];
  if (sr < 0 || sr >= a.rows) sr = r;
  const float* s = a.src[i] + (size_t)sr * a.H;
  float* d = a.dst[i] + (size_t)r * a.H;
  for (int k = threadIdx.x; k < a.H; k += 256) d[k] = s[k];
}

__global__ __launch_bounds__(64) void beam_backtrack_kernel(int steps, int B, int W, const int32_t* parent, const long long* token,
                                                            const int32_t* order, long long* out) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= B * W) return;
  const int b = e / W;
  int cur = order != nullptr ? order[e] : e - b * W;
  for (int j = steps - 1; j >= 0; --j) {
    if (cur < 0 || cur >= W) cur = 0;
    const size_t at = ((size_t)j * B + b) * W + cur;
    out[((size_t)j * B) * W + e] = token[at];
    cur = parent[at];
  }
}

using vmlmf_side::fail;   // (every call site gives the entry point's name itself)

}  // namespace

VMLMF_SIDE_LIBRARY(vmlmf_beam, VMLMF_BEAM_ABI_VERSION)

extern "C" {

size_t vmlmf_beam_workspace_bytes(int B, int W, int V) { return step_workspace_bytes(B, W, V); }

int vmlmf_beam_step(int B, int W, int H, int V, const float* scores, const float* bias, const float* cum, const int32_t* finished,
                    const int32_t* length, int eos, const float* embed, int32_t* parent, int64_t* token, float* total,
                    int32_t* finished_out, int32_t* length_out, float* x_next, int32_t* src_row, uint32_t* ticket, void* workspace,
                    size_t workspace_bytes, void* stream) {
  std::string why;
  BeamStepArgs a;
  if (const int rc = step_args(a, &why, B, W, H, V, scores, bias, cum, finished, length, eos, embed, parent, token, total, finished_out,
                               length_out, x_next, src_row, ticket, workspace, workspace_bytes, "vmlmf_beam_workspace_bytes"))
    return fail(rc, "vmlmf_beam_step: " + why);
  // the step with every candidate offered (vmlmf_beam_core.h has the kernel)
  hipLaunchKernelGGL(beam_step_kernel<OfferAll>, dim3(B * W), dim3(BS_NT), 0, static_cast<hipStream_t>(stream), a, OfferAll{});
  return vmlmf_side::launch_tail("vmlmf_beam_step");
}

int vmlmf_beam_gather(int n, int rows, int H, const int32_t* src_row, const void* const* src, void* const* dst, void* stream) {
  if (n < 1 || n > VMLMF_BEAM_MAX_TENSORS) return fail(VMLMF_E_BADARG, "vmlmf_beam_gather: n must lie in [1, 16] tensors a launch");
  if (rows < 1 || H < 1) return fail(VMLMF_E_BADARG, "vmlmf_beam_gather: rows and H must be >= 1");
  if (rows > 65535 * 1024) return fail(VMLMF_E_BADARG, "vmlmf_beam_gather: too many rows for one launch");
  if (!src_row || !src || !dst) return fail(VMLMF_E_BADARG, "vmlmf_beam_gather: null pointer");
  BeamGatherArgs a;
  for (int i = 0; i < VMLMF_BEAM_MAX_TENSORS; ++i) a.src[i] = nullptr, a.dst[i] = nullptr;
  for (int i = 0; i < n; ++i) {
    if (!src[i] || !dst[i]) return fail(VMLMF_E_BADARG, "vmlmf_beam_gather: null pointer in the table");
    a.src[i] = static_cast<const float*>(src[i]), a.dst[i] = static_cast<float*>(dst[i]);
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j)
      if (dst[i] == src[j]) return fail(VMLMF_E_BADARG, "vmlmf_beam_gather: a destination is also a source (rows would be read after they were overwritten)");
  a.src_row = src_row, a.rows = rows, a.H = H;
  hipLaunchKernelGGL(beam_gather_kernel, dim3(rows, n), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return vmlmf_side::launch_tail("vmlmf_beam_gather");
}

int vmlmf_beam_backtrack(int steps, int B, int W, const int32_t* parent, const int64_t* token, const int32_t* order, int64_t* out,
                         void* stream) {
  if (steps < 1 || B < 1) return fail(VMLMF_E_BADARG, "vmlmf_beam_backtrack: steps and B must be >= 1");
  if (W < 1 || W > VMLMF_BEAM_MAX_BEAMS) return fail(VMLMF_E_BADARG, "vmlmf_beam_backtrack: W (beams) must lie in [1, 32]");
  if ((long long)B * W >= (1ll << 31)) return fail(VMLMF_E_BADARG, "vmlmf_beam_backtrack: B W must stay below 2^31");
  if (!parent || !token || !out) return fail(VMLMF_E_BADARG, "vmlmf_beam_backtrack: null pointer (only order may be null)");
  hipLaunchKernelGGL(beam_backtrack_kernel, dim3((B * W + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream), steps, B, W, parent,
                     reinterpret_cast<const long long*>(token), order, reinterpret_cast<long long*>(out));
  return vmlmf_side::launch_tail("vmlmf_beam_backtrack");
}

}  // extern "C"
