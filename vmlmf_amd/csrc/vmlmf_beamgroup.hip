// The step of diverse (group) beam search (Model.group_beam_search): libvmlmf_beamgroup.so, a library of its own beside
// libvmlmf_beam.so (include/vmlmf_beamgroup.h has the contract), built by the Makefile's `more`.  One launch:
//   beam_step_kernel<OfferGroups>   vmlmf_beam_step's selection (csrc/vmlmf_beam_core.h - the kernel is written once, this file
//                          instantiates it with the policy below) whose per-beam half is the plain step's and whose merge, in the last
//                          workgroup of a batch row, runs group by group: a group's candidates ranked by total - lambda n, n the number
//                          of earlier groups' survivors of this step with the same token
// Every candidate is offered (the policy closes nothing); vmlmf_beam_core.h says why the per-beam first W candidates are enough.
// docs/design/lm_group_beam.md has the numbers.  Plain HIP C++ for wave64, no inline assembly.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vmlmf_beamgroup.h"
#include "vmlmf_beam_core.h"
#include "vmlmf_side.h"

namespace {

using namespace vmlmf_beam_core;

// the grouped merge policy (vmlmf_beam_core.h: merges_in_groups): everything open, no history, G groups under a penalty lambda
struct OfferGroups {
  static constexpr bool controlled = false;
  int groups;
  float lambda;
  struct Row {};
  __device__ __forceinline__ Row row(int) const { return Row{}; }
};
static_assert(merges_in_groups<OfferGroups>::value && !merges_in_groups<OfferAll>::value, "the trait finds the grouped policy alone");

using vmlmf_side::fail;

}  // namespace

VMLMF_SIDE_LIBRARY(vmlmf_beamgroup, VMLMF_BEAMGROUP_ABI_VERSION)

extern "C" {

size_t vmlmf_beamgroup_workspace_bytes(int B, int W, int V) { return step_workspace_bytes(B, W, V); }

int vmlmf_beamgroup_step(int B, int W, int H, int V, const float* scores, const float* bias, const float* cum, const int32_t* finished,
                         const int32_t* length, int eos, const float* embed, int32_t* parent, int64_t* token, float* total,
                         int32_t* finished_out, int32_t* length_out, float* x_next, int32_t* src_row, uint32_t* ticket, void* workspace,
                         size_t workspace_bytes, int groups, float diversity_penalty, void* stream) {
  const std::string name = "vmlmf_beamgroup_step: ";
  std::string why;
  BeamStepArgs a;
  if (const int rc = step_args(a, &why, B, W, H, V, scores, bias, cum, finished, length, eos, embed, parent, token, total, finished_out,
                               length_out, x_next, src_row, ticket, workspace, workspace_bytes, "vmlmf_beamgroup_workspace_bytes"))
    return fail(rc, name + why);
  if (groups < 1) return fail(VMLMF_E_BADARG, name + "groups must be >= 1");
  if (W % groups != 0) return fail(VMLMF_E_BADARG, name + "groups must divide W (beams): a group owns W / groups slots");
  if (!(diversity_penalty >= 0.f) || !isfinite(diversity_penalty))
    return fail(VMLMF_E_BADARG, name + "diversity_penalty must be finite and >= 0");
  OfferGroups p;
  p.groups = groups, p.lambda = diversity_penalty;
  hipLaunchKernelGGL(beam_step_kernel<OfferGroups>, dim3(B * W), dim3(BS_NT), 0, static_cast<hipStream_t>(stream), a, p);
  return vmlmf_side::launch_tail("vmlmf_beamgroup_step");
}

}  // extern "C"
