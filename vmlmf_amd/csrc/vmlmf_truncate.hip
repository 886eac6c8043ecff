// The truncation samplers of the LM decoder (Model.generate with min_p / typical_p / epsilon_cutoff / eta_cutoff, vmlmf_amd/lm.py):
// libvmlmf_truncate.so, a library of its own beside libvmlmf_hip.so (include/vmlmf_truncate.h has the contract).  One launch per
// decode step behind the head's GEMM, a workgroup of 1024 threads per row - pick_row's shape on the same SelScratch (under 64 KB of
// static LDS): truncate_row (vmlmf_truncate.h) runs the stages and the draw, on the raw scores (PlainScores) or on a controlled
// row's (ControlledScores, vmlmf_controlled.h: the finished rows and the state update are vmlmf_decode_choose's, written once there).
// Plain HIP C++ for wave64, no inline assembly, no atomics on global memory.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vmlmf_truncate.h"
#include "vmlmf_controlled.h"
#include "vmlmf_refusals.h"
#include "vmlmf_select.h"
#include "vmlmf_side.h"
#include "vmlmf_truncate.h"

namespace {

constexpr int TR_NT = 1024;   // the selection's workgroup (lm_choose_filtered_kernel's)

struct TruncateArgs {
  ControlledRows rows;   // the scores and the outputs; with controls, the controls and the rows' state
  const unsigned long long* state;
  TruncParams tp;
  float inv_temp, top_p;
  int B, step, top_k;
};

template <bool CONTROLLED>
__global__ __launch_bounds__(TR_NT) void truncate_choose_kernel(TruncateArgs a) {
  __shared__ SelScratch S;
  const int b = blockIdx.x;
  const DropKey key = sample_key(a.state);
  const unsigned position = (unsigned)a.step * (unsigned)a.B + (unsigned)b;
  if (CONTROLLED) {
    if (a.rows.padding(b)) return;   // (uniform over the workgroup) a finished row: nothing of its state moves
    const RowPick pk = truncate_row(S, a.rows.source(b), a.rows.V, a.inv_temp, a.top_k, a.top_p, a.tp, key, position);
    a.rows.finish(pk, b);
  } else {
    PlainScores src;
    src.row = a.rows.scores + (size_t)b * a.rows.V, src.bias = a.rows.bias;
    const RowPick pk = truncate_row(S, src, a.rows.V, a.inv_temp, a.top_k, a.top_p, a.tp, key, position);
    write_pick(pk, b, a.rows.H, a.rows.tokens, a.rows.logprob, a.rows.kept, a.rows.x_next, a.rows.embed);
  }
}

int fail(int code, const char* msg) { return vmlmf_side::fail(code, std::string("vmlmf_truncate_choose: ") + msg); }

}  // namespace

VMLMF_SIDE_LIBRARY(vmlmf_truncate, VMLMF_TRUNCATE_ABI_VERSION)

extern "C" {

int vmlmf_truncate_choose(int B, int H, int V, const float* scores, const float* bias, const float* embed, float inv_temperature, int top_k,
                          float top_p, const vmlmf_truncation* t, const int64_t* state, int step, const vmlmf_decode_controls* c,
                          int64_t* tokens, float* logprob, float* x_next, int32_t* kept, void* stream) {
  if (B < 1 || V < 1 || (x_next && H < 1)) return fail(VMLMF_E_BADARG, "B, V (and H with x_next) must be >= 1");
  if (!scores || !tokens) return fail(VMLMF_E_BADARG, "null pointer (scores, tokens)");
  if (!t) return fail(VMLMF_E_BADARG, "null truncation");
  if (c && (!c->seen || !c->finished || !c->length))
    return fail(VMLMF_E_BADARG, "null pointer in the controls (seen, finished and length are required)");
  if (const int rc = sampler_refusal(fail, B, inv_temperature, state, embed, x_next, step)) return rc;
  if (inv_temperature == 0.f) return fail(VMLMF_E_UNSUPPORTED, "greedy decoding ignores truncation: run vmlmf_lm_choose or vmlmf_decode_choose");
  if (const int rc = filter_refusal(fail, top_k, top_p)) return rc;
  if (const int rc = truncation_refusal(fail, t->min_p, t->typical_p, t->epsilon_cutoff, t->eta_cutoff)) return rc;
  if (c)
    if (const int rc = controls_refusal(fail, V, c->eos, c->repetition_penalty, c->min_length)) return rc;
  TruncateArgs a;
  a.rows.scores = scores, a.rows.bias = bias, a.rows.embed = embed, a.rows.logit_bias = c ? c->logit_bias : nullptr;
  a.rows.tokens = reinterpret_cast<long long*>(tokens), a.rows.logprob = logprob, a.rows.x_next = x_next, a.rows.kept = kept;
  a.rows.seen = c ? c->seen : nullptr, a.rows.finished = c ? c->finished : nullptr, a.rows.length = c ? c->length : nullptr;
  a.rows.theta = c ? c->repetition_penalty : 1.f, a.rows.H = H, a.rows.V = V, a.rows.eos = c ? c->eos : -1;
  a.rows.min_length = c ? c->min_length : 0;
  a.state = reinterpret_cast<const unsigned long long*>(state);
  // log a once, in fp64, rounded to fp32: every pass compares fl(z - z_max) with the same bits
  a.tp.log_a = t->min_p > 0.f ? (float)log((double)t->min_p) : -INFINITY;
  a.tp.typical_p = t->typical_p, a.tp.epsilon = t->epsilon_cutoff, a.tp.eta = t->eta_cutoff;
  a.inv_temp = inv_temperature, a.top_p = top_p, a.B = B, a.step = step, a.top_k = top_k >= V ? 0 : top_k;
  if (c)
    hipLaunchKernelGGL(truncate_choose_kernel<true>, dim3(B), dim3(TR_NT), 0, static_cast<hipStream_t>(stream), a);
  else
    hipLaunchKernelGGL(truncate_choose_kernel<false>, dim3(B), dim3(TR_NT), 0, static_cast<hipStream_t>(stream), a);
  return vmlmf_side::launch_tail("vmlmf_truncate_choose");
}

}  // extern "C"
