// The controlled choice of the LM decoder (Model.generate with eos / min_length / repetition_penalty / logit_bias / banned_tokens,
// vmlmf_amd/lm.py): libvmlmf_decode.so, a library of its own beside libvmlmf_hip.so (include/vmlmf_decode.h has the contract).
// One launch per decode step behind the head's GEMM, a workgroup per row: the row's controlled score
//   c[v] = (seen[v] ? (x > 0 ? x / theta : x theta) : x) + logit_bias[v],   c[eos] = -inf below the minimum length
// takes the place of x = bias + scores in the keys and the tempered scores of the selection (vmlmf_select.h: the sampler's own
// pick_row / choose_row, instantiated here for ControlledScores - nothing of the selection is written twice), while the raw x keeps
// feeding (max, sum exp) and the log-probability.  The controls cost loads, not passes: pass 1 of the selection fetches a token's
// logit_bias and seen byte beside its score, eight tokens in flight; rows that fit LDS (V <= SF_LDS_V) never look at them again.
// A finished row writes its padding and returns; a live row's state (seen, length, finished) is updated in place by thread 0 behind a
// workgroup barrier, after every read of it (ControlledScores and that state update are vmlmf_controlled.h's: vmlmf_truncate.hip runs
// them too).  Plain HIP C++ for wave64, no inline assembly, no atomics on global memory.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vmlmf_decode.h"
#include "vmlmf_controlled.h"
#include "vmlmf_refusals.h"
#include "vmlmf_select.h"
#include "vmlmf_side.h"

namespace {

constexpr int DC_FILTERED_NT = 1024;   // the selection's workgroup (lm_choose_filtered_kernel's)

struct DecodeArgs {
  ControlledRows rows;   // vmlmf_controlled.h: the scores, the controls, the rows' state and the outputs
  const unsigned long long* state;
  float inv_temp, top_p;
  int B, step, top_k;
};

__global__ __launch_bounds__(DC_FILTERED_NT) void decode_choose_kernel(DecodeArgs a) {
  __shared__ SelScratch S;
  const int b = blockIdx.x;
  if (a.rows.padding(b)) return;   // (uniform over the workgroup) a finished row: nothing of its state moves
  const ControlledScores src = a.rows.source(b);
  const bool sampling = a.inv_temp > 0.f;
  const DropKey key = sampling ? sample_key(a.state) : DropKey{0u, 0u, 0u, 0u};
  const unsigned position = (unsigned)a.step * (unsigned)a.B + (unsigned)b;
  // the host launches DC_FILTERED_NT threads with a filter on, SM_CHOOSE_NT without
  const RowPick pk = blockDim.x == DC_FILTERED_NT ? pick_row(S, src, a.rows.V, a.inv_temp, a.top_k, a.top_p, key, position)
                                                  : choose_row(&S.red[0][0], 8, src, a.rows.V, a.inv_temp, sampling, key, position);
  a.rows.finish(pk, b);
}

int fail(int code, const char* msg) { return vmlmf_side::fail(code, std::string("vmlmf_decode_choose: ") + msg); }

}  // namespace

VMLMF_SIDE_LIBRARY(vmlmf_decode, VMLMF_DECODE_ABI_VERSION)

extern "C" {

int vmlmf_decode_choose(int B, int H, int V, const float* scores, const float* bias, const float* embed, float inv_temperature, int top_k,
                        float top_p, const int64_t* state, int step, const vmlmf_decode_controls* c, int64_t* tokens, float* logprob,
                        float* x_next, int32_t* kept, void* stream) {
  if (B < 1 || V < 1 || (x_next && H < 1)) return fail(VMLMF_E_BADARG, "B, V (and H with x_next) must be >= 1");
  if (!scores || !tokens) return fail(VMLMF_E_BADARG, "null pointer (scores, tokens)");
  if (!c) return fail(VMLMF_E_BADARG, "null controls");
  if (!c->seen || !c->finished || !c->length) return fail(VMLMF_E_BADARG, "null pointer in the controls (seen, finished and length are required)");
  if (const int rc = sampler_refusal(fail, B, inv_temperature, state, embed, x_next, step)) return rc;
  if (const int rc = filter_refusal(fail, top_k, top_p)) return rc;
  if (const int rc = controls_refusal(fail, V, c->eos, c->repetition_penalty, c->min_length)) return rc;
  DecodeArgs a;
  a.rows.scores = scores, a.rows.bias = bias, a.rows.embed = embed, a.rows.logit_bias = c->logit_bias;
  a.rows.tokens = reinterpret_cast<long long*>(tokens), a.rows.logprob = logprob, a.rows.x_next = x_next, a.rows.kept = kept;
  a.rows.seen = c->seen, a.rows.finished = c->finished, a.rows.length = c->length, a.rows.theta = c->repetition_penalty;
  a.rows.H = H, a.rows.V = V, a.rows.eos = c->eos, a.rows.min_length = c->min_length;
  a.state = reinterpret_cast<const unsigned long long*>(state);
  a.inv_temp = inv_temperature, a.top_p = top_p, a.B = B, a.step = step, a.top_k = top_k >= V ? 0 : top_k;
  const bool filtered = inv_temperature > 0.f && (a.top_k > 0 || top_p < 1.f);
  hipLaunchKernelGGL(decode_choose_kernel, dim3(B), dim3(filtered ? DC_FILTERED_NT : SM_CHOOSE_NT), 0, static_cast<hipStream_t>(stream), a);
  return vmlmf_side::launch_tail("vmlmf_decode_choose");
}

}  // extern "C"
