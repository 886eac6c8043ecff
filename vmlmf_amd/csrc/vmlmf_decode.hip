// The controlled choice of the LM decoder (Model.generate with eos / min_length / repetition_penalty / logit_bias / banned_tokens,
// vmlmf_amd/lm.py): libvmlmf_decode.so, a library of its own beside libvmlmf_hip.so (include/vmlmf_decode.h has the contract).
// One launch per decode step behind the head's GEMM, a workgroup per row: the row's controlled score
//   c[v] = (seen[v] ? (x > 0 ? x / theta : x theta) : x) + logit_bias[v],   c[eos] = -inf below the minimum length
// takes the place of x = bias + scores in the keys and the tempered scores of the selection (vmlmf_select.h: the sampler's own
// pick_row / choose_row, instantiated here for ControlledScores - nothing of the selection is written twice), while the raw x keeps
// feeding (max, sum exp) and the log-probability.  The controls cost loads, not passes: pass 1 of the selection fetches a token's
// logit_bias and seen byte beside its score, eight tokens in flight; rows that fit LDS (V <= SF_LDS_V) never look at them again.
// A finished row writes its padding and returns; a live row's state (seen, length, finished) is updated in place by thread 0 behind a
// workgroup barrier, after every read of it.  Plain HIP C++ for wave64, no inline assembly, no atomics on global memory.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vmlmf_decode.h"
#include "vmlmf_refusals.h"
#include "vmlmf_select.h"
#include "vmlmf_side.h"

namespace {

constexpr int DC_FILTERED_NT = 1024;   // the selection's workgroup (lm_choose_filtered_kernel's)

struct DecodeArgs {
  const float *scores, *bias, *embed;
  const unsigned long long* state;
  long long* tokens;
  float *logprob, *x_next;
  int* kept;
  float inv_temp, top_p, theta;
  int B, H, V, step, top_k, eos, min_length;
  const float* logit_bias;
  unsigned char* seen;
  int *finished, *length;
};

// x -> c of one row (steps 1 - 3 of the contract)
struct ControlledScores {
  static constexpr bool CONTROLLED = true;
  struct Ctl {
    float lb;
    unsigned char seen;
  };
  const float *row, *bias, *logit_bias;
  const unsigned char* seen;
  float theta;
  int eos_ban;   // eos while the row is below its minimum length, else -1
  __device__ __forceinline__ float raw(int v) const { return (bias != nullptr ? bias[v] : 0.f) + row[v]; }
  __device__ __forceinline__ Ctl ctl(int v) const { return Ctl{logit_bias != nullptr ? logit_bias[v] : 0.f, seen[v]}; }
  __device__ __forceinline__ float score(int v, float x, const Ctl& ct) const {
    // (explicitly rounded operations: no contraction, so every pass of a long row forms the same bits)
    const float r = ct.seen != 0 ? (x > 0.f ? __fdiv_rn(x, theta) : __fmul_rn(x, theta)) : x;
    return v == eos_ban ? -INFINITY : __fadd_rn(r, ct.lb);
  }
};

__global__ __launch_bounds__(DC_FILTERED_NT) void decode_choose_kernel(DecodeArgs a) {
  __shared__ SelScratch S;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (a.eos >= 0 && a.finished[b] != 0) {   // (uniform over the workgroup) padding: nothing of the row's state moves
    if (tid == 0) {
      a.tokens[b] = a.eos;
      if (a.logprob != nullptr) a.logprob[b] = 0.f;
      if (a.kept != nullptr) a.kept[b] = 0;
    }
    if (a.x_next != nullptr) {
      const float* src = a.embed + (size_t)a.eos * a.H;
      for (int e = tid; e < a.H; e += blockDim.x) a.x_next[(size_t)b * a.H + e] = src[e];
    }
    return;
  }
  unsigned char* seen = a.seen + (size_t)b * a.V;
  ControlledScores src;
  src.row = a.scores + (size_t)b * a.V, src.bias = a.bias, src.logit_bias = a.logit_bias, src.seen = seen, src.theta = a.theta;
  src.eos_ban = (a.eos >= 0 && a.length[b] < a.min_length) ? a.eos : -1;
  const bool sampling = a.inv_temp > 0.f;
  const DropKey key = sampling ? sample_key(a.state) : DropKey{0u, 0u, 0u, 0u};
  const unsigned position = (unsigned)a.step * (unsigned)a.B + (unsigned)b;
  // the host launches DC_FILTERED_NT threads with a filter on, SM_CHOOSE_NT without
  const RowPick pk = blockDim.x == DC_FILTERED_NT ? pick_row(S, src, a.V, a.inv_temp, a.top_k, a.top_p, key, position)
                                                  : choose_row(&S.red[0][0], 8, src, a.V, a.inv_temp, sampling, key, position);
  write_pick(pk, b, a.H, a.tokens, a.logprob, a.kept, a.x_next, a.embed);
  __syncthreads();   // every thread has read what it needs of seen and length
  if (tid == 0) {
    const int tok = pk.idx != SM_NOIDX ? pk.idx : 0;
    seen[tok] = 1;
    a.length[b] += 1;
    if (tok == a.eos) a.finished[b] = 1;
  }
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
  a.scores = scores, a.bias = bias, a.embed = embed, a.state = reinterpret_cast<const unsigned long long*>(state);
  a.tokens = reinterpret_cast<long long*>(tokens), a.logprob = logprob, a.x_next = x_next, a.kept = kept;
  a.inv_temp = inv_temperature, a.top_p = top_p, a.theta = c->repetition_penalty;
  a.B = B, a.H = H, a.V = V, a.step = step, a.top_k = top_k >= V ? 0 : top_k, a.eos = c->eos, a.min_length = c->min_length;
  a.logit_bias = c->logit_bias, a.seen = c->seen, a.finished = c->finished, a.length = c->length;
  const bool filtered = inv_temperature > 0.f && (a.top_k > 0 || top_p < 1.f);
  hipLaunchKernelGGL(decode_choose_kernel, dim3(B), dim3(filtered ? DC_FILTERED_NT : SM_CHOOSE_NT), 0, static_cast<hipStream_t>(stream), a);
  return vmlmf_side::launch_tail("vmlmf_decode_choose");
}

}  // extern "C"
