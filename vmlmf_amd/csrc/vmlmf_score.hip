// Scoring given text (Model.score, vmlmf_amd.lm_score; vmlmf_amd/scoring.py): libvmlmf_score.so, a library of its own beside
// libvmlmf_hip.so (include/vmlmf_score.h has the contract).  One launch behind the head's GEMM, a workgroup per row: the target's
// log-probability and rank, and the row's `top` most probable tokens in order.
// The row is read by the sampler's own choose_row (vmlmf_select.h) - so (max, sum exp) are its bits, and the greedy token's
// log-probability is vmlmf_lm_choose's - through a Src whose raw() also does whatever else needs every score once: it compares the
// score's key with the target's (the rank) and, with top > 0, leaves the key in LDS.  The top tokens are then the selection of the
// filtered sampler on those keys: radix_select over counts finds the top-th key, tie_cutoff the last index admitted from its tie
// group; the <= 32 survivors are gathered into LDS (an integer counter hands out the slots, in whatever order) and every one of them
// finds its place by counting the survivors ahead of it, which makes the written order independent of the gathering's.
// Rows longer than SF_LDS_V are read again from memory by each pass of the selection (four levels, the tie cut, the gathering).
// Plain HIP C++ for wave64, no inline assembly, no atomics on floats or on global memory.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vmlmf_score.h"
#include "vmlmf_select.h"
#include "vmlmf_side.h"

namespace {

struct ScoreArgs {
  const float *scores, *bias;
  const long long* targets;
  float *logprob, *top_logprob;
  int* rank;
  long long* top_tokens;
  int V, top;
};

// the key the order runs on: larger x <=> larger key, -0 and +0 share one (what SelRow::key forms at temperature 1)
__device__ __forceinline__ unsigned order_key(float x) { return key_of(tempered(x, 1.f)); }

// a row as choose_row reads it - every score once - and what else that one read serves
struct ScoredRow {
  static constexpr bool CONTROLLED = false;
  struct Ctl {};
  PlainScores x;
  unsigned* keys;       // LDS (top > 0 and the row fits), or nullptr
  unsigned ky;          // the target's key and index; without a target (0xffffffff, -1): nothing is ahead
  int y;
  mutable int ahead;    // this thread's tokens ahead of the target
  mutable bool nan;
  __device__ __forceinline__ float raw(int v) const {
    const float s = x.raw(v);
    const unsigned k = order_key(s);
    if (keys != nullptr) keys[v] = k;
    ahead += (k > ky || (k == ky && v < y)) ? 1 : 0;
    nan = nan || s != s;
    return s;
  }
  __device__ __forceinline__ Ctl ctl(int) const { return Ctl{}; }
  __device__ __forceinline__ float score(int, float s, const Ctl&) const { return s; }
};

template <bool TOP>
struct Scratch;
template <>
struct Scratch<false> {
  float red[SM_CHOOSE_NT / 64][8];
  __device__ __forceinline__ float* reduction() { return &red[0][0]; }
  __device__ __forceinline__ unsigned* keys() { return nullptr; }
};
template <>
struct Scratch<true> {
  SelScratch sel;
  unsigned ckey[VMLMF_SCORE_MAX_TOP];   // the survivors, as gathered
  int cidx[VMLMF_SCORE_MAX_TOP];
  int n;
  __device__ __forceinline__ float* reduction() { return &sel.red[0][0]; }
  __device__ __forceinline__ unsigned* keys() { return sel.keys; }
};

// TOP: a.top > 0 (the other instance holds no key buffer, so as many of its workgroups fit a CU as of vmlmf_lm_choose's)
template <bool TOP>
__global__ __launch_bounds__(SM_CHOOSE_NT) void score_rows_kernel(ScoreArgs a) {
  __shared__ Scratch<TOP> S;
  const int r = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, V = a.V;
  const long long y64 = a.targets != nullptr ? a.targets[r] : -1ll;
  const bool has_y = y64 >= 0, in_row = has_y && y64 < (long long)V;
  const PlainScores plain{a.scores + (size_t)r * V, a.bias};
  const float xy = in_row ? plain.raw((int)y64) : 0.f;   // (a target past the row: nothing is loaded for it)
  const bool resident = TOP && V <= SF_LDS_V;
  if constexpr (TOP) {   // (visible behind choose_row's barrier)
    if (tid < VMLMF_SCORE_MAX_TOP) S.ckey[tid] = 0u, S.cidx[tid] = 0;
    if (tid == 0) S.n = 0;
  }
  ScoredRow src{plain, resident ? S.keys() : nullptr, in_row ? order_key(xy) : 0xffffffffu, in_row ? (int)y64 : -1, 0, false};
  float* red = S.reduction();
  // the one read of the row: choose_row's slots are red[wave][0..4], the count and the NaN flag go to [6] and [7] behind its barrier
  const RowPick pk = choose_row(red, 8, src, V, 0.f, false, DropKey{0u, 0u, 0u, 0u}, 0u);
  int ahead = src.ahead;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) ahead += __shfl_xor(ahead, o, 64);
  const bool wave_nan = __ballot(src.nan) != 0ull;
  if (lane == 0) red[wave * 8 + 6] = __int_as_float(ahead), red[wave * 8 + 7] = __int_as_float(wave_nan ? 1 : 0);
  __syncthreads();
  ahead = 0;
  int any_nan = 0;
#pragma unroll
  for (int w = 0; w < SM_CHOOSE_NT / 64; ++w) ahead += __float_as_int(red[w * 8 + 6]), any_nan |= __float_as_int(red[w * 8 + 7]);
  const float lse = any_nan != 0 ? NAN : pk.m + logf(pk.s);
  if (tid == 0) {
    if (a.logprob != nullptr) a.logprob[r] = !has_y ? 0.f : in_row ? xy - lse : NAN;
    if (a.rank != nullptr) a.rank[r] = in_row ? ahead : -1;
  }
  if constexpr (TOP) {
    SelScratch& sel = S.sel;
    SelRow<PlainScores> row;
    row.src = plain, row.inv_temp = 1.f, row.zmax = 0.f, row.V = V, row.nt = SM_CHOOSE_NT, row.resident = resident, row.keys = sel.keys;
    // the top-th key K, and the last index admitted from its tie group (top == V: every token)
    unsigned K = 0u;
    int cut = V;
    if (a.top < V) {
      u64 target = (u64)a.top, above, leaf;
      radix_select(row, sel, false, false, 0u, 0ull, 1.f, target, K, above, leaf);
      const u64 n_tie = target - above;
      if (n_tie < leaf) cut = tie_cutoff(row, sel, K, (int)n_tie);
    }
    for_quads(row, [&](int qd, const unsigned(&k4)[4]) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int v = 4 * qd + e;
        if (v < V && (k4[e] > K || (k4[e] == K && v <= cut))) {
          const int slot = atomicAdd(&S.n, 1);
          if (slot < VMLMF_SCORE_MAX_TOP) S.ckey[slot] = k4[e], S.cidx[slot] = v;
        }
      }
    });
    __syncthreads();
    if (tid < a.top) {
      const unsigned k = S.ckey[tid];
      const int v = S.cidx[tid];
      int pos = 0;
      for (int j = 0; j < a.top; ++j) pos += (S.ckey[j] > k || (S.ckey[j] == k && S.cidx[j] < v)) ? 1 : 0;
      if (pos < a.top) {   // (always: the survivors are distinct tokens)
        a.top_tokens[(size_t)r * a.top + pos] = v;
        a.top_logprob[(size_t)r * a.top + pos] = z_of(k) - lse;
      }
    }
  }
}

int fail(int code, const char* msg) { return vmlmf_side::fail(code, std::string("vmlmf_score_rows: ") + msg); }

}  // namespace

VMLMF_SIDE_LIBRARY(vmlmf_score, VMLMF_SCORE_ABI_VERSION)

extern "C" {

int vmlmf_score_rows(int R, int V, const float* scores, const float* bias, const int64_t* targets, int top, float* logprob, int32_t* rank,
                     int64_t* top_tokens, float* top_logprob, void* stream) {
  if (R < 1 || V < 1) return fail(VMLMF_E_BADARG, "R and V must be >= 1");
  if (!scores) return fail(VMLMF_E_BADARG, "null pointer (scores)");
  if (top < 0 || top > VMLMF_SCORE_MAX_TOP || top > V) return fail(VMLMF_E_BADARG, "top must lie in [0, min(32, V)]");
  if (top > 0 && (!top_tokens || !top_logprob)) return fail(VMLMF_E_BADARG, "top > 0 needs top_tokens and top_logprob");
  if (targets && !logprob) return fail(VMLMF_E_BADARG, "targets need logprob");
  ScoreArgs a;
  a.scores = scores, a.bias = bias, a.targets = reinterpret_cast<const long long*>(targets);
  a.logprob = logprob, a.top_logprob = top_logprob, a.rank = rank, a.top_tokens = reinterpret_cast<long long*>(top_tokens);
  a.V = V, a.top = top;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (top > 0) hipLaunchKernelGGL(score_rows_kernel<true>, dim3(R), dim3(SM_CHOOSE_NT), 0, s, a);
  else hipLaunchKernelGGL(score_rows_kernel<false>, dim3(R), dim3(SM_CHOOSE_NT), 0, s, a);
  return vmlmf_side::launch_tail("vmlmf_score_rows");
}

}  // extern "C"
