// The step of contrastive search (Model.contrastive_search): libvmlmf_contrast.so, a library of its own (include/vmlmf_contrast.h has
// the contract), built by the Makefile's `extra`.  Three kernels:
//   contrast_append_kernel   a wave per (t, b): the row h[t][b] as a unit vector behind the row's history
//   contrast_advance_kernel  hist_len[b] += T behind it (a launch of its own: the append's waves read hist_len)
//   contrast_choose_kernel   the step, ONE launch over B x parts workgroups of sixteen waves.  A workgroup leaves the row's k unit
//                            candidates in LDS, then each of its waves streams history rows - one row at a time, lane l the 16-, 8- or
//                            4-byte pieces l, l + 64, ... with a whole row's loads in flight, k running sums per lane, a butterfly per
//                            sum - and keeps the k maxima; the waves' maxima meet in LDS, the workgroup's go to the workspace, and the
//                            row's last-arriving workgroup (the ticket protocol of csrc/vmlmf_beam_core.h) merges the parts' maxima,
//                            chooses, appends the chosen unit vector and routes the states.
// A dot product belongs to one wave and is summed in an order fixed by H; the maxima are exact: the same bits for every `parts`.
// docs/design/lm_contrastive.md has the numbers, what bounds the launch and why the fp32 MFMA form was not built.  Plain HIP C++ for wave64, no inline assembly.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/vmlmf_contrast.h"
#include "vmlmf_rowops.h"
#include "vmlmf_side.h"

namespace {

constexpr int CS_NT = 1024;          // threads of a choose workgroup: sixteen waves share one copy of the unit candidates
constexpr int CS_NW = CS_NT / 64;
constexpr int CS_MAXK = VMLMF_CONTRAST_MAX_K;
// a lane's loads of one history row in flight: a row of up to 1024 floats (512 for 4-byte pieces) is requested whole
template <int VW>
constexpr int cs_unroll() { return VW == 4 ? 4 : 8; }

using vmlmf_side::fail;

// ---- the normalisation rule, written once: every lane of ONE full wave calls it and gets 1 / |x| (0: x stays or becomes zero) ----
__device__ __forceinline__ float unit_scale(const float* __restrict__ x, int H, int lane) {
  float s = 0.f;
  for (int e0 = lane; e0 < H; e0 += 4 * 64) {   // four loads in flight; the order of the sum is the plain loop's
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = x[e0 + 64 * q < H ? e0 + 64 * q : e0];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (e0 + 64 * q < H) s = __fmaf_rn(v[q], v[q], s);
  }
  s = wave_sum(s);
  return (s > 0.f && s < INFINITY) ? 1.0f / sqrtf(s) : 0.f;
}
__device__ __forceinline__ float unit_of(float x, float inv) { return inv != 0.f ? __fmul_rn(x, inv) : 0.f; }

// an exact maximum that a NaN wins whatever the order (-inf is its neutral element)
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || b != b) ? NAN : fmaxf(a, b); }

__global__ __launch_bounds__(64) void contrast_append_kernel(int B, int T, int H, int Tcap, const float* __restrict__ h,
                                                             float* __restrict__ hist, const int32_t* __restrict__ hist_len) {
  const int lane = threadIdx.x, row = blockIdx.x, t = row / B, b = row - t * B;
  int L = hist_len[b];
  L = L < 0 ? 0 : L;
  if ((long long)L + t >= Tcap) return;   // a full history is never written past (uniform)
  const float* x = h + (size_t)row * H;
  float* out = hist + ((size_t)b * Tcap + L + t) * H;
  const float inv = unit_scale(x, H, lane);
  for (int e = lane; e < H; e += 64) out[e] = unit_of(x[e], inv);
}

__global__ void contrast_advance_kernel(int B, int T, int Tcap, int32_t* hist_len) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int L = hist_len[b];
  L = L < 0 ? 0 : L;
  hist_len[b] = (long long)L + T >= Tcap ? Tcap : L + T;
}

struct ChooseArgs {
  int B, k, H, Tcap, eos, parts;
  float alpha;
  const float *cand_h, *cand_logp;
  const long long* cand_tok;
  float *hist, *logprob, *sim, *h_next, *part_max;
  int32_t *hist_len, *finished, *length, *chosen, *src_row;
  long long* token;
  unsigned* ticket;
};

template <int VW>
struct Piece;
template <>
struct Piece<4> {
  typedef float4 type;
  static __device__ __forceinline__ float dot(float4 a, float4 b, float s) {
    return __fmaf_rn(a.w, b.w, __fmaf_rn(a.z, b.z, __fmaf_rn(a.y, b.y, __fmaf_rn(a.x, b.x, s))));
  }
};
template <>
struct Piece<2> {
  typedef float2 type;
  static __device__ __forceinline__ float dot(float2 a, float2 b, float s) { return __fmaf_rn(a.y, b.y, __fmaf_rn(a.x, b.x, s)); }
};
template <>
struct Piece<1> {
  typedef float type;
  static __device__ __forceinline__ float dot(float a, float b, float s) { return __fmaf_rn(a, b, s); }
};

// KT: k rounded up to a power of two (the running sums are registers: their index must be a constant); VW: floats per piece
template <int KT, int VW>
__global__ __launch_bounds__(CS_NT) void contrast_choose_kernel(ChooseArgs a) {
  typedef typename Piece<VW>::type piece_t;
  constexpr int CS_UNROLL = cs_unroll<VW>();
  extern __shared__ float4 cs_lds4[];               // (k, Hp) unit candidates, rows padded to four floats
  float* unit = reinterpret_cast<float*>(cs_lds4);
  __shared__ float wave_m[CS_NW][CS_MAXK];
  __shared__ float part_m[VMLMF_CONTRAST_MAX_PARTS][CS_MAXK];
  __shared__ float row_m[CS_MAXK];
  __shared__ int s_last, s_pick;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P = a.parts, b = blockIdx.x / P, part = blockIdx.x - b * P;
  const int k = a.k, H = a.H, Hp = (H + 3) & ~3;
  const bool done = a.eos >= 0 && a.finished[b] != 0;
  int t = a.hist_len[b];
  t = t < 0 ? 0 : (t > a.Tcap ? a.Tcap : t);
  const float* ch = a.cand_h + (size_t)b * k * H;
  // this part's rows: part NW + wave, then every P NW-th; a finished row's history is not read
  const bool works = !done && part * CS_NW < t;
  float m[KT];
#pragma unroll
  for (int j = 0; j < KT; ++j) m[j] = -INFINITY;
  if (works) {   // (uniform over the workgroup)
    for (int j = wave; j < k; j += CS_NW) {
      const float* x = ch + (size_t)j * H;
      const float inv = unit_scale(x, H, lane);
      for (int e = lane; e < Hp; e += 64) unit[j * Hp + e] = e < H ? unit_of(x[e], inv) : 0.f;
    }
    __syncthreads();
    const int nch = H / VW;   // (VW divides H: the host chose it so)
    const piece_t* U = reinterpret_cast<const piece_t*>(unit);
    // a sum beyond k repeats candidate k - 1 and is never looked at: no branch in the loop below
    int urow[KT];
#pragma unroll
    for (int j = 0; j < KT; ++j) urow[j] = (j < k ? j : k - 1) * (Hp / VW);
    for (int i = part * CS_NW + wave; i < t; i += P * CS_NW) {
      const piece_t* row = reinterpret_cast<const piece_t*>(a.hist + ((size_t)b * a.Tcap + i) * H);
      float acc[KT];
#pragma unroll
      for (int j = 0; j < KT; ++j) acc[j] = 0.f;
      for (int c0 = lane; c0 < nch; c0 += 64 * CS_UNROLL) {
        piece_t v[CS_UNROLL];
#pragma unroll
        for (int q = 0; q < CS_UNROLL; ++q) v[q] = row[c0 + 64 * q < nch ? c0 + 64 * q : c0];
#pragma unroll
        for (int q = 0; q < CS_UNROLL; ++q) {
          const int c = c0 + 64 * q;
          if (c < nch) {
#pragma unroll
            for (int j = 0; j < KT; ++j) acc[j] = Piece<VW>::dot(v[q], U[urow[j] + c], acc[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < KT; ++j)
        if (j < k) m[j] = nan_max(m[j], wave_sum(acc[j]));
    }
  }
  // the waves' maxima -> the workgroup's, by the threads j < k
#pragma unroll
  for (int j = 0; j < KT; ++j)
    if (lane == 0 && j < k) wave_m[wave][j] = m[j];
  __syncthreads();
  if (tid < k) {
    float r = wave_m[0][tid];
#pragma unroll
    for (int w = 1; w < CS_NW; ++w) r = nan_max(r, wave_m[w][tid]);
    row_m[tid] = r;
    if (P > 1) a.part_max[((size_t)b * P + part) * CS_MAXK + tid] = r;
  }
  __syncthreads();   // orders the stores above before thread 0's release
  if (P > 1) {
    if (tid == 0) {
      const unsigned got = __hip_atomic_fetch_add(a.ticket + b, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
      s_last = got == (unsigned)P - 1u;
    }
    __syncthreads();
    if (!s_last) return;
    // last arrival of row b: acquire in every wave, then the parts' maxima in part order (any order gives the same bits)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    {   // thread (p, j) takes part p's maximum of candidate j, then the parts meet in LDS
      static_assert(CS_NT / CS_MAXK >= VMLMF_CONTRAST_MAX_PARTS, "a thread per part and candidate");
      const int j = tid & (CS_MAXK - 1), p = tid / CS_MAXK;
      if (p < VMLMF_CONTRAST_MAX_PARTS) part_m[p][j] = (j < k && p < P) ? a.part_max[((size_t)b * P + p) * CS_MAXK + j] : -INFINITY;
      __syncthreads();
      if (tid < k) {
        float r = part_m[0][tid];
        for (int q = 1; q < P; ++q) r = nan_max(r, part_m[q][tid]);
        row_m[tid] = r;
      }
    }
    __syncthreads();
    if (tid == 0) __hip_atomic_store(a.ticket + b, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // the choice, by thread 0: k <= 16 values in order
  if (tid == 0) {
    int best = -1;
    float bv = 0.f;
    if (!done) {
      const float keep = __fsub_rn(1.0f, a.alpha);
      for (int j = 0; j < k; ++j) {
        const float s = t > 0 ? row_m[j] : 0.f;
        const float v = __fsub_rn(__fmul_rn(keep, expf(a.cand_logp[(size_t)b * k + j])), __fmul_rn(a.alpha, s));
        if (v == v && (best < 0 || v > bv)) best = j, bv = v;
      }
    }
    s_pick = best < 0 ? 0 : best;
  }
  __syncthreads();
  const int pick = s_pick;
  if (tid < k) {
    a.sim[(size_t)b * k + tid] = done ? 0.f : (t > 0 ? row_m[tid] : 0.f);
    a.src_row[(size_t)b * k + tid] = b * k + pick;
  }
  const float* win = ch + (size_t)pick * H;
  for (int e = tid; e < H; e += CS_NT) a.h_next[(size_t)b * H + e] = win[e];
  if (tid == 0) {
    a.chosen[b] = pick;
    if (done) {
      a.token[b] = a.eos, a.logprob[b] = 0.f;
    } else {
      const long long tok = a.cand_tok[(size_t)b * k + pick];
      a.token[b] = tok, a.logprob[b] = a.cand_logp[(size_t)b * k + pick];
      a.length[b] = a.length[b] + 1;
      if (a.eos >= 0 && tok == (long long)a.eos) a.finished[b] = 1;
      if (t < a.Tcap) a.hist_len[b] = t + 1;
    }
  }
  // the chosen candidate behind the row's history, by the rule the append uses (wave 0; every part read hist_len before its ticket)
  if (!done && t < a.Tcap && wave == 0) {
    float* out = a.hist + ((size_t)b * a.Tcap + t) * H;
    const float inv = unit_scale(win, H, lane);
    for (int e = lane; e < H; e += 64) out[e] = unit_of(win[e], inv);
  }
}

int auto_parts(int B, int Tcap) {
  // the host does not know t: from Tcap.  A wave walks its rows one after the other, a row's loads in flight at a time, so the launch
  // is a chain of memory latencies that more waves shorten: a wave should meet one row, the grid stay near 128 workgroups (measured:
  // docs/design/lm_contrastive.md)
  int p = (Tcap + CS_NW - 1) / CS_NW;
  const int room = 128 / B;
  p = p > room ? room : p;
  p = p > VMLMF_CONTRAST_MAX_PARTS ? VMLMF_CONTRAST_MAX_PARTS : p;
  return p < 1 ? 1 : p;
}

int choose_sizes(int B, int k, int H, int Tcap, std::string* why) {
  if (B < 1 || H < 1 || Tcap < 1) return *why = "B, H and Tcap must be >= 1", VMLMF_E_BADARG;
  if (k < 1 || k > CS_MAXK) return *why = "k (candidates) must lie in [1, 16]", VMLMF_E_BADARG;
  if ((long long)k * (long long)((H + 3) & ~3) > VMLMF_CONTRAST_LDS_FLOATS)
    return *why = "k * 4 * ceil(H / 4) must not exceed 14336 floats: the k unit candidates wait in LDS", VMLMF_E_BADARG;
  if ((long long)B * k >= (1ll << 31) || (long long)B * Tcap >= (1ll << 31)) return *why = "B k and B Tcap must stay below 2^31", VMLMF_E_BADARG;
  return 0;
}

template <int KT>
void launch_choose(const ChooseArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)(a.B * a.parts)), block(CS_NT);
  const size_t lds = (size_t)a.k * ((a.H + 3) & ~3) * sizeof(float);
  if (a.H % 4 == 0) hipLaunchKernelGGL((contrast_choose_kernel<KT, 4>), grid, block, lds, stream, a);
  else if (a.H % 2 == 0) hipLaunchKernelGGL((contrast_choose_kernel<KT, 2>), grid, block, lds, stream, a);
  else hipLaunchKernelGGL((contrast_choose_kernel<KT, 1>), grid, block, lds, stream, a);
}

}  // namespace

VMLMF_SIDE_LIBRARY(vmlmf_contrast, VMLMF_CONTRAST_ABI_VERSION)

extern "C" {

size_t vmlmf_contrast_workspace_bytes(int B, int k, int H, int Tcap) {
  std::string why;
  if (choose_sizes(B, k, H, Tcap, &why) != 0) return 0;
  return (size_t)B * VMLMF_CONTRAST_MAX_PARTS * CS_MAXK * sizeof(float);
}

int vmlmf_contrast_append(int B, int T, int H, const float* h, float* hist, int32_t* hist_len, int Tcap, void* stream) {
  const std::string name = "vmlmf_contrast_append: ";
  if (B < 1 || T < 1 || H < 1 || Tcap < 1) return fail(VMLMF_E_BADARG, name + "B, T, H and Tcap must be >= 1");
  if ((long long)B * Tcap >= (1ll << 31) || (long long)B * T >= (1ll << 31))
    return fail(VMLMF_E_BADARG, name + "B Tcap and B T must stay below 2^31");
  if (!h || !hist || !hist_len) return fail(VMLMF_E_BADARG, name + "null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(contrast_append_kernel, dim3((unsigned)(B * T)), dim3(64), 0, s, B, T, H, Tcap, h, hist, hist_len);
  hipLaunchKernelGGL(contrast_advance_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, B, T, Tcap, hist_len);
  return vmlmf_side::launch_tail("vmlmf_contrast_append");
}

int vmlmf_contrast_choose(int B, int k, int H, int Tcap, const float* cand_h, const int64_t* cand_tok, const float* cand_logp, float alpha,
                          int eos, float* hist, int32_t* hist_len, int32_t* finished, int32_t* length, int64_t* token, float* logprob,
                          int32_t* chosen, float* sim, float* h_next, int32_t* src_row, uint32_t* ticket, void* workspace,
                          size_t workspace_bytes, int parts, void* stream) {
  const std::string name = "vmlmf_contrast_choose: ";
  std::string why;
  if (const int rc = choose_sizes(B, k, H, Tcap, &why)) return fail(rc, name + why);
  if (!(alpha >= 0.f && alpha <= 1.f)) return fail(VMLMF_E_BADARG, name + "alpha must lie in [0, 1]");
  if (eos < -1) return fail(VMLMF_E_BADARG, name + "eos must be a token, or -1 for none");
  if (parts < 0 || parts > VMLMF_CONTRAST_MAX_PARTS) return fail(VMLMF_E_BADARG, name + "parts must lie in [0, 64] (0: automatic)");
  if ((long long)B * VMLMF_CONTRAST_MAX_PARTS >= (1ll << 31)) return fail(VMLMF_E_BADARG, name + "B must stay below 2^25");
  if (!cand_h || !cand_tok || !cand_logp || !hist || !hist_len || !finished || !length || !token || !logprob || !chosen || !sim ||
      !h_next || !src_row || !ticket || !workspace)
    return fail(VMLMF_E_BADARG, name + "null pointer");
  if (((uintptr_t)hist & 15u) != 0) return fail(VMLMF_E_BADARG, name + "hist must be 16-byte aligned");
  if (((uintptr_t)workspace & 3u) != 0) return fail(VMLMF_E_BADARG, name + "the workspace must be 4-byte aligned");
  if (workspace_bytes < vmlmf_contrast_workspace_bytes(B, k, H, Tcap))
    return fail(VMLMF_E_WORKSPACE, name + "workspace smaller than vmlmf_contrast_workspace_bytes(B, k, H, Tcap)");
  ChooseArgs a;
  a.B = B, a.k = k, a.H = H, a.Tcap = Tcap, a.eos = eos, a.alpha = alpha;
  a.parts = parts > 0 ? parts : auto_parts(B, Tcap);
  a.cand_h = cand_h, a.cand_logp = cand_logp, a.cand_tok = reinterpret_cast<const long long*>(cand_tok);
  a.hist = hist, a.logprob = logprob, a.sim = sim, a.h_next = h_next, a.part_max = static_cast<float*>(workspace);
  a.hist_len = hist_len, a.finished = finished, a.length = length, a.chosen = chosen, a.src_row = src_row;
  a.token = reinterpret_cast<long long*>(token), a.ticket = ticket;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (k == 1) launch_choose<1>(a, s);
  else if (k == 2) launch_choose<2>(a, s);
  else if (k <= 4) launch_choose<4>(a, s);
  else if (k <= 8) launch_choose<8>(a, s);
  else launch_choose<16>(a, s);
  return vmlmf_side::launch_tail("vmlmf_contrast_choose");
}

}  // extern "C"
