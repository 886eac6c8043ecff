// Scoring under a continuous cache (Model.cache_score): libvmlmf_ncache.so, a library of its own (include/vmlmf_ncache.h has the
// contract), built by the Makefile's `further`.  One kernel, ONE launch over B x ceil(T / 16) x parts workgroups of four waves:
//   1. the key tiles.  A workgroup leaves its tile of 16 queries in LDS (rows padded with zeros to a multiple of 16 floats, 8 floats
//      of stride on top against bank conflicts).  Each wave then takes tiles of 16 keys of the union of the tile's bands: lane l holds
//      key row l & 15 and query row l & 15, the pieces (l >> 4) of every step over H - 16-, 8- or 4-byte pieces by H's divisibility,
//      a batch of them in flight -, and v_mfma_f32_16x16x4_f32 forms the 16 x 16 dot products in exact fp32, two accumulators
//      alternating.  With the scores in registers the wave masks each query's band, and per query a butterfly over the 16 columns
//      gives the tile's maximum, its sum of expf against that maximum and the sum over the matching pairs: three numbers per query
//      and key tile go to the workspace, the scores themselves never leave the registers.
//   2. the ticket (csrc/vmlmf_contrast.hip's protocol): the last workgroup of a query tile to arrive goes on, the others are done.
//   3. the merge.  16 lanes per query: the exact maximum over the band's key tiles, then the tiles' sums scaled to it, in tile
//      order, logf, the mixture.
// Every output is the same bits for every `parts`: the key tiles are the units of the sums, the parts only decide who computes which.
// docs/design/lm_ncache.md has the budget, the error bound, the numbers and the form this replaced (all scores through the workspace).
// Plain HIP C++ for wave64, no inline assembly.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/vmlmf_ncache.h"
#include "vmlmf_side.h"

namespace {

constexpr int NC_NT = 256;           // threads of a workgroup: four waves share one copy of the query tile
constexpr int NC_NW = NC_NT / 64;
constexpr int NC_Q = 16;             // queries of a tile, keys of a key tile: the MFMA's 16 x 16
constexpr int NC_PAD = 8;            // floats between the LDS rows of two queries on top of the padded H

using vmlmf_side::fail;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct ScoreArgs {
  int B, T, n, H, window, parts, QT, Wp, S;   // QT query tiles per row; Wp / 16 key tiles per query tile at most; S floats of an LDS row
  float theta, lam, log_keep, log_lam;        // log1p(-lam), log(lam)
  const float *keys, *lv;
  const long long* tok;
  float *logp, *lc, *ws;
  unsigned* ticket;
};

template <int VW>
struct Piece;
template <>
struct Piece<4> {
  typedef float4 type;
  static __device__ __forceinline__ float4 zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  static __device__ __forceinline__ float at(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
};
template <>
struct Piece<2> {
  typedef float2 type;
  static __device__ __forceinline__ float2 zero() { return make_float2(0.f, 0.f); }
  static __device__ __forceinline__ float at(const float2& v, int e) { return e == 0 ? v.x : v.y; }
};
template <>
struct Piece<1> {
  typedef float type;
  static __device__ __forceinline__ float zero() { return 0.f; }
  static __device__ __forceinline__ float at(const float& v, int) { return v; }
};

// an exact maximum that a NaN wins whatever the order (-inf is its neutral element)
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || b != b) ? NAN : fmaxf(a, b); }

// VW: floats per piece (VW divides H: the host chose it so)
template <int VW>
__global__ __launch_bounds__(NC_NT) void ncache_score_kernel(ScoreArgs a) {
  typedef typename Piece<VW>::type piece_t;
  constexpr int U = VW == 4 ? 8 : 16;   // a lane's pieces of one key row in flight (twice as many measured slower: the loads are
                                        // bound by the 16 rows every one of them touches, not by latency)
  constexpr int HS = 4 * VW;            // floats of H one step covers: four lanes' pieces per row
  constexpr int QU = 4;                 // a lane's pieces of one query row in flight while the tile is staged
  constexpr int MU = 4;                 // a lane's key tiles in flight in the merge
  extern __shared__ float4 nc_lds4[];   // (16, S) the query tile
  float* q = reinterpret_cast<float*>(nc_lds4);
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P = a.parts, H = a.H, L = a.n + a.T;
  const int part = blockIdx.x % P, tile = blockIdx.x / P, qt = tile % a.QT, b = tile / a.QT;
  const int q0 = qt * NC_Q, qlast = q0 + NC_Q - 1 < a.T ? q0 + NC_Q - 1 : a.T - 1;
  // the union of the tile's bands: keys [jlo, jhi) of the row, in tiles of 16 from jlo
  const int jlo = a.n + q0 - a.window > 0 ? a.n + q0 - a.window : 0, jhi = a.n + qlast;
  const int KT = (jhi - jlo + NC_Q - 1) / NC_Q;
  const float* kb = a.keys + (size_t)b * L * H;
  float* ws = a.ws + (size_t)tile * 3 * a.Wp;   // (Wp / 16 key tiles) x (max, sum, matching sum) x 16 queries

  // ---- 1. this part's key tiles: part NW + wave, then every P NW-th
  const long long* tk = a.tok + (size_t)b * L;
  if (part * NC_NW < KT) {   // (uniform over the workgroup)
    {   // the query tile: a wave takes four rows, piece by piece, the four rows' loads of a pass in flight together
      const int np = a.S / VW, hp = H / VW;
      piece_t* q4 = reinterpret_cast<piece_t*>(q);
      for (int p0 = lane; p0 < np; p0 += 64 * QU) {
        piece_t v[NC_Q / NC_NW][QU];
#pragma unroll
        for (int r = 0; r < NC_Q / NC_NW; ++r) {
          const int i = wave + NC_NW * r;
          const bool live = q0 + i < a.T;
          const piece_t* x = reinterpret_cast<const piece_t*>(kb + (size_t)(a.n + (live ? q0 + i : qlast)) * H);
#pragma unroll
          for (int u = 0; u < QU; ++u) {
            const int p = p0 + 64 * u;
            v[r][u] = x[p < hp ? p : 0];
            if (!(live && p < hp)) v[r][u] = Piece<VW>::zero();
          }
        }
#pragma unroll
        for (int r = 0; r < NC_Q / NC_NW; ++r)
#pragma unroll
          for (int u = 0; u < QU; ++u)
            if (p0 + 64 * u < np) q4[(wave + NC_NW * r) * np + p0 + 64 * u] = v[r][u];
      }
    }
    __syncthreads();
    const int col = lane & 15, kl = lane >> 4;
    const int nsteps = (H + HS - 1) / HS;
    const float* qrow = q + col * a.S + kl * VW;
    // the four queries this lane holds results of: 4 (l >> 4) + r; their targets and the lower ends of their bands
    long long y[4];
    int lo[4], hi[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t = q0 + kl * 4 + r;
      y[r] = tk[a.n + (t < a.T ? t : qlast)];
      hi[r] = t < a.T ? a.n + t : 0;   // band [lo, hi): empty for a query beyond T
      lo[r] = hi[r] - a.window > 0 ? hi[r] - a.window : 0;
    }
    for (int c = part * NC_NW + wave; c < KT; c += P * NC_NW) {
      const int jj = jlo + c * NC_Q + col;
      const int j = jj < jhi ? jj : jhi - 1;   // a column beyond the union repeats its last key and is in nobody's band
      const float* krow = kb + (size_t)j * H;
      const long long w = tk[j];
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      for (int s0 = 0; s0 < nsteps; s0 += U) {
        piece_t kv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int h = (s0 + u) * HS + kl * VW;   // this lane's piece: whole inside H, or whole outside (then the row's first)
          const bool in = h < H;
          kv[u] = *reinterpret_cast<const piece_t*>(krow + (in ? h : 0));
          if (!in) kv[u] = Piece<VW>::zero();
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (s0 + u < nsteps) {   // (uniform)
            const piece_t qv = *reinterpret_cast<const piece_t*>(qrow + (s0 + u) * HS);
#pragma unroll
            for (int e = 0; e < VW; ++e) {
              if (e & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(Piece<VW>::at(qv, e), Piece<VW>::at(kv[u], e), acc1, 0, 0, 0);
              else acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(Piece<VW>::at(qv, e), Piece<VW>::at(kv[u], e), acc0, 0, 0, 0);
            }
          }
        }
      }
      // D: lane l holds the queries 4 (l >> 4) + r of key column l & 15.  Per query the tile's (max, sum, matching sum) over the
      // columns in its band: butterflies over the 16 lanes of a query's row
      float* out = ws + (size_t)c * 3 * NC_Q + kl * 4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool in = jj >= lo[r] && jj < hi[r];
        const float s = in ? __fmul_rn(a.theta, __fadd_rn(acc0[r], acc1[r])) : -INFINITY;
        float mx = s;
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) mx = nan_max(mx, __shfl_xor(mx, d, 16));
        const float e = in ? expf(__fsub_rn(s, mx)) : 0.f;
        float z = e, nn = (in && w == y[r]) ? e : 0.f;   // the same values in the same order into both sums
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) {
          z = __fadd_rn(z, __shfl_xor(z, d, 16));
          nn = __fadd_rn(nn, __shfl_xor(nn, d, 16));
        }
        if (col == 0) out[r] = mx, out[NC_Q + r] = z, out[2 * NC_Q + r] = nn;
      }
    }
  }
  __syncthreads();   // orders the stores above before thread 0's release (and before this workgroup's own reads where P == 1)

  // ---- 2. the ticket
  if (P > 1) {
    if (tid == 0) {
      const unsigned got = __hip_atomic_fetch_add(a.ticket + tile, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
      s_last = got == (unsigned)P - 1u;
    }
    __syncthreads();
    if (!s_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // last arrival of the tile: acquire in every wave
    if (tid == 0) __hip_atomic_store(a.ticket + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }

  // ---- 3. the key tiles of a query's band, merged in tile order: 16 lanes per query (a group of 16 lanes shares every branch below)
  const int i = tid >> 4, sub = tid & 15, t = q0 + i;
  if (t >= a.T) return;
  const int jr = a.n + t, jl = jr - a.window > 0 ? jr - a.window : 0, m = jr - jl;
  const size_t o = (size_t)t * a.B + b;
  const float lv = a.lv[o];
  if (m == 0) {   // an empty cache: the vocabulary's bits
    if (sub == 0) a.logp[o] = lv, a.lc[o] = -INFINITY;
    return;
  }
  const int c0 = (jl - jlo) / NC_Q, c1 = (jr - 1 - jlo) / NC_Q + 1;   // the key tiles [c0, c1) meet the band
  const float* mine = ws + i;
  float M = -INFINITY;
  for (int c = c0 + sub; c < c1; c += 16 * MU) {
    float v[MU];
#pragma unroll
    for (int u = 0; u < MU; ++u) v[u] = c + 16 * u < c1 ? mine[(size_t)(c + 16 * u) * 3 * NC_Q] : -INFINITY;
#pragma unroll
    for (int u = 0; u < MU; ++u) M = nan_max(M, v[u]);
  }
#pragma unroll
  for (int d = 8; d >= 1; d >>= 1) M = nan_max(M, __shfl_xor(M, d, 16));
  float z = 0.f, nn = 0.f;
  for (int c = c0 + sub; c < c1; c += 16 * MU) {
    float vm[MU], vz[MU], vn[MU];
#pragma unroll
    for (int u = 0; u < MU; ++u) {
      const bool in = c + 16 * u < c1;
      const float* at = mine + (size_t)(in ? c + 16 * u : c0) * 3 * NC_Q;
      vm[u] = in ? at[0] : -INFINITY, vz[u] = in ? at[NC_Q] : 0.f, vn[u] = in ? at[2 * NC_Q] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < MU; ++u) {   // the same factors in the same order into both sums
      const float f = expf(__fsub_rn(vm[u], M));
      z = __fadd_rn(z, __fmul_rn(vz[u], f));
      nn = __fadd_rn(nn, __fmul_rn(vn[u], f));
    }
  }
#pragma unroll
  for (int d = 8; d >= 1; d >>= 1) {
    z = __fadd_rn(z, __shfl_xor(z, d, 16));
    nn = __fadd_rn(nn, __shfl_xor(nn, d, 16));
  }
  if (sub != 0) return;
  const float lc = __fsub_rn(logf(nn), logf(z));   // N == 0: -inf; N == Z: 0.0
  float out;
  const float keep = __fadd_rn(a.log_keep, lv);
  if (a.lam == 0.f) out = lv;
  else if (nn == 0.f || keep != keep) out = keep;
  else {
    const float hit = __fadd_rn(a.log_lam, lc);
    const float hi = fmaxf(keep, hit), lo = fminf(keep, hit);
    out = hit != hit ? hit : __fadd_rn(hi, log1pf(expf(__fsub_rn(lo, hi))));
  }
  a.logp[o] = out, a.lc[o] = lc;
}

long long row_width(int T, int n, int window) {   // keys of the widest union of a query tile's bands, in whole key tiles
  const long long L = (long long)n + T, w = (long long)window + NC_Q - 1;
  return ((w < L ? w : L) + NC_Q - 1) / NC_Q * NC_Q;
}

int score_sizes(int B, int T, int n, int H, int window, std::string* why) {
  if (B < 1 || T < 1 || H < 1 || window < 1) return *why = "B, T, H and window must be >= 1", VMLMF_E_BADARG;
  if (n < 0) return *why = "n (carried pairs) must be >= 0", VMLMF_E_BADARG;
  if (H > VMLMF_NCACHE_MAX_H) return *why = "H must not exceed 2048: a tile of 16 queries waits in LDS", VMLMF_E_BADARG;
  if ((long long)B * ((long long)n + T) >= (1ll << 31)) return *why = "B (n + T) must stay below 2^31", VMLMF_E_BADARG;
  if ((long long)B * ((T + NC_Q - 1) / NC_Q) >= (1ll << 25)) return *why = "B ceil(T / 16) must stay below 2^25", VMLMF_E_BADARG;
  return 0;
}

int auto_parts(int B, int T, int n, int window) {
  // a key tile is a chain of memory latencies that more waves shorten, so a wave should meet one key tile; but every workgroup stages
  // the query tile again, so the grid stays near 512 workgroups (measured: docs/design/lm_ncache.md)
  const int QT = (T + NC_Q - 1) / NC_Q;
  const long long KT = row_width(T, n, window) / NC_Q;
  long long p = (KT + NC_NW - 1) / NC_NW;
  const long long room = 512 / ((long long)B * QT);
  p = p > room ? room : p;
  p = p > VMLMF_NCACHE_MAX_PARTS ? VMLMF_NCACHE_MAX_PARTS : p;
  return p < 1 ? 1 : (int)p;
}

template <int VW>
int launch_score(const ScoreArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)(a.B * a.QT * a.parts)), block(NC_NT);
  const size_t lds = (size_t)NC_Q * a.S * sizeof(float);
  if (lds + 1024 > 64 * 1024) {   // beyond the default limit of a launch's dynamic LDS
    const hipError_t rc = hipFuncSetAttribute(reinterpret_cast<const void*>(&ncache_score_kernel<VW>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (rc != hipSuccess) return fail((int)rc, std::string("vmlmf_ncache_score: dynamic LDS limit: ") + hipGetErrorString(rc));
  }
  hipLaunchKernelGGL((ncache_score_kernel<VW>), grid, block, lds, stream, a);
  return vmlmf_side::launch_tail("vmlmf_ncache_score");
}

}  // namespace

VMLMF_SIDE_LIBRARY(vmlmf_ncache, VMLMF_NCACHE_ABI_VERSION)

extern "C" {

size_t vmlmf_ncache_workspace_bytes(int B, int T, int n, int H, int window) {
  std::string why;
  if (score_sizes(B, T, n, H, window, &why) != 0) return 0;
  return (size_t)B * ((T + NC_Q - 1) / NC_Q) * 3 * (size_t)row_width(T, n, window) * sizeof(float);
}

int vmlmf_ncache_score(int B, int T, int n, int H, int window, float theta, float lam, const float* keys, const int64_t* key_tok,
                       const float* vocab_logp, float* logp, float* cache_logp, uint32_t* ticket, void* workspace, size_t workspace_bytes,
                       int parts, void* stream) {
  const std::string name = "vmlmf_ncache_score: ";
  std::string why;
  if (const int rc = score_sizes(B, T, n, H, window, &why)) return fail(rc, name + why);
  if (!(theta - theta == 0.f)) return fail(VMLMF_E_BADARG, name + "theta must be finite");
  if (!(lam >= 0.f && lam < 1.f)) return fail(VMLMF_E_BADARG, name + "lam must lie in [0, 1)");
  if (parts < 0 || parts > VMLMF_NCACHE_MAX_PARTS) return fail(VMLMF_E_BADARG, name + "parts must lie in [0, 64] (0: automatic)");
  if (!keys || !key_tok || !vocab_logp || !logp || !cache_logp || !ticket || !workspace) return fail(VMLMF_E_BADARG, name + "null pointer");
  if (((uintptr_t)keys & 15u) != 0) return fail(VMLMF_E_BADARG, name + "keys must be 16-byte aligned");
  if (((uintptr_t)workspace & 3u) != 0) return fail(VMLMF_E_BADARG, name + "the workspace must be 4-byte aligned");
  if (workspace_bytes < vmlmf_ncache_workspace_bytes(B, T, n, H, window))
    return fail(VMLMF_E_WORKSPACE, name + "workspace smaller than vmlmf_ncache_workspace_bytes(B, T, n, H, window)");
  ScoreArgs a;
  a.B = B, a.T = T, a.n = n, a.H = H, a.window = window;
  a.parts = parts > 0 ? parts : auto_parts(B, T, n, window);
  a.QT = (T + NC_Q - 1) / NC_Q, a.Wp = (int)row_width(T, n, window), a.S = (H + 15) / 16 * 16 + NC_PAD;
  a.theta = theta, a.lam = lam, a.log_keep = (float)log1p(-(double)lam), a.log_lam = lam > 0.f ? (float)log((double)lam) : -INFINITY;
  a.keys = keys, a.lv = vocab_logp, a.tok = reinterpret_cast<const long long*>(key_tok);
  a.logp = logp, a.lc = cache_logp, a.ws = static_cast<float*>(workspace), a.ticket = ticket;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (H % 4 == 0) return launch_score<4>(a, s);
  if (H % 2 == 0) return launch_score<2>(a, s);
  return launch_score<1>(a, s);
}

}  // extern "C"
