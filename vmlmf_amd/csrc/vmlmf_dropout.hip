// Dropout launches of the LM network for the places no layer kernel covers (vmlmf_dropout.h has the scheme): the generator's
// per-forward snapshot, the embedding gather with its dropout in the same pass (vmlmf_lm.py:434-435), the stand-alone form for
// activations of layers whose kernels do not take DropArgs (y = x * factor: the forward and, with the same snapshot, the backward),
// the factors themselves for the parity tests (what a fused kernel applied, as a tensor an oracle can multiply by), and the top
// layer's dropout together with the activation regularisers that need its raw output (AR / TAR: the second half of this file).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vmlmf_dropout.h"
#include "vmlmf_launch.h"

namespace {

__global__ void drop_advance_kernel(unsigned long long* state, unsigned long long* snap) {
  const unsigned long long seed = state[0], off = state[1];
  snap[0] = seed, snap[1] = off;
  state[1] = off + 1ull;
}

// the factor of one column on a layer's map (group layers: a call per column; kept out of line, the library is held to a size)
__device__ __noinline__ float mapped_factor(const DropKey k, const unsigned thresh, const float scale, const DropCols cm, const unsigned r, const int n) {
  const int col = (n / cm.Hg) * cm.gstride + n % cm.Hg;
  float w[4];
  drop_factors(k, thresh, scale, r, (unsigned)(col >> 2), w);
  return w[col & 3];
}
// the factors of columns n0 .. n0 + 3 at position r: one call on the identity map, a call per column on a layer's map
__device__ __forceinline__ void quad_factors(const DropKey& k, const DropArgs& d, const DropCols& cm, const unsigned r, const int n0, const int H,
                                             float (&f)[4]) {
  if (cm.gstride == 0 || cm.Hg >= H) {
    drop_factors(k, d.thresh, d.scale, r, (unsigned)(n0 >> 2), f);
    return;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) f[e] = mapped_factor(k, d.thresh, d.scale, cm, r, n0 + e < H ? n0 + e : H - 1);
}

// One thread per four columns of a position; mode 0: y = x * factor, mode 1: y = factor, mode 2: y = w[tokens[position]] * factor
// (a uniform branch of one kernel: the library is held to a size).
// Under a locked mask (d.period == B; docs/design/lm_locked.md) a thread keeps its (batch row, four columns) for DR_TC time steps
// and draws once: the factors do not depend on t.  Per element (d.period == 0) the walk is one position long.
constexpr int DR_TC = 4;
__host__ __device__ inline long long drop_rows_threads(long long R, int quads, int period) {
  return period != 0 ? (long long)period * ((R / period + DR_TC - 1) / DR_TC) * quads : R * quads;
}
// one position's four columns: y = x * f / f / w[token] * f
__device__ __forceinline__ void drop_row(const int MODE, const long long r, const int n0, const int H, const int V, const float (&f)[4],
                                         const float* __restrict__ x, const long long* __restrict__ tokens, float* __restrict__ y) {
  const float* src = x;
  if (MODE == 2) {
    long long t = tokens[r];
    t = t < 0 ? 0 : (t >= V ? V - 1 : t);   // (the stock gather faults on such a token; here it reads a valid row)
    src = x + (size_t)t * H;
  } else if (MODE == 0) {
    src = x + (size_t)r * H;
  }
  float* dst = y + (size_t)r * H;
  if ((H & 3) == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {   // 16-byte accesses where the rows allow them
    float4 v = make_float4(1.f, 1.f, 1.f, 1.f);
    if (MODE != 1) v = *reinterpret_cast<const float4*>(src + n0);
    *reinterpret_cast<float4*>(dst + n0) = make_float4(v.x * f[0], v.y * f[1], v.z * f[2], v.w * f[3]);
  } else {   // (H = 650 of the PTB network: rows start 8 bytes off)
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (MODE != 1 && n0 + e < H) ? src[n0 + e] : 1.f;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (n0 + e < H) dst[n0 + e] = v[e] * f[e];
  }
}
__global__ void __launch_bounds__(256) drop_rows_kernel(const int MODE, long long R, int H, int V, DropArgs d, DropCols cm, const float* __restrict__ x,
                                                        const long long* __restrict__ tokens, float* __restrict__ y) {
  const int quads = (H + 3) >> 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  float f[4];   // (a layer's map - what a row-block layer's kernels apply, as a tensor -: a call per column)
  if (d.period == 0) {   // per element: the thread's one position, straight through (the path every release had)
    if (i >= R * quads) return;
    const long long r = i / quads;
    const int n0 = (int)(i - r * quads) * 4;
    quad_factors(drop_key(d), d, cm, drop_position(0, (unsigned)r), n0, H, f);
    drop_row(MODE, r, n0, H, V, f, x, tokens, y);
    return;
  }
  if (i >= drop_rows_threads(R, quads, d.period)) return;
  long long r = i / quads;   // = chunk B + b (below 2^32: the host refuses more positions): the chunk's first position of row b
  const int n0 = (int)(i - r * quads) * 4;
  r += (long long)((unsigned)r / (unsigned)d.period) * (DR_TC - 1) * d.period;
  long long rend = r + (long long)DR_TC * d.period;
  if (rend > R) rend = R;
  quad_factors(drop_key(d), d, cm, drop_position(d.period, (unsigned)r), n0, H, f);
  for (; r < rend; r += d.period) drop_row(MODE, r, n0, H, V, f, x, tokens, y);
}

// The gather under word dropout (vmlmf_embed_dropout_forward_ex; docs/design/lm_tied.md): out[r] = (w[tok_r] * fw[tok_r]) * f[r] -
// AWD-LSTM's masked table, then the input dropout: two single-rounded multiplications in that order, each skipped where its
// probability is 0 (uniform branches of the one instantiation).  A thread owns four columns of a position as above; a dropped
// word's quad is written as zeros without reading the table.  Accesses choose their width per address.
__global__ void __launch_bounds__(256) embed_fwd_ex_kernel(int R, int H, int V, DropArgs d, WordDrop wd, const float* __restrict__ w,
                                                           const long long* __restrict__ tokens, float* __restrict__ y) {
  const int quads = (H + 3) >> 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)R * quads) return;
  const int r = (int)(i / quads);
  const int n0 = (int)(i - (long long)r * quads) * 4;
  const int valid = H - n0 < 4 ? H - n0 : 4;
  long long t = tokens[r];
  t = t < 0 ? 0 : (t >= V ? V - 1 : t);   // (as drop_rows_kernel: a valid row for a token the stock gather faults on)
  float* dst = y + (size_t)r * H + n0;
  float x[4] = {0.f, 0.f, 0.f, 0.f};
  float fw = 1.f;
  if (wd.word) fw = word_factor(d.state, wd.thresh, wd.scale, (unsigned)t);
  if (fw != 0.f) {
    load_quad(w + (size_t)t * H + n0, valid, x);
    if (wd.word) {
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] = __fmul_rn(x[e], fw);
    }
    if (wd.drop) {
      float f[4];
      drop_factors(drop_key(d), d.thresh, d.scale, drop_position(d.period, (unsigned)r), (unsigned)(n0 >> 2), f);
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] = __fmul_rn(x[e], f[e]);
    }
  }
  store_quad(dst, valid, x);
}

// ---- activation regularisation of the top layer (AR / TAR; include/vmlmf_hip.h: vmlmf_actreg_forward; docs/design/lm_actreg.md) ----
// A thread owns four neighbouring columns of one batch row and walks AR_TC time steps with them: grid (ceil(B quads / 256), ceil(T /
// AR_TC)).  It loads its AR_TC rows and the halo a difference over time needs (forward: the row behind the block; backward: the rows on
// both sides) up front - at (35, 32, 650) the tensor is 2.9 MB and a launch is a few microseconds of latency, not of bandwidth, so the
// loads of a thread are all in flight at once and the grid has 21 x 9 workgroups rather than 21 long-running ones (measured: 4 steps
// per thread 20.8 us for the pair there, 8 steps 27.0 us; at (70, 256, 650) 86 against 78 us: docs/design/lm_actreg.md).  The dropout
// factors are drop_rows_kernel's: one Philox call per (position, four columns) on the identity map.
// Every fp32 operation below is written as a single rounded one (__fmul_rn, __fadd_rn, ...: no contraction into fused multiply-adds),
// in the order docs/design/lm_actreg.md counts; tests/actreg_cases.py restates both kernels in numpy's float32.
constexpr int AR_TC = 4;

// the workgroup's sums of a and b, left in thread 0: a wave's shuffle tree (lane l takes lane l + 32, + 16, ... + 1), then the four
// waves in order - the same order every time
__device__ __forceinline__ void block_sum2(float& a, float& b, float (*red)[2]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a = __fadd_rn(a, __shfl_down(a, o, 64)), b = __fadd_rn(b, __shfl_down(b, o, 64));
  const int tid = threadIdx.x;
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6][0] = a, red[tid >> 6][1] = b;
  __syncthreads();
  if (tid == 0)
    for (int w = 1; w < 4; ++w) a = __fadd_rn(a, red[w][0]), b = __fadd_rn(b, red[w][1]);
}
// the thread's batch row, first column, number of columns and the row's valid length; false: a thread behind the last quad
__device__ __forceinline__ bool actreg_place(const ActRegArgs& a, int& b, int& n0, int& valid, int& len) {
  const int quads = (a.H + 3) >> 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)a.B * quads) return false;
  b = (int)(i / quads);
  n0 = (int)(i - (long long)b * quads) * 4;
  valid = a.H - n0 < 4 ? a.H - n0 : 4;
  len = a.T;
  if (a.lengths != nullptr) {
    const long long l = a.lengths[b];
    len = l < 0 ? 0 : (l > a.T ? a.T : (int)l);
  }
  return true;
}

__global__ void __launch_bounds__(256) actreg_fwd_kernel(const ActRegArgs a) {
  const bool DROP = a.d.state != nullptr;   // (one kernel for both: the library is held to a size, and the branch is uniform)
  __shared__ float red[4][2];
  __shared__ unsigned long long count[2];
  __shared__ int last;
  const int tid = threadIdx.x, t0 = blockIdx.y * AR_TC;
  const bool ar_on = a.ar > 0.f, tar_on = a.tar > 0.f;
  float s_ar = 0.f, s_tar = 0.f;
  int b, n0, valid, len;
  if (actreg_place(a, b, n0, valid, len)) {
    float v[AR_TC + 1][4];   // rows t0 .. t0 + AR_TC: the last one is the halo of the pair (t0 + AR_TC - 1, t0 + AR_TC)
#pragma unroll
    for (int j = 0; j <= AR_TC; ++j) {
      const int t = t0 + j;
      if (j < AR_TC ? t < a.T : (tar_on && t < len)) {
        load_quad(a.raw + ((size_t)t * a.B + b) * a.H + n0, valid, v[j]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[j][e] = 0.f;
      }
    }
    DropKey k = {0u, 0u, 0u, 0u};
    if (DROP) k = drop_key(a.d);
    float f[4];   // under a locked mask (a.d.period == B) drawn at the walk's first step (t0 < T always) and kept: one call per thread
#pragma unroll
    for (int j = 0; j < AR_TC; ++j) {
      const int t = t0 + j;
      if (t < a.T) {
        float y[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = v[j][e];
        if (DROP) {
          if (j == 0 || a.d.period == 0) quad_factors(k, a.d, a.cm, drop_position(drop_tstride(a.d.period, a.B), t, b), n0, a.H, f);
#pragma unroll
          for (int e = 0; e < 4; ++e) y[e] = __fmul_rn(v[j][e], f[e]);
          store_quad(a.d.yd + ((size_t)t * a.B + b) * a.H + n0, valid, y);
        }
        if (ar_on && t < len) {
#pragma unroll
          for (int e = 0; e < 4; ++e) s_ar = __fadd_rn(s_ar, __fmul_rn(y[e], y[e]));
        }
        if (tar_on && t + 1 < len) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float dt = __fsub_rn(v[j + 1][e], v[j][e]);
            s_tar = __fadd_rn(s_tar, __fmul_rn(dt, dt));
          }
        }
      }
    }
  }
  block_sum2(s_ar, s_tar, red);
  // The workgroup's pair goes out as ONE 8-byte word, written through to agent scope by the lane that then - its store counted - takes
  // the ticket; the workgroup that draws the last ticket reads every pair past its L1 and finishes.  Nobody waits for anybody.
  const unsigned nwg = gridDim.x * gridDim.y, wg = blockIdx.y * gridDim.x + blockIdx.x;
  if (tid == 0) {
    const unsigned long long word = ((unsigned long long)__float_as_uint(s_tar) << 32) | __float_as_uint(s_ar);
    __hip_atomic_store(a.part + wg, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned long long t = __hip_atomic_fetch_add(a.ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = t == (unsigned long long)nwg - 1ull;
    count[0] = count[1] = 0ull;
  }
  __syncthreads();
  if (!last) return;
  s_ar = s_tar = 0.f;
  for (unsigned w = tid; w < nwg; w += 256) {   // a thread's pairs in ascending order, then the workgroup's tree
    const unsigned long long word = __hip_atomic_load(a.part + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_ar = __fadd_rn(s_ar, __uint_as_float((unsigned)word)), s_tar = __fadd_rn(s_tar, __uint_as_float((unsigned)(word >> 32)));
  }
  // the valid positions and pairs, from the lengths (integers: their order does not matter)
  unsigned long long c_ar = 0ull, c_tar = 0ull;
  if (a.lengths != nullptr) {
    for (int r = tid; r < a.B; r += 256) {
      const long long l = a.lengths[r];
      const unsigned long long n = l < 0 ? 0ull : (l > a.T ? (unsigned long long)a.T : (unsigned long long)l);
      c_ar += n, c_tar += n > 0ull ? n - 1ull : 0ull;
    }
    if (c_ar != 0ull) atomicAdd(&count[0], c_ar);
    if (c_tar != 0ull) atomicAdd(&count[1], c_tar);
  }
  block_sum2(s_ar, s_tar, red);   // (its barriers order the counts too)
  if (tid != 0) return;
  if (a.lengths == nullptr) count[0] = (unsigned long long)a.T * a.B, count[1] = (unsigned long long)(a.T - 1) * a.B;
  const unsigned long long n_ar = count[0] * (unsigned long long)a.H, n_tar = count[1] * (unsigned long long)a.H;
  const float f_ar = (float)(n_ar > 0ull ? n_ar : 1ull), f_tar = (float)(n_tar > 0ull ? n_tar : 1ull);
  float p_ar = 0.f, p_tar = 0.f, c0 = 0.f, c1 = 0.f;
  if (ar_on) p_ar = __fmul_rn(a.batch_scale, __fdiv_rn(s_ar, f_ar)), c0 = __fdiv_rn(__fmul_rn(2.f * a.ar, a.batch_scale), f_ar);
  if (tar_on) p_tar = __fmul_rn(a.batch_scale, __fdiv_rn(s_tar, f_tar)), c1 = __fdiv_rn(__fmul_rn(2.f * a.tar, a.batch_scale), f_tar);
  a.stats[0] = __fadd_rn(__fmul_rn(a.ar, p_ar), __fmul_rn(a.tar, p_tar));
  a.stats[1] = p_ar, a.stats[2] = p_tar, a.stats[3] = c0, a.stats[4] = c1;
  a.stats[5] = (float)n_ar, a.stats[6] = (float)n_tar, a.stats[7] = 0.f;
  __hip_atomic_store(a.ticket, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(256) actreg_bwd_kernel(const ActRegArgs a) {
  const bool DROP = a.d.state != nullptr;
  const int t0 = blockIdx.y * AR_TC;
  const bool ar_on = a.ar > 0.f, tar_on = a.tar > 0.f;
  int b, n0, valid, len;
  if (!actreg_place(a, b, n0, valid, len)) return;
  float c_ar = a.stats[3], c_tar = a.stats[4];
  if (a.dpenalty != nullptr) {   // an upstream gradient of the penalty other than one
    const float s = a.dpenalty[0];
    c_ar = __fmul_rn(s, c_ar), c_tar = __fmul_rn(s, c_tar);
  }
  float v[AR_TC + 2][4], g[AR_TC][4];   // raw: rows t0 - 1 .. t0 + AR_TC, read only where a valid position needs them
#pragma unroll
  for (int j = 0; j < AR_TC + 2; ++j) {
    const int t = t0 - 1 + j;
    const bool centre = j >= 1 && j <= AR_TC;
    if (t >= 0 && t < len && (centre ? (ar_on || tar_on) : (tar_on && t0 < len))) {
      load_quad(a.raw + ((size_t)t * a.B + b) * a.H + n0, valid, v[j]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[j][e] = 0.f;
    }
  }
#pragma unroll
  for (int j = 0; j < AR_TC; ++j) {
    const int t = t0 + j;
    if (t < a.T) {
      load_quad(a.g + ((size_t)t * a.B + b) * a.H + n0, valid, g[j]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) g[j][e] = 0.f;
    }
  }
  DropKey k = {0u, 0u, 0u, 0u};
  if (DROP) k = drop_key(a.d);
  float f[4] = {1.f, 1.f, 1.f, 1.f};   // (locked: the first step's call serves the walk, as in the forward)
#pragma unroll
  for (int j = 0; j < AR_TC; ++j) {
    const int t = t0 + j;
    if (t >= a.T) continue;
    if (DROP && (j == 0 || a.d.period == 0)) quad_factors(k, a.d, a.cm, drop_position(drop_tstride(a.d.period, a.B), t, b), n0, a.H, f);
    const bool live = t < len, prev = live && t >= 1, next = t + 1 < len;
    float out[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float x = v[j + 1][e];
      float u = g[j][e];
      if (ar_on && live) u = __fadd_rn(u, __fmul_rn(c_ar, DROP ? __fmul_rn(x, f[e]) : x));
      if (DROP) u = __fmul_rn(f[e], u);
      if (tar_on && (prev || next)) {
        const float dt = __fsub_rn(x, v[j][e]), dn = __fsub_rn(v[j + 2][e], x);
        const float d = prev ? (next ? __fsub_rn(dt, dn) : dt) : -dn;
        u = __fadd_rn(u, __fmul_rn(c_tar, d));
      }
      out[e] = u;
    }
    store_quad(a.draw + ((size_t)t * a.B + b) * a.H + n0, valid, out);
  }
}

}  // namespace

long long actreg_workgroups(int T, int B, int H) {
  return (((long long)B * ((H + 3) / 4) + 255) / 256) * ((T + AR_TC - 1) / AR_TC);
}

static dim3 actreg_grid(const ActRegArgs& a) {
  return dim3((unsigned)(((long long)a.B * ((a.H + 3) / 4) + 255) / 256), (unsigned)((a.T + AR_TC - 1) / AR_TC));
}

int launch_actreg_fwd(const ActRegArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(actreg_fwd_kernel, actreg_grid(a), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

int launch_actreg_bwd(const ActRegArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(actreg_bwd_kernel, actreg_grid(a), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

int launch_drop_advance(unsigned long long* state, unsigned long long* snap, hipStream_t s) {
  hipLaunchKernelGGL(drop_advance_kernel, dim3(1), dim3(1), 0, s, state, snap);
  return (int)hipGetLastError();
}

int launch_drop_rows(int mode, long long R, int H, int V, const DropArgs& d, const DropCols& cm, const float* x, const long long* tokens, float* y,
                     hipStream_t s) {
  const long long n = drop_rows_threads(R, (H + 3) / 4, d.period);
  if (n <= 0) return 0;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipLaunchKernelGGL(drop_rows_kernel, grid, block, 0, s, mode, R, H, V, d, cm, x, tokens, y);
  return (int)hipGetLastError();
}

int launch_embed_fwd_ex(int R, int H, int V, const DropArgs& d, const WordDrop& wd, const float* w, const long long* tokens, float* y,
                        hipStream_t s) {
  const long long n = (long long)R * ((H + 3) / 4);
  if (n <= 0) return 0;
  hipLaunchKernelGGL(embed_fwd_ex_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, R, H, V, d, wd, w, tokens, y);
  return (int)hipGetLastError();
}
