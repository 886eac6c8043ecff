// The choice of one token from a row of scores by one workgroup - what vmlmf_sample.hip (libvmlmf_hip.so: vmlmf_lm_sample*,
// vmlmf_lm_choose*) and vmlmf_decode.hip (libvmlmf_decode.so: vmlmf_decode_choose) both run, written once.  The contract of the
// filters, the total order and the noise is at the head of vmlmf_sample.hip; this header holds
//   best_merge / lse_merge          the two merges of the fixed reduction trees
//   gumbel_of / sample_key / gumbel the sampler's noise: Philox4x32-10 at (position, v >> 2, VMLMF_SITE_SAMPLE, offset)
//   key_of / z_of / tempered        the order-preserving 32-bit key of a tempered score
//   radix_select / tie_cutoff       the k-th key and the key at which the running mass reaches p; the tie group's cut
//   pick_row                        the filtered choice (top-k, top-p, Gumbel-max over the kept set) of one row
//   choose_row                      the unfiltered choice (greedy, or Gumbel-max over the whole row) of one row, 256 threads
//   write_pick                      a row's outputs
// all parameterised by HOW A ROW'S SCORE IS READ, a `Src`:
//   Src::CONTROLLED                 false: the score that is chosen on is the raw score (PlainScores below)
//   float raw(v)                    x[v]: what (max, sum exp) and the log-probability are formed from
//   Src::Ctl, Ctl ctl(v)            whatever else of token v the controlled score needs, LOADED (so a pass can put eight tokens'
//                                   loads in flight before it waits for one)
//   float score(v, x, ctl)          the score the choice runs on (keys, z); -inf: never chosen, not counted in `kept`
// With PlainScores every function here is the arithmetic vmlmf_sample.hip held before the split, operation for operation: the
// existing entry points give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vmlmf_hip.h"
#include "vmlmf_dropout.h"

constexpr int SM_NOIDX = 0x7fffffff;

// (z, raw, idx): the larger perturbed score wins, equal ones go to the lower index
__device__ __forceinline__ void best_merge(float& z, float& raw, int& idx, float z2, float raw2, int idx2) {
  if (z2 > z || (z2 == z && idx2 < idx)) z = z2, raw = raw2, idx = idx2;
}
// (m, s) = (max, sum exp(x - max)) of two sets
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
  const float M = fmaxf(m, m2);
  if (M == -INFINITY) return;
  s = s * expf(m - M) + s2 * expf(m2 - M);
  m = M;
}

// G = -log(-log u), u = ((word >> 8) + 0.5) 2^-24, in fp32 without ever rounding u to 1: below 2^23 the mantissa holds m + 0.5
// exactly; above it 1 - u = ((2^24 - 1 - m) + 0.5) 2^-24 does, and -log u = -log1p(-(1 - u))
__device__ __forceinline__ float gumbel_of(unsigned word) {
  const unsigned m = word >> 8;
  const float e = m < (1u << 23) ? -logf(((float)m + 0.5f) * 5.9604644775390625e-8f)
                                 : -log1pf(-((float)((1u << 24) - 1u - m) + 0.5f) * 5.9604644775390625e-8f);
  return -logf(e);
}
__device__ __forceinline__ DropKey sample_key(const unsigned long long* state) {
  const unsigned long long seed = state[0], off = state[1];
  DropKey k;
  k.k0 = (unsigned)seed, k.k1 = (unsigned)(seed >> 32) + (unsigned)(off >> 32), k.c2 = VMLMF_SITE_SAMPLE, k.c3 = (unsigned)off;
  return k;
}
__device__ __forceinline__ float gumbel(const DropKey& k, unsigned position, int v) {
  unsigned w[4];
  philox4x32_10(position, (unsigned)v >> 2, k.c2, k.c3, k.k0, k.k1, w);
  const int j = v & 3;
  return gumbel_of(j == 0 ? w[0] : j == 1 ? w[1] : j == 2 ? w[2] : w[3]);
}

// the scores of the existing entry points: row (V) of a GEMM, + bias where given; the choice runs on the raw score
struct PlainScores {
  static constexpr bool CONTROLLED = false;
  struct Ctl {};
  const float *row, *bias;
  __device__ __forceinline__ float raw(int v) const { return (bias != nullptr ? bias[v] : 0.f) + row[v]; }
  __device__ __forceinline__ Ctl ctl(int) const { return Ctl{}; }
  __device__ __forceinline__ float score(int, float x, const Ctl&) const { return x; }
};

// ---- the filtered choice of one row by a workgroup of NT threads (256: the fused launch; 1024: the choice launch, whose rows are
// long and whose passes are latency chains per thread); every thread returns the same RowPick ----
constexpr int SF_LDS_V = 12288;             // longest row whose keys stay in LDS (48 KB); longer rows re-read their scores
constexpr float SF_ONE = 1099511627776.f;   // 2^40: the fixed-point mass of the row's largest tempered score
typedef unsigned long long u64;

constexpr int SF_MAX_NT = 1024;
struct SelScratch {
  alignas(16) unsigned keys[SF_LDS_V];
  u64 hist[256];
  float red[SF_MAX_NT / 64][8];
  int tcnt[SF_MAX_NT];
  int cut[4];
};
struct RowPick {
  int idx, kept;         // idx: SM_NOIDX if nothing could be chosen (every score NaN)
  float raw, m, s;       // the chosen token's untempered score; (max, sum exp) of the untempered row
};

// larger float <=> larger key (-0 never gets here: tempered() adds +0)
__device__ __forceinline__ unsigned key_of(float z) {
  const unsigned u = __float_as_uint(z);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float z_of(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }
__device__ __forceinline__ float tempered(float sc, float inv_temp) { return sc * inv_temp + 0.f; }
constexpr unsigned SF_KEY_NEG_INF = 0x007fffffu;   // key_of(-inf): a controlled score that is never chosen
__device__ __forceinline__ u64 mass_of(unsigned k, float zmax) { return (u64)__float2ull_rn(expf(z_of(k) - zmax) * SF_ONE); }
__device__ __forceinline__ u64 shfl64(u64 v, int src) {
  return ((u64)(unsigned)__shfl((int)(v >> 32), src, 64) << 32) | (unsigned)__shfl((int)(unsigned)v, src, 64);
}
__device__ __forceinline__ u64 shfl_up64(u64 v, int d) {
  return ((u64)(unsigned)__shfl_up((int)(v >> 32), d, 64) << 32) | (unsigned)__shfl_up((int)(unsigned)v, d, 64);
}
// a[j] of eight registers by a rolled loop's j, without indexing them
__device__ __forceinline__ float pick8(const float (&sc)[8], int j) {
  const float a = j & 1 ? sc[1] : sc[0], b = j & 1 ? sc[3] : sc[2], c = j & 1 ? sc[5] : sc[4], d = j & 1 ? sc[7] : sc[6];
  return j < 4 ? (j < 2 ? a : b) : (j < 6 ? c : d);
}

template <class Src>
struct SelRow {
  Src src;
  float inv_temp, zmax;
  int V, nt;   // nt: threads of the workgroup
  bool resident;
  const unsigned* keys;
  __device__ __forceinline__ float score(int v) const { return src.score(v, src.raw(v), src.ctl(v)); }
  __device__ __forceinline__ unsigned key(int v) const { return resident ? keys[v] : key_of(tempered(score(v), inv_temp)); }
  // the keys of vocabulary rows 4 qd .. 4 qd + 3 (rows past V: anything)
  __device__ __forceinline__ void quad(int qd, unsigned (&k)[4]) const {
    if (resident) {
      const uint4 t = reinterpret_cast<const uint4*>(keys)[qd];
      k[0] = t.x, k[1] = t.y, k[2] = t.z, k[3] = t.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) k[e] = key(4 * qd + e < V ? 4 * qd + e : V - 1);
    }
  }
};
// f(qd, keys of the quad) over a thread's quads qd = tid, tid + NT, ...: four quads' loads in flight at a time (one after the other
// they cost a round trip each, and a pass has nothing else to wait for)
template <class Src, class F>
__device__ __forceinline__ void for_quads(const SelRow<Src>& r, F f) {
  const int NT = r.nt;
  const int quads = (r.V + 3) >> 2;
  for (int q0 = threadIdx.x; q0 < quads; q0 += 4 * NT) {
    unsigned k[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) r.quad(q0 + NT * j < quads ? q0 + NT * j : q0, k[j]);
    // (the work on a quad is written once, not four times: the library's size is held to a limit)
#pragma unroll 1
    for (int j = 0; j < 4 && q0 + NT * j < quads; ++j) {
      unsigned kj[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) kj[e] = j == 0 ? k[0][e] : j == 1 ? k[1][e] : j == 2 ? k[2][e] : k[3][e];
      f(q0 + NT * j, kj);
    }
  }
}

// Radix select over the row's keys from the most significant byte.  Weights are counts (mass = false) or fixed-point masses; with
// `floor` only keys above floor_key weigh in, and the keys equal to it weigh floor_w together (the tokens top-k admitted from its tie
// group).  target: the rank looked for (counts) / ceil(p x total) (masses, formed at the first level).  Finds the key K at which the
// running weight, walked from the largest key down, reaches the target: above = weight of the keys > K (< target), leaf = weight of
// the keys == K (above + leaf >= target).  Every thread returns the same values.
template <class Src>
__device__ __forceinline__ void radix_select(const SelRow<Src>& r, SelScratch& S, bool mass, bool floor, unsigned floor_key, u64 floor_w, float p, u64& target,
                             unsigned& K, u64& above, u64& leaf) {
  const int tid = threadIdx.x, lane = tid & 63;
  unsigned prefix = 0u;
  u64 acc = 0ull, lf = 0ull;
  for (int level = 0; level < 4; ++level) {
    const int shift = 24 - 8 * level;
    __syncthreads();   // the previous level's readers are done with hist
    if (tid < 256) S.hist[tid] = 0ull;
    __syncthreads();
    // a thread's keys mostly share their leading bytes: runs of one digit go to the histogram in one atomic
    int cur = -1;
    u64 w = 0ull;
    for_quads(r, [&](int qd, const unsigned(&k4)[4]) {
#pragma unroll 1
      for (int e = 0; e < 4; ++e) {
        const unsigned k = e == 0 ? k4[0] : e == 1 ? k4[1] : e == 2 ? k4[2] : k4[3];
        if (4 * qd + e >= r.V || (level > 0 && (k >> (shift + 8)) != prefix) || (floor && k <= floor_key)) continue;
        const int d = (int)((k >> shift) & 255u);
        if (d != cur) {
          if (cur >= 0) atomicAdd(&S.hist[cur], w);
          cur = d, w = 0ull;
        }
        w += mass ? mass_of(k, r.zmax) : 1ull;
      }
    });
    if (cur >= 0) atomicAdd(&S.hist[cur], w);
    if (tid == 0 && floor && floor_w != 0ull && (level == 0 || (floor_key >> (shift + 8)) == prefix))
      atomicAdd(&S.hist[(floor_key >> shift) & 255u], floor_w);
    __syncthreads();
    // every wave on its own: lane l holds digits 255 - 4 l .. 252 - 4 l, a scan over the lanes runs from the largest digit down
    const u64 h0 = S.hist[255 - 4 * lane], h1 = S.hist[254 - 4 * lane], h2 = S.hist[253 - 4 * lane], h3 = S.hist[252 - 4 * lane];
    const u64 own = (h0 + h1) + (h2 + h3);
    u64 incl = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const u64 t = shfl_up64(incl, o);
      if (lane >= o) incl += t;
    }
    if (level == 0 && mass) {
      const u64 total = shfl64(incl, 63);
      const double want = ceil((double)p * (double)total);
      target = want >= (double)total ? total : (u64)want;
      if (target < 1ull) target = 1ull;
    }
    const u64 excl = incl - own;
    const bool mine = acc + excl < target && target <= acc + incl;
    const unsigned long long vote = __ballot(mine);
    const int src = vote != 0ull ? __ffsll((long long)vote) - 1 : 63;
    u64 a = excl, hv = h0;
    int j = 0;
    if (acc + a + h0 < target) {
      a += h0, hv = h1, j = 1;
      if (acc + a + h1 < target) {
        a += h1, hv = h2, j = 2;
        if (acc + a + h2 < target) a += h2, hv = h3, j = 3;
      }
    }
    const int d = __shfl(255 - 4 * lane - j, src, 64);
    acc += shfl64(a, src);
    lf = shfl64(hv, src);
    prefix = (prefix << 8) | (unsigned)d;
  }
  K = prefix, above = acc, leaf = lf;
}

// the index of the n-th (n >= 1) token, in index order, whose key is K: threads own contiguous ranges
template <class Src>
__device__ __forceinline__ int tie_cutoff(const SelRow<Src>& r, SelScratch& S, unsigned K, int n) {
  const int NT = r.nt;
  const int tid = threadIdx.x, chunk = (r.V + NT - 1) >> (31 - __clz(NT));   // NT: a power of two
  const int lo = tid * chunk < r.V ? tid * chunk : r.V, hi = lo + chunk < r.V ? lo + chunk : r.V;
  int c = 0;
  for (int v = lo; v < hi; ++v) c += r.key(v) == K;
  __syncthreads();
  S.tcnt[tid] = c;
  __syncthreads();
  if (tid == 0) {
    int rem = n, t = 0;
    for (; t < NT - 1; ++t) {
      if (S.tcnt[t] >= rem) break;
      rem -= S.tcnt[t];
    }
    S.cut[0] = t, S.cut[1] = rem, S.cut[2] = r.V - 1;
  }
  __syncthreads();
  if (tid == S.cut[0]) {
    int rem = S.cut[1];
    for (int v = lo; v < hi; ++v)
      if (r.key(v) == K && --rem == 0) {
        S.cut[2] = v;
        break;
      }
  }
  __syncthreads();
  return S.cut[2];
}

// src (V scores) -> the filtered choice, by the whole workgroup on the scratch S.  top_k in [0, V) (0: off), top_p in (0, 1]
// (1: off), inv_temp > 0.
template <class Src>
__device__ __forceinline__ RowPick pick_row(SelScratch& S, const Src& src, int V, float inv_temp, int top_k, float top_p, DropKey key,
                                            unsigned position) {
  const int NT = blockDim.x, NW = NT >> 6;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  SelRow<Src> r;
  r.src = src, r.inv_temp = inv_temp, r.V = V, r.nt = NT, r.resident = V <= SF_LDS_V, r.keys = S.keys, r.zmax = -INFINITY;
  // pass 1: keys to LDS; (max, sum exp) of the untempered scores; the largest tempered score
  float m = -INFINITY, s = 0.f, zmax = -INFINITY;
  __syncthreads();   // the previous row's readers are done with the scratch
  for (int v0 = tid; v0 < V; v0 += 8 * NT) {
    float sc[8], cs[8];
    typename Src::Ctl ct[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {   // eight tokens' loads in flight
      const int v = v0 + NT * j < V ? v0 + NT * j : v0;
      sc[j] = src.raw(v);
      if (Src::CONTROLLED) ct[j] = src.ctl(v);
    }
    if (Src::CONTROLLED) {
#pragma unroll
      for (int j = 0; j < 8; ++j) cs[j] = src.score(v0 + NT * j < V ? v0 + NT * j : v0, sc[j], ct[j]);
    }
#pragma unroll 1
    for (int j = 0; j < 8 && v0 + NT * j < V; ++j) {
      const float x = pick8(sc, j);
      const float z = tempered(Src::CONTROLLED ? pick8(cs, j) : x, inv_temp);
      if (r.resident) S.keys[v0 + NT * j] = key_of(z);
      lse_merge(m, s, x, 1.f);
      zmax = fmaxf(zmax, z);
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    lse_merge(m, s, m2, s2);
    zmax = fmaxf(zmax, __shfl_xor(zmax, o, 64));
  }
  if (lane == 0) S.red[wave][0] = m, S.red[wave][1] = s, S.red[wave][2] = zmax;
  __syncthreads();
  m = S.red[0][0], s = S.red[0][1], zmax = S.red[0][2];
#pragma unroll
  for (int w = 1; w < NW; ++w) {
    lse_merge(m, s, S.red[w][0], S.red[w][1]);
    zmax = fmaxf(zmax, S.red[w][2]);
  }
  r.zmax = zmax;
  // the threshold key Kf, and how many of the tokens that carry it are admitted (n_tie of n_have, lowest indices first)
  const bool has_k = top_k > 0 && top_k < V, has_p = top_p < 1.f;
  unsigned Kk = 0u, Kf = 0u;
  long long n_tie = V, n_have = V, k_tie = 0, k_have = 0;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {   // 0: counts for top-k, 1: masses for top-p
    const bool mass = pass == 1;
    if (mass ? !has_p : !has_k) continue;
    unsigned K;
    u64 above, leaf, target = (u64)top_k;
    radix_select(r, S, mass, mass && has_k, Kk, mass && has_k ? (u64)k_tie * mass_of(Kk, zmax) : 0ull, top_p, target, K, above, leaf);
    if (!mass) {
      Kk = Kf = K, n_tie = k_tie = (long long)(target - above), n_have = k_have = (long long)leaf;
    } else {
      const u64 mu = mass_of(K, zmax);
      const bool same = has_k && K == Kk;
      // tokens of the tie group: how many there are, how many the mass asks for (one copy of the 64-bit division)
      u64 num[2] = {leaf, target - above + mu - 1ull};
#pragma unroll 1
      for (int i = 0; i < 2; ++i) num[i] = num[i] / (mu != 0ull ? mu : 1ull);
      const long long avail = same ? k_tie : (mu != 0ull ? (long long)num[0] : 1);
      const long long need = mu != 0ull ? (long long)num[1] : avail;
      Kf = K, n_tie = need < avail ? need : avail, n_have = same ? k_have : avail;
    }
  }
  const int cut = n_tie < n_have ? tie_cutoff(r, S, Kf, (int)(n_tie < 1 ? 1 : n_tie)) : V;
  // last pass: Gumbel-max over the kept tokens, a thread takes four neighbours at a time so one Philox call serves them
  float bz = -INFINITY, braw = 0.f;
  int bidx = SM_NOIDX, cnt = 0;
  for_quads(r, [&](int qd, const unsigned(&k4)[4]) {
    bool keep[4], any = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int v = 4 * qd + e;
      keep[e] = v < V && (k4[e] > Kf || (k4[e] == Kf && v <= cut));
      if (Src::CONTROLLED) keep[e] = keep[e] && k4[e] != SF_KEY_NEG_INF;   // (top-k can reach down to the banned tokens)
      any = any || keep[e];
    }
    if (!any) return;
    unsigned w[4];
    philox4x32_10(position, (unsigned)qd, key.c2, key.c3, key.k0, key.k1, w);
#pragma unroll 1
    for (int e = 0; e < 4; ++e)
      if (e == 0 ? keep[0] : e == 1 ? keep[1] : e == 2 ? keep[2] : keep[3]) {
        const unsigned k = e == 0 ? k4[0] : e == 1 ? k4[1] : e == 2 ? k4[2] : k4[3];
        best_merge(bz, braw, bidx, z_of(k) + gumbel_of(e == 0 ? w[0] : e == 1 ? w[1] : e == 2 ? w[2] : w[3]), 0.f, 4 * qd + e);
        ++cnt;
      }
  });
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float z2 = __shfl_xor(bz, o, 64);
    const int i2 = __shfl_xor(bidx, o, 64);
    best_merge(bz, braw, bidx, z2, 0.f, i2);
    cnt += __shfl_xor(cnt, o, 64);
  }
  if (lane == 0) S.red[wave][4] = bz, S.red[wave][5] = __int_as_float(bidx), S.red[wave][6] = __int_as_float(cnt);
  __syncthreads();
  bz = S.red[0][4], bidx = __float_as_int(S.red[0][5]), cnt = __float_as_int(S.red[0][6]);
#pragma unroll
  for (int w = 1; w < NW; ++w) {
    best_merge(bz, braw, bidx, S.red[w][4], 0.f, __float_as_int(S.red[w][5]));
    cnt += __float_as_int(S.red[w][6]);
  }
  RowPick out;
  out.idx = (bidx >= 0 && bidx < V) ? bidx : SM_NOIDX;
  out.kept = cnt, out.m = m, out.s = s;
  out.raw = out.idx != SM_NOIDX ? src.raw(out.idx) : 0.f;
  return out;
}

// ---- the unfiltered choice of one row by a workgroup of SM_CHOOSE_NT threads: greedy (gumbel false: argmax, ties to the lower
// index) or Gumbel-max over the whole row.  A thread takes four neighbouring vocabulary rows at a time, so one Philox call serves
// them all.  The row is read once; per-thread (best, max, sum of exp) partials meet in a fixed tree (64-lane butterfly, then the
// four waves in order).  red: 4 x red_stride floats of LDS (red_stride >= 6).  kept: the tokens a controlled score left finite
// (plain scores: V) ----
constexpr int SM_CHOOSE_NT = 256;
template <class Src>
__device__ __forceinline__ RowPick choose_row(float* red, int red_stride, const Src& src, int V, float inv_temp, bool gumbel_on, DropKey key,
                                              unsigned position) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float z = -INFINITY, raw = 0.f, m = -INFINITY, s = 0.f;
  int idx = SM_NOIDX, cnt = 0;
  const int quads = (V + 3) >> 2;
  for (int qd = tid; qd < quads; qd += SM_CHOOSE_NT) {
    unsigned w[4] = {0u, 0u, 0u, 0u};
    if (gumbel_on) philox4x32_10(position, (unsigned)qd, key.c2, key.c3, key.k0, key.k1, w);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int v = 4 * qd + e;
      if (v < V) {
        const float sc = src.raw(v);
        if (Src::CONTROLLED) {
          const float c = src.score(v, sc, src.ctl(v));
          if (c != -INFINITY) {
            best_merge(z, raw, idx, gumbel_on ? fmaf(c, inv_temp, gumbel_of(w[e])) : c, sc, v);
            ++cnt;
          }
        } else {
          best_merge(z, raw, idx, gumbel_on ? fmaf(sc, inv_temp, gumbel_of(w[e])) : sc, sc, v);
        }
        lse_merge(m, s, sc, 1.f);
      }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float z2 = __shfl_xor(z, o, 64), r2 = __shfl_xor(raw, o, 64), m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    const int i2 = __shfl_xor(idx, o, 64);
    best_merge(z, raw, idx, z2, r2, i2);
    lse_merge(m, s, m2, s2);
    if (Src::CONTROLLED) cnt += __shfl_xor(cnt, o, 64);
  }
  float* mine = red + wave * red_stride;
  if (lane == 0) {
    mine[0] = z, mine[1] = raw, mine[2] = __int_as_float(idx), mine[3] = m, mine[4] = s;
    if (Src::CONTROLLED) mine[5] = __int_as_float(cnt);
  }
  __syncthreads();
  z = red[0], raw = red[1], idx = __float_as_int(red[2]), m = red[3], s = red[4];
  if (Src::CONTROLLED) cnt = __float_as_int(red[5]);
#pragma unroll
  for (int w = 1; w < SM_CHOOSE_NT / 64; ++w) {
    const float* o = red + w * red_stride;
    best_merge(z, raw, idx, o[0], o[1], __float_as_int(o[2]));
    lse_merge(m, s, o[3], o[4]);
    if (Src::CONTROLLED) cnt += __float_as_int(o[5]);
  }
  RowPick out;
  out.idx = (idx >= 0 && idx < V) ? idx : SM_NOIDX;
  out.kept = Src::CONTROLLED ? cnt : V, out.m = m, out.s = s, out.raw = raw;
  return out;
}

// the outputs of one row, by the whole workgroup
__device__ __forceinline__ void write_pick(const RowPick& pk, int b, int H, long long* tokens, float* logprob, int* kept, float* x_next,
                                           const float* embed) {
  const int tok = pk.idx != SM_NOIDX ? pk.idx : 0;   // (every score NaN: token 0, NaN log-probability)
  if (threadIdx.x == 0) {
    tokens[b] = tok;
    if (logprob != nullptr) logprob[b] = pk.idx == tok ? pk.raw - (pk.m + logf(pk.s)) : NAN;
    if (kept != nullptr) kept[b] = pk.kept;
  }
  if (x_next != nullptr) {
    const float* src = embed + (size_t)tok * H;
    for (int e = threadIdx.x; e < H; e += blockDim.x) x_next[(size_t)b * H + e] = src[e];
  }
}
