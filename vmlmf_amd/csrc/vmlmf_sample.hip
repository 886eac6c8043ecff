// One decoded token of the LM (Model.generate, vmlmf_amd/lm.py) in ONE launch: the vocabulary projection of the top layer's
// output (Linear, V/src/models/vmlmf_lm.py:345-361: fc.w (V, H) row-major, fc.b (V)), the choice of the next token, its
// log-probability and - optionally - the next step's input row of the embedding table.  No (B, V) score tensor exists.
//   scores[b][v] = fc.b[v] + sum_k h[b][k] fc.w[v][k]               fp32, fixed order (bit-identical from run to run)
//   greedy (inverse temperature 0):  token = argmax_v scores[b][v], ties to the lowest index
//   sampling:                         token = argmax_v scores[b][v] / tau + G[b][v], G = -log(-log u) Gumbel noise: exactly a draw
//                                     from softmax(scores / tau) without sort, prefix sum or probability tensor
//   logprob[b] = scores[b][token] - logsumexp_v scores[b][v]    (untempered: what nll_loss charges for that token)
// u comes from Philox4x32-10 laid out as the dropout's (vmlmf_dropout.h): counter = (position = step B + b, v >> 2, SITE_SAMPLE,
// offset low word), key = (seed low word, seed high word + offset high word), word = out[v & 3], u = ((word >> 8) + 0.5) 2^-24.
//
// Tiles.  A workgroup (four waves) owns a strip of `tpw` vocabulary tiles of 16 rows; each tile is one 16 x 16 block of scores on
// v_mfma_f32_16x16x4_f32 (M = vocabulary rows, N = batch rows padded to 16), the four waves splitting H (lane (r, q) of wave w
// feeds k = 16 i + 4 w + q of step i) and meeting in LDS in wave order.  A batch wider than 16 takes passes of 16 rows.
// Merge.  Each workgroup leaves per batch row (best perturbed score, its raw score and index) and (max, sum of exp) of its strip,
// written through to agent scope, then takes a ticket; the LAST workgroup to arrive merges the strips in a fixed tree, writes the
// outputs and puts the ticket back to zero.  Nobody waits for anybody: no co-residency is needed, a captured launch replays.
//
// Filters (top_k, top_p; the *_filtered entry points).  They act on the tempered scores z = scores / tau, in the order temperature,
// top-k, top-p over the renormalised survivors of top-k, under ONE total order on tokens: larger z first, equal z to the lower index
// (best_merge's tie rule).
//   top_k = k        exactly the first min(k, V) tokens of the order are kept (0 and k >= V: off)
//   top_p = p        of those, the shortest prefix whose mass reaches p: the token at sorted position j is kept iff the mass of the
//                    tokens before it is < p (the first token always is; 1: off).  Mass = exp(z_v - z_max) over the set top-k kept,
//                    normalised by its own sum, held in FIXED POINT with 40 fractional bits (the largest token's mass is 2^40, a row's
//                    sum stays below 2^63 for V < 2^23): integer sums do not depend on the order of arrival.
//   token = argmax over the kept set of z + G, G exactly the unfiltered kernels' noise for (step B + b, v); Philox runs for the quads
//   that hold a kept token only.  logprob stays the untempered, unfiltered log-softmax; kept[b] = how many tokens survived.
// Selection (pick_filtered: one workgroup per row, ONE non-inlined device function that both filtered kernels call - 1024 threads in
// the choice launch, where a pass is a chain of round trips per thread, 256 in the fused launch, whose strips set the workgroup's
// size; the per-quad and per-token work is written as rolled loops: the library's size is held to a limit, tests/test_cabi.py).  One
// pass reads the row and parks the
// order-preserving 32-bit key of z in LDS (rows longer than SF_LDS_V re-read the scores instead).  A radix select from the most
// significant byte follows - four levels of a 256-bin histogram in LDS, 64-bit integer atomics - once over counts (the k-th key) and
// once over masses (the key at which the running mass reaches p).  Tokens whose key equals the threshold key are admitted in index
// order until the count or the mass is met.  A last pass does Gumbel-max over the kept tokens.  Everything is integer or fixed-order
// fp32: bit-identical from run to run.
// The fused form with filters: the strips write their scores (B x V floats) through to agent scope instead of the per-strip partials,
// and the last workgroup to arrive runs pick_filtered over them, a row after the other.  Same ticket, still nobody waits.  One
// workgroup's selection is what a token then waits for: measured slower than the GEMM + choice form at every width
// (docs/design/lm_sampling.md), so vmlmf_amd.lm_sample takes this form only where it is asked for.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vmlmf_hip.h"
#include "vmlmf_device.h"
#include "vmlmf_dropout.h"
#include "vmlmf_launch.h"

namespace {

constexpr int SM_NI = 41;        // MFMA steps per wave and chunk of H: a chunk is 4 waves x 4 x 41 = 656 >= 650 (the PTB LM)
constexpr int SM_MAXWG = 512;    // strips: the merge reads at most 8 partials per lane
constexpr int SM_NOIDX = 0x7fffffff;

typedef float f32x4s __attribute__((ext_vector_type(4)));

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
__device__ __forceinline__ u64 mass_of(unsigned k, float zmax) { return (u64)__float2ull_rn(expf(z_of(k) - zmax) * SF_ONE); }
__device__ __forceinline__ u64 shfl64(u64 v, int src) {
  return ((u64)(unsigned)__shfl((int)(v >> 32), src, 64) << 32) | (unsigned)__shfl((int)(unsigned)v, src, 64);
}
__device__ __forceinline__ u64 shfl_up64(u64 v, int d) {
  return ((u64)(unsigned)__shfl_up((int)(v >> 32), d, 64) << 32) | (unsigned)__shfl_up((int)(unsigned)v, d, 64);
}

struct SelRow {
  const float *row, *bias;
  float inv_temp, zmax;
  int V, nt;   // nt: threads of the workgroup
  bool resident;
  const unsigned* keys;
  __device__ __forceinline__ float score(int v) const { return (bias != nullptr ? bias[v] : 0.f) + row[v]; }
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
template <class F>
__device__ __forceinline__ void for_quads(const SelRow& r, F f) {
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
__device__ __forceinline__ void radix_select(const SelRow& r, SelScratch& S, bool mass, bool floor, unsigned floor_key, u64 floor_w, float p, u64& target,
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
__device__ __forceinline__ int tie_cutoff(const SelRow& r, SelScratch& S, unsigned K, int n) {
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

// row (V scores, + bias where given) -> the filtered choice.  top_k in [0, V) (0: off), top_p in (0, 1] (1: off), inv_temp > 0.
// (one copy in the library, called by both kernels: the scratch is the function's own LDS)
__device__ __attribute__((noinline, minsize)) RowPick pick_filtered(const float* row, const float* bias, int V, float inv_temp, int top_k, float top_p,
                                                            DropKey key, unsigned position) {
  __shared__ SelScratch S;
  const int NT = blockDim.x, NW = NT >> 6;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  SelRow r;
  r.row = row, r.bias = bias, r.inv_temp = inv_temp, r.V = V, r.nt = NT, r.resident = V <= SF_LDS_V, r.keys = S.keys, r.zmax = -INFINITY;
  // pass 1: keys to LDS; (max, sum exp) of the untempered scores; the largest tempered score
  float m = -INFINITY, s = 0.f, zmax = -INFINITY;
  __syncthreads();   // the previous row's readers are done with the scratch
  for (int v0 = tid; v0 < V; v0 += 8 * NT) {
    float sc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) sc[j] = r.score(v0 + NT * j < V ? v0 + NT * j : v0);   // eight loads in flight
#pragma unroll 1
    for (int j = 0; j < 8 && v0 + NT * j < V; ++j) {
      const float a = j & 1 ? sc[1] : sc[0], b = j & 1 ? sc[3] : sc[2], c = j & 1 ? sc[5] : sc[4], d = j & 1 ? sc[7] : sc[6];
      const float x = j < 4 ? (j < 2 ? a : b) : (j < 6 ? c : d);
      const float z = tempered(x, inv_temp);
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
  out.raw = out.idx != SM_NOIDX ? r.score(out.idx) : 0.f;
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

// a.scores != NULL (filters): the strips leave their scores instead of the partials and the last workgroup runs pick_filtered over
// them.  (One kernel for both, not two instantiations: the strips' code is most of it, and the library's size is held to a limit.)
__global__ __launch_bounds__(256) void lm_sample_kernel(LmSampleArgs a) {
  const bool FILT = a.scores != nullptr;
  __shared__ float red[4][256];
  __shared__ int last_flag;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
  const int tiles = (a.V + 15) >> 4;
  const int t0 = blockIdx.x * a.tpw, t1 = t0 + a.tpw < tiles ? t0 + a.tpw : tiles;
  const int bb = tid >> 4, vv = tid & 15;   // epilogue role: batch row bb of the pass, vocabulary row vv of the tile
  const bool GUMBEL = a.inv_temp > 0.f;
  const DropKey key = GUMBEL ? sample_key(a.state) : DropKey{0u, 0u, 0u, 0u};
  for (int b0 = 0; b0 < a.B; b0 += 16) {
    const bool bok = b0 + r < a.B;   // operand role: batch row b0 + r feeds the MFMA's column r
    const float* hp = a.h + (size_t)(bok ? b0 + r : 0) * a.H;
    float bz = -INFINITY, braw = 0.f, m = -INFINITY, s = 0.f;
    int bidx = SM_NOIDX;
    for (int t = t0; t < t1; ++t) {
      const int v0 = t << 4;
      const bool vok = v0 + r < a.V;
      const float* wp = a.w + (size_t)(vok ? v0 + r : 0) * a.H;
      f32x4s acc = {0.f, 0.f, 0.f, 0.f};
#ifdef VMLMF_SAMPLE_VALU_HEAD
      float vdot = 0.f;
      {
        const int v = v0 + vv, b = b0 + bb;
        const float* wr = a.w + (size_t)(v < a.V ? v : 0) * a.H;
        const float* hr = a.h + (size_t)(b < a.B ? b : 0) * a.H;
        float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
        int k = 0;
        for (; k + 3 < a.H; k += 4) d0 = fmaf(wr[k], hr[k], d0), d1 = fmaf(wr[k + 1], hr[k + 1], d1), d2 = fmaf(wr[k + 2], hr[k + 2], d2), d3 = fmaf(wr[k + 3], hr[k + 3], d3);
        for (; k < a.H; ++k) d0 = fmaf(wr[k], hr[k], d0);
        vdot = (d0 + d1) + (d2 + d3);
      }
      if (false)
#endif
      for (int kc = 0; kc < a.H; kc += 16 * SM_NI) {
        const int rem = (a.H - kc + 15) >> 4, nact = rem < SM_NI ? rem : SM_NI;
        float av[SM_NI], bv[SM_NI];
        // every load of the chunk in flight before the first MFMA: unconditional, clamped addresses (a load under a branch waited for
        // the one before it: 41 round trips a tile)
#pragma unroll
        for (int i = 0; i < SM_NI; ++i) {
          const int k = kc + 16 * i + 4 * wave + q;
          const bool in = k < a.H;
          const int kk = in ? k : 0;
          const float wv = wp[kk], hv = hp[kk];
          av[i] = (in && vok) ? wv : 0.f;
          bv[i] = (in && bok) ? hv : 0.f;
        }
#pragma unroll
        for (int i = 0; i < SM_NI; ++i)
          if (i < nact) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[i], acc, 0, 0, 0);
      }
      __syncthreads();   // the previous tile's epilogue has read `red`
#pragma unroll
      for (int i = 0; i < 4; ++i) red[wave][(4 * q + i) * 16 + r] = acc[i];   // lane (r, q), element i: vocabulary row 4 q + i, batch column r
      __syncthreads();
      const int v = v0 + vv, b = b0 + bb;
      if (v < a.V && b < a.B) {
        const int e = vv * 16 + bb;
#ifdef VMLMF_SAMPLE_VALU_HEAD
        const float sc = (a.bias != nullptr ? a.bias[v] : 0.f) + vdot;
#else
        const float sc = (a.bias != nullptr ? a.bias[v] : 0.f) + (((red[0][e] + red[1][e]) + red[2][e]) + red[3][e]);
#endif
        if (FILT) {
          st1g_agent((gf32*)(a.scores + (size_t)b * a.V + v), sc);
        } else {
          const float z = GUMBEL ? fmaf(sc, a.inv_temp, gumbel(key, (unsigned)a.step * (unsigned)a.B + (unsigned)b, v)) : sc;
          best_merge(bz, braw, bidx, z, sc, v);
          lse_merge(m, s, sc, 1.f);
        }
      }
    }
    if (!FILT) {
      // the 16 lanes of batch row bb (one 16-lane group): butterfly, every lane ends with the same bits
#pragma unroll
      for (int o = 8; o >= 1; o >>= 1) {
        const float z2 = __shfl_xor(bz, o, 64), r2 = __shfl_xor(braw, o, 64), m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        const int i2 = __shfl_xor(bidx, o, 64);
        best_merge(bz, braw, bidx, z2, r2, i2);
        lse_merge(m, s, m2, s2);
      }
      if (vv == 0 && b0 + bb < a.B) {
        float* p = a.part + ((size_t)blockIdx.x * a.B + b0 + bb) * 8;
        st4g_agent((gf32*)p, make_float4(bz, braw, __int_as_float(bidx), 0.f));
        st4g_agent((gf32*)(p + 4), make_float4(m, s, 0.f, 0.f));
      }
    }
  }
  // every strip's partials (filtered: scores) are out (written through to agent scope: visible on every XCD once vmcnt has counted them); then the ticket
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const unsigned long long t = __hip_atomic_fetch_add(a.ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last_flag = t == (unsigned long long)gridDim.x - 1ull;
  }
  __syncthreads();
  if (!last_flag) return;
  // last arrival: an agent-scope acquire in every wave (this CU's stale lines dropped), then plain 16-byte loads - all of a row's in
  // flight at once (one relaxed atomic load per word serialised them: 48 round trips a row).  A wave per batch row, lane l
  // merges strips l, l + 64, ... in order, then a 64-lane butterfly.
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (FILT) {
    for (int b = 0; b < a.B; ++b) {
      const RowPick pk = pick_filtered(a.scores + (size_t)b * a.V, nullptr, a.V, a.inv_temp, a.top_k, a.top_p, key,
                                       (unsigned)a.step * (unsigned)a.B + (unsigned)b);
      write_pick(pk, b, a.H, a.tokens, a.logprob, a.kept, a.x_next, a.embed);
    }
    if (tid == 0) __hip_atomic_store(a.ticket, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  const int G = gridDim.x;
  for (int b = wave; b < a.B; b += 4) {
    float4 p0[SM_MAXWG / 64], p1[SM_MAXWG / 64];
#pragma unroll
    for (int j = 0; j < SM_MAXWG / 64; ++j) {
      const int gi = lane + 64 * j;
      const float* p = a.part + ((size_t)(gi < G ? gi : 0) * a.B + b) * 8;
      p0[j] = ld4(p), p1[j] = ld4(p + 4);
    }
    float z = -INFINITY, raw = 0.f, mm = -INFINITY, ss = 0.f;
    int idx = SM_NOIDX;
#pragma unroll
    for (int j = 0; j < SM_MAXWG / 64; ++j) {
      if (lane + 64 * j < G) {
        best_merge(z, raw, idx, p0[j].x, p0[j].y, __float_as_int(p0[j].z));
        lse_merge(mm, ss, p1[j].x, p1[j].y);
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float z2 = __shfl_xor(z, o, 64), r2 = __shfl_xor(raw, o, 64), m2 = __shfl_xor(mm, o, 64), s2 = __shfl_xor(ss, o, 64);
      const int i2 = __shfl_xor(idx, o, 64);
      best_merge(z, raw, idx, z2, r2, i2);
      lse_merge(mm, ss, m2, s2);
    }
    const int tok = (idx >= 0 && idx < a.V) ? idx : 0;   // (every score NaN: token 0, NaN log-probability)
    if (lane == 0) {
      a.tokens[b] = tok;
      if (a.logprob != nullptr) a.logprob[b] = idx == tok ? raw - (mm + logf(ss)) : NAN;
    }
    if (a.x_next != nullptr) {
      const float* src = a.embed + (size_t)tok * a.H;
      float* dst = a.x_next + (size_t)b * a.H;
      for (int e = lane; e < a.H; e += 64) dst[e] = src[e];
    }
  }
  if (tid == 0) __hip_atomic_store(a.ticket, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the filtered choice over the (B, V) scores of a library GEMM: one workgroup of SF_CHOOSE_NT threads per row
constexpr int SF_CHOOSE_NT = 1024;
__global__ __launch_bounds__(SF_CHOOSE_NT) void lm_choose_filtered_kernel(LmChooseArgs a) {
  const int b = blockIdx.x;
  const RowPick pk = pick_filtered(a.scores + (size_t)b * a.V, a.bias, a.V, a.inv_temp, a.top_k, a.top_p, sample_key(a.state),
                                   (unsigned)a.step * (unsigned)a.B + (unsigned)b);
  write_pick(pk, b, a.H, a.tokens, a.logprob, a.kept, a.x_next, a.embed);
}

// ---- the same choice over a (B, V) score matrix a library GEMM produced: the form for batches wider than one 16-row tile ----
// One workgroup per row; a thread takes four neighbouring vocabulary rows at a time, so one Philox call serves them all.  The row is
// read once; per-thread (best, max, sum of exp) partials meet in a fixed tree (64-lane butterfly, then the four waves in order).
__global__ __launch_bounds__(256) void lm_choose_kernel(LmChooseArgs a) {
  __shared__ float red[4][5];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, b = blockIdx.x;
  const bool GUMBEL = a.inv_temp > 0.f;
  const DropKey key = GUMBEL ? sample_key(a.state) : DropKey{0u, 0u, 0u, 0u};
  const float* row = a.scores + (size_t)b * a.V;
  const unsigned position = (unsigned)a.step * (unsigned)a.B + (unsigned)b;
  float z = -INFINITY, raw = 0.f, m = -INFINITY, s = 0.f;
  int idx = SM_NOIDX;
  const int quads = (a.V + 3) >> 2;
  for (int qd = tid; qd < quads; qd += 256) {
    unsigned w[4] = {0u, 0u, 0u, 0u};
    if (GUMBEL) philox4x32_10(position, (unsigned)qd, key.c2, key.c3, key.k0, key.k1, w);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int v = 4 * qd + e;
      if (v < a.V) {
        const float sc = (a.bias != nullptr ? a.bias[v] : 0.f) + row[v];
        best_merge(z, raw, idx, GUMBEL ? fmaf(sc, a.inv_temp, gumbel_of(w[e])) : sc, sc, v);
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
  }
  if (lane == 0) red[wave][0] = z, red[wave][1] = raw, red[wave][2] = __int_as_float(idx), red[wave][3] = m, red[wave][4] = s;
  __syncthreads();
  z = red[0][0], raw = red[0][1], idx = __float_as_int(red[0][2]), m = red[0][3], s = red[0][4];
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    best_merge(z, raw, idx, red[w][0], red[w][1], __float_as_int(red[w][2]));
    lse_merge(m, s, red[w][3], red[w][4]);
  }
  const int tok = (idx >= 0 && idx < a.V) ? idx : 0;
  if (tid == 0) {
    a.tokens[b] = tok;
    if (a.logprob != nullptr) a.logprob[b] = idx == tok ? raw - (m + logf(s)) : NAN;
  }
  if (a.x_next != nullptr) {
    const float* src = a.embed + (size_t)tok * a.H;
    for (int e = tid; e < a.H; e += 256) a.x_next[(size_t)b * a.H + e] = src[e];
  }
}

int sample_strips(int V, int* tpw) {
  const int tiles = (V + 15) / 16;
  const int per = (tiles + SM_MAXWG - 1) / SM_MAXWG;
  if (tpw != nullptr) *tpw = per;
  return (tiles + per - 1) / per;
}

}  // namespace

size_t lm_sample_workspace_bytes(int B, int V) {
  const int tiles = (V + 15) / 16;
  return (size_t)(tiles < SM_MAXWG ? tiles : SM_MAXWG) * (size_t)B * 8 * sizeof(float);
}
// the unfiltered launch's partials (filters off: that launch runs on this workspace), then the (B, V) scores
size_t lm_sample_filtered_workspace_bytes(int B, int V) { return lm_sample_workspace_bytes(B, V) + (size_t)B * (size_t)V * sizeof(float); }

// a.top_k in [0, V) (0: off), a.top_p in (0, 1] (1: off); with either on (and sampling) the filtered kernel runs, a.kept takes its counts
static bool filters_on(float inv_temp, int top_k, float top_p) { return inv_temp > 0.f && (top_k > 0 || top_p < 1.f); }

int launch_lm_sample(LmSampleArgs a, hipStream_t s) {
  const int G = sample_strips(a.V, &a.tpw);
  if (filters_on(a.inv_temp, a.top_k, a.top_p))
    a.scores = a.part + lm_sample_workspace_bytes(a.B, a.V) / sizeof(float);
  else
    a.scores = nullptr;
  hipLaunchKernelGGL(lm_sample_kernel, dim3(G), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

int launch_lm_choose(const LmChooseArgs& a, hipStream_t s) {
  if (filters_on(a.inv_temp, a.top_k, a.top_p)) hipLaunchKernelGGL(lm_choose_filtered_kernel, dim3(a.B), dim3(SF_CHOOSE_NT), 0, s, a);
  else hipLaunchKernelGGL(lm_choose_kernel, dim3(a.B), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}
