// The truncated choice of one row by one workgroup of 1024 threads: top-k, top-p, min-p, locally typical, epsilon and eta sampling in
// Hugging Face's order, then Gumbel-max over what they kept (include/vmlmf_truncate.h has the contract).  It stands on vmlmf_select.h -
// SelRow, for_quads, the keys, the fixed-point masses, the merges, the noise, radix_select / tie_cutoff for the two prefix filters -
// and adds what the new stages need:
//   TruncSet / in_set            the conjunction of the stages' predicates on (index, resident key)
//   sum_pass                     (S, sum mass (z_max - z), the largest key) of the current set: an exact 64-bit sum, an fp64 sum through
//                                a fixed tree (thread partials in for_quads' order, a 64-lane butterfly, then the waves in order)
//   view_select / view_tie_cut   radix select and tie cut over a KEY VIEW: the ordering key is computed on the fly from the resident
//                                key of z (typical sampling orders by |surprise - entropy|), the weights stay the masses of the z key,
//                                and the members of a tie group may weigh differently.  This is radix_select / tie_cutoff's scan a
//                                second time: those two are held to their bits and to the main library's size, so the view could not
//                                be threaded through them (docs/design/lm_truncation.md)
//   truncate_row                 the row: pass 1, the prefix stages, the stages on sums, the final pass
// Every threshold is formed once per row and then compared as an integer, a key or a correctly rounded fp32 difference, so every pass
// of a row - resident in LDS or re-read - sees the same set.  Plain HIP C++ for wave64; the LDS histogram atomics are 64-bit adds.
#pragma once
#include "vmlmf_select.h"

struct TruncParams {
  float log_a;                     // min-p: log(min_p), formed once on the host in fp64 and rounded to fp32; -inf: off
  float typical_p, epsilon, eta;   // 1, 0, 0: off
};

// the current set: every stage so far, as tests on (v, key of z)
struct TruncSet {
  unsigned Kf;      // the prefix stages: key > Kf, or key == Kf and v <= cut
  int cut;
  float log_a;      // min-p: z - z_max >= log a (-inf: off)
  bool typical;     // the band: deviation key > Kt, or == Kt and v <= cut_t
  float cbar;
  unsigned Kt;
  int cut_t;
  u64 min_mass;     // epsilon / eta: mass >= min_mass (0: off), or key >= ktop (the most probable survivor stays)
  unsigned ktop;
};

// z_max - z: the token's surprise up to the row's log S
__device__ __forceinline__ float surprise_of(unsigned k, float zmax) { return __fsub_rn(zmax, z_of(k)); }
// smaller |surprise - cbar| <=> larger key (the difference of two rounded operations, its sign dropped: the bits of a float >= 0
// order as unsigned integers)
__device__ __forceinline__ unsigned deviation_key(unsigned k, float zmax, float cbar) {
  return ~__float_as_uint(fabsf(__fsub_rn(surprise_of(k, zmax), cbar)));
}
__device__ __forceinline__ bool in_set(const TruncSet& t, float zmax, int v, unsigned k) {
  if (k == SF_KEY_NEG_INF || !(k > t.Kf || (k == t.Kf && v <= t.cut))) return false;
  if (!(__fsub_rn(z_of(k), zmax) >= t.log_a)) return false;
  if (t.typical) {
    const unsigned d = deviation_key(k, zmax, t.cbar);
    if (!(d > t.Kt || (d == t.Kt && v <= t.cut_t))) return false;
  }
  return t.min_mass == 0ull || k >= t.ktop || mass_of(k, zmax) >= t.min_mass;
}
__device__ __forceinline__ unsigned pick4(const unsigned (&k4)[4], int e) { return e == 0 ? k4[0] : e == 1 ? k4[1] : e == 2 ? k4[2] : k4[3]; }

struct TruncSums {
  u64 S;           // sum of the fixed-point masses
  double A;        // sum mass (z_max - z)
  unsigned ktop;   // the largest key
};
// the sums of the set t; every thread returns the same values
template <class Src>
__device__ __forceinline__ TruncSums sum_pass(const SelRow<Src>& r, SelScratch& S, const TruncSet& t) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, NW = r.nt >> 6;
  u64 s = 0ull;
  double a = 0.0;
  unsigned top = 0u;
  for_quads(r, [&](int qd, const unsigned(&k4)[4]) {
#pragma unroll 1
    for (int e = 0; e < 4; ++e) {
      const unsigned k = pick4(k4, e);
      if (4 * qd + e >= r.V || !in_set(t, r.zmax, 4 * qd + e, k)) continue;
      const u64 w = mass_of(k, r.zmax);
      s += w;
      a = __fma_rn((double)w, (double)surprise_of(k, r.zmax), a);
      top = k > top ? k : top;
    }
  });
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    s += shfl64(s, lane ^ o);
    a = __dadd_rn(a, __longlong_as_double((long long)shfl64((u64)__double_as_longlong(a), lane ^ o)));
    const unsigned t2 = (unsigned)__shfl_xor((int)top, o, 64);
    top = t2 > top ? t2 : top;
  }
  __syncthreads();   // the readers of hist (a select, an earlier sum) are done
  if (lane == 0) S.hist[3 * wave] = s, S.hist[3 * wave + 1] = (u64)__double_as_longlong(a), S.hist[3 * wave + 2] = top;
  __syncthreads();
  TruncSums out;
  out.S = S.hist[0], out.A = __longlong_as_double((long long)S.hist[1]), out.ktop = (unsigned)S.hist[2];
  for (int w = 1; w < NW; ++w) {
    out.S += S.hist[3 * w];
    out.A = __dadd_rn(out.A, __longlong_as_double((long long)S.hist[3 * w + 1]));
    const unsigned t2 = (unsigned)S.hist[3 * w + 2];
    out.ktop = t2 > out.ktop ? t2 : out.ktop;
  }
  return out;
}

// radix_select over a key view.  view(v, k, okey): whether token v (resident key k) takes part, and its ordering key; the weights are
// the masses of k.  Finds the ordering key K at which the running mass, walked from the largest ordering key down, reaches
// target = ceil(p x total) (formed at the first level): above = mass of the keys > K (< target), leaf = mass of the keys == K
// (above + leaf >= target).  Every thread returns the same values.
template <class Src, class View>
__device__ __forceinline__ void view_select(const SelRow<Src>& r, SelScratch& S, const View& view, float p, u64& target, unsigned& K, u64& above,
                                            u64& leaf) {
  const int tid = threadIdx.x, lane = tid & 63;
  unsigned prefix = 0u;
  u64 acc = 0ull, lf = 0ull;
  for (int level = 0; level < 4; ++level) {
    const int shift = 24 - 8 * level;
    __syncthreads();   // the previous level's readers are done with hist
    if (tid < 256) S.hist[tid] = 0ull;
    __syncthreads();
    int cur = -1;
    u64 w = 0ull;
    for_quads(r, [&](int qd, const unsigned(&k4)[4]) {
#pragma unroll 1
      for (int e = 0; e < 4; ++e) {
        const unsigned k = pick4(k4, e);
        unsigned ok;
        if (4 * qd + e >= r.V || !view(4 * qd + e, k, ok) || (level > 0 && (ok >> (shift + 8)) != prefix)) continue;
        const int d = (int)((ok >> shift) & 255u);
        if (d != cur) {
          if (cur >= 0) atomicAdd(&S.hist[cur], w);
          cur = d, w = 0ull;
        }
        w += mass_of(k, r.zmax);
      }
    });
    if (cur >= 0) atomicAdd(&S.hist[cur], w);
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
    if (level == 0) {
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

// the index at which the mass of the view's tokens with ordering key K, summed in index order, reaches `need` (>= 1): the members of
// the tie group up to it are kept (threads own contiguous ranges, as in tie_cutoff; the members' masses may differ)
template <class Src, class View>
__device__ __forceinline__ int view_tie_cut(const SelRow<Src>& r, SelScratch& S, const View& view, unsigned K, u64 need) {
  const int NT = r.nt, NW = NT >> 6;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, chunk = (r.V + NT - 1) >> (31 - __clz(NT));   // NT: a power of two
  const int lo = tid * chunk < r.V ? tid * chunk : r.V, hi = lo + chunk < r.V ? lo + chunk : r.V;
  u64 own = 0ull;
  for (int v = lo; v < hi; ++v) {
    const unsigned k = r.key(v);
    unsigned ok;
    if (view(v, k, ok) && ok == K) own += mass_of(k, r.zmax);
  }
  u64 incl = own;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 t = shfl_up64(incl, o);
    if (lane >= o) incl += t;
  }
  __syncthreads();   // the readers of hist and cut are done
  if (lane == 63) S.hist[wave] = incl;
  if (tid == 0) S.cut[2] = r.V - 1;
  __syncthreads();
  u64 before = incl - own;
  for (int w = 0; w < NW; ++w)
    if (w < wave) before += S.hist[w];
  if (before < need && need <= before + own) {   // one thread at most: the running mass crosses `need` inside its range
    u64 run = before;
    for (int v = lo; v < hi; ++v) {
      const unsigned k = r.key(v);
      unsigned ok;
      if (!(view(v, k, ok) && ok == K)) continue;
      run += mass_of(k, r.zmax);
      if (run >= need) {
        S.cut[2] = v;
        break;
      }
    }
  }
  __syncthreads();
  return S.cut[2];
}

// src (V scores) -> the truncated choice, by the whole workgroup (1024 threads) on the scratch S.  top_k in [0, V) (0: off), top_p in
// (0, 1] (1: off), tp as the entry point checked it, inv_temp > 0.  (max, sum exp) of the raw row go through choose_row's tree - 256
// threads, a thread's quads in order, a 64-lane butterfly, four waves in order - so the log-probability is the unfiltered choice's
// to the bit.
template <class Src>
__device__ __forceinline__ RowPick truncate_row(SelScratch& S, const Src& src, int V, float inv_temp, int top_k, float top_p, const TruncParams& tp,
                                                DropKey key, unsigned position) {
  const int NT = blockDim.x, NW = NT >> 6;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  SelRow<Src> r;
  r.src = src, r.inv_temp = inv_temp, r.V = V, r.nt = NT, r.resident = V <= SF_LDS_V, r.keys = S.keys, r.zmax = -INFINITY;
  // pass 1: keys to LDS; the largest tempered score
  float zmax = -INFINITY;
  __syncthreads();
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
      const float z = tempered(Src::CONTROLLED ? pick8(cs, j) : pick8(sc, j), inv_temp);
      if (r.resident) S.keys[v0 + NT * j] = key_of(z);
      zmax = fmaxf(zmax, z);
    }
  }
  // ... and (max, sum exp) of the untempered scores, in choose_row's order
  float m = -INFINITY, s = 0.f;
  if (tid < SM_CHOOSE_NT) {
    const int quads = (V + 3) >> 2;
    for (int qd = tid; qd < quads; qd += SM_CHOOSE_NT) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * qd + e < V) lse_merge(m, s, src.raw(4 * qd + e), 1.f);
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
  for (int w = 1; w < SM_CHOOSE_NT / 64; ++w) lse_merge(m, s, S.red[w][0], S.red[w][1]);
  for (int w = 1; w < NW; ++w) zmax = fmaxf(zmax, S.red[w][2]);
  r.zmax = zmax;

  // the prefix stages, as pick_row runs them: the threshold key Kf and the cut inside its tie group
  TruncSet t;
  t.Kf = 0u, t.cut = V, t.log_a = tp.log_a, t.typical = false, t.cbar = 0.f, t.Kt = 0u, t.cut_t = V;
  t.min_mass = 0ull, t.ktop = 0xffffffffu;
  {
    const bool has_k = top_k > 0 && top_k < V, has_p = top_p < 1.f;
    unsigned Kk = 0u;
    long long n_tie = V, n_have = V, k_tie = 0, k_have = 0;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {   // 0: counts for top-k, 1: masses for top-p
      const bool mass = pass == 1;
      if (mass ? !has_p : !has_k) continue;
      unsigned K;
      u64 above, leaf, target = (u64)top_k;
      radix_select(r, S, mass, mass && has_k, Kk, mass && has_k ? (u64)k_tie * mass_of(Kk, zmax) : 0ull, top_p, target, K, above, leaf);
      if (!mass) {
        Kk = t.Kf = K, n_tie = k_tie = (long long)(target - above), n_have = k_have = (long long)leaf;
      } else {
        const u64 mu = mass_of(K, zmax);
        const bool same = has_k && K == Kk;
        const u64 d = mu != 0ull ? mu : 1ull;
        const long long avail = same ? k_tie : (mu != 0ull ? (long long)(leaf / d) : 1);
        const long long need = mu != 0ull ? (long long)((target - above + mu - 1ull) / d) : avail;
        t.Kf = K, n_tie = need < avail ? need : avail, n_have = same ? k_have : avail;
      }
    }
    if (n_tie < n_have) t.cut = tie_cutoff(r, S, t.Kf, (int)(n_tie < 1 ? 1 : n_tie));
  }
  // (min-p is t.log_a: a test on the key, no pass)

  // locally typical: the survivors by |surprise - cbar|, smaller first, until their mass reaches typical_p S
  if (tp.typical_p < 1.f) {
    const TruncSums sums = sum_pass(r, S, t);
    const float cbar = sums.S != 0ull ? (float)(sums.A / (double)sums.S) : 0.f;
    const auto view = [&](int v, unsigned k, unsigned& ok) {
      ok = deviation_key(k, zmax, cbar);
      return in_set(t, zmax, v, k);
    };
    unsigned K;
    u64 above, leaf, target = 0ull;
    view_select(r, S, view, tp.typical_p, target, K, above, leaf);
    const int cut_t = view_tie_cut(r, S, view, K, target - above);
    t.typical = true, t.cbar = cbar, t.Kt = K, t.cut_t = cut_t;
  }
  // epsilon: p_v >= epsilon over the survivors, as mass_v >= ceil(epsilon S)
  if (tp.epsilon > 0.f) {
    const TruncSums sums = sum_pass(r, S, t);
    t.min_mass = (u64)ceil((double)tp.epsilon * (double)sums.S), t.ktop = sums.ktop;
  }
  // eta: p_v >= min(eta, sqrt(eta) exp(-H)), H = log S + A / S the entropy of the survivors (S in units of 2^-40)
  if (tp.eta > 0.f) {
    const TruncSums sums = sum_pass(r, S, t);
    __syncthreads();   // (sum_pass's readers are done with hist)
    if (tid == 0) {
      const double Sd = (double)sums.S;
      const double H = sums.S != 0ull ? log(Sd * (1.0 / (double)SF_ONE)) + sums.A / Sd : 0.0;
      const double thr = fmin((double)tp.eta, sqrt((double)tp.eta) * exp(-H));
      S.hist[64] = (u64)ceil(thr * Sd);
    }
    __syncthreads();
    const u64 mm = S.hist[64];
    t.min_mass = mm > t.min_mass ? mm : t.min_mass, t.ktop = sums.ktop;
  }

  // last pass: Gumbel-max over the kept tokens, a thread takes four neighbours at a time so one Philox call serves them
  float bz = -INFINITY, braw = 0.f;
  int bidx = SM_NOIDX, cnt = 0;
  for_quads(r, [&](int qd, const unsigned(&k4)[4]) {
    bool keep[4], any = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      keep[e] = 4 * qd + e < V && in_set(t, zmax, 4 * qd + e, k4[e]);
      any = any || keep[e];
    }
    if (!any) return;
    unsigned w[4];
    philox4x32_10(position, (unsigned)qd, key.c2, key.c3, key.k0, key.k1, w);
#pragma unroll 1
    for (int e = 0; e < 4; ++e)
      if (e == 0 ? keep[0] : e == 1 ? keep[1] : e == 2 ? keep[2] : keep[3]) {
        best_merge(bz, braw, bidx, z_of(pick4(k4, e)) + gumbel_of(pick4(w, e)), 0.f, 4 * qd + e);
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
  __syncthreads();   // pass 1's readers are done with red
  if (lane == 0) S.red[wave][4] = bz, S.red[wave][5] = __int_as_float(bidx), S.red[wave][6] = __int_as_float(cnt);
  __syncthreads();
  bz = S.red[0][4], bidx = __float_as_int(S.red[0][5]), cnt = __float_as_int(S.red[0][6]);
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
