// Row-block recurrent kernels (gfx950): kernels and launcher template.  Included by vmlmf_rb_*.hip, one translation unit
// per family of instantiations (see vmlmf_rb.hip for the design and the operand images).
#pragma once
#include "vmlmf_launch.h"
#include <cstring>

typedef float f32x4v __attribute__((ext_vector_type(4)));

namespace {

constexpr int RB = 16;        // batch rows per workgroup (the N of the MFMA tiles)
constexpr int RB_WAVES = 4;   // compute waves per workgroup, one per SIMD
constexpr int RB_FLAG_STRIDE = 32;   // unsigned words between two members' epoch words: one 128-byte line each (sixteen words in
                                     // one line serialised the members' publications at the memory side: 272 -> 234 us)

__device__ __forceinline__ f32x4v mfma4(float a, float b, f32x4v c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// ---- bf16 variant (desc.dtype = VMLMF_DT_BF16; BASELINE configs[2] "bf16 MFMA"): the four contraction steps r = 0..3 that
// an fp32 product takes with v_mfma_f32_16x16x4_f32 are ONE v_mfma_f32_16x16x16_bf16 (lane (c, kq) supplies k = 4 kq + r, the same
// pairing), weights are rounded to bf16 once when they are loaded into registers, activations (h, Q, dpre, dQ) where they enter
// an MFMA; accumulators, c, the gate arithmetic and every sum stay fp32.  The big tapes (x-side pre-activations, activated
// gates, dpre) are stored as bf16: 8 bytes per unit and step instead of 16.
typedef short bf16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ unsigned short f2bf(float f) {   // round to nearest even (inputs are finite)
  const unsigned u = __float_as_uint(f);
  return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ float bf2f(unsigned short b) { return __uint_as_float((unsigned)b << 16); }
__device__ __forceinline__ bf16x4 pack_bf4(f32x4v v) {
  return bf16x4{(short)f2bf(v[0]), (short)f2bf(v[1]), (short)f2bf(v[2]), (short)f2bf(v[3])};
}
__device__ __forceinline__ f32x4v unpack_bf4(bf16x4 v) {
  return f32x4v{bf2f((unsigned short)v[0]), bf2f((unsigned short)v[1]), bf2f((unsigned short)v[2]), bf2f((unsigned short)v[3])};
}
template <bool BF> struct RbOp { typedef f32x4v type; };
template <> struct RbOp<true> { typedef bf16x4 type; };
// operand of four contraction steps from four fp32 values
template <bool BF>
__device__ __forceinline__ typename RbOp<BF>::type rb_op(f32x4v v) {
  if constexpr (BF) return pack_bf4(v); else return v;
}
// c += sum_{r < NR} a[r] x b[r]  (NR < 4 only in the last rank tile of a width that is not a multiple of 16; bf16 pads with zeros)
template <bool BF, int NR = 4>
__device__ __forceinline__ f32x4v rb_dot(typename RbOp<BF>::type a, typename RbOp<BF>::type b, f32x4v c) {
  if constexpr (BF) {
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
  } else {
#pragma unroll
    for (int r = 0; r < NR; ++r) c = mfma4(a[r], b[r], c);
    return c;
  }
}
// four-gate tape element of one (row, unit): fp32 = 16 bytes, bf16 = 8
template <bool BF>
__device__ __forceinline__ f32x4v tape_ld4(const float* base, size_t elem) {
  if constexpr (BF) return unpack_bf4(*reinterpret_cast<const bf16x4*>(reinterpret_cast<const char*>(base) + elem * 8));
  else return *reinterpret_cast<const f32x4v*>(base + elem * 4);
}
template <bool BF>
__device__ __forceinline__ void tape_st4(float* base, size_t elem, f32x4v v) {
  if constexpr (BF) *reinterpret_cast<bf16x4*>(reinterpret_cast<char*>(base) + elem * 8) = pack_bf4(v);
  else *reinterpret_cast<f32x4v*>(base + elem * 4) = v;
}

// ---------------------------------------------------------------------------------------------------
// cross-workgroup sum of the K-partial rank-space tiles (clusters of S workgroups, S > 1)
// ---------------------------------------------------------------------------------------------------
typedef __attribute__((address_space(1))) unsigned gu32;
__device__ __forceinline__ void xq_store(float* p, f32x4v v) {   // write-through (sc1): visible at agent scope once vmcnt has counted it
  asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"((gf32*)p), "v"(v) : "memory");
}
// NL loads that bypass this CU's L1, all in flight before ONE wait (the loads and their s_waitcnt in one statement: hipcc
// does not count asm loads).  A load-then-wait per member cost one L2 round trip each: 14 per step in a cluster of 8.
template <int NL>
__device__ __forceinline__ void xq_gather(const float* const (&p)[NL], f32x4v (&v)[NL]) {
  static_assert(NL == 2 || NL == 4 || NL == 8, "chunk of 2, 4 or 8 members");
  if constexpr (NL == 2) {
    asm volatile("global_load_dwordx4 %0, %2, off sc0 sc1\n\tglobal_load_dwordx4 %1, %3, off sc0 sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]) : "v"((const gf32*)p[0]), "v"((const gf32*)p[1]) : "memory");
  } else if constexpr (NL == 4) {
    asm volatile("global_load_dwordx4 %0, %4, off sc0 sc1\n\tglobal_load_dwordx4 %1, %5, off sc0 sc1\n\t"
                 "global_load_dwordx4 %2, %6, off sc0 sc1\n\tglobal_load_dwordx4 %3, %7, off sc0 sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3])
                 : "v"((const gf32*)p[0]), "v"((const gf32*)p[1]), "v"((const gf32*)p[2]), "v"((const gf32*)p[3]) : "memory");
  } else {
    asm volatile("global_load_dwordx4 %0, %8, off sc0 sc1\n\tglobal_load_dwordx4 %1, %9, off sc0 sc1\n\t"
                 "global_load_dwordx4 %2, %10, off sc0 sc1\n\tglobal_load_dwordx4 %3, %11, off sc0 sc1\n\t"
                 "global_load_dwordx4 %4, %12, off sc0 sc1\n\tglobal_load_dwordx4 %5, %13, off sc0 sc1\n\t"
                 "global_load_dwordx4 %6, %14, off sc0 sc1\n\tglobal_load_dwordx4 %7, %15, off sc0 sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7])
                 : "v"((const gf32*)p[0]), "v"((const gf32*)p[1]), "v"((const gf32*)p[2]), "v"((const gf32*)p[3]),
                   "v"((const gf32*)p[4]), "v"((const gf32*)p[5]), "v"((const gf32*)p[6]), "v"((const gf32*)p[7]) : "memory");
  }
}

// sixteen members with ALL loads in flight before the one wait: two asm statements (an asm takes at most 30 operands); the
// second one carries the first one's results as in/out operands, so nothing may read them before its s_waitcnt
__device__ __forceinline__ void xq_gather16(const float* const (&p)[16], f32x4v (&v)[16]) {
  asm volatile("global_load_dwordx4 %0, %8, off sc0 sc1\n\tglobal_load_dwordx4 %1, %9, off sc0 sc1\n\t"
               "global_load_dwordx4 %2, %10, off sc0 sc1\n\tglobal_load_dwordx4 %3, %11, off sc0 sc1\n\t"
               "global_load_dwordx4 %4, %12, off sc0 sc1\n\tglobal_load_dwordx4 %5, %13, off sc0 sc1\n\t"
               "global_load_dwordx4 %6, %14, off sc0 sc1\n\tglobal_load_dwordx4 %7, %15, off sc0 sc1"
               : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7])
               : "v"((const gf32*)p[0]), "v"((const gf32*)p[1]), "v"((const gf32*)p[2]), "v"((const gf32*)p[3]),
                 "v"((const gf32*)p[4]), "v"((const gf32*)p[5]), "v"((const gf32*)p[6]), "v"((const gf32*)p[7]) : "memory");
  asm volatile("global_load_dwordx4 %0, %16, off sc0 sc1\n\tglobal_load_dwordx4 %1, %17, off sc0 sc1\n\t"
               "global_load_dwordx4 %2, %18, off sc0 sc1\n\tglobal_load_dwordx4 %3, %19, off sc0 sc1\n\t"
               "global_load_dwordx4 %4, %20, off sc0 sc1\n\tglobal_load_dwordx4 %5, %21, off sc0 sc1\n\t"
               "global_load_dwordx4 %6, %22, off sc0 sc1\n\tglobal_load_dwordx4 %7, %23, off sc0 sc1\n\ts_waitcnt vmcnt(0)"
               : "=&v"(v[8]), "=&v"(v[9]), "=&v"(v[10]), "=&v"(v[11]), "=&v"(v[12]), "=&v"(v[13]), "=&v"(v[14]), "=&v"(v[15]),
                 "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7])
               : "v"((const gf32*)p[8]), "v"((const gf32*)p[9]), "v"((const gf32*)p[10]), "v"((const gf32*)p[11]),
                 "v"((const gf32*)p[12]), "v"((const gf32*)p[13]), "v"((const gf32*)p[14]), "v"((const gf32*)p[15]) : "memory");
}

struct RbXchg {
  float* xq;        // [nrb][2 parity][S][NMT][64][4] partial tiles
  unsigned* flag;   // [nrb][S][RB_FLAG_STRIDE] epoch words, one 128-byte line each (zeroed before every launch: rb_pack_kernel /
                    // rb_zero_pad_kernel, or a memset node)
  unsigned* err;    // set when a bounded spin gives up
  unsigned* status; // host-visible status word (or NULL)
};

// One exchange.  `tile(m)` is this workgroup's partial of M-tile m for this lane (already summed over its waves), wave w
// handles the M-tiles m = w, w + 4, ...; afterwards full[m] (LDS, [NMT][64][4]) holds the sum over the cluster in a fixed
// order (same bits in every member).  Two workgroup barriers; epoch = step + 1.
// tgcode (or 0): per M-tile the one group whose members hold a non-zero partial of it (RbGeo::tgcode; forward reduce of the
// two-group layers); mygrp: this member's group.  Tiles of the other group are neither stored nor fetched: half the bytes.
struct RbNoHook {
  __device__ __forceinline__ void operator()() const {}
};
// `between`: work of the calling wave that does not depend on the exchange, run after this member's partials are published and
// before it starts to wait for the others' (the step's tape traffic)
template <int NMT, class F, class H = RbNoHook>
__device__ __forceinline__ void rb_cluster_sum(const RbXchg& X, int S, int rbi, int sidx, unsigned epoch, int wave, int lane,
                                               float* full, F&& tile, bool live, unsigned tgcode = 0, int mygrp = 0,
                                               int G = 1, H&& between = RbNoHook()) {
  // `live`: this lane's batch row exists (c < rbl).  Dead lanes move no exchange bytes: with 4 live rows a member's
  // partial is 2 KB instead of 8 and the gather of a cluster of 16 reads 32 KB instead of 128.
  const int par = (int)(epoch & 1u);
  float* mine = X.xq + ((((size_t)rbi * 2 + par) * S + sidx) * NMT) * 256;
#pragma unroll
  for (int i = 0; i < (NMT + 3) / 4; ++i) {
    const int m = wave + 4 * i;
    if (m < NMT) {
      const f32x4v v = tile(m);
      const int tgm = m < 8 ? (int)((tgcode >> (4 * m)) & 15u) - 1 : -1;   // (tiles beyond the eighth - the x ranks of vmlmf_rbx.hip - are fed by every member)
      const bool mine_too = tgm < 0 || tgm == mygrp || S < 2 * G;
      if (live && mine_too) xq_store(mine + (size_t)m * 256 + lane * 4, v);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave drains its write-through stores ...
  __syncthreads();                                   // ... before ONE lane publishes the epoch
  gu32* fl = (gu32*)(X.flag + (size_t)rbi * S * RB_FLAG_STRIDE);   // one 128-byte line per member's word
  if (wave == 0 && lane == 0) __hip_atomic_store(fl + sidx * RB_FLAG_STRIDE, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  between();
  // every wave polls the other members' words itself (lane i < S polls member i): no second barrier for the hand-over
  bool ok = true;
  if (lane < S && lane != sidx) {
    unsigned spins = 0;
    while (__hip_atomic_load(fl + lane * RB_FLAG_STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < epoch) {
      __builtin_amdgcn_s_sleep(1);
      if (++spins > (1u << 22)) {   // bounded: a member that never arrives must not hang the GPU
        ok = false;
        break;
      }
    }
  }
  // a member that never arrived: raise the error word AND poison this step's sum, so that the failure reaches the caller's
  // outputs as NaN instead of as plausible numbers (the bound only exists to keep a broken launch from hanging the GPU)
  const bool lost = !__all(ok);
  if (lost && lane == 0) {
    __hip_atomic_store((gu32*)X.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    vg_raise(X.status, VMLMF_ST_CLUSTER);
  }
  // members are read in chunks of NL (all loads of a chunk in flight together) and added in member order: the same
  // bits in every workgroup of the cluster.  The own partial is read back like the others (it was drained above).
  auto chunked = [&](auto NLc, int m, int lo, int cnt) {
    constexpr int NL = decltype(NLc)::value;
    {
      {
        f32x4v acc = {0.f, 0.f, 0.f, 0.f};
        for (int s0 = lo; s0 < lo + cnt; s0 += NL) {
          const float* src[NL];
          f32x4v v[NL];
#pragma unroll
          for (int j = 0; j < NL; ++j) src[j] = X.xq + ((((size_t)rbi * 2 + par) * S + s0 + j) * NMT + m) * 256 + lane * 4;
          if (live) {
            if constexpr (NL == 16) xq_gather16(src, v);
            else xq_gather<NL>(src, v);
#pragma unroll
            for (int j = 0; j < NL; ++j) acc += v[j];
          }
        }
        if (lost) acc = f32x4v{NAN, NAN, NAN, NAN};
        *reinterpret_cast<f32x4v*>(full + (size_t)m * 256 + lane * 4) = acc;
      }
    }
  };
  // Two-group forward at S = 16 (the PTB group layer): a wave's first two tiles, wave and wave + 4, are each fed by the eight members of
  // one group - their 8 + 8 loads in flight together, ONE L2 round trip instead of two (round 6; same member order of the sums).
  int i0 = 0;
  if constexpr (NMT >= 8) {
    const int m0 = wave, m1 = wave + 4;
    const int g0 = (int)((tgcode >> (4 * m0)) & 15u) - 1, g1 = (int)((tgcode >> (4 * m1)) & 15u) - 1;
    if (S == 16 && G == 2 && g0 >= 0 && g1 >= 0) {
      const float* src[16];
      f32x4v v[16];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        src[j] = X.xq + ((((size_t)rbi * 2 + par) * S + g0 * 8 + j) * NMT + m0) * 256 + lane * 4;
        src[8 + j] = X.xq + ((((size_t)rbi * 2 + par) * S + g1 * 8 + j) * NMT + m1) * 256 + lane * 4;
      }
      f32x4v a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
      if (live) {
        xq_gather16(src, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) a0 += v[j], a1 += v[8 + j];
      }
      if (lost) a0 = a1 = f32x4v{NAN, NAN, NAN, NAN};
      *reinterpret_cast<f32x4v*>(full + (size_t)m0 * 256 + lane * 4) = a0;
      *reinterpret_cast<f32x4v*>(full + (size_t)m1 * 256 + lane * 4) = a1;
      i0 = 2;
    }
  }
#pragma unroll
  for (int i = 0; i < (NMT + 3) / 4; ++i) {
    const int m = wave + 4 * i;
    if (i >= i0 && m < NMT) {
      // members that hold a partial of this tile: all of them, or the S / G members of the one group that feeds it
      const int tgm = m < 8 ? (int)((tgcode >> (4 * m)) & 15u) - 1 : -1;
      const bool one = tgm >= 0 && S >= 2 * G;
      const int cnt = one ? S / G : S, lo = one ? tgm * cnt : 0;
      if (cnt == 16) chunked(std::integral_constant<int, 16>{}, m, lo, cnt);
      else if (cnt >= 8) chunked(std::integral_constant<int, 8>{}, m, lo, cnt);
      else if (cnt == 4) chunked(std::integral_constant<int, 4>{}, m, lo, cnt);
      else chunked(std::integral_constant<int, 2>{}, m, lo, cnt);
    }
  }
  __syncthreads();
}

struct RbFwdArgs {
  const float *gx, *EH, *h0, *c0, *img;
  float *y, *hT, *cT, *gates, *cs, *Qs;
  RbXchg X;
  DropArgs drop;
};
struct RbBwdArgs {
  const float *gates, *cs, *dy, *dhT, *dcT, *EH, *img;
  float *dpre, *dQs, *dh0, *dc0;
  RbXchg X;
  DropArgs drop;
};

// KS = KH / 4 contraction steps of the expansion (KH = padded rank width of one rank-space vector), MT = tiles per wave,
// NMU = M-tiles of the padded rank space a group's units couple to, FLAT = V4 (gates i,f read vector 0, gates o,n vector 1)
// (Two forms built in round 4, parity-green and measured no faster, live in tools/experiments/rb_xfold_and_rb_wgrad.patch: the x side
//  of the pre-activations as a third MFMA product inside this kernel, and the weight-gradient products inside rb_bwd_kernel between
//  a member's publication and its poll - docs/design/row_block_mfma.md has their numbers.)
template <int KS, int MT, int NMU, bool FLAT, int G, bool BF>
__global__ void __launch_bounds__(256) rb_fwd_kernel(VGeo g, RbGeo q, RbFwdArgs a) {
  constexpr int NP = (KS + 3) / 4, NMT = G * NP, NQ = FLAT ? 2 * NP : NP;
  constexpr int NRL = KS - 4 * (NP - 1);   // contraction steps of the last rank tile
  typedef typename RbOp<BF>::type op_t;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, kq = lane >> 4;
  const int S = q.S, NT = g.NT, B = g.B, T = g.T, H = g.H;
  // block -> (row block, member): the S members of a cluster sit 8 blocks apart, i.e. on ONE XCD under the round-robin
  // dispatch this chip uses (block b -> XCD b % 8; a speed matter only: the hand-offs are agent-scope either way)
  const int rbi = ((int)blockIdx.x / (8 * S)) * 8 + ((int)blockIdx.x & 7), sidx = ((int)blockIdx.x >> 3) % S;
  if (rbi >= q.nrb) return;   // grid is rounded up to 8 row blocks (whole workgroups leave: no barrier is skipped)
  // wave slot -> group and tile range
  const int ws = sidx * RB_WAVES + wave, grp = ws / q.WSG, wi = ws - grp * q.WSG;
  const int t0 = wi * MT, nt = min(MT, q.TPGV - t0);   // tiles [t0, t0 + nt) of the group (nt <= 0: a spare wave)
  const int row = rbi * q.rbl + c;
  const bool rok = c < q.rbl && row < B;
  const int rowc = rok ? row : B - 1;
  const bool train = a.gates != nullptr;
  const size_t sstride = (size_t)B * NT;

  extern __shared__ float4 smem4[];
  float* part = reinterpret_cast<float*>(smem4);        // [2][RB_WAVES][NMT][64][4]
  float* full = part + 2 * RB_WAVES * NMT * 256;        // [NMT][64][4]   (clusters only)

  // ---- resident operands
  op_t ua[MT][NMU], va[MT][4][NP];
  float eh[MT][4][4];
  f32x4v h[MT], cst[MT];
  int sbt[MT];
  bool uval[MT][4];
#pragma unroll
  for (int tl = 0; tl < MT; ++tl) {
    const bool on = tl < nt;
    const int tg = on ? t0 + tl : 0, tv = grp * q.TPGV + tg;
    sbt[tl] = grp * 64 * g.W + 16 * tg;
#pragma unroll
    for (int u = 0; u < NMU; ++u) {
      f32x4v w;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = a.img[q.UA + (((size_t)tv * NMT + q.mlist[grp][u]) * 4 + r) * 64 + lane];
        w[r] = on ? v : 0.f;
      }
      ua[tl][u] = rb_op<BF>(w);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int mv = 0; mv < NP; ++mv) {
        f32x4v w;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int s4 = 4 * mv + r;
          const float v = a.img[q.VA + (((size_t)tv * 4 + k) * KS + (s4 < KS ? s4 : 0)) * 64 + lane];
          w[r] = (on && s4 < KS) ? v : 0.f;
        }
        va[tl][k][mv] = rb_op<BF>(w);
      }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int m = 16 * tg + 4 * kq + reg;          // unit index inside the group
      uval[tl][reg] = on && m < g.Hg;
      const int slot = sbt[tl] + 4 * kq + reg, n = grp * g.Hg + (m < g.Hg ? m : 0);
#pragma unroll
      for (int k = 0; k < 4; ++k) eh[tl][k][reg] = on ? a.EH[k * NT + slot] : 0.f;
      const bool ld = uval[tl][reg] && rok;
      h[tl][reg] = (ld && a.h0 != nullptr) ? a.h0[(size_t)rowc * H + n] : 0.f;
      cst[tl][reg] = (ld && a.c0 != nullptr) ? a.c0[(size_t)rowc * H + n] : 0.f;
    }
    if (train && on && rok) *reinterpret_cast<f32x4v*>(a.cs + (size_t)row * NT + sbt[tl] + 4 * kq) = cst[tl];   // slice 0 = c_{-1}
  }
  // partial slots this wave never writes must read as zero
  for (int i = threadIdx.x; i < 2 * RB_WAVES * NMT * 64; i += 256) reinterpret_cast<float4*>(part)[i] = f4zero();
  __syncthreads();

  // gx of step 0
  f32x4v gxn[MT][4];
  auto fetch_gx = [&](int t) {
    const int tc = t < T ? t : T - 1;
#pragma unroll
    for (int tl = 0; tl < MT; ++tl)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        gxn[tl][reg] = tape_ld4<BF>(a.gx, (size_t)tc * sstride + (size_t)rowc * NT + sbt[tl] + 4 * kq + reg);
  };
  fetch_gx(0);
  // the tape of a step: activated gates, c_t (slice t + 1), h_t = y[t] - from the registers that hold them until the next step's
  // gates overwrite them
  // (DEFER: the kernels with one tile per wave - the clusters the automatic choice makes; with more tiles per wave the kept
  // gates would cost the registers the resident weights need)
  constexpr bool DEFER = MT == 1;
  f32x4v pg[MT][4];
  const bool dropping = a.drop.state != nullptr;
  DropKey dkey = {0u, 0u, 0u, 0u};
  if (dropping) dkey = drop_key(a.drop);
  const int dts = drop_tstride(a.drop.period, B);
  auto store_tile = [&](const int ts, const int tl, const f32x4v& ig, const f32x4v& fg, const f32x4v& og, const f32x4v& ng) {
    if (tl < nt && rok) {
      const size_t so = (size_t)ts * sstride + (size_t)row * NT + sbt[tl] + 4 * kq;
      if (train) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) tape_st4<BF>(a.gates, so + reg, f32x4v{ig[reg], fg[reg], og[reg], ng[reg]});
        *reinterpret_cast<f32x4v*>(a.cs + so + sstride) = cst[tl];
      }
      const size_t yo = (size_t)ts * g.syT + (size_t)row * g.syB + grp * g.Hg + 16 * (t0 + tl) + 4 * kq;
      float* yt = a.y + yo;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        if (uval[tl][reg]) yt[reg] = h[tl][reg];
      if (dropping) {   // the copy the next layer / the projection reads (vmlmf_lm.py:438-439), the lane's four units in one call
        float f[4];
        drop_factors(dkey, a.drop.thresh, a.drop.scale, drop_position(dts, ts, row), (unsigned)(sbt[tl] >> 2) + kq, f);
        float* yd = a.drop.yd + yo;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          if (uval[tl][reg]) yd[reg] = h[tl][reg] * f[reg];
      }
    }
  };
  auto store_tape = [&](const int ts) {   // (clusters: every tile of the step, from the kept gates)
#pragma unroll
    for (int tl = 0; tl < MT; ++tl) store_tile(ts, tl, pg[tl][0], pg[tl][1], pg[tl][2], pg[tl][3]);
  };

  for (int t = 0; t < T; ++t) {
    const int buf = t & 1;
    // ---- 1. reduce: this wave's K-partial of the rank-space tiles it couples to
    f32x4v qa[NMU];
#pragma unroll
    for (int u = 0; u < NMU; ++u) qa[u] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tl = 0; tl < MT; ++tl) {
      const op_t hb = rb_op<BF>(h[tl]);
#pragma unroll
      for (int u = 0; u < NMU; ++u) qa[u] = rb_dot<BF>(ua[tl][u], hb, qa[u]);
    }
    float* pw = part + ((size_t)(buf * RB_WAVES + wave) * NMT) * 256;
#pragma unroll
    for (int u = 0; u < NMU; ++u) *reinterpret_cast<f32x4v*>(pw + (size_t)q.mlist[grp][u] * 256 + lane * 4) = qa[u];
    // x-side pre-activations of this step (fetched during the previous one); start the next fetch
    f32x4v gxc[MT][4];
#pragma unroll
    for (int tl = 0; tl < MT; ++tl)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) gxc[tl][reg] = gxn[tl][reg];
    __syncthreads();
    // ---- 2. sum over the waves (and over the cluster) -> the vectors this wave's gates read
    const float* pb = part + (size_t)buf * RB_WAVES * NMT * 256;
    auto wave_sum = [&](int m) {
      f32x4v s = *reinterpret_cast<const f32x4v*>(pb + (size_t)m * 256 + lane * 4);
#pragma unroll
      for (int w = 1; w < RB_WAVES; ++w) s += *reinterpret_cast<const f32x4v*>(pb + ((size_t)w * NMT + m) * 256 + lane * 4);
      return s;
    };
    f32x4v qs[NQ];
    const int mq0 = FLAT ? 0 : grp * NP;   // first M-tile of the vector(s) this wave's gates read
    if (S > 1 && DEFER) {
      // Everything of a step that is not the exchange - the tape of the step before (gates, c, h), the next step's x side - is
      // issued HERE, between this member's publication and its wait for the others: the exchange's two s_waitcnt vmcnt(0)
      // (loads and stores share the counter and may complete out of order: no counted wait) then find nothing foreign
      // outstanding before the publication, and these operations complete while the wave polls.  (With the tape stores at the
      // end of a step the drain before the next publication paid for them: rb_fwd_kernel 248 us with, 205 us without a tape.)
      auto others = [&]() {
        if (t > 0) store_tape(t - 1);
        fetch_gx(t + 1);
      };
      rb_cluster_sum<NMT>(a.X, S, rbi, sidx, (unsigned)(t + 1), wave, lane, full, wave_sum, c < q.rbl, q.tgcode, grp, G, others);
#pragma unroll
      for (int i = 0; i < NQ; ++i) qs[i] = *reinterpret_cast<const f32x4v*>(full + (size_t)(mq0 + i) * 256 + lane * 4);
    } else {
      if (S > 1) {
        rb_cluster_sum<NMT>(a.X, S, rbi, sidx, (unsigned)(t + 1), wave, lane, full, wave_sum, c < q.rbl, q.tgcode, grp, G);
#pragma unroll
        for (int i = 0; i < NQ; ++i) qs[i] = *reinterpret_cast<const f32x4v*>(full + (size_t)(mq0 + i) * 256 + lane * 4);
      } else {
#pragma unroll
        for (int i = 0; i < NQ; ++i) qs[i] = wave_sum(mq0 + i);
      }
      // next step's x side: behind the exchange and ahead of the expansion MFMAs that hide it
      fetch_gx(t + 1);
    }
    // Q[t] for the weight gradients: wave w stores the M-tiles m = w, w + 4, ... (member 0 of a cluster)
    if (train && sidx == 0) {
      for (int m = wave; m < NMT; m += RB_WAVES) {
        const f32x4v s = S > 1 ? *reinterpret_cast<const f32x4v*>(full + (size_t)m * 256 + lane * 4) : wave_sum(m);
        const int j = m / NP, mv = m - j * NP;
        float* qt = a.Qs + (((size_t)t * B + rowc) * G + j) * g.KH;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int rr = 16 * mv + 4 * r + kq;
          if (rok && rr < g.KH) qt[rr] = s[r];
        }
      }
    }
    // ---- 3. expand + gates, tile by tile
    op_t qb[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) qb[i] = rb_op<BF>(qs[i]);
#pragma unroll
    for (int tl = 0; tl < MT; ++tl) {
      f32x4v acc[4];
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) acc[k][reg] = fmaf(h[tl][reg], eh[tl][k][reg], gxc[tl][reg][k]);
#pragma unroll
      for (int mv = 0; mv < NP; ++mv)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (mv < NP - 1) acc[k] = rb_dot<BF>(va[tl][k][mv], qb[(FLAT ? (k >> 1) * NP : 0) + mv], acc[k]);
          else acc[k] = rb_dot<BF, NRL>(va[tl][k][mv], qb[(FLAT ? (k >> 1) * NP : 0) + mv], acc[k]);
        }
      f32x4v ig, fg, og, ng;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        ig[reg] = fast_sigmoid(acc[0][reg]);
        fg[reg] = fast_sigmoid(acc[1][reg]);
        og[reg] = fast_sigmoid(acc[2][reg]);
        ng[reg] = fast_tanh(acc[3][reg]);
        cst[tl][reg] = fmaf(fg[reg], cst[tl][reg], ig[reg] * ng[reg]);
        h[tl][reg] = og[reg] * fast_tanh(cst[tl][reg]);
      }
      // one workgroup per row block: the tile's tape at once; clusters: in the next step's exchange, or after the loop
      if constexpr (DEFER) {
        if (S <= 1) store_tile(t, tl, ig, fg, og, ng);
        else pg[tl][0] = ig, pg[tl][1] = fg, pg[tl][2] = og, pg[tl][3] = ng;
      } else {
        store_tile(t, tl, ig, fg, og, ng);
      }
    }
  }
  if (S > 1 && DEFER) store_tape(T - 1);
#pragma unroll
  for (int tl = 0; tl < MT; ++tl) {
    if (tl < nt && rok) {
      const size_t o = (size_t)row * H + grp * g.Hg + 16 * (t0 + tl) + 4 * kq;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        if (uval[tl][reg]) {
          if (a.hT != nullptr) a.hT[o + reg] = h[tl][reg];
          if (a.cT != nullptr) a.cT[o + reg] = cst[tl][reg];
        }
      }
    }
  }
}

template <int KS, int MT, int NMU, bool FLAT, int G, bool BF>
__global__ void __launch_bounds__(256) rb_bwd_kernel(VGeo g, RbGeo q, RbBwdArgs a) {
  constexpr int NP = (KS + 3) / 4, NMT = G * NP, NJ = FLAT ? 2 : 1;
  typedef typename RbOp<BF>::type op_t;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, kq = lane >> 4;
  const int S = q.S, NT = g.NT, B = g.B, T = g.T, H = g.H;
  // block -> (row block, member): the S members of a cluster sit 8 blocks apart, i.e. on ONE XCD under the round-robin
  // dispatch this chip uses (block b -> XCD b % 8; a speed matter only: the hand-offs are agent-scope either way)
  const int rbi = ((int)blockIdx.x / (8 * S)) * 8 + ((int)blockIdx.x & 7), sidx = ((int)blockIdx.x >> 3) % S;
  if (rbi >= q.nrb) return;   // grid is rounded up to 8 row blocks (whole workgroups leave: no barrier is skipped)
  const int ws = sidx * RB_WAVES + wave, grp = ws / q.WSG, wi = ws - grp * q.WSG;
  const int t0 = wi * MT, nt = min(MT, q.TPGV - t0);
  const int row = rbi * q.rbl + c;
  const bool rok = c < q.rbl && row < B;
  const int rowc = rok ? row : B - 1;
  const bool has_dy = a.dy != nullptr;
  const size_t sstride = (size_t)B * NT;

  extern __shared__ float4 smem4[];
  float* part = reinterpret_cast<float*>(smem4);        // [2][RB_WAVES][NMT][64][4]
  float* full = part + 2 * RB_WAVES * NMT * 256;

  op_t vb[MT][4][NP], ub[MT][NMU];
  float eh[MT][4][4];
  f32x4v dhrec[MT], dcs[MT], ccur[MT];
  int sbt[MT];
  bool uval[MT][4];
#pragma unroll
  for (int tl = 0; tl < MT; ++tl) {
    const bool on = tl < nt;
    const int tg = on ? t0 + tl : 0, tv = grp * q.TPGV + tg;
    sbt[tl] = grp * 64 * g.W + 16 * tg;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int mv = 0; mv < NP; ++mv) {
        f32x4v w;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = a.img[q.VB + ((((size_t)tv * 4 + k) * NP + mv) * 4 + r) * 64 + lane];
          w[r] = on ? v : 0.f;
        }
        vb[tl][k][mv] = rb_op<BF>(w);
      }
#pragma unroll
    for (int u = 0; u < NMU; ++u) {
      f32x4v w;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = a.img[q.UB + (((size_t)tv * NMT + q.mlist[grp][u]) * 4 + r) * 64 + lane];
        w[r] = on ? v : 0.f;
      }
      ub[tl][u] = rb_op<BF>(w);
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int m = 16 * tg + 4 * kq + reg;
      uval[tl][reg] = on && m < g.Hg;
      const int slot = sbt[tl] + 4 * kq + reg, n = grp * g.Hg + (m < g.Hg ? m : 0);
#pragma unroll
      for (int k = 0; k < 4; ++k) eh[tl][k][reg] = on ? a.EH[k * NT + slot] : 0.f;
      const bool ld = uval[tl][reg] && rok;
      dhrec[tl][reg] = (ld && a.dhT != nullptr) ? a.dhT[(size_t)rowc * H + n] : 0.f;
      dcs[tl][reg] = (ld && a.dcT != nullptr) ? a.dcT[(size_t)rowc * H + n] : 0.f;
    }
    ccur[tl] = *reinterpret_cast<const f32x4v*>(a.cs + (size_t)T * sstride + (size_t)rowc * NT + sbt[tl] + 4 * kq);
  }
  for (int i = threadIdx.x; i < 2 * RB_WAVES * NMT * 64; i += 256) reinterpret_cast<float4*>(part)[i] = f4zero();
  __syncthreads();

  // tape of a step: activated gates, c of the step before, upstream dy
  f32x4v gtn[MT][4], cpn[MT], dyn[MT], dfn[MT];
#pragma unroll
  for (int tl = 0; tl < MT; ++tl) dfn[tl] = f32x4v{1.f, 1.f, 1.f, 1.f};
  const bool dropping = a.drop.state != nullptr && has_dy;   // dy is the gradient of the DROPPED copy of y
  DropKey dkey = {0u, 0u, 0u, 0u};
  if (dropping) dkey = drop_key(a.drop);
  const int dts = drop_tstride(a.drop.period, B);
  auto fetch_tape = [&](int t) {
    const int tc = t > 0 ? t : 0;
#pragma unroll
    for (int tl = 0; tl < MT; ++tl) {
      const size_t so = (size_t)tc * sstride + (size_t)rowc * NT + sbt[tl] + 4 * kq;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) gtn[tl][reg] = tape_ld4<BF>(a.gates, so + reg);
      cpn[tl] = *reinterpret_cast<const f32x4v*>(a.cs + so);   // slice tc = c_{tc-1}
      const int tg = tl < nt ? t0 + tl : 0;
      const float* dyt = a.dy + (size_t)tc * g.syT + (size_t)rowc * g.syB + grp * g.Hg + 16 * tg + 4 * kq;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) dyn[tl][reg] = (has_dy && uval[tl][reg]) ? dyt[reg] : 0.f;
      // the factors of the same step into registers of their own, multiplied in where dy is CONSUMED (next iteration): a product
      // here made the compiler wait for the loads above in front of the branch - with dropout off too (rb_bwd_kernel 240 -> 262 us)
      if (dropping) {
        float f[4];
        drop_factors(dkey, a.drop.thresh, a.drop.scale, drop_position(dts, tc, rowc), (unsigned)(sbt[tl] >> 2) + kq, f);
        dfn[tl] = f32x4v{f[0], f[1], f[2], f[3]};
      }
    }
  };
  fetch_tape(T - 1);

  for (int t = T - 1; t >= 0; --t) {
    const int buf = t & 1;
    f32x4v gt[MT][4], cp[MT], dyv[MT];
#pragma unroll
    for (int tl = 0; tl < MT; ++tl) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) gt[tl][reg] = gtn[tl][reg];
      cp[tl] = cpn[tl], dyv[tl] = dropping ? dyn[tl] * dfn[tl] : dyn[tl];
    }
    constexpr bool DEFER = MT == 1;
    if (S <= 1 || !DEFER) fetch_tape(t - 1);   // (clusters with one tile per wave: inside the exchange, below)
    // ---- 1. gate derivatives, dpre to the tape, K-partial of dQ
    f32x4v qa[NJ][NP], ehterm[MT];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int mv = 0; mv < NP; ++mv) qa[j][mv] = f32x4v{0.f, 0.f, 0.f, 0.f};
    f32x4v dpk[MT][4];   // dpre of the step: to the tape inside the exchange (clusters), at once otherwise
#pragma unroll
    for (int tl = 0; tl < MT; ++tl) {
      f32x4v (&dp)[4] = dpk[tl];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const float ig = gt[tl][reg][0], fg = gt[tl][reg][1], og = gt[tl][reg][2], ng = gt[tl][reg][3];
        const float tc = fast_tanh(ccur[tl][reg]);
        const float dh = (rok ? dyv[tl][reg] : 0.f) + dhrec[tl][reg];
        const float dct = fmaf(dh, og * (1.f - tc * tc), dcs[tl][reg]);
        dp[0][reg] = dct * (ng * ig * (1.f - ig));
        dp[1][reg] = dct * (cp[tl][reg] * fg * (1.f - fg));
        dp[2][reg] = dh * (tc * og * (1.f - og));
        dp[3][reg] = dct * (ig * (1.f - ng * ng));
        dcs[tl][reg] = dct * fg;
        ehterm[tl][reg] = (dp[0][reg] * eh[tl][0][reg] + dp[1][reg] * eh[tl][1][reg]) +
                          (dp[2][reg] * eh[tl][2][reg] + dp[3][reg] * eh[tl][3][reg]);
      }
      ccur[tl] = cp[tl];
      if ((S <= 1 || !DEFER) && tl < nt && rok) {
        const size_t de = (size_t)t * sstride + (size_t)row * NT + sbt[tl] + 4 * kq;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) tape_st4<BF>(a.dpre, de + reg, f32x4v{dp[0][reg], dp[1][reg], dp[2][reg], dp[3][reg]});
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const op_t db = rb_op<BF>(dp[k]);   // (bf16: the same rounding the tape stores, so dQ and the weight gradients agree)
#pragma unroll
        for (int mv = 0; mv < NP; ++mv) qa[FLAT ? (k >> 1) : 0][mv] = rb_dot<BF>(vb[tl][k][mv], db, qa[FLAT ? (k >> 1) : 0][mv]);
      }
    }
    float* pw = part + ((size_t)(buf * RB_WAVES + wave) * NMT) * 256;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int mv = 0; mv < NP; ++mv)
        *reinterpret_cast<f32x4v*>(pw + (size_t)((FLAT ? j : grp) * NP + mv) * 256 + lane * 4) = qa[j][mv];
    __syncthreads();
    // ---- 2. sum over waves (and cluster)
    const float* pb = part + (size_t)buf * RB_WAVES * NMT * 256;
    auto wave_sum = [&](int m) {
      f32x4v s = *reinterpret_cast<const f32x4v*>(pb + (size_t)m * 256 + lane * 4);
#pragma unroll
      for (int w = 1; w < RB_WAVES; ++w) s += *reinterpret_cast<const f32x4v*>(pb + ((size_t)w * NMT + m) * 256 + lane * 4);
      return s;
    };
    f32x4v qs[NMU];
    if (S > 1) {
      if constexpr (!DEFER) {
        rb_cluster_sum<NMT>(a.X, S, rbi, sidx, (unsigned)(T - t), wave, lane, full, wave_sum, c < q.rbl);
      } else {
        // the step's dpre stores and the next step's tape loads go out between this member's publication and its wait for the
        // others (see rb_fwd_kernel): nothing foreign is outstanding at the drain before the publication
        auto others = [&]() {
#pragma unroll
          for (int tl = 0; tl < MT; ++tl) {
            if (tl < nt && rok) {
              const size_t de = (size_t)t * sstride + (size_t)row * NT + sbt[tl] + 4 * kq;
#pragma unroll
              for (int reg = 0; reg < 4; ++reg)
                tape_st4<BF>(a.dpre, de + reg, f32x4v{dpk[tl][0][reg], dpk[tl][1][reg], dpk[tl][2][reg], dpk[tl][3][reg]});
            }
          }
          fetch_tape(t - 1);
        };
        rb_cluster_sum<NMT>(a.X, S, rbi, sidx, (unsigned)(T - t), wave, lane, full, wave_sum, c < q.rbl, 0u, 0, 1, others);
      }
#pragma unroll
      for (int u = 0; u < NMU; ++u) qs[u] = *reinterpret_cast<const f32x4v*>(full + (size_t)q.mlist[grp][u] * 256 + lane * 4);
    } else {
#pragma unroll
      for (int u = 0; u < NMU; ++u) qs[u] = wave_sum(q.mlist[grp][u]);
    }
    if (sidx == 0) {   // dQ[t] for the weight gradients
      for (int m = wave; m < NMT; m += RB_WAVES) {
        const f32x4v s = S > 1 ? *reinterpret_cast<const f32x4v*>(full + (size_t)m * 256 + lane * 4) : wave_sum(m);
        const int j = m / NP, mv = m - j * NP;
        float* qt = a.dQs + (((size_t)t * B + rowc) * G + j) * g.KH;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int rr = 16 * mv + 4 * r + kq;
          if (rok && rr < g.KH) qt[rr] = s[r];
        }
      }
    }
    // ---- 3. expand: dh_{t-1} = dQ . U + dpre . eh
#pragma unroll
    for (int tl = 0; tl < MT; ++tl) {
      f32x4v acc = ehterm[tl];
#pragma unroll
      for (int u = 0; u < NMU; ++u) acc = rb_dot<BF>(ub[tl][u], rb_op<BF>(qs[u]), acc);
      dhrec[tl] = acc;
    }
  }
#pragma unroll
  for (int tl = 0; tl < MT; ++tl) {
    if (tl < nt && rok) {
      const size_t o = (size_t)row * H + grp * g.Hg + 16 * (t0 + tl) + 4 * kq;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        if (uval[tl][reg]) {
          if (a.dh0 != nullptr) a.dh0[o + reg] = dhrec[tl][reg];
          if (a.dc0 != nullptr) a.dc0[o + reg] = dcs[tl][reg];
        }
      }
    }
  }
}

template <int KS, int MT, int NMU, bool FLAT, int G, bool BF = false>
int rb_launch(const VGeo& g, const RbGeo& q, const RbIo& io, bool fwd, hipStream_t s) {
  constexpr int NP = (KS + 3) / 4, NMT = G * NP;
  const size_t lds = sizeof(float) * ((size_t)2 * RB_WAVES * NMT * 256 + (q.S > 1 ? (size_t)NMT * 256 : 0));
  const dim3 grid((q.nrb + 7) / 8 * 8 * q.S), block(256);
  RbXchg X;
  X.xq = io.xq, X.flag = io.flag, X.err = io.flag != nullptr ? io.flag + (size_t)q.nrb * q.S * RB_FLAG_STRIDE : nullptr, X.status = io.status;
  if (fwd) {
    RbFwdArgs a;
    memset(&a, 0, sizeof(a));
    a.gx = io.gx, a.EH = io.EH, a.h0 = io.h0, a.c0 = io.c0, a.img = io.img, a.y = io.y, a.hT = io.hT, a.cT = io.cT;
    a.gates = io.gates, a.cs = io.cs, a.Qs = io.Qs, a.X = X, a.drop = io.drop;
    auto kern = rb_fwd_kernel<KS, MT, NMU, FLAT, G, BF>;
    if (lds > 64 * 1024) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kern, grid, block, lds, s, g, q, a);
  } else {
    RbBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.gates = io.gates, a.cs = io.cs, a.dy = io.dy, a.dhT = io.dhT, a.dcT = io.dcT, a.EH = io.EH, a.img = io.img;
    a.dpre = io.dpre, a.dQs = io.dQs, a.dh0 = io.dh0, a.dc0 = io.dc0, a.X = X, a.drop = io.drop;
    auto kern = rb_bwd_kernel<KS, MT, NMU, FLAT, G, BF>;
    if (lds > 64 * 1024) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kern, grid, block, lds, s, g, q, a);
  }
  return (int)hipGetLastError();
}

#define RB_CASE(ks_, mt_, nmu_, flat_, gg_)                                                                \
  if (KS == ks_ && q.MT == mt_ && q.nmu == nmu_ && isflat == flat_ && g.G == gg_)                           \
    return rb_launch<ks_, mt_, nmu_, flat_, gg_>(g, q, io, fwd, s);
#define RB_CASE_BF(ks_, mt_, nmu_)                                                                         \
  if (KS == ks_ && q.MT == mt_ && q.nmu == nmu_ && !isflat && g.G == 1)                                     \
    return rb_launch<ks_, mt_, nmu_, false, 1, true>(g, q, io, fwd, s);
#define RB_CASES_MT_BF(ks_, nmu_) RB_CASE_BF(ks_, 1, nmu_) RB_CASE_BF(ks_, 2, nmu_) RB_CASE_BF(ks_, 3, nmu_) RB_CASE_BF(ks_, 4, nmu_)
#define RB_CASES_MT(ks_, nmu_, flat_, gg_) \
  RB_CASE(ks_, 1, nmu_, flat_, gg_) RB_CASE(ks_, 2, nmu_, flat_, gg_) RB_CASE(ks_, 3, nmu_, flat_, gg_) RB_CASE(ks_, 4, nmu_, flat_, gg_)

}  // namespace
