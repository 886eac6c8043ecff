// Persistent recurrent forward kernel (gfx950).  Included by vmlmf_rec_fwd_kh*.hip (one TU per rank width).
//
// One workgroup owns R batch rows for all T timesteps.  NW compute waves (thread <-> hidden unit, vmlmf_geo.h)
// plus ONE mover wave.  The hidden->hidden factors never leave the compute waves' registers:
//   ve01/ve23[KH]  this unit's rows of V_h as (gate, gate) pairs  -> expansion  pre[k] += Q . ve[k]   (v_pk_fma_f32)
//   ur[KQ]         rotated image of U_h for the 16-lane DPP reduce -> Q = h_{t-1} U_h
// Compute waves, per timestep (ONE workgroup barrier, and NO global memory instruction):
//   1. reduce   v_fmac_f32_dpp row_ror:kk: each lane multiplies the h it receives from its row neighbour
//               with its rotated weight; after 16 steps lane i of a row holds rank (16p+i) summed over the
//               row's 16 units; two permlane swaps add the 4 rows; lanes 0-15 of every wave store the wave
//               partial to LDS (double-buffered by step parity).
//   2. s_waitcnt lgkmcnt(0) ; s_barrier
//   3. expand   sum the CNT wave partials of the source group (independent broadcast ds_read_b128), 4*KH FMAs
//               against ve, add the x-side pre-activation gx[t] (staged in LDS by the mover) and h .* eh,
//               LSTM gates (v_exp/v_rcp), leave (gates, c, h) in an LDS out-stage.
// Mover wave (sits on the SIMD the compute waves leave free for H <= 192; measured: global stores, their
// address arithmetic and the counted vmcnt waits cost the compute waves ~290 of ~1360 cycles per step):
//   streams gx[t+2..t+4] HBM -> registers -> LDS ring, drains the out-stage of step t-1 to y / the tape,
//   and sums the partials once more to store Q[t] for the weight-gradient kernel.
// Replaces the time loop + cell forward: vmlmf.py:300-314 + 78-125, vmlmf_group.py:85-155,
// vmlmf_lm.py:272-280 + 222-269, 166-174 + 97-163.
#include "vmlmf_launch.h"
#include "vmlmf_direct.inc"

constexpr int FWD_NB = 6;   // depth of the gx ring in LDS
// The instantiations with the x-projection wave (XW: one row, at most 192 thread slots, one workgroup per CU by their registers)
// have a ring of FWD_XNB = 8 slots - a power of two: the slot of step t is t & 7, no division by six per wave and step - and lay
// the ring and the out-stage out for FWD_XNTS thread slots whatever NT is: the compute waves' step loop, unrolled over the ring's
// period, then addresses LDS by a per-thread base plus an immediate offset.
constexpr int FWD_XNB = 8;
constexpr int FWD_XNTS = 192;

// Rank-major partials: the instantiations of rec_fwd_kernel with one row, at most 256 thread slots (so at most four compute waves),
// one 16-rank pass and at most four waves per consumer keep the wave partials of the rank reduce as [buffer][rank][wave], one float4
// per rank, as rec3_fwd_kernel and rec3_bwd_kernel do: lane i of a 16-lane row reads rank i's four partials with its one
// ds_read_b128 and adds them with plain adds - no DPP butterfly over the waves.  Columns of waves that do not exist stay zero.
template <int KH, int R, bool FLAT, int MAXT, int CNT>
constexpr bool fwd_rank_major() { return !FLAT && R == 1 && MAXT == 256 && (KH == 8 || KH == 16) && CNT <= 4; }
// floats of the partials' double buffer in LDS
template <int KH, int R, bool FLAT, int MAXT, int CNT>
__host__ __device__ constexpr size_t fwd_part_floats(int NW) {
  return fwd_rank_major<KH, R, FLAT, MAXT, CNT>() ? (size_t)128 : (size_t)2 * R * NW * ((KH + 15) / 16 * 16);
}


// ---------------------------------------------------------------------------------------------------
// x-projection wave.  For a narrow input (I <= 16) and at most three compute waves, wave NW computes the
// non-recurrent half of the pre-activations itself, one step ahead of the recurrence, straight into the LDS ring
// the compute waves read.  With so few inputs the factorised form (x U_x) V_x^T costs more than the dense one,
// so pack_kernel multiplies the x-side out once per call, W_x = diag(d_x) + (U_x V_x^T minus its diagonal),
// and the wave does   gx[t][n][k] = b[k][n] + sum_m x_t[m] W_x[m][k][n]   with W_x for its three thread slots in
// registers and x_t[m] in SGPRs (v_readlane), i.e. 2 I packed FMAs per slot and step.  That removes xproj_kernel
// and the 25 MB it wrote and rec_fwd_kernel read back per launch.  x streams through a small LDS ring with the
// loader's counted-DMA scheme; qx = x U_x (needed by the weight gradients) goes to the storer wave through LDS.
// Not inlined, and it reads the kernel-argument segment itself: inlined, a second role's register pressure
// spills SGPRs into the other waves' per-step loops (measured).
// ---------------------------------------------------------------------------------------------------
template <typename S>
__device__ __forceinline__ void copy_from_kernarg(S* dst, const __attribute__((address_space(4))) char* src) {
  static_assert(sizeof(S) % 4 == 0, "dword-sized argument structs");
  const __attribute__((address_space(4))) int* w = (const __attribute__((address_space(4))) int*)src;
  int tmp[sizeof(S) / 4];
#pragma unroll
  for (unsigned i = 0; i < sizeof(S) / 4; ++i) tmp[i] = w[i];   // scalar loads
  __builtin_memcpy(dst, tmp, sizeof(S));
}
constexpr size_t karg_align8(size_t v) { return (v + 7) & ~(size_t)7; }
constexpr size_t KARG_FWD = karg_align8(sizeof(VGeo));
constexpr size_t KARG_XW = karg_align8(KARG_FWD + sizeof(FwdArgs));

// ---------------------------------------------------------------------------------------------------
// Classifier epilogue (HeadFwd): logits[row][c] = sum_n hT[n] W[c][n] + bias[c] for the row this workgroup owns, by ONE wave,
// from the final out-stage in LDS (published by the last barrier): lanes stride the units, every class is a 64-lane sum in
// a fixed order.  Replaces a launch of head_fwd_kernel (4.5 us + the boundary at the headline shape).  Not inlined and fed
// from the kernel-argument segment: it must not cost the recurrent loop a register.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_total(float v) {   // every lane gets the sum over the 64 lanes (fixed order)
  v = add_ror16<8>(v);
  v = add_ror16<4>(v);
  v = add_ror16<2>(v);
  v = add_ror16<1>(v);
  return rowsum4(v);
}
// With a criterion riding too (CeFwd; `lscr`: 32 floats of LDS nobody else writes any more): the waves leave their logits in
// LDS, meet at a barrier of their own (the mover waves have ended or end without it: a barrier waits for the surviving waves
// only), and wave 0 forms the row's cross-entropy terms; the last row to finish sums the rows' terms in index order.
__device__ __forceinline__ float wave_max64(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __attribute__((noinline)) void head_epilogue(const __attribute__((address_space(4))) char* ka,
                                                        const __attribute__((address_space(3))) float* ch, int row, int wave,
                                                        __attribute__((address_space(3))) float* lscr) {
  // wave w of the NW compute waves owns classes w, w + NW, ... (eight per pass), lanes stride the units: every load of a
  // pass is issued before its first FMA, the accumulators stay in registers (as one wave over all 32 classes the role
  // spilled to scratch and took 9 us)
  // no classifier on this layer: one scalar load and out
  if (((const __attribute__((address_space(4))) int*)(ka + KARG_XW + offsetof(XwArgs, hd) + offsetof(HeadFwd, C)))[0] <= 0) return;
  VGeo g;
  XwArgs xa;
  copy_from_kernarg(&g, ka);
  copy_from_kernarg(&xa, ka + KARG_XW);
  const HeadFwd hd = xa.hd;
  if (hd.C <= 0 || row >= g.B) return;
  const int lane = threadIdx.x & 63, H = g.H, NT = g.NT, C = hd.C, NW = g.NW;
  constexpr int CP = 8;
  for (int c0 = wave; c0 < C; c0 += CP * NW) {
    float acc[CP];
#pragma unroll
    for (int j = 0; j < CP; ++j) acc[j] = 0.f;
    for (int slot = lane; slot < NT; slot += 64) {
      int n;
      const bool valid = vg_slot_unit(g, slot, n);
      const float hv = valid ? ch[slot * 2 + 1] : 0.f;
      const int nc = valid ? n : 0;
      float w[CP];
#pragma unroll
      for (int j = 0; j < CP; ++j) w[j] = hd.W[(size_t)(c0 + j * NW < C ? c0 + j * NW : 0) * H + nc];   // clamped: unconditional loads
#pragma unroll
      for (int j = 0; j < CP; ++j) acc[j] = fmaf(hv, c0 + j * NW < C ? w[j] : 0.f, acc[j]);
    }
#pragma unroll
    for (int j = 0; j < CP; ++j) {
      const float t = wave_total(acc[j]);
      const int c = c0 + j * NW;
      if (lane == 0 && c < C) {
        const float z = t + (hd.bias != nullptr ? hd.bias[c] : 0.f);
        hd.logits[(size_t)row * C + c] = z;
        lscr[c] = z;
      }
    }
  }
}

// The criterion's half of the epilogue (CeFwd), a function of its own so that its registers are not the classes' loop's: called by
// every compute wave behind head_epilogue; without a criterion it is one scalar load and out.
__device__ __attribute__((noinline)) void ce_epilogue(const __attribute__((address_space(4))) char* ka, int row, int wave,
                                                      __attribute__((address_space(3))) float* lscr) {
  if (((const __attribute__((address_space(4))) long long*)(ka + KARG_XW + offsetof(XwArgs, ce) + offsetof(CeFwd, tgt)))[0] == 0) return;
  VGeo g;
  XwArgs xa;
  copy_from_kernarg(&g, ka);
  copy_from_kernarg(&xa, ka + KARG_XW);
  const CeFwd ce = xa.ce;
  const int lane = threadIdx.x & 63, C = xa.hd.C, B = g.B;
  if (C <= 0 || row >= B) return;
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // every class of the row is in lscr
  if (wave != 0) return;
  // ---- the row's cross-entropy terms (ce_fwd_kernel's arithmetic: lse = m + log sum exp(z - m); dz = (exp(z - lse) - onehot) / N)
  const float z = lane < C ? lscr[lane] : -INFINITY;
  const float m = wave_max64(z);
  const float l = m + logf(wave_total(lane < C ? expf(z - m) : 0.f));
  int cnt = 0;   // rows that count: every workgroup counts them itself (integers: any order)
  for (int b = lane; b < B; b += 64) cnt += ce.tgt[b] != ce.ignore ? 1 : 0;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  const float nv = (float)cnt, scale = 1.f / nv;
  const long long t = ce.tgt[row];
  const bool counted = t != ce.ignore, inr = t >= 0 && t < C;
  // (a class index outside [0, C) poisons the loss instead of reading out of bounds, as ce_fwd_kernel does)
  const float rl = counted ? (inr ? l - lscr[inr ? (int)t : 0] : NAN) : 0.f;
  if (ce.dz != nullptr && lane < C) ce.dz[(size_t)row * C + lane] = counted ? scale * (expf(z - l) - (lane == (int)t ? 1.f : 0.f)) : 0.f;
  // ---- the mean over the rows: ONE returning atomic per row, no fence.  Ticket word 0 carries the count of rows that have
  // arrived (bits 63..48) AND the sum of their loss terms in fixed point (bits 46..0, SH fraction bits: integer addition is
  // associative, so the sum is the same in whatever order the rows arrive - run-to-run identical without a pass over the rows
  // and without anything another workgroup wrote having to be visible).  The row whose ticket completes the count holds the whole
  // sum in its own return value.  Terms the fine scale cannot hold go to word 1 FIRST (coarser fixed point for [2048, 2^(36 - lb)),
  // sticky bits for +Inf / beyond and for NaN; that atomic has returned before the row takes its ticket) and set bit 47 of word 0:
  // only then does the last row read word 1.  lb = ceil(log2 B); SH = 35 - lb, i.e. 2^-29 at B = 64; the coarse scale is 2^-10.
  typedef unsigned long long u64;
  int lb = 0;
  while ((1 << lb) < B) ++lb;
  const int SH = 35 - lb;
  const bool fits = rl >= 0.f && rl < 2048.f;   // (false for NaN)
  u64 mine = (u64)1 << 48, old = 0;
  if (fits) mine += (u64)__double2ll_rn((double)rl * (double)((u64)1 << SH));
  if (lane == 0) {
    ce.lse[row] = l;
    if (!fits) {
      const bool nan = rl != rl, big = !nan && !(rl < (float)((u64)1 << (36 - lb)));   // (+Inf included)
      const u64 add1 = nan ? (u64)1 << 63 : (big ? (u64)1 << 62 : (u64)__double2ll_rn((double)rl * 1024.0));
      u64 r1;
      if (nan || big) r1 = __hip_atomic_fetch_or(ce.ticket + 1, add1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else r1 = __hip_atomic_fetch_add(ce.ticket + 1, add1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      // the flag (an OR: it must not carry into the count), issued when word 1 has ANSWERED: the empty asm consumes the returned
      // value in a register (the compiler has to place the s_waitcnt for it here; `r1 & 0` alone folds to a constant and orders
      // nothing) and its memory clobber keeps the two atomics below behind it; ahead of this row's ticket on the same word
      asm volatile("" :: "v"(r1) : "memory");
      __hip_atomic_fetch_or(ce.ticket, (u64)1 << 47, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    old = __hip_atomic_fetch_add(ce.ticket, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  const unsigned olo = __builtin_amdgcn_readfirstlane((unsigned)old), ohi = __builtin_amdgcn_readfirstlane((unsigned)(old >> 32));
  const u64 total = (((u64)ohi << 32) | olo) + mine, flag = total & ((u64)1 << 47);
  if ((unsigned)(total >> 48) != (unsigned)B) return;
  // ---- the last row
  double sum = (double)(total & (((u64)1 << 47) - 1)) / (double)((u64)1 << SH);
  if (flag != 0) {
    const u64 w1 = __hip_atomic_load(ce.ticket + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sum += (double)(w1 & (((u64)1 << 47) - 1)) / 1024.0;
    if ((w1 >> 62) & 1) sum = (double)INFINITY;
    if ((w1 >> 63) & 1) sum = (double)NAN;
  }
  if (lane == 0) {
    ce.loss[0] = (float)(sum / (double)nv);   // 0 / 0 = NaN when every target is ignored, as PyTorch returns
    ce.nvalid[0] = nv;
    __hip_atomic_store(ce.ticket, (u64)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (flag != 0) __hip_atomic_store(ce.ticket + 1, (u64)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

constexpr int XW_SLOTS = 3;     // thread slots per lane (NT <= 192)
constexpr int XW_NB = 12;       // depth of the x ring
constexpr int XW_DIST = 8;      // DMA issue distance in steps: 6 in flight, i.e. ~3.4 us of latency budget (with 2 in
                                // flight the wave stalled on the ~1.2 us DMA latency every step: 0.63 us per step)

// LDS of the role, in floats: x ring, qx hand-over (double-buffered, 32 ranks at most)
__host__ __device__ inline size_t xwave_lds_floats() { return (size_t)XW_NB * 64 + 2 * 32; }

// IM: input width rounded up to a multiple of 4 (the x row is read as float4s); IE: columns that enter the FMA loop (I itself at the
// UCI-HAR width: 18 instead of 24 packed FMAs per slot - once the storer stopped being what the barrier waits for, this wave was:
// 12 -> 10 -> 9 columns 0.1546 -> 0.1534 -> 0.1527 ms per step same-box, (git c7e095c) tools/sessions/r03yf.sh; dropping the then-redundant input
// masks as well gave the gain back: 0.1550)
template <int IM, int IE = IM>
__device__ __attribute__((noinline)) void xwave_role(const __attribute__((address_space(4))) char* ka, float* gxs,
                                                     float* xlds, int row) {
  VGeo g;
  XwArgs xa;
  copy_from_kernarg(&g, ka);
  copy_from_kernarg(&xa, ka + KARG_XW);
  const int lane = threadIdx.x & 63;
  const int I = g.I, H = g.H, NT = g.NT, T = g.T, KX = g.KX;
  // LDS through address-space-3 pointers: generic ones would become flat_load / flat_store in this non-inlined
  // function, which also tick vmcnt and would break the counted waits on the x DMAs
  typedef __attribute__((address_space(3))) float lds_f;
  typedef __attribute__((address_space(3))) f32x4 lds_f4;
  lds_f* xring = (lds_f*)xlds;              // [XW_NB][64]
  lds_f* qxs = xring + XW_NB * 64;          // [2][32]
  lds_f* gxl = (lds_f*)gxs;
  const bool rowok = row < g.B;
  const int rowc = rowok ? row : g.B - 1;

  f32x2 w01[XW_SLOTS][IM], w23[XW_SLOTS][IM], b01[XW_SLOTS], b23[XW_SLOTS];
  float uxc[IM];                            // column `lane` of U_x (lanes < KX)
  bool real[XW_SLOTS];
  if (xa.direct != 0) {
    // direct mode (vmlmf_direct.inc): the compute waves have formed W_x and the bias sums of their own units in LDS ([4 I + 4][NT]
    // behind this role's rings: rows (m, gate), then the four bias rows) - a barrier of the whole workgroup, then this wave picks
    // up the rows of its three thread slots (slots without a unit hold zeros)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    const lds_f* wxl = (const lds_f*)xlds + xwave_lds_floats();
#pragma unroll
    for (int i = 0; i < XW_SLOTS; ++i) {
      const int slot = lane + 64 * i;
      real[i] = slot < NT;
      const int sc = real[i] ? slot : 0;
#pragma unroll
      for (int m = 0; m < IM; ++m) {
        const bool mk = real[i] && m < I;
        const int mc = m < I ? m : 0;
        const float q0 = wxl[(mc * 4 + 0) * NT + sc], q1 = wxl[(mc * 4 + 1) * NT + sc];
        const float q2 = wxl[(mc * 4 + 2) * NT + sc], q3 = wxl[(mc * 4 + 3) * NT + sc];
        w01[i][m] = mk ? f32x2{q0, q1} : f32x2{0.f, 0.f};
        w23[i][m] = mk ? f32x2{q2, q3} : f32x2{0.f, 0.f};
      }
      const float c0 = wxl[(4 * I + 0) * NT + sc], c1 = wxl[(4 * I + 1) * NT + sc], c2 = wxl[(4 * I + 2) * NT + sc], c3 = wxl[(4 * I + 3) * NT + sc];
      b01[i] = real[i] ? f32x2{c0, c1} : f32x2{0.f, 0.f};
      b23[i] = real[i] ? f32x2{c2, c3} : f32x2{0.f, 0.f};
    }
  } else
#pragma unroll
  for (int i = 0; i < XW_SLOTS; ++i) {
    const int slot = lane + 64 * i;
    int n = 0;
    real[i] = slot < NT;
    const bool valid = real[i] && vg_slot_unit(g, slot, n);
    const int sc = real[i] ? slot : 0, nc = valid ? n : 0;
#pragma unroll
    for (int m = 0; m < IM; ++m) {
      const bool mk = valid && m < I;
      const int mc = m < I ? m : 0;
      w01[i][m] = mk ? f32x2{xa.WXD[(size_t)(mc * 4 + 0) * NT + sc], xa.WXD[(size_t)(mc * 4 + 1) * NT + sc]} : f32x2{0.f, 0.f};
      w23[i][m] = mk ? f32x2{xa.WXD[(size_t)(mc * 4 + 2) * NT + sc], xa.WXD[(size_t)(mc * 4 + 3) * NT + sc]} : f32x2{0.f, 0.f};
    }
    b01[i] = valid ? f32x2{xa.BBT[0 * H + nc], xa.BBT[1 * H + nc]} : f32x2{0.f, 0.f};
    b23[i] = valid ? f32x2{xa.BBT[2 * H + nc], xa.BBT[3 * H + nc]} : f32x2{0.f, 0.f};
  }
#pragma unroll
  for (int m = 0; m < IM; ++m) uxc[m] = (m < I && lane < KX && g.foldx == 0) ? xa.UXP[(m < I ? m : 0) * KX + (lane < KX ? lane : 0)] : 0.f;

  // (the row's base pointer once, the time offset advanced by one stride per call - issue() is called for 0, 1, 2, ... in order -
  //  instead of a 64-bit multiply-add per step)
  const float* xrow = xa.x + ((size_t)rowc * g.sxB + (lane < I ? lane : 0));
  size_t xoff = 0;
  auto issue = [&](int ttarget) {   // x row of step ttarget (clamped) -> ring slot; lanes >= I re-read element 0
    __builtin_amdgcn_global_load_lds((gl_cvoid_t*)(xrow + xoff), (lds_void_t*)(xring + (ttarget % XW_NB) * 64), 4, 0, 0);
    if (ttarget + 1 < T) xoff += (size_t)g.sxT;
  };
  auto produce = [&](int t) {       // ring slot of step t <- gx[t]; needs x[t] landed
    // x[m] for every lane: broadcast LDS reads (all lanes read the same address) instead of v_readlane into
    // SGPRs: the scalar write port is shared by the CU's waves, and the compute waves need it for their own
    // 16 readlanes per step
    float sx[IM];
    const lds_f4* xr4 = (const lds_f4*)(xring + (t % XW_NB) * 64);
#pragma unroll
    for (int m4 = 0; m4 < IM / 4; ++m4) {
      const f32x4 v = xr4[m4];
      sx[4 * m4 + 0] = (rowok && 4 * m4 + 0 < I) ? v[0] : 0.f;
      sx[4 * m4 + 1] = (rowok && 4 * m4 + 1 < I) ? v[1] : 0.f;
      sx[4 * m4 + 2] = (rowok && 4 * m4 + 2 < I) ? v[2] : 0.f;
      sx[4 * m4 + 3] = (rowok && 4 * m4 + 3 < I) ? v[3] : 0.f;
    }
    float q = 0.f;                  // qx[lane] = sum_m x[m] U_x[m][lane]  (not needed under the x-fold)
    if (g.foldx == 0) {
#pragma unroll
      for (int m = 0; m < IM; ++m) q = fmaf(sx[m], uxc[m], q);
    }
    if (g.foldx == 0 && lane < KX) qxs[(t & 1) * 32 + lane] = q;
    lds_f* dst = gxl + (size_t)(t & (FWD_XNB - 1)) * FWD_XNTS * 4;
#pragma unroll
    for (int i = 0; i < XW_SLOTS; ++i) {
      if (real[i]) {   // wave-uniform
        f32x2 p01a = b01[i], p01b = f32x2{0.f, 0.f}, p23a = b23[i], p23b = f32x2{0.f, 0.f};
#pragma unroll
        for (int m = 0; m + 1 < IE; m += 2) {
          p01a = pk_fma(splat2(sx[m]), w01[i][m], p01a);
          p23a = pk_fma(splat2(sx[m]), w23[i][m], p23a);
          p01b = pk_fma(splat2(sx[m + 1]), w01[i][m + 1], p01b);
          p23b = pk_fma(splat2(sx[m + 1]), w23[i][m + 1], p23b);
        }
        if constexpr ((IE & 1) != 0) {
          p01a = pk_fma(splat2(sx[IE - 1]), w01[i][IE - 1], p01a);
          p23a = pk_fma(splat2(sx[IE - 1]), w23[i][IE - 1], p23a);
        }
        const f32x2 p01 = p01a + p01b, p23 = p23a + p23b;
        *(lds_f4*)(dst + (size_t)(lane + 64 * i) * 4) = f32x4{p01.x, p01.y, p23.x, p23.y};
      }
    }
  };
  for (int s0 = 0; s0 < XW_DIST; ++s0) issue(s0);
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(XW_DIST - 1) : "memory");   // x[0] has landed
  produce(0);
  wait_vm_barrier<XW_DIST - 2>();          // barrier(0); x[1] has landed
  for (int t = 0; t < T; ++t) {            // segment t: produce step t + 1 while the recurrence consumes step t
    issue(t + XW_DIST);
    produce(t + 1);
    wait_vm_barrier<XW_DIST - 2>();        // barrier(t+1); x[t+2] has landed
  }
}

// XW: wave NW is the x-projection wave (xwave_role) instead of the gx loader
// (the ablation switches and s_memtime stamps the design notes quote live in tools/experiments/ablation_switches.patch)
template <int KH, int R, bool FLAT, int MAXT, int CNT, bool XW = false>
__global__ void __launch_bounds__(VG_REC_BOUNDS) rec_fwd_kernel(VGeo g, FwdArgs a, XwArgs xwargs) {
  constexpr int NP = (KH + 15) / 16, KQ = NP * 16, NC = KH / 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NT = g.NT, NW = g.NW, W = g.W, H = g.H, B = g.B, T = g.T;
  const bool mover = tid >= NT;
  const bool train = a.gates != nullptr;
  const size_t sstride = (size_t)g.Bp * NT;   // slots per time slice of the slot-padded buffers

  extern __shared__ float4 smem4[];
  constexpr bool RM = fwd_rank_major<KH, R, FLAT, MAXT, CNT>();
  float* part = reinterpret_cast<float*>(smem4);           // [2][R][NW][KQ]; RM: [2][16 ranks][4 waves]
  static_assert(!XW || (R == 1 && MAXT == 256 && !FLAT), "the x-projection wave's instantiations");
  constexpr int NB = XW ? FWD_XNB : FWD_NB;                // depth of the gx ring
  const int NTS = XW ? FWD_XNTS : NT;                      // thread slots a ring slot / an out-stage buffer is laid out for
  float* gxs = part + fwd_part_floats<KH, R, FLAT, MAXT, CNT>(NW);   // [NB][R][NTS][4]
  // out-stage, structure of arrays: [2][ R x NT x (i f o n) | R x NT x (c h) | R x NT x 2 spare ].  As one 32-byte record per
  // thread the 16-byte and 8-byte accesses hit every bank 2 and 4 times (rocprofv3: 42 % of the kernel's LDS cycles were
  // bank conflicts, profiles/r02_pmc_util.json); contiguous 16- and 8-byte elements are conflict-free
  float* outs = gxs + NB * R * NTS * 4;
  float* zero4 = outs + 2 * R * NTS * 8 + 256;             // 4 zero floats (after the spare kilobyte)
  if (tid < 4) zero4[tid] = 0.f;

  if (mover) {
    // ------------------------------------------------------------------ the two mover waves
    // LOADER (wave NW): only LDS-DMAs (global_load_lds, no registers), so its counted vmcnt is exact.  The gx
    // ring slot of step s is issued during segment s-DIST, confirmed landed one segment before it is needed
    // (all but the newest DEPTH*NDMA operations complete) and read by the compute waves after barrier(s).
    // MAXS DMAs per row are always issued (dummy ones go to a spare LDS kilobyte) so that the vmcnt immediate is
    // a compile-time constant.
    // STORER (wave NW+1): drains the out-stage of step t-1 to y / the tape and stores Q[t]; it never waits on
    // vmcnt, so HBM write latency (~1 us, longer than a step) is never on anybody's critical path.
    constexpr int MAXS = MAXT / 64;
    constexpr int NDMA = R * MAXS;
    constexpr int DEPTH = (2 * NDMA <= 63) ? 2 : 1;      // segments of DMAs allowed in flight
    constexpr int DIST = DEPTH + 2;                      // issue distance in steps
    static_assert(DIST < NB && (!XW || (NB & (NB - 1)) == 0), "gx ring too shallow");
    float* spare = outs + 2 * R * NTS * 8;   // 256 floats
    int row[R];
    bool rok[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      row[r] = blockIdx.x * R + r;
      rok[r] = row[r] < B;
    }
    if (wave == NW) {
      if constexpr (XW) {   // this wave computes the x-projection instead of loading it
        const __attribute__((address_space(4))) char* ka =
            (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
        float* xlds = zero4 + 4;
        switch ((g.I + 3) / 4) {
          case 1: xwave_role<4>(ka, gxs, xlds, row[0]); break;
          case 2: xwave_role<8>(ka, gxs, xlds, row[0]); break;
          case 3:
            if (g.I == 9) xwave_role<12, 9>(ka, gxs, xlds, row[0]);   // UCI-HAR: nine real columns of the twelve
            else if (g.I == 10) xwave_role<12, 10>(ka, gxs, xlds, row[0]);
            else xwave_role<12>(ka, gxs, xlds, row[0]);
            break;
          default: xwave_role<16>(ka, gxs, xlds, row[0]); break;
        }
        return;
      }
      auto issue = [&](int ttarget) {
        const int tc = ttarget < T ? ttarget : T - 1;
        float* dst = gxs + (size_t)(ttarget % NB) * R * NTS * 4;
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int i = 0; i < MAXS; ++i) {
            const bool real = i < NW;
            const int i0 = real ? i : 0;
            dma16(a.gx + ((size_t)tc * sstride + (size_t)row[r] * NT + lane + 64 * i0) * 4,
                  real ? dst + ((size_t)r * NTS + 64 * i0) * 4 : spare);
          }
      };
      for (int s0 = 0; s0 < DIST; ++s0) issue(s0);           // targets 0 .. DIST-1
      wait_vm_barrier<(DIST - 2) * NDMA>();                  // barrier(0): targets 0 and 1 have landed
      for (int t = 0; t < T; ++t) {                          // segment t, between barrier(t) and barrier(t+1)
        issue(t + DIST);
        wait_vm_barrier<DEPTH * NDMA>();                     // target t+2 has landed
      }
      return;
    }
    // The storer shares SIMD 0 with compute wave 0 and is the wave every barrier waits for (busy 1034 of 1137 ticks per step,
    // ~350 ticks behind the compute waves): with the higher issue priority it arrives earlier - rec_fwd_kernel 71.5 -> 69.2 us,
    // 0.1606 -> 0.1576 ms per step same-box ((git c7e095c) tools/sessions/r03v.sh); the compute waves at priority 3 instead: 80 us.
    __builtin_amdgcn_s_setprio(3);
    if (a.prog != nullptr && lane < R && rok[lane < R ? lane : 0])   // the backward rows' progress words (WRide) start at zero
      a.prog[(size_t)(blockIdx.x * R + lane) * WR_PROG_STRIDE] = 0u;
    // per-lane constants of the storer, computed once: slot validity, offsets, and the Q element it owns
    // Per-lane BYTE offsets (32 bit) against wave-uniform base pointers: the stores then use the scalar-base +
    // vector-offset form and the per-step address arithmetic is scalar.  (With 64-bit per-lane pointers this wave
    // issued ~200 vector instructions per step, on a SIMD it shares with a compute wave.)
    bool sv[R][MAXS];
    unsigned so_[R][MAXS], yo_[R][MAXS];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int i = 0; i < MAXS; ++i) {
        const int slot = lane + 64 * (i < NW ? i : 0);
        int n;
        const bool valid = vg_slot_unit(g, slot, n);
        sv[r][i] = i < NW && valid && rok[r];
        so_[r][i] = (unsigned)(row[r] * NT + slot) * 4u;                          // bytes into a [Bp][NT] float slice
        yo_[r][i] = (unsigned)((rok[r] ? row[r] : 0) * g.syB + n) * 4u;           // bytes into y[t]
      }
    // Q[ts][j][rr] = sum over the W waves of source group (j + s) mod G; this lane owns up to 2 elements
    constexpr int QE = 2;
    bool qv[QE];
    unsigned qsrc[QE], qdst[QE];
#pragma unroll
    for (int q = 0; q < QE; ++q) {
      const int e = lane + 64 * q;
      const int GK = g.G * KH;
      const bool in = e < R * GK;
      const int ec = in ? e : 0;
      const int r = ec / GK, jr = ec - r * GK, j = jr / KH, rr = jr - j * KH;
      const int s = (g.G == 2 && rr >= g.off1) ? 1 : 0;
      const int w0 = ((j + s) % g.G) * W;
      qv[q] = in && train && (blockIdx.x * R + r) < B;
      qsrc[q] = RM ? (unsigned)(rr * 4 + w0) : (unsigned)((r * NW + w0) * KQ + rr);
      qdst[q] = (unsigned)((blockIdx.x * R + r) * GK + jr);
    }
    // One segment of the storer: out-stage of step td -> y / tape (td < 0: nothing yet), Q[tq] and, with the
    // x-projection wave, qx[tq].  EVERY LDS read of the segment is issued before the first global store: read ->
    // wait -> store per slot, one slot after the other, put four to five LDS latencies in series and made this wave
    // (1400 cycles per step) the one everybody waited for at the barrier (the compute waves need ~920).
    const float* qxs = zero4 + 4 + XW_NB * 64;
    const bool qx_out = XW && train && g.foldx == 0 && rok[0] && lane < g.KX;
    constexpr bool SAFE_ST = FLAT && MAXT == 512;   // (vmlmf_device.h, hazard 2: what tools/check_asm_hazards.py flags without it)
    auto segment = [&](int td, int tq) {
      // raised for the LDS reads only: with the priority up for the whole segment the storer reaches the barrier ~110 ticks AHEAD of
      // the compute waves and compute wave 0, which shares its SIMD, becomes the last to arrive (profiles/r03_z_rec_probe_xwave_final.txt);
      // back to normal before the stores: 0.1566 -> 0.1554 ms per step same-box ((git c7e095c) tools/sessions/r03yc.sh)
      __builtin_amdgcn_s_setprio(3);
      const int tdc = td < 0 ? 0 : td, tqc = tq < 0 ? 0 : tq;
      const float* src = outs + (size_t)(tdc & 1) * R * NTS * 8;
      const float* qsrc_ = part + (RM ? (size_t)(tqc & 1) * 64 : (size_t)(tqc & 1) * R * NW * KQ);
      float4 g4[R][MAXS];
      float2 ch[R][MAXS];
      float v[QE][MAXS];
      float qxv = 0.f;
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int i = 0; i < MAXS; ++i) {
          const int slot = lane + 64 * (i < NW ? i : 0);
          g4[r][i] = ld4(src + ((size_t)r * NTS + slot) * 4);
          ch[r][i] = *reinterpret_cast<const float2*>(src + (size_t)R * NTS * 4 + ((size_t)r * NTS + slot) * 2);
        }
#pragma unroll
      for (int q = 0; q < QE; ++q)
#pragma unroll
        for (int w = 0; w < MAXS; ++w) v[q][w] = qsrc_[qsrc[q] + (w < W ? w : 0) * (RM ? 1 : KQ)];
      if constexpr (XW) qxv = qxs[(tqc & 1) * 32 + (lane & 31)];
      __builtin_amdgcn_s_setprio(0);
      if (td >= 0) {
        char* gt = reinterpret_cast<char*>(a.gates + (size_t)td * sstride * 4);   // wave-uniform bases
        char* ct = reinterpret_cast<char*>(a.cs + (size_t)(td + 1) * sstride);
        char* yt = reinterpret_cast<char*>(a.y + (size_t)td * g.syT);
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
          for (int i = 0; i < MAXS; ++i) {
            if (i < NW) {
              if (train) {   // (streamed: the non-temporal hint where the store needs no hazard padding, vmlmf_device.h)
                st4_sv<SAFE_ST, !SAFE_ST>(gt, 4u * so_[r][i], g4[r][i]);
                st1_sv<SAFE_ST, !SAFE_ST>(ct, so_[r][i], ch[r][i].x);
              }
              if (sv[r][i]) st1_sv<SAFE_ST, !SAFE_ST>(yt, yo_[r][i], ch[r][i].y);
            }
          }
        }
      }
      if (tq >= 0) {
        const float* qt = a.Qs + (size_t)tq * B * g.G * KH;
#pragma unroll
        for (int q = 0; q < QE; ++q) {
          if (qv[q]) {
            float acc = 0.f;
#pragma unroll
            for (int w = 0; w < MAXS; ++w) acc += w < W ? v[q][w] : 0.f;   // same order as the compute waves' sum
            st1_sv<SAFE_ST>(qt, 4u * qdst[q], acc);
          }
        }
        if constexpr (XW) {
          if (qx_out) st1_sv<SAFE_ST>(a.qxw + (size_t)tq * B * g.KX, 4u * (unsigned)(row[0] * g.KX + lane), qxv);
        }
      }
    };
    if constexpr (XW) {
      if ((a.xwave & 2) != 0) asm volatile("s_barrier" ::: "memory");   // direct mode: the barrier that publishes the compute waves' W_x
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // barrier(0)
    for (int t = 0; t < T; ++t) {   // segment t
      segment(t - 1, t);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // barrier(t+1): LDS reads done, stores in flight
    }
    segment(T - 1, -1);
    return;
  }

  // -------------------------------------------------------------------- compute waves
  const int grp = tid / (64 * W);
  const int m = tid - grp * 64 * W;
  const bool valid = m < g.Hg;
  const int n = grp * g.Hg + (valid ? m : 0);

  // register-resident weights; gate pairs (i,f) and (o,n) are packed for v_pk_fma_f32
  f32x2 ve01[KH], ve23[KH], eh01, eh23;
  float ur[KQ];
  bool direct = false;
  // (kernels with the x-projection wave only: they run one workgroup per CU whatever the compute waves' register count)
  constexpr bool CAN_DIRECT = XW && KH <= 16 && !FLAT && R == 1;
  if constexpr (CAN_DIRECT) direct = (a.xwave & 2) != 0;   // (wave-uniform)
  if (direct) {
    // direct mode (vmlmf_direct.inc): VE / UR / EH point at the reference's own v_h (4H, KH), u_h (H, KH), dia_h (1, H)
    if constexpr (CAN_DIRECT) {
      // every load of the prologue is issued before the first value is used (the unit's rows of v_h, u_h, v_x, its biases and vm
      // entries): one memory latency
      float vr[4][16], ur0[16], bs[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) dr_load_row<KH>(a.VE, (size_t)k * H + n, valid, vr[k]);
      dr_load_row<KH>(a.UR, (size_t)n, valid, ur0);
      {
        float bxv[4], bhv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) bxv[k] = xwargs.BBT[(size_t)k * H + n], bhv[k] = xwargs.BH[(size_t)k * H + n];
#pragma unroll
        for (int k = 0; k < 4; ++k) bs[k] = bxv[k] + bhv[k];
      }
      const float dh = a.EH[n], dxv = xwargs.DX[n < g.I ? n : 0];
      const float vf = valid ? 1.f : 0.f;
      // first the x side of this unit for the x-projection wave - W_x[m][gate] and the bias sums into LDS (dr_wx_unit; the v_x rows'
      // registers are free again afterwards) - then this thread's own images; the barrier behind them publishes W_x.
      // (One block per x-rank width: rows filled in two branches of one array went to scratch memory.)
      float* wxl = zero4 + 4 + xwave_lds_floats();
      auto xside = [&](auto kxc) {
        constexpr int KX_ = decltype(kxc)::value;
        float vx[4][16];
#pragma unroll
        for (int k = 0; k < 4; ++k) dr_load_row<KX_>(xwargs.WXD, (size_t)k * H + n, valid, vx[k]);
        dr_wx_unit<KX_>(vx, bs, dxv, xwargs.UXP, g.I, NT, n, vf, tid, wxl);
      };
      if (g.KX == 16) xside(std::integral_constant<int, 16>{});
      else xside(std::integral_constant<int, 8>{});
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int rr = 0; rr < KH; ++rr) ve01[rr] = f32x2{vr[0][rr], vr[1][rr]}, ve23[rr] = f32x2{vr[2][rr], vr[3][rr]};
      eh01 = f32x2{(dh - dr_chain<KH>(ur0, vr[0])) * vf, (dh - dr_chain<KH>(ur0, vr[1])) * vf};
      eh23 = f32x2{(dh - dr_chain<KH>(ur0, vr[2])) * vf, (dh - dr_chain<KH>(ur0, vr[3])) * vf};
      // rotated image of the rank reduce: ur[kk] = U_h[unit this lane RECEIVES FROM under row_ror:kk][rank = this lane's place i in
      // its row].  The source lane (place i + d kk) finds that entry in its own row at rank (its place - d kk): it picks it there
      // (dr_at, through its LDS slot in the not yet used out-stage) and row_ror:kk delivers it.
      float* scr = outs + (size_t)tid * DR_SCR_FLOATS;
      dr_put(scr, ur0);
      const int li = lane & 15, dn = 16 - dr_ror_dir(lane);   // (- d mod 16)
      sfor<16>([&](auto kk) {
        constexpr int K = decltype(kk)::value;
        ur[K] = ror16<K>(dr_at(scr, li + dn * K));
      });
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // W_x is published (every wave of a direct launch takes this barrier once)
    }
  } else {
#pragma unroll
    for (int rr = 0; rr < KH; ++rr) {
      ve01[rr] = f32x2{a.VE[(size_t)(0 * KH + rr) * NT + tid], a.VE[(size_t)(1 * KH + rr) * NT + tid]};
      ve23[rr] = f32x2{a.VE[(size_t)(2 * KH + rr) * NT + tid], a.VE[(size_t)(3 * KH + rr) * NT + tid]};
    }
    eh01 = f32x2{a.EH[0 * NT + tid], a.EH[1 * NT + tid]};
    eh23 = f32x2{a.EH[2 * NT + tid], a.EH[3 * NT + tid]};
#pragma unroll
    for (int j = 0; j < KQ; ++j) ur[j] = a.UR[(size_t)j * NT + tid];
  }

  // LDS offset (floats) of the first contributing wave's partial for each 4-rank chunk
  int pb[NC];
  int pb2[FLAT ? NC : 1];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int s = (g.G == 2 && 4 * c >= g.off1) ? 1 : 0;
    const int q0 = FLAT ? 0 : grp;
    pb[c] = (((q0 + s) % g.G) * W) * KQ + 4 * c;
    if (FLAT) pb2[c] = (((1 + s) % g.G) * W) * KQ + 4 * c;
  }

  // Cross-wave sum of the partials, cooperative form (FASTQ): lane i of every 16-lane row reads ONE float4,
  // partial of wave (i / NC), chunk (i % NC); a DPP butterfly over the row adds the waves; v_readlane moves
  // the KH totals into SGPRs, which the expansion FMAs read directly.  One ds_read_b128 per wave instead of
  // NC*CNT (the redundant broadcast reads cost ~36 KB of LDS traffic per step at H=180).
  // FASTQ64: the same with all 64 lanes when (chunks rounded up to a power of two) x waves does not fit a 16-lane row
  // (ranks 17-32, or more than four waves): lane l reads the partial of wave l / NCP, chunk l % NCP, the row butterfly
  // adds the waves inside a row and rowsum4 adds the four rows.  Without it a thread read NC*CNT float4 broadcasts
  // per step (24 at H = 256, rank 24: ~100 KB of LDS traffic per step and workgroup).
  constexpr int NCP = NC <= 2 ? 2 : (NC <= 4 ? 4 : 8);
  constexpr bool FASTQ16 = !FLAT && NC == NCP && NC * CNT <= 16;
  constexpr bool FASTQ64 = !FLAT && !FASTQ16 && NC <= 8 && NCP * CNT <= 64;
  // FLATQ (V4): a unit reads BOTH rank-space vectors (gates i,f from Q[0], o,n from Q[1]); lanes 0-31 sum the waves
  // that feed Q[0], lanes 32-63 those of Q[1] (row butterfly, then rowsum2 over the two rows of a half).
  constexpr bool FLATQ = FLAT && NC <= 8 && NCP * CNT <= 32;
  constexpr bool FASTQ = FASTQ16 || FASTQ64 || FLATQ;
  int rdoff = 0;
  {
    const int li = FLATQ ? (lane & 31) : (FASTQ64 ? lane : (lane & 15)), cc = li % NCP, w = li / NCP;
    const int ccl = cc < NC ? cc : 0;
    const int s = (g.G == 2 && 4 * ccl >= g.off1) ? 1 : 0;
    const int q0 = FLATQ ? (lane >> 5) : grp;   // which rank-space vector this lane helps to sum
    rdoff = (w < CNT && cc < NC) ? ((((q0 + s) % g.G) * W + w) * KQ + 4 * cc) : -1;
  }
  // RM: lane i of a row sums rank i.  With two groups (then CNT <= 2) the rank may come from the second group's waves, columns
  // W .. 2 W - 1 (the choice per 4-rank chunk, as above); with one group the columns past NW are zero, once and for all.
  static_assert(!RM || FASTQ16, "rank-major partials replace the 16-lane butterfly");
  bool rmsel = false;
  if constexpr (RM) {
    const int li = lane & 15;
    const int s = (g.G == 2 && 4 * (li >> 2) >= g.off1) ? 1 : 0;
    rmsel = ((grp + s) % g.G) != 0;
    if (wave == 0 && lane < 16)
      for (int w = NW; w < 4; ++w) part[lane * 4 + w] = 0.f, part[64 + lane * 4 + w] = 0.f;
  }

  float h[R], c[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = blockIdx.x * R + r;
    const bool ok = valid && row < B;
    const int rowc = row < B ? row : B - 1;
    h[r] = (ok && a.h0 != nullptr) ? a.h0[(size_t)rowc * H + n] : 0.f;
    c[r] = (ok && a.c0 != nullptr) ? a.c0[(size_t)rowc * H + n] : 0.f;
    if (train) a.cs[(size_t)row * NT + tid] = c[r];  // tape slice 0 = c_{-1}
  }

  // One time step t, named by what it addresses: ring = the gx ring slot of step t, buf = t & 1.
  auto step = [&](const int ring, const int buf) __attribute__((always_inline)) {
    // ---- 1. rank-space reduce of h_{t-1}
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float hv = h[r];
      dpp_fence(hv);
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        float a0 = 0.f, a1 = 0.f;
        fmac_ror_x16(a0, a1, hv, &ur[p * 16]);
        const float s = rowsum4(a0 + a1);
        if constexpr (RM) {
          if (lane < 16) part[buf * 64 + lane * 4 + wave] = s;
        } else {
          if (lane < 16) part[((buf * R + r) * NW + wave) * KQ + p * 16 + lane] = s;
        }
      }
    }
    // ---- 2. barrier(t): partials of step t, gx ring slot t and the previous out-stage are published
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    // ---- 3. expand + gates
    const float* gxt = gxs + (size_t)ring * R * NTS * 4;
    float* ot = outs + (size_t)buf * R * NTS * 8;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float* src = part + (size_t)(buf * R + r) * NW * KQ;
      const float4 gx4 = ld4(gxt + ((size_t)r * NTS + tid) * 4);
      float4 q[NC], q2[FLAT ? NC : 1];
      if constexpr (RM) {
        // the sum in the order the butterfly had: (w0 + w2) + (w1 + w3), absent waves zero (class_sum16<4>: first the lane eight
        // places on, then the one four places on - the lanes of waves 2 and then 1 / 3 under either direction of the rotation)
        const float4 v = ld4(part + buf * 64 + (lane & 15) * 4);
        float tot;
        if constexpr (CNT >= 3) {
          tot = (v.x + v.z) + (v.y + v.w);
        } else {
          const float a0 = CNT == 1 ? (rmsel ? v.y : v.x) : (rmsel ? v.z : v.x);
          const float a1 = CNT == 1 ? 0.f : (rmsel ? v.w : v.y);
          tot = (a0 + 0.f) + (a1 + 0.f);
        }
#pragma unroll
        for (int cc = 0; cc < NC; ++cc)
          q[cc] = make_float4(bcast_lane(tot, 4 * cc), bcast_lane(tot, 4 * cc + 1), bcast_lane(tot, 4 * cc + 2), bcast_lane(tot, 4 * cc + 3));
      } else if constexpr (FASTQ) {
        const float4 v = ld4(rdoff >= 0 ? src + rdoff : zero4);
        float sx = class_sum16<NCP>(v.x), sy = class_sum16<NCP>(v.y);
        float sz = class_sum16<NCP>(v.z), sw = class_sum16<NCP>(v.w);
        if constexpr (FASTQ64) sx = rowsum4(sx), sy = rowsum4(sy), sz = rowsum4(sz), sw = rowsum4(sw);
        if constexpr (FLATQ) sx = rowsum2(sx), sy = rowsum2(sy), sz = rowsum2(sz), sw = rowsum2(sw);
#pragma unroll
        for (int cc = 0; cc < NC; ++cc)
          q[cc] = make_float4(bcast_lane(sx, cc), bcast_lane(sy, cc), bcast_lane(sz, cc), bcast_lane(sw, cc));
        if constexpr (FLATQ) {
#pragma unroll
          for (int cc = 0; cc < NC; ++cc)
            q2[cc] = make_float4(bcast_lane(sx, 32 + cc), bcast_lane(sy, 32 + cc), bcast_lane(sz, 32 + cc), bcast_lane(sw, 32 + cc));
        }
      }
#pragma unroll
      for (int cc = 0; cc < (FASTQ ? 0 : NC); ++cc) {
        float4 v[CNT];
#pragma unroll
        for (int w = 0; w < CNT; ++w) v[w] = ld4(src + pb[cc] + w * KQ);
        q[cc] = v[0];
#pragma unroll
        for (int w = 1; w < CNT; ++w) q[cc] = f4add(q[cc], v[w]);
        if (FLAT) {
#pragma unroll
          for (int w = 0; w < CNT; ++w) v[w] = ld4(src + pb2[cc] + w * KQ);
          q2[cc] = v[0];
#pragma unroll
          for (int w = 1; w < CNT; ++w) q2[cc] = f4add(q2[cc], v[w]);
        }
      }
      const f32x2 hh = splat2(h[r]);
      // two accumulators per gate pair: shorter dependent chains
      f32x2 p01a = pk_fma(hh, eh01, f32x2{gx4.x, gx4.y}), p01b = f32x2{0.f, 0.f};
      f32x2 p23a = pk_fma(hh, eh23, f32x2{gx4.z, gx4.w}), p23b = f32x2{0.f, 0.f};
#pragma unroll
      for (int cc = 0; cc < NC; ++cc) {
        const float4 qa = q[cc];
        const float4 qb = FLAT ? q2[cc] : q[cc];
        p01a = pk_fma(splat2(qa.x), ve01[4 * cc + 0], p01a);
        p23a = pk_fma(splat2(qb.x), ve23[4 * cc + 0], p23a);
        p01b = pk_fma(splat2(qa.y), ve01[4 * cc + 1], p01b);
        p23b = pk_fma(splat2(qb.y), ve23[4 * cc + 1], p23b);
        p01a = pk_fma(splat2(qa.z), ve01[4 * cc + 2], p01a);
        p23a = pk_fma(splat2(qb.z), ve23[4 * cc + 2], p23a);
        p01b = pk_fma(splat2(qa.w), ve01[4 * cc + 3], p01b);
        p23b = pk_fma(splat2(qb.w), ve23[4 * cc + 3], p23b);
      }
      const f32x2 pre01 = p01a + p01b, pre23 = p23a + p23b;
      const CellFwd cell = cell_fwd(pre01.x, pre01.y, pre23.x, pre23.y, c[r]);
      c[r] = cell.c, h[r] = cell.h;
      st4(ot + ((size_t)r * NTS + tid) * 4, cell.gates);
      *reinterpret_cast<float2*>(ot + (size_t)R * NTS * 4 + ((size_t)r * NTS + tid) * 2) = make_float2(c[r], h[r]);
    }
  };
  // The headline's instantiation: whole periods of the ring first, t = 8 k .. 8 k + 7 with every slot and buffer a constant (every
  // LDS address of the step a loop-invariant per-thread base plus an immediate, no index arithmetic, no loop-carried register
  // copies), then the T mod 8 steps that remain; every other instantiation takes slot and buffer from t.
  // (Unrolled in the headline's instantiation alone - ranks up to 16, three waves: eight copies of the step in every XW
  //  instantiation would take the library past the size it is held to.)
  int t = 0;
  if constexpr (XW && KH == 16 && CNT == 3) {
    static_assert(FWD_XNB == 8, "the unrolled period below");
    for (; t + FWD_XNB <= T; t += FWD_XNB) {
      step(0, 0);
      step(1, 1);
      step(2, 0);
      step(3, 1);
      step(4, 0);
      step(5, 1);
      step(6, 0);
      step(7, 1);
    }
  }
  for (; t < T; ++t) step(XW ? (t & (FWD_XNB - 1)) : t % FWD_NB, t & 1);
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // barrier(T): last out-stage published

#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = blockIdx.x * R + r;
    if (valid && row < B) {
      if (a.hT != nullptr) a.hT[(size_t)row * H + n] = h[r];
      if (a.cT != nullptr) a.cT[(size_t)row * H + n] = c[r];
    }
  }
  if constexpr (R == 1) {
    {   // classifier on the final hidden state (one scalar load and out without one; a flag in FwdArgs instead cost the
        // recurrent loop 5 us: one more live scalar)
      typedef __attribute__((address_space(3))) float lds_f;
      const float* chp = outs + (size_t)((T - 1) & 1) * R * NTS * 8 + (size_t)R * NTS * 4;
      head_epilogue((const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr(), (const lds_f*)chp,
                    (int)blockIdx.x, wave, (lds_f*)part);   // (the partials' slots: nothing reads them after barrier(T))
      ce_epilogue((const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr(), (int)blockIdx.x, wave, (lds_f*)part);
    }
  }
}

template <int KH, int R, bool FLAT, int MAXT, int CNT>
static int fwd_launch_one(const VGeo& g, const FwdArgs& a, const XwArgs& xw, hipStream_t s) {
  if (a.xwave != 0) {
    if constexpr (R == 1 && MAXT == 256 && !FLAT) {
      // (ring and out-stage laid out for FWD_XNTS thread slots: the kernel's NB / NTS)
      const size_t ldsx = sizeof(float) * (fwd_part_floats<KH, R, FLAT, MAXT, CNT>(g.NW) + (size_t)FWD_XNB * FWD_XNTS * 4 + (size_t)2 * FWD_XNTS * 8 +
                                           256 + 4 + xwave_lds_floats() + ((a.xwave & 2) != 0 ? (size_t)(4 * g.I + 4) * g.NT : 0));
      auto kernx = rec_fwd_kernel<KH, R, FLAT, MAXT, CNT, true>;
      if (g.NT > FWD_XNTS) return -3;
      if (ldsx > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernx), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsx);
        if (e != hipSuccess) return (int)e;
      }
      hipLaunchKernelGGL(kernx, dim3(g.nwg), dim3(g.NT + 128), ldsx, s, g, a, xw);
      return (int)hipGetLastError();
    } else {
      return -3;
    }
  }
  const size_t lds = sizeof(float) * (fwd_part_floats<KH, R, FLAT, MAXT, CNT>(g.NW) + (size_t)FWD_NB * R * g.NT * 4 + (size_t)2 * R * g.NT * 8 + 256 + 4);
  auto kern = rec_fwd_kernel<KH, R, FLAT, MAXT, CNT>;
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kern, dim3(g.nwg), dim3(g.NT + 128), lds, s, g, a, xw);
  return (int)hipGetLastError();
}

// Instantiations: only the (slot tier, waves per consumer) pairs a layer can have.  One group: NT = 64 W (W = 1..4 | 5, 6 | 7, 8);
// two groups: NT = 128 W (W = 1, 2 | 3 | 4); the flat V4 layout exists with two groups only.  (Rounds 1-4 instantiated all
// fourteen pairs for both layouts: 256 kernels, half of them unreachable - 2.6 MB of the library.)
template <int KH, int MAXT, int CNT, bool ALSO_FLAT>
static int fwd_launch_mode(const VGeo& g, const FwdArgs& a, const XwArgs& xw, hipStream_t s) {
  if (g.R != 1) return -3;
  if (g.flat) {
    if constexpr (ALSO_FLAT) return g.G == 2 ? fwd_launch_one<KH, 1, true, MAXT, CNT>(g, a, xw, s) : -3;
    else return -3;
  }
  return fwd_launch_one<KH, 1, false, MAXT, CNT>(g, a, xw, s);
}

template <int KH>
static int fwd_launch_kh(const VGeo& g, const FwdArgs& a, const XwArgs& xw, hipStream_t s) {
  const int cnt = g.W;  // waves summed by a consumer
  if (g.NT <= 256) {
    switch (cnt) {
      case 1: return fwd_launch_mode<KH, 256, 1, true>(g, a, xw, s);
      case 2: return fwd_launch_mode<KH, 256, 2, true>(g, a, xw, s);
      case 3: return fwd_launch_mode<KH, 256, 3, false>(g, a, xw, s);
      case 4: return fwd_launch_mode<KH, 256, 4, false>(g, a, xw, s);
    }
  } else if (g.NT <= 384) {
    // 6 compute waves + 2 movers = 8 waves = two per SIMD: the 256-VGPR budget the wide ranks need (the 512-slot
    // tier below is compiled for 10 waves, 168 VGPRs, and spills at these ranks: 1.13 ms instead of 0.4 at H = 384);
    // for ranks <= 16 it is 2 % faster than the 512 tier (fewer mover slots per step)
    switch (cnt) {
      case 3: return fwd_launch_mode<KH, 384, 3, true>(g, a, xw, s);    // two groups of three waves
      case 5: return fwd_launch_mode<KH, 384, 5, false>(g, a, xw, s);
      case 6: return fwd_launch_mode<KH, 384, 6, false>(g, a, xw, s);
    }
  } else if (g.NT <= 512) {
    switch (cnt) {
      case 4: return fwd_launch_mode<KH, 512, 4, true>(g, a, xw, s);    // two groups of four waves
      case 7: return fwd_launch_mode<KH, 512, 7, false>(g, a, xw, s);
      case 8: return fwd_launch_mode<KH, 512, 8, false>(g, a, xw, s);
    }
  }
  return -3;
}
