// Persistent recurrent kernels, third form (gfx950): the one-group layers with a padded hidden rank of at most 16 and at most
// three waves of hidden units (BASELINE configs A, B, D; the reference's demo shapes) - vmlmf.py:300-314 + 78-125.
//
// What changed against rec_fwd_kernel / rec_bwd_kernel (vmlmf_rec_fwd.inc, vmlmf_rec_bwd.inc), and why - measured with
// tools/microbench/rec_probe.hip, xchg_probe.hip and issue_probe.hip (profiles/r03_*):
//  * A compute wave is bound by its own instruction issue (v_pk_fma_f32 4.4, v_fmac_f32_dpp 5.1, v_exp / v_rcp 8.3-9 ticks
//    each with one wave on a SIMD), and a mover wave that shares a SIMD with another wave gets the slots that one leaves.  In
//    the x-projection form of rec_fwd_kernel the x-projection wave (72 packed FMAs a step) and the storer wave were the last
//    at every barrier: the compute waves waited ~350 of ~1200 ticks a step for them (61 us with the pre-activations read from
//    memory, 71 us with the x-projection wave).
//    Here the compute waves form their own unit's x-side pre-activation of the NEXT step (2 I packed FMAs against the dense
//    x-side matrix in registers) in the shadow of the LDS round trip behind the barrier, the row's whole input sequence sits
//    in LDS from the start (T x I floats: no DMA ring, no counted waits), and the workgroup is NW compute waves + ONE storer
//    wave: one wave per SIMD.
//  * Partials of the rank-space reduce meet in LDS as [rank][wave]: one ds_read_b128 per lane and two plain adds give lane i
//    of every 16-lane row the total of rank i - no DPP butterfly over the waves (8 DPP adds with their wait states).
//  * Backward: the rank-space reduce of the four gate derivatives was 64 v_fmac_f32_dpp (5.1-6.4 ticks each); here a lane first
//    folds its four derivatives into 16 per-rank values with 32 packed FMAs against a rank-rotated image of V_h, and 15
//    v_add_f32_dpp row rotations sum them across the row (lane i keeps rank i); the expansion dh = dQ . U_h is the same
//    16-step rotation as the forward reduce (v_fmac_f32_dpp against a rotated image of the lane's own U_h row) instead of 16
//    v_readlane + 8 packed FMAs; the factors of the next step's gate derivatives are prepared in the shadow of the barrier.
#include "vmlmf_rec_fwd.inc"
#include "vmlmf_rec_bwd.inc"

constexpr int R3_MAXS = 3;   // waves of hidden units (thread slots / 64) these kernels cover


// sum of the (up to four) wave partials of this lane's rank, in wave order: three plain adds.  (The first sum is made opaque:
// left alone, the compiler packs the two inner sums into one v_pk_add_f32 and pays three v_mov_b32 to line the pairs up - five
// instructions on the dependent chain, right behind the partials' read, instead of three.)
__device__ __forceinline__ float r3_total(float4 p) {
  float lo = p.x + p.y;
  asm("" : "+v"(lo));
  return lo + (p.z + p.w);
}

// 16 rotations with four accumulators (two dependent chains of eight measured 6.4 ticks a step, independent ones 5.1)
__device__ __forceinline__ float fmac_ror_x16_4(float src, const float* w) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  asm("v_fmac_f32 %0, %4, %5\n\t" VG_DPP1(1, 4, 6, 1) VG_DPP1(2, 4, 7, 2) VG_DPP1(3, 4, 8, 3) VG_DPP1(0, 4, 9, 4) VG_DPP1(1, 4, 10, 5)
      VG_DPP1(2, 4, 11, 6) VG_DPP1(3, 4, 12, 7) VG_DPP1(0, 4, 13, 8) VG_DPP1(1, 4, 14, 9) VG_DPP1(2, 4, 15, 10) VG_DPP1(3, 4, 16, 11)
      VG_DPP1(0, 4, 17, 12) VG_DPP1(1, 4, 18, 13) VG_DPP1(2, 4, 19, 14) VG_DPP1(3, 4, 20, 15)
      : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3)
      : "v"(src), "v"(w[0]), "v"(w[1]), "v"(w[2]), "v"(w[3]), "v"(w[4]), "v"(w[5]), "v"(w[6]), "v"(w[7]), "v"(w[8]), "v"(w[9]),
        "v"(w[10]), "v"(w[11]), "v"(w[12]), "v"(w[13]), "v"(w[14]), "v"(w[15]));
  return (a0 + a1) + (a2 + a3);
}

__host__ __device__ inline size_t rec3_fwd_lds_floats(int NT, int T, int IM) { return 128 + (size_t)12 * NT + (size_t)(T + 32) * IM + 8; }

// KH: padded hidden rank (8 or 16); IM: input width rounded up to a multiple of four.
// (The x side on the matrix cores - v_mfma_f32_16x16x4_f32 by each compute wave or by the storer - measured no faster than the
//  packed FMAs in the barrier's shadow: tools/experiments/rec3_xm.patch, with the ablation switches.)
template <int KH, int IM>
__global__ void __launch_bounds__(256) rec3_fwd_kernel(VGeo g, FwdArgs a, XwArgs xwargs) {
  static_assert(KH == 8 || KH == 16, "one 16-rank pass");
  static_assert(IM % 4 == 0 && IM >= 4 && IM <= 16, "narrow inputs");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NT = g.NT, NW = g.NW, H = g.H, B = g.B, T = g.T, I = g.I;
  const bool train = a.gates != nullptr;
  const size_t sstride = (size_t)g.Bp * NT;   // slots per time slice of the slot-padded buffers
  const int row = blockIdx.x;                 // one batch row per workgroup (grid = B)

  extern __shared__ float4 smem4[];
  float* part = reinterpret_cast<float*>(smem4);   // [2][16 ranks][4 waves]; slots of waves that do not exist stay zero
  float* outs = part + 128;                        // [2][ NT x (i f o n) | NT x (c h) ]
  float* xs = outs + 12 * NT;                      // [T + 32][IM]: the row's inputs, zero-padded (slices >= T: zeros)
  if (tid < 128) part[tid] = 0.f;
  {
    const float* xr = xwargs.x + (size_t)row * g.sxB;
    const int n = (T + 32) * IM;
    for (int e = tid; e < n; e += (int)blockDim.x) {
      const int t = e / IM, m = e - t * IM;
      const bool ok = t < T && m < I;
      const float v = xr[(size_t)(ok ? t : 0) * g.sxT + (ok ? m : 0)];   // clamped: unconditional load
      xs[e] = ok ? v : 0.f;
    }
  }

  if (wave >= NW) {
    // ---------------------------------------------------------------------------------------------- storer wave
    // drains the out-stage of step t-1 to y / the tape and stores Q[t]; it never waits on vmcnt, so the write latency is on
    // nobody's critical path.  Alone on its SIMD.
    if (a.prog != nullptr && lane == 0) a.prog[(size_t)row * WR_PROG_STRIDE] = 0u;   // backward rows' progress words (WRide)
    bool sv[R3_MAXS];
    unsigned so_[R3_MAXS], yo_[R3_MAXS];
#pragma unroll
    for (int i = 0; i < R3_MAXS; ++i) {
      const int slot = lane + 64 * (i < NW ? i : 0);
      int n;
      const bool valid = vg_slot_unit(g, slot, n);
      sv[i] = i < NW && valid;
      so_[i] = (unsigned)(row * NT + slot) * 4u;          // bytes into a [Bp][NT] float slice
      yo_[i] = (unsigned)(row * g.syB + n) * 4u;          // bytes into y[t]
    }
    const bool qv = train && lane < KH;
    const unsigned qdst = (unsigned)(row * KH + (lane < KH ? lane : 0)) * 4u;
    const bool wide = (H & 3) == 0 && (g.syT & 3) == 0 && (g.syB & 3) == 0;
    auto segment = [&](int td, int tq) {   // every LDS read of the segment is issued before the first global store
      const int tdc = td < 0 ? 0 : td, tqc = tq < 0 ? 0 : tq;
      const float* src = outs + (size_t)(tdc & 1) * NT * 6;
      float4 g4[R3_MAXS];
      float2 ch[R3_MAXS];
#pragma unroll
      for (int i = 0; i < R3_MAXS; ++i) {
        const int slot = lane + 64 * (i < NW ? i : 0);
        g4[i] = ld4(src + (size_t)slot * 4);
        if (!wide) ch[i] = *reinterpret_cast<const float2*>(src + (size_t)NT * 4 + (size_t)slot * 2);
      }
      const float4 pq = ld4(part + (tqc & 1) * 64 + (lane & 15) * 4);
      // wide form (H a multiple of four): lane l takes the (c, h) pairs of the four slots 4 l .. 4 l + 3 and stores c and h
      // as one 16-byte store each - 2 store instructions a step instead of 2 NW (the bytes are the same; measured: see DESIGN)
      float4 w0 = make_float4(0.f, 0.f, 0.f, 0.f), w1 = w0;
      if (wide && lane < NT / 4) {
        w0 = ld4(src + (size_t)NT * 4 + (size_t)lane * 8);
        w1 = ld4(src + (size_t)NT * 4 + (size_t)lane * 8 + 4);
      }
      if (td >= 0) {
        char* gt = reinterpret_cast<char*>(a.gates + (size_t)td * sstride * 4);   // wave-uniform bases
        char* ct = reinterpret_cast<char*>(a.cs + (size_t)(td + 1) * sstride);
        char* yt = reinterpret_cast<char*>(a.y + (size_t)td * g.syT);
#pragma unroll
        for (int i = 0; i < R3_MAXS; ++i) {
          if (i < NW) {
            if (train) {
              st4_sv<false, true>(gt, 4u * so_[i], g4[i]);   // (tape: non-temporal, see st4_sv)
              if (!wide) st1_sv<false, true>(ct, so_[i], ch[i].x);
            }
            if (!wide && sv[i]) st1_sv<false, true>(yt, yo_[i], ch[i].y);
          }
        }
        if (wide && lane < NT / 4) {
          if (train) st4_sv<false, true>(ct, (unsigned)(row * NT + 4 * lane) * 4u, make_float4(w0.x, w0.z, w1.x, w1.z));
          if (4 * lane < H) st4_sv<false, true>(yt, (unsigned)(row * g.syB + 4 * lane) * 4u, make_float4(w0.y, w0.w, w1.y, w1.w));
        }
      }
      if (tq >= 0 && qv) st1_sv(a.Qs + (size_t)tq * B * KH, qdst, r3_total(pq));   // same order as the compute waves' sum
    };
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // x and the zeroed partials are published
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // barrier(0)
    for (int t = 0; t < T; ++t) {   // segment t
      segment(t - 1, t);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // barrier(t+1): LDS reads done, stores in flight
    }
    segment(T - 1, -1);
    return;
  }

  // ------------------------------------------------------------------------------------------------ compute waves
  const bool valid = tid < H;
  const int n = valid ? tid : 0;

  f32x2 ve01[KH], ve23[KH], eh01, eh23, wx01[IM], wx23[IM], b01, b23;
  float ur[16];
#pragma unroll
  for (int rr = 0; rr < KH; ++rr) {
    ve01[rr] = f32x2{a.VE[(size_t)(0 * KH + rr) * NT + tid], a.VE[(size_t)(1 * KH + rr) * NT + tid]};
    ve23[rr] = f32x2{a.VE[(size_t)(2 * KH + rr) * NT + tid], a.VE[(size_t)(3 * KH + rr) * NT + tid]};
  }
  eh01 = f32x2{a.EH[0 * NT + tid], a.EH[1 * NT + tid]};
  eh23 = f32x2{a.EH[2 * NT + tid], a.EH[3 * NT + tid]};
#pragma unroll
  for (int j = 0; j < 16; ++j) ur[j] = a.UR[(size_t)j * NT + tid];
#pragma unroll
  for (int m = 0; m < IM; ++m) {
    const bool mk = valid && m < I;
    const int mc = m < I ? m : 0;
    const float w0 = xwargs.WXD[(size_t)(mc * 4 + 0) * NT + tid], w1 = xwargs.WXD[(size_t)(mc * 4 + 1) * NT + tid];
    const float w2 = xwargs.WXD[(size_t)(mc * 4 + 2) * NT + tid], w3 = xwargs.WXD[(size_t)(mc * 4 + 3) * NT + tid];
    wx01[m] = mk ? f32x2{w0, w1} : f32x2{0.f, 0.f};
    wx23[m] = mk ? f32x2{w2, w3} : f32x2{0.f, 0.f};
  }
  {
    const float q0 = xwargs.BBT[0 * H + n], q1 = xwargs.BBT[1 * H + n], q2 = xwargs.BBT[2 * H + n], q3 = xwargs.BBT[3 * H + n];
    b01 = valid ? f32x2{q0, q1} : f32x2{0.f, 0.f};
    b23 = valid ? f32x2{q2, q3} : f32x2{0.f, 0.f};
  }

  float h = (valid && a.h0 != nullptr) ? a.h0[(size_t)row * H + n] : 0.f;
  float c = (valid && a.c0 != nullptr) ? a.c0[(size_t)row * H + n] : 0.f;
  if (train) a.cs[(size_t)row * NT + tid] = c;   // tape slice 0 = c_{-1}

  // x-side pre-activation of one step from the inputs in LDS (broadcast reads: every lane the same address)
  f32x2 gx01 = b01, gx23 = b23;
  auto xload = [&](int t, float4 (&xv)[IM / 4]) {
    const float4* xp = reinterpret_cast<const float4*>(xs + (size_t)t * IM);
#pragma unroll
    for (int m4 = 0; m4 < IM / 4; ++m4) xv[m4] = xp[m4];
  };
  auto xproj = [&](const float4 (&xv)[IM / 4], f32x2& o01, f32x2& o23) {
    f32x2 p01a = b01, p01b = f32x2{0.f, 0.f}, p23a = b23, p23b = f32x2{0.f, 0.f};
#pragma unroll
    for (int m4 = 0; m4 < IM / 4; ++m4) {
      p01a = pk_fma(splat2(xv[m4].x), wx01[4 * m4 + 0], p01a);
      p23a = pk_fma(splat2(xv[m4].x), wx23[4 * m4 + 0], p23a);
      p01b = pk_fma(splat2(xv[m4].y), wx01[4 * m4 + 1], p01b);
      p23b = pk_fma(splat2(xv[m4].y), wx23[4 * m4 + 1], p23b);
      p01a = pk_fma(splat2(xv[m4].z), wx01[4 * m4 + 2], p01a);
      p23a = pk_fma(splat2(xv[m4].z), wx23[4 * m4 + 2], p23a);
      p01b = pk_fma(splat2(xv[m4].w), wx01[4 * m4 + 3], p01b);
      p23b = pk_fma(splat2(xv[m4].w), wx23[4 * m4 + 3], p23b);
    }
    o01 = p01a + p01b, o23 = p23a + p23b;
  };
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");   // x and the zeroed partials are published
  {
    float4 xv[IM / 4];
    xload(0, xv);
    xproj(xv, gx01, gx23);
  }

  // The step is written as phases with scheduling fences between them, so that everything that is NOT on the dependent chain
  // (h -> reduce -> LDS -> barrier -> LDS -> expansion -> gates -> h) lands where the chain waits anyway: phase B (behind the
  // partial's ds_write, in front of the barrier) and phase D (behind the barrier, while the partials' read is in flight).
  // Left to the compiler, the x-side arithmetic ended up interleaved with the gates (7 - 11 us a launch).
  float4 og4 = make_float4(0.f, 0.f, 0.f, 0.f);   // gates, c, h of the previous step: their out-stage writes are deferred to phase B
  float2 och = make_float2(0.f, 0.f);
  for (int t = 0; t < T; ++t) {
    const int buf = t & 1;
    // ---- A. rank-space reduce of h_{t-1}: lane i of a row ends with rank i summed over the wave's 64 units
    float hv = h;
    dpp_fence(hv);
    const float s = rowsum4(fmac_ror_x16_4(hv, ur));
    if (lane < 16) part[buf * 64 + lane * 4 + wave] = s;
    __builtin_amdgcn_sched_barrier(0);
    // ---- B. shadow of that write: out-stage of step t-1, half of the x side
    if (t > 0) {
      float* ot = outs + (size_t)((t - 1) & 1) * NT * 6;
      st4(ot + (size_t)tid * 4, og4);
      *reinterpret_cast<float2*>(ot + (size_t)NT * 4 + (size_t)tid * 2) = och;
    }
    float4 xv[IM / 4];
    f32x2 gn01 = b01, gn23 = b23;
    xload(t + 1, xv);   // inputs of the next step (slices >= T: zeros)
    // ---- barrier(t): partials of step t and the out-stage of step t-1 are published
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    const float4 p = ld4(part + buf * 64 + (lane & 15) * 4);
    __builtin_amdgcn_sched_barrier(0);
    // ---- D. shadow of that read: the rest of the x side, h . eh
    xproj(xv, gn01, gn23);
    const f32x2 hh = splat2(h);
    f32x2 p01a = pk_fma(hh, eh01, gx01), p01b = f32x2{0.f, 0.f};
    f32x2 p23a = pk_fma(hh, eh23, gx23), p23b = f32x2{0.f, 0.f};
    __builtin_amdgcn_sched_barrier(0);
    // ---- E. expand + gates
    const float tot = r3_total(p);
#pragma unroll
    for (int r = 0; r < KH; r += 4) {
      const float q0 = bcast_lane(tot, r), q1 = bcast_lane(tot, r + 1), q2 = bcast_lane(tot, r + 2), q3 = bcast_lane(tot, r + 3);
      p01a = pk_fma(splat2(q0), ve01[r + 0], p01a);
      p23a = pk_fma(splat2(q0), ve23[r + 0], p23a);
      p01b = pk_fma(splat2(q1), ve01[r + 1], p01b);
      p23b = pk_fma(splat2(q1), ve23[r + 1], p23b);
      p01a = pk_fma(splat2(q2), ve01[r + 2], p01a);
      p23a = pk_fma(splat2(q2), ve23[r + 2], p23a);
      p01b = pk_fma(splat2(q3), ve01[r + 3], p01b);
      p23b = pk_fma(splat2(q3), ve23[r + 3], p23b);
    }
    const f32x2 pre01 = p01a + p01b, pre23 = p23a + p23b;
    const CellFwd cell = cell_fwd(pre01.x, pre01.y, pre23.x, pre23.y, c);
    c = cell.c, h = cell.h;
    og4 = cell.gates, och = make_float2(c, h);
    gx01 = gn01, gx23 = gn23;
    __builtin_amdgcn_sched_barrier(0);
  }
  {   // out-stage of the last step
    float* ot = outs + (size_t)((T - 1) & 1) * NT * 6;
    st4(ot + (size_t)tid * 4, og4);
    *reinterpret_cast<float2*>(ot + (size_t)NT * 4 + (size_t)tid * 2) = och;
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // barrier(T): last out-stage published

  if (valid) {
    if (a.hT != nullptr) a.hT[(size_t)row * H + n] = h;
    if (a.cT != nullptr) a.cT[(size_t)row * H + n] = c;
  }
  {
    typedef __attribute__((address_space(3))) float lds_f;
    const float* chp = outs + (size_t)((T - 1) & 1) * NT * 6 + (size_t)NT * 4;
    head_epilogue((const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr(), (const lds_f*)chp, row, wave,
                  (lds_f*)part);   // (the partials' slots: nothing reads them after barrier(T))
    ce_epilogue((const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr(), row, wave, (lds_f*)part);
  }
}

// which layers: one group, not the flat layout, one 16-rank pass, the x-projection wave's envelope (dense x-side image in
// PACK), the x-fold (no qx tape is written), the whole input row in LDS
__host__ inline bool rec3_fwd_ok(const VGeo& g) {
  if (!vg_xwave_ok(g) || g.G != 1 || g.flat || g.KH > 16 || !g.foldx || g.R != 1 || g.NW > R3_MAXS) return false;
  const int IM = (g.I + 3) / 4 * 4;
  return sizeof(float) * rec3_fwd_lds_floats(g.NT, g.T, IM) <= 150 * 1024;
}

template <int KH, int IM>
static int rec3_fwd_launch_one(const VGeo& g, const FwdArgs& a, const XwArgs& xw, hipStream_t s) {
  const size_t lds = sizeof(float) * rec3_fwd_lds_floats(g.NT, g.T, IM);
  auto kern = rec3_fwd_kernel<KH, IM>;
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kern, dim3(g.nwg), dim3(g.NT + 64), lds, s, g, a, xw);
  return (int)hipGetLastError();
}
template <int KH>
static int rec3_fwd_launch_kh(const VGeo& g, const FwdArgs& a, const XwArgs& xw, hipStream_t s) {
  switch ((g.I + 3) / 4) {
    case 1: return rec3_fwd_launch_one<KH, 4>(g, a, xw, s);
    case 2: return rec3_fwd_launch_one<KH, 8>(g, a, xw, s);
    case 3: return rec3_fwd_launch_one<KH, 12>(g, a, xw, s);
    case 4: return rec3_fwd_launch_one<KH, 16>(g, a, xw, s);
  }
  return -3;
}

// ====================================================================================================================
// backward
// ====================================================================================================================
// The tape ring of rec3_bwd_kernel is R3_NB = 8 slots deep: a power of two, so that the slot of step t is t & 7 (two's complement:
// also for the steps below zero the loader and the last fetch name) and the compute waves' step loop, unrolled over the ring's
// period, names every slot and both out-stage buffers by a constant.  (BWD_NB = 6 cost every wave a division by six per step.)
// fixed: the riding launches, which own their CU (84 KB asked for), lay the ring and the out-stage out for R3_NTS = 192 thread
// slots whatever NT is - every LDS address of the step loop is then a per-thread base plus an immediate offset.
constexpr int R3_NB = 8;
constexpr int R3_NTS = 64 * R3_MAXS;
// (+ DR_SCR_FLOATS per thread slot: the compute waves' slots for the direct mode's per-lane rotations, vmlmf_direct.inc)
__host__ __device__ inline size_t rec3_bwd_lds_floats(int NT, bool fixed = false) {
  const size_t nts = fixed ? R3_NTS : NT;
  return 128 + (size_t)R3_NB * nts * 6 + (size_t)2 * nts * 4 + 256 + 4 + (size_t)DR_SCR_FLOATS * NT;
}

// z[0] + sum_k (z[k] received through row_ror:k), 15 v_add_f32_dpp on three accumulators.  With register k of lane l holding
// the lane's contribution to the rank k rotation steps away, lane i of every 16-lane row ends with rank i summed over the row.
// (s_nop 1: the registers were written by VALU instructions right in front - two wait states before a DPP read.)
#define VG_ADD1(acc, src, k) "v_add_f32_dpp %" #acc ", %" #src ", %" #acc " row_ror:" #k " row_mask:0xf bank_mask:0xf\n\t"
// (The second and third accumulator start as 0 + their first term, the zero read from a register of its own: the same sums as
//  into zeroed accumulators, without a v_mov_b32 per accumulator and step.)
#define VG_ADD0(acc, src, k) "v_add_f32_dpp %" #acc ", %" #src ", %18 row_ror:" #k " row_mask:0xf bank_mask:0xf\n\t"
__device__ __forceinline__ float add_ror_x16(const float (&z)[16]) {
  float a0 = z[0], a1, a2;
  const float zero = 0.f;
  asm("s_nop 1\n\t" VG_ADD0(1, 3, 1) VG_ADD0(2, 4, 2) VG_ADD1(0, 5, 3) VG_ADD1(1, 6, 4) VG_ADD1(2, 7, 5) VG_ADD1(0, 8, 6) VG_ADD1(1, 9, 7)
      VG_ADD1(2, 10, 8) VG_ADD1(0, 11, 9) VG_ADD1(1, 12, 10) VG_ADD1(2, 13, 11) VG_ADD1(0, 14, 12) VG_ADD1(1, 15, 13) VG_ADD1(2, 16, 14)
      VG_ADD1(0, 17, 15)
      : "+v"(a0), "=&v"(a1), "=&v"(a2)
      : "v"(z[1]), "v"(z[2]), "v"(z[3]), "v"(z[4]), "v"(z[5]), "v"(z[6]), "v"(z[7]), "v"(z[8]), "v"(z[9]), "v"(z[10]), "v"(z[11]),
        "v"(z[12]), "v"(z[13]), "v"(z[14]), "v"(z[15]), "v"(zero));
  return (a0 + a1) + a2;
}

// RIDE: as rec_bwd_kernel (the weight-gradient workers behind the rows' workgroups; B-column tiles of the products)
template <int KH, int RIDE = 0>
__global__ void __launch_bounds__(320) rec3_bwd_kernel(VGeo g, BwdArgs a) {
  static_assert(KH == 8 || KH == 16, "one 16-rank pass");
  if constexpr (RIDE > 0) {
    if ((int)blockIdx.x >= g.nwg) {
      wride_worker<RIDE>(g, a.wr);
      return;
    }
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NT = g.NT, NW = g.NW, H = g.H, B = g.B, T = g.T;
  const bool has_dy = a.dy != nullptr;
  const size_t sstride = (size_t)g.Bp * NT;
  const int row = blockIdx.x;

  const int NTS = RIDE > 0 ? R3_NTS : NT;          // thread slots a ring slot / an out-stage buffer is laid out for (rec3_bwd_lds_floats)
  extern __shared__ float4 smem4[];
  float* part = reinterpret_cast<float*>(smem4);   // [2][16 ranks][4 waves]
  float* tg = part + 128;                          // [R3_NB][NTS][4]  gates of the step
  float* tcp = tg + R3_NB * NTS * 4;               // [R3_NB][NTS]     c_{t-1}
  float* tdy = tcp + R3_NB * NTS;                  // [R3_NB][NTS]     dy_t
  float* outs = tdy + R3_NB * NTS;                 // [2][NTS][4]      dpre
  float* spare = outs + 2 * NTS * 4;               // 256 floats: target of the dummy DMAs
  float* drscr = spare + 256 + 4;                  // [NT][DR_SCR_FLOATS]: direct mode, compute waves' prologue only
  if (tid < 128) part[tid] = 0.f;

  if (tid >= NT) {
    // ------------------------------------------------------------------ loader + storer waves (as rec_bwd_kernel's)
    constexpr int MAXS = R3_MAXS;
    constexpr int NDMA = 3 * MAXS;
    constexpr int DEPTH = 2;
    constexpr int DIST = DEPTH + 2;
    static_assert(DIST < R3_NB && (R3_NB & (R3_NB - 1)) == 0 && 2 * NDMA <= 63, "tape ring");
    if (wave == NW) {
      auto issue = [&](int ttarget) {   // tape of step ttarget (clamped at 0) -> ring slot
        const int tc = ttarget > 0 ? ttarget : 0;
        const int ring = ttarget & (R3_NB - 1);
#pragma unroll
        for (int i = 0; i < MAXS; ++i) {
          const bool real = i < NW;
          const int slot = lane + 64 * (real ? i : 0);
          const size_t e = (size_t)tc * sstride + (size_t)row * NT + slot;
          int n;
          if (!vg_slot_unit(g, slot, n)) n = 0;   // pad slots must not index past the row
          const size_t lo = (size_t)ring * NTS + 64 * (real ? i : 0);
          dma16(a.gates + e * 4, real ? tg + lo * 4 : spare);
          dma4(a.cs + e, real ? tcp + lo : spare);                      // slice tc = c_{tc-1}
          dma4(has_dy ? a.dy + ((size_t)tc * g.syT + (size_t)row * g.syB + n) : a.cs + e, real ? tdy + lo : spare);
        }
      };
      for (int s0 = 0; s0 < DIST; ++s0) issue(T - 1 - s0);    // tapes T-1 .. T-DIST
      wait_vm_barrier<(DIST - 2) * NDMA>();                   // opening barrier: tapes T-1 and T-2 have landed
      for (int t = T - 1; t >= 0; --t) {
        issue(t - DIST);
        wait_vm_barrier<DEPTH * NDMA>();                      // barrier(t): tape t-2 has landed
      }
      return;
    }
    const bool qv = lane < KH;
    const unsigned qdst = (unsigned)(row * KH + (lane < KH ? lane : 0)) * 4u;
    constexpr bool SAFE_ST = false;   // (vmlmf_device.h, hazard 2: set for the instantiations tools/check_asm_hazards.py flags)
    auto drain = [&](int ts) {   // dpre of step ts -> HBM (every slot is written), dQ[ts]
      const float* src = outs + (size_t)(ts & 1) * NTS * 4;
      float* dt = a.dpre + (size_t)ts * sstride * 4;
      float4 d4[MAXS];
#pragma unroll
      for (int i = 0; i < MAXS; ++i) d4[i] = ld4(src + ((size_t)lane + 64 * (i < NW ? i : 0)) * 4);
      const float4 pq = ld4(part + (ts & 1) * 64 + (lane & 15) * 4);
#pragma unroll
      for (int i = 0; i < MAXS; ++i)
        if (i < NW) {
          if constexpr (RIDE > 0) st4_sv_sys<SAFE_ST>(dt, 16u * (unsigned)(row * NT + lane + 64 * i), d4[i]);
          else st4_sv(dt, 16u * (unsigned)(row * NT + lane + 64 * i), d4[i]);
        }
      float* qt = a.dQs + (size_t)ts * B * KH;
      if (qv) {
        if constexpr (RIDE > 0) st1_sv_sys<SAFE_ST>(qt, qdst, r3_total(pq));
        else st1_sv(qt, qdst, r3_total(pq));
      }
    };
    // RIDE: stores per segment = NW row slices of dpre + the dQ store (lane 0 is live in each) + the progress word
    const int nd = NW + 1;
    const int lag = a.wr.lag;
    const int nwait = nd * lag;
    // The counted wait of a segment takes its count as an immediate, and the count is fixed for the launch: the loop exists once
    // with the count of the default lag at three waves of units (WR_LAG_DEFAULT segments of nd = 4 stores; NWAIT >= 0) and once
    // with the run-time count behind wait_vm_dyn's branch tree, which every other launch takes (NWAIT < 0).
    auto segments = [&](auto nwait_c) {
      constexpr int NWAIT = decltype(nwait_c)::value;
      for (int t = T - 1; t >= 0; --t) {   // segment t: step t+1 is complete
        if (t + 1 < T) {
          drain(t + 1);
          if constexpr (RIDE > 0) {
            if constexpr (NWAIT >= 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NWAIT) : "memory");
            else wait_vm_dyn(nwait);
            const int done = T - (t + 1 + lag);   // steps T-1 .. t+1+lag are in memory
            if (lane == 0 && (t & 1) == 0)
              st1_sv_sys<SAFE_ST>(a.wr.prog, 4u * (unsigned)(row * WR_PROG_STRIDE), (unsigned)(done > 0 ? done : 0));
          }
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // barrier(t)
      }
    };
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // opening barrier
    if constexpr (RIDE == 1 && KH == 16) {   // (the headline instantiation: the library's size)
      switch (nwait) {
        case 4 * WR_LAG_DEFAULT: segments(std::integral_constant<int, 4 * WR_LAG_DEFAULT>{}); break;   // three waves of units
        default: segments(std::integral_constant<int, -1>{}); break;
      }
    } else {
      segments(std::integral_constant<int, -1>{});
    }
    drain(0);
    if constexpr (RIDE > 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) st1_sv_sys<SAFE_ST>(a.wr.prog, 4u * (unsigned)(row * WR_PROG_STRIDE), (unsigned)T);
    }
    return;
  }

  // -------------------------------------------------------------------- compute waves
  const bool valid = tid < H;
  const int n = valid ? tid : 0;

  // classifier prologue first, while nothing else is live (see rec_bwd_kernel)
  float dh_head;
  if constexpr (RIDE > 0)
    dh_head = a.hd.C > 0 ? head_dh_body((const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr(), row, n, valid) : 0.f;
  else
    dh_head = a.hd.C > 0 ? head_dh((const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr(), row, n, valid) : 0.f;

  // Which lane does row_ror:1 deliver from?  (direction of the rotation, found by rotating the lane ids.)  d = +1 or -1 mod 16.
  const int li = lane & 15;
  const int d = (__float_as_int(ror16<1>(__int_as_float(li))) - li) & 15;
  // reduce image: register k holds V_h[gate][this unit][rank (li - d k) mod 16] - rotated k steps it arrives at the lane of that
  // rank; expansion image: register k holds U_h[this unit][rank (li + d k) mod 16] - the rank whose total arrives with rotation k
  f32x2 vz[4][8];
  float ue[16], eh[4];
  bool direct = false;
  if constexpr (RIDE > 0) direct = a.wr.direct != 0;   // (the riding forms: one workgroup per CU whatever the register count)
  if (direct) {
    // direct mode (vmlmf_direct.inc): this unit's own rows of v_h / u_h, rotated by the lane's place in its DPP row in registers
   if constexpr (RIDE > 0) {
    float vr[4][16], ur0[16];
#pragma unroll
    for (int gk = 0; gk < 4; ++gk) dr_load_row<KH>(a.VE, (size_t)gk * H + n, valid, vr[gk]);
    dr_load_row<KH>(a.UE, (size_t)n, valid, ur0);
    const float dh = a.EH[n], vf = valid ? 1.f : 0.f;
    float* scr = drscr + (size_t)tid * DR_SCR_FLOATS;   // this lane's LDS slot (dr_put / dr_at: a register array indexed per lane)
    const int dn = 16 - d;                                // (- d mod 16)
#pragma unroll
    for (int gk = 0; gk < 4; ++gk) {
      eh[gk] = (dh - dr_chain<KH>(ur0, vr[gk])) * vf;
      dr_put(scr, vr[gk]);
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const float vv = dr_at(scr, li + dn * k);         // rank (li - d k) & 15
        if (k & 1) vz[gk][k >> 1].y = vv;
        else vz[gk][k >> 1].x = vv;
      }
    }
    dr_put(scr, ur0);
#pragma unroll
    for (int k = 0; k < 16; ++k) ue[k] = dr_at(scr, li + d * k);   // rank (li + d k) & 15
   }
  } else {
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int rr = (li - d * k) & 15, re = (li + d * k) & 15;
    const bool inr = rr < KH, ine = re < KH;
#pragma unroll
    for (int gk = 0; gk < 4; ++gk) {
      const float v = a.VE[(size_t)(gk * KH + (inr ? rr : 0)) * NT + tid];
      const float vv = inr ? v : 0.f;
      if (k & 1) vz[gk][k >> 1].y = vv;
      else vz[gk][k >> 1].x = vv;
    }
    const float u = a.UE[(size_t)(ine ? re : 0) * NT + tid];
    ue[k] = ine ? u : 0.f;
  }
#pragma unroll
  for (int gk = 0; gk < 4; ++gk) eh[gk] = a.EH[gk * NT + tid];
  }

  float dhrec, dcs, ccur;
  {
    const size_t bh = (size_t)row * H + n;
    dhrec = (valid && a.dhT != nullptr) ? a.dhT[bh] : 0.f;
    dhrec += dh_head;
    dcs = (valid && a.dcT != nullptr) ? a.dcT[bh] : 0.f;
    ccur = a.cs[(size_t)T * sstride + (size_t)row * NT + tid];
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");   // opening barrier: tapes T-1 and T-2 have landed

  float4 g4n;
  float cprvn, dyvn;
  auto fetch_tape = [&](const int ringn) __attribute__((always_inline)) {   // ringn: the ring slot, step & (R3_NB - 1)
    const size_t lo = (size_t)ringn * NTS + tid;
    g4n = ld4(tg + lo * 4);
    cprvn = tcp[lo];
    dyvn = tdy[lo];
  };
  CellBwdFactors fac;
  float fdy;
  auto prepare = [&]() {   // the factors of a step's gate derivatives that do not depend on dh
    fac = cell_bwd_factors(g4n, ccur, cprvn);
    fdy = (valid && has_dy) ? dyvn : 0.f;
    ccur = cprvn;   // c of the step before
  };
  fetch_tape((T - 1) & (R3_NB - 1));
  prepare();
  // One time step t.  It names the step by what it addresses: ringp = ring slot of step t-1's tape, buf = t & 1.  Called with
  // constants (the unrolled loop below), every LDS access of the step is a loop-invariant per-thread base plus an immediate offset
  // and nothing of the step is index arithmetic.
  auto step = [&](const int ringp, const int buf) __attribute__((always_inline)) {
    // tape of step t-1: landed at the barrier before this segment (the loader's counted wait); consumed by prepare() below
    fetch_tape(ringp);   // (t = 0: a valid, unused ring slot)
    const float4 dp = cell_bwd_step(fac, fdy + dhrec, dcs);
    st4(outs + (size_t)buf * NTS * 4 + (size_t)tid * 4, dp);
    const float ehterm = cell_ehterm_fma(dp, eh[0], eh[1], eh[2], eh[3]);   // (explicit fused multiply-adds: see there)
    // ---- rank-space reduce of dpre: fold the four gates per lane, then rotate-and-add across the row
    f32x2 z2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) z2[j] = splat2(dp.x) * vz[0][j];
#pragma unroll
    for (int j = 0; j < 8; ++j) z2[j] = pk_fma(splat2(dp.y), vz[1][j], z2[j]);
#pragma unroll
    for (int j = 0; j < 8; ++j) z2[j] = pk_fma(splat2(dp.z), vz[2][j], z2[j]);
#pragma unroll
    for (int j = 0; j < 8; ++j) z2[j] = pk_fma(splat2(dp.w), vz[3][j], z2[j]);
    float z[16];
#pragma unroll
    for (int j = 0; j < 8; ++j) z[2 * j] = z2[j].x, z[2 * j + 1] = z2[j].y;
    const float s = rowsum4(add_ror_x16(z));
    if (lane < 16) part[buf * 64 + lane * 4 + wave] = s;
    // ---- in the shadow of that write and of the barrier: the dh-independent factors of step t-1
    // (behind the barrier instead, in the shadow of the partials' read: no faster - tools/experiments/step_loops_prepare_behind_barrier.patch)
    prepare();
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // barrier(t)
    const float4 p = ld4(part + buf * 64 + (lane & 15) * 4);
    float tot = r3_total(p);
    dpp_fence(tot);
    dhrec = ehterm + fmac_ror_x16_4(tot, ue);
  };
  // Steps T-1 .. 0: first the (T mod 8) steps down to a ring boundary, slot and buffer taken from t; then whole periods of the
  // ring, t = 8 k + 7 .. 8 k, every slot and buffer a constant.  (No loop-carried register copies at a period's end either.)
  // RIDE == 0 shares its CU with other rows' workgroups and keeps every step in the first loop: eight slots' worth of hoisted
  // addresses took it from 132 to 148 VGPRs, past the 136 its occupancy rests on (tools/kernel_budget.py).
  // (Nor the other riding instantiations: eight copies of the step in each would take the library past the size it is held to.)
  constexpr bool PERIODS = RIDE == 1 && KH == 16;
  int t = T - 1;
  for (; PERIODS ? (t & (R3_NB - 1)) != R3_NB - 1 : t >= 0; --t) step((t - 1) & (R3_NB - 1), t & 1);
  if constexpr (PERIODS) {
    for (; t >= 0; t -= R3_NB) {
      step(6, 1);
      step(5, 0);
      step(4, 1);
      step(3, 0);
      step(2, 1);
      step(1, 0);
      step(0, 1);
      step(7, 0);
    }
    static_assert(R3_NB == 8, "the unrolled period above");
  }

  if (valid) {
    if (a.dh0 != nullptr) a.dh0[(size_t)row * H + n] = dhrec;
    if (a.dc0 != nullptr) a.dc0[(size_t)row * H + n] = dcs;
  }
}

__host__ inline bool rec3_bwd_ok(const VGeo& g) {
  return !g.generic && !g.rb && !g.bf && g.G == 1 && !g.flat && g.KH <= 16 && g.R == 1 && g.NW <= R3_MAXS;
}

template <int KH>
static int rec3_bwd_launch_kh(const VGeo& g, const BwdArgs& a, hipStream_t s) {
  const size_t lds = sizeof(float) * rec3_bwd_lds_floats(g.NT, a.wr.K > 0);
  if (a.wr.K > 0) {
    const int n1 = (vg_nb1(g) + 31) / 32, n2 = (g.G * g.KH + 31) / 32;
    if (n1 > 2 || n2 > 2) return -3;
    // more than half a CU's LDS per workgroup: ONE workgroup per CU, so that a worker never shares a CU with a row's recurrence
    const size_t lds1 = lds > 84 * 1024 ? lds : (size_t)84 * 1024;
    const dim3 grid(g.nwg + a.wr.K * a.wr.ntg), block(g.NT + 128);
    auto k1 = rec3_bwd_kernel<KH, 1>;
    auto k2 = rec3_bwd_kernel<KH, 2>;
    auto kern = (n1 == 1 && n2 == 1) ? k1 : k2;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kern, grid, block, lds1, s, g, a);
    return (int)hipGetLastError();
  }
  hipLaunchKernelGGL((rec3_bwd_kernel<KH>), dim3(g.nwg), dim3(g.NT + 128), lds, s, g, a);
  return (int)hipGetLastError();
}
