// Persistent recurrent backward kernel, fourth form (gfx950): rec3_bwd_kernel's recurrence with the WEIGHT GRADIENTS FORMED IN
// THE ROW'S OWN WORKGROUP - autograd's replay of vmlmf.py:300-314 + 78-125 for the one-group, x-fold layers (BASELINE configs
// A, B, D).
//
// Why (verdict r3, weak 2 + 4; profiles/r03_bench_strong_1gpu.jsonl): the batched weight-gradient kernel behind the recurrence
// re-reads what the recurrence has just written - dpre, 16 B per unit and step written + read again, beside the 24 B tape it
// already reads.  At 128 / 256 / 512 rows per GPU wgrad_mfma_kernel was 22 / 31 / 36 % of the step and rec_bwd ran at the HBM
// roof (503 MB in 92 us at B = 512); the riding workers (<= 64 rows) re-read the same bytes from idle CUs.  But every operand
// of the products is in this workgroup's LDS at the moment the step is computed:
//      G  += dpre_t^T [x_t | Q_t]      (dV_x / dU_x through the x-fold, dV_h)       dpre_t: out-stage of the compute waves
//      GU += h_{t-1}^T dQ_t            (dU_h)                                        dQ_t:   the rank-space partials
//      e  += dpre_t . {h_{t-1}, x_t, 1}   (d(eh), d(ex), db)
// and a compute wave uses one VALU issue slot in four or five and no matrix pipe at all.  So the workgroup gets NW + 1 more
// waves - "accumulator waves", one beside each compute wave and one beside the loader - that contract two time steps per
// v_mfma_f32_32x32x2_f32 (K = 2: steps t, t-1 of this row; exact fp32 FMA chain) straight from LDS: per pair of steps a wave
// issues 8 MFMAs (512 cycles of its SIMD's otherwise idle matrix pipe out of ~2500) and ~40 LDS / VALU instructions.  Nothing
// of dpre or dQ goes to memory, there is no storer wave, no weight-gradient launch and no re-read: the backward launch reads the
// tape (24 B + h: 28 B per unit and step) and writes ONE partial block per workgroup at its end, which reduce_cg_kernel sums
// in fixed order (deterministic; same block layout as the stand-alone kernel's chunks: vmlmf_atb.inc).
//
// Rings in LDS: dpre out-stage and rank-space partials 4 deep (a pair is consumed up to three steps after it was produced),
// h_{t-1} 8 deep (the loader runs four steps ahead), tape as rec3_bwd_kernel (BWD_NB).  [x | Q] of the whole row sits in LDS
// from the start (T x 32 floats).
#include "vmlmf_rec3.inc"

constexpr int R4_NO = 4;   // dpre / partial ring depth
constexpr int R4_NH = 8;   // h ring depth

// floats of the row's rings, and 256 + 4 floats of spare
__host__ __device__ inline size_t rec4_row_floats(int NT, int T) {
  return (size_t)R4_NO * 64 + (size_t)BWD_NB * NT * 6 + (size_t)R4_NH * NT + (size_t)R4_NO * NT * 4 + (size_t)T * 32;
}
__host__ __device__ inline size_t rec4_bwd_lds_floats(int NT, int T) { return rec4_row_floats(NT, T) + 256 + 4; }

// KH: padded hidden rank (8 or 16).  Block = NW compute waves | the loader | NW dpre-accumulator waves | one h-accumulator wave.
// (A form with TWO rows per workgroup - one set of accumulators, an MFMA contracting the two rows of a step - and the ablation
//  builds behind the numbers in docs/design/in_row_weight_gradients.md: tools/experiments/rec4_two_rows_and_ablations.patch.)
template <int KH>
__global__ void __launch_bounds__(512) rec4_bwd_kernel(VGeo g, BwdArgs a) {
  static_assert(KH == 8 || KH == 16, "one 16-rank pass");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NT = g.NT, NW = g.NW, H = g.H, B = g.B, T = g.T, KX = g.KX;
  const bool has_dy = a.dy != nullptr;
  const size_t sstride = (size_t)g.Bp * NT;
  const AtbArgs& w = a.wr.a;      // operands of the products: x, y, h0, Qs; P = this launch's partial blocks
  const int NC = NW;              // compute waves; then the loader; then NW + 1 accumulator waves
  const int row = (int)blockIdx.x;   // one batch row per workgroup (grid = B)

  extern __shared__ float4 smem4[];
  const size_t ROWF = rec4_row_floats(NT, T);
  float* lds0 = reinterpret_cast<float*>(smem4);
  float* part = lds0;                              // [R4_NO][16 ranks][4 waves]
  float* tg = part + R4_NO * 64;                   // [BWD_NB][NT][4]  gates of the step
  float* tcp = tg + BWD_NB * NT * 4;               // [BWD_NB][NT]     c_{t-1}
  float* tdy = tcp + BWD_NB * NT;                  // [BWD_NB][NT]     dy_t
  float* th = tdy + BWD_NB * NT;                   // [R4_NH][NT]      h_{t-1}
  float* outs = th + R4_NH * NT;                   // [R4_NO][NT][4]   dpre
  float* bq = outs + R4_NO * NT * 4;               // [T][32]          B operand rows: x_t (KX columns, zero beyond I) | Q_t (KH) | 0
  float* spare = lds0 + ROWF;                      // 256 floats: target of the dummy DMAs
  const size_t o_th = (size_t)(th - part), o_outs = (size_t)(outs - part), o_bq = (size_t)(bq - part);   // offsets inside a row's block
  for (int e = tid; e < R4_NO * 64; e += (int)blockDim.x) lds0[e] = 0.f;
  {
    const int rr = row;
    float* bqr = lds0 + o_bq;
    // [x | Q] rows of the whole sequence: batches of eight elements per thread, every load of a batch issued (clamped addresses,
    // masked values) before the first LDS write - as a plain loop this prologue was a chain of T / 16 memory latencies
    const float* xr = w.x + (size_t)rr * g.sxB;
    const int n = T * 32, nth = (int)blockDim.x;
    for (int e0 = tid; e0 < n; e0 += 8 * nth) {
      float xv[8], qv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = e0 + u * nth < n ? e0 + u * nth : n - 1;
        const int t = e >> 5, c = e & 31;
        const bool isx = c < g.I, isq = c >= KX && c - KX < KH;
        xv[u] = xr[(size_t)t * g.sxT + (isx ? c : 0)];
        qv[u] = w.Qs[((size_t)t * B + rr) * KH + (isq ? c - KX : 0)];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = e0 + u * nth;
        const int c = e & 31;
        const bool isx = c < g.I, isq = c >= KX && c - KX < KH;
        if (e < n) bqr[e] = isx ? xv[u] : (isq ? qv[u] : 0.f);
      }
    }
  }

  if (wave == NC) {
    // ------------------------------------------------------------------ loader wave: tape + h_{t-1} into the LDS rings
    constexpr int MAXS = R3_MAXS;
    constexpr int NDMA = 4 * MAXS;
    constexpr int DEPTH = 2;
    constexpr int DIST = DEPTH + 2;
    static_assert(DIST < BWD_NB && 2 * NDMA <= 63 && DIST + 3 <= R4_NH, "rings");
    const bool has_h0 = w.h0 != nullptr;
    auto issue = [&](int ttarget) {   // tape of step ttarget (clamped at 0) -> ring slots
      const int tc = ttarget > 0 ? ttarget : 0;
      const int ring = ((ttarget % BWD_NB) + BWD_NB) % BWD_NB;
      const int ringh = ((ttarget % R4_NH) + R4_NH) % R4_NH;
#pragma unroll
      for (int i = 0; i < MAXS; ++i) {
        const bool real = i < NW;
        const int slot = lane + 64 * (real ? i : 0);
        const size_t e = (size_t)tc * sstride + (size_t)row * NT + slot;
        int n;
        if (!vg_slot_unit(g, slot, n)) n = 0;   // pad slots must not index past the row
        const size_t lo = (size_t)ring * NT + 64 * (real ? i : 0);
        dma16(a.gates + e * 4, real ? tg + lo * 4 : spare);
        dma4(a.cs + e, real ? tcp + lo : spare);                      // slice tc = c_{tc-1}
        dma4(has_dy ? a.dy + ((size_t)tc * g.syT + (size_t)row * g.syB + n) : a.cs + e, real ? tdy + lo : spare);
        // h_{tc-1}: y[tc-1]; step 0: h0 (without one the consumers mask the value)
        const float* hp = tc > 0 ? w.y + ((size_t)(tc - 1) * g.syT + (size_t)row * g.syB + n)
                                 : (has_h0 ? w.h0 + (size_t)row * H + n : w.y + (size_t)row * g.syB + n);
        dma4(hp, real ? th + (size_t)ringh * NT + 64 * i : spare);
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

  if (wave > NC) {
    // ------------------------------------------------------------------ accumulator waves
    const int aw = wave - NC - 1;                  // 0 .. NW-1: dpre tiles of the slots 64 aw ..; NW: the h^T dQ tiles
    const int li = lane & 31, lk = lane >> 5;
    const bool hmode = aw == NW;
    const int MT2 = (H + 31) / 32;
    f32x16 acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    float eh[4] = {0.f, 0.f, 0.f, 0.f}, ex[4] = {0.f, 0.f, 0.f, 0.f}, eb[4] = {0.f, 0.f, 0.f, 0.f};
    // element sums: this lane's thread slot (dpre waves)
    const int slot = 64 * (hmode ? 0 : aw) + lane;
    int un;
    const bool uv = vg_slot_unit(g, slot, un);
    const float hmask0 = (uv && !hmode) ? 1.f : 0.f;
    const bool xm = uv && un < g.I && !hmode;
    const int xcol = xm ? un : 0;
    const float h0mask = w.h0 != nullptr ? 1.f : 0.f;
    // h-mode A operand: unit 32 j + li of tile j
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");   // opening barrier (bq, zeroed partials published)

    // One MFMA contracts K = 2 (step, row) items: lanes 0-31 supply item 0, lanes 32-63 item 1.
    //   items (thi, row) and (thi - 1, row) - a pair of time steps (thi - 1 < 0: that half contributes nothing)
    auto pair = [&](int thi) {
      const int tt = thi - lk;
      const bool live = tt >= 0;
      const int tc = tt >= 0 ? tt : 0;
      const float* rb = lds0;
      if (!hmode) {
        const float bv = live ? rb[o_bq + (size_t)tc * 32 + li] : 0.f;
        const float* src = rb + o_outs + (size_t)(tc & (R4_NO - 1)) * NT * 4 + (size_t)(8 * aw) * 32 + li;
#pragma unroll
        for (int j0 = 0; j0 < 8; j0 += 4) {   // four operands at a time
          float av[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) av[j] = src[(j0 + j) * 32];
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j0 + j] = __builtin_amdgcn_mfma_f32_32x32x2f32(live ? av[j] : 0.f, bv, acc[j0 + j], 0, 0, 0);
        }
        // element sums of both items (every lane: its own slot)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int t2 = thi - s;
          const bool on = t2 >= 0;
          if (on) {   // wave-uniform
            const float* r2 = lds0;
            const float4 d = ld4(r2 + o_outs + (size_t)(t2 & (R4_NO - 1)) * NT * 4 + (size_t)slot * 4);
            const float hv = hmask0 * (t2 > 0 ? 1.f : h0mask) * r2[o_th + (size_t)(t2 & (R4_NH - 1)) * NT + slot];
            const float xv = xm ? r2[o_bq + (size_t)t2 * 32 + xcol] : 0.f;
            eh[0] = fmaf(d.x, hv, eh[0]), eh[1] = fmaf(d.y, hv, eh[1]), eh[2] = fmaf(d.z, hv, eh[2]), eh[3] = fmaf(d.w, hv, eh[3]);
            ex[0] = fmaf(d.x, xv, ex[0]), ex[1] = fmaf(d.y, xv, ex[1]), ex[2] = fmaf(d.z, xv, ex[2]), ex[3] = fmaf(d.w, xv, ex[3]);
            eb[0] += d.x, eb[1] += d.y, eb[2] += d.z, eb[3] += d.w;
          }
        }
      } else {
        // B: dQ_tt[rank li] = the partials' total, in the compute waves' order
        const float4 pq = ld4(rb + (size_t)(tc & (R4_NO - 1)) * 64 + (li & 15) * 4);
        const float bv = (live && li < KH) ? r3_total(pq) : 0.f;
        const float hm = (live && (tc > 0 || h0mask != 0.f)) ? 1.f : 0.f;
        const float* src = rb + o_th + (size_t)(tc & (R4_NH - 1)) * NT;
        float av[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          const int u = 32 * j + li;                       // G = 1: unit == thread slot
          av[j] = (j < MT2 && u < H) ? hm * src[u < NT ? u : 0] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 6; ++j)
          if (j < MT2) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv, acc[j], 0, 0, 0);
      }
    };
    // iteration t runs in front of barrier(t): steps > t are complete.
    //   pairs (T-1, T-2), (T-3, T-4), ... each as soon as its second step is complete
    for (int t = T - 1; t >= 0; --t) {
      if (t + 2 <= T - 1 && ((T - 1 - (t + 2)) & 1) == 0) pair(t + 2);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // barrier(t)
    }
    pair((T & 1) ? 0 : 1);   // what is left after barrier(0): the pair (1, 0), or step 0 alone

    // ---- the partial block of this workgroup (layout: vmlmf_atb.inc: C1 [NT*4][NB1p] | C2 [M2p][NB2p] | C3 | E [3][NT*4])
    const int NB1p = (vg_nb1(g) + 31) / 32 * 32, NB2p = (KH + 31) / 32 * 32, NB3p = (KX + 31) / 32 * 32;
    const int MT3 = (g.I + 31) / 32;
    const size_t o2 = (size_t)NT * 4 * NB1p, o3 = o2 + (size_t)MT2 * 32 * NB2p, oe = o3 + (size_t)MT3 * 32 * NB3p;
    float* P = w.P + (size_t)blockIdx.x * g.PCH;
    if (!hmode) {
      const int NB = KX + KH;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int mt = 8 * aw + j;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = (r & 3) + 8 * (r >> 2) + 4 * lk;
          if (li < NB) P[(size_t)(mt * 32 + i) * NB1p + li] = acc[j][r];
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        P[oe + 0 * (size_t)NT * 4 + (size_t)slot * 4 + k] = eh[k];
        P[oe + 1 * (size_t)NT * 4 + (size_t)slot * 4 + k] = ex[k];
        P[oe + 2 * (size_t)NT * 4 + (size_t)slot * 4 + k] = eb[k];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        if (j < MT2) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int i = (r & 3) + 8 * (r >> 2) + 4 * lk;
            if (li < KH) P[o2 + (size_t)(j * 32 + i) * NB2p + li] = acc[j][r];
          }
        }
      }
    }
    return;
  }

  // -------------------------------------------------------------------- compute waves (rec3_bwd_kernel's, rings 4 deep)
  const int uw = wave;                         // this wave's index among the compute waves
  const int utid = uw * 64 + lane;             // thread slot inside the row
  const bool valid = utid < H;
  const int n = valid ? utid : 0;
  const float dh_head = a.hd.C > 0 ? head_dh_body((const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr(), row, n, valid) : 0.f;
  const int li = lane & 15;
  const int d = (__float_as_int(ror16<1>(__int_as_float(li))) - li) & 15;
  f32x2 vz[4][8];
  float ue[16], eh[4];
  if (a.wr.direct != 0) {
    // direct mode (vmlmf_direct.inc): this unit's own rows of v_h / u_h, rotated by the lane's place in its DPP row in registers
    float vr[4][16], ur0[16];
#pragma unroll
    for (int gk = 0; gk < 4; ++gk) dr_load_row<KH>(a.VE, (size_t)gk * H + n, valid, vr[gk]);
    dr_load_row<KH>(a.UE, (size_t)n, valid, ur0);
    const float dh = a.EH[n], vf = valid ? 1.f : 0.f;
    float* scr = outs + (size_t)utid * DR_SCR_FLOATS;   // this lane's LDS slot (dr_put / dr_at: a register array indexed per lane)
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
  } else {
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int rr = (li - d * k) & 15, re = (li + d * k) & 15;
    const bool inr = rr < KH, ine = re < KH;
#pragma unroll
    for (int gk = 0; gk < 4; ++gk) {
      const float v = a.VE[(size_t)(gk * KH + (inr ? rr : 0)) * NT + utid];
      const float vv = inr ? v : 0.f;
      if (k & 1) vz[gk][k >> 1].y = vv;
      else vz[gk][k >> 1].x = vv;
    }
    const float u = a.UE[(size_t)(ine ? re : 0) * NT + utid];
    ue[k] = ine ? u : 0.f;
  }
#pragma unroll
  for (int gk = 0; gk < 4; ++gk) eh[gk] = a.EH[gk * NT + utid];
  }

  float dhrec, dcs, ccur;
  {
    const size_t bh = (size_t)row * H + n;
    dhrec = (valid && a.dhT != nullptr) ? a.dhT[bh] : 0.f;
    dhrec += dh_head;
    dcs = (valid && a.dcT != nullptr) ? a.dcT[bh] : 0.f;
    ccur = a.cs[(size_t)T * sstride + (size_t)row * NT + utid];
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");   // opening barrier: tapes T-1 and T-2 have landed

  float4 g4n;
  float cprvn, dyvn;
  auto fetch_tape = [&](int tt) {
    const int ringn = ((tt % BWD_NB) + BWD_NB) % BWD_NB;
    const size_t lo = (size_t)ringn * NT + utid;
    g4n = ld4(tg + lo * 4);
    cprvn = tcp[lo];
    dyvn = tdy[lo];
  };
  CellBwdFactors fac;
  float fdy;
  auto prepare = [&]() {   // the factors of a step's gate derivatives that do not depend on dh
    fac = cell_bwd_factors(g4n, ccur, cprvn);
    fdy = (valid && has_dy) ? dyvn : 0.f;
    ccur = cprvn;
  };
  fetch_tape(T - 1);
  prepare();
  __builtin_amdgcn_s_setprio(2);   // the chain outranks the accumulator wave it shares its SIMD with
  for (int t = T - 1; t >= 0; --t) {
    const int buf = t & (R4_NO - 1);
    fetch_tape(t - 1);
    const float4 dp = cell_bwd_step(fac, fdy + dhrec, dcs);
    st4(outs + (size_t)buf * NT * 4 + (size_t)utid * 4, dp);
    const float ehterm = cell_ehterm_fma(dp, eh[0], eh[1], eh[2], eh[3]);   // (explicit fused multiply-adds: see there)
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
    if (lane < 16) part[buf * 64 + lane * 4 + uw] = s;
    prepare();
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // barrier(t)
    const float4 p = ld4(part + buf * 64 + (lane & 15) * 4);
    float tot = r3_total(p);
    dpp_fence(tot);
    dhrec = ehterm + fmac_ror_x16_4(tot, ue);
  }
  if (valid) {
    if (a.dh0 != nullptr) a.dh0[(size_t)row * H + n] = dhrec;
    if (a.dc0 != nullptr) a.dc0[(size_t)row * H + n] = dcs;
  }
}

// which layers: rec3_bwd_kernel's, with the x-fold (the x side of the product contracts x itself) and [x | Q] in one 32-column
// tile; the row's [x | Q] sequence and the rings must fit the LDS
__host__ inline bool rec4_bwd_ok(const VGeo& g) {
  if (!rec3_bwd_ok(g) || !g.foldx || g.KX + g.KH > 32 || g.I > g.KX || g.T < 2) return false;
  return sizeof(float) * rec4_bwd_lds_floats(g.NT, g.T) <= 150 * 1024;
}

template <int KH>
static int rec4_bwd_launch_kh(const VGeo& g, const BwdArgs& a, hipStream_t s) {
  const size_t lds = sizeof(float) * rec4_bwd_lds_floats(g.NT, g.T);
  auto kern = rec4_bwd_kernel<KH>;
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kern, dim3(g.B), dim3(2 * g.NT + 128), lds, s, g, a);
  return (int)hipGetLastError();
}
