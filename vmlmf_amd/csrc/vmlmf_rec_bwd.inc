// Persistent recurrent backward kernel (gfx950).  Included by vmlmf_rec_bwd_kh*.hip.  Mirror image of
// rec_fwd_kernel: NW compute waves (thread <-> hidden unit) + one mover wave.
//   vr[4][KQ]  rotated image of this row's V_h for the DPP reduce   dQ = sum_{k,n} dpre[k][n] V_h[k][n][:]
//   ue2[KH/2]  this unit's own U_h weights (pairs)                  dh_{t-1} = dQ . ue + dpre . eh
// Compute waves per timestep (one LDS-only barrier, no global memory instruction): gate derivatives from
// the tape staged in LDS by the mover (gates, c_{t-1}, dy) -> dpre into an LDS out-stage -> rank-space
// reduce -> barrier -> expand to dh_{t-1}.  The mover DMAs the tape of step t-3 into the LDS ring, drains
// dpre of step t+1 to HBM (input of the weight-gradient kernels) and stores dQ[t].
// Weight gradients are NOT accumulated here: they are batched sums over all (t,b) and run on the whole chip
// in wgrad_mfma afterwards, off the serial chain.
// Replaces autograd's replay of the time loop (SURVEY.md section 8a, row a7).
#include "vmlmf_launch.h"
#include "vmlmf_atb.inc"

constexpr int BWD_NB = 6;   // depth of the tape ring in LDS

// a counted vmcnt wait whose count is only known at run time (wave-uniform): at most n vector-memory operations outstanding
// (exact up to 49; a larger n waits for 49, which is stricter)
__device__ __forceinline__ void wait_vm_dyn(int n) {
  switch (n) {
#define WVM(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break
    WVM(0); WVM(1); WVM(2); WVM(3); WVM(4); WVM(5); WVM(6); WVM(7); WVM(8); WVM(9); WVM(10); WVM(11); WVM(12); WVM(13);
    WVM(14); WVM(15); WVM(16); WVM(17); WVM(18); WVM(19); WVM(20); WVM(21); WVM(22); WVM(23); WVM(24); WVM(25); WVM(26);
    WVM(27); WVM(28); WVM(29); WVM(30); WVM(31); WVM(32); WVM(33); WVM(34); WVM(35); WVM(36); WVM(37); WVM(38); WVM(39);
    WVM(40); WVM(41); WVM(42); WVM(43); WVM(44); WVM(45); WVM(46); WVM(47); WVM(48);
#undef WVM
    default: asm volatile("s_waitcnt vmcnt(49)" ::: "memory"); break;
  }
}

// The weight-gradient workers of a RIDE launch: workgroups behind the rows', one wave per task (vmlmf_atb.inc).
template <int NBT>
__device__ __forceinline__ void wride_worker(const VGeo& g, const WRide& w) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wb = blockIdx.x - g.nwg, k = wb / w.ntg, tg = wb - k * w.ntg;
  const int task = tg * (blockDim.x >> 6) + wave;
  const int MT1 = g.NT / 8, MT2 = (g.H + 31) / 32;
  extern __shared__ float4 smem4[];
  float* word = reinterpret_cast<float*>(smem4);   // the poll result of wave 0, handed to the other waves
  // (a wave without a task leaves: the barriers of the others do not count it)
  if (task < MT1) {
    // its tile's share of d(u_x) (WRide::dux): the 32 rows of v_x its (slot, gate) columns meet go into LDS now, while the rows'
    // recurrence has not produced anything yet: [row i of the tile][16 ranks], rank columns beyond rw zero
    float* vxs = word + 64 + (size_t)wave * 512;
    if (w.dux != nullptr) {
      const int i = lane >> 1, hf = lane & 1;
      const int slot = task * 8 + (i >> 2), kk = i & 3;
      int n;
      const bool uv = vg_slot_unit(g, slot, n);
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int r = hf * 8 + j;
        v[j] = w.vx[((size_t)kk * g.H + (uv ? n : 0)) * g.rw + (r < g.rw ? r : 0)];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) vxs[i * 16 + hf * 8 + j] = (uv && hf * 8 + j < g.rw) ? v[j] : 0.f;
    }
    atb_ride_task<1, NBT, 1, true>(g, w.a, task, k, lane, 0, word, w.prog, w.K, w.S, wave, w.spin, w.status, w.dux, vxs);
  }
  else if (task < MT1 + MT2)
    atb_ride_task<2, NBT, 1, true>(g, w.a, task - MT1, k, lane, 0, word, w.prog, w.K, w.S, wave, w.spin, w.status);
}

// (Inlined on purpose although every change of the worker's code moves the register allocation of the rows' half of the
// kernel, whose storer wave is on the critical path of the step - 0.164 <-> 0.172 ms at the headline shape for changes that
// only touched the worker: behind a noinline call the launch aborted with a memory fault that tools/check_asm_hazards.py
// does not explain.)
// Classifier prologue (HeadBwd): the gradient the classifier sends into the final hidden state, d(hT)[n] = sum_c dlogits[row][c]
// W[c][n], formed where it is consumed instead of by a launch of head_bwd_kernel in front of this kernel (its dW / db halves
// are outputs of finish_kernel).  Not inlined, fed from the kernel-argument segment: inlined it raised the kernel from 110 to
// 167 VGPRs (three instead of four workgroups per CU at large batches) for the same time.
__device__ __forceinline__ float head_dh_body(const __attribute__((address_space(4))) char* ka, int row, int n, bool ok) {
  typedef __attribute__((address_space(4))) int karg_i;
  constexpr size_t off = ((sizeof(VGeo) + 7) & ~(size_t)7) + offsetof(BwdArgs, hd);
  if (((const karg_i*)(ka + off + offsetof(HeadBwd, C)))[0] <= 0) return 0.f;   // no classifier: one scalar load and out
  HeadBwd hd;
  {
    const karg_i* w = (const karg_i*)(ka + off);
    int tmp[sizeof(HeadBwd) / 4];
#pragma unroll
    for (unsigned i = 0; i < sizeof(HeadBwd) / 4; ++i) tmp[i] = w[i];
    __builtin_memcpy(&hd, tmp, sizeof(HeadBwd));
  }
  if (hd.C <= 0) return 0.f;
  const karg_i* gw = (const karg_i*)ka;
  const int H = gw[offsetof(VGeo, H) / 4];
  // all 2 x 32 loads go out (clamped indices) before the first FMA: as a loop over the classes this was a chain of C memory
  // latencies in front of the recurrence (5.7 us at 18 classes)
  float w[32], d[32];
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    const int cc = c < hd.C ? c : 0;
    w[c] = hd.W[(size_t)cc * H + n];
    d[c] = hd.dl[(size_t)row * hd.C + cc];
  }
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
  for (int c = 0; c < 32; c += 4) {
    a0 = fmaf(c + 0 < hd.C ? d[c + 0] : 0.f, w[c + 0], a0);
    a1 = fmaf(c + 1 < hd.C ? d[c + 1] : 0.f, w[c + 1], a1);
    a2 = fmaf(c + 2 < hd.C ? d[c + 2] : 0.f, w[c + 2], a2);
    a3 = fmaf(c + 3 < hd.C ? d[c + 3] : 0.f, w[c + 3], a3);
  }
  return ok ? (a0 + a1) + (a2 + a3) : 0.f;
}
__device__ __attribute__((noinline)) float head_dh(const __attribute__((address_space(4))) char* ka, int row, int n, bool ok) {
  return head_dh_body(ka, row, n, ok);
}

// RIDE (0 = off, else the 32-wide B tiles of the products): the launch carries wr.K * wr.ntg more workgroups that form the
// weight gradients behind the rows (wride_worker); the rows' storer waves write through and publish their progress.
template <int KH, int R, bool FLAT, int MAXT, int CNT, int RIDE = 0>
__global__ void __launch_bounds__(VG_REC_BOUNDS) rec_bwd_kernel(VGeo g, BwdArgs a) {
  constexpr int NP = (KH + 15) / 16, KQ = NP * 16, NC = KH / 4;
  constexpr int NJ = FLAT ? 2 : 1;  // rank-space vectors a wave contributes to
  if constexpr (RIDE > 0) {
    if ((int)blockIdx.x >= g.nwg) {
      wride_worker<RIDE>(g, a.wr);
      return;
    }
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NT = g.NT, NW = g.NW, W = g.W, H = g.H, B = g.B, T = g.T;
  const bool mover = tid >= NT;
  const bool has_dy = a.dy != nullptr;
  const size_t sstride = (size_t)g.Bp * NT;

  extern __shared__ float4 smem4[];
  float* part = reinterpret_cast<float*>(smem4);      // [2][R][NW][NJ][KQ]
  float* tg = part + 2 * R * NW * NJ * KQ;            // [BWD_NB][R][NT][4]  gates of the step
  float* tcp = tg + BWD_NB * R * NT * 4;              // [BWD_NB][R][NT]     c_{t-1}
  float* tdy = tcp + BWD_NB * R * NT;                 // [BWD_NB][R][NT]     dy_t
  float* outs = tdy + BWD_NB * R * NT;                // [2][R][NT][4]       dpre
  float* spare = outs + 2 * R * NT * 4;               // 256 floats: target of the dummy DMAs
  float* zero4 = spare + 256;                         // 4 zero floats
  if (tid < 4) zero4[tid] = 0.f;

  if (mover) {
    // ------------------------------------------------------------------ loader + storer waves (see rec_fwd_kernel)
    constexpr int MAXS = MAXT / 64;
    constexpr int NDMA = 3 * R * MAXS;
    constexpr int DEPTH = (2 * NDMA <= 63) ? 2 : 1;
    constexpr int DIST = DEPTH + 2;
    static_assert(DIST < BWD_NB, "tape ring too shallow");
    int row[R];
    bool rok[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      row[r] = blockIdx.x * R + r;
      rok[r] = row[r] < B;
    }
    if (wave == NW) {
      auto issue = [&](int ttarget) {   // tape of step ttarget (clamped at 0) -> ring slot
        const int tc = ttarget > 0 ? ttarget : 0;
        const int ring = ((ttarget % BWD_NB) + BWD_NB) % BWD_NB;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int rowc = rok[r] ? row[r] : B - 1;
#pragma unroll
          for (int i = 0; i < MAXS; ++i) {
            const bool real = i < NW;
            const int slot = lane + 64 * (real ? i : 0);
            const size_t e = (size_t)tc * sstride + (size_t)row[r] * NT + slot;
            int n;
            if (!vg_slot_unit(g, slot, n)) n = 0;   // pad slots must not index past the row (last row: past dy)
            const size_t lo = ((size_t)ring * R + r) * NT + 64 * (real ? i : 0);
            dma16(a.gates + e * 4, real ? tg + lo * 4 : spare);
            dma4(a.cs + e, real ? tcp + lo : spare);                      // slice tc = c_{tc-1}
            dma4(has_dy ? a.dy + ((size_t)tc * g.syT + (size_t)rowc * g.syB + n) : a.cs + e, real ? tdy + lo : spare);
          }
        }
      };
      for (int s0 = 0; s0 < DIST; ++s0) issue(T - 1 - s0);    // tapes T-1 .. T-DIST
      wait_vm_barrier<(DIST - 2) * NDMA>();                   // opening barrier: tapes T-1 and T-2 have landed
      // segment t: between the barrier that published step t+1 and barrier(t)
      for (int t = T - 1; t >= 0; --t) {
        issue(t - DIST);
        wait_vm_barrier<DEPTH * NDMA>();                      // barrier(t): tape t-2 has landed
      }
      return;
    }
    // per-lane constants of the storer: the dQ elements it owns
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
      qv[q] = in && (blockIdx.x * R + r) < B;
      // non-FLAT: waves of group j;  FLAT: every wave, vector j
      qsrc[q] = FLAT ? (unsigned)(((r * NW) * NJ + j) * KQ + rr) : (unsigned)((r * NW + j * W) * KQ + rr);
      qdst[q] = (unsigned)((blockIdx.x * R + r) * GK + jr);
    }
    // stores behind a possible reload of their scalar base (vmlmf_device.h, hazard 2): the instantiations
    // tools/check_asm_hazards.py flags without it
    // (set for exactly the instantiations the checker flags: the stores' wait states cost the storer wave, which is on the
    // critical path of the step, ~7 us per 128 steps.  A change anywhere in this kernel - the worker half included - can move
    // the register allocation and make the checker flag others: add them here.)
    constexpr bool SAFE_ST = RIDE == 2 && KH > 16;
    // every LDS read of a step is issued before the first global store (see rec_fwd_kernel's storer)
    auto drain = [&](int ts) {   // dpre of step ts -> HBM (slot-padded: every slot is written)
      const float* src = outs + (size_t)(ts & 1) * R * NT * 4;
      float* dt = a.dpre + (size_t)ts * sstride * 4;
      float4 d4[R][MAXS];
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int i = 0; i < MAXS; ++i) d4[r][i] = ld4(src + ((size_t)r * NT + lane + 64 * (i < NW ? i : 0)) * 4);
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int i = 0; i < MAXS; ++i)
          if (i < NW) {
            if constexpr (RIDE > 0) st4_sv_sys<SAFE_ST>(dt, 16u * (unsigned)(row[r] * NT + lane + 64 * i), d4[r][i]);
            else st4_sv(dt, 16u * (unsigned)(row[r] * NT + lane + 64 * i), d4[r][i]);
          }
    };
    auto store_dq = [&](int ts) {
      const float* src = part + (size_t)(ts & 1) * R * NW * NJ * KQ;
      float* qt = a.dQs + (size_t)ts * B * g.G * KH;
      const int cnt = FLAT ? NW : W;
      float v[QE][MAXS];
#pragma unroll
      for (int q = 0; q < QE; ++q)
#pragma unroll
        for (int w = 0; w < MAXS; ++w) v[q][w] = src[qsrc[q] + (w < cnt ? w : 0) * NJ * KQ];   // independent reads
#pragma unroll
      for (int q = 0; q < QE; ++q) {
        if (RIDE > 0 && 64 * q >= R * g.G * KH) continue;   // (wave-uniform: a RIDE segment issues a known number of stores)
        if (qv[q]) {
          float acc = 0.f;
#pragma unroll
          for (int w = 0; w < MAXS; ++w) acc += w < cnt ? v[q][w] : 0.f;
          if constexpr (RIDE > 0) st1_sv_sys<SAFE_ST>(qt, 4u * qdst[q], acc);
          else st1_sv(qt, 4u * qdst[q], acc);
        }
      }
    };
    // RIDE: stores per segment = NW row slices of dpre + the dQ stores (R = 1: lane 0 of each is live, none is skipped) + the
    // progress word; a word published in segment t covers the steps whose stores are older than the last lag - 1 segments
    static_assert(RIDE == 0 || R == 1, "progress words: one row per workgroup");
    const int nd = NW + (R * g.G * KH + 63) / 64;
    const int lag = a.wr.lag;   // segments between a step's stores and the progress word that covers them
    // (every other segment without its word: counting nd per earlier segment is the safe side)
    const int nwait = nd * lag;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // opening barrier
    for (int t = T - 1; t >= 0; --t) {   // segment t: step t+1 is complete
      if (t + 1 < T) {
        drain(t + 1);
        store_dq(t + 1);
        if constexpr (RIDE > 0) {
          wait_vm_dyn(nwait);
          const int done = T - (t + 1 + lag);   // steps T-1 .. t+1+lag are in memory
          if (lane == 0 && (t & 1) == 0)
            st1_sv_sys<SAFE_ST>(a.wr.prog, 4u * (unsigned)(row[0] * WR_PROG_STRIDE), (unsigned)(done > 0 ? done : 0));
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // barrier(t)
    }
    drain(0);
    store_dq(0);
    if constexpr (RIDE > 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) st1_sv_sys<SAFE_ST>(a.wr.prog, 4u * (unsigned)(row[0] * WR_PROG_STRIDE), (unsigned)T);
    }
    return;
  }

  // -------------------------------------------------------------------- compute waves
  const int grp = tid / (64 * W);
  const int m = tid - grp * 64 * W;
  const bool valid = m < g.Hg;
  const int n = grp * g.Hg + (valid ? m : 0);

  // classifier prologue FIRST, while nothing else is live: a callee's registers sit on top of the caller's live ones, and
  // called after the weights were loaded this function raised the kernel from 110 to 166 VGPRs (three instead of four
  // workgroups per SIMD set: config D on one GPU lost 9 %)
  float dh_head[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = blockIdx.x * R + r;
    // (RIDE: one workgroup per CU whatever the register count, and no call in a kernel this large: the combined kernel with the
    // call faulted - scalar registers spilled into vector lanes around it - whenever the worker's half changed)
    if constexpr (RIDE > 0)
      dh_head[r] = a.hd.C > 0 ? head_dh_body((const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr(),
                                             row < B ? row : B - 1, n, valid && row < B)
                              : 0.f;
    else
    dh_head[r] = a.hd.C > 0 ? head_dh((const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr(),
                                      row < B ? row : B - 1, n, valid && row < B)
                            : 0.f;
  }

  float vr[4][KQ];
  f32x2 ue2[KH / 2];
  float eh[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int j = 0; j < KQ; ++j) vr[k][j] = a.VR[(size_t)(k * KQ + j) * NT + tid];
    eh[k] = a.EH[k * NT + tid];
  }
#pragma unroll
  for (int rr = 0; rr < KH / 2; ++rr)
    ue2[rr] = f32x2{a.UE[(size_t)(2 * rr) * NT + tid], a.UE[(size_t)(2 * rr + 1) * NT + tid]};

  // chunk c of block s: this unit needs dQ[dest][chunk], dest = (grp - s) mod G.
  //   non-FLAT: contributors are the W waves of group dest (qsel = group of the unit)
  //   FLAT:     every wave contributes to both vectors; slot [wave][dest]
  int pb[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int s = (g.G == 2 && 4 * c >= g.off1) ? 1 : 0;
    const int dst = (grp - s + g.G) % g.G;
    pb[c] = FLAT ? (dst * KQ + 4 * c) : (dst * W * KQ + 4 * c);
  }
  constexpr int wstride = NJ * KQ;
  // cooperative cross-wave sum (see rec_fwd_kernel)
  constexpr int NCP = NC <= 2 ? 2 : (NC <= 4 ? 4 : 8);
  constexpr bool FASTQ16 = !FLAT && NC == NCP && NC * CNT <= 16;
  constexpr bool FASTQ64 = !FLAT && !FASTQ16 && NC <= 8 && NCP * CNT <= 64;   // all 64 lanes + rowsum4 (see rec_fwd_kernel)
  constexpr bool FLATQ = FLAT && NC <= 8 && NCP * CNT <= 64;   // V4: every wave contributes, slot [wave][dest]
  constexpr bool FASTQ = FASTQ16 || FASTQ64 || FLATQ;
  int rdoff = 0;
  {
    const int li = (FASTQ64 || FLATQ) ? lane : (lane & 15), cc = li % NCP, w = li / NCP;
    const int ccl = cc < NC ? cc : 0;
    const int s = (g.G == 2 && 4 * ccl >= g.off1) ? 1 : 0;
    const int dst = (grp - s + g.G) % g.G;
    rdoff = (w < CNT && cc < NC) ? (FLATQ ? ((w * NJ + dst) * KQ + 4 * cc) : ((dst * W + w) * KQ + 4 * cc)) : -1;
  }

  bool ok[R];
  float dhrec[R], dcs[R], ccur[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = blockIdx.x * R + r;
    ok[r] = valid && row < B;
    const int rowc = row < B ? row : B - 1;
    const size_t bh = (size_t)rowc * H + n;
    dhrec[r] = (ok[r] && a.dhT != nullptr) ? a.dhT[bh] : 0.f;
    dhrec[r] += dh_head[r];
    dcs[r] = (ok[r] && a.dcT != nullptr) ? a.dcT[bh] : 0.f;
    ccur[r] = a.cs[(size_t)T * sstride + (size_t)row * NT + tid];
  }

  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");   // barrier for step T-1
  // The tape of a step is read from the LDS ring one half-step early (right after the previous step's barrier,
  // when the loader guarantees it has landed), so that its ~130 cycles of LDS latency hide under the expansion
  // FMAs instead of opening every step's dependent chain.
  // Everything of a step's gate derivatives that does not depend on dh_t is prepared during the previous step's
  // second half as well (factors A, F0..F3 below), which leaves seven dependent operations between dhrec and
  // the DPP reduce instead of about twenty-five.
  float4 g4n[R];
  float cprvn[R], dyvn[R];
  auto fetch_tape = [&](int tt) {
    const int ringn = ((tt % BWD_NB) + BWD_NB) % BWD_NB;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const size_t lo = ((size_t)ringn * R + r) * NT + tid;
      g4n[r] = ld4(tg + lo * 4);
      cprvn[r] = tcp[lo];
      dyvn[r] = tdy[lo];
    }
  };
  CellBwdFactors fac[R];
  float fdy[R];
  auto prepare = [&]() {   // from the fetched tape and c of the step (ccur): the dh-independent factors
#pragma unroll
    for (int r = 0; r < R; ++r) {
      fac[r] = cell_bwd_factors(g4n[r], ccur[r], cprvn[r]);
      fdy[r] = (ok[r] && has_dy) ? dyvn[r] : 0.f;
      ccur[r] = cprvn[r];   // c of the step before
    }
  };
  fetch_tape(T - 1);
  prepare();
  for (int t = T - 1; t >= 0; --t) {
    const int buf = t & 1;
    float* ot = outs + (size_t)buf * R * NT * 4;
    float ehterm[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float dh = fdy[r] + dhrec[r];
      const float4 d = cell_bwd_step(fac[r], dh, dcs[r]);
      float dp[4] = {d.x, d.y, d.z, d.w};
      st4(ot + ((size_t)r * NT + tid) * 4, d);
      ehterm[r] = cell_ehterm(d, eh[0], eh[1], eh[2], eh[3]);
      // rank-space reduce of dpre
      asm volatile("s_nop 1" : "+v"(dp[0]), "+v"(dp[1]), "+v"(dp[2]), "+v"(dp[3]));   // one DPP fence for the four
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        fmac_ror_4x4<0>(acc, dp, &vr[0][p * 16], &vr[1][p * 16], &vr[2][p * 16], &vr[3][p * 16]);
        fmac_ror_4x4<4>(acc, dp, &vr[0][p * 16], &vr[1][p * 16], &vr[2][p * 16], &vr[3][p * 16]);
        fmac_ror_4x4<8>(acc, dp, &vr[0][p * 16], &vr[1][p * 16], &vr[2][p * 16], &vr[3][p * 16]);
        fmac_ror_4x4<12>(acc, dp, &vr[0][p * 16], &vr[1][p * 16], &vr[2][p * 16], &vr[3][p * 16]);
        float* wdst = part + ((size_t)((buf * R + r) * NW + wave) * NJ) * KQ + p * 16 + lane;
        if (FLAT) {
          const float s0 = rowsum4(acc[0] + acc[1]);
          const float s1 = rowsum4(acc[2] + acc[3]);
          if (lane < 16) {
            wdst[0] = s0;
            wdst[KQ] = s1;
          }
        } else {
          const float s0 = rowsum4((acc[0] + acc[1]) + (acc[2] + acc[3]));
          if (lane < 16) wdst[0] = s0;
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    fetch_tape(t - 1);   // landed since the previous barrier (t = 0: reads a valid, unused ring slot)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float* src = part + (size_t)(buf * R + r) * NW * NJ * KQ;
      float4 q[NC];
      if constexpr (FASTQ) {
        const float4 v = ld4(rdoff >= 0 ? src + rdoff : zero4);
        float sx = class_sum16<NCP>(v.x), sy = class_sum16<NCP>(v.y);
        float sz = class_sum16<NCP>(v.z), sw = class_sum16<NCP>(v.w);
        if constexpr (FASTQ64 || FLATQ) sx = rowsum4(sx), sy = rowsum4(sy), sz = rowsum4(sz), sw = rowsum4(sw);
#pragma unroll
        for (int cc = 0; cc < NC; ++cc)
          q[cc] = make_float4(bcast_lane(sx, cc), bcast_lane(sy, cc), bcast_lane(sz, cc), bcast_lane(sw, cc));
      }
#pragma unroll
      for (int cc = 0; cc < (FASTQ ? 0 : NC); ++cc) {
        float4 v[CNT];
#pragma unroll
        for (int w = 0; w < CNT; ++w) v[w] = ld4(src + pb[cc] + w * wstride);
        q[cc] = v[0];
#pragma unroll
        for (int w = 1; w < CNT; ++w) q[cc] = f4add(q[cc], v[w]);
      }
      f32x2 d2 = f32x2{ehterm[r], 0.f}, d2b = f32x2{0.f, 0.f};   // two chains
#pragma unroll
      for (int cc = 0; cc < NC; ++cc) {
        d2 = pk_fma(f32x2{q[cc].x, q[cc].y}, ue2[2 * cc + 0], d2);
        d2b = pk_fma(f32x2{q[cc].z, q[cc].w}, ue2[2 * cc + 1], d2b);
      }
      d2 = d2 + d2b;
      dhrec[r] = d2.x + d2.y;
    }
    prepare();   // factors of step t-1 (its tape was fetched after the barrier)
  }

#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = blockIdx.x * R + r;
    if (ok[r]) {
      if (a.dh0 != nullptr) a.dh0[(size_t)row * H + n] = dhrec[r];
      if (a.dc0 != nullptr) a.dc0[(size_t)row * H + n] = dcs[r];
    }
  }
}

template <int KH, int R, bool FLAT, int MAXT, int CNT>
static int bwd_launch_one(const VGeo& g, const BwdArgs& a, hipStream_t s) {
  constexpr int KQ = (KH + 15) / 16 * 16;
  const size_t lds = sizeof(float) * ((size_t)2 * R * g.NW * (FLAT ? 2 : 1) * KQ + (size_t)BWD_NB * R * g.NT * 6 +
                                      (size_t)2 * R * g.NT * 4 + 256 + 4);
  // with the weight-gradient workers behind the rows (wr.K: chosen by the caller: plan_wride asks for the x-fold, which the flat
  // layout's LM layers - input as wide as the hidden state - never have)
  // (instantiated where rec3_bwd_kernel<KH, 1> does not cover the layer - rec_bwd_rides() in vmlmf_launch.h: with
  //  vmlmf_tune("rec3", 0) the layers it covers take the stand-alone weight-gradient launch instead)
  if constexpr (MAXT == 256 && R == 1 && !FLAT && (KH > 16 || CNT > 3)) {
    if (a.wr.K > 0) {
      const int n1 = (vg_nb1(g) + 31) / 32, n2 = (g.G * g.KH + 31) / 32;
      if (n1 > 2 || n2 > 2) return -3;
      // more than half a CU's LDS per workgroup: ONE workgroup per CU, so that a worker never shares a CU (and its issue
      // slots) with a row's recurrence
      const size_t lds1 = lds > 84 * 1024 ? lds : (size_t)84 * 1024;
      const dim3 grid(g.nwg + a.wr.K * a.wr.ntg), block(g.NT + 128);
      // (one riding instantiation, two 32-wide B tiles: a layer whose products need one tile - e.g. two groups of rank 8 - runs it
      //  with the second tile's MFMAs on zeros; the one-tile form exists where it matters, rec3_bwd_kernel<KH, 1> of configs A / D)
      auto kern = rec_bwd_kernel<KH, R, FLAT, MAXT, CNT, 2>;
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1);
      if (e != hipSuccess) return (int)e;
      hipLaunchKernelGGL(kern, grid, block, lds1, s, g, a);
      return (int)hipGetLastError();
    }
  }
  if (a.wr.K > 0) return -3;
  auto kern = rec_bwd_kernel<KH, R, FLAT, MAXT, CNT>;
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kern, dim3(g.nwg), dim3(g.NT + 128), lds, s, g, a);
  return (int)hipGetLastError();
}

// (instantiations: rec_fwd's table - only the (slot tier, waves per consumer) pairs a layer can have; a consumer of the flat V4
//  layout sums all NW = 2 W waves)
template <int KH, int MAXT, int CNT, bool FLAT>
static int bwd_launch_mode(const VGeo& g, const BwdArgs& a, hipStream_t s) {
  if (g.R != 1 || (FLAT && g.G != 2)) return -3;
  return bwd_launch_one<KH, 1, FLAT, MAXT, CNT>(g, a, s);
}

template <int KH>
static int bwd_launch_kh(const VGeo& g, const BwdArgs& a, hipStream_t s) {
  const int cnt = g.flat ? g.NW : g.W;  // waves summed by a consumer
  if (g.flat) {
    if (g.NT <= 256) {
      if (cnt == 2) return bwd_launch_mode<KH, 256, 2, true>(g, a, s);
      if (cnt == 4) return bwd_launch_mode<KH, 256, 4, true>(g, a, s);
    } else if (g.NT <= 384) {
      if (cnt == 6) return bwd_launch_mode<KH, 384, 6, true>(g, a, s);
    } else if (g.NT <= 512) {
      if (cnt == 8) return bwd_launch_mode<KH, 512, 8, true>(g, a, s);
    }
    return -3;
  }
  if (g.NT <= 256) {
    switch (cnt) {
      case 1: return bwd_launch_mode<KH, 256, 1, false>(g, a, s);
      case 2: return bwd_launch_mode<KH, 256, 2, false>(g, a, s);
      case 3: return bwd_launch_mode<KH, 256, 3, false>(g, a, s);
      case 4: return bwd_launch_mode<KH, 256, 4, false>(g, a, s);
    }
  } else if (g.NT <= 384) {
    // 6 compute waves + 2 movers = 8 waves = two per SIMD: the 256-VGPR budget the wide ranks need (the 512-slot
    // tier below is compiled for 10 waves, 168 VGPRs, and spills at these ranks: 1.13 ms instead of 0.4 at H = 384);
    // for ranks <= 16 it is 2 % faster than the 512 tier (fewer mover slots per step)
    switch (cnt) {
      case 3: return bwd_launch_mode<KH, 384, 3, false>(g, a, s);
      case 5: return bwd_launch_mode<KH, 384, 5, false>(g, a, s);
      case 6: return bwd_launch_mode<KH, 384, 6, false>(g, a, s);
    }
  } else if (g.NT <= 512) {
    switch (cnt) {
      case 4: return bwd_launch_mode<KH, 512, 4, false>(g, a, s);
      case 7: return bwd_launch_mode<KH, 512, 7, false>(g, a, s);
      case 8: return bwd_launch_mode<KH, 512, 8, false>(g, a, s);
    }
  }
  return -3;
}
