// Wavefront kernels for stacked layers (gfx950).  Included by vmlmf_wave_k*.hip (one TU per padded rank).
//
// The time loop of a stack, vmlmf.py:300-314 (MyLSTM.forward: `for t: for layer: h,c = cell(x,h,c); x = h`) and
// vmlmf_lm.py:437-439, as ONE launch per direction: workgroup = (layer, batch row).  A workgroup is the persistent
// recurrent workgroup of vmlmf_rec_fwd.inc / vmlmf_rec_bwd.inc (thread <-> hidden unit, U_h / V_h in registers, DPP rank
// reduce, one barrier per step) plus an X-TEAM of as many waves that does the layer's x side in-kernel:
//   forward   gx[t] = (x_t U_x) V_x^T + x_t .* ex + b       (the same reduce / expand shape as the h side, U_x / V_x in the
//                                                             x-team's registers; replaces xproj_kernel and its gx round trip)
//   backward  dqx[t] = dpre[t] V_x,  dx[t] = dqx[t] U_x^T + dpre[t] .* ex      (replaces dqx_dx_kernel)
// The x side has no recurrence, so the team runs two steps ahead (forward) / behind (backward) of the compute waves on
// the SIMD issue slots their dependent chain leaves idle.  Above the first layer x_t is the h_t of the layer below: its
// storer wave writes y[t] through to memory and publishes a progress word per row, this layer's loader wave polls it
// before it DMAs the row into LDS, so a layer runs ~9 steps (7 us) behind the one below instead of after it.  Backward mirrors
// it with dx of the layer above = dy of this one.  Workgroups of one row group (8 rows x L layers) have consecutive block
// ids: the producer is always dispatched before its consumer (no deadlock however many workgroups are resident), and a row's
// layers land on one XCD (block b -> XCD b % 8), so the hand-over stays in that L2 (speed only: every hand-over is
// system-scope write-through + polled word).  A classifier on the top layer's final hidden state (Net.lin) rides on the
// launches: logits in the forward epilogue, d(hT) formed by the top layer's loader wave in the backward prologue.
//
// Rank reduce with a HALF pass: ranks are padded to multiples of 8; a block of 16 ranks takes 16 row_ror steps (lane i
// of a 16-lane row owns rank i), a trailing block of 8 takes 8 steps with lanes i and i+8 sharing rank i over disjoint
// halves of the row, then one row_ror:8 add.  Rank 24 thus needs 24 weight registers (not 32) per reduced vector: with it
// the rank-24 kernels fit the 168-VGPR budget of a 10-wave workgroup (H = 256: 4 compute + 4 x-team + loader + storer).
#include "vmlmf_launch.h"

typedef __attribute__((address_space(3))) float wlds_f;
typedef __attribute__((address_space(3))) f32x4 wlds_f4;
typedef __attribute__((address_space(4))) char wkarg_c;
typedef __attribute__((address_space(4))) int wkarg_i;
typedef __attribute__((address_space(1))) unsigned wgu32;

constexpr int WF_XNB = 8;   // depth of the x ring in LDS (forward)
constexpr int WF_DL = 3;    // steps a row's DMA is issued ahead of the barrier that needs it landed (~1.5 us)
constexpr int WF_BNB = 6;   // depth of the tape ring (backward)
constexpr unsigned WF_SPIN = 1u << 22;
// The host-visible status word's address, read from the kernel-argument segment INSIDE the give-up branch (the offset goes
// through an empty asm so that the scalar load cannot be hoisted out of it): two more live scalar registers in the hot loops
// made the register allocator spill scalar registers into vector lanes next to the asm stores (wf_bwd_kernel<16,1,2,192>:
// tools/check_asm_hazards.py, hazard 2 of vmlmf_device.h - memory faults in every group-cell stack).
__device__ __forceinline__ unsigned* wf_status_karg(size_t off_in_args) {
  size_t off = ((sizeof(VGeo) + 7) & ~(size_t)7) + off_in_args;
  asm volatile("" : "+s"(off));
  const __attribute__((address_space(4))) char* ka = (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
  return *(unsigned* const __attribute__((address_space(4)))*)(ka + off);
}

template <typename S>
__device__ __forceinline__ void wf_copy_kernarg(S* dst, const wkarg_c* src) {
  static_assert(sizeof(S) % 4 == 0, "dword-sized argument structs");
  const wkarg_i* w = (const wkarg_i*)src;
  int tmp[sizeof(S) / 4];
#pragma unroll
  for (unsigned i = 0; i < sizeof(S) / 4; ++i) tmp[i] = w[i];   // scalar loads
  __builtin_memcpy(dst, tmp, sizeof(S));
}
// A layer's DropArgs (WfFwdArgs::drop / WfBwdArgs::drop) read from the kernel-argument segment WHERE IT IS USED, once per step: the
// offset goes through an empty asm so that the eight scalar loads cannot be hoisted out of the step loop - kept live across the loop
// (with the Philox key derived from them) they pushed the allocator into spilling scalar registers next to the storer's asm stores
// (wf_bwd_kernel<24,1,2,192>: tools/check_asm_hazards.py, hazard 2).  Only the `state` pointer (is there a dropout at all?) stays live.
__device__ __forceinline__ DropArgs wf_drop_karg(size_t off_in_args) {
  size_t off = ((sizeof(VGeo) + 7) & ~(size_t)7) + off_in_args;
  asm volatile("" : "+s"(off));
  const wkarg_c* ka = (const wkarg_c*)__builtin_amdgcn_kernarg_segment_ptr();
  DropArgs d;
  wf_copy_kernarg(&d, ka + off);
  return d;
}
// ... and its `period` alone, as one dword load of its own in front of the rest: read with the other seven words it made the
// struct one eight-register tuple, and wf_bwd_kernel<24,4,1,256,false> answered with 470 more v_readlane_b32 (docs/design/lm_locked.md)
__device__ __forceinline__ int wf_drop_period_karg(size_t off_in_args) {
  size_t off = ((sizeof(VGeo) + 7) & ~(size_t)7) + off_in_args + offsetof(DropArgs, period);
  asm volatile("" : "+s"(off));
  const wkarg_c* ka = (const wkarg_c*)__builtin_amdgcn_kernarg_segment_ptr();
  return *(const wkarg_i*)(ka + off);
}
__device__ __forceinline__ const void* wf_ptr_karg(size_t off_in_args) {   // one pointer of the argument block (not laundered: two registers)
  const __attribute__((address_space(4))) char* ka = (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
  return *(const void* const __attribute__((address_space(4)))*)(ka + ((sizeof(VGeo) + 7) & ~(size_t)7) + off_in_args);
}

constexpr size_t wf_align8(size_t v) { return (v + 7) & ~(size_t)7; }
constexpr size_t WF_KARG_ARGS = wf_align8(sizeof(VGeo));

// write-through stores / cache-bypassing DMA for the rows another workgroup consumes during the launch
__device__ __forceinline__ void dma4_sys(const float* gsrc, float* lds_dst) {
  __builtin_amdgcn_global_load_lds((gl_cvoid_t*)gsrc, (lds_void_t*)lds_dst, 4, 0, 17);   // aux: sc0 | sc1
}
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void wf_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---------------------------------------------------------------------------------------------------
// rank reduce of one value per lane against K rotated weights (full passes of 16 + a half pass of 8); the wave's
// partial (summed over its four 16-lane rows) goes to dst[0..KQ)
// ---------------------------------------------------------------------------------------------------
template <int K, class P>
__device__ __forceinline__ void wf_reduce1(float v, const float (&w)[K], P dst, int lane) {
  constexpr int NPF = K / 16, HALF = (K % 16) / 8;
  dpp_fence(v);
#pragma unroll
  for (int p = 0; p < NPF; ++p) {
    float a0 = 0.f, a1 = 0.f;
    fmac_ror_x16(a0, a1, v, &w[p * 16]);
    const float s = rowsum4(a0 + a1);
    if (lane < 16) dst[p * 16 + lane] = s;
  }
  if constexpr (HALF) {
    float a0 = 0.f, a1 = 0.f;
    fmac_ror_x8(a0, a1, v, &w[NPF * 16]);
    const float s = rowsum4(add_ror16<8>(a0 + a1));
    if (lane < 8) dst[NPF * 16 + lane] = s;
  }
}
// the same for the four gate derivatives against four rotated images (backward): one sum over the gates
template <int K, class P>
__device__ __forceinline__ void wf_reduce4(float (&dp)[4], const float (&w)[4][K], P dst, int lane) {
  constexpr int NPF = K / 16, HALF = (K % 16) / 8;
  asm volatile("s_nop 1" : "+v"(dp[0]), "+v"(dp[1]), "+v"(dp[2]), "+v"(dp[3]));   // one DPP fence for the four
#pragma unroll
  for (int p = 0; p < NPF; ++p) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    fmac_ror_4x4<0>(acc, dp, &w[0][p * 16], &w[1][p * 16], &w[2][p * 16], &w[3][p * 16]);
    fmac_ror_4x4<4>(acc, dp, &w[0][p * 16], &w[1][p * 16], &w[2][p * 16], &w[3][p * 16]);
    fmac_ror_4x4<8>(acc, dp, &w[0][p * 16], &w[1][p * 16], &w[2][p * 16], &w[3][p * 16]);
    fmac_ror_4x4<12>(acc, dp, &w[0][p * 16], &w[1][p * 16], &w[2][p * 16], &w[3][p * 16]);
    const float s = rowsum4((acc[0] + acc[1]) + (acc[2] + acc[3]));
    if (lane < 16) dst[p * 16 + lane] = s;
  }
  if constexpr (HALF) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    fmac_ror_4x4<0>(acc, dp, &w[0][NPF * 16], &w[1][NPF * 16], &w[2][NPF * 16], &w[3][NPF * 16]);
    fmac_ror_4x4<4>(acc, dp, &w[0][NPF * 16], &w[1][NPF * 16], &w[2][NPF * 16], &w[3][NPF * 16]);
    const float s = rowsum4(add_ror16<8>((acc[0] + acc[1]) + (acc[2] + acc[3])));
    if (lane < 8) dst[NPF * 16 + lane] = s;
  }
}

// Cooperative cross-wave sum of the CNT waves' partials (see rec_fwd_kernel: FASTQ16 / FASTQ64): lane -> (wave, 4-rank
// chunk), one ds_read_b128, a DPP butterfly; afterwards lane cc (< NC) holds chunk cc's four totals in (sx, sy, sz, sw).
template <int K, int CNT>
struct WfQ {
  static constexpr int KQ = (K + 15) / 16 * 16, NC = K / 4, NCP = NC <= 2 ? 2 : (NC <= 4 ? 4 : 8);
  static constexpr bool F16 = NC == NCP && NC * CNT <= 16;
  static_assert(F16 || NCP * CNT <= 64, "partials do not fit the cooperative sum");
  static __device__ __forceinline__ int rdoff(int lane) {
    const int li = F16 ? (lane & 15) : lane, cc = li % NCP, w = li / NCP;
    return (w < CNT && cc < NC) ? (w * KQ + 4 * cc) : -1;
  }
  // two groups (V2, V6): the units of group grp take rank block 0 (ranks < off1) from the waves of their own group and
  // block 1 from the other group's - forward (source (grp + s) mod 2) and backward (destination (grp - s) mod 2) alike
  static __device__ __forceinline__ int rdoff_g(int lane, int grp, int off1, int G) {
    const int li = F16 ? (lane & 15) : lane, cc = li % NCP, w = li / NCP;
    const int s = (G == 2 && 4 * (cc < NC ? cc : 0) >= off1) ? 1 : 0;
    return (w < CNT && cc < NC) ? ((((grp + s) % G) * CNT + w) * KQ + 4 * cc) : -1;
  }
  static __device__ __forceinline__ void finish(f32x4 v, float& sx, float& sy, float& sz, float& sw) {
    sx = class_sum16<NCP>(v[0]), sy = class_sum16<NCP>(v[1]), sz = class_sum16<NCP>(v[2]), sw = class_sum16<NCP>(v[3]);
    if constexpr (!F16) sx = rowsum4(sx), sy = rowsum4(sy), sz = rowsum4(sz), sw = rowsum4(sw);
  }
};

// thread slot -> hidden unit (vmlmf_geo.h): the G groups are wave-aligned, W waves each, Hg units per group
__device__ __forceinline__ bool wf_unit(int slot, int Hg, int W, int& n) {
  const int grp = slot / (64 * W), m = slot - grp * 64 * W;
  n = grp * Hg + (m < Hg ? m : 0);
  return m < Hg;
}

// block id -> (layer position, batch row): groups of 8 rows x L layers, the L workgroups of a row 8 ids apart
__device__ __forceinline__ void wf_decode(int bid, int L, int& pos, int& row) {
  const int grp = bid / (8 * L), within = bid - grp * 8 * L;
  pos = within >> 3;
  row = grp * 8 + (within & 7);
}

// =====================================================================================================
// forward
// =====================================================================================================
// x-team wave xw (0 .. CNT-1): slot = xw * 64 + lane is BOTH the input it feeds into the rank reduce and the hidden unit
// whose four x-side pre-activations it expands.  Fed from the kernel-argument segment; inlined: as a real call (the form
// xwave_role needs) its prologue saved 52 callee-saved VGPRs per lane to scratch, 13.6 MB per launch at config C (rocprofv3
// WRITE_SIZE: 50.7 MB against the tape's 37), and neither role's loop spills an SGPR inlined.
// Barrier schedule of the workgroup: P0, P1, b(0) .. b(T).  x-step s is reduced in the segment before b(s-1) and expanded
// in the segment before b(s); the compute waves read it after b(s).
template <int K, int CNT>   // CNT: ALL waves of units (the x side is not grouped: its partials are summed over every wave)
__device__ __forceinline__ void wf_xteam_fwd(const wkarg_c* ka, int pos, int xw, wlds_f* partx, wlds_f* xring,
                                                       wlds_f* gxs, wlds_f* qxs, wlds_f* zero4) {
  typedef WfQ<K, CNT> Q;
  constexpr int KQ = Q::KQ, NC = Q::NC, NT = CNT * 64;
  const int T = ((const wkarg_i*)(ka + offsetof(VGeo, T)))[0], Wg = ((const wkarg_i*)(ka + offsetof(VGeo, W)))[0];
  WfFwdLayer a;
  wf_copy_kernarg(&a, ka + WF_KARG_ARGS + offsetof(WfFwdArgs, l) + (size_t)pos * sizeof(WfFwdLayer));
  const int H = a.H, Hg = a.Hg;   // (this layer's: the layers of a stack share ranks and wave count, not the hidden size)
  const int lane = threadIdx.x & 63, slot = xw * 64 + lane;
  int n;
  const bool valid = wf_unit(slot, Hg, Wg, n);
  float urx[K];
  f32x2 vx01[K], vx23[K], ex01, ex23, b01, b23;
#pragma unroll
  for (int j = 0; j < K; ++j) urx[j] = a.URX[(size_t)j * NT + slot];
#pragma unroll
  for (int r = 0; r < K; ++r) {   // unconditional loads (clamped unit), masked values
    const float v0 = a.VXT[(size_t)(0 * K + r) * H + n], v1 = a.VXT[(size_t)(1 * K + r) * H + n];
    const float v2 = a.VXT[(size_t)(2 * K + r) * H + n], v3 = a.VXT[(size_t)(3 * K + r) * H + n];
    vx01[r] = valid ? f32x2{v0, v1} : f32x2{0.f, 0.f};
    vx23[r] = valid ? f32x2{v2, v3} : f32x2{0.f, 0.f};
  }
  {
    const float e0 = a.EXT[0 * H + n], e1 = a.EXT[1 * H + n], e2 = a.EXT[2 * H + n], e3 = a.EXT[3 * H + n];
    const float c0 = a.BBT[0 * H + n], c1 = a.BBT[1 * H + n], c2 = a.BBT[2 * H + n], c3 = a.BBT[3 * H + n];
    ex01 = valid ? f32x2{e0, e1} : f32x2{0.f, 0.f}, ex23 = valid ? f32x2{e2, e3} : f32x2{0.f, 0.f};
    b01 = valid ? f32x2{c0, c1} : f32x2{0.f, 0.f}, b23 = valid ? f32x2{c2, c3} : f32x2{0.f, 0.f};
  }
  const int rdoff = Q::rdoff(lane);
  auto reduce = [&](int s) -> float {
    const float xv = xring[(s % WF_XNB) * NT + slot];
    wf_reduce1<K>(xv, urx, partx + ((s & 1) * CNT + xw) * KQ, lane);
    return xv;
  };
  auto expand = [&](int s, float xv) {
    const wlds_f* src = partx + (s & 1) * CNT * KQ;
    const f32x4 v = *(const wlds_f4*)(rdoff >= 0 ? src + rdoff : zero4);
    float sx, sy, sz, sw;
    Q::finish(v, sx, sy, sz, sw);
    if (xw == 0 && lane < NC) *(wlds_f4*)(qxs + (s & 1) * 32 + 4 * lane) = f32x4{sx, sy, sz, sw};   // qx[s] for the storer
    f32x2 p01a = pk_fma(splat2(xv), ex01, b01), p01b = f32x2{0.f, 0.f};
    f32x2 p23a = pk_fma(splat2(xv), ex23, b23), p23b = f32x2{0.f, 0.f};
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) {
      const float qx_ = bcast_lane(sx, cc), qy = bcast_lane(sy, cc), qz = bcast_lane(sz, cc), qw = bcast_lane(sw, cc);
      p01a = pk_fma(splat2(qx_), vx01[4 * cc + 0], p01a);
      p23a = pk_fma(splat2(qx_), vx23[4 * cc + 0], p23a);
      p01b = pk_fma(splat2(qy), vx01[4 * cc + 1], p01b);
      p23b = pk_fma(splat2(qy), vx23[4 * cc + 1], p23b);
      p01a = pk_fma(splat2(qz), vx01[4 * cc + 2], p01a);
      p23a = pk_fma(splat2(qz), vx23[4 * cc + 2], p23a);
      p01b = pk_fma(splat2(qw), vx01[4 * cc + 3], p01b);
      p23b = pk_fma(splat2(qw), vx23[4 * cc + 3], p23b);
    }
    const f32x2 p01 = p01a + p01b, p23 = p23a + p23b;
    *(wlds_f4*)(gxs + ((s & 1) * NT + slot) * 4) = f32x4{p01.x, p01.y, p23.x, p23.y};
  };
  wf_barrier();                 // P0: x[0] has landed
  float xv = reduce(0);
  wf_barrier();                 // P1
  expand(0, xv);
  xv = reduce(1);
  wf_barrier();                 // b(0)
  for (int j = 0; j < T; ++j) {
    expand(j + 1, xv);          // (steps past the end work on the clamped last row: finite, never consumed)
    xv = reduce(j + 2);
    wf_barrier();               // b(j + 1)
  }
}

// BT: the gate tape as bf16 (four gates of a unit and step in 8 bytes: VGeo::bt; the arithmetic stays fp32)
template <int K, int W, int G, int MAXT, bool BT = false>   // W waves of units per group, G groups
__global__ void __launch_bounds__(2 * MAXT + 128) wf_fwd_kernel(VGeo g, WfFwdArgs args) {
  typedef WfQ<K, W> Q;
  constexpr int KQ = Q::KQ, NC = Q::NC, NW = G * W, NT = NW * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int B = g.B, T = g.T, L = args.c.L;
  int pos, row;
  wf_decode((int)blockIdx.x, L, pos, row);
  if (row >= B) return;
  const wkarg_c* ka = (const wkarg_c*)__builtin_amdgcn_kernarg_segment_ptr();

  extern __shared__ float4 smem4[];
  float* part = reinterpret_cast<float*>(smem4);   // [2][NW][KQ]   h-side partials
  float* partx = part + 2 * NW * KQ;                // [2][NW][KQ]   x-side partials
  float* gxs = partx + 2 * NW * KQ;                 // [2][NT][4]    x-side pre-activations of a step
  float* xring = gxs + 2 * NT * 4;                  // [WF_XNB][NT]  input rows (by slot)
  float* outs = xring + WF_XNB * NT;                // [2][ NT x (i f o n) | NT x (c h) | NT x 2 spare ]
  float* qxs = outs + 2 * NT * 8;                   // [2][32]       qx of a step for the storer
  float* zero4 = qxs + 64;                          // 4 zero floats
  float* fring = zero4 + 4;                         // [2][NT]       dropout factors of a step's output row (loader -> storer)
  if (tid < 4) zero4[tid] = 0.f;

  if (wave >= NW && wave < 2 * NW) {   // -------------------------------------------------- x-team
    wf_xteam_fwd<K, NW>(ka, pos, wave - NW, (wlds_f*)partx, (wlds_f*)xring, (wlds_f*)gxs, (wlds_f*)qxs, (wlds_f*)zero4);
    return;
  }
  WfFwdLayer a;
  wf_copy_kernarg(&a, ka + WF_KARG_ARGS + offsetof(WfFwdArgs, l) + (size_t)pos * sizeof(WfFwdLayer));
  const bool train = a.gates != nullptr;
  const bool pub = pos + 1 < L;          // a layer above consumes y during the launch
  const size_t sstride = (size_t)g.Bp * NT;
  const int H = a.H, Hg = a.Hg;          // this layer's hidden size (round 6: layers of a stack may differ in it)

  if (wave == 2 * NW) {   // ------------------------------------------------------------- loader
    // x rows -> LDS ring by DMA, WF_DL steps ahead of the barrier that needs them; above the first layer a row is only
    // fetched once the layer below has published it
    const bool poll = pos > 0;
    wgu32* fl = (wgu32*)(args.c.flag + ((size_t)(poll ? pos - 1 : 0) * B + row) * WF_FLAG_STRIDE);
    wgu32* err = (wgu32*)(args.c.flag + (size_t)(L - 1) * B * WF_FLAG_STRIDE);
    unsigned prog = poll ? 0u : 0xffffffffu;
    bool dead = false;
    const int I = a.I;
    auto issue = [&](int s) {
      const int sc = s < T ? s : T - 1;
      if (prog < (unsigned)(sc + 1)) {
        unsigned spins = 0;
        while (true) {
          prog = __builtin_amdgcn_readfirstlane(__hip_atomic_load(fl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
          if (prog >= (unsigned)(sc + 1)) break;
          __builtin_amdgcn_s_sleep(1);
          if (++spins > WF_SPIN) {   // bounded: a producer that never arrives must not hang the GPU ...
            if (lane == 0) {
              __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
              vg_raise(wf_status_karg(offsetof(WfFwdArgs, c) + offsetof(WfCommon, status)), VMLMF_ST_WF_FWD);
            }
            prog = 0xffffffffu;
            dead = true;             // ... and must not pass for a result: the ring is filled with NaN and no row is fetched any more,
            for (int i = lane; i < WF_XNB * NT; i += 64) xring[i] = __builtin_nanf("");   // so this layer's outputs are NaN from here on
            break;
          }
        }
      }
      if (dead) return;
      float* dst = xring + (s % WF_XNB) * NT;
      const float* src = a.x + ((size_t)sc * a.sxT + (size_t)row * a.sxB);
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        int nu;
        const bool uok = wf_unit(lane + 64 * i, Hg, W, nu);
        const float* p = src + ((uok && nu < I) ? nu : 0);   // lanes without an input re-read element 0 (finite; zero weights)
        if (poll) dma4_sys(p, dst + 64 * i);
        else dma4(p, dst + 64 * i);
      }
    };
    // dropout of this layer's output (round 6): the factors of time step j - one Philox call, lane l the columns 4 l .. 4 l + 3 -
    // go into fring[j & 1] in the segment that ends with b(j + 1) (the one in which the compute waves form h_j); the storer drains
    // step j between b(j + 1) and b(j + 2), reading fring[j & 1], while this wave fills the other half
    // (one-group stacks only - the LM's layers: the two-group instantiations have no scalar register to spare, see wf_drop_karg)
    const size_t droff = offsetof(WfFwdArgs, drop) + (size_t)pos * sizeof(DropArgs);
    bool dropping = false;
    if constexpr (G == 1) dropping = wf_ptr_karg(droff + offsetof(DropArgs, state)) != nullptr;
    auto factors = [&](int j) {
      if (dropping && j >= 0 && j < T && 4 * lane < NT) {
        const unsigned position = drop_position(drop_tstride(wf_drop_period_karg(droff), B), j, row);
        const DropArgs dr = wf_drop_karg(droff);
        const DropKey dkey = drop_key(dr);
        float f[4];
        drop_factors(dkey, dr.thresh, dr.scale, position, (unsigned)lane, f);
        st4(fring + (size_t)(j & 1) * NT + 4 * lane, make_float4(f[0], f[1], f[2], f[3]));
      }
    };
    for (int s = 0; s <= WF_DL; ++s) issue(s);
    wait_vm_barrier<WF_DL * NW>();                     // P0: x[0] has landed
    for (int j = -2; j < T; ++j) {
      issue(j + 3 + WF_DL);
      factors(j);                                      // (published by this iteration's barrier, b(j + 1))
      wait_vm_barrier<WF_DL * NW>();                   // P1, b(0), b(j + 1): x[j + 3] has landed
    }
    return;
  }

  if (wave == 2 * NW + 1) {   // --------------------------------------------------------- storer
    bool sv[NW];
    unsigned so_[NW], yo_[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int slot = lane + 64 * i;
      int nu;
      sv[i] = wf_unit(slot, Hg, W, nu);
      so_[i] = (unsigned)(row * NT + slot) * 4u;                          // bytes into a [Bp][NT] float slice
      yo_[i] = (unsigned)(row * a.syB + nu) * 4u;                         // bytes into y[t]
    }
    // the tapes keep their own widths (Q: KH, qx: KX; K is the wider of the two)
    // Q[ts][j][rr] = sum over the W waves of source group (j + s) mod G (s: rank block of rr); one element per lane
    const int KH = g.KH, KX = g.KX;
    const bool qv = lane < G * KH, qxv_ok = lane < KX;
    const int qe = qv ? lane : 0, qj = qe / KH, qrr = qe - qj * KH;
    const int qw0 = ((qj + ((G == 2 && qrr >= g.off1) ? 1 : 0)) % G) * W;
    const unsigned qoff = 4u * (unsigned)(row * G * KH + qe), qxoff = 4u * (unsigned)(row * KX + (qxv_ok ? lane : 0));
    wgu32* fl = (wgu32*)(args.c.flag + ((size_t)(pub ? pos : 0) * B + row) * WF_FLAG_STRIDE);
    // the dropped copy of y beside y (a layer above reads THAT copy); only its address stays live here
    float* ydrop = nullptr;
    if constexpr (G == 1) ydrop = (float*)wf_ptr_karg(offsetof(WfFwdArgs, drop) + (size_t)pos * sizeof(DropArgs) + offsetof(DropArgs, yd));
    const bool dropping = ydrop != nullptr;
    auto segment = [&](int td, int tq) {   // every LDS read before the first global store (see rec_fwd_kernel's storer)
      const int tdc = td < 0 ? 0 : td, tqc = tq < 0 ? 0 : tq;
      const float* src = outs + (size_t)(tdc & 1) * NT * 8;
      const float* qsrc = part + (size_t)(tqc & 1) * NW * KQ;
      float4 g4[NW];
      float2 ch[NW];
      float v[W], fac[NW];
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        g4[i] = ld4(src + (size_t)(lane + 64 * i) * 4);
        ch[i] = *reinterpret_cast<const float2*>(src + (size_t)NT * 4 + (size_t)(lane + 64 * i) * 2);
        fac[i] = dropping ? fring[(size_t)(tdc & 1) * NT + lane + 64 * i] : 1.f;
      }
#pragma unroll
      for (int w = 0; w < W; ++w) v[w] = qsrc[(qw0 + w) * KQ + qrr];
      const float qxv = qxs[(tqc & 1) * 32 + (lane & 31)];
      if (td >= 0) {
        char* gt = reinterpret_cast<char*>(a.gates + (size_t)td * sstride * (BT ? 2 : 4));   // wave-uniform bases
        char* ct = reinterpret_cast<char*>(a.cs + (size_t)(td + 1) * sstride);
        char* yt = reinterpret_cast<char*>(a.y + (size_t)td * a.syT);
#pragma unroll
        for (int i = 0; i < NW; ++i) {
          if (train) {
            if constexpr (BT) {   // (i, f | o, n) rounded to bf16: two dwords at half the fp32 tape's slot offset
              // (v_cvt_pk_bf16_f32: round to nearest even, two values per instruction)
              typedef __bf16 bf2_t __attribute__((ext_vector_type(2)));
              const bf2_t p0 = __builtin_convertvector(f32x2{g4[i].x, g4[i].y}, bf2_t), p1 = __builtin_convertvector(f32x2{g4[i].z, g4[i].w}, bf2_t);
              float2 pk;
              __builtin_memcpy(&pk.x, &p0, 4);
              __builtin_memcpy(&pk.y, &p1, 4);
              st2_sv_nt(gt, 2u * so_[i], pk);
            } else {
              st4_sv<false, true>(gt, 4u * so_[i], g4[i]);   // (tape: non-temporal, see st4_sv)
            }
            st1_sv<false, true>(ct, so_[i], ch[i].x);
          }
          if (pub && !dropping) {
            if (sv[i]) st1_sv_sys(yt, yo_[i], ch[i].y);
          } else {
            if (sv[i]) st1_sv(yt, yo_[i], ch[i].y);
          }
          if (dropping) {
            char* ydt = reinterpret_cast<char*>(ydrop + (size_t)td * a.syT);
            if (pub) {
              if (sv[i]) st1_sv_sys(ydt, yo_[i], ch[i].y * fac[i]);
            } else {
              if (sv[i]) st1_sv(ydt, yo_[i], ch[i].y * fac[i]);
            }
          }
        }
      }
      if (tq >= 0 && train) {
        float acc = 0.f;
#pragma unroll
        for (int w = 0; w < W; ++w) acc += v[w];   // same order as the compute waves' sum
        if (qv) st1_sv(a.Qs + (size_t)tq * B * G * KH, qoff, acc);
        if (qxv_ok) st1_sv(a.qx + (size_t)tq * B * KX, qxoff, qxv);
      }
    };
    // vector-memory operations of one full segment: the counted wait below leaves exactly those in flight, i.e. every
    // store of the segment before has completed (stores complete in order) and the row it wrote may be published
    constexpr int NSEG_TRAIN = 3 * NW + 2, NSEG_INFER = NW;
    wf_barrier();   // P0
    wf_barrier();   // P1
    wf_barrier();   // b(0)
    for (int t = 0; t < T; ++t) {   // segment t
      segment(t - 1, t);
      if (pub && t >= 2) {
        if (dropping) {   // (a segment has NW more stores: the dropped copy)
          if (train) wait_vm<NSEG_TRAIN + NW>();
          else wait_vm<NSEG_INFER + NW>();
        } else if (train) wait_vm<NSEG_TRAIN>();
        else wait_vm<NSEG_INFER>();
        if (lane == 0) __hip_atomic_store(fl, (unsigned)(t - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // rows 0 .. t-2
      }
      wf_barrier();   // b(t + 1)
    }
    segment(T - 1, -1);
    if (pub) {
      wait_vm<0>();
      if (lane == 0) __hip_atomic_store(fl, (unsigned)T, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    return;
  }

  // ------------------------------------------------------------------------------------- compute waves
  int n;
  const bool valid = wf_unit(tid, Hg, W, n);
  const int grp = tid / (64 * W);
  f32x2 ve01[K], ve23[K], eh01, eh23;
  float ur[K];
#pragma unroll
  for (int rr = 0; rr < K; ++rr) {
    ve01[rr] = f32x2{a.VE[(size_t)(0 * K + rr) * NT + tid], a.VE[(size_t)(1 * K + rr) * NT + tid]};
    ve23[rr] = f32x2{a.VE[(size_t)(2 * K + rr) * NT + tid], a.VE[(size_t)(3 * K + rr) * NT + tid]};
  }
  eh01 = f32x2{a.EH[0 * NT + tid], a.EH[1 * NT + tid]};
  eh23 = f32x2{a.EH[2 * NT + tid], a.EH[3 * NT + tid]};
#pragma unroll
  for (int j = 0; j < K; ++j) ur[j] = a.UR[(size_t)j * NT + tid];
  const int rdoff = Q::rdoff_g(lane, grp, g.off1, G);
  float h = (valid && a.h0 != nullptr) ? a.h0[(size_t)row * H + n] : 0.f;
  float c = (valid && a.c0 != nullptr) ? a.c0[(size_t)row * H + n] : 0.f;
  if (train) a.cs[(size_t)row * NT + tid] = c;   // tape slice 0 = c_{-1}
  wf_barrier();   // P0
  wf_barrier();   // P1
  for (int t = 0; t < T; ++t) {
    const int buf = t & 1;
    wf_reduce1<K>(h, ur, part + (buf * NW + wave) * KQ, lane);
    wf_barrier();   // b(t): partials of step t, the x-side of step t and the previous out-stage are published
    const float4 gx4 = ld4(gxs + ((size_t)buf * NT + tid) * 4);
    const float* src = part + (size_t)buf * NW * KQ;
    const float4 v = ld4(rdoff >= 0 ? src + rdoff : zero4);
    float sx, sy, sz, sw;
    Q::finish(f32x4{v.x, v.y, v.z, v.w}, sx, sy, sz, sw);
    const f32x2 hh = splat2(h);
    f32x2 p01a = pk_fma(hh, eh01, f32x2{gx4.x, gx4.y}), p01b = f32x2{0.f, 0.f};
    f32x2 p23a = pk_fma(hh, eh23, f32x2{gx4.z, gx4.w}), p23b = f32x2{0.f, 0.f};
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) {
      const float qx_ = bcast_lane(sx, cc), qy = bcast_lane(sy, cc), qz = bcast_lane(sz, cc), qw = bcast_lane(sw, cc);
      p01a = pk_fma(splat2(qx_), ve01[4 * cc + 0], p01a);
      p23a = pk_fma(splat2(qx_), ve23[4 * cc + 0], p23a);
      p01b = pk_fma(splat2(qy), ve01[4 * cc + 1], p01b);
      p23b = pk_fma(splat2(qy), ve23[4 * cc + 1], p23b);
      p01a = pk_fma(splat2(qz), ve01[4 * cc + 2], p01a);
      p23a = pk_fma(splat2(qz), ve23[4 * cc + 2], p23a);
      p01b = pk_fma(splat2(qw), ve01[4 * cc + 3], p01b);
      p23b = pk_fma(splat2(qw), ve23[4 * cc + 3], p23b);
    }
    const f32x2 pre01 = p01a + p01b, pre23 = p23a + p23b;
    const CellFwd cell = cell_fwd(pre01.x, pre01.y, pre23.x, pre23.y, c);
    c = cell.c, h = cell.h;
    float* ot = outs + (size_t)buf * NT * 8;
    st4(ot + (size_t)tid * 4, cell.gates);
    *reinterpret_cast<float2*>(ot + (size_t)NT * 4 + (size_t)tid * 2) = make_float2(c, h);
  }
  wf_barrier();   // b(T): last out-stage published
  if (valid) {
    if (a.hT != nullptr) a.hT[(size_t)row * H + n] = h;
    if (a.cT != nullptr) a.cT[(size_t)row * H + n] = c;
  }
  // classifier on the top layer's final hidden state (HeadFwd; see head_epilogue of rec_fwd_kernel): wave w owns classes
  // w, w + NW, ..., lanes stride the units of the final out-stage, every class is a 64-lane sum in a fixed order
  if (pos == L - 1 && args.hd.C > 0) {
    const HeadFwd hd = args.hd;
    const float* chp = outs + (size_t)((T - 1) & 1) * NT * 8 + (size_t)NT * 4;   // (c, h) pairs
    constexpr int CP = 8;
    for (int c0 = wave; c0 < hd.C; c0 += CP * NW) {
      float acc[CP];
#pragma unroll
      for (int j = 0; j < CP; ++j) acc[j] = 0.f;
      for (int slot = lane; slot < NT; slot += 64) {
        int nc;
        const bool uv = wf_unit(slot, Hg, W, nc);
        const float hv = uv ? chp[slot * 2 + 1] : 0.f;
        float w[CP];
#pragma unroll
        for (int j = 0; j < CP; ++j) w[j] = hd.W[(size_t)(c0 + j * NW < hd.C ? c0 + j * NW : 0) * H + nc];   // clamped: unconditional loads
#pragma unroll
        for (int j = 0; j < CP; ++j) acc[j] = fmaf(hv, c0 + j * NW < hd.C ? w[j] : 0.f, acc[j]);
      }
#pragma unroll
      for (int j = 0; j < CP; ++j) {
        float t = add_ror16<8>(acc[j]);
        t = add_ror16<4>(t);
        t = add_ror16<2>(t);
        t = add_ror16<1>(t);
        t = rowsum4(t);
        const int cls = c0 + j * NW;
        if (lane == 0 && cls < hd.C) hd.logits[(size_t)row * hd.C + cls] = t + (hd.bias != nullptr ? hd.bias[cls] : 0.f);
      }
    }
  }
}

template <int K, int W, int G>
static int wf_fwd_launch(const VGeo& g, const WfFwdArgs& a, hipStream_t s) {
  constexpr int KQ = (K + 15) / 16 * 16, NW = G * W, NT = NW * 64, MAXT = NW <= 3 ? 192 : 256;
  const size_t lds = sizeof(float) * ((size_t)4 * NW * KQ + (size_t)2 * NT * 4 + (size_t)WF_XNB * NT + (size_t)2 * NT * 8 + 64 + 4 + (size_t)2 * NT);
  const int groups = (g.B + 7) / 8;
  if constexpr (G == 1 && (K == 16 || K == 24)) {   // (the bf16 tape: instantiated for the one-group stacks of ranks 16 / 24)
    if (g.bt) {
      hipLaunchKernelGGL((wf_fwd_kernel<K, W, G, MAXT, true>), dim3(groups * 8 * a.c.L), dim3(2 * NT + 128), lds, s, g, a);
      return (int)hipGetLastError();
    }
  }
  if (g.bt) return -3;
  hipLaunchKernelGGL((wf_fwd_kernel<K, W, G, MAXT>), dim3(groups * 8 * a.c.L), dim3(2 * NT + 128), lds, s, g, a);
  return (int)hipGetLastError();
}

template <int K>
static int wf_fwd_dispatch(const VGeo& g, const WfFwdArgs& a, hipStream_t s) {
  if (g.G == 2) {   // two groups: W waves each
    if (g.W == 1) return wf_fwd_launch<K, 1, 2>(g, a, s);
    if constexpr (K <= 24) {
      if (g.W == 2) return wf_fwd_launch<K, 2, 2>(g, a, s);
    }
    return -3;
  }
  switch (g.NW) {
    case 1: return wf_fwd_launch<K, 1, 1>(g, a, s);
    case 2: return wf_fwd_launch<K, 2, 1>(g, a, s);
    case 3: return wf_fwd_launch<K, 3, 1>(g, a, s);
    case 4:
      if constexpr (K <= 24) return wf_fwd_launch<K, 4, 1>(g, a, s);
      break;
  }
  return -3;
}

// =====================================================================================================
// backward
// =====================================================================================================
// Launch position p = 0 is the TOP layer (it has no producer), p + 1 the layer below it.  Barrier schedule of a
// workgroup: O, b(T-1) .. b(0), E1, E2.  The compute waves leave dpre[t] in the LDS out-stage before b(t); the x-team
// reduces it against V_x in the segment after b(t) (phase A) and turns the summed dqx[t] into dx[t] in the segment after
// b(t-1) (phase B); the storer drains dx[t] in the segment after b(t-2) and publishes it one segment later.
template <int K, int CNT>   // CNT: ALL waves of units (see wf_xteam_fwd)
__device__ __forceinline__ void wf_xteam_bwd(const wkarg_c* ka, int pos, int xw, wlds_f* partx, wlds_f* outs,
                                                       wlds_f* dxs, wlds_f* dqs, wlds_f* zero4) {
  typedef WfQ<K, CNT> Q;
  constexpr int KQ = Q::KQ, NC = Q::NC, NT = CNT * 64;
  const int T = ((const wkarg_i*)(ka + offsetof(VGeo, T)))[0];
  WfBwdLayer a;
  wf_copy_kernarg(&a, ka + WF_KARG_ARGS + offsetof(WfBwdArgs, l) + (size_t)pos * sizeof(WfBwdLayer));
  const int lane = threadIdx.x & 63, slot = xw * 64 + lane;
  float vrx[4][K], uxo[K], exi[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int j = 0; j < K; ++j) vrx[k][j] = a.VRX[(size_t)(k * K + j) * NT + slot];
    exi[k] = a.EXI[k * NT + slot];
  }
#pragma unroll
  for (int r = 0; r < K; ++r) uxo[r] = a.UXO[(size_t)r * NT + slot];
  const int rdoff = Q::rdoff(lane);
  f32x4 d = f32x4{0.f, 0.f, 0.f, 0.f};
  auto phaseA = [&](int t) {
    d = *(const wlds_f4*)(outs + ((t & 1) * NT + slot) * 4);
    float dp[4] = {d[0], d[1], d[2], d[3]};
    wf_reduce4<K>(dp, vrx, partx + ((t & 1) * CNT + xw) * KQ, lane);
  };
  auto phaseB = [&](int t) {   // uses the d of phaseA(t)
    const wlds_f* src = partx + (t & 1) * CNT * KQ;
    const f32x4 v = *(const wlds_f4*)(rdoff >= 0 ? src + rdoff : zero4);
    float sx, sy, sz, sw;
    Q::finish(v, sx, sy, sz, sw);
    if (xw == 0 && lane < NC) *(wlds_f4*)(dqs + (t & 1) * 32 + 4 * lane) = f32x4{sx, sy, sz, sw};   // dqx[t] for the storer
    float x0 = (d[0] * exi[0] + d[1] * exi[1]), x1 = (d[2] * exi[2] + d[3] * exi[3]);
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) {
      x0 = fmaf(bcast_lane(sx, cc), uxo[4 * cc + 0], x0);
      x1 = fmaf(bcast_lane(sy, cc), uxo[4 * cc + 1], x1);
      x0 = fmaf(bcast_lane(sz, cc), uxo[4 * cc + 2], x0);
      x1 = fmaf(bcast_lane(sw, cc), uxo[4 * cc + 3], x1);
    }
    dxs[(t & 1) * NT + slot] = x0 + x1;
  };
  wf_barrier();                 // O
  for (int t = T - 1; t >= 0; --t) {
    wf_barrier();               // b(t)
    if (t + 1 < T) phaseB(t + 1);
    phaseA(t);
  }
  wf_barrier();                 // E1
  phaseB(0);
  wf_barrier();                 // E2
}

template <int K, int W, int G, int MAXT, bool BT = false>
__global__ void __launch_bounds__(2 * MAXT + 128) wf_bwd_kernel(VGeo g, WfBwdArgs args) {
  typedef WfQ<K, W> Q;
  constexpr int KQ = Q::KQ, NC = Q::NC, NW = G * W, NT = NW * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int B = g.B, T = g.T, L = args.c.L;
  int pos, row;
  wf_decode((int)blockIdx.x, L, pos, row);
  if (row >= B) return;
  const wkarg_c* ka = (const wkarg_c*)__builtin_amdgcn_kernarg_segment_ptr();

  extern __shared__ float4 smem4[];
  float* part = reinterpret_cast<float*>(smem4);   // [2][NW][KQ]      dQ partials
  float* partx = part + 2 * NW * KQ;                // [2][NW][KQ]      dqx partials
  float* tg = partx + 2 * NW * KQ;                  // [WF_BNB][NT][4]  gates of the step
  float* tcp = tg + WF_BNB * NT * 4;                // [WF_BNB][NT]     c_{t-1}
  float* tdy = tcp + WF_BNB * NT;                   // [WF_BNB][NT]     dy_t
  float* outs = tdy + WF_BNB * NT;                  // [2][NT][4]       dpre
  float* dxs = outs + 2 * NT * 4;                   // [2][NT]          dx of a step for the storer
  float* dqs = dxs + 2 * NT;                        // [2][32]          dqx of a step for the storer
  float* zero4 = dqs + 64;                          // 4 zero floats
  float* tfac = zero4 + 4;                          // [WF_BNB][NT]     dropout factors of dy_t (loader; 1 everywhere without dropout)
  if (tid < 4) zero4[tid] = 0.f;

  if (wave >= NW && wave < 2 * NW) {   // -------------------------------------------------- x-team
    wf_xteam_bwd<K, NW>(ka, pos, wave - NW, (wlds_f*)partx, (wlds_f*)outs, (wlds_f*)dxs, (wlds_f*)dqs, (wlds_f*)zero4);
    return;
  }
  WfBwdLayer a;
  wf_copy_kernarg(&a, ka + WF_KARG_ARGS + offsetof(WfBwdArgs, l) + (size_t)pos * sizeof(WfBwdLayer));
  const bool has_dy = a.dy != nullptr;
  const bool pub = pos + 1 < L;   // the layer below consumes dx during the launch
  const int H = a.H, Hg = a.Hg;   // this layer's hidden size
  const size_t sstride = (size_t)g.Bp * NT;

  if (wave == 2 * NW) {   // ------------------------------------------------------------- loader
    // (bf16 tape, an even number of waves: ONE 16-byte DMA covers two slots - lane l the slots 2 l, 2 l + 1 of a block of 128)
    constexpr bool PAIR = BT && NW % 2 == 0;
    constexpr int NDMA = PAIR ? 2 * NW + NW / 2 : (BT ? 4 : 3) * NW;
    constexpr int DEPTH = (2 * NDMA <= 63) ? 2 : 1;
    constexpr int DIST = DEPTH + 2;
    static_assert(DIST < WF_BNB, "tape ring too shallow");
    const bool poll = pos > 0;
    wgu32* fl = (wgu32*)(args.c.flag + ((size_t)(poll ? pos - 1 : 0) * B + row) * WF_FLAG_STRIDE);
    wgu32* err = (wgu32*)(args.c.flag + (size_t)(L - 1) * B * WF_FLAG_STRIDE);
    unsigned prog = poll ? 0u : 0xffffffffu;
    bool dead = false;
    // dy is the gradient of the DROPPED copy of this layer's output (round 6): the forward's factors again, beside the tape
    const size_t droff = offsetof(WfBwdArgs, drop) + (size_t)pos * sizeof(DropArgs);
    bool dropping = false;   // (one-group stacks only, as in the forward)
    if constexpr (G == 1) dropping = wf_ptr_karg(droff + offsetof(DropArgs, state)) != nullptr && has_dy;
    auto issue = [&](int ttarget) {   // tape of step ttarget (clamped at 0) -> ring slot
      const int tc = ttarget > 0 ? ttarget : 0;
      const int ring = ((ttarget % WF_BNB) + WF_BNB) % WF_BNB;
      if (dropping && 4 * lane < NT) {
        const unsigned position = drop_position(drop_tstride(wf_drop_period_karg(droff), B), tc, row);
        const DropArgs dr = wf_drop_karg(droff);
        const DropKey dkey = drop_key(dr);
        float f[4];
        drop_factors(dkey, dr.thresh, dr.scale, position, (unsigned)lane, f);
        st4(tfac + (size_t)ring * NT + 4 * lane, make_float4(f[0], f[1], f[2], f[3]));
      }
      if (prog < (unsigned)(T - tc)) {   // dy[tc] exists once the layer above has published T - tc rows
        unsigned spins = 0;
        while (true) {
          prog = __builtin_amdgcn_readfirstlane(__hip_atomic_load(fl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
          if (prog >= (unsigned)(T - tc)) break;
          __builtin_amdgcn_s_sleep(1);
          if (++spins > WF_SPIN) {   // (see the forward loader: error word, and NaN instead of a plausible result)
            if (lane == 0) {
              __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
              vg_raise(wf_status_karg(offsetof(WfBwdArgs, c) + offsetof(WfCommon, status)), VMLMF_ST_WF_BWD);
            }
            prog = 0xffffffffu;
            dead = true;
            for (int i = lane; i < WF_BNB * NT; i += 64) tdy[i] = __builtin_nanf(""), tcp[i] = __builtin_nanf("");
            break;
          }
        }
      }
      if (dead) return;
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        const int slot = lane + 64 * i;
        const size_t e = (size_t)tc * sstride + (size_t)row * NT + slot;
        int n;
        wf_unit(slot, Hg, W, n);           // pad slots must not index past the row (n is clamped into the group)
        const size_t lo = (size_t)ring * NT + 64 * i;
        if constexpr (PAIR) {   // [ring][NT][2 dwords]
          if ((i & 1) == 0) dma16(a.gates + ((size_t)tc * sstride + (size_t)row * NT + 64 * i + 2 * lane) * 2, tg + ((size_t)ring * NT + 64 * i) * 2);
        } else if constexpr (BT) {   // 8 bytes per slot as two 4-byte DMAs (there is no 8-byte LDS-DMA) into two planes of the ring:
                                     // [ring][NT] dwords of (i, f), then [ring][NT] dwords of (o, n)
          dma4(a.gates + e * 2, tg + lo);
          dma4(a.gates + e * 2 + 1, tg + (size_t)WF_BNB * NT + lo);
        } else {
          dma16(a.gates + e * 4, tg + lo * 4);
        }
        dma4(a.cs + e, tcp + lo);              // slice tc = c_{tc-1}
        const float* dsrc = has_dy ? a.dy + ((size_t)tc * a.syT + (size_t)row * a.syB + n) : a.cs + e;
        if (poll) dma4_sys(dsrc, tdy + lo);
        else dma4(dsrc, tdy + lo);
      }
    };
    // Classifier prologue of the top layer (HeadBwd; see head_dh of rec_bwd_kernel): d(hT)[n] = sum_c dlogits[row][c] W[c][n],
    // formed by THIS wave while the compute waves load their weights, handed over in LDS (the dx stage, idle until the
    // x-team's first phase B) and published by barrier O.  In the compute waves the 2 x 32 loads would sit on top of the
    // recurrence's register budget; as a called function the kernel faulted in its two-wave instantiation.
    if (pos == 0 && args.hd.C > 0) {
      const HeadBwd hd = args.hd;
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        const int slot = lane + 64 * i;
        int nn;
        const bool uok = wf_unit(slot, Hg, W, nn);
        float w[32], d[32];
#pragma unroll
        for (int c = 0; c < 32; ++c) {
          const int cc = c < hd.C ? c : 0;
          w[c] = hd.W[(size_t)cc * H + nn];
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
        dxs[slot] = uok ? (a0 + a1) + (a2 + a3) : 0.f;
      }
    }
    if constexpr (G == 1) {
      if (!dropping)   // (the compute waves multiply dy by the ring's factors either way: ones, written once)
        for (int i = lane; i < WF_BNB * NT; i += 64) tfac[i] = 1.f;
    }
    for (int s0 = 0; s0 < DIST; ++s0) issue(T - 1 - s0);
    wait_vm_barrier<(DIST - 2) * NDMA>();       // O: tapes T-1 and T-2 have landed
    for (int t = T - 1; t >= 0; --t) {
      issue(t - DIST);
      wait_vm_barrier<DEPTH * NDMA>();          // b(t): tape t-2 has landed
    }
    // the word has reached its final value (the last row was polled for) and this loader is its only reader: cleared here,
    // a second backward over the same reserve (retain_graph) starts from zero again
    if (poll && lane == 0) __hip_atomic_store(fl, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    wf_barrier();   // E1
    wf_barrier();   // E2
    return;
  }

  if (wave == 2 * NW + 1) {   // --------------------------------------------------------- storer
    const int KH = g.KH, KX = g.KX;   // (the tapes keep their own widths)
    // dQ[ts][j][rr] = sum over the W waves of group j; one element per lane
    const bool qv = lane < G * KH, qxv_ok = lane < KX;
    const int qe = qv ? lane : 0, qj = qe / KH, qrr = qe - qj * KH;
    const unsigned qoff = 4u * (unsigned)(row * G * KH + qe), qxoff = 4u * (unsigned)(row * KX + (qxv_ok ? lane : 0));
    bool xv[NW];
    unsigned xo_[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      int nu;
      const bool uok = wf_unit(lane + 64 * i, Hg, W, nu);
      xv[i] = uok && nu < a.I && a.want_dx != 0;
      xo_[i] = (unsigned)((size_t)row * a.sxB + ((uok && nu < a.I) ? nu : 0)) * 4u;   // bytes into dx[t]
    }
    wgu32* fl = (wgu32*)(args.c.flag + ((size_t)(pub ? pos : 0) * B + row) * WF_FLAG_STRIDE);
    // segment u: dpre / dQ of step u + 1 and dx / dqx of step u + 3 (each when the step exists); every LDS read before
    // the first global store
    auto segment = [&](int u) {
      const int ta = u + 1, tb = u + 3;
      const bool hasA = ta >= 0 && ta < T, hasB = tb >= 0 && tb < T;
      const int tac = hasA ? ta : 0, tbc = hasB ? tb : 0;
      float4 d4[NW];
      float v[W], xs[NW];
      const float* src = outs + (size_t)(tac & 1) * NT * 4;
      const float* qsrc = part + (size_t)(tac & 1) * NW * KQ;
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        d4[i] = ld4(src + (size_t)(lane + 64 * i) * 4);
        xs[i] = dxs[(tbc & 1) * NT + lane + 64 * i];
      }
#pragma unroll
      for (int w = 0; w < W; ++w) v[w] = qsrc[(qj * W + w) * KQ + qrr];
      const float dqv = dqs[(tbc & 1) * 32 + (lane & 31)];
      if (hasA) {
        float* dt = a.dpre + (size_t)ta * sstride * 4;
#pragma unroll
        for (int i = 0; i < NW; ++i) st4_sv(dt, 16u * (unsigned)(row * NT + lane + 64 * i), d4[i]);
        float acc = 0.f;
#pragma unroll
        for (int w = 0; w < W; ++w) acc += v[w];
        // (the dword stores of this wave take the guarded form: with per-layer sizes in scalar registers some instantiations reload
        //  a base from its spill lane right in front of the store - vmlmf_device.h, hazard (2); 5 clocks a store on a wave off the chain)
        if (qv) st1_sv<true>(a.dQs + (size_t)ta * B * G * KH, qoff, acc);
      }
      if (hasB) {
        if (a.want_dx != 0) {
          const float* xt = a.dx + (size_t)tb * a.sxT;
#pragma unroll
          for (int i = 0; i < NW; ++i) {
            if (pub) {
              if (xv[i]) st1_sv_sys<true>(xt, xo_[i], xs[i]);
            } else {
              if (xv[i]) st1_sv<true>(xt, xo_[i], xs[i]);
            }
          }
        }
        if (qxv_ok) st1_sv<true>(a.dqx + (size_t)tb * B * KX, qxoff, dqv);
      }
      if (pub) {
        // leave exactly this segment's stores in flight: the previous segment's rows (dx of step u + 4) are in memory
        if (hasA && hasB) wait_vm<2 * NW + 2>();
        else if (hasA || hasB) wait_vm<NW + 1>();
        else wait_vm<0>();
        const int done = T - (u + 4);   // rows T-1 .. u+4
        if (done >= 1 && done <= T && lane == 0) __hip_atomic_store(fl, (unsigned)done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    };
    wf_barrier();   // O
    for (int u = T - 1; u >= -2; --u) {
      segment(u);
      wf_barrier();   // b(u) .. b(0), E1, E2
    }
    segment(-3);
    if (pub) {
      wait_vm<0>();
      if (lane == 0) __hip_atomic_store(fl, (unsigned)T, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    return;
  }

  // ------------------------------------------------------------------------------------- compute waves
  int n;
  const bool ok = wf_unit(tid, Hg, W, n);
  const int grp = tid / (64 * W);
  float vr[4][K];
  f32x2 ue2[K / 2];
  float eh[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int j = 0; j < K; ++j) vr[k][j] = a.VR[(size_t)(k * K + j) * NT + tid];
    eh[k] = a.EH[k * NT + tid];
  }
#pragma unroll
  for (int rr = 0; rr < K / 2; ++rr) ue2[rr] = f32x2{a.UE[(size_t)(2 * rr) * NT + tid], a.UE[(size_t)(2 * rr + 1) * NT + tid]};
  const int rdoff = Q::rdoff_g(lane, grp, g.off1, G);
  const size_t bh = (size_t)row * H + n;
  float dhrec = (ok && a.dhT != nullptr) ? a.dhT[bh] : 0.f;
  float dcs = (ok && a.dcT != nullptr) ? a.dcT[bh] : 0.f;
  float ccur = a.cs[(size_t)T * sstride + (size_t)row * NT + tid];
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");   // O
  if (pos == 0 && args.hd.C > 0) dhrec += dxs[tid];   // the classifier's d(hT) (formed by the loader wave)
  float4 g4n;
  float cprvn, dyvn;
  auto fetch_tape = [&](int tt) {
    const int ringn = ((tt % WF_BNB) + WF_BNB) % WF_BNB;
    const size_t lo = (size_t)ringn * NT + tid;
    if constexpr (BT) {
      constexpr bool PAIR = NW % 2 == 0;   // (the loader's layout: [ring][NT][2] or two planes)
      const unsigned p0 = __float_as_uint(PAIR ? tg[lo * 2] : tg[lo]), p1 = __float_as_uint(PAIR ? tg[lo * 2 + 1] : tg[(size_t)WF_BNB * NT + lo]);
      g4n = make_float4(__uint_as_float(p0 << 16), __uint_as_float(p0 & 0xffff0000u), __uint_as_float(p1 << 16), __uint_as_float(p1 & 0xffff0000u));
    } else {
      g4n = ld4(tg + lo * 4);
    }
    cprvn = tcp[lo];
    dyvn = tdy[lo];
    if constexpr (G == 1) dyvn *= tfac[lo];
  };
  CellBwdFactors fac;
  float fdy;
  auto prepare = [&]() {   // the dh-independent factors of the step whose tape was fetched (see rec_bwd_kernel)
    fac = cell_bwd_factors(g4n, ccur, cprvn);
    fdy = (ok && has_dy) ? dyvn : 0.f;
    ccur = cprvn;
  };
  fetch_tape(T - 1);
  prepare();
  for (int t = T - 1; t >= 0; --t) {
    const int buf = t & 1;
    const float dh = fdy + dhrec;
    const float4 d = cell_bwd_step(fac, dh, dcs);
    float dp[4] = {d.x, d.y, d.z, d.w};
    st4(outs + ((size_t)buf * NT + tid) * 4, d);
    const float ehterm = cell_ehterm(d, eh[0], eh[1], eh[2], eh[3]);
    wf_reduce4<K>(dp, vr, part + (buf * NW + wave) * KQ, lane);
    wf_barrier();   // b(t)
    fetch_tape(t - 1);   // landed since the previous barrier (t = 0: reads a valid, unused ring slot)
    const float* src = part + (size_t)buf * NW * KQ;
    const float4 v = ld4(rdoff >= 0 ? src + rdoff : zero4);
    float sx, sy, sz, sw;
    Q::finish(f32x4{v.x, v.y, v.z, v.w}, sx, sy, sz, sw);
    f32x2 d2 = f32x2{ehterm, 0.f}, d2b = f32x2{0.f, 0.f};
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) {
      d2 = pk_fma(f32x2{bcast_lane(sx, cc), bcast_lane(sy, cc)}, ue2[2 * cc + 0], d2);
      d2b = pk_fma(f32x2{bcast_lane(sz, cc), bcast_lane(sw, cc)}, ue2[2 * cc + 1], d2b);
    }
    d2 = d2 + d2b;
    dhrec = d2.x + d2.y;
    prepare();
  }
  wf_barrier();   // E1
  wf_barrier();   // E2
  if (ok) {
    if (a.dh0 != nullptr) a.dh0[bh] = dhrec;
    if (a.dc0 != nullptr) a.dc0[bh] = dcs;
  }
}

template <int K, int W, int G>
static int wf_bwd_launch(const VGeo& g, const WfBwdArgs& a, hipStream_t s) {
  constexpr int KQ = (K + 15) / 16 * 16, NW = G * W, NT = NW * 64, MAXT = NW <= 3 ? 192 : 256;
  const size_t lds = sizeof(float) * ((size_t)4 * NW * KQ + (size_t)WF_BNB * NT * 6 + (size_t)2 * NT * 4 + (size_t)2 * NT + 64 + 4 + (size_t)WF_BNB * NT);
  const int groups = (g.B + 7) / 8;
  auto kern = wf_bwd_kernel<K, W, G, MAXT>;
  if constexpr (G == 1 && (K == 16 || K == 24)) {
    if (g.bt) kern = wf_bwd_kernel<K, W, G, MAXT, true>;   // the forward of the call kept the gate tape as bf16
  } else if (g.bt) {
    return -3;
  }
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kern, dim3(groups * 8 * a.c.L), dim3(2 * NT + 128), lds, s, g, a);
  return (int)hipGetLastError();
}

template <int K>
static int wf_bwd_dispatch(const VGeo& g, const WfBwdArgs& a, hipStream_t s) {
  if (g.G == 2) {
    if (g.W == 1) return wf_bwd_launch<K, 1, 2>(g, a, s);
    if constexpr (K <= 24) {
      if (g.W == 2) return wf_bwd_launch<K, 2, 2>(g, a, s);
    }
    return -3;
  }
  switch (g.NW) {
    case 1: return wf_bwd_launch<K, 1, 1>(g, a, s);
    case 2: return wf_bwd_launch<K, 2, 1>(g, a, s);
    case 3: return wf_bwd_launch<K, 3, 1>(g, a, s);
    case 4:
      if constexpr (K <= 24) return wf_bwd_launch<K, 4, 1>(g, a, s);
      break;
  }
  return -3;
}
