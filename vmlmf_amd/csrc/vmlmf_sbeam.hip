// The step of stochastic beam search (Model.stochastic_beam_search; Kool, van Hoof and Welling, "Stochastic Beams and Where to Find
// Them"): libvmlmf_sbeam.so, a library of its own beside libvmlmf_beam.so (include/vmlmf_sbeam.h has the contract), built by the
// Makefile's `beyond`.  One launch over B W workgroups of BS_NT threads, a workgroup per beam, a ticket per batch row:
//   sbeam_step_kernel      pass 1  x = bias + score to LDS and the thread's (max, sum exp) - vmlmf_beam_step's pass 1 and its fixed
//                                  reduction tree, operation for operation (the one contraction the plain kernel's compiler made, s E + e0
//                                  in pass 1, is written out as fmaf; everything else is rounded separately): lse has the plain step's bits
//                          pass 2  a thread takes four neighbouring tokens at a time, one Philox call for them (as choose_row does):
//                                  gt = phi + gumbel replaces x in LDS; Z = max gt over the workgroup
//                          pass 3  G, the perturbed value conditioned on the parent's T and the maximum Z, replaces gt in LDS; the
//                                  thread's best candidate by (G, index)
//                          rounds  W rounds of wg_max over the threads' bests, the winner's thread rescans its own tokens in LDS
//                          merge   the beam's W keys (G, flat index) and their phi go to the workspace; the row's last workgroup holds the
//                                  W x W candidates one per thread, runs W rounds over them and writes the outputs
// Rows beyond BS_LDS_V keep nothing in LDS: passes 2 and 3 and every rescan re-read the scores and form gt and G again by the same
// operations - the same bits.  The key, the maxima, the scratch, the ticket protocol and the host's refusals are vmlmf_beam_core.h's,
// the noise is vmlmf_select.h's; this file holds no copy of either.  docs/design/lm_sbeam.md has the budget and the numbers.
// Plain HIP C++ for wave64, no inline assembly, no float atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vmlmf_sbeam.h"
#include "vmlmf_beam_core.h"
#include "vmlmf_select.h"
#include "vmlmf_side.h"

namespace {

using namespace vmlmf_beam_core;
typedef unsigned long long k64;   // a candidate key (vmlmf_beam_core::key_of)

// what the step takes beyond vmlmf_beam_step's arguments
struct SbeamArgs {
  const float* perturbed;
  float* perturbed_out;
  const int32_t* draw;
  int32_t* draw_out;
  const unsigned long long* state;
  float* cand_phi;   // workspace behind the keys: (B W, W) totals of the candidates
};

__global__ __launch_bounds__(BS_NT) void sbeam_step_kernel(BeamStepArgs a, SbeamArgs g) {
  // every operation below is rounded on its own: the contract states them one by one, and lse must keep the plain step's bits
#pragma clang fp contract(off)
  __shared__ __align__(16) BeamScratch S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = blockIdx.x, b = row / a.W, w = row - b * a.W;
  const int V = a.V, W = a.W;
  const float cum = a.cum[row], T = g.perturbed[row];
  const bool done = a.eos >= 0 && a.finished[row] != 0;
  const float* sc = a.scores + (size_t)row * V;
  float lse = 0.f;
  if (done) {
    // a finished beam offers (w, eos) alone and keeps its value
    if (tid < W) S.sel[tid] = tid == 0 ? key_of(T, a.eos) : BS_NONE;
  } else {
    const bool resident = V <= BS_LDS_V;
    // pass 1 (vmlmf_beam_core.h's): x = bias + score, kept in LDS where the row fits, and the thread's own (max, sum exp); eight
    // elements' loads in flight
    float m = -INFINITY, s = 0.f;
    for (int v0 = tid; v0 < V; v0 += 8 * BS_NT) {
      float x[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int v = v0 + BS_NT * j < V ? v0 + BS_NT * j : v0;
        x[j] = (a.bias != nullptr ? a.bias[v] : 0.f) + sc[v];
      }
      float bm = m;
#pragma unroll
      for (int j = 0; j < 8; ++j) bm = fmaxf(bm, x[j]);
      if (bm != -INFINITY) {
        s = fmaf(s, expf(m - bm), expf(x[0] - bm));   // (the plain kernel's one fused operation; element 0 is always in range)
#pragma unroll
        for (int j = 1; j < 8; ++j)
          if (v0 + BS_NT * j < V) s += expf(x[j] - bm);
        m = bm;
      }
      if (resident) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (v0 + BS_NT * j < V) S.vals[v0 + BS_NT * j] = x[j];
      }
    }
    // the row's: the maximum first, then the sums rescaled to it, in the plain step's fixed tree
    float wm = m;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) wm = fmaxf(wm, __shfl_xor(wm, o, 64));
    float ws = wm != -INFINITY ? s * expf(m - wm) : 0.f;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) ws += __shfl_xor(ws, o, 64);
    if (lane == 0) S.red_m[wave] = wm, S.red_s[wave] = ws;
    __syncthreads();
    float M = S.red_m[0];
#pragma unroll
    for (int k = 1; k < BS_NW; ++k) M = fmaxf(M, S.red_m[k]);
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < BS_NW; ++k) sum += M != -INFINITY ? S.red_s[k] * expf(S.red_m[k] - M) : 0.f;
    lse = M + logf(sum);

    // from here a thread owns QUADS of neighbouring tokens, qd = tid, tid + BS_NT, ...: one Philox call serves a quad (the barrier above
    // stands between pass 1's stores and these reads)
    const DropKey key = sample_key(g.state);
    const unsigned position = (unsigned)g.draw[b] * ((unsigned)a.B * (unsigned)W) + (unsigned)b * (unsigned)W + (unsigned)w;
    const int quads = (V + 3) >> 2;
    float4* vals4 = reinterpret_cast<float4*>(S.vals);
    // x of tokens 4 qd .. 4 qd + 3 (past V: anything)
    auto load_x = [&](int qd, float(&x)[4]) {
      if (resident) {
        const float4 t = vals4[qd];
        x[0] = t.x, x[1] = t.y, x[2] = t.z, x[3] = t.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int v = 4 * qd + e < V ? 4 * qd + e : V - 1;
          x[e] = (a.bias != nullptr ? a.bias[v] : 0.f) + sc[v];
        }
      }
    };
    // gt = phi + gumbel of the quad's tokens; NaN past V - no candidate, and skipped by every maximum
    auto gt_of = [&](int qd, const float(&x)[4], float(&gt)[4]) {
      unsigned wd[4];
      philox4x32_10(position, (unsigned)qd, key.c2, key.c3, key.k0, key.k1, wd);
#pragma unroll
      for (int e = 0; e < 4; ++e) gt[e] = 4 * qd + e < V ? (cum + (x[e] - lse)) + gumbel_of(wd[e]) : NAN;
    };
    // pass 2: gt to LDS, the thread's maximum; two quads' loads in flight (eight tokens)
    float zt = -INFINITY;
    for (int q0 = tid; q0 < quads; q0 += 2 * BS_NT) {
      float x[2][4];
#pragma unroll
      for (int j = 0; j < 2; ++j) load_x(q0 + BS_NT * j < quads ? q0 + BS_NT * j : q0, x[j]);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int qd = q0 + BS_NT * j;
        if (qd < quads) {
          float gt[4];
          gt_of(qd, x[j], gt);
          if (resident) vals4[qd] = make_float4(gt[0], gt[1], gt[2], gt[3]);
#pragma unroll
          for (int e = 0; e < 4; ++e) zt = fmaxf(zt, gt[e]);
        }
      }
    }
    // Z = max gt: an exact maximum, any tree.  The waves' maxima meet in wg_max's second buffer, which round 0 does not touch and
    // round 1 writes behind round 0's barrier
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) zt = fmaxf(zt, __shfl_xor(zt, o, 64));
    float* zred = reinterpret_cast<float*>(&S.red_k[1][0]);
    if (lane == 0) zred[wave] = zt;
    __syncthreads();
    float Z = zred[0];
#pragma unroll
    for (int k = 1; k < BS_NW; ++k) Z = fmaxf(Z, zred[k]);
    // the candidate's perturbed value (include/vmlmf_sbeam.h states the operations)
    auto G_of = [&](float gt) {
      float G = T;
      if (gt != Z) {
        const float u = (T - gt) + log1pf(-expf(gt - Z));
        G = (T - fmaxf(u, 0.f)) - log1pf(expf(-fabsf(u)));
      }
      if (T == -INFINITY || cum == -INFINITY || gt == -INFINITY) G = -INFINITY;
      return gt != gt ? NAN : G;
    };
    // G of the quad's tokens wherever it is asked for: from LDS, or formed again by the same operations
    auto G_quad = [&](int qd, float(&G)[4]) {
      if (resident) {
        const float4 t = vals4[qd];
        G[0] = t.x, G[1] = t.y, G[2] = t.z, G[3] = t.w;
      } else {
        float x[4], gt[4];
        load_x(qd, x);
        gt_of(qd, x, gt);
#pragma unroll
        for (int e = 0; e < 4; ++e) G[e] = G_of(gt[e]);
      }
    };
    // pass 3: G replaces gt in LDS (a thread rewrites its own quads only); the thread's best candidate
    float bc = 0.f;
    int bv = BS_NOIDX;
    for (int qd = tid; qd < quads; qd += BS_NT) {
      float G[4];
      if (resident) {
        const float4 t = vals4[qd];
        G[0] = G_of(t.x), G[1] = G_of(t.y), G[2] = G_of(t.z), G[3] = G_of(t.w);
        vals4[qd] = make_float4(G[0], G[1], G[2], G[3]);
      } else {
        G_quad(qd, G);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int v = 4 * qd + e;
        if (v < V && G[e] == G[e] && (bv == BS_NOIDX || G[e] > bc)) bc = G[e], bv = v;   // (rising v: an equal G does not replace)
      }
    }
    // ... and its best strictly after the winner (lt, li)
    auto scan = [&](float lt, int li) {
      float bc = 0.f;
      int bv = BS_NOIDX;
      for (int qd = tid; qd < quads; qd += BS_NT) {
        float G[4];
        G_quad(qd, G);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int v = 4 * qd + e;
          const bool after = G[e] < lt || (G[e] == lt && v > li);
          if (v < V && after && (bv == BS_NOIDX || G[e] > bc)) bc = G[e], bv = v;
        }
      }
      return bv != BS_NOIDX ? key_of(bc, bv) : BS_NONE;
    };
    // W rounds of a workgroup-wide maximum over the threads' bests; only the thread that held the winner looks for its next one
    k64 mine = bv != BS_NOIDX ? key_of(bc, bv) : BS_NONE;
    for (int r = 0; r < W; ++r) {
      const k64 k = wg_max(S, r, mine);
      if (tid == 0) S.sel[r] = k;
      if (k != BS_NONE && mine == k) mine = scan(total_of(k), index_of(k));
    }
  }
  __syncthreads();
  // local index -> flat index w V + v, and the candidate's total by the plain step's three operations; the stores of a thread stand in
  // front of the barrier below, which orders them before thread 0's release
  if (tid < W) {
    const k64 k = S.sel[tid];
    float phi = NAN;
    if (k != BS_NONE) {
      const int v = index_of(k);
      phi = done ? cum : cum + (((a.bias != nullptr ? a.bias[v] : 0.f) + sc[v]) - lse);
    }
    a.cand[(size_t)row * W + tid] = k != BS_NONE ? key_of(total_of(k), w * V + index_of(k)) : BS_NONE;
    g.cand_phi[(size_t)row * W + tid] = phi;
  }
  __syncthreads();
  if (tid == 0) {
    const unsigned t = __hip_atomic_fetch_add(a.ticket + b, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    S.last = t == (unsigned)W - 1u;
  }
  __syncthreads();
  if (!S.last) return;
  // last arrival of batch row b: acquire in every wave, one candidate per thread, W rounds over them (flat indices are unique: the
  // thread that held a winner leaves its total in the values' room, free since the rounds, and is out)
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  k64 mine = tid < W * W ? a.cand[(size_t)b * W * W + tid] : BS_NONE;
  const float mine_phi = tid < W * W ? g.cand_phi[(size_t)b * W * W + tid] : 0.f;
  float* sel_phi = S.vals;
  for (int r = 0; r < W; ++r) {
    const k64 k = wg_max(S, r, mine);
    if (tid == 0) S.sel[r] = k;
    if (k != BS_NONE && mine == k) sel_phi[r] = mine_phi, mine = BS_NONE;
  }
  __syncthreads();
  if (tid == 0) {
    g.draw_out[b] = g.draw[b] + 1;
    __hip_atomic_store(a.ticket + b, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (tid < W) {
    const k64 k = S.sel[tid];
    const int slot = b * W + tid;
    const bool ok = k != BS_NONE;
    const int i = ok ? index_of(k) : 0;
    const int par = i / V, tok = i - par * V;
    const int prow = b * W + par;
    const bool pdone = a.eos >= 0 && a.finished[prow] != 0;
    a.parent[slot] = par;
    a.token[slot] = tok;
    a.total[slot] = ok ? sel_phi[tid] : NAN;
    g.perturbed_out[slot] = ok ? total_of(k) : NAN;
    a.finished_out[slot] = (pdone || (a.eos >= 0 && tok == a.eos)) ? 1 : 0;
    a.length_out[slot] = a.length[prow] + (pdone ? 0 : 1);
    a.src_row[slot] = prow;
  }
  if (a.x_next != nullptr) {
    const int n = W * a.H;
    float* xo = a.x_next + (size_t)b * n;
    for (int e0 = tid; e0 < n; e0 += 4 * BS_NT) {   // four rows' loads in flight
      float x[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = e0 + BS_NT * j < n ? e0 + BS_NT * j : e0;
        const int r = e / a.H, c = e - r * a.H;
        const k64 k = S.sel[r];
        x[j] = a.embed[(size_t)(k != BS_NONE ? index_of(k) % V : 0) * a.H + c];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e0 + BS_NT * j < n) xo[e0 + BS_NT * j] = x[j];
    }
  }
}

using vmlmf_side::fail;

}  // namespace

VMLMF_SIDE_LIBRARY(vmlmf_sbeam, VMLMF_SBEAM_ABI_VERSION)

extern "C" {

// the keys of vmlmf_beam_step's workspace and an fp32 total beside each
size_t vmlmf_sbeam_workspace_bytes(int B, int W, int V) { return step_workspace_bytes(B, W, V) / 8 * 12; }

int vmlmf_sbeam_step(int B, int W, int H, int V, const float* scores, const float* bias, const float* cum, const int32_t* finished,
                     const int32_t* length, int eos, const float* embed, int32_t* parent, int64_t* token, float* total,
                     int32_t* finished_out, int32_t* length_out, float* x_next, int32_t* src_row, uint32_t* ticket, void* workspace,
                     size_t workspace_bytes, const float* perturbed, float* perturbed_out, const int32_t* draw, int32_t* draw_out,
                     const void* state, void* stream) {
  const std::string name = "vmlmf_sbeam_step: ";
  std::string why;
  BeamStepArgs a;
  if (const int rc = step_args(a, &why, B, W, H, V, scores, bias, cum, finished, length, eos, embed, parent, token, total, finished_out,
                               length_out, x_next, src_row, ticket, workspace, workspace_bytes, "vmlmf_sbeam_workspace_bytes"))
    return fail(rc, name + why);
  if (!perturbed || !perturbed_out || !draw || !draw_out || !state)
    return fail(VMLMF_E_BADARG, name + "null pointer (perturbed, perturbed_out, draw, draw_out and state are required)");
  if (perturbed_out == perturbed || perturbed_out == cum || perturbed_out == total || total == perturbed || draw_out == draw)
    return fail(VMLMF_E_BADARG, name + "the outputs must not alias the inputs or each other (perturbed_out, total, draw_out)");
  if (workspace_bytes < vmlmf_sbeam_workspace_bytes(B, W, V))
    return fail(VMLMF_E_WORKSPACE, name + "workspace smaller than vmlmf_sbeam_workspace_bytes(B, W, V)");
  SbeamArgs g;
  g.perturbed = perturbed, g.perturbed_out = perturbed_out, g.draw = draw, g.draw_out = draw_out;
  g.state = static_cast<const unsigned long long*>(state);
  g.cand_phi = reinterpret_cast<float*>(static_cast<char*>(workspace) + step_workspace_bytes(B, W, V));
  hipLaunchKernelGGL(sbeam_step_kernel, dim3(B * W), dim3(BS_NT), 0, static_cast<hipStream_t>(stream), a, g);
  return vmlmf_side::launch_tail("vmlmf_sbeam_step");
}

}  // extern "C"
