// The beam step's selection, written once for libvmlmf_beam.so (vmlmf_beam.hip: every candidate is offered) and libvmlmf_beamctl.so
// (vmlmf_beamctl.hip: closed tokens, per-beam ban sets, a minimum length, the beams' histories) and libvmlmf_automaton.so
// (vmlmf_automaton.hip: closed tokens, a minimum length, a token automaton's state per beam): the candidate key, the workgroup
// maximum, the scratch, the step's kernel - templated on an OFFER POLICY, decided with `if constexpr`, so the plain instantiation is the
// code it was before the policy existed - and the host's refusals of sizes and pointers.
// A policy P has  static constexpr bool controlled;  and, where controlled,
//   row(row).closes(v)           whether beam `row` (= b W + w) withholds token v; row() is taken once, in front of pass 1, so what
//                                it loads (the beam's length) is not waited for between the passes
//   bool keeps_history()         uniform over the launch
//   hist / hist_len / hist_out / hist_len_out / overflow / cap    the histories the last workgroup of a batch row copies
// (a policy without keeps_history() keeps none), and, where it moves a state of its own on with the survivors,
//   survivor(slot, parent's row, parent finished, token, has a candidate)    called by the thread that writes the slot's outputs
// and, where the merge runs in GROUPS (libvmlmf_beamgroup.so, vmlmf_beamgroup.hip: diverse beam search), the members
//   int groups; float lambda     G divides W; group g owns beams and slots g Wg .. g Wg + Wg - 1 (Wg = W / G) and keeps the first Wg of
//                                ITS beams' candidates under aug = total - lambda n, n = how many survivors the groups before it chose in
//                                this step with the candidate's token and a live parent (include/vmlmf_beamgroup.h has the contract)
// The per-beam half needs no change for it.  Group g penalises at most g Wg <= W - Wg distinct tokens, and a beam holds each token
// once: among the beam's first W raw candidates at least Wg are unpenalised.  Each of those precedes every candidate of that beam
// outside its first W - in the raw order, and still after the penalty, because aug <= total (a rounded non-negative product is
// subtracted).  So a survivor of group g is among the first W raw candidates of one of the group's Wg beams: what the workspace holds.
// Selection: a workgroup per BEAM, a ticket per batch row.  A survivor of the row is among its own beam's first W candidates, so each
// workgroup forms those (W rounds of a workgroup-wide argmax over the threads' own best candidates; after a round only the thread
// that held the winner looks for its next one, strictly after the winner in the order - the winners wait in LDS, a global store per
// round would be waited for at every barrier), leaves them in the workspace and takes the row's ticket with an agent-scope release; the
// last of the W workgroups to arrive acquires, holds the W x W candidates one per thread, runs the same W rounds over them, writes the
// outputs and puts the ticket back to zero (the protocol of csrc/vmlmf_sample.hip).  No workgroup waits for another, so a captured
// launch replays and no co-residency is needed.  A candidate travels as one 64-bit key whose unsigned order is the order of the search
// (key_of), so a round is an integer maximum - no order of arrival to depend on -, taken word by word with DPP row steps (wg_max: a
// step is one wave's chain of dependent instructions, and twelve ds_bpermute a round were a third of it); the one floating-point
// reduction, (max, sum exp), runs in a fixed tree (64-lane butterfly, then the waves in order): bit-identical from run to run.
// Rows up to BS_LDS_V keep their totals in LDS between the rounds; longer rows re-read their scores and form each total again by the
// same three operations (the same bits).  A CLOSED candidate is a NaN in place of its total: the first scan and every rescan skip NaN,
// so the rounds cost a controlled step nothing; (max, sum exp) is taken over the raw row under every policy.
// Plain HIP C++ for wave64, no inline assembly.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>
#include <type_traits>

#include "../../include/vmlmf_beam.h"

namespace vmlmf_beam_core {

constexpr int BS_NT = 1024;        // threads of a selection workgroup: >= MAX_BEAMS^2, the merge holds one candidate per thread
constexpr int BS_NW = BS_NT / 64;
constexpr int BS_LDS_V = 12288;    // longest row whose totals stay in LDS (48 KB)
constexpr int BS_NOIDX = 0x7fffffff;
static_assert(VMLMF_BEAM_MAX_BEAMS * VMLMF_BEAM_MAX_BEAMS <= BS_NT, "the merge holds one candidate per thread");

struct BeamStepArgs {
  int B, W, H, V, eos;
  const float *scores, *bias, *cum, *embed;
  const int32_t *finished, *length;
  int32_t *parent, *finished_out, *length_out, *src_row;
  long long* token;
  float *total, *x_next;
  unsigned* ticket;
  unsigned long long* cand;   // workspace: (B W, W) candidate keys (key_of: total and flat index)
};

// the plain policy: everything open, no history
struct OfferAll {
  static constexpr bool controlled = false;
  struct Row {};
  __device__ __forceinline__ Row row(int) const { return Row{}; }
};

// what a policy declares beyond `controlled`, found at compile time: the plain and the controlled policy are asked nothing new
template <class P, class = void>
struct keeps_histories : std::false_type {};
template <class P>
struct keeps_histories<P, std::void_t<decltype(&P::keeps_history)>> : std::true_type {};
template <class P, class = void>
struct moves_states : std::false_type {};
template <class P>
struct moves_states<P, std::void_t<decltype(&P::survivor)>> : std::true_type {};
template <class P, class = void>
struct merges_in_groups : std::false_type {};
template <class P>
struct merges_in_groups<P, std::void_t<decltype(&P::groups), decltype(&P::lambda)>> : std::true_type {};

typedef unsigned long long u64;
// A candidate as ONE 64-bit key whose unsigned order is the order of the search: the order-preserving image of the total in the high
// word (larger total, larger key), BS_NOIDX - index in the low word (equal totals: lower index, larger key).  0 is "no candidate": no
// real key is 0 (that would be the image of a NaN), and a NaN total gets it - it comes nowhere in the order.  -0 is keyed as +0.
constexpr u64 BS_NONE = 0ull;
__device__ __forceinline__ u64 key_of(float t, int i) {
  if (t != t) return BS_NONE;
  const unsigned u = __float_as_uint(t + 0.f);
  return ((u64)(u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u)) << 32) | (unsigned)(BS_NOIDX - i);
}
__device__ __forceinline__ float total_of(u64 k) {
  const unsigned u = (unsigned)(k >> 32);
  return __uint_as_float(u ^ ((u >> 31) ? 0x80000000u : 0xffffffffu));
}
__device__ __forceinline__ int index_of(u64 k) { return BS_NOIDX - (int)(unsigned)k; }
struct BeamScratch {
  float vals[BS_LDS_V];
  u64 red_k[2][BS_NW];
  float red_m[BS_NW], red_s[BS_NW];
  u64 sel[VMLMF_BEAM_MAX_BEAMS];
  int last;
};

// max over each row of 16 lanes, in every lane of the row: four DPP steps (lane ^ 1, lane ^ 2, the other quad of the half row, the
// other half row), no LDS round trip.  Every lane of the wave must be active.
__device__ __forceinline__ unsigned row_max(unsigned v) {
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xf, 0xf, false));    // quad_perm [1, 0, 3, 2]
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xf, 0xf, false));    // quad_perm [2, 3, 0, 1]
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xf, 0xf, false));   // row_half_mirror
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xf, 0xf, false));   // row_mirror
  return v;
}
__device__ __forceinline__ unsigned wave_max(unsigned v) {
  v = row_max(v);
  return max(max((unsigned)__builtin_amdgcn_readlane((int)v, 0), (unsigned)__builtin_amdgcn_readlane((int)v, 16)),
             max((unsigned)__builtin_amdgcn_readlane((int)v, 32), (unsigned)__builtin_amdgcn_readlane((int)v, 48)));
}
// the workgroup's largest key of one per thread; every thread returns it.  A maximum of integers, word by word: the largest high
// word, then the largest low word among its holders.  `round` picks one of two LDS buffers, so one barrier a round is enough (a wave
// that is still reading round r never meets round r + 1's writes).  Every thread of the workgroup must call it.
__device__ __forceinline__ u64 wg_max(BeamScratch& S, int round, u64 k) {
  static_assert(BS_NW == 16, "the waves' maxima meet in one DPP row");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, buf = round & 1;
  unsigned hi = (unsigned)(k >> 32), lo = (unsigned)k;
  const unsigned whi = wave_max(hi);
  const unsigned wlo = wave_max(hi == whi ? lo : 0u);
  if (lane == 0) S.red_k[buf][wave] = ((u64)whi << 32) | wlo;
  __syncthreads();
  const u64 r = S.red_k[buf][lane & 15];
  hi = (unsigned)(r >> 32), lo = (unsigned)r;
  const unsigned ghi = row_max(hi);
  const unsigned glo = row_max(hi == ghi ? lo : 0u);
  return ((u64)ghi << 32) | glo;
}

// The step's kernel: either library instantiates it with its policy and launches it over B W workgroups of BS_NT threads.  The body
// stands in the __global__ function itself, not in a device function a kernel of each library would call: inlined from one, the
// compiler simplifies it before it knows the kernel's arguments and, measured on the plain step, came out with other instructions -
// the sum of the waves' partial sums contracted into fused multiply-adds, other bits.  As a template kernel the plain instantiation is
// instruction for instruction the kernel it was (docs/design/lm_beam_controls.md).
template <class P>
__global__ __launch_bounds__(BS_NT) void beam_step_kernel(BeamStepArgs a, P p) {
  __shared__ BeamScratch S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = blockIdx.x, b = row / a.W, w = row - b * a.W;
  const int V = a.V, W = a.W;
  const float cum = a.cum[row];
  const bool done = a.eos >= 0 && a.finished[row] != 0;
  const auto offer = p.row(row);   // (OfferAll: an empty object)
  if (done) {
    // a finished beam offers (w, eos) alone - whatever is closed
    if (tid < W) S.sel[tid] = tid == 0 ? key_of(cum, a.eos) : BS_NONE;
  } else {
    const float* sc = a.scores + (size_t)row * V;
    const bool resident = V <= BS_LDS_V;
    // pass 1: x = bias + score (kept in LDS where the row fits) and the thread's own (max, sum exp).  Eight elements' loads in flight
    // at a time: one after the other they cost a round trip each, and the pass has nothing else to wait for
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
      for (int j = 0; j < 8; ++j) bm = fmaxf(bm, x[j]);   // (the clamped repeats of x[0] change nothing)
      if (bm != -INFINITY) {
        s *= expf(m - bm);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (v0 + BS_NT * j < V) s += expf(x[j] - bm);
        m = bm;
      }
      if (resident) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (v0 + BS_NT * j < V) S.vals[v0 + BS_NT * j] = x[j];
      }
    }
    // the row's: the maximum first, then the sums rescaled to it, in a fixed tree (64-lane butterfly, then the waves in order)
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
    const float lse = M + logf(sum);
    // a candidate's total, formed by the same operations wherever it is formed; a closed candidate's is NaN - it is not offered
    auto total = [&](int v) {
      const float t = cum + (((a.bias != nullptr ? a.bias[v] : 0.f) + sc[v]) - lse);
      if constexpr (P::controlled) return offer.closes(v) ? NAN : t;
      else return t;
    };
    // the thread's best candidate; the totals replace x in LDS (a thread rewrites its own elements only)
    float bc = 0.f;
    int bv = BS_NOIDX;
    for (int v0 = tid; v0 < V; v0 += 8 * BS_NT) {
      float c[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int v = v0 + BS_NT * j < V ? v0 + BS_NT * j : v0;
        c[j] = resident ? cum + (S.vals[v] - lse) : total(v);
        if constexpr (P::controlled)
          if (resident && offer.closes(v)) c[j] = NAN;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int v = v0 + BS_NT * j;
        if (v < V) {
          if (resident) S.vals[v] = c[j];
          if (c[j] == c[j] && (bv == BS_NOIDX || c[j] > bc)) bc = c[j], bv = v;   // (rising v: an equal total does not replace)
        }
      }
    }
    // ... and its best strictly after the winner (lt, li) - plain float compares, the key is formed once at the end
    auto scan = [&](float lt, int li) {
      float bc = 0.f;
      int bv = BS_NOIDX;
      for (int v0 = tid; v0 < V; v0 += 8 * BS_NT) {
        float c[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int v = v0 + BS_NT * j < V ? v0 + BS_NT * j : v0;
          c[j] = resident ? S.vals[v] : total(v);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int v = v0 + BS_NT * j;
          const bool after = c[j] < lt || (c[j] == lt && v > li);
          if (v < V && after && (bv == BS_NOIDX || c[j] > bc)) bc = c[j], bv = v;
        }
      }
      return bv != BS_NOIDX ? key_of(bc, bv) : BS_NONE;
    };
    // W rounds of a workgroup-wide maximum over the threads' bests; only the thread that held the winner looks for its next one
    // (the others' bests still come after the winner and are still their best)
    u64 mine = bv != BS_NOIDX ? key_of(bc, bv) : BS_NONE;
    for (int r = 0; r < W; ++r) {
      const u64 k = wg_max(S, r, mine);
      if (tid == 0) S.sel[r] = k;   // (BS_NONE: nothing left that can be ordered - NaN scores, closed tokens -, and nothing will be)
      if (k != BS_NONE && mine == k) mine = scan(total_of(k), index_of(k));
    }
  }
  __syncthreads();
  // local index -> flat index w V + v; one store per thread, the barrier below orders them before thread 0's release
  if (tid < W) {
    const u64 k = S.sel[tid];
    a.cand[(size_t)row * W + tid] = k != BS_NONE ? key_of(total_of(k), w * V + index_of(k)) : BS_NONE;
  }
  __syncthreads();
  if (tid == 0) {
    const unsigned t = __hip_atomic_fetch_add(a.ticket + b, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    S.last = t == (unsigned)W - 1u;
  }
  __syncthreads();
  if (!S.last) return;
  // last arrival of batch row b: acquire in every wave, one candidate per thread, W rounds over them (flat indices are unique: the
  // thread that held a winner is out)
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  u64 mine = tid < W * W ? a.cand[(size_t)b * W * W + tid] : BS_NONE;
  if constexpr (merges_in_groups<P>::value) {
    // G passes, W rounds in all: in pass g the threads of group g's beams (thread tid holds a candidate of beam tid / W) rank their
    // candidate by aug, everybody else holds BS_NONE; the thread that held a round's winner leaves its RAW key in the slot and the
    // token it chose (-1: a finished parent's eos, which is no choice) in the totals' room, free since the rounds; behind a barrier
    // the next group counts its tokens there.  Every thread calls every wg_max.
    const int Wg = W / p.groups;
    int* chosen = reinterpret_cast<int*>(S.vals);
    const int beam = tid < W * W ? tid / W : 0, idx = index_of(mine);
    const int tok = idx - beam * V;   // (meaningful where mine is a candidate)
    const bool pdone = mine != BS_NONE && a.eos >= 0 && a.finished[b * W + beam] != 0;
    for (int g = 0; g < p.groups; ++g) {
      u64 key = BS_NONE;
      if (mine != BS_NONE && beam / Wg == g) {
        int n = 0;
        for (int i = 0; i < g * Wg; ++i) n += chosen[i] == tok ? 1 : 0;
        key = pdone || n == 0 ? mine : key_of(__fsub_rn(total_of(mine), __fmul_rn(p.lambda, (float)n)), idx);
      }
      for (int r = 0; r < Wg; ++r) {
        const int slot = g * Wg + r;
        const u64 k = wg_max(S, slot, key);
        if (k == BS_NONE) {   // nothing left that can be ordered in this group, and nothing will be
          if (tid == 0) S.sel[slot] = BS_NONE, chosen[slot] = -1;
        } else if (key == k) {
          S.sel[slot] = mine, chosen[slot] = pdone ? -1 : tok;
          key = BS_NONE;
        }
      }
      __syncthreads();
    }
  } else {
    for (int r = 0; r < W; ++r) {
      const u64 k = wg_max(S, r, mine);
      if (tid == 0) S.sel[r] = k;
      if (mine == k) mine = BS_NONE;
    }
  }
  __syncthreads();
  if (tid == 0) __hip_atomic_store(a.ticket + b, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid < W) {
    const u64 k = S.sel[tid];
    const int slot = b * W + tid;
    const bool ok = k != BS_NONE;
    const int i = ok ? index_of(k) : 0;
    const int par = i / V, tok = i - par * V;
    const int prow = b * W + par;
    const bool pdone = a.eos >= 0 && a.finished[prow] != 0;
    a.parent[slot] = par;
    a.token[slot] = tok;
    a.total[slot] = ok ? total_of(k) : NAN;
    a.finished_out[slot] = (pdone || (a.eos >= 0 && tok == a.eos)) ? 1 : 0;
    a.length_out[slot] = a.length[prow] + (pdone ? 0 : 1);
    a.src_row[slot] = prow;
    if constexpr (moves_states<P>::value) p.survivor(slot, prow, pdone, tok, ok);
    if constexpr (keeps_histories<P>::value) {
      // the survivor's history: where it comes from and how long it is, left in LDS (the totals' room, free since the rounds) for the
      // copy below; the token behind it and the lengths are this thread's own stores
      if (p.keeps_history()) {
        int L = p.hist_len[prow];
        L = L < 0 ? 0 : (L > p.cap ? p.cap : L);
        int* meta = reinterpret_cast<int*>(S.vals);
        meta[2 * tid] = prow, meta[2 * tid + 1] = L;
        int* ho = p.hist_out + (size_t)slot * p.cap;
        if (pdone) {
          p.hist_len_out[slot] = L;
        } else if (L < p.cap) {
          ho[L] = tok;
          p.hist_len_out[slot] = L + 1;
        } else {   // a full history is never written past
          p.hist_len_out[slot] = L;
          p.overflow[b] = 1;
        }
      }
    }
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
        const u64 k = S.sel[r];
        x[j] = a.embed[(size_t)(k != BS_NONE ? index_of(k) % V : 0) * a.H + c];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e0 + BS_NT * j < n) xo[e0 + BS_NT * j] = x[j];
    }
  }
  if constexpr (keeps_histories<P>::value) {
    if (p.keeps_history()) {   // (uniform)
      __syncthreads();
      const int* meta = reinterpret_cast<const int*>(S.vals);
      // the W histories, a wave per survivor at a time: hist_out[slot][0 .. L) = hist[parent's row][0 .. L)
      for (int r = wave; r < W; r += BS_NW) {
        const int prow = meta[2 * r], L = meta[2 * r + 1];
        const int* hi = p.hist + (size_t)prow * p.cap;
        int* ho = p.hist_out + (size_t)(b * W + r) * p.cap;
        for (int c0 = lane; c0 < L; c0 += 4 * 64) {   // four loads in flight
          int t[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) t[j] = hi[c0 + 64 * j < L ? c0 + 64 * j : c0];
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (c0 + 64 * j < L) ho[c0 + 64 * j] = t[j];
        }
      }
    }
  }
}

// ---- the host's refusals, shared by vmlmf_beam_step and vmlmf_beamctl_step ----
// 0, or why a step refuses these sizes
inline int step_sizes(int B, int W, int H, int V, int eos, std::string* why) {
  if (B < 1 || H < 1 || V < 1) return *why = "B, H and V must be >= 1", VMLMF_E_BADARG;
  if (W < 1 || W > VMLMF_BEAM_MAX_BEAMS) return *why = "W (beams) must lie in [1, 32]", VMLMF_E_BADARG;
  if (W > V) return *why = "W (beams) must not exceed V: a live beam offers V candidates", VMLMF_E_BADARG;
  if ((long long)W * (long long)V >= (1ll << 31)) return *why = "W V must stay below 2^31: flat candidate indices are 32-bit", VMLMF_E_BADARG;
  if ((long long)B * (long long)W >= (1ll << 31)) return *why = "B W must stay below 2^31", VMLMF_E_BADARG;
  if (eos < -1 || eos >= V) return *why = "eos must be a token in [0, V), or -1 for none", VMLMF_E_BADARG;
  return 0;
}
inline size_t step_workspace_bytes(int B, int W, int V) {
  std::string why;
  if (step_sizes(B, W, 1, V, -1, &why) != 0) return 0;
  return (size_t)B * (size_t)W * (size_t)W * sizeof(unsigned long long);
}
// 0 and the launch's arguments in `a`, or the code and the reason in `why` (without the entry point's name)
inline int step_args(BeamStepArgs& a, std::string* why, int B, int W, int H, int V, const float* scores, const float* bias, const float* cum,
                     const int32_t* finished, const int32_t* length, int eos, const float* embed, int32_t* parent, int64_t* token,
                     float* total, int32_t* finished_out, int32_t* length_out, float* x_next, int32_t* src_row, uint32_t* ticket,
                     void* workspace, size_t workspace_bytes, const char* workspace_fn) {
  if (const int rc = step_sizes(B, W, H, V, eos, why)) return rc;
  if (!scores || !cum || !finished || !length || !parent || !token || !total || !finished_out || !length_out || !src_row || !ticket ||
      !workspace)
    return *why = "null pointer (only bias, embed and x_next may be null)", VMLMF_E_BADARG;
  if ((embed == nullptr) != (x_next == nullptr)) return *why = "embed and x_next come together (both, or both null)", VMLMF_E_BADARG;
  if (cum == total || finished == finished_out || length == length_out)
    return *why = "the outputs must not alias the inputs (the merge reads cum, finished and length of other slots)", VMLMF_E_BADARG;
  if (((uintptr_t)workspace & 7u) != 0) return *why = "the workspace must be 8-byte aligned", VMLMF_E_BADARG;
  if (workspace_bytes < step_workspace_bytes(B, W, V))
    return *why = std::string("workspace smaller than ") + workspace_fn + "(B, W, V)", VMLMF_E_WORKSPACE;
  a.B = B, a.W = W, a.H = H, a.V = V, a.eos = eos;
  a.scores = scores, a.bias = bias, a.cum = cum, a.embed = embed, a.finished = finished, a.length = length;
  a.parent = parent, a.finished_out = finished_out, a.length_out = length_out, a.src_row = src_row;
  a.token = reinterpret_cast<long long*>(token), a.total = total, a.x_next = x_next, a.ticket = ticket;
  a.cand = static_cast<unsigned long long*>(workspace);
  return 0;
}

}  // namespace vmlmf_beam_core
