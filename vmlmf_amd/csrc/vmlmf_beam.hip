// The beam-search step of the LM decoder (Model.beam_search, vmlmf_amd/lm.py): libvmlmf_beam.so, a library of its own beside
// libvmlmf_hip.so (include/vmlmf_beam.h has the contract).  Three launches:
//   beam_step_kernel       one step's selection over the (B W, V) scores of the head's GEMM: per beam (max, sum exp), the candidate
//                          totals cum[w] + (x[v] - lse), the first W candidates of each batch row under the total order (larger total
//                          first, equal totals to the lower flat index w V + v - the sampler's tie rule over beams), and per survivor
//                          parent, token, total, finished flag, length, the next input row embed[token] and the source state row
//   beam_gather_kernel     the 2 L state tensors reordered by the source rows, all in one launch over a pointer table passed by value
//   beam_backtrack_kernel  the (steps, B, W) parent / token arrays read back into hypotheses, one thread per (b, w)
// Selection: a workgroup per BEAM, a ticket per batch row.  A survivor of the row is among its own beam's first W candidates, so each
// workgroup forms those (W rounds of a workgroup-wide argmax over the threads' own best candidates; after a round only the thread
// that held the winner looks for its next one, strictly after the winner in the order - the winners wait in LDS, a global store per
// round would be waited for at every barrier), leaves them in the workspace and takes the row's ticket with an agent-scope release; the last of the W workgroups to arrive acquires, holds the W x W candidates one per thread, runs the same W
// rounds over them, writes the outputs and puts the ticket back to zero (the protocol of csrc/vmlmf_sample.hip).  No workgroup waits
// for another, so a captured launch replays and no co-residency is needed.  A candidate travels as one 64-bit key whose unsigned order
// is the order of the search (key_of), so a round is an integer maximum - no order of arrival to depend on -, taken word by word
// with DPP row steps (wg_max: a step is one wave's chain of dependent instructions, and twelve ds_bpermute a round were a third of
// it); the one floating-point reduction, (max, sum exp), runs in a fixed tree (64-lane butterfly, then the waves in order):
// bit-identical from run to run.  docs/design/lm_beam_search.md has the numbers.
// Rows up to BS_LDS_V keep their totals in LDS between the rounds; longer rows re-read their scores and form each total again by the
// same three operations (the same bits).  Plain HIP C++ for wave64, no inline assembly.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vmlmf_beam.h"
#include "vmlmf_side.h"

namespace {

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

__global__ __launch_bounds__(BS_NT) void beam_step_kernel(BeamStepArgs a) {
  __shared__ BeamScratch S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = blockIdx.x, b = row / a.W, w = row - b * a.W;
  const int V = a.V, W = a.W;
  const float cum = a.cum[row];
  const bool done = a.eos >= 0 && a.finished[row] != 0;
  if (done) {
    // a finished beam offers (w, eos) alone
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
    // a candidate's total, formed by the same operations wherever it is formed
    auto total = [&](int v) { return cum + (((a.bias != nullptr ? a.bias[v] : 0.f) + sc[v]) - lse); };
    // the thread's best candidate; the totals replace x in LDS (a thread rewrites its own elements only)
    float bc = 0.f;
    int bv = BS_NOIDX;
    for (int v0 = tid; v0 < V; v0 += 8 * BS_NT) {
      float c[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int v = v0 + BS_NT * j < V ? v0 + BS_NT * j : v0;
        c[j] = resident ? cum + (S.vals[v] - lse) : total(v);
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
      if (tid == 0) S.sel[r] = k;   // (BS_NONE: nothing left that can be ordered - NaN scores -, and nothing will be)
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
  for (int r = 0; r < W; ++r) {
    const u64 k = wg_max(S, r, mine);
    if (tid == 0) S.sel[r] = k;
    if (mine == k) mine = BS_NONE;
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
}

struct BeamGatherArgs {
  const float* src[VMLMF_BEAM_MAX_TENSORS];
  float* dst[VMLMF_BEAM_MAX_TENSORS];
  const int32_t* src_row;
  int rows, H;
};
// grid (rows, n): workgroup (r, i) copies row src_row[r] of tensor i
__global__ __launch_bounds__(256) void beam_gather_kernel(BeamGatherArgs a) {
  const int r = blockIdx.x, i = blockIdx.y;
  int sr = a.src_row[r];
  if (sr < 0 || sr >= a.rows) sr = r;
  const float* s = a.src[i] + (size_t)sr * a.H;
  float* d = a.dst[i] + (size_t)r * a.H;
  for (int k = threadIdx.x; k < a.H; k += 256) d[k] = s[k];
}

__global__ __launch_bounds__(64) void beam_backtrack_kernel(int steps, int B, int W, const int32_t* parent, const long long* token,
                                                            const int32_t* order, long long* out) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= B * W) return;
  const int b = e / W;
  int cur = order != nullptr ? order[e] : e - b * W;
  for (int j = steps - 1; j >= 0; --j) {
    if (cur < 0 || cur >= W) cur = 0;
    const size_t at = ((size_t)j * B + b) * W + cur;
    out[((size_t)j * B) * W + e] = token[at];
    cur = parent[at];
  }
}

using vmlmf_side::fail;   // (every call site gives the entry point's name itself)
// 0, or why vmlmf_beam_step refuses these sizes
int step_sizes(int B, int W, int H, int V, int eos, std::string* why) {
  if (B < 1 || H < 1 || V < 1) return *why = "B, H and V must be >= 1", VMLMF_E_BADARG;
  if (W < 1 || W > VMLMF_BEAM_MAX_BEAMS) return *why = "W (beams) must lie in [1, 32]", VMLMF_E_BADARG;
  if (W > V) return *why = "W (beams) must not exceed V: a live beam offers V candidates", VMLMF_E_BADARG;
  if ((long long)W * (long long)V >= (1ll << 31)) return *why = "W V must stay below 2^31: flat candidate indices are 32-bit", VMLMF_E_BADARG;
  if ((long long)B * (long long)W >= (1ll << 31)) return *why = "B W must stay below 2^31", VMLMF_E_BADARG;
  if (eos < -1 || eos >= V) return *why = "eos must be a token in [0, V), or -1 for none", VMLMF_E_BADARG;
  return 0;
}

}  // namespace

VMLMF_SIDE_LIBRARY(vmlmf_beam, VMLMF_BEAM_ABI_VERSION)

extern "C" {

size_t vmlmf_beam_workspace_bytes(int B, int W, int V) {
  std::string why;
  if (step_sizes(B, W, 1, V, -1, &why) != 0) return 0;
  return (size_t)B * (size_t)W * (size_t)W * sizeof(unsigned long long);
}

int vmlmf_beam_step(int B, int W, int H, int V, const float* scores, const float* bias, const float* cum, const int32_t* finished,
                    const int32_t* length, int eos, const float* embed, int32_t* parent, int64_t* token, float* total,
                    int32_t* finished_out, int32_t* length_out, float* x_next, int32_t* src_row, uint32_t* ticket, void* workspace,
                    size_t workspace_bytes, void* stream) {
  std::string why;
  if (const int rc = step_sizes(B, W, H, V, eos, &why)) return fail(rc, "vmlmf_beam_step: " + why);
  if (!scores || !cum || !finished || !length || !parent || !token || !total || !finished_out || !length_out || !src_row || !ticket ||
      !workspace)
    return fail(VMLMF_E_BADARG, "vmlmf_beam_step: null pointer (only bias, embed and x_next may be null)");
  if ((embed == nullptr) != (x_next == nullptr))
    return fail(VMLMF_E_BADARG, "vmlmf_beam_step: embed and x_next come together (both, or both null)");
  if (cum == total || finished == finished_out || length == length_out)
    return fail(VMLMF_E_BADARG, "vmlmf_beam_step: the outputs must not alias the inputs (the merge reads cum, finished and length of other slots)");
  if (((uintptr_t)workspace & 7u) != 0) return fail(VMLMF_E_BADARG, "vmlmf_beam_step: the workspace must be 8-byte aligned");
  if (workspace_bytes < vmlmf_beam_workspace_bytes(B, W, V))
    return fail(VMLMF_E_WORKSPACE, "vmlmf_beam_step: workspace smaller than vmlmf_beam_workspace_bytes(B, W, V)");
  BeamStepArgs a;
  a.B = B, a.W = W, a.H = H, a.V = V, a.eos = eos;
  a.scores = scores, a.bias = bias, a.cum = cum, a.embed = embed, a.finished = finished, a.length = length;
  a.parent = parent, a.finished_out = finished_out, a.length_out = length_out, a.src_row = src_row;
  a.token = reinterpret_cast<long long*>(token), a.total = total, a.x_next = x_next, a.ticket = ticket;
  a.cand = static_cast<unsigned long long*>(workspace);
  hipLaunchKernelGGL(beam_step_kernel, dim3(B * W), dim3(BS_NT), 0, static_cast<hipStream_t>(stream), a);
  return vmlmf_side::launch_tail("vmlmf_beam_step");
}

int vmlmf_beam_gather(int n, int rows, int H, const int32_t* src_row, const void* const* src, void* const* dst, void* stream) {
  if (n < 1 || n > VMLMF_BEAM_MAX_TENSORS) return fail(VMLMF_E_BADARG, "vmlmf_beam_gather: n must lie in [1, 16] tensors a launch");
  if (rows < 1 || H < 1) return fail(VMLMF_E_BADARG, "vmlmf_beam_gather: rows and H must be >= 1");
  if (rows > 65535 * 1024) return fail(VMLMF_E_BADARG, "vmlmf_beam_gather: too many rows for one launch");
  if (!src_row || !src || !dst) return fail(VMLMF_E_BADARG, "vmlmf_beam_gather: null pointer");
  BeamGatherArgs a;
  for (int i = 0; i < VMLMF_BEAM_MAX_TENSORS; ++i) a.src[i] = nullptr, a.dst[i] = nullptr;
  for (int i = 0; i < n; ++i) {
    if (!src[i] || !dst[i]) return fail(VMLMF_E_BADARG, "vmlmf_beam_gather: null pointer in the table");
    a.src[i] = static_cast<const float*>(src[i]), a.dst[i] = static_cast<float*>(dst[i]);
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j)
      if (dst[i] == src[j]) return fail(VMLMF_E_BADARG, "vmlmf_beam_gather: a destination is also a source (rows would be read after they were overwritten)");
  a.src_row = src_row, a.rows = rows, a.H = H;
  hipLaunchKernelGGL(beam_gather_kernel, dim3(rows, n), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return vmlmf_side::launch_tail("vmlmf_beam_gather");
}

int vmlmf_beam_backtrack(int steps, int B, int W, const int32_t* parent, const int64_t* token, const int32_t* order, int64_t* out,
                         void* stream) {
  if (steps < 1 || B < 1) return fail(VMLMF_E_BADARG, "vmlmf_beam_backtrack: steps and B must be >= 1");
  if (W < 1 || W > VMLMF_BEAM_MAX_BEAMS) return fail(VMLMF_E_BADARG, "vmlmf_beam_backtrack: W (beams) must lie in [1, 32]");
  if ((long long)B * W >= (1ll << 31)) return fail(VMLMF_E_BADARG, "vmlmf_beam_backtrack: B W must stay below 2^31");
  if (!parent || !token || !out) return fail(VMLMF_E_BADARG, "vmlmf_beam_backtrack: null pointer (only order may be null)");
  hipLaunchKernelGGL(beam_backtrack_kernel, dim3((B * W + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream), steps, B, W, parent,
                     reinterpret_cast<const long long*>(token), order, reinterpret_cast<long long*>(out));
  return vmlmf_side::launch_tail("vmlmf_beam_backtrack");
}

}  // extern "C"
