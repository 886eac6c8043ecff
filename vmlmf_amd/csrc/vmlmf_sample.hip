// One decoded token of the LM (Model.generate, vmlmf_amd/lm.py) in ONE launch: the vocabulary projection of the top layer's
// output (Linear, V/src/models/vmlmf_lm.py:345-361: fc.w (V, H) row-major, fc.b (V)), the choice of the next token, its
// log-probability and - optionally - the next step's input row of the embedding table.  No (B, V) score tensor exists.
//   scores[b][v] = fc.b[v] + sum_k h[b][k] fc.w[v][k]               fp32, fixed order (bit-identical from run to run)
//   greedy (inverse temperature 0):  token = argmax_v scores[b][v], ties to the lowest index
//   sampling:                         token = argmax_v scores[b][v] / tau + G[b][v], G = -log(-log u) Gumbel noise: exactly a draw
//                                     from softmax(scores / tau) without sort, prefix sum or probability tensor
//   logprob[b] = scores[b][token] - logsumexp_v scores[b][v]    (untempered: what nll_loss charges for that token)
// u comes from Philox4x32-10 laid out as the dropout's (vmlmf_dropout.h): counter = (position = step B + b, v >> 2, SITE_SAMPLE,
// offset low word), key = (seed low word, seed high word + offset high word), word = out[v & 3], u = ((word >> 8) + 0.5) 2^-24.
//
// Tiles.  A workgroup (four waves) owns a strip of `tpw` vocabulary tiles of 16 rows; each tile is one 16 x 16 block of scores on
// v_mfma_f32_16x16x4_f32 (M = vocabulary rows, N = batch rows padded to 16), the four waves splitting H (lane (r, q) of wave w
// feeds k = 16 i + 4 w + q of step i) and meeting in LDS in wave order.  A batch wider than 16 takes passes of 16 rows.
// Merge.  Each workgroup leaves per batch row (best perturbed score, its raw score and index) and (max, sum of exp) of its strip,
// written through to agent scope, then takes a ticket; the LAST workgroup to arrive merges the strips in a fixed tree, writes the
// outputs and puts the ticket back to zero.  Nobody waits for anybody: no co-residency is needed, a captured launch replays.
//
// Filters (top_k, top_p; the *_filtered entry points).  They act on the tempered scores z = scores / tau, in the order temperature,
// top-k, top-p over the renormalised survivors of top-k, under ONE total order on tokens: larger z first, equal z to the lower index
// (best_merge's tie rule).
//   top_k = k        exactly the first min(k, V) tokens of the order are kept (0 and k >= V: off)
//   top_p = p        of those, the shortest prefix whose mass reaches p: the token at sorted position j is kept iff the mass of the
//                    tokens before it is < p (the first token always is; 1: off).  Mass = exp(z_v - z_max) over the set top-k kept,
//                    normalised by its own sum, held in FIXED POINT with 40 fractional bits (the largest token's mass is 2^40, a row's
//                    sum stays below 2^63 for V < 2^23): integer sums do not depend on the order of arrival.
//   token = argmax over the kept set of z + G, G exactly the unfiltered kernels' noise for (step B + b, v); Philox runs for the quads
//   that hold a kept token only.  logprob stays the untempered, unfiltered log-softmax; kept[b] = how many tokens survived.
// Selection (pick_filtered - the body is pick_row of vmlmf_select.h, which libvmlmf_decode.so instantiates for its controlled scores -:
// one workgroup per row, ONE non-inlined device function that both filtered kernels call - 1024 threads in
// the choice launch, where a pass is a chain of round trips per thread, 256 in the fused launch, whose strips set the workgroup's
// size; the per-quad and per-token work is written as rolled loops: the library's size is held to a limit, tests/test_cabi.py).  One
// pass reads the row and parks the
// order-preserving 32-bit key of z in LDS (rows longer than SF_LDS_V re-read the scores instead).  A radix select from the most
// significant byte follows - four levels of a 256-bin histogram in LDS, 64-bit integer atomics - once over counts (the k-th key) and
// once over masses (the key at which the running mass reaches p).  Tokens whose key equals the threshold key are admitted in index
// order until the count or the mass is met.  A last pass does Gumbel-max over the kept tokens.  Everything is integer or fixed-order
// fp32: bit-identical from run to run.
// The fused form with filters: the strips write their scores (B x V floats) through to agent scope instead of the per-strip partials,
// and the last workgroup to arrive runs pick_filtered over them, a row after the other.  Same ticket, still nobody waits.  One
// workgroup's selection is what a token then waits for: measured slower than the GEMM + choice form at every width
// (docs/design/lm_sampling.md), so vmlmf_amd.lm_sample takes this form only where it is asked for.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vmlmf_hip.h"
#include "vmlmf_device.h"
#include "vmlmf_dropout.h"
#include "vmlmf_launch.h"
#include "vmlmf_select.h"

namespace {

constexpr int SM_NI = 41;        // MFMA steps per wave and chunk of H: a chunk is 4 waves x 4 x 41 = 656 >= 650 (the PTB LM)
constexpr int SM_MAXWG = 512;    // strips: the merge reads at most 8 partials per lane

typedef float f32x4s __attribute__((ext_vector_type(4)));

// row (V scores, + bias where given) -> the filtered choice (pick_row, vmlmf_select.h).  top_k in [0, V) (0: off), top_p in (0, 1]
// (1: off), inv_temp > 0.  (one copy in the library, called by both kernels: the scratch is the function's own LDS)
__device__ __attribute__((noinline, minsize)) RowPick pick_filtered(const float* row, const float* bias, int V, float inv_temp, int top_k, float top_p,
                                                            DropKey key, unsigned position) {
  __shared__ SelScratch S;
  return pick_row(S, PlainScores{row, bias}, V, inv_temp, top_k, top_p, key, position);
}

// a.scores != NULL (filters): the strips leave their scores instead of the partials and the last workgroup runs pick_filtered over
// them.  (One kernel for both, not two instantiations: the strips' code is most of it, and the library's size is held to a limit.)
__global__ __launch_bounds__(256) void lm_sample_kernel(LmSampleArgs a) {
  const bool FILT = a.scores != nullptr;
  __shared__ float red[4][256];
  __shared__ int last_flag;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
  const int tiles = (a.V + 15) >> 4;
  const int t0 = blockIdx.x * a.tpw, t1 = t0 + a.tpw < tiles ? t0 + a.tpw : tiles;
  const int bb = tid >> 4, vv = tid & 15;   // epilogue role: batch row bb of the pass, vocabulary row vv of the tile
  const bool GUMBEL = a.inv_temp > 0.f;
  const DropKey key = GUMBEL ? sample_key(a.state) : DropKey{0u, 0u, 0u, 0u};
  for (int b0 = 0; b0 < a.B; b0 += 16) {
    const bool bok = b0 + r < a.B;   // operand role: batch row b0 + r feeds the MFMA's column r
    const float* hp = a.h + (size_t)(bok ? b0 + r : 0) * a.H;
    float bz = -INFINITY, braw = 0.f, m = -INFINITY, s = 0.f;
    int bidx = SM_NOIDX;
    for (int t = t0; t < t1; ++t) {
      const int v0 = t << 4;
      const bool vok = v0 + r < a.V;
      const float* wp = a.w + (size_t)(vok ? v0 + r : 0) * a.H;
      f32x4s acc = {0.f, 0.f, 0.f, 0.f};
#ifdef VMLMF_SAMPLE_VALU_HEAD
      float vdot = 0.f;
      {
        const int v = v0 + vv, b = b0 + bb;
        const float* wr = a.w + (size_t)(v < a.V ? v : 0) * a.H;
        const float* hr = a.h + (size_t)(b < a.B ? b : 0) * a.H;
        float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
        int k = 0;
        for (; k + 3 < a.H; k += 4) d0 = fmaf(wr[k], hr[k], d0), d1 = fmaf(wr[k + 1], hr[k + 1], d1), d2 = fmaf(wr[k + 2], hr[k + 2], d2), d3 = fmaf(wr[k + 3], hr[k + 3], d3);
        for (; k < a.H; ++k) d0 = fmaf(wr[k], hr[k], d0);
        vdot = (d0 + d1) + (d2 + d3);
      }
      if (false)
#endif
      for (int kc = 0; kc < a.H; kc += 16 * SM_NI) {
        const int rem = (a.H - kc + 15) >> 4, nact = rem < SM_NI ? rem : SM_NI;
        float av[SM_NI], bv[SM_NI];
        // every load of the chunk in flight before the first MFMA: unconditional, clamped addresses (a load under a branch waited for
        // the one before it: 41 round trips a tile)
#pragma unroll
        for (int i = 0; i < SM_NI; ++i) {
          const int k = kc + 16 * i + 4 * wave + q;
          const bool in = k < a.H;
          const int kk = in ? k : 0;
          const float wv = wp[kk], hv = hp[kk];
          av[i] = (in && vok) ? wv : 0.f;
          bv[i] = (in && bok) ? hv : 0.f;
        }
#pragma unroll
        for (int i = 0; i < SM_NI; ++i)
          if (i < nact) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[i], acc, 0, 0, 0);
      }
      __syncthreads();   // the previous tile's epilogue has read `red`
#pragma unroll
      for (int i = 0; i < 4; ++i) red[wave][(4 * q + i) * 16 + r] = acc[i];   // lane (r, q), element i: vocabulary row 4 q + i, batch column r
      __syncthreads();
      const int v = v0 + vv, b = b0 + bb;
      if (v < a.V && b < a.B) {
        const int e = vv * 16 + bb;
#ifdef VMLMF_SAMPLE_VALU_HEAD
        const float sc = (a.bias != nullptr ? a.bias[v] : 0.f) + vdot;
#else
        const float sc = (a.bias != nullptr ? a.bias[v] : 0.f) + (((red[0][e] + red[1][e]) + red[2][e]) + red[3][e]);
#endif
        if (FILT) {
          st1g_agent((gf32*)(a.scores + (size_t)b * a.V + v), sc);
        } else {
          const float z = GUMBEL ? fmaf(sc, a.inv_temp, gumbel(key, (unsigned)a.step * (unsigned)a.B + (unsigned)b, v)) : sc;
          best_merge(bz, braw, bidx, z, sc, v);
          lse_merge(m, s, sc, 1.f);
        }
      }
    }
    if (!FILT) {
      // the 16 lanes of batch row bb (one 16-lane group): butterfly, every lane ends with the same bits
#pragma unroll
      for (int o = 8; o >= 1; o >>= 1) {
        const float z2 = __shfl_xor(bz, o, 64), r2 = __shfl_xor(braw, o, 64), m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        const int i2 = __shfl_xor(bidx, o, 64);
        best_merge(bz, braw, bidx, z2, r2, i2);
        lse_merge(m, s, m2, s2);
      }
      if (vv == 0 && b0 + bb < a.B) {
        float* p = a.part + ((size_t)blockIdx.x * a.B + b0 + bb) * 8;
        st4g_agent((gf32*)p, make_float4(bz, braw, __int_as_float(bidx), 0.f));
        st4g_agent((gf32*)(p + 4), make_float4(m, s, 0.f, 0.f));
      }
    }
  }
  // every strip's partials (filtered: scores) are out (written through to agent scope: visible on every XCD once vmcnt has counted them); then the ticket
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const unsigned long long t = __hip_atomic_fetch_add(a.ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last_flag = t == (unsigned long long)gridDim.x - 1ull;
  }
  __syncthreads();
  if (!last_flag) return;
  // last arrival: an agent-scope acquire in every wave (this CU's stale lines dropped), then plain 16-byte loads - all of a row's in
  // flight at once (one relaxed atomic load per word serialised them: 48 round trips a row).  A wave per batch row, lane l
  // merges strips l, l + 64, ... in order, then a 64-lane butterfly.
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (FILT) {
    for (int b = 0; b < a.B; ++b) {
      const RowPick pk = pick_filtered(a.scores + (size_t)b * a.V, nullptr, a.V, a.inv_temp, a.top_k, a.top_p, key,
                                       (unsigned)a.step * (unsigned)a.B + (unsigned)b);
      write_pick(pk, b, a.H, a.tokens, a.logprob, a.kept, a.x_next, a.embed);
    }
    if (tid == 0) __hip_atomic_store(a.ticket, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  const int G = gridDim.x;
  for (int b = wave; b < a.B; b += 4) {
    float4 p0[SM_MAXWG / 64], p1[SM_MAXWG / 64];
#pragma unroll
    for (int j = 0; j < SM_MAXWG / 64; ++j) {
      const int gi = lane + 64 * j;
      const float* p = a.part + ((size_t)(gi < G ? gi : 0) * a.B + b) * 8;
      p0[j] = ld4(p), p1[j] = ld4(p + 4);
    }
    float z = -INFINITY, raw = 0.f, mm = -INFINITY, ss = 0.f;
    int idx = SM_NOIDX;
#pragma unroll
    for (int j = 0; j < SM_MAXWG / 64; ++j) {
      if (lane + 64 * j < G) {
        best_merge(z, raw, idx, p0[j].x, p0[j].y, __float_as_int(p0[j].z));
        lse_merge(mm, ss, p1[j].x, p1[j].y);
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float z2 = __shfl_xor(z, o, 64), r2 = __shfl_xor(raw, o, 64), m2 = __shfl_xor(mm, o, 64), s2 = __shfl_xor(ss, o, 64);
      const int i2 = __shfl_xor(idx, o, 64);
      best_merge(z, raw, idx, z2, r2, i2);
      lse_merge(mm, ss, m2, s2);
    }
    const int tok = (idx >= 0 && idx < a.V) ? idx : 0;   // (every score NaN: token 0, NaN log-probability)
    if (lane == 0) {
      a.tokens[b] = tok;
      if (a.logprob != nullptr) a.logprob[b] = idx == tok ? raw - (mm + logf(ss)) : NAN;
    }
    if (a.x_next != nullptr) {
      const float* src = a.embed + (size_t)tok * a.H;
      float* dst = a.x_next + (size_t)b * a.H;
      for (int e = lane; e < a.H; e += 64) dst[e] = src[e];
    }
  }
  if (tid == 0) __hip_atomic_store(a.ticket, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the filtered choice over the (B, V) scores of a library GEMM: one workgroup of SF_CHOOSE_NT threads per row
constexpr int SF_CHOOSE_NT = 1024;
__global__ __launch_bounds__(SF_CHOOSE_NT) void lm_choose_filtered_kernel(LmChooseArgs a) {
  const int b = blockIdx.x;
  const RowPick pk = pick_filtered(a.scores + (size_t)b * a.V, a.bias, a.V, a.inv_temp, a.top_k, a.top_p, sample_key(a.state),
                                   (unsigned)a.step * (unsigned)a.B + (unsigned)b);
  write_pick(pk, b, a.H, a.tokens, a.logprob, a.kept, a.x_next, a.embed);
}

// ---- the same choice over a (B, V) score matrix a library GEMM produced: the form for batches wider than one 16-row tile ----
// One workgroup per row; a thread takes four neighbouring vocabulary rows at a time, so one Philox call serves them all.  The row is
// read once; per-thread (best, max, sum of exp) partials meet in a fixed tree (64-lane butterfly, then the four waves in order).
__global__ __launch_bounds__(SM_CHOOSE_NT) void lm_choose_kernel(LmChooseArgs a) {
  __shared__ float red[4][5];
  const int b = blockIdx.x;
  const bool GUMBEL = a.inv_temp > 0.f;
  const DropKey key = GUMBEL ? sample_key(a.state) : DropKey{0u, 0u, 0u, 0u};
  const RowPick pk = choose_row(&red[0][0], 5, PlainScores{a.scores + (size_t)b * a.V, a.bias}, a.V, a.inv_temp, GUMBEL, key,
                                (unsigned)a.step * (unsigned)a.B + (unsigned)b);
  // (write_pick with this workgroup's constant stride and no counts: through write_pick itself the launch measured 0.1 us slower)
  const int tid = threadIdx.x, tok = pk.idx != SM_NOIDX ? pk.idx : 0;
  if (tid == 0) {
    a.tokens[b] = tok;
    if (a.logprob != nullptr) a.logprob[b] = pk.idx == tok ? pk.raw - (pk.m + logf(pk.s)) : NAN;
  }
  if (a.x_next != nullptr) {
    const float* src = a.embed + (size_t)tok * a.H;
    for (int e = tid; e < a.H; e += SM_CHOOSE_NT) a.x_next[(size_t)b * a.H + e] = src[e];
  }
}

int sample_strips(int V, int* tpw) {
  const int tiles = (V + 15) / 16;
  const int per = (tiles + SM_MAXWG - 1) / SM_MAXWG;
  if (tpw != nullptr) *tpw = per;
  return (tiles + per - 1) / per;
}

}  // namespace

size_t lm_sample_workspace_bytes(int B, int V) {
  const int tiles = (V + 15) / 16;
  return (size_t)(tiles < SM_MAXWG ? tiles : SM_MAXWG) * (size_t)B * 8 * sizeof(float);
}
// the unfiltered launch's partials (filters off: that launch runs on this workspace), then the (B, V) scores
size_t lm_sample_filtered_workspace_bytes(int B, int V) { return lm_sample_workspace_bytes(B, V) + (size_t)B * (size_t)V * sizeof(float); }

// a.top_k in [0, V) (0: off), a.top_p in (0, 1] (1: off); with either on (and sampling) the filtered kernel runs, a.kept takes its counts
static bool filters_on(float inv_temp, int top_k, float top_p) { return inv_temp > 0.f && (top_k > 0 || top_p < 1.f); }

int launch_lm_sample(LmSampleArgs a, hipStream_t s) {
  const int G = sample_strips(a.V, &a.tpw);
  if (filters_on(a.inv_temp, a.top_k, a.top_p))
    a.scores = a.part + lm_sample_workspace_bytes(a.B, a.V) / sizeof(float);
  else
    a.scores = nullptr;
  hipLaunchKernelGGL(lm_sample_kernel, dim3(G), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

int launch_lm_choose(const LmChooseArgs& a, hipStream_t s) {
  if (filters_on(a.inv_temp, a.top_k, a.top_p)) hipLaunchKernelGGL(lm_choose_filtered_kernel, dim3(a.B), dim3(SF_CHOOSE_NT), 0, s, a);
  else hipLaunchKernelGGL(lm_choose_kernel, dim3(a.B), dim3(SM_CHOOSE_NT), 0, s, a);
  return (int)hipGetLastError();
}
