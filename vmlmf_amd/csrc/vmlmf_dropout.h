// Dropout of the LM network (V/src/models/vmlmf_lm.py:434-439: `x = self.dropout(x)` behind the embedding and behind every LSTM
// layer, nn.Dropout(p) of :402) without mask tensors and, on the layer kernels that take it, without launches of its own (verdict
// r4 item 3): the keep / drop decision of an element is a pure function of (seed, offset, site, position, column) - Philox4x32-10
// (Salmon et al., SC'11; the counter-based generator the stock op uses too), one call per four neighbouring columns - so the
// forward kernel that stores an activation writes its dropped copy beside it, and the backward kernel that reads the upstream
// gradient of that copy regenerates the same bits.
//   counter = (position, column >> 2, site, offset low word), key = (seed low word, seed high word + offset high word)
//   element (position, column) is DROPPED iff word[column & 3] < thresh, thresh = round(p 2^32); kept values are scaled by 1/(1-p)
//   position = t B + b (the row of the flattened (T, B) grid), site = 0 for the embedding's output, l + 1 for layer l's
//              locked (variational) dropout, DropArgs::period == B > 0: position = b for every time step - ONE mask per forward
//              pass, shared by every t (docs/design/lm_locked.md); drop_position below is the one place that says so.  Its site
//              word carries VMLMF_SITE_LOCKED, so a site's locked stream is not its per-element stream
//   column   = the hidden unit, or - inside the row-block kernels - the unit's thread slot (vmlmf_geo.h: group g's units start at
//              slot 64 W g, a multiple of four, so the four units a lane owns are one call; DropCols below is that map)
// (seed, offset) live in device memory: a captured graph replays with fresh masks because vmlmf_dropout_advance - a node of the
// same graph - snapshots the pair and increments the offset.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct DropArgs {
  const unsigned long long* state;   // {seed, offset} snapshot of this forward; nullptr: no dropout
  float* yd;                         // forward of a layer: the dropped copy of y (same layout)
  unsigned thresh;                   // dropped iff word < thresh
  float scale;                       // 1 / (1 - p)
  int site, period;                  // period: 0 per-element factors, B > 0 locked ones (drop_position)
};
// hidden unit -> column of the counter: (n / Hg) * gstride + n % Hg; identity: Hg = H, gstride = 0
struct DropCols {
  int Hg, gstride;
};

struct DropKey {
  unsigned k0, k1, c2, c3;
};
__device__ __forceinline__ DropKey drop_key(const DropArgs& d) {
  const unsigned long long seed = d.state[0], off = d.state[1];
  DropKey k;
  k.k0 = (unsigned)seed, k.k1 = (unsigned)(seed >> 32) + (unsigned)(off >> 32), k.c2 = (unsigned)d.site, k.c3 = (unsigned)off;
  return k;
}
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1, c3 = (unsigned)p0, c0 = n0, c2 = n2;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}
// the four factors (0 or scale) of columns 4 quad .. 4 quad + 3 at `position`
__device__ __forceinline__ void drop_factors(const DropKey& k, const unsigned thresh, const float scale, const unsigned position, const unsigned quad,
                                             float (&f)[4]) {
  unsigned w[4];
  philox4x32_10(position, quad, k.c2, k.c3, k.k0, k.k1, w);
#pragma unroll
  for (int i = 0; i < 4; ++i) f[i] = w[i] < thresh ? 0.f : scale;
}

// The counter's position word, for every caller of drop_factors: the row t B + b of the flattened (T, B) grid per element (period ==
// 0: the bits of every release before `period` existed), the batch row b alone under a locked mask (period == B).  The recurrent
// kernels know (t, b); the flat-row kernels know r = t B + b.
// A kernel that walks time steps forms t's stride once, in front of its loop (B, or 0 under a locked mask), so a step's position
// costs what it cost before there was a period.
__device__ __forceinline__ int drop_tstride(const int period, const int B) { return period != 0 ? 0 : B; }
__device__ __forceinline__ unsigned drop_position(const int tstride, const int t, const int b) {
  return (unsigned)t * (unsigned)tstride + (unsigned)b;   // (unsigned: the host admits T B up to 2^32 positions)
}
__device__ __forceinline__ unsigned drop_position(const int period, const unsigned r) { return period != 0 ? r % (unsigned)period : r; }

// four neighbouring columns of a row: one 16-byte access where the address allows it, two 8-byte ones where it is 8 bytes off (H =
// 650: every second position), by element for a row's tail or an odd width; columns behind the row read as zero
__device__ __forceinline__ void load_quad(const float* __restrict__ p, const int valid, float (&v)[4]) {
  const uintptr_t at = reinterpret_cast<uintptr_t>(p);
  if (valid == 4 && (at & 15) == 0) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else if (valid == 4 && (at & 7) == 0) {
    const float2 lo = *reinterpret_cast<const float2*>(p), hi = *reinterpret_cast<const float2*>(p + 2);
    v[0] = lo.x, v[1] = lo.y, v[2] = hi.x, v[3] = hi.y;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = e < valid ? p[e] : 0.f;
  }
}
__device__ __forceinline__ void store_quad(float* __restrict__ p, const int valid, const float (&v)[4]) {
  const uintptr_t at = reinterpret_cast<uintptr_t>(p);
  if (valid == 4 && (at & 15) == 0) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else if (valid == 4 && (at & 7) == 0) {
    *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
    *reinterpret_cast<float2*>(p + 2) = make_float2(v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < valid) p[e] = v[e];
  }
}

// Word (embedding-row) dropout of the tied / AWD-LSTM table (docs/design/lm_tied.md): ONE factor per vocabulary row v, shared by
// every position that holds the word - word 0 of the call with counter (v, 0, DROP_SITE_WORD, offset low word) under the forward's
// key; 0 iff word < thresh, else scale.  Kept out of line: its callers hold a generator call of their own already, and the library
// is held to a size.
constexpr unsigned DROP_SITE_WORD = 0x574F5244u;   // "WORD" (include/vmlmf_hip.h: VMLMF_SITE_WORD)
static __device__ __noinline__ float word_factor(const unsigned long long* state, const unsigned thresh, const float scale, const unsigned v) {
  const unsigned long long seed = state[0], off = state[1];
  unsigned w[4];
  philox4x32_10(v, 0u, DROP_SITE_WORD, (unsigned)off, (unsigned)seed, (unsigned)(seed >> 32) + (unsigned)(off >> 32), w);
  return w[0] < thresh ? 0.f : scale;
}
// what the _ex embedding entries take beside the element dropout's DropArgs (d.state is also the word factors' state)
struct WordDrop {
  unsigned thresh;   // the word is dropped iff its generator word < thresh
  float scale;       // 1 / (1 - word_p)
  int drop, word;    // element dropout on (p > 0) / word dropout on (word_p > 0): uniform branches of one kernel
};

// host side of DropArgs: p in [0, 1)
inline unsigned drop_thresh(float p) {
  const double t = (double)p * 4294967296.0 + 0.5;
  return t >= 4294967295.0 ? 4294967295u : (unsigned)t;
}
