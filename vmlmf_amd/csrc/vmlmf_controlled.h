// The controlled rows of the LM decoder, written once for vmlmf_decode.hip (libvmlmf_decode.so: vmlmf_decode_choose) and
// vmlmf_truncate.hip (libvmlmf_truncate.so: vmlmf_truncate_choose): how a row's controlled score is formed from its raw score
// (include/vmlmf_decode.h, steps 1 - 3), what a finished row writes, and how a live row's state moves behind its choice (step 6).
// Device code only; the selection itself is vmlmf_select.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "vmlmf_select.h"

// x -> c of one row (steps 1 - 3 of the contract)
struct ControlledScores {
  static constexpr bool CONTROLLED = true;
  struct Ctl {
    float lb;
    unsigned char seen;
  };
  const float *row, *bias, *logit_bias;
  const unsigned char* seen;
  float theta;
  int eos_ban;   // eos while the row is below its minimum length, else -1
  __device__ __forceinline__ float raw(int v) const { return (bias != nullptr ? bias[v] : 0.f) + row[v]; }
  __device__ __forceinline__ Ctl ctl(int v) const { return Ctl{logit_bias != nullptr ? logit_bias[v] : 0.f, seen[v]}; }
  __device__ __forceinline__ float score(int v, float x, const Ctl& ct) const {
    // (explicitly rounded operations: no contraction, so every pass of a long row forms the same bits)
    const float r = ct.seen != 0 ? (x > 0.f ? __fdiv_rn(x, theta) : __fmul_rn(x, theta)) : x;
    return v == eos_ban ? -INFINITY : __fadd_rn(r, ct.lb);
  }
};

// the rows' state and what the choice of a controlled row writes (the pointers of vmlmf_decode_controls and of the entry point)
struct ControlledRows {
  const float *scores, *bias, *embed, *logit_bias;
  long long* tokens;
  float *logprob, *x_next;
  int* kept;
  unsigned char* seen;
  int *finished, *length;
  float theta;
  int H, V, eos, min_length;
  // row b's scores as the selection reads them
  __device__ __forceinline__ ControlledScores source(int b) const {
    ControlledScores src;
    src.row = scores + (size_t)b * V, src.bias = bias, src.logit_bias = logit_bias, src.seen = seen + (size_t)b * V, src.theta = theta;
    src.eos_ban = (eos >= 0 && length[b] < min_length) ? eos : -1;
    return src;
  }
  // (uniform over the workgroup) a finished row: its padding is written, nothing of its state moves; false: the row is live
  __device__ __forceinline__ bool padding(int b) const {
    if (!(eos >= 0 && finished[b] != 0)) return false;
    if (threadIdx.x == 0) {
      tokens[b] = eos;
      if (logprob != nullptr) logprob[b] = 0.f;
      if (kept != nullptr) kept[b] = 0;
    }
    if (x_next != nullptr) {
      const float* src = embed + (size_t)eos * H;
      for (int e = threadIdx.x; e < H; e += blockDim.x) x_next[(size_t)b * H + e] = src[e];
    }
    return true;
  }
  // a live row's outputs, then - by thread 0, behind a workgroup barrier that every read of the row's state precedes - its state
  __device__ __forceinline__ void finish(const RowPick& pk, int b) const {
    write_pick(pk, b, H, tokens, logprob, kept, x_next, embed);
    __syncthreads();   // every thread has read what it needs of seen and length
    if (threadIdx.x == 0) {
      const int tok = pk.idx != SM_NOIDX ? pk.idx : 0;
      seen[(size_t)b * V + tok] = 1;
      length[b] += 1;
      if (tok == eos) finished[b] = 1;
    }
  }
};
