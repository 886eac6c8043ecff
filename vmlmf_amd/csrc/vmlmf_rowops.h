// Device helpers of the kernels that hold a row of scores in a 256-thread workgroup's registers (vmlmf_nll.hip, vmlmf_head_loss.hip)
// and the wave reductions vmlmf_head.hip and vmlmf_contrast.hip share with them.  Plain HIP C++ for wave64; every order of summation
// is fixed.  (vmlmf_rec_fwd.inc's DPP reductions and vmlmf_pack.hip's half_wave_sum are other instruction sequences and live there.)
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// workgroup-wide reduction of N values per thread (256 threads) in ONE exchange, results broadcast; `red` has 4 * N floats
template <int N, bool MAX>
__device__ __forceinline__ void block_reduce(float (&v)[N], float* red) {
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = MAX ? wave_max(v[n]) : wave_sum(v[n]);
  __syncthreads();   // red may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int n = 0; n < N; ++n) red[4 * n + (threadIdx.x >> 6)] = v[n];
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < N; ++n) {
    const float* r = red + 4 * n;
    v[n] = MAX ? fmaxf(fmaxf(r[0], r[1]), fmaxf(r[2], r[3])) : (r[0] + r[1]) + (r[2] + r[3]);
  }
}
// ... of one value: N = 1
template <bool MAX>
__device__ __forceinline__ float block_reduce(float v, float* red) {
  float a[1] = {v};
  block_reduce<1, MAX>(a, red);
  return a[0];
}

__device__ __forceinline__ float4 f4(float a) { return make_float4(a, a, a, a); }
__device__ __forceinline__ float pick(const float4& v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }
// A row as a buffer: one descriptor per row in scalar registers, a lane's slot at the 32-bit byte offset 16 (tid + 256 i).  The
// hardware's range check takes the place of index clamps and of 64-bit addresses per slot (48 VGPRs of loop invariants with plain
// pointers): a load past the row's `bytes` returns zeros, a store there is dropped (the stores are predicated all the same).
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_buffer(const float* row, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(row), 0, bytes, 0x00020000);
}
__device__ __forceinline__ float4 load4(__amdgpu_buffer_rsrc_t r, int off) {
  const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
  return make_float4(__uint_as_float(w.x), __uint_as_float(w.y), __uint_as_float(w.z), __uint_as_float(w.w));
}
__device__ __forceinline__ void store4(__amdgpu_buffer_rsrc_t r, int off, const float4& v) {
  const u32x4 w = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
  __builtin_amdgcn_raw_buffer_store_b128(w, r, off, 0, 0);
}
// A lane's index behind a compiler barrier: what a phase of the row loop derives from it (slot offsets, column numbers) is formed
// in that phase again, not carried through the loop as a dozen and more invariant registers per use.
__device__ __forceinline__ int fresh(int v) {
  asm volatile("" : "+v"(v));
  return v;
}
