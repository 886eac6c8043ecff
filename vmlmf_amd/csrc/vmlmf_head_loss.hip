// The LM head's losses in their training form: loss AND the gradient of the (R, V) score matrix in ONE pass over it, in place - the
// softmax negative log-likelihood of vmlmf_nll.hip (vmlmf_nll_forward_grad, ABI 9) and knowledge distillation (Hinton, Vinyals, Dean:
// "Distilling the Knowledge in a Neural Network"; vmlmf_distill_forward_grad), which adds tau^2 KL(P || Q) against a teacher's
// distribution P.  Per row r, z = scores + bias, Q = softmax(z / tau):
//   hard = logsumexp(z) - z[y]                                soft = tau^2 sum_v P[v] (log P[v] - log Q[v])
//   dz   = scale ((1 - alpha)(softmax(z) - onehot(y)) + alpha tau (Q - P))
// The LM head's backward needs dz and the bias gradient (its column sums); the two-kernel form of vmlmf_nll.hip reads the scores twice,
// writes a second 358 MB matrix and leaves the column sums to a third pass.  Here a 256-thread workgroup walks rows w, w + NWG, ...:
// a row (plus the bias, which the GEMM in front then need not add) lives in its registers as twelve float4 slots between max, sum and
// target pick, every load unconditional, is written back IN PLACE as its own gradient (for d(loss) = 1; the caller scales
// otherwise), and every thread keeps the column sums of the columns it owns over all its rows for the bias gradient.  One read + one
// write of the matrix; NWG x V column partials (fixed-order sum in head_loss_finish_kernel).  No atomics, fixed summation orders: the
// same bits from run to run.  Three bodies of that one walk, one finish and one launch tail:
//   nll_grad_kernel           the NLL alone: plain pointers, the bias held in registers (a teacher-less source of the body below was
//                             measured at 1.3 x its time: docs/design/head_loss_optim_lm.md)
//   distill_grad_kernel<SRC>  with a teacher SOURCE: DenseTeacher, an (R, V) score matrix, P = softmax(t / tau), or TopTeacher, the
//                             row's k <= 32 top tokens and their scores, P = softmax over those k and zero elsewhere
//   objective_grad_kernel     a padding mask, label smoothing, z-loss and unlikelihood against a set of negatives (its own block
//                             comment below; vmlmf_objective_forward_grad, docs/design/lm_objective.md)
// With a teacher everything is formed around the row maxima m_z and m_t: with x = z - m_z, u = t - m_t and the four sums
//   s1 = sum exp(x)    sq = sum exp(x / tau)    st = sum exp(u / tau)    d = sum exp(u / tau) (u - x)
// hard = log s1 - x[y] and soft = tau^2 (d / (tau st) - log st + log sq); at tau == 1 (a uniform branch) sq is s1 and the row's
// second exponential is skipped.  The slots hold first x, then the numerators exp(x) and exp(x / tau) side by side, so every
// exponential is taken once; two block reductions per row (the two maxima; the four sums).  The teacher's row lies in one V-wide
// row of LDS, each lane reading and writing its own slots only:
//   dense:  the teacher's scores, loaded through registers; the sum pass replaces them by the numerators exp(u / tau)
//   top-k:  zeros but at the row's k columns, where lanes j < k scatter exp(u_j / tau) behind the maxima and clear it behind the
//           write pass (a barrier each) - a column's owner reads P like a dense operand and the k entries need no search
// so the write pass is the same for both.  There the bias is read again with every row (V floats that stay in the cache): student
// numerators (2 x 48) + column sums (48) already are 144 VGPRs, and the LDS row is taken; rows are buffers (vmlmf_rowops.h).
// Register, LDS and occupancy numbers: docs/design/lm_distill.md.
#include <hip/hip_runtime.h>

#include "vmlmf_launch.h"
#include "vmlmf_rowops.h"

namespace {

constexpr int DQ = 12;   // float4 per thread: rows up to 256 * 12 * 4 = 12288 wide

// ---- the NLL alone ---------------------------------------------------------------------------------------------------------------
constexpr int NLL_GQ = DQ;   // (192 VGPRs of row + bias + column sums)
__global__ __launch_bounds__(256, 2) void nll_grad_kernel(int R, int V, float scale, float* __restrict__ scores,
                                                          const float* __restrict__ bias, const long long* __restrict__ y,
                                                          float* __restrict__ rowloss, float* __restrict__ dbpart) {
  __shared__ float red[4];
  const int tid = threadIdx.x, nq = V >> 2;
  float4 bv[NLL_GQ], cs[NLL_GQ];
#pragma unroll
  for (int i = 0; i < NLL_GQ; ++i) {
    const int q = tid + 256 * i;
    const float4 t = bias != nullptr ? reinterpret_cast<const float4*>(bias)[q < nq ? q : 0] : make_float4(0.f, 0.f, 0.f, 0.f);
    bv[i] = q < nq ? t : make_float4(0.f, 0.f, 0.f, 0.f);
    cs[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (int row = blockIdx.x; row < R; row += gridDim.x) {
    float* z = scores + (size_t)row * V;
    float4 v[NLL_GQ];
#pragma unroll
    for (int i = 0; i < NLL_GQ; ++i) {   // clamped index: every load unconditional
      const int q = tid + 256 * i;
      v[i] = reinterpret_cast<const float4*>(z)[q < nq ? q : 0];
    }
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < NLL_GQ; ++i) {
      const int q = tid + 256 * i;
      v[i].x += bv[i].x, v[i].y += bv[i].y, v[i].z += bv[i].z, v[i].w += bv[i].w;
      if (q >= nq) v[i] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      m = fmaxf(m, fmaxf(fmaxf(v[i].x, v[i].y), fmaxf(v[i].z, v[i].w)));
    }
    m = block_reduce<true>(m, red);
    const long long t = y[row];
    const bool inr = t >= 0 && t < V;
    const int tc = inr ? (int)t : -1;
    float s = 0.f, ztm = 0.f;   // ztm: (target's score - m), held by the thread that owns the target's column
#pragma unroll
    for (int i = 0; i < NLL_GQ; ++i) {   // keep the exponentials: they are the softmax numerators
      const int q = tid + 256 * i;
      if ((tc >> 2) == q) ztm = ((tc & 3) == 0 ? v[i].x : (tc & 3) == 1 ? v[i].y : (tc & 3) == 2 ? v[i].z : v[i].w) - m;
      v[i].x = __expf(v[i].x - m), v[i].y = __expf(v[i].y - m), v[i].z = __expf(v[i].z - m), v[i].w = __expf(v[i].w - m);
      s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
    s = block_reduce<false>(s, red);
    const float inv = scale / s;
#pragma unroll
    for (int i = 0; i < NLL_GQ; ++i) {
      const int q = tid + 256 * i;
      if (q < nq) {
        if ((tc >> 2) == q) rowloss[row] = __logf(s) - ztm;   // lse - z_t
        float4 o;
        o.x = v[i].x * inv - (4 * q + 0 == tc ? scale : 0.f);
        o.y = v[i].y * inv - (4 * q + 1 == tc ? scale : 0.f);
        o.z = v[i].z * inv - (4 * q + 2 == tc ? scale : 0.f);
        o.w = v[i].w * inv - (4 * q + 3 == tc ? scale : 0.f);
        reinterpret_cast<float4*>(z)[q] = o;
        cs[i].x += o.x, cs[i].y += o.y, cs[i].z += o.z, cs[i].w += o.w;
      }
    }
    if (!inr && tid == 0) rowloss[row] = NAN;   // a target outside [0, V): NaN loss (the reference's indexing raises)
  }
#pragma unroll
  for (int i = 0; i < NLL_GQ; ++i) {
    const int q = tid + 256 * i;
    if (q < nq) reinterpret_cast<float4*>(dbpart + (size_t)blockIdx.x * V)[q] = cs[i];
  }
}

// ---- the teacher sources -------------------------------------------------------------------------------------------------------
// What differs between them in the body: how the teacher's row gets into LDS (`aux`), its maximum (a per-thread partial, folded
// into the reduction of the student's maximum), and who forms the sums st and d.
struct DenseTeacher {   // (R, V) scores
  static constexpr bool DENSE = true;
  const float* teacher;
};
struct TopTeacher {     // (R, k) tokens and scores
  static constexpr bool DENSE = false;
  const long long* tokens;
  const float* scores;
  int k;
};

template <class SRC>
__global__ __launch_bounds__(256, 2) void distill_grad_kernel(int R, int V, float scale, float alpha, float tau, float* __restrict__ scores,
                                                              const float* __restrict__ bias, const long long* __restrict__ y, SRC src,
                                                              float* __restrict__ rowloss, float* __restrict__ dbpart) {
  __shared__ float4 aux[256 * DQ];   // the teacher's row - dense: its scores; top-k: its numerators at the k columns, zero elsewhere
  __shared__ float red[16];
  const int tid = threadIdx.x, nq = V >> 2;
  const float it = 1.f / tau;
  const bool unit = tau == 1.f;      // Q is the hard softmax: one exponential per score
  const float c1 = scale * (1.f - alpha), c2 = scale * alpha * tau;
  const __amdgpu_buffer_rsrc_t bias_row = row_buffer(bias, bias != nullptr ? 4 * V : 0);   // no bias: no records, zeros
  float4 cs[DQ];
#pragma unroll
  for (int i = 0; i < DQ; ++i) {
    aux[tid + 256 * i] = f4(0.f);
    cs[i] = f4(0.f);
  }
  __syncthreads();
  for (int row = blockIdx.x; row < R; row += gridDim.x) {
    const __amdgpu_buffer_rsrc_t z = row_buffer(scores + (size_t)row * V, 4 * V);
    float4 v[DQ];
    float mx[2] = {-INFINITY, -INFINITY};   // of the student's row, of the teacher's
    long long tok = -1;                     // top-k: lane j < k holds the row's j-th token and score
    float tsc = -INFINITY;
    {
      const int tl = fresh(tid);
#pragma unroll
      for (int i = 0; i < DQ; ++i) v[i] = load4(z, 16 * (tl + 256 * i));   // every load unconditional
      if constexpr (SRC::DENSE) {           // the teacher's row through registers into LDS, a lane's slots its own: no barrier
        const __amdgpu_buffer_rsrc_t trow = row_buffer(src.teacher + (size_t)row * V, 4 * V);
        float4 u[DQ];
#pragma unroll
        for (int i = 0; i < DQ; ++i) u[i] = load4(trow, 16 * (tl + 256 * i));
#pragma unroll
        for (int i = 0; i < DQ; ++i) {
          const int q = tl + 256 * i;
          if (q < nq) mx[1] = fmaxf(mx[1], fmaxf(fmaxf(u[i].x, u[i].y), fmaxf(u[i].z, u[i].w)));
          aux[q] = u[i];
        }
      } else {
        const int j = tid < src.k ? tid : 0;
        const long long a = src.tokens[(size_t)row * src.k + j];
        const float s = src.scores[(size_t)row * src.k + j];
        if (tid < src.k) tok = a, tsc = s;
        mx[1] = tsc;
      }
#pragma unroll
      for (int i = 0; i < DQ; ++i) {        // the bias: the same V floats for every row, from the cache
        const int q = tl + 256 * i;
        const float4 b = load4(bias_row, 16 * q);
        v[i].x += b.x, v[i].y += b.y, v[i].z += b.z, v[i].w += b.w;
        if (q >= nq) v[i] = f4(-INFINITY);
        mx[0] = fmaxf(mx[0], fmaxf(fmaxf(v[i].x, v[i].y), fmaxf(v[i].z, v[i].w)));
      }
    }
    block_reduce<2, true>(mx, red);
    const float mz = mx[0], mt = mx[1];
    float sm[4] = {0.f, 0.f, 0.f, 0.f};   // s1, sq, st, d
    if constexpr (!SRC::DENSE) {          // lane j: its numerator into the LDS row; st and the teacher's half of d
      if (tid < src.k) {
        const float u = tsc - mt, et = __expf(u * it);
        sm[2] = et, sm[3] = et * u;
        if (tok >= 0 && tok < V) reinterpret_cast<float*>(aux)[tok] = et;
      }
      __syncthreads();
    }
    const long long t = y[row];
    const bool inr = t >= 0 && t < V;
    const int tc = inr ? (int)t : -1;     // the target's column: float4 (tc >> 2) is slot (tc >> 10) of lane (tc >> 2) & 255
    const bool own = inr && ((tc >> 2) & 255) == tid;
    float xt = 0.f;                       // x of the target, held by the thread that owns the target's column
    float4 w[DQ];                         // Q's numerators exp(x / tau); v becomes the hard softmax's, exp(x)
    {
      const int ts = fresh(tid);
#pragma unroll
      for (int i = 0; i < DQ; ++i) {
        const int q = ts + 256 * i;
        v[i].x -= mz, v[i].y -= mz, v[i].z -= mz, v[i].w -= mz;   // x; -inf in the padding
        if (own && (tc >> 10) == i) xt = pick(v[i], tc & 3);
        if (q < nq) {                     // (the padding: 0 * (inf - inf))
          const float4 a = aux[q];
          if constexpr (SRC::DENSE) {     // the teacher's numerators take its scores' place in LDS
            const float4 u = make_float4(a.x - mt, a.y - mt, a.z - mt, a.w - mt);
            const float4 e = make_float4(__expf(u.x * it), __expf(u.y * it), __expf(u.z * it), __expf(u.w * it));
            sm[2] += (e.x + e.y) + (e.z + e.w);
            sm[3] += (e.x * (u.x - v[i].x) + e.y * (u.y - v[i].y)) + (e.z * (u.z - v[i].z) + e.w * (u.w - v[i].w));
            aux[q] = e;
          } else {                        // zero but at the teacher's columns: the student's half of d
            sm[3] -= (a.x * v[i].x + a.y * v[i].y) + (a.z * v[i].z + a.w * v[i].w);
          }
        }
        if (!unit) {
          w[i] = make_float4(__expf(v[i].x * it), __expf(v[i].y * it), __expf(v[i].z * it), __expf(v[i].w * it));
          sm[1] += (w[i].x + w[i].y) + (w[i].z + w[i].w);
        }
        v[i] = make_float4(__expf(v[i].x), __expf(v[i].y), __expf(v[i].z), __expf(v[i].w));
        sm[0] += (v[i].x + v[i].y) + (v[i].z + v[i].w);
      }
    }
    block_reduce<4, false>(sm, red);
    const float s1 = sm[0], sq = unit ? sm[0] : sm[1], st = sm[2], d = sm[3];
    const float k1 = unit ? (c1 + c2) / s1 : c1 / s1, k2 = unit ? 0.f : c2 / sq, kt = c2 / st;
    {                                     // the gradient: the student's two shares minus the teacher's and the target's
      const int tw = fresh(tid);
#pragma unroll
      for (int i = 0; i < DQ; ++i) {
        const int q = tw + 256 * i, dc = tc - 4 * q;   // dc: the target's column within this float4, if it is in 0 .. 3
        if (q < nq) {
          const float4 p = aux[q];        // the teacher's numerators
          if (unit) w[i] = f4(0.f);
          float4 o;
          o.x = v[i].x * k1 + w[i].x * k2 - (p.x * kt + (dc == 0 ? c1 : 0.f));
          o.y = v[i].y * k1 + w[i].y * k2 - (p.y * kt + (dc == 1 ? c1 : 0.f));
          o.z = v[i].z * k1 + w[i].z * k2 - (p.z * kt + (dc == 2 ? c1 : 0.f));
          o.w = v[i].w * k1 + w[i].w * k2 - (p.w * kt + (dc == 3 ? c1 : 0.f));
          store4(z, 16 * q, o);
          cs[i].x += o.x, cs[i].y += o.y, cs[i].z += o.z, cs[i].w += o.w;
        }
      }
    }
    if (own) rowloss[row] = __logf(s1) - xt;   // lse - z_t
    if (tid == 0) {
      if (!inr) rowloss[row] = NAN;       // a target outside [0, V): NaN loss, as in nll_grad_kernel
      rowloss[(size_t)R + row] = tau * tau * (d * it / st - __logf(st) + __logf(sq));
    }
    if constexpr (!SRC::DENSE) {          // the LDS row back to zeros, behind the last read of it
      __syncthreads();
      if (tid < src.k && tok >= 0 && tok < V) reinterpret_cast<float*>(aux)[tok] = 0.f;
    }
  }
  const __amdgpu_buffer_rsrc_t part = row_buffer(dbpart + (size_t)blockIdx.x * V, 4 * V);
#pragma unroll
  for (int i = 0; i < DQ; ++i) {
    if (tid + 256 * i < nq) store4(part, 16 * (tid + 256 * i), cs[i]);
  }
}

// ---- the general objective: mask, label smoothing, z-loss, unlikelihood (docs/design/lm_objective.md) ------------------------------
// The third body of the walk.  With p = softmax(z), lse = logsumexp(z), x = z - max and s = sum exp(x), per row
//   nll = log s - x[y]     sm = log s - mean x     zl = lse^2     ul = sum over the row's negative SET of -log(max(1 - p, 1e-5))
//   dz  = sc (p (1 + 2 zeta lse - alpha S) - (1 - eps)[v == y] - eps / V + alpha w),  w = p / (1 - p) on the set where 1 - p > 1e-5
// ONE instantiation, the terms behind uniform branches: with eps = zeta = alpha = 0 and no masked row every value is formed by
// nll_grad_kernel's operations in its order (the same bits).  A row whose target is -1 is masked: zeros are stored over it, no
// arithmetic.  The negative set is a bitmap of V bits in LDS: lane j < k sets the bit of the row's j-th negative (an integer OR: the
// same bits in any order) between the row's first two reductions, whose barriers publish it; a column's owner tests its quad's four
// bits and ignores the target's; the same lanes clear their words behind the write pass.
constexpr float UL_FLOOR = 1e-5f;   // torch.clamp(1 - p, min=1e-5) of the paper's code: constant below it, no gradient
__device__ __forceinline__ unsigned quad_bits(const unsigned* bits, int q, bool own_slot, int tc) {
  const unsigned nib = (bits[q >> 3] >> (4 * (q & 7))) & 15u;
  return own_slot ? nib & ~(1u << (tc & 3)) : nib;
}
// w = p / (1 - p) of a negative (0 under the floor); its -log(max(1 - p, floor)) is added to ul.  The hardware reciprocal (1 ulp),
// not a division: a lane forms this for up to 48 columns in two passes per row (the division's expansion: 206 -> 197 us at 8960 rows
// of 10 000 with 35 negatives, docs/design/lm_objective.md).
__device__ __forceinline__ float ul_weight(float p, float& ul) {
  const float om = 1.f - p;
  ul -= __logf(fmaxf(om, UL_FLOOR));
  return om > UL_FLOOR ? p * __builtin_amdgcn_rcpf(om) : 0.f;
}

__global__ __launch_bounds__(256, 2) void objective_grad_kernel(int R, int V, float scale, ObjectiveArgs o, float* __restrict__ scores,
                                                                const float* __restrict__ bias, const long long* __restrict__ y,
                                                                float* __restrict__ rowloss, float* __restrict__ dbpart) {
  __shared__ unsigned bits[(256 * DQ * 4) / 32];   // the row's negative set, one bit per column
  __shared__ float red[8];
  const int tid = threadIdx.x, nq = V >> 2;
  const float sc = o.scale_dev != nullptr ? scale * *o.scale_dev : scale;
  const bool smooth = o.eps > 0.f, unlike = o.alpha > 0.f;
  const float ct = sc * (1.f - o.eps), ce = sc * o.eps / (float)V, ca = sc * o.alpha;
  const __amdgpu_buffer_rsrc_t bias_row = row_buffer(bias, bias != nullptr ? 4 * V : 0);   // no bias: no records, zeros
  float4 bv[DQ], cs[DQ];                    // the bias in registers, as nll_grad_kernel holds it
#pragma unroll
  for (int i = 0; i < DQ; ++i) {
    bv[i] = load4(bias_row, 16 * (tid + 256 * i));
    cs[i] = f4(0.f);
  }
  for (int i = tid; i < (256 * DQ * 4) / 32; i += 256) bits[i] = 0u;
  __syncthreads();
  for (int row = blockIdx.x; row < R; row += gridDim.x) {
    const __amdgpu_buffer_rsrc_t z = row_buffer(scores + (size_t)row * V, 4 * V);
    const long long t = y[row];
    if (t == -1) {                          // masked (the same for the whole workgroup): the row held scores, so zeros are written
      const int tm = fresh(tid);
#pragma unroll
      for (int i = 0; i < DQ; ++i) {
        if (tm + 256 * i < nq) store4(z, 16 * (tm + 256 * i), f4(0.f));
      }
      if (tid < 4) rowloss[(size_t)tid * R + row] = 0.f;
      continue;
    }
    const bool inr = t >= 0 && t < V;
    const int tc = inr ? (int)t : -1;       // the target's column: float4 (tc >> 2) is slot (tc >> 10) of lane (tc >> 2) & 255
    const bool own = inr && ((tc >> 2) & 255) == tid;
    float4 v[DQ];
    long long neg = -1;                     // lane j < k: the row's j-th negative
    float m = -INFINITY;
    {
      const int tl = fresh(tid);
#pragma unroll
      for (int i = 0; i < DQ; ++i) v[i] = load4(z, 16 * (tl + 256 * i));   // every load unconditional
      if (unlike && tid < o.k) neg = o.negatives[(size_t)row * o.k + tid];
#pragma unroll
      for (int i = 0; i < DQ; ++i) {
        const int q = tl + 256 * i;
        v[i].x += bv[i].x, v[i].y += bv[i].y, v[i].z += bv[i].z, v[i].w += bv[i].w;
        if (q >= nq) v[i] = f4(-INFINITY);
        m = fmaxf(m, fmaxf(fmaxf(v[i].x, v[i].y), fmaxf(v[i].z, v[i].w)));
      }
    }
    m = block_reduce<true>(m, red);
    const bool isneg = neg >= 0 && neg < V;
    if (isneg) atomicOr(&bits[(int)neg >> 5], 1u << ((int)neg & 31));   // published by the barriers of the next reduction
    float sm[2] = {0.f, 0.f};               // s = sum exp(x); sum x over the real columns
    float xt = 0.f;                         // x of the target, held by the thread that owns the target's column
    {
      const int ts = fresh(tid);
#pragma unroll
      for (int i = 0; i < DQ; ++i) {        // keep the exponentials: they are the softmax numerators
        v[i].x -= m, v[i].y -= m, v[i].z -= m, v[i].w -= m;
        if (own && (tc >> 10) == i) xt = pick(v[i], tc & 3);
        if (smooth && ts + 256 * i < nq) sm[1] += (v[i].x + v[i].y) + (v[i].z + v[i].w);
        v[i] = make_float4(__expf(v[i].x), __expf(v[i].y), __expf(v[i].z), __expf(v[i].w));
        sm[0] += (v[i].x + v[i].y) + (v[i].z + v[i].w);
      }
    }
    block_reduce<2, false>(sm, red);
    const float s = sm[0], logs = __logf(s), lse = m + logs;
    float un[2] = {0.f, 0.f};               // S = sum of w over the set; ul
    if (unlike) {
      const float invs = 1.f / s;
      const int tn = fresh(tid);
#pragma unroll
      for (int i = 0; i < DQ; ++i) {
        const int q = tn + 256 * i;
        const unsigned nib = q < nq ? quad_bits(bits, q, own && (tc >> 10) == i, tc) : 0u;
        if (nib != 0u) {
          if (nib & 1u) un[0] += ul_weight(v[i].x * invs, un[1]);
          if (nib & 2u) un[0] += ul_weight(v[i].y * invs, un[1]);
          if (nib & 4u) un[0] += ul_weight(v[i].z * invs, un[1]);
          if (nib & 8u) un[0] += ul_weight(v[i].w * invs, un[1]);
        }
      }
      block_reduce<2, false>(un, red);
    }
    const float kp = (sc * (1.f + 2.f * o.zeta * lse - o.alpha * un[0])) / s;
    {                                       // the gradient, in place
      const float invs = 1.f / s;
      const int tw = fresh(tid);
#pragma unroll
      for (int i = 0; i < DQ; ++i) {
        const int q = tw + 256 * i, dc = tc - 4 * q;   // dc: the target's column within this float4, if it is in 0 .. 3
        if (q < nq) {
          float4 g;
          g.x = v[i].x * kp - (dc == 0 ? ct : 0.f);
          g.y = v[i].y * kp - (dc == 1 ? ct : 0.f);
          g.z = v[i].z * kp - (dc == 2 ? ct : 0.f);
          g.w = v[i].w * kp - (dc == 3 ? ct : 0.f);
          if (smooth) g.x -= ce, g.y -= ce, g.z -= ce, g.w -= ce;
          if (unlike) {
            const unsigned nib = quad_bits(bits, q, own && (tc >> 10) == i, tc);
            if (nib != 0u) {
              float drop = 0.f;
              if (nib & 1u) g.x += ca * ul_weight(v[i].x * invs, drop);
              if (nib & 2u) g.y += ca * ul_weight(v[i].y * invs, drop);
              if (nib & 4u) g.z += ca * ul_weight(v[i].z * invs, drop);
              if (nib & 8u) g.w += ca * ul_weight(v[i].w * invs, drop);
            }
          }
          store4(z, 16 * q, g);
          cs[i].x += g.x, cs[i].y += g.y, cs[i].z += g.z, cs[i].w += g.w;
        }
      }
    }
    if (own) rowloss[row] = logs - xt;      // lse - z_t
    if (tid == 0) {
      if (!inr) rowloss[row] = NAN;         // a target outside [0, V) that is not the mask: NaN loss, as in nll_grad_kernel
      rowloss[(size_t)R + row] = smooth ? logs - sm[1] / (float)V : 0.f;   // lse - mean z
      rowloss[2 * (size_t)R + row] = lse * lse;
      rowloss[3 * (size_t)R + row] = un[1];
    }
    if (unlike) {                           // the bitmap back to zeros, behind the last test of it
      __syncthreads();
      if (isneg) bits[(int)neg >> 5] = 0u;
    }
  }
  const __amdgpu_buffer_rsrc_t part = row_buffer(dbpart + (size_t)blockIdx.x * V, 4 * V);
#pragma unroll
  for (int i = 0; i < DQ; ++i) {
    if (tid + 256 * i < nq) store4(part, 16 * (tid + 256 * i), cs[i]);
  }
}

// dbias[v] = sum over the workgroups' column partials (fixed order); block 0 also finishes the losses.  A workgroup takes 32
// columns, its eight 32-lane groups an eighth of the partial rows each (eight loads in flight), the eight sums meet in LDS in
// group order.  (One thread per column walking all 512 partial rows was a chain of 64 round trips on 40 workgroups: 34 us.)
// PARTS = 1: rowloss (R), loss = scale * sum.  PARTS = 2: rowloss (2, R) hard | soft, loss = {total, hard, soft}, hard and soft
// scaled by `scale`, total = (1 - alpha) hard + alpha soft.  PARTS = 4: rowloss (4, R) nll | smooth | z | unlikelihood, loss = {total,
// the four parts}, the parts scaled by scale * *scale_dev (where given), total = (1 - eps) nll + eps smooth + zeta z + alpha unlikelihood.
template <int PARTS>
__device__ __forceinline__ void head_loss_finish(int R, int V, int nwg, float scale, float alpha, float eps, float zeta,
                                                 const float* __restrict__ scale_dev, const float* __restrict__ rowloss,
                                                 const float* __restrict__ dbpart, float* __restrict__ dbias, float* __restrict__ loss) {
  __shared__ float red[4 * PARTS];
  __shared__ float col[8][32];
  const int li = threadIdx.x & 31, grp = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + li, cc = c < V ? c : V - 1;
  if (dbias != nullptr) {
    const int per = (nwg + 7) / 8;
    const int w0 = grp * per < nwg ? grp * per : nwg, w1 = w0 + per < nwg ? w0 + per : nwg;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    int w = w0;
    for (; w + 7 < w1; w += 8) {
      float t[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) t[i] = dbpart[(size_t)(w + i) * V + cc];
#pragma unroll
      for (int i = 0; i < 8; ++i) a[i & 3] += t[i];
    }
    for (; w < w1; ++w) a[0] += dbpart[(size_t)w * V + cc];
    col[grp][li] = (a[0] + a[1]) + (a[2] + a[3]);
    __syncthreads();
    if (grp == 0 && c < V) {
      float total = col[0][li];
#pragma unroll
      for (int q = 1; q < 8; ++q) total += col[q][li];
      dbias[c] = total;
    }
  }
  if (blockIdx.x == 0) {
    float part[PARTS];
#pragma unroll
    for (int p = 0; p < PARTS; ++p) part[p] = 0.f;
    for (int r = threadIdx.x; r < R; r += 256) {
#pragma unroll
      for (int p = 0; p < PARTS; ++p) part[p] += rowloss[(size_t)p * R + r];
    }
    block_reduce<PARTS, false>(part, red);
    if (threadIdx.x == 0) {
      if constexpr (PARTS == 1) {
        *loss = scale * part[0];
      } else if constexpr (PARTS == 2) {
        const float hard = scale * part[0], soft = scale * part[1];
        loss[0] = (1.f - alpha) * hard + alpha * soft, loss[1] = hard, loss[2] = soft;
      } else {
        const float sc = scale_dev != nullptr ? scale * *scale_dev : scale;
#pragma unroll
        for (int p = 0; p < PARTS; ++p) loss[1 + p] = part[p] = sc * part[p];
        loss[0] = (1.f - eps) * part[0] + eps * part[1] + zeta * part[2] + alpha * part[3];
      }
    }
  }
}

template <int PARTS>
__global__ __launch_bounds__(256) void head_loss_finish_kernel(int R, int V, int nwg, float scale, float alpha,
                                                               const float* __restrict__ rowloss, const float* __restrict__ dbpart,
                                                               float* __restrict__ dbias, float* __restrict__ loss) {
  head_loss_finish<PARTS>(R, V, nwg, scale, alpha, 0.f, 0.f, nullptr, rowloss, dbpart, dbias, loss);
}
// the PARTS = 4 form of the same finish under the objective's name, with its weights and device scale
__global__ __launch_bounds__(256) void objective_finish_kernel(int R, int V, int nwg, float scale, ObjectiveArgs o,
                                                               const float* __restrict__ rowloss, const float* __restrict__ dbpart,
                                                               float* __restrict__ dbias, float* __restrict__ loss) {
  head_loss_finish<4>(R, V, nwg, scale, o.alpha, o.eps, o.zeta, o.scale_dev, rowloss, dbpart, dbias, loss);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// A pass and the finish; `obj`: the general objective; else `kd`: with a teacher - dense where `teacher` is given, else the top-k form.  -3 (VMLMF_E_UNSUPPORTED at
// the C ABI) when the in-register form does not cover the row width or an operand's alignment.  The scratch pointer's alignment is
// part of the check for every source: the column partials are stored sixteen bytes at a time (before the sources shared this tail,
// vmlmf_nll_forward_grad made that store on a misaligned scratch).
int launch_head_loss(bool kd, int R, int V, float* scores, const float* bias, const long long* y, float scale, float alpha, float tau,
                     const float* teacher, const long long* top_tokens, const float* top_scores, int top, float* loss, float* rowloss,
                     float* dbias, float* scratch, hipStream_t s, const ObjectiveArgs* obj = nullptr) {
  if (V % 4 != 0 || V > 256 * DQ * 4 || !aligned16(scores) || !aligned16(bias) || !aligned16(teacher) || !aligned16(scratch)) return -3;
  const int nwg = head_loss_workgroups(R);
  const dim3 grid(nwg), block(256);
  if (obj != nullptr) {                  // the general objective: `alpha` is its unlikelihood weight
    hipLaunchKernelGGL(objective_grad_kernel, grid, block, 0, s, R, V, scale, *obj, scores, bias, y, rowloss, scratch);
  } else if (!kd) {
    hipLaunchKernelGGL(nll_grad_kernel, grid, block, 0, s, R, V, scale, scores, bias, y, rowloss, scratch);
  } else if (teacher != nullptr) {
    const DenseTeacher src = {teacher};
    hipLaunchKernelGGL(distill_grad_kernel<DenseTeacher>, grid, block, 0, s, R, V, scale, alpha, tau, scores, bias, y, src, rowloss, scratch);
  } else {
    const TopTeacher src = {top_tokens, top_scores, top};
    hipLaunchKernelGGL(distill_grad_kernel<TopTeacher>, grid, block, 0, s, R, V, scale, alpha, tau, scores, bias, y, src, rowloss, scratch);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  const dim3 fgrid((V + 31) / 32);
  if (obj != nullptr) {
    hipLaunchKernelGGL(objective_finish_kernel, fgrid, block, 0, s, R, V, nwg, scale, *obj, rowloss, scratch, dbias, loss);
  } else {
    const auto finish = kd ? head_loss_finish_kernel<2> : head_loss_finish_kernel<1>;
    hipLaunchKernelGGL(finish, fgrid, block, 0, s, R, V, nwg, scale, alpha, rowloss, scratch, dbias, loss);
  }
  return (int)hipGetLastError();
}

}  // namespace

// workgroups of nll_grad_kernel, distill_grad_kernel and objective_grad_kernel (two per CU: 192 + VGPRs each); the column partials need NWG x V floats of scratch
int head_loss_workgroups(int R) { return R < 512 ? R : 512; }

int launch_nll_fwd_grad(int R, int V, float* scores, const float* bias, const long long* y, float scale, float* loss, float* rowloss,
                        float* dbias, float* scratch, hipStream_t s) {
  return launch_head_loss(false, R, V, scores, bias, y, scale, 0.f, 1.f, nullptr, nullptr, nullptr, 0, loss, rowloss, dbias, scratch, s);
}

int launch_distill_fwd_grad(int R, int V, float* scores, const float* bias, const long long* y, float scale, float alpha, float tau,
                            const float* teacher, const long long* top_tokens, const float* top_scores, int top, float* loss,
                            float* rowloss, float* dbias, float* scratch, hipStream_t s) {
  return launch_head_loss(true, R, V, scores, bias, y, scale, alpha, tau, teacher, top_tokens, top_scores, top, loss, rowloss, dbias, scratch, s);
}

int launch_objective_fwd_grad(int R, int V, float* scores, const float* bias, const long long* y, float scale, const ObjectiveArgs& o,
                              float* loss, float* rowloss, float* dbias, float* scratch, hipStream_t s) {
  return launch_head_loss(false, R, V, scores, bias, y, scale, o.alpha, 1.f, nullptr, nullptr, nullptr, 0, loss, rowloss, dbias, scratch, s, &o);
}
