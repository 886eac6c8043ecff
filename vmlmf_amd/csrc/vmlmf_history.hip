// The choice of the LM decoder under controls that need a row's SEQUENCE of tokens (Model.generate with no_repeat_ngram_size /
// banned_sequences / frequency_penalty / presence_penalty, vmlmf_amd/lm.py): libvmlmf_history.so, a library of its own beside
// libvmlmf_hip.so and libvmlmf_decode.so (include/vmlmf_history.h has the contract).  One launch per decode step behind the head's
// GEMM, a workgroup per row, as vmlmf_decode_choose - whose controls it applies too:
//   c[v] = ((seen[v] ? (x > 0 ? x / theta : x theta) : x) - alpha count[v] - (count[v] > 0 ? beta : 0)) + logit_bias[v],
//   c[eos] = -inf below the minimum length,   c[v] = -inf for v in the row's ban set
// PHASE 0 forms the ban set (history_bans below): a bitmap of ceil(V / 32) words in LDS, zeroed; threads stride over the positions of
// the row's history at which the n-gram that ends it could have stood before, and over the banned sequences; a match sets its bit
// with an LDS atomic OR - integer OR, so the bitmap does not depend on the order of arrival -; one barrier.  Then the selection of
// vmlmf_select.h (pick_row / choose_row, instantiated here for HistoryScores - nothing of it is written twice) reads the bit beside
// logit_bias, seen and count: no pass over the scores is added, and no launch.  The state (seen, length, finished, count, hist,
// hist_len, overflow) is updated in place by thread 0 behind a workgroup barrier, after every read of it.  Plain HIP C++ for wave64,
// no inline assembly, no atomics on global memory, no waiting between workgroups.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vmlmf_history.h"
#include "vmlmf_refusals.h"
#include "vmlmf_select.h"
#include "vmlmf_side.h"

namespace {

constexpr int HC_FILTERED_NT = 1024;                           // the selection's workgroup (decode_choose_kernel's)
constexpr int HC_BANS_NT = 256;                                // history_bans_kernel's
constexpr int HC_BITMAP_WORDS = VMLMF_HISTORY_MAX_V / 32;
static_assert(sizeof(SelScratch) + sizeof(unsigned) * HC_BITMAP_WORDS <= 65536, "the ban bitmap must fit a kernel's static LDS beside the selection's scratch");

// what phase 0 reads: the row's history is found from (hist, hist_len, capacity) per row
struct BanArgs {
  const int *hist, *hist_len;
  const int *seq_tokens, *seq_offsets;
  int capacity, n, n_sequences, V;
};

struct HistoryArgs {
  const float *scores, *bias, *embed;
  const unsigned long long* state;
  long long* tokens;
  float *logprob, *x_next;
  int* kept;
  float inv_temp, top_p, theta, alpha, beta;
  int B, H, step, top_k, eos, min_length;
  const float* logit_bias;
  unsigned char* seen;
  int *finished, *length;
  unsigned short* count;
  int *hist_w, *hist_len_w, *overflow;   // null: no history is kept
  int bans;                              // a ban is on: phase 0 runs
  BanArgs ban;
};

__device__ __forceinline__ int history_length(const BanArgs& a, int b) {
  const int L = a.hist_len[b];
  return L < 0 ? 0 : (L > a.capacity ? a.capacity : L);   // (never an index outside the row, whatever the word holds)
}

// PHASE 0, by the whole workgroup: bm[0 .. ceil(V / 32)) = row b's ban set (step 5 of the contract); ends behind a barrier
__device__ __forceinline__ void history_bans(unsigned* bm, const BanArgs& a, int b) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int words = (a.V + 31) >> 5;
  for (int w = tid; w < words; w += nt) bm[w] = 0u;
  __syncthreads();
  const int* h = a.hist + (size_t)b * a.capacity;
  const int L = history_length(a, b);
  const auto ban = [&](int t) {
    if ((unsigned)t < (unsigned)a.V) atomicOr(&bm[t >> 5], 1u << (t & 31));
  };
  const int n = a.n;
  if (n >= 1 && L >= n) {   // (L + 1 == n: no earlier n-gram yet)
    const int* tail = h + (L - n + 1);   // the n - 1 tokens the next one would follow
    for (int i = tid; i <= L - n; i += nt) {
      bool eq = true;
      for (int j = 0; j < n - 1 && eq; ++j) eq = h[i + j] == tail[j];
      if (eq) ban(h[i + n - 1]);
    }
  }
  for (int s = tid; s < a.n_sequences; s += nt) {
    const int lo = a.seq_offsets[s], m = a.seq_offsets[s + 1] - lo;
    if (m < 1 || L < m - 1) continue;
    const int* tail = h + (L - m + 1);
    bool eq = true;
    for (int j = 0; j < m - 1 && eq; ++j) eq = tail[j] == a.seq_tokens[lo + j];
    if (eq) ban(a.seq_tokens[lo + m - 1]);
  }
  __syncthreads();
}

// x -> c of one row (steps 1 - 5 of the contract)
struct HistoryScores {
  static constexpr bool CONTROLLED = true;
  struct Ctl {
    float lb;
    unsigned short count;
    unsigned char seen, banned;
  };
  const float *row, *bias, *logit_bias;
  const unsigned char* seen;
  const unsigned short* count;   // null: every count is 0
  const unsigned* bitmap;        // null: no ban set
  float theta, alpha, beta;
  int eos_ban;   // eos while the row is below its minimum length, else -1
  __device__ __forceinline__ float raw(int v) const { return (bias != nullptr ? bias[v] : 0.f) + row[v]; }
  __device__ __forceinline__ Ctl ctl(int v) const {
    return Ctl{logit_bias != nullptr ? logit_bias[v] : 0.f, count != nullptr ? count[v] : (unsigned short)0, seen[v],
               (unsigned char)(bitmap != nullptr ? (bitmap[v >> 5] >> (v & 31)) & 1u : 0u)};
  }
  __device__ __forceinline__ float score(int v, float x, const Ctl& ct) const {
    // (explicitly rounded operations: no contraction, so every pass of a long row forms the same bits)
    const float r = ct.seen != 0 ? (x > 0.f ? __fdiv_rn(x, theta) : __fmul_rn(x, theta)) : x;
    const float q = __fsub_rn(__fsub_rn(r, __fmul_rn(alpha, (float)ct.count)), ct.count != 0 ? beta : 0.f);
    return (v == eos_ban || ct.banned != 0) ? -INFINITY : __fadd_rn(q, ct.lb);
  }
};

struct HistoryLds {
  SelScratch S;
  unsigned bitmap[HC_BITMAP_WORDS];
};

__global__ __launch_bounds__(HC_FILTERED_NT) void history_choose_kernel(HistoryArgs a) {
  __shared__ HistoryLds lds;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int V = a.ban.V;
  if (a.eos >= 0 && a.finished[b] != 0) {   // (uniform over the workgroup) padding: nothing of the row's state moves
    if (tid == 0) {
      a.tokens[b] = a.eos;
      if (a.logprob != nullptr) a.logprob[b] = 0.f;
      if (a.kept != nullptr) a.kept[b] = 0;
    }
    if (a.x_next != nullptr) {
      const float* src = a.embed + (size_t)a.eos * a.H;
      for (int e = tid; e < a.H; e += blockDim.x) a.x_next[(size_t)b * a.H + e] = src[e];
    }
    return;
  }
  if (a.bans != 0) history_bans(lds.bitmap, a.ban, b);   // (uniform)
  unsigned char* seen = a.seen + (size_t)b * V;
  unsigned short* count = a.count != nullptr ? a.count + (size_t)b * V : nullptr;
  HistoryScores src;
  src.row = a.scores + (size_t)b * V, src.bias = a.bias, src.logit_bias = a.logit_bias, src.seen = seen, src.count = count;
  src.bitmap = a.bans != 0 ? lds.bitmap : nullptr;
  src.theta = a.theta, src.alpha = a.alpha, src.beta = a.beta;
  src.eos_ban = (a.eos >= 0 && a.length[b] < a.min_length) ? a.eos : -1;
  const bool sampling = a.inv_temp > 0.f;
  const DropKey key = sampling ? sample_key(a.state) : DropKey{0u, 0u, 0u, 0u};
  const unsigned position = (unsigned)a.step * (unsigned)a.B + (unsigned)b;
  // the host launches HC_FILTERED_NT threads with a filter on, SM_CHOOSE_NT without
  const RowPick pk = blockDim.x == HC_FILTERED_NT ? pick_row(lds.S, src, V, a.inv_temp, a.top_k, a.top_p, key, position)
                                                  : choose_row(&lds.S.red[0][0], 8, src, V, a.inv_temp, sampling, key, position);
  write_pick(pk, b, a.H, a.tokens, a.logprob, a.kept, a.x_next, a.embed);
  __syncthreads();   // every thread has read what it needs of the row's state
  if (tid == 0) {
    const int tok = pk.idx != SM_NOIDX ? pk.idx : 0;
    seen[tok] = 1;
    a.length[b] += 1;
    if (tok == a.eos) a.finished[b] = 1;
    if (count != nullptr && count[tok] != 65535) count[tok] += 1;
    if (a.hist_w != nullptr) {
      const int L = a.hist_len_w[b];
      if (L >= 0 && L < a.ban.capacity) {
        a.hist_w[(size_t)b * a.ban.capacity + L] = tok;
        a.hist_len_w[b] = L + 1;
      } else {
        a.overflow[b] = 1;   // a full history is never written past
      }
    }
  }
}

__global__ __launch_bounds__(HC_BANS_NT) void history_bans_kernel(BanArgs a, int eos, const int* finished, unsigned* out) {
  __shared__ unsigned bitmap[HC_BITMAP_WORDS];
  const int b = blockIdx.x, words = (a.V + 31) >> 5;
  unsigned* mine = out + (size_t)b * words;
  if (eos >= 0 && finished != nullptr && finished[b] != 0) {   // (uniform over the workgroup)
    for (int w = threadIdx.x; w < words; w += blockDim.x) mine[w] = 0u;
    return;
  }
  history_bans(bitmap, a, b);
  for (int w = threadIdx.x; w < words; w += blockDim.x) mine[w] = bitmap[w];
}

int fail_choose(int code, const char* msg) { return vmlmf_side::fail(code, std::string("vmlmf_history_choose: ") + msg); }
int fail_bans(int code, const char* msg) { return vmlmf_side::fail(code, std::string("vmlmf_history_bans: ") + msg); }

// what both entry points refuse of the history's own fields; fills `ban`
template <class Refuse>
int bans_refusal(const Refuse& refuse, int V, const vmlmf_history_controls* c, BanArgs& ban) {
  if (c->no_repeat_ngram_size < 0) return refuse(VMLMF_E_BADARG, "no_repeat_ngram_size must be >= 0 (0: off)");
  if (c->hist_capacity < 1) return refuse(VMLMF_E_BADARG, "hist_capacity must be >= 1");
  if (c->n_sequences < 0) return refuse(VMLMF_E_BADARG, "n_sequences must be >= 0");
  if (c->n_sequences > 0 && (!c->seq_tokens || !c->seq_offsets))
    return refuse(VMLMF_E_BADARG, "null pointer in the controls (seq_tokens and seq_offsets are required with n_sequences > 0)");
  ban.hist = c->hist, ban.hist_len = c->hist_len, ban.seq_tokens = c->seq_tokens, ban.seq_offsets = c->seq_offsets;
  ban.capacity = c->hist_capacity, ban.n = c->no_repeat_ngram_size, ban.n_sequences = c->n_sequences, ban.V = V;
  return 0;
}
const char* const TOO_WIDE = "history bans (n-grams, sequences) need V <= VMLMF_HISTORY_MAX_V (65536): the ban bitmap lives in LDS";

}  // namespace

VMLMF_SIDE_LIBRARY(vmlmf_history, VMLMF_HISTORY_ABI_VERSION)

extern "C" {

int vmlmf_history_choose(int B, int H, int V, const float* scores, const float* bias, const float* embed, float inv_temperature, int top_k,
                         float top_p, const int64_t* state, int step, const vmlmf_history_controls* c, int64_t* tokens, float* logprob,
                         float* x_next, int32_t* kept, void* stream) {
  const auto& fail = fail_choose;
  if (B < 1 || V < 1 || (x_next && H < 1)) return fail(VMLMF_E_BADARG, "B, V (and H with x_next) must be >= 1");
  if (!scores || !tokens) return fail(VMLMF_E_BADARG, "null pointer (scores, tokens)");
  if (!c) return fail(VMLMF_E_BADARG, "null controls");
  if (!c->seen || !c->finished || !c->length) return fail(VMLMF_E_BADARG, "null pointer in the controls (seen, finished and length are required)");
  if (const int rc = sampler_refusal(fail, B, inv_temperature, state, embed, x_next, step)) return rc;
  if (const int rc = filter_refusal(fail, top_k, top_p)) return rc;
  if (const int rc = controls_refusal(fail, V, c->eos, c->repetition_penalty, c->min_length)) return rc;
  HistoryArgs a;
  if (const int rc = bans_refusal(fail, V, c, a.ban)) return rc;
  const float alpha = c->frequency_penalty, beta = c->presence_penalty;
  if (!(alpha >= 0.f) || alpha > 3.0e38f) return fail(VMLMF_E_BADARG, "frequency_penalty must be finite and >= 0 (0: off)");
  if (!(beta >= 0.f) || beta > 3.0e38f) return fail(VMLMF_E_BADARG, "presence_penalty must be finite and >= 0 (0: off)");
  const bool bans = c->no_repeat_ngram_size >= 1 || c->n_sequences >= 1;
  const bool keeps = c->hist && c->hist_len && c->overflow;
  if (bans && !keeps) return fail(VMLMF_E_BADARG, "null pointer in the controls (hist, hist_len and overflow are required with a ban on)");
  if ((alpha > 0.f || beta > 0.f) && !c->count) return fail(VMLMF_E_BADARG, "null pointer in the controls (count is required with a penalty on)");
  if (bans && V > VMLMF_HISTORY_MAX_V) return fail(VMLMF_E_BADARG, TOO_WIDE);
  a.scores = scores, a.bias = bias, a.embed = embed, a.state = reinterpret_cast<const unsigned long long*>(state);
  a.tokens = reinterpret_cast<long long*>(tokens), a.logprob = logprob, a.x_next = x_next, a.kept = kept;
  a.inv_temp = inv_temperature, a.top_p = top_p, a.theta = c->repetition_penalty;
  a.alpha = alpha > 0.f ? alpha : 0.f, a.beta = beta > 0.f ? beta : 0.f;   // (a zero is +0: q == r to the bit)
  a.B = B, a.H = H, a.step = step, a.top_k = top_k >= V ? 0 : top_k, a.eos = c->eos, a.min_length = c->min_length;
  a.logit_bias = c->logit_bias, a.seen = c->seen, a.finished = c->finished, a.length = c->length, a.count = c->count;
  a.hist_w = keeps ? c->hist : nullptr, a.hist_len_w = keeps ? c->hist_len : nullptr, a.overflow = keeps ? c->overflow : nullptr;
  a.bans = bans ? 1 : 0;
  const bool filtered = inv_temperature > 0.f && (a.top_k > 0 || top_p < 1.f);
  hipLaunchKernelGGL(history_choose_kernel, dim3(B), dim3(filtered ? HC_FILTERED_NT : SM_CHOOSE_NT), 0, static_cast<hipStream_t>(stream), a);
  return vmlmf_side::launch_tail("vmlmf_history_choose");
}

int vmlmf_history_bans(int B, int V, const vmlmf_history_controls* c, uint32_t* bitmap, void* stream) {
  const auto& fail = fail_bans;
  if (B < 1 || V < 1) return fail(VMLMF_E_BADARG, "B and V must be >= 1");
  if (!c) return fail(VMLMF_E_BADARG, "null controls");
  if (!bitmap) return fail(VMLMF_E_BADARG, "null pointer (bitmap)");
  if (!c->hist || !c->hist_len) return fail(VMLMF_E_BADARG, "null pointer in the controls (hist and hist_len are required)");
  if (c->eos < -1 || c->eos >= V) return fail(VMLMF_E_BADARG, "eos must be a token in [0, V), or -1 for none");
  BanArgs ban;
  if (const int rc = bans_refusal(fail, V, c, ban)) return rc;
  if (V > VMLMF_HISTORY_MAX_V) return fail(VMLMF_E_BADARG, TOO_WIDE);
  hipLaunchKernelGGL(history_bans_kernel, dim3(B), dim3(HC_BANS_NT), 0, static_cast<hipStream_t>(stream), ban, (int)c->eos,
                     (const int*)c->finished, reinterpret_cast<unsigned*>(bitmap));
  return vmlmf_side::launch_tail("vmlmf_history_bans");
}

}  // extern "C"
