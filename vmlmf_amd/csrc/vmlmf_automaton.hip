// Decoding under a token automaton (Model.generate and Model.beam_search with automaton=): libvmlmf_automaton.so, a library of its own
// beside libvmlmf_hip.so (include/vmlmf_automaton.h has the contract).  Every row of a decode, every beam of a search, carries one
// state of a dense table next (S, V) on the device; the state's table row says which tokens are open and where each leads.  Two launches:
//   automaton_choose_kernel         vmlmf_decode_choose's kernel on a score source that wraps ControlledScores (vmlmf_controlled.h): a
//                                   token's `next` word is fetched in ctl(v) beside its logit_bias and seen byte - one more 4-byte
//                                   coalesced load in the same eight-deep batch -, a closed token's controlled score is -inf; the
//                                   finished rows and the state update are ControlledRows', the row's state is moved on by the same
//                                   thread behind the same barrier.  The selection is vmlmf_select.h's, instantiated here.
//   beam_step_kernel<OfferAutomaton> vmlmf_beam_step's selection (vmlmf_beam_core.h, written once) under a third offer policy: a live
//                                   beam withholds what the shared `closed` words, min_length and its state's table row close; the W
//                                   threads of a batch row's last workgroup that write the outputs write the survivors' states.
// No address is formed from a state outside [0, S): such a row (beam) has a null table row and offers nothing.
// Plain HIP C++ for wave64, no inline assembly, no float atomics, nothing new in LDS.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vmlmf_automaton.h"
#include "vmlmf_beam_core.h"
#include "vmlmf_controlled.h"
#include "vmlmf_refusals.h"
#include "vmlmf_select.h"
#include "vmlmf_side.h"

namespace {

using namespace vmlmf_beam_core;

constexpr int AC_FILTERED_NT = 1024;   // the selection's workgroup (vmlmf_decode_choose's sizes: 1024 with a filter on, SM_CHOOSE_NT without)

// x -> c of one row under the automaton: ControlledScores' steps 1 - 3, then step 3a
struct AutomatonScores {
  static constexpr bool CONTROLLED = true;
  struct Ctl {
    ControlledScores::Ctl base;
    int next;
  };
  ControlledScores base;
  const int32_t* trow;   // next[s], or null for a state outside [0, S)
  __device__ __forceinline__ float raw(int v) const { return base.raw(v); }
  __device__ __forceinline__ Ctl ctl(int v) const { return Ctl{base.ctl(v), trow != nullptr ? trow[v] : -1}; }
  __device__ __forceinline__ float score(int v, float x, const Ctl& ct) const {
    const float c = base.score(v, x, ct.base);
    return ct.next < 0 ? -INFINITY : c;
  }
};

struct ChooseArgs {
  ControlledRows rows;   // vmlmf_controlled.h: the scores, the controls, the rows' state and the outputs
  const unsigned long long* state;
  const int32_t* next;
  int32_t *row_state, *dead;
  float inv_temp, top_p;
  int B, step, top_k, S;
};

__global__ __launch_bounds__(AC_FILTERED_NT) void automaton_choose_kernel(ChooseArgs a) {
  __shared__ SelScratch S;
  const int b = blockIdx.x;
  const int s = a.row_state[b];    // (a finished row reads it too; it writes nothing)
  if (a.rows.padding(b)) return;   // (uniform over the workgroup) a finished row: nothing of its state moves
  AutomatonScores src;
  src.base = a.rows.source(b);
  src.trow = (s >= 0 && s < a.S) ? a.next + (size_t)s * a.rows.V : nullptr;
  const bool sampling = a.inv_temp > 0.f;
  const DropKey key = sampling ? sample_key(a.state) : DropKey{0u, 0u, 0u, 0u};
  const unsigned position = (unsigned)a.step * (unsigned)a.B + (unsigned)b;
  const RowPick pk = blockDim.x == AC_FILTERED_NT ? pick_row(S, src, a.rows.V, a.inv_temp, a.top_k, a.top_p, key, position)
                                                  : choose_row(&S.red[0][0], 8, src, a.rows.V, a.inv_temp, sampling, key, position);
  // the state the token leads to (-1: nothing had c > -inf), read in front of the barrier like everything else of the row
  const int to = (pk.idx != SM_NOIDX && src.trow != nullptr) ? src.trow[pk.idx] : -1;
  a.rows.finish(pk, b);   // (its barrier stands behind every thread's read of row_state[b] too)
  if (threadIdx.x == 0) {
    if (to >= 0)
      a.row_state[b] = to;
    else
      a.dead[b] = 1;   // the state stays
  }
}

// the automaton's offer policy (vmlmf_beam_core.h says what a policy is)
struct OfferAutomaton {
  static constexpr bool controlled = true;
  int min_length, eos, S, V;
  const uint32_t* closed;
  const int32_t *length, *next, *state;
  int32_t* state_out;
  struct Row {
    const uint32_t* closed;   // the shared words
    const int32_t* trow;      // next[s], or null for a state outside [0, S): nothing is offered
    int held;                 // eos while the beam is below min_length, else -1
    __device__ __forceinline__ bool closes(int v) const {
      if (trow == nullptr) return true;
      const unsigned m = closed != nullptr ? closed[v >> 5] : 0u;
      return ((m >> (v & 31)) & 1u) != 0u || v == held || trow[v] < 0;
    }
  };
  __device__ __forceinline__ const int32_t* table_row(int r) const {
    const int s = state[r];
    return (s >= 0 && s < S) ? next + (size_t)s * V : nullptr;
  }
  __device__ __forceinline__ Row row(int r) const { return Row{closed, table_row(r), (eos >= 0 && length[r] < min_length) ? eos : -1}; }
  // the state of the survivor in `slot`: its parent's where the parent was finished, the transition's otherwise; -1 without a candidate
  __device__ __forceinline__ void survivor(int slot, int prow, bool pdone, int tok, bool ok) const {
    int s = -1;
    if (ok) {
      if (pdone) {
        s = state[prow];
      } else {
        const int32_t* t = table_row(prow);
        s = t != nullptr ? t[tok] : -1;
      }
    }
    state_out[slot] = s;
  }
};

int fail_choose(int code, const char* msg) { return vmlmf_side::fail(code, std::string("vmlmf_automaton_choose: ") + msg); }

// 0, or why these entry points refuse the table
const char* table_refusal(const vmlmf_token_automaton* t, int V) {
  if (!t->next) return "null pointer (the table's next)";
  if (t->S < 1) return "the table needs S >= 1 states";
  if ((long long)t->S * (long long)V >= (1ll << 31)) return "S V must stay below 2^31";
  return nullptr;
}

}  // namespace

VMLMF_SIDE_LIBRARY(vmlmf_automaton, VMLMF_AUTOMATON_ABI_VERSION)

extern "C" {

int vmlmf_automaton_choose(int B, int H, int V, const float* scores, const float* bias, const float* embed, float inv_temperature, int top_k,
                           float top_p, const int64_t* state, int step, const vmlmf_automaton_controls* c, int64_t* tokens, float* logprob,
                           float* x_next, int32_t* kept, void* stream) {
  const auto& fail = fail_choose;
  if (B < 1 || V < 1 || (x_next && H < 1)) return fail(VMLMF_E_BADARG, "B, V (and H with x_next) must be >= 1");
  if (!scores || !tokens) return fail(VMLMF_E_BADARG, "null pointer (scores, tokens)");
  if (!c) return fail(VMLMF_E_BADARG, "null controls");
  const vmlmf_decode_controls& d = c->decode;
  if (!d.seen || !d.finished || !d.length) return fail(VMLMF_E_BADARG, "null pointer in the controls (seen, finished and length are required)");
  if (const int rc = sampler_refusal(fail, B, inv_temperature, state, embed, x_next, step)) return rc;
  if (const int rc = filter_refusal(fail, top_k, top_p)) return rc;
  if (const int rc = controls_refusal(fail, V, d.eos, d.repetition_penalty, d.min_length)) return rc;
  if (const char* why = table_refusal(&c->table, V)) return fail(VMLMF_E_BADARG, why);
  if (!c->row_state || !c->dead) return fail(VMLMF_E_BADARG, "null pointer (row_state and dead are required)");
  ChooseArgs a;
  a.rows.scores = scores, a.rows.bias = bias, a.rows.embed = embed, a.rows.logit_bias = d.logit_bias;
  a.rows.tokens = reinterpret_cast<long long*>(tokens), a.rows.logprob = logprob, a.rows.x_next = x_next, a.rows.kept = kept;
  a.rows.seen = d.seen, a.rows.finished = d.finished, a.rows.length = d.length, a.rows.theta = d.repetition_penalty;
  a.rows.H = H, a.rows.V = V, a.rows.eos = d.eos, a.rows.min_length = d.min_length;
  a.state = reinterpret_cast<const unsigned long long*>(state);
  a.next = c->table.next, a.S = c->table.S, a.row_state = c->row_state, a.dead = c->dead;
  a.inv_temp = inv_temperature, a.top_p = top_p, a.B = B, a.step = step, a.top_k = top_k >= V ? 0 : top_k;
  const bool filtered = inv_temperature > 0.f && (a.top_k > 0 || top_p < 1.f);
  hipLaunchKernelGGL(automaton_choose_kernel, dim3(B), dim3(filtered ? AC_FILTERED_NT : SM_CHOOSE_NT), 0, static_cast<hipStream_t>(stream), a);
  return vmlmf_side::launch_tail("vmlmf_automaton_choose");
}

size_t vmlmf_automaton_workspace_bytes(int B, int W, int V) { return step_workspace_bytes(B, W, V); }

int vmlmf_automaton_beam_step(int B, int W, int H, int V, const float* scores, const float* bias, const float* cum, const int32_t* finished,
                              const int32_t* length, int eos, const float* embed, int min_length, const uint32_t* closed,
                              const vmlmf_token_automaton* table, const int32_t* beam_state, int32_t* beam_state_out, int32_t* parent,
                              int64_t* token, float* total, int32_t* finished_out, int32_t* length_out, float* x_next, int32_t* src_row,
                              uint32_t* ticket, void* workspace, size_t workspace_bytes, void* stream) {
  using vmlmf_side::fail;
  const std::string name = "vmlmf_automaton_beam_step: ";
  std::string why;
  BeamStepArgs a;
  if (const int rc = step_args(a, &why, B, W, H, V, scores, bias, cum, finished, length, eos, embed, parent, token, total, finished_out,
                               length_out, x_next, src_row, ticket, workspace, workspace_bytes, "vmlmf_automaton_workspace_bytes"))
    return fail(rc, name + why);
  if (min_length < 0) return fail(VMLMF_E_BADARG, name + "min_length must be >= 0");
  if (min_length > 0 && eos < 0) return fail(VMLMF_E_BADARG, name + "min_length needs eos (the token it holds back)");
  if (!table) return fail(VMLMF_E_BADARG, name + "null table");
  if (const char* t = table_refusal(table, V)) return fail(VMLMF_E_BADARG, name + t);
  if (!beam_state || !beam_state_out) return fail(VMLMF_E_BADARG, name + "null pointer (beam_state and beam_state_out are required)");
  if (beam_state == beam_state_out)
    return fail(VMLMF_E_BADARG, name + "beam_state_out must not alias beam_state (the merge reads other slots' states)");
  OfferAutomaton p;
  p.min_length = min_length, p.eos = eos, p.S = table->S, p.V = V, p.closed = closed, p.length = length, p.next = table->next;
  p.state = beam_state, p.state_out = beam_state_out;
  hipLaunchKernelGGL(beam_step_kernel<OfferAutomaton>, dim3(B * W), dim3(BS_NT), 0, static_cast<hipStream_t>(stream), a, p);
  return vmlmf_side::launch_tail("vmlmf_automaton_beam_step");
}

}  // extern "C"
