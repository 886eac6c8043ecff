// What every form of the sampler step refuses, written once for vmlmf_lm_sample / vmlmf_lm_choose and their filtered forms
// (vmlmf_ops.hip), for vmlmf_decode_choose (vmlmf_decode.hip), for vmlmf_history_choose (vmlmf_history.hip) and for
// vmlmf_truncate_choose (vmlmf_truncate.hip); what the controlled choices refuse of the controls they share is controls_refusal, what
// the truncated choice refuses of its four samplers truncation_refusal.  `refuse(code, text)` is the caller's: it puts the entry point's
// name before the text, keeps the result as its library's error and returns the code.  Host code only.
#pragma once
#include "../../include/vmlmf_hip.h" /* VMLMF_E_* */

template <class Refuse>
static int sampler_refusal(const Refuse& refuse, int B, float inv_temperature, const void* state, const void* embed, const void* x_next, int step) {
  if (!(inv_temperature >= 0.f) || inv_temperature > 3.0e38f)
    return refuse(VMLMF_E_BADARG, "the inverse temperature must be finite and >= 0 (0: greedy)");
  if (inv_temperature > 0.f && !state) return refuse(VMLMF_E_BADARG, "sampling needs the {seed, offset} snapshot");
  if (x_next && !embed) return refuse(VMLMF_E_BADARG, "x_next needs the embedding table");
  if (step < 0) return refuse(VMLMF_E_BADARG, "step must be >= 0");
  if ((long long)(step + 1ll) * B > (1ll << 32)) return refuse(VMLMF_E_UNSUPPORTED, "2^32 positions (step * B + b) and more");
  return 0;
}
template <class Refuse>
static int filter_refusal(const Refuse& refuse, int top_k, float top_p) {
  if (top_k < 0) return refuse(VMLMF_E_BADARG, "top_k must be >= 0 (0: off)");
  if (!(top_p > 0.f && top_p <= 1.f)) return refuse(VMLMF_E_BADARG, "top_p must lie in (0, 1] (1: off)");
  return 0;
}
// eos, the repetition penalty and the minimum length of a controlled choice (vmlmf_decode_controls, and vmlmf_history_controls' head)
template <class Refuse>
static int controls_refusal(const Refuse& refuse, int V, int eos, float repetition_penalty, int min_length) {
  if (eos < -1 || eos >= V) return refuse(VMLMF_E_BADARG, "eos must be a token in [0, V), or -1 for none");
  if (!(repetition_penalty > 0.f) || repetition_penalty > 3.0e38f)
    return refuse(VMLMF_E_BADARG, "repetition_penalty must be finite and > 0 (1: off)");
  if (min_length < 0) return refuse(VMLMF_E_BADARG, "min_length must be >= 0");
  if (min_length > 0 && eos < 0) return refuse(VMLMF_E_BADARG, "min_length needs eos");
  return 0;
}
// the four truncation samplers of vmlmf_truncate_choose (vmlmf_truncation: min_p, typical_p, epsilon_cutoff, eta_cutoff)
template <class Refuse>
static int truncation_refusal(const Refuse& refuse, float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff) {
  if (!(min_p >= 0.f && min_p <= 1.f)) return refuse(VMLMF_E_BADARG, "min_p must lie in [0, 1] (0: off)");
  if (!(typical_p > 0.f && typical_p <= 1.f)) return refuse(VMLMF_E_BADARG, "typical_p must lie in (0, 1] (1: off)");
  if (!(epsilon_cutoff >= 0.f && epsilon_cutoff < 1.f)) return refuse(VMLMF_E_BADARG, "epsilon_cutoff must lie in [0, 1) (0: off)");
  if (!(eta_cutoff >= 0.f && eta_cutoff < 1.f)) return refuse(VMLMF_E_BADARG, "eta_cutoff must lie in [0, 1) (0: off)");
  return 0;
}
