// The thin entry points of the C ABI: argument checks and one launch each (head, criterion, embedding, dropout, sampler, transpose).
#include "vmlmf_host.h"
#include "vmlmf_refusals.h"

using namespace vmlmf_host;

extern "C" {

int vmlmf_head_forward(int B, int H, int C, const float* h, long long ldh, const float* weight,
                       const float* bias, float* logits, void* stream) {
  if (B < 1 || H < 1 || C < 1 || ldh < H) return fail(VMLMF_E_BADARG, "head: B, H, C must be >= 1 and ldh >= H");
  if (C > head_max_classes()) return fail(VMLMF_E_UNSUPPORTED, "head: more than 32 classes");
  if (h == nullptr || weight == nullptr || logits == nullptr) return fail(VMLMF_E_BADARG, "head: null pointer");
  hipStream_t s = (hipStream_t)stream;
  Scope sc(SL_HEAD_FWD, s);
  return hip_tail((int)launch_head_fwd(B, H, C, h, ldh, weight, bias, logits, s));
}

int vmlmf_head_backward(int B, int H, int C, const float* h, long long ldh, const float* weight,
                        const float* dlogits, float* dh, float* dweight, float* dbias, void* stream) {
  if (B < 1 || H < 1 || C < 1 || ldh < H) return fail(VMLMF_E_BADARG, "head: B, H, C must be >= 1 and ldh >= H");
  if (C > head_max_classes()) return fail(VMLMF_E_UNSUPPORTED, "head: more than 32 classes");
  if (h == nullptr || weight == nullptr || dlogits == nullptr) return fail(VMLMF_E_BADARG, "head: null pointer");
  hipStream_t s = (hipStream_t)stream;
  Scope sc(SL_HEAD_BWD, s);
  return hip_tail((int)launch_head_bwd(B, H, C, h, ldh, weight, dlogits, dh, dweight, dbias, s));
}

int vmlmf_ce_forward(int B, int C, const float* logits, const int64_t* target, int64_t ignore_index, float* loss,
                     float* lse, float* nvalid, float* dlogits_unit, void* stream) {
  if (B < 1 || C < 1) return fail(VMLMF_E_BADARG, "ce: B and C must be >= 1");
  if (!logits || !target || !loss || !lse || !nvalid) return fail(VMLMF_E_BADARG, "ce: null pointer");
  hipStream_t s = (hipStream_t)stream;
  Scope sc(SL_CE_FWD, s);
  return hip_tail((int)launch_ce_fwd(B, C, logits, (const long long*)target, (long long)ignore_index, loss, lse, nvalid, dlogits_unit, s));
}

int vmlmf_ce_backward(int B, int C, const float* logits, const int64_t* target, int64_t ignore_index,
                      const float* lse, const float* nvalid, const float* dloss, float* dlogits, void* stream) {
  if (B < 1 || C < 1) return fail(VMLMF_E_BADARG, "ce: B and C must be >= 1");
  if (!logits || !target || !lse || !nvalid || !dloss || !dlogits) return fail(VMLMF_E_BADARG, "ce: null pointer");
  hipStream_t s = (hipStream_t)stream;
  Scope sc(SL_CE_BWD, s);
  return hip_tail((int)launch_ce_bwd(B, C, logits, (const long long*)target, (long long)ignore_index, lse, nvalid, dloss, dlogits, s));
}

int vmlmf_nll_forward(int R, int V, const float* scores, const int64_t* y, float scale, float* loss, float* lse,
                      float* rowloss, void* stream) {
  if (R < 1 || V < 1) return fail(VMLMF_E_BADARG, "nll: R and V must be >= 1");
  if (!scores || !y || !loss || !lse || !rowloss) return fail(VMLMF_E_BADARG, "nll: null pointer");
  return hip_tail((int)launch_nll_fwd(R, V, scores, (const long long*)y, scale, loss, lse, rowloss, (hipStream_t)stream));
}

int vmlmf_nll_backward(int R, int V, const float* scores, const int64_t* y, float scale, const float* lse,
                       const float* dloss, float* dscores, void* stream) {
  if (R < 1 || V < 1) return fail(VMLMF_E_BADARG, "nll: R and V must be >= 1");
  if (!scores || !y || !lse || !dloss || !dscores) return fail(VMLMF_E_BADARG, "nll: null pointer");
  return hip_tail((int)launch_nll_bwd(R, V, scores, (const long long*)y, scale, lse, dloss, dscores, (hipStream_t)stream));
}

// the training forms of the head's losses (vmlmf_head_loss.hip): one scratch size, one refusal
static size_t head_loss_scratch_floats(int R, int V) { return (size_t)head_loss_workgroups(R < 1 ? 1 : R) * (size_t)(V < 1 ? 1 : V); }
static int head_loss_tail(int rc) {
  if (rc == -3) return fail(VMLMF_E_UNSUPPORTED, "head loss: rows must be 16-byte aligned, a multiple of four and at most 12288 wide");
  return hip_tail(rc);
}

size_t vmlmf_nll_grad_scratch_floats(int R, int V) { return head_loss_scratch_floats(R, V); }

int vmlmf_nll_forward_grad(int R, int V, float* scores, const float* bias, const int64_t* y, float scale, float* loss,
                           float* rowloss, float* dbias, float* scratch, void* stream) {
  if (R < 1 || V < 1) return fail(VMLMF_E_BADARG, "nll: R and V must be >= 1");
  if (!scores || !y || !loss || !rowloss || !scratch) return fail(VMLMF_E_BADARG, "nll: null pointer");
  return head_loss_tail(launch_nll_fwd_grad(R, V, scores, bias, (const long long*)y, scale, loss, rowloss, dbias, scratch, (hipStream_t)stream));
}

size_t vmlmf_distill_scratch_floats(int R, int V) { return head_loss_scratch_floats(R, V); }

int vmlmf_distill_forward_grad(int R, int V, float* scores, const float* bias, const int64_t* y, float scale, const vmlmf_distill* kd,
                               float* loss, float* rowloss, float* dbias, float* scratch, void* stream) {
  if (R < 1 || V < 1) return fail(VMLMF_E_BADARG, "distill: R and V must be >= 1");
  if (!scores || !y || !kd || !loss || !rowloss || !scratch) return fail(VMLMF_E_BADARG, "distill: null pointer");
  if (!(kd->alpha >= 0.f && kd->alpha <= 1.f)) return fail(VMLMF_E_BADARG, "distill: alpha must lie in [0, 1]");
  if (!(kd->temperature > 0.f) || !(kd->temperature < INFINITY)) return fail(VMLMF_E_BADARG, "distill: the temperature must be finite and positive");
  const bool dense = kd->teacher != nullptr, topk = kd->top_tokens != nullptr || kd->top_scores != nullptr || kd->top != 0;
  if (dense == topk) return fail(VMLMF_E_BADARG, "distill: exactly one teacher form - teacher (R, V), or top_tokens and top_scores (R, top)");
  if (topk && (!kd->top_tokens || !kd->top_scores)) return fail(VMLMF_E_BADARG, "distill: the top-k form takes top_tokens and top_scores");
  if (topk && (kd->top < 1 || kd->top > 32)) return fail(VMLMF_E_BADARG, "distill: top must lie in [1, 32]");
  return head_loss_tail(launch_distill_fwd_grad(R, V, scores, bias, (const long long*)y, scale, kd->alpha, kd->temperature, kd->teacher,
                                                (const long long*)kd->top_tokens, kd->top_scores, kd->top, loss, rowloss, dbias, scratch,
                                                (hipStream_t)stream));
}

size_t vmlmf_objective_scratch_floats(int R, int V) { return head_loss_scratch_floats(R, V); }

int vmlmf_objective_forward_grad(int R, int V, float* scores, const float* bias, const int64_t* y, float scale, const vmlmf_objective* obj,
                                 float* loss, float* rowloss, float* dbias, float* scratch, void* stream) {
  if (R < 1 || V < 1) return fail(VMLMF_E_BADARG, "objective: R and V must be >= 1");
  if (!scores || !y || !obj || !loss || !rowloss || !scratch) return fail(VMLMF_E_BADARG, "objective: null pointer");
  if (!(obj->label_smoothing >= 0.f && obj->label_smoothing < 1.f)) return fail(VMLMF_E_BADARG, "objective: label_smoothing must lie in [0, 1)");
  if (!(obj->z_loss >= 0.f) || !(obj->z_loss < INFINITY)) return fail(VMLMF_E_BADARG, "objective: z_loss must be finite and >= 0");
  if (!(obj->unlikelihood >= 0.f) || !(obj->unlikelihood < INFINITY)) return fail(VMLMF_E_BADARG, "objective: unlikelihood must be finite and >= 0");
  if (obj->k < 0 || obj->k > 256) return fail(VMLMF_E_BADARG, "objective: k must lie in [0, 256]");
  if (obj->unlikelihood > 0.f && (!obj->negatives || obj->k < 1)) return fail(VMLMF_E_BADARG, "objective: unlikelihood > 0 takes negatives (R, k), k >= 1");
  const ObjectiveArgs o = {obj->label_smoothing, obj->z_loss, obj->unlikelihood, (const long long*)obj->negatives, obj->k, obj->scale_dev};
  return head_loss_tail(launch_objective_fwd_grad(R, V, scores, bias, (const long long*)y, scale, o, loss, rowloss, dbias, scratch, (hipStream_t)stream));
}

size_t vmlmf_embed_backward_scratch_bytes(int R, int V) { return embed_bwd_scratch_bytes(R < 1 ? 1 : R, V < 1 ? 1 : V); }

int vmlmf_embed_backward(int R, int H, int V, const int64_t* tokens, const float* dy, float* dweight, void* scratch,
                         size_t scratch_bytes, void* stream) {
  if (R < 1 || H < 1 || V < 1) return fail(VMLMF_E_BADARG, "embed: R, H, V must be >= 1");
  if (!tokens || !dy || !dweight) return fail(VMLMF_E_BADARG, "embed: null pointer");
  const int rc = launch_embed_bwd(R, H, V, (const long long*)tokens, dy, dweight, scratch, scratch_bytes, (hipStream_t)stream);
  if (rc == -3) return fail(VMLMF_E_UNSUPPORTED, "embed_backward: embedding width > 1024");
  if (rc == -4) return fail(VMLMF_E_WORKSPACE, "embed_backward: scratch smaller than vmlmf_embed_backward_scratch_bytes()");
  return hip_tail(rc);
}

// ---- dropout of the LM network (ABI 11; vmlmf_dropout.h) ----
int vmlmf_dropout_fused(const vmlmf_desc* d) {
  VGeo g;
  RbGeo q;
  if (make_geo(d, &g, &q) != 0) return 0;
  return drop_fused(g) ? 1 : 0;
}

int vmlmf_dropout_advance(int64_t* state, int64_t* snapshot, void* stream) {
  if (!state || !snapshot || state == snapshot) return fail(VMLMF_E_BADARG, "dropout_advance: two distinct device words pairs");
  return hip_tail(launch_drop_advance(reinterpret_cast<unsigned long long*>(state), reinterpret_cast<unsigned long long*>(snapshot), (hipStream_t)stream));
}

// B: 0 for the flat entries; the _locked forms' batch rows (R = T B positions, time-major), the flag set here
static int locked_site(int64_t R, int B, int* site) {
  if (B < 1 || R % B != 0) return fail(VMLMF_E_BADARG, "dropout: a locked mask takes B >= 1 and R = T B rows");
  *site |= VMLMF_SITE_LOCKED;
  return 0;
}

static int drop_rows(int mode, int64_t R, int H, int V, float p, const int64_t* state, int site, const DropCols& cm, const float* x,
                     const int64_t* tokens, float* y, void* stream, int B = 0) {
  if (R < 0 || H < 1) return fail(VMLMF_E_BADARG, "dropout: R >= 0, H >= 1");
  DropArgs d;
  const int rc = drop_args(p, state, site, nullptr, &d, B);
  if (rc != 0) return rc;
  if (!state || !y || (mode != 1 && !x) || (mode == 2 && !tokens)) return fail(VMLMF_E_BADARG, "dropout: null pointer");
  if (R >= (1ll << 32)) return fail(VMLMF_E_UNSUPPORTED, "dropout: 2^32 positions and more");
  return hip_tail(launch_drop_rows(mode, R, H, V, d, cm, x, (const long long*)tokens, y, (hipStream_t)stream));
}

int vmlmf_dropout_apply(int64_t R, int H, const float* x, float* y, float p, const int64_t* state, int site, void* stream) {
  const DropCols cm = {H, 0};
  return drop_rows(0, R, H, 0, p, state, site, cm, x, nullptr, y, stream);
}

int vmlmf_dropout_apply_locked(int64_t R, int B, int H, const float* x, float* y, float p, const int64_t* state, int site, void* stream) {
  if (int rc = locked_site(R, B, &site)) return rc;
  const DropCols cm = {H, 0};
  return drop_rows(0, R, H, 0, p, state, site, cm, x, nullptr, y, stream, B);
}

static int drop_factors_entry(const vmlmf_desc* d, int64_t R, int B, int H, float p, const int64_t* state, int site, float* factors, void* stream) {
  DropCols cm = {H, 0};
  if (d != nullptr) {
    VGeo g;
    RbGeo q;
    int rc = make_geo(d, &g, &q);
    if (rc != 0) return rc;
    if (g.H != H) return fail(VMLMF_E_BADARG, "dropout_factors: H is not the layer's hidden size");
    if (g.rb) cm.Hg = g.Hg, cm.gstride = 64 * g.W;
  }
  return drop_rows(1, R, H, 0, p, state, site, cm, nullptr, nullptr, factors, stream, B);
}

int vmlmf_dropout_factors(const vmlmf_desc* d, int64_t R, int H, float p, const int64_t* state, int site, float* factors, void* stream) {
  return drop_factors_entry(d, R, 0, H, p, state, site, factors, stream);
}

int vmlmf_dropout_factors_locked(const vmlmf_desc* d, int64_t R, int B, int H, float p, const int64_t* state, int site, float* factors,
                                 void* stream) {
  if (int rc = locked_site(R, B, &site)) return rc;
  return drop_factors_entry(d, R, B, H, p, state, site, factors, stream);
}

int vmlmf_embed_dropout_forward(int R, int H, int V, const int64_t* tokens, const float* weight, float* out, float p, const int64_t* state,
                                int site, void* stream) {
  if (V < 1) return fail(VMLMF_E_BADARG, "embed: V must be >= 1");
  const DropCols cm = {H, 0};
  return drop_rows(2, R, H, V, p, state, site, cm, weight, tokens, out, stream);
}

int vmlmf_embed_dropout_backward(int R, int H, int V, const int64_t* tokens, const float* dy, float* dweight, void* scratch,
                                 size_t scratch_bytes, float p, const int64_t* state, int site, void* stream) {
  if (R < 1 || H < 1 || V < 1) return fail(VMLMF_E_BADARG, "embed: R, H, V must be >= 1");
  if (!tokens || !dy || !dweight || !state) return fail(VMLMF_E_BADARG, "embed: null pointer");
  DropArgs d;
  int rc = drop_args(p, state, site, nullptr, &d);
  if (rc != 0) return rc;
  rc = launch_embed_bwd(R, H, V, (const long long*)tokens, dy, dweight, scratch, scratch_bytes, (hipStream_t)stream, &d);
  if (rc == -3) return fail(VMLMF_E_UNSUPPORTED, "embed_dropout_backward: embedding width > 1024");
  if (rc == -4) return fail(VMLMF_E_WORKSPACE, "embed_backward: scratch smaller than vmlmf_embed_backward_scratch_bytes()");
  return hip_tail(rc);
}

// ---- the table that is embedding and vocabulary projection at once, and word dropout (docs/design/lm_tied.md) ----
// both probabilities checked, the element dropout's arguments and the word dropout's; the state is needed iff one of them is on
static int embed_ex_args(float p, float word_p, const int64_t* state, int site, DropArgs* d, WordDrop* wd, int B = 0) {
  int rc = drop_args(p, state, site, nullptr, d, B);
  if (rc != 0) return rc;
  if (!(word_p >= 0.f && word_p < 1.f)) return fail(VMLMF_E_BADARG, "embed: word_p must be in [0, 1)");
  wd->thresh = drop_thresh(word_p), wd->scale = 1.f / (1.f - word_p), wd->drop = p > 0.f, wd->word = word_p > 0.f;
  if ((wd->drop || wd->word) && !state) return fail(VMLMF_E_BADARG, "embed: dropout without a generator state");
  return 0;
}

// the _ex entries (B == 0) and their _lk forms (B >= 1, the flag set), written once
static int embed_forward_entry(int R, int B, int H, int V, const int64_t* tokens, const float* weight, float* out, float p, float word_p,
                               const int64_t* state, int site, void* stream) {
  if (R < 0 || H < 1 || V < 1) return fail(VMLMF_E_BADARG, "embed: R >= 0, H >= 1, V >= 1");
  DropArgs d;
  WordDrop wd;
  if (int rc = embed_ex_args(p, word_p, state, site, &d, &wd, B)) return rc;
  if (!tokens || !weight || !out) return fail(VMLMF_E_BADARG, "embed: null pointer");
  return hip_tail(launch_embed_fwd_ex(R, H, V, d, wd, weight, (const long long*)tokens, out, (hipStream_t)stream));
}

int vmlmf_embed_dropout_forward_ex(int R, int H, int V, const int64_t* tokens, const float* weight, float* out, float p, float word_p,
                                   const int64_t* state, int site, void* stream) {
  return embed_forward_entry(R, 0, H, V, tokens, weight, out, p, word_p, state, site, stream);
}

int vmlmf_embed_dropout_forward_lk(int R, int B, int H, int V, const int64_t* tokens, const float* weight, float* out, float p,
                                   float word_p, const int64_t* state, int site, void* stream) {
  if (int rc = locked_site(R, B, &site)) return rc;
  return embed_forward_entry(R, B, H, V, tokens, weight, out, p, word_p, state, site, stream);
}

static int embed_backward_entry(int R, int B, int H, int V, const int64_t* tokens, const float* dy, float* dweight, int accumulate,
                                void* scratch, size_t scratch_bytes, float p, float word_p, const int64_t* state, int site, void* stream) {
  if (R < 1 || H < 1 || V < 1) return fail(VMLMF_E_BADARG, "embed: R, H, V must be >= 1");
  if (!tokens || !dy || !dweight) return fail(VMLMF_E_BADARG, "embed: null pointer");
  DropArgs d;
  WordDrop wd;
  if (int rc = embed_ex_args(p, word_p, state, site, &d, &wd, B)) return rc;
  const int rc = launch_embed_bwd_ex(R, H, V, (const long long*)tokens, dy, dweight, accumulate, scratch, scratch_bytes, d, wd, (hipStream_t)stream);
  if (rc == -3) return fail(VMLMF_E_UNSUPPORTED, "embed_backward_ex: embedding width > 1024");
  if (rc == -4) return fail(VMLMF_E_WORKSPACE, "embed_backward_ex: scratch smaller than vmlmf_embed_backward_scratch_bytes()");
  return hip_tail(rc);
}

int vmlmf_embed_backward_ex(int R, int H, int V, const int64_t* tokens, const float* dy, float* dweight, int accumulate, void* scratch,
                            size_t scratch_bytes, float p, float word_p, const int64_t* state, int site, void* stream) {
  return embed_backward_entry(R, 0, H, V, tokens, dy, dweight, accumulate, scratch, scratch_bytes, p, word_p, state, site, stream);
}

int vmlmf_embed_backward_lk(int R, int B, int H, int V, const int64_t* tokens, const float* dy, float* dweight, int accumulate,
                            void* scratch, size_t scratch_bytes, float p, float word_p, const int64_t* state, int site, void* stream) {
  if (int rc = locked_site(R, B, &site)) return rc;
  return embed_backward_entry(R, B, H, V, tokens, dy, dweight, accumulate, scratch, scratch_bytes, p, word_p, state, site, stream);
}

// ---- activation regularisation of the LM's top layer (vmlmf_dropout.hip; docs/design/lm_actreg.md) ----
size_t vmlmf_actreg_scratch_floats(int T, int B, int H) { return (T < 1 || B < 1 || H < 1) ? 0 : 2 * (size_t)actreg_workgroups(T, B, H); }

// the arguments both directions share; the site's dropout is off (no state read) at p == 0
static int actreg_args(int T, int B, int H, const float* raw, const int64_t* lengths, float ar, float tar, float p, const int64_t* state,
                       int site, const vmlmf_desc* d, float* yd, ActRegArgs* a) {
  memset(a, 0, sizeof(*a));
  if (T < 1 || B < 1 || H < 1) return fail(VMLMF_E_BADARG, "actreg: T, B, H must be >= 1");
  if (!(ar >= 0.f && ar < INFINITY && tar >= 0.f && tar < INFINITY)) return fail(VMLMF_E_BADARG, "actreg: ar and tar must be finite and >= 0");
  if ((long long)T * B >= (1ll << 32)) return fail(VMLMF_E_UNSUPPORTED, "actreg: 2^32 positions and more");
  int rc = drop_args(p, p > 0.f ? state : nullptr, site, yd, &a->d, B);
  if (rc != 0) return rc;
  if (raw == nullptr || (p > 0.f && state == nullptr)) return fail(VMLMF_E_BADARG, "actreg: null pointer");
  a->cm.Hg = H, a->cm.gstride = 0;
  if (d != nullptr) {
    VGeo g;
    RbGeo q;
    if ((rc = make_geo(d, &g, &q)) != 0) return rc;
    if (g.H != H) return fail(VMLMF_E_BADARG, "actreg: H is not the layer's hidden size");
    if (g.rb) a->cm.Hg = g.Hg, a->cm.gstride = 64 * g.W;
  }
  a->T = T, a->B = B, a->H = H, a->raw = raw, a->lengths = (const long long*)lengths, a->ar = ar, a->tar = tar;
  return 0;
}

int vmlmf_actreg_forward(int T, int B, int H, const float* raw, float* yd, const int64_t* lengths, float ar, float tar, float batch_scale,
                         float p, const int64_t* state, int site, const vmlmf_desc* d, float* stats, float* scratch, int64_t* ticket,
                         void* stream) {
  ActRegArgs a;
  const int rc = actreg_args(T, B, H, raw, lengths, ar, tar, p, state, site, d, yd, &a);
  if (rc != 0) return rc;
  if (!(batch_scale >= 0.f && batch_scale < INFINITY)) return fail(VMLMF_E_BADARG, "actreg: batch_scale must be finite and >= 0");
  if (!stats || !scratch || !ticket || (p > 0.f && !yd)) return fail(VMLMF_E_BADARG, "actreg: null pointer");
  a.batch_scale = batch_scale, a.stats = stats;
  a.part = reinterpret_cast<unsigned long long*>(scratch), a.ticket = reinterpret_cast<unsigned long long*>(ticket);
  return hip_tail(launch_actreg_fwd(a, (hipStream_t)stream));
}

int vmlmf_actreg_backward(int T, int B, int H, const float* raw, const float* g, float* draw, const int64_t* lengths, float ar, float tar,
                          float p, const int64_t* state, int site, const vmlmf_desc* d, const float* stats, const float* dpenalty,
                          void* stream) {
  ActRegArgs a;
  const int rc = actreg_args(T, B, H, raw, lengths, ar, tar, p, state, site, d, nullptr, &a);
  if (rc != 0) return rc;
  if (!g || !draw || !stats || g == draw) return fail(VMLMF_E_BADARG, "actreg: null pointer, or draw aliases g");
  a.stats = const_cast<float*>(stats), a.g = g, a.dpenalty = dpenalty, a.draw = draw;
  return hip_tail(launch_actreg_bwd(a, (hipStream_t)stream));
}

// ---- decoding the LM (vmlmf_sample.hip) ----
size_t vmlmf_lm_sample_workspace_bytes(int B, int V) { return (B < 1 || V < 1) ? 0 : lm_sample_workspace_bytes(B, V); }
size_t vmlmf_lm_sample_filtered_workspace_bytes(int B, int V) { return (B < 1 || V < 1) ? 0 : lm_sample_filtered_workspace_bytes(B, V); }

}  // extern "C"

namespace {

// "<entry point>: <text>" (one copy of the string work for all the refusals below)
__attribute__((noinline)) int refuse(int code, const char* name, const char* text) { return fail(code, std::string(name) + ": " + text); }

// what both forms of the sampler step refuse (vmlmf_refusals.h), under the entry point's name
int sampler_and_filter_refusal(const char* name, int B, float inv_temperature, int top_k, float top_p, const void* state, const void* embed,
                               const void* x_next, int step) {
  const auto named = [name](int code, const char* text) { return refuse(code, name, text); };
  if (int rc = sampler_refusal(named, B, inv_temperature, state, embed, x_next, step)) return rc;
  return filter_refusal(named, top_k, top_p);
}
// the launch where no selection runs (filters off, or greedy: the argmax is always kept) writes no counts: the whole row then
int kept_is_the_row(int B, int V, float inv_temperature, int top_k, float top_p, int32_t* kept_out, hipStream_t s) {
  if (kept_out == nullptr || (inv_temperature > 0.f && (top_k > 0 || top_p < 1.f))) return 0;
  return (int)hipMemsetD32Async((hipDeviceptr_t)kept_out, V, (size_t)B, s);
}

int lm_sample_entry(const char* name, size_t need, int B, int H, int V, const float* h, const float* weight, const float* bias,
                    const float* embed, float inv_temperature, int top_k, float top_p, const int64_t* state, int step, int64_t* tokens_out,
                    float* logprob_out, float* x_next, int32_t* kept_out, int64_t* ticket, void* workspace, size_t workspace_bytes,
                    void* stream) {
  if (B < 1 || H < 1 || V < 1) return refuse(VMLMF_E_BADARG, name, "B, H, V must be >= 1");
  if (!h || !weight || !tokens_out || !ticket || !workspace) return refuse(VMLMF_E_BADARG, name, "null pointer");
  if (int rc = sampler_and_filter_refusal(name, B, inv_temperature, top_k, top_p, state, embed, x_next, step)) return rc;
  if (workspace_bytes < need) return fail(VMLMF_E_WORKSPACE, std::string(name) + ": workspace smaller than vmlmf_" + name + "_workspace_bytes()");
  LmSampleArgs a;
  memset(&a, 0, sizeof(a));
  a.h = h, a.w = weight, a.bias = bias, a.embed = embed;
  a.state = reinterpret_cast<const unsigned long long*>(state);
  a.tokens = reinterpret_cast<long long*>(tokens_out), a.logprob = logprob_out, a.x_next = x_next;
  a.part = static_cast<float*>(workspace), a.ticket = reinterpret_cast<unsigned long long*>(ticket);
  a.inv_temp = inv_temperature, a.B = B, a.H = H, a.V = V, a.step = step;
  a.top_k = top_k >= V ? 0 : top_k, a.top_p = top_p, a.kept = kept_out;
  if (int rc = kept_is_the_row(B, V, inv_temperature, a.top_k, top_p, kept_out, (hipStream_t)stream)) return hip_tail(rc);
  return hip_tail(launch_lm_sample(a, (hipStream_t)stream));
}

int lm_choose_entry(const char* name, int B, int H, int V, const float* scores, const float* bias, const float* embed,
                    float inv_temperature, int top_k, float top_p, const int64_t* state, int step, int64_t* tokens_out, float* logprob_out,
                    float* x_next, int32_t* kept_out, void* stream) {
  if (B < 1 || V < 1 || (x_next && H < 1)) return refuse(VMLMF_E_BADARG, name, "B, V (and H with x_next) must be >= 1");
  if (!scores || !tokens_out) return refuse(VMLMF_E_BADARG, name, "null pointer");
  if (int rc = sampler_and_filter_refusal(name, B, inv_temperature, top_k, top_p, state, embed, x_next, step)) return rc;
  LmChooseArgs a;
  memset(&a, 0, sizeof(a));
  a.scores = scores, a.bias = bias, a.embed = embed, a.state = reinterpret_cast<const unsigned long long*>(state);
  a.tokens = reinterpret_cast<long long*>(tokens_out), a.logprob = logprob_out, a.x_next = x_next;
  a.inv_temp = inv_temperature, a.B = B, a.H = H, a.V = V, a.step = step;
  a.top_k = top_k >= V ? 0 : top_k, a.top_p = top_p, a.kept = kept_out;
  if (int rc = kept_is_the_row(B, V, inv_temperature, a.top_k, top_p, kept_out, (hipStream_t)stream)) return hip_tail(rc);
  return hip_tail(launch_lm_choose(a, (hipStream_t)stream));
}

}  // namespace

extern "C" {

int vmlmf_lm_sample(int B, int H, int V, const float* h, const float* weight, const float* bias, const float* embed, float inv_temperature,
                    const int64_t* state, int step, int64_t* tokens_out, float* logprob_out, float* x_next, int64_t* ticket, void* workspace,
                    size_t workspace_bytes, void* stream) {
  return lm_sample_entry("lm_sample", B < 1 || V < 1 ? 0 : lm_sample_workspace_bytes(B, V), B, H, V, h, weight, bias, embed, inv_temperature,
                         0, 1.f, state, step, tokens_out, logprob_out, x_next, nullptr, ticket, workspace, workspace_bytes, stream);
}

int vmlmf_lm_sample_filtered(int B, int H, int V, const float* h, const float* weight, const float* bias, const float* embed,
                             float inv_temperature, int top_k, float top_p, const int64_t* state, int step, int64_t* tokens_out,
                             float* logprob_out, float* x_next, int32_t* kept_out, int64_t* ticket, void* workspace, size_t workspace_bytes,
                             void* stream) {
  return lm_sample_entry("lm_sample_filtered", B < 1 || V < 1 ? 0 : lm_sample_filtered_workspace_bytes(B, V), B, H, V, h, weight, bias, embed,
                         inv_temperature, top_k, top_p, state, step, tokens_out, logprob_out, x_next, kept_out, ticket, workspace,
                         workspace_bytes, stream);
}

int vmlmf_lm_choose(int B, int H, int V, const float* scores, const float* bias, const float* embed, float inv_temperature,
                    const int64_t* state, int step, int64_t* tokens_out, float* logprob_out, float* x_next, void* stream) {
  return lm_choose_entry("lm_choose", B, H, V, scores, bias, embed, inv_temperature, 0, 1.f, state, step, tokens_out, logprob_out, x_next,
                         nullptr, stream);
}

int vmlmf_lm_choose_filtered(int B, int H, int V, const float* scores, const float* bias, const float* embed, float inv_temperature,
                             int top_k, float top_p, const int64_t* state, int step, int64_t* tokens_out, float* logprob_out, float* x_next,
                             int32_t* kept_out, void* stream) {
  return lm_choose_entry("lm_choose_filtered", B, H, V, scores, bias, embed, inv_temperature, top_k, top_p, state, step, tokens_out,
                         logprob_out, x_next, kept_out, stream);
}

int vmlmf_transpose(int rows, int cols, const float* src, float* dst, void* stream) {
  if (rows < 1 || cols < 1) return fail(VMLMF_E_BADARG, "transpose: rows, cols must be >= 1");
  if (!src || !dst || src == dst) return fail(VMLMF_E_BADARG, "transpose: two distinct buffers");
  return hip_tail(launch_transpose(rows, cols, src, dst, (hipStream_t)stream));
}

}  // extern "C"
