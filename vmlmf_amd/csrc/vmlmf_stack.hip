// Stacked layers of the C ABI: the wavefront launches (vmlmf_wave.inc) and the clustered form (vmlmf_rbx.hip).
#include "vmlmf_host.h"

using namespace vmlmf_host;

namespace {
struct StackPlan {
  int L;
  bool rbx;    // the clustered form (vmlmf_rbx.hip): every layer on clusters of workgroups, all layers in one launch per direction
  RbGeo q;     // ... its geometry (all layers alike)
  VGeo g[WF_MAXL];
  VPack P[WF_MAXL];
  WfPack W;
  Layout lay[WF_MAXL];
  long long ws_flag, ws_layer[WF_MAXL], ws_dx[WF_MAXL], ws_total;   // float offsets in the workspace
  long long flag_words;
};
const HeadBwd NO_HEAD = {};   // no classifier riding on a launch (C = 0)

// what the layers of either form share: layer l against layer 0
static bool same_frame(const VGeo& g, const VGeo& g0) {
  return g.variant == g0.variant && g.B == g0.B && g.T == g0.T && g.rw == g0.rw && g.ru0 == g0.ru0 && g.ru1 == g0.ru1 && g.G == g0.G &&
         g.time_major == g0.time_major && g.training == g0.training;
}
// every layer's image and buffer layouts, and the workspace: [o: what the form keeps in front] then, per layer, its own piece and its dx
static void stack_offsets(StackPlan& S, long long o) {
  for (int l = 0; l < S.L; ++l) {
    S.P[l] = vg_pack_layout(S.g[l], S.q.total, S.W.total);
    S.lay[l] = make_layout(S.g[l], S.P[l], S.q);
    const long long per = S.lay[l].ws_total();
    S.ws_layer[l] = o, o += align64(per);
    S.ws_dx[l] = o, o += align64(l > 0 ? (long long)S.g[0].T * S.g[0].B * S.g[l].I : 0);   // dx of layer l = dy of layer l - 1
  }
  S.ws_total = o;
}

// layers on clusters of workgroups (factors beyond one CU): the clustered form, or nothing.  g0: layer 0's geometry as a layer call's
static int plan_clustered(int L, const vmlmf_stack_layer* ly, const VGeo& g0, StackPlan& S) {
  if (!g_rbx) return fail(VMLMF_E_UNSUPPORTED, "stack: the clustered form is switched off (VMLMF_RBX=0)");
  if (L < 2 && g_rbx != 2) return fail(VMLMF_E_UNSUPPORTED, "stack: a single clustered layer runs as vmlmf_seq_forward");
  if (L > RBX_MAXL) return fail(VMLMF_E_UNSUPPORTED, "stack: at most four clustered layers");
  for (int l = 0; l < L; ++l) {
    RbGeo ql;
    vmlmf_desc dd = ly[l].desc;
    const int rc = make_geo(&dd, &S.g[l], &ql);
    if (rc != 0) return rc;
    const VGeo& g = S.g[l];
    if (!same_frame(g, g0) || g.H != g0.H || g.I != g0.I || dd.dtype != VMLMF_DT_F32 || g.rb != g0.rb)
      return fail(VMLMF_E_UNSUPPORTED, "stack: layers must agree in variant, B, T, sizes, ranks, layout and training flag");
    if (g.I != g.H || !g.time_major || g.sxT != g.syT || g.sxB != g.syB)
      return fail(VMLMF_E_UNSUPPORTED, "stack (clustered form): time-major layers with input_size == hidden_size");
  }
  // live rows per workgroup: the fewest (4, 8, 16) with which the clusters of ALL layers are co-resident, one workgroup per CU
  const int cus = device_cus();
  bool found = false;
  for (int rows = 4; rows <= 16 && !found; rows *= 2) {
    RbGeo q;
    if (!rb_geometry(g0, g0.rb, &q, rows, 1) || !rbx_supported(g0, q)) continue;
    if ((long long)L * q.nrb * q.S > cus) continue;
    S.q = q, found = true;
  }
  if (!found)
    return fail(VMLMF_E_UNSUPPORTED, "stack (clustered form): V3 / V4 layers with w_rank 17..32 whose clusters are co-resident for all layers "
                                     "(L x ceil(B / 16) x 16 workgroups <= CUs)");
  S.rbx = true;
  S.flag_words = 0;
  memset(&S.W, 0, sizeof(S.W));
  S.ws_flag = 0;
  stack_offsets(S, 0);
  return 0;
}

static int plan_wavefront(int L, const vmlmf_stack_layer* ly, StackPlan& S) {
  // layers of a stack may differ in hidden_size (MyLSTM builds any hidden_layer_sizes, vmlmf.py:283-292; a VMLMF cell needs input_size
  // <= hidden_size, vmlmf.py:94, so the sizes cannot shrink): every layer then runs on the widest layer's wave count
  int Wmax = 0;
  for (int l = 0; l < L; ++l) {
    RbGeo q;
    VGeo gl;
    vmlmf_desc dd = ly[l].desc;
    if (dd.dtype == VMLMF_DT_BF16) dd.dtype = VMLMF_DT_F32;
    const int rc = make_geo(&dd, &gl, &q);
    if (rc != 0) return rc;
    Wmax = gl.W > Wmax ? gl.W : Wmax;
  }
  for (int l = 0; l < L; ++l) {
    RbGeo q;
    // dtype bf16 on a stack: below the batch where the bf16-MFMA row blocks pay (4096 rows: DESIGN.md section 4.8) the wavefront
    // kernels run it with fp32 arithmetic and a bf16 GATE TAPE (VGeo::bt: half the tape bytes written and read back; one-group
    // layers of padded rank 16 / 24); from there on, and for the layers those instantiations do not cover, the caller chains the
    // row-block kernels (VMLMF_E_UNSUPPORTED here)
    vmlmf_desc dd = ly[l].desc;
    const bool bt = dd.dtype == VMLMF_DT_BF16;
    if (bt) {
      if (dd.B >= 4096) return fail(VMLMF_E_UNSUPPORTED, "stack: dtype bf16 at 4096 rows and more runs the row-block bf16-MFMA kernels layer by layer");
      dd.dtype = VMLMF_DT_F32;
    }
    const int rc = make_geo(&dd, &S.g[l], &q, Wmax);
    if (rc != 0) return rc;
    if (bt) {
      const int K = wf_width(S.g[l]);
      if (S.g[l].G != 1 || !(K == 16 || K == 24) || !g_wf_bwd)
        return fail(VMLMF_E_UNSUPPORTED, "stack: the bf16 gate tape covers one-group layers of padded rank 16 / 24");
      S.g[l].bt = 1;
    }
    const VGeo& g = S.g[l];
    if (!wf_supported(g))
      return fail(VMLMF_E_UNSUPPORTED, "stack: layer not covered by the wavefront kernels (V1-V3, V5, V6; at most four waves of hidden units; padded ranks "
                                       "<= 24, or 32 with at most three waves; fp32)");
    if (l > 0) {
      const VGeo& g0 = S.g[0];
      if (!same_frame(g, g0) || g.KH != g0.KH || g.KX != g0.KX || g.bt != g0.bt || g.W != g0.W)
        return fail(VMLMF_E_UNSUPPORTED, "stack: layers must agree in variant, B, T, ranks, layout and training flag");
      if (g.I != S.g[l - 1].H) return fail(VMLMF_E_SHAPE, "stack: layer l > 0 reads the layer below: its input_size must equal that layer's hidden_size");
      if (g.H != g0.H && (g.bt || g.G != 1 || g.KH != g.KX))
        return fail(VMLMF_E_UNSUPPORTED, "stack: layers of different hidden sizes: one-group layers, fp32 tapes, equal padded ranks on both sides");
    }
  }
  {   // the batched weight-gradient launch of these stacks holds one workgroup per CU: few enough chunks for one round (vmlmf_wgrad4.hip)
    const int rc2 = wgrad4_chunk_rows(L, S.g, device_cus());
    if (rc2 > 0)
      for (int l = 0; l < L; ++l) {
        const int TB = S.g[l].T * S.g[l].B;
        S.g[l].RC2 = rc2, S.g[l].nchunk = (TB + rc2 - 1) / rc2;
      }
  }
  S.W = wf_pack_layout(S.g[0]);
  memset(&S.q, 0, sizeof(S.q));
  S.flag_words = ((long long)(L > 1 ? L - 1 : 0) * S.g[0].B + 1) * WF_FLAG_STRIDE;
  S.ws_flag = 0;
  stack_offsets(S, align64(S.flag_words));
  return 0;
}

static int stack_plan(int L, const vmlmf_stack_layer* ly, StackPlan* out) {
  if (ly == nullptr) return fail(VMLMF_E_BADARG, "stack: null layers");
  if (L < 1 || L > WF_MAXL) return fail(VMLMF_E_UNSUPPORTED, "stack: 1..4 layers");
  out->L = L;
  out->rbx = false;
  RbGeo q0;
  vmlmf_desc d0 = ly[0].desc;
  VGeo g0;
  if (d0.dtype == VMLMF_DT_F32 && make_geo(&d0, &g0, &q0) == 0 && g0.generic && g0.rb > 1) return plan_clustered(L, ly, g0, *out);
  return plan_wavefront(L, ly, *out);
}
// layer l's input: x, or the rows of the layer below - their dropped copy under dropout (vmlmf_lm.py:438-439)
static const float* stack_input(const vmlmf_stack_layer* ly, int l, const float* x) {
  return l == 0 ? x : (ly[l - 1].drop != nullptr ? ly[l - 1].drop->y_dropped : ly[l - 1].y);
}
// the batched half of layer l's backward through the per-layer launches
static int stack_tail(const StackPlan& S, const vmlmf_stack_layer* ly, int l, const float* x, float* ws, hipStream_t s) {
  return backward_tail(S.g[l], plan_layer(S.g[l], ly[l].params, false, false, false, PLAN_CHAINED), S.lay[l], ly[l].params, ly[l].grads,
                       stack_input(ly, l, x), ly[l].y, ly[l].h0, (const float*)ly[l].reserve, ws + S.ws_layer[l], NO_HEAD, s);
}
// layer l's pointers: a forward checks them layer by layer, between the layers' dropout arguments; a backward checks all layers first
static int check_stack_layer(const StackPlan& S, const vmlmf_stack_layer* ly, int l, bool forward) {
  int rc;
  if ((rc = check_params(S.g[l], ly[l].params)) != 0) return rc;
  if (forward) {
    if (ly[l].y == nullptr) return fail(VMLMF_E_BADARG, "stack: null y");
    if (S.g[0].training && ly[l].reserve == nullptr) return fail(VMLMF_E_BADARG, "stack: training forward needs the layers' reserve buffers");
    return 0;
  }
  if ((rc = check_grads(S.g[l], ly[l].grads)) != 0) return rc;
  if (ly[l].y == nullptr || ly[l].reserve == nullptr) return fail(VMLMF_E_BADARG, "stack: null y / reserve");
  return 0;
}
static int check_stack_layers(const StackPlan& S, const vmlmf_stack_layer* ly) {   // (a backward's)
  for (int l = 0, rc; l < S.L; ++l)
    if ((rc = check_stack_layer(S, ly, l, false)) != 0) return rc;
  return 0;
}

// The finishing ladder of a stack's backward, from the layers' partial blocks (wparts) to the reference-layout gradients: one launch
// where it covers the layers, else - `ffb`, the caller's rule: the two forms read VMLMF_FFB differently - the finishing launch summing
// the blocks itself, else reduce + finish.  wcs: the chunk counts of the layers' wgrad_ring_kernel launches (clustered form), or NULL
static int finish_stack_gradients(const StackPlan& S, const vmlmf_stack_layer* ly, float* ws, const HeadBwd& hb_top, const ReduceCounts* wcs,
                                  bool ffb, hipStream_t s) {
  const int L = S.L;
  int rc;
  RefP rps[WF_MAXL];
  RefG ogs[WF_MAXL];
  const float* wparts[WF_MAXL];
  float* cgs[WF_MAXL];
  const float* ccgs[WF_MAXL];
  bool fu = g_finish_units;
  for (int l = 0; l < L; ++l) {
    float* wl = ws + S.ws_layer[l];
    wparts[l] = wl + S.lay[l].b_wpart, ccgs[l] = cgs[l] = wl + S.lay[l].b_cgrad;
    rps[l] = to_refp(ly[l].params), ogs[l] = to_refg(ly[l].grads);
    fu = fu && finish_units_ok(S.g[l]);
  }
  if (fu)   // a workgroup per hidden unit sums that unit's partial sums once and finishes its gradient entries
    return run(SL_FINISH, s, "finish", [&] { return launch_finish_units_stack(L, S.g, rps, ogs, hb_top, s, health_word(s), wparts, wcs); });
  if (ffb) return run(SL_FINISH, s, "finish", [&] { return launch_finish_stack(L, S.g, rps, ccgs, ogs, hb_top, s, health_word(s), wparts, wcs); });
  if ((rc = run(SL_REDUCE, s, "reduce", [&] { return launch_reduce_stack(L, S.g, wparts, cgs, s, wcs); })) != 0) return rc;
  return run(SL_FINISH, s, "finish", [&] { return launch_finish_stack(L, S.g, rps, ccgs, ogs, hb_top, s, health_word(s)); });
}

// ---- the clustered form (vmlmf_rbx.hip)
static_assert(RBX_MAXL <= WF_MAXL, "finish_stack_gradients sizes its per-layer arrays by WF_MAXL");
static int rbx_stack_forward(const StackPlan& S, const vmlmf_stack_layer* ly, const float* x, float* ws, hipStream_t s) {
  const int L = S.L;
  const bool training = S.g[0].training != 0;
  int rc;
  RbxFwdArgs a;
  memset(&a, 0, sizeof(a));
  a.status = status_word(s), a.L = L;
  RefP rps[RBX_MAXL];
  float* packs[RBX_MAXL];
  float* imgs[RBX_MAXL];
  unsigned* fflags[RBX_MAXL];
  for (int l = 0; l < L; ++l) {
    if ((rc = check_stack_layer(S, ly, l, true)) != 0) return rc;
    float* rs = (float*)ly[l].reserve;
    const Layout& Lr = S.lay[l];
    float* wl = ws + S.ws_layer[l];
    float* pack = training ? rs + Lr.r_pack : wl + Lr.f_pack;
    rps[l] = to_refp(ly[l].params), packs[l] = pack, imgs[l] = pack + S.P[l].RB, fflags[l] = reinterpret_cast<unsigned*>(wl + Lr.f_flag);
    RbxLayerF& w = a.l[l];
    if ((rc = site_drop(ly[l].drop, true, S.g[0].B, &w.drop)) != 0) return rc;
    w.x = stack_input(ly, l, x);
    w.EH = pack + S.P[l].EH, w.EXT = pack + S.P[l].EXT, w.BBT = pack + S.P[l].BBT, w.img = pack + S.P[l].RB;
    w.h0 = ly[l].h0, w.c0 = ly[l].c0, w.y = ly[l].y, w.hT = ly[l].hT, w.cT = ly[l].cT;
    w.gates = training ? rs + Lr.r_gates : nullptr, w.cs = training ? rs + Lr.r_cs : nullptr;
    w.Qs = training ? rs + Lr.r_Qs : nullptr, w.qx = training ? rs + Lr.r_qx : nullptr;
    w.xq = wl + Lr.f_xq, w.flag = reinterpret_cast<unsigned*>(wl + Lr.f_flag);
    w.pflag = l > 0 ? reinterpret_cast<unsigned*>(ws + S.ws_layer[l - 1] + S.lay[l - 1].f_flag) : nullptr;
    w.pub = l < L - 1 ? 1 : 0;
  }
  {   // every layer's parameter images in two launches (pack_kernel's for all layers, the clusters' MFMA operand images for all
      // layers; the second also clears the forward launch's epoch words)
    Scope sc(SL_PACK, s);
    WfPack W0;
    memset(&W0, 0, sizeof(W0));
    if ((rc = hip_fail(launch_pack_stack(L, S.g, rps, S.P, W0, packs, nullptr, 0, nullptr, 0, s, PACK_CLUSTERED), "pack")) != 0) return rc;
    if ((rc = hip_fail(launch_rb_pack_stack(S.g[0], S.q, L, rps, imgs, fflags, s), "rb_pack")) != 0) return rc;
  }
  return run(SL_REC_FWD, s, "rbx_fwd", [&] { return launch_rbx_fwd(S.g[0], S.q, a, s); });
}

static int rbx_stack_backward(const StackPlan& S, const vmlmf_stack_layer* ly, const float* x, const float* dy, float* dx, float* ws,
                              hipStream_t s) {
  const int L = S.L;
  int rc;
  if ((rc = check_stack_layers(S, ly)) != 0) return rc;
  RbxBwdArgs a;
  memset(&a, 0, sizeof(a));
  a.status = status_word(s), a.L = L;
  float* dpres[RBX_MAXL];
  unsigned* flags[RBX_MAXL];
  for (int l = 0; l < L; ++l) {
    const Layout& Lr = S.lay[l];
    const float* rs = (const float*)ly[l].reserve;
    const float* pack = rs + Lr.r_pack;
    float* wl = ws + S.ws_layer[l];
    RbxLayerB& w = a.l[L - 1 - l];   // launch position 0 is the top layer: the producer comes first in the grid
    if ((rc = site_drop(ly[l].drop, false, S.g[0].B, &w.drop)) != 0) return rc;
    w.gates = rs + Lr.r_gates, w.cs = rs + Lr.r_cs, w.EH = pack + S.P[l].EH, w.EXT = pack + S.P[l].EXT, w.img = pack + S.P[l].RB;
    w.dy = l == L - 1 ? dy : ws + S.ws_dx[l + 1];
    w.dhT = ly[l].dhT, w.dcT = ly[l].dcT, w.dh0 = ly[l].dh0, w.dc0 = ly[l].dc0;
    w.dpre = wl + Lr.b_dpre, w.dQs = wl + Lr.b_dQs, w.dqx = wl + Lr.b_dqx;
    w.dx = l == 0 ? dx : ws + S.ws_dx[l];
    w.xq = wl + Lr.b_xq, w.flag = reinterpret_cast<unsigned*>(wl + Lr.b_flag);
    w.pflag = l < L - 1 ? reinterpret_cast<unsigned*>(ws + S.ws_layer[l + 1] + S.lay[l + 1].b_flag) : nullptr;
    w.pub = l > 0 ? 1 : 0;
    dpres[l] = wl + Lr.b_dpre, flags[l] = reinterpret_cast<unsigned*>(wl + Lr.b_flag);
  }
  {   // (one scope over both launches)
    Scope sc(SL_REC_BWD, s);
    if ((rc = hip_fail(launch_rbx_zero(S.g[0], S.q, L, dpres, flags, s), "rbx_zero")) != 0) return rc;
    if ((rc = hip_fail(launch_rbx_bwd(S.g[0], S.q, a, s), "rbx_bwd")) != 0) return rc;
  }
  // the batched half of every layer: weight-gradient products (per layer: the ring kernel fills the chip), then ONE launch that sums
  // every layer's partial blocks and ONE that writes every layer's reference-layout gradients
  const bool ring = g_wring != 0 && wgrad_ring_ok(S.g[0]) && (g_wring > 0 || (long long)S.g[0].T * S.g[0].B >= 1024);
  if (!ring) {
    for (int l = L - 1; l >= 0; --l)
      if ((rc = stack_tail(S, ly, l, x, ws, s)) != 0) return rc;
    return 0;
  }
  ReduceCounts wcs[RBX_MAXL];
  for (int l = L - 1; l >= 0; --l) {
    const WghArgs wh = wgrad_args(S.lay[l], stack_input(ly, l, x), ly[l].y, ly[l].h0, (const float*)ly[l].reserve, ws + S.ws_layer[l]);
    int nc[3] = {0, 0, 0};
    Scope sc(SL_WGRAD, s);   // (covers the fallback's launches too)
    const int rr = launch_wgrad_ring(S.g[l], wh, device_cus(), nc, s);
    if (rr == 0) ++g_ring_launches;
    if (rr == -3) {   // no LDS / instantiation for the ring on this device: the per-layer path for every layer from here
      for (int k = l; k >= 0; --k)
        if ((rc = stack_tail(S, ly, k, x, ws, s)) != 0) return rc;
      // (the layers above l: their blocks are formed, finish them one by one)
      for (int k = L - 1; k > l; --k) {
        float* wk = ws + S.ws_layer[k];
        float* cg = wk + S.lay[k].b_cgrad;
        if ((rc = run(SL_REDUCE, s, "reduce", [&] { return launch_reduce(S.g[k], wk + S.lay[k].b_wpart, cg, nullptr, s, wcs[k]); })) != 0) return rc;
        if ((rc = run(SL_FINISH, s, "finish", [&] {
               return launch_finish(S.g[k], to_refp(ly[k].params), cg, to_refg(ly[k].grads), NO_HEAD, s, health_word(s));
             })) != 0) return rc;
      }
      return 0;
    }
    if ((rc = hip_fail(rr, "wgrad")) != 0) return rc;
    wcs[l] = ReduceCounts{{nc[0], nc[1], nc[2]}};
  }
  // ffb: any non-zero VMLMF_FFB - the ring kernel leaves few partial blocks; the layers are all alike, so layer 0 answers for them
  return finish_stack_gradients(S, ly, ws, NO_HEAD, wcs, g_ffb != 0 && finish_from_blocks_ok(S.g[0]), s);
}
}  // namespace

extern "C" {

int vmlmf_stack_dropout_fused(int L, const vmlmf_stack_layer* layers) {
  StackPlan S;
  if (stack_plan(L, layers, &S) != 0) return 0;
  return (S.rbx || (S.g[0].G == 1 && g_wf_bwd)) ? 1 : 0;   // the clustered form; the wavefront launches for one-group layers
}

int vmlmf_stack_query(int L, const vmlmf_stack_layer* layers, size_t* reserve_bytes, size_t* workspace_bytes) {
  StackPlan S;
  const int rc = stack_plan(L, layers, &S);
  if (rc != 0) return rc;
  for (int l = 0; l < L; ++l)   // (layer 0's reserve ends with the progress words of the backward launch: the forward clears them)
    if (reserve_bytes != nullptr) reserve_bytes[l] = (size_t)(S.lay[l].r_total + (l == 0 ? align64(S.flag_words) : 0)) * sizeof(float);
  if (workspace_bytes != nullptr) *workspace_bytes = (size_t)S.ws_total * sizeof(float);
  return 0;
}

int vmlmf_stack_forward(int L, const vmlmf_stack_layer* ly, const float* x, const vmlmf_head* head_in, void* workspace,
                        size_t workspace_bytes, void* stream) {
  StackPlan S;
  int rc = take_status();
  if (rc != 0) return rc;
  if ((rc = stack_plan(L, ly, &S)) != 0) return rc;
  if (x == nullptr || workspace == nullptr) return fail(VMLMF_E_BADARG, "stack: null x / workspace");
  const vmlmf_head* head = (head_in != nullptr && head_in->classes != 0) ? head_in : nullptr;
  if ((rc = check_head(S.g[L - 1], head, true)) != 0) return rc;
  if (workspace_bytes < (size_t)S.ws_total * sizeof(float)) return fail(VMLMF_E_WORKSPACE, "stack: workspace smaller than vmlmf_stack_query() reported");
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const bool training = S.g[0].training != 0;
  if (S.rbx) {
    if (head != nullptr) return fail(VMLMF_E_UNSUPPORTED, "stack (clustered form): no classifier head");
    return rbx_stack_forward(S, ly, x, ws, s);
  }
  for (int l = 0; l < L; ++l)
    if (ly[l].drop != nullptr && S.g[0].G != 1)
      return fail(VMLMF_E_UNSUPPORTED, "stack: dropout inside the wavefront launches for one-group layers (vmlmf_stack_dropout_fused)");
  WfFwdArgs a;
  memset(&a, 0, sizeof(a));
  a.c.flag = reinterpret_cast<unsigned*>(ws + S.ws_flag), a.c.L = L, a.c.status = status_word(s);
  if (head != nullptr) a.hd.W = head->weight, a.hd.bias = head->bias, a.hd.logits = head->logits, a.hd.C = head->classes;
  RefP rps[WF_MAXL];
  float* packs[WF_MAXL];
  for (int l = 0; l < L; ++l) {
    const VGeo& g = S.g[l];
    if ((rc = check_stack_layer(S, ly, l, true)) != 0) return rc;
    float* rs = (float*)ly[l].reserve;
    const Layout& Lr = S.lay[l];
    float* pack = training ? rs + Lr.r_pack : ws + S.ws_layer[l] + Lr.f_pack;
    rps[l] = to_refp(ly[l].params), packs[l] = pack;
    WfFwdLayer& w = a.l[l];
    w.x = stack_input(ly, l, x);
    if ((rc = site_drop(ly[l].drop, true, S.g[0].B, &a.drop[l])) != 0) return rc;
    w.sxT = g.sxT, w.sxB = g.sxB, w.I = g.I;
    w.syT = g.syT, w.syB = g.syB, w.H = g.H, w.Hg = g.Hg;
    const bool mixed = g.KH != g.KX;   // both sides at the wider padded rank: re-laid images in the WF region
    const float* wf = pack + S.P[l].WF;
    w.VE = mixed ? wf + S.W.VE : pack + S.P[l].VE, w.VXT = mixed ? wf + S.W.VXK : pack + S.P[l].VXT;
    w.EH = pack + S.P[l].EH, w.EXT = pack + S.P[l].EXT, w.BBT = pack + S.P[l].BBT;
    w.UR = wf + S.W.UR, w.URX = wf + S.W.URX;
    w.h0 = ly[l].h0, w.c0 = ly[l].c0, w.y = ly[l].y, w.hT = ly[l].hT, w.cT = ly[l].cT;
    w.gates = training ? rs + Lr.r_gates : nullptr, w.cs = training ? rs + Lr.r_cs : nullptr;
    w.Qs = training ? rs + Lr.r_Qs : nullptr, w.qx = training ? rs + Lr.r_qx : nullptr;
  }
  // one launch: every layer's parameter images, and the progress words of this launch and of the backward one cleared
  unsigned* z0 = L > 1 ? reinterpret_cast<unsigned*>(ws + S.ws_flag) : nullptr;
  unsigned* z1 = (L > 1 && training) ? reinterpret_cast<unsigned*>((float*)ly[0].reserve + S.lay[0].r_total) : nullptr;
  if ((rc = run(SL_PACK, s, "pack", [&] {
         return launch_pack_stack(L, S.g, rps, S.P, S.W, packs, z0, (int)S.flag_words, z1, (int)S.flag_words, s,
                                  (g_wf_bwd && g_pack_slim) ? PACK_WAVEFRONT : PACK_ALL);
       })) != 0) return rc;
  return run(SL_REC_FWD, s, "wf_fwd", [&] { return launch_wf_fwd(S.g[0], a, s); });
}

int vmlmf_stack_backward(int L, const vmlmf_stack_layer* ly, const float* x, const float* dy, float* dx,
                         const vmlmf_head* head_in, void* workspace, size_t workspace_bytes, void* stream) {
  StackPlan S;
  int rc = take_status();
  if (rc != 0) return rc;
  if ((rc = stack_plan(L, ly, &S)) != 0) return rc;
  if (x == nullptr || workspace == nullptr) return fail(VMLMF_E_BADARG, "stack: null x / workspace");
  const vmlmf_head* head = (head_in != nullptr && head_in->classes != 0) ? head_in : nullptr;
  if ((rc = check_head(S.g[L - 1], head, false)) != 0) return rc;
  if (workspace_bytes < (size_t)S.ws_total * sizeof(float)) return fail(VMLMF_E_WORKSPACE, "stack: workspace smaller than vmlmf_stack_query() reported");
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  if ((rc = check_stack_layers(S, ly)) != 0) return rc;
  const HeadBwd hb_top = head_bwd_args(head, S.g[L - 1], ly[L - 1].y);   // the classifier on the top layer
  if (S.rbx) {
    if (head != nullptr) return fail(VMLMF_E_UNSUPPORTED, "stack (clustered form): no classifier head");
    return rbx_stack_backward(S, ly, x, dy, dx, ws, s);
  }
  const bool wave = g_wf_bwd;
  for (int l = 0; l < L; ++l)
    if (!wave && ly[l].drop != nullptr) return fail(VMLMF_E_UNSUPPORTED, "stack: dropout rides on the wavefront backward only (VMLMF_WF_BWD=0 is an A/B switch)");
  if (!wave && head != nullptr) return fail(VMLMF_E_UNSUPPORTED, "stack: the classifier rides on the wavefront backward only (VMLMF_WF_BWD=0 is an A/B switch)");
  if (wave) {
    WfBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.c.flag = reinterpret_cast<unsigned*>((float*)ly[0].reserve + S.lay[0].r_total), a.c.L = L, a.c.status = status_word(s);   // cleared by the forward
    a.hd = hb_top;
    for (int l = 0; l < L; ++l) {
      const VGeo& g = S.g[l];
      const Layout& Lr = S.lay[l];
      const float* rs = (const float*)ly[l].reserve;
      const float* pack = rs + Lr.r_pack;
      float* wl = ws + S.ws_layer[l];
      WfBwdLayer& w = a.l[L - 1 - l];   // launch position 0 is the top layer
      if ((rc = site_drop(ly[l].drop, false, S.g[0].B, &a.drop[L - 1 - l])) != 0) return rc;
      if (ly[l].drop != nullptr && S.g[0].G != 1) return fail(VMLMF_E_UNSUPPORTED, "stack: dropout inside the wavefront launches for one-group layers");
      w.gates = rs + Lr.r_gates, w.cs = rs + Lr.r_cs;
      w.dy = l == L - 1 ? dy : ws + S.ws_dx[l + 1];
      w.dhT = ly[l].dhT, w.dcT = ly[l].dcT, w.dh0 = ly[l].dh0, w.dc0 = ly[l].dc0;
      const bool mixed = g.KH != g.KX;
      const float* wf = pack + S.P[l].WF;
      w.UE = mixed ? wf + S.W.UE : pack + S.P[l].UE, w.UXO = mixed ? wf + S.W.UXK : pack + S.P[l].UXO;
      w.EH = pack + S.P[l].EH, w.EXI = pack + S.P[l].EXI;
      w.VR = wf + S.W.VR, w.VRX = wf + S.W.VRX;
      w.dpre = wl + Lr.b_dpre, w.dQs = wl + Lr.b_dQs, w.dqx = wl + Lr.b_dqx;
      w.dx = l == 0 ? dx : ws + S.ws_dx[l];
      w.want_dx = w.dx != nullptr ? 1 : 0;
      w.sxT = g.sxT, w.sxB = g.sxB, w.I = g.I;
      w.syT = g.syT, w.syB = g.syB, w.H = g.H, w.Hg = g.Hg;
    }
    if ((rc = run(SL_REC_BWD, s, "wf_bwd", [&] { return launch_wf_bwd(S.g[0], a, s); })) != 0) return rc;
    // the batched half of every layer's backward: one launch each for the whole stack
    WghArgs wh[WF_MAXL];
    for (int l = 0; l < L; ++l)
      wh[l] = wgrad_args(S.lay[l], stack_input(ly, l, x), ly[l].y, ly[l].h0, (const float*)ly[l].reserve, ws + S.ws_layer[l]);
    if ((rc = run(SL_WGRAD, s, "wgrad", [&] { return launch_wgrad_h_stack(L, S.g, wh, s); })) != 0) return rc;
    // ffb: only a positive VMLMF_FFB - wavefront stacks leave 48 - 64 blocks per layer; on only when asked for (measured: DESIGN.md) -
    // and only where the kernel covers every layer (the layers may differ in size)
    bool ffb = g_ffb > 0;
    for (int l = 0; l < L; ++l) ffb = ffb && finish_from_blocks_ok(S.g[l]);
    return finish_stack_gradients(S, ly, ws, hb_top, nullptr, ffb, s);
  }
  for (int l = L - 1; l >= 0; --l) {   // the per-layer kernels, chained through the dx buffers
    const float* rs = (const float*)ly[l].reserve;
    float* wl = ws + S.ws_layer[l];
    float* dxl = l == 0 ? dx : ws + S.ws_dx[l];
    // PLAN_CHAINED: never rec4_bwd_kernel, riding workers or direct mode - the tape is a stack launch's, not a layer call's
    LayerPlan pl = plan_layer(S.g[l], ly[l].params, false, false, dxl != nullptr, PLAN_CHAINED);
    const LayerBwdIo io = {stack_input(ly, l, x), ly[l].y, ly[l].h0, ly[l].c0, l == L - 1 ? dy : ws + S.ws_dx[l + 1], ly[l].dhT, ly[l].dcT,
                           dxl, ly[l].dh0, ly[l].dc0};
    if ((rc = valu_backward(S.g[l], &pl, S.lay[l], S.P[l], rs + S.lay[l].r_pack, ly[l].params, io, NO_HEAD, rs, wl, s)) != 0) return rc;
    if ((rc = backward_tail(S.g[l], pl, S.lay[l], ly[l].params, ly[l].grads, io.x, io.y, io.h0, rs, wl, NO_HEAD, s)) != 0) return rc;
  }
  return 0;
}

}  // extern "C"
