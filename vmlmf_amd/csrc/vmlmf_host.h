// Host-only internals shared by the translation units of the C ABI (include/vmlmf_hip.h): vmlmf_state.hip (process state),
// vmlmf_api.hip (geometry, layout, one layer's plan and its forward / backward), vmlmf_stack.hip (stacks) and vmlmf_ops.hip (the
// thin entry points).  No device code; no kernel source includes this.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/vmlmf_hip.h"
#include "vmlmf_launch.h"

#pragma GCC visibility push(hidden)   // internal to the library: nothing here joins its exported symbols
namespace vmlmf_host {

// ---- error text (vmlmf_state.hip): fail() records the text vmlmf_last_error() returns; hip_fail() maps a launcher's return code
// (0, a hipError_t, or -3: no kernel instantiation) and names the launch; hip_tail() is the thin entry points' form of it
int fail(int code, const std::string& msg);
int hip_fail(int rc, const char* what);
inline int hip_tail(int rc) { return rc == 0 ? 0 : fail(rc, hipGetErrorString((hipError_t)rc)); }

// ---- process-wide switches (vmlmf_state.hip: one row each in g_switches)
extern int g_debug_sync, g_adam_guard, g_xwave, g_wchunks, g_wmin, g_rc, g_wride, g_wride_k, g_wride_maxb, g_wride_lag, g_wride_rc, g_rb_mode,
    g_rb_minB, g_rb_S, g_rb_rows, g_rec3, g_inrow, g_wring, g_direct, g_finish2, g_wf_bwd, g_pack_slim, g_finish_units, g_rbx, g_ffb;
extern int g_wride_spin, g_tune_generation;
extern std::atomic<int> g_wride_tripped;
extern std::atomic<int> g_ring_launches;   // launches of wgrad_ring_kernel by this process (vmlmf_tune_get "wring_launches")

// ---- profiling (bench.py): HIP event pairs around every internal launch, on the launch stream.  The slots and their names
// (vmlmf_kernel_name, vmlmf_profile_read): the order is part of the ABI
enum Slot { SL_PACK, SL_XPROJ, SL_REC_FWD, SL_REC_BWD, SL_DQX_DX, SL_WGRAD, SL_REDUCE, SL_FINISH, SL_HEAD_FWD, SL_HEAD_BWD, SL_CE_FWD,
            SL_CE_BWD, SL_FINISH2, NKERN };
inline const char* kernel_label(int k) {
  static const char* const names[NKERN] = {"pack_kernel",     "xproj_kernel",      "rec_fwd_kernel",   "rec_bwd_kernel",
                                           "dqx_dx_kernel",   "wgrad_mfma_kernel", "reduce_cg_kernel", "finish_kernel",
                                           "head_fwd_kernel", "head_bwd_kernel",   "ce_fwd_kernel",    "ce_bwd_kernel", "finish2_kernel"};
  return (k >= 0 && k < NKERN) ? names[k] : "";
}
struct Prof {
  std::mutex mu;
  unsigned mask = 0;  // bit k: bracket kernel k with an event pair
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[NKERN];
};
extern Prof g_prof;

struct Scope {
  int k;
  hipStream_t s;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  Scope(Slot which, hipStream_t st) : k(which), s(st) {
    if (g_debug_sync) fprintf(stderr, "[vmlmf] launching %s\n", kernel_label(which));
    if ((g_prof.mask >> which) & 1u) {
      // (profiling instrumentation: an event that could not be made or recorded shows up as a missing / zero sample)
      (void)hipEventCreate(&e0);
      (void)hipEventCreate(&e1);
      (void)hipEventRecord(e0, s);
    }
  }
  ~Scope() {
    if (g_debug_sync) {
      const hipError_t e = hipStreamSynchronize(s);
      fprintf(stderr, "[vmlmf] %s done: %s\n", kernel_label(k), hipGetErrorString(e));
    }
    if (e0 != nullptr) {
      (void)hipEventRecord(e1, s);
      std::lock_guard<std::mutex> lk(g_prof.mu);
      g_prof.ev[k].push_back({e0, e1});
    }
  }
};
// one launch under its Scope: `launch` returns the launcher's code (a scope that covers two launches is written out where it stands)
template <class F>
int run(Slot k, hipStream_t s, const char* what, F&& launch) {
  Scope sc(k, s);
  return hip_fail((int)launch(), what);
}

// ---- status and health words, the device (vmlmf_state.hip)
unsigned* status_word(hipStream_t s);
unsigned* health_word(hipStream_t s);
int take_status();
int debug_status(hipStream_t s);
int device_cus();

// ---- geometry and buffer layouts, float offsets (vmlmf_api.hip)
inline long long align64(long long v) { return (v + 63) / 64 * 64; }
int make_geo(const vmlmf_desc* d, VGeo* out, RbGeo* rbout = nullptr, int force_W = 0);
struct Layout {
  // reserve (training) : PACK | qx | gates | cs | Qs
  long long r_pack, r_qx, r_gates, r_cs, r_Qs, r_prog, r_total;
  // forward workspace  : PACK (inference only) | gx
  long long f_pack, f_gx, f_qx, f_trash, f_Qtmp, f_P, f_ccar, f_zeros, f_part, f_xq, f_flag, f_xrows, f_total;
  // backward workspace : dpre | dQs | wpart | cgrad
  long long b_dpre, b_dQs, b_dqx, b_wpart, b_cgrad, b_trash, b_dHrec, b_ehterm, b_dcar, b_part, b_xq, b_flag, b_headdh, b_dux, b_wide, b_total;
  // the ONE workspace size of a layer (vmlmf_query reports it, forward and backward both demand it)
  long long ws_total() const { return f_total > b_total ? f_total : b_total; }
};
Layout make_layout(const VGeo& g, const VPack& P, const RbGeo& q);

inline RefP to_refp(const vmlmf_params* p) {
  RefP r;
  r.dia_x = p->dia_x, r.dia_h = p->dia_h, r.u_x = p->u_x, r.v_x = p->v_x, r.b_x = p->b_x, r.b_h = p->b_h;
  r.u_h0 = p->u_h[0], r.u_h1 = p->u_h[1], r.v_h0 = p->v_h[0], r.v_h1 = p->v_h[1];
  for (int k = 0; k < 4; ++k) r.wg[k] = p->w_gate[k], r.ug[k] = p->u_gate[k], r.bg[k] = p->b_gate[k];
  return r;
}
inline RefG to_refg(const vmlmf_grads* gr) {
  RefG og;
  og.dia_x = gr->dia_x, og.dia_h = gr->dia_h, og.u_x = gr->u_x, og.v_x = gr->v_x, og.b_x = gr->b_x;
  og.b_h = gr->b_h, og.u_h0 = gr->u_h[0], og.u_h1 = gr->u_h[1], og.v_h0 = gr->v_h[0], og.v_h1 = gr->v_h[1];
  for (int k = 0; k < 4; ++k) og.wg[k] = gr->w_gate[k], og.ug[k] = gr->u_gate[k], og.bg[k] = gr->b_gate[k];
  return og;
}

// ---- argument checks (vmlmf_api.hip)
int check_params(const VGeo& g, const vmlmf_params* p);
int check_grads(const VGeo& g, const vmlmf_grads* gr);
int check_head(const VGeo& g, const vmlmf_head* hd, bool fwd);

// ---- dropout (vmlmf_dropout.h).  One builder of the kernel arguments of a site: yd is the dropped copy a forward writes (else NULL)
// B: the batch rows of an entry that knows them - a site with VMLMF_SITE_LOCKED then draws locked factors (period = B); 0: a flat
// entry, which refuses the flag (it would draw per-element factors under a site word that promises locked ones)
inline int drop_args(float p, const void* state, int site, float* yd, DropArgs* out, int B = 0) {
  memset(out, 0, sizeof(*out));
  if (!(p >= 0.f && p < 1.f)) return fail(VMLMF_E_BADARG, "dropout: p must be in [0, 1)");
  if ((site & VMLMF_SITE_LOCKED) != 0) {
    if (B < 1) return fail(VMLMF_E_BADARG, "dropout: VMLMF_SITE_LOCKED takes an entry that knows B (the _locked / _lk forms)");
    out->period = B;
  }
  out->state = reinterpret_cast<const unsigned long long*>(state), out->yd = yd;
  out->thresh = drop_thresh(p), out->scale = 1.f / (1.f - p), out->site = site;
  return 0;
}
// ... of a layer call's or a stack layer's vmlmf_dropout (NULL: none, all-zero arguments)
int site_drop(const vmlmf_dropout* dr, bool forward, int B, DropArgs* out);
// the layers whose own launches apply it (vmlmf_dropout_fused): row-block layers in the time-major layout
inline bool drop_fused(const VGeo& g) { return g.rb && g.syT == (long long)g.B * g.H; }

// ---- the kernels of one layer call (vmlmf_api.hip)
// The forward and the backward of a call build the same plan from the same inputs, so they agree by construction on the family, the
// x-projection wave and direct mode (the backward of a direct-mode forward reads images its forward never wrote otherwise).
enum Family { FAM_RB, FAM_STEP, FAM_VALU };   // row-block MFMA recurrence / step-wise path (wide layers included) / VALU kernels
enum RecKernel { K_REC, K_REC3, K_REC4 };     // rec_*_kernel / rec3_*_kernel / rec4_bwd_kernel (weight gradients in the rows' workgroups)
// PLAN_CHAINED: a layer of a stack's backward run by the per-layer kernels (its tape comes from a stack launch): no riding workers,
// no in-row weight gradients (never K_REC4), no direct mode
enum PlanCtx { PLAN_CALL, PLAN_CHAINED };
struct LayerPlan {
  Family family;
  bool xwave;          // the x projection inside the forward recurrence (else xproj_kernel / the wide GEMMs first)
  RecKernel fwd, bwd;  // the VALU family's recurrent kernels
  bool direct;         // the recurrent kernels build their images from the reference layouts (vmlmf_direct.inc)
  bool head_inside;    // the classifier rides inside the recurrent kernels (else the stand-alone head kernels)
  bool dqx;            // the VALU backward runs dqx_dx (with the x-fold dqx only feeds dx)
  bool finish2;        // the riding workers' gradients are finished by one launch (finish2_kernel)
  WRide ride;          // ride.K > 0: weight-gradient workers ride on the backward launch (buffers: ride_buffers)
};
// want_dx: the backward writes dx (the forward reads no field that depends on it)
LayerPlan plan_layer(const VGeo& g, const vmlmf_params* p, bool packed, bool head, bool want_dx, PlanCtx ctx = PLAN_CALL);

inline WghArgs wgrad_args(const Layout& L, const float* x, const float* y, const float* h0, const float* rs, float* ws) {
  WghArgs wh;
  wh.dpre = ws + L.b_dpre, wh.x = x, wh.y = y, wh.h0 = h0, wh.qx = rs + L.r_qx, wh.dqx = ws + L.b_dqx;
  wh.Qs = rs + L.r_Qs, wh.dQs = ws + L.b_dQs, wh.wpart = ws + L.b_wpart;
  return wh;
}
// the classifier's gradients riding on a backward launch: the layer's final hidden state is the last time slice of y (NULL head: none)
inline HeadBwd head_bwd_args(const vmlmf_head* head, const VGeo& g, const float* y) {
  HeadBwd hb;
  memset(&hb, 0, sizeof(hb));
  if (head == nullptr) return hb;
  hb.W = head->weight, hb.dl = head->dlogits, hb.hlast = y + (size_t)(g.T - 1) * g.syT, hb.ldh = g.syB, hb.dW = head->dweight, hb.db = head->dbias;
  hb.C = head->classes;
  return hb;
}
// the tensors of one layer's backward
struct LayerBwdIo {
  const float *x, *y, *h0, *c0, *dy, *dhT, *dcT;
  float *dx, *dh0, *dc0;
};
// the recurrent half of a VALU layer's backward (rec / rec3 / rec4 as planned, then dqx_dx); pack: the layer's parameter images.
// (pl is not const only because the buffers of its riding workers are filled in here; backward_tail reads them from it)
int valu_backward(const VGeo& g, LayerPlan* pl, const Layout& L, const VPack& P, const float* pack, const vmlmf_params* p, const LayerBwdIo& io,
                  const HeadBwd& hb, const float* rs, float* ws, hipStream_t s);
// the batched half of a layer's backward: every weight gradient (MFMA products over all rows), their fixed-order sum, and
// the reference-layout gradients
int backward_tail(const VGeo& g, const LayerPlan& pl, const Layout& L, const vmlmf_params* p, const vmlmf_grads* gr, const float* x,
                  const float* y, const float* h0, const float* rs, float* ws, const HeadBwd& hb, hipStream_t s);

}  // namespace vmlmf_host
#pragma GCC visibility pop
