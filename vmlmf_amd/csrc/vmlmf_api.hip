// Host side of the C ABI (include/vmlmf_hip.h): descriptor validation, launch geometry, buffer layout,
// and the kernel sequences of one layer's forward / backward.  No torch, no allocation, no sync.
#include "vmlmf_host.h"

using namespace vmlmf_host;

namespace vmlmf_host {

// ---- geometry ----
// force_W: at least this many waves of hidden units per group (a stack whose layers differ in hidden_size runs every layer on the
// widest one's thread-slot geometry: the surplus slots are padding, as the slots behind a hidden size that is no multiple of 64 are)
int make_geo(const vmlmf_desc* d, VGeo* out, RbGeo* rbout, int force_W) {
  if (d == nullptr) return fail(VMLMF_E_BADARG, "null descriptor");
  VGeo g;
  memset(&g, 0, sizeof(g));
  g.variant = d->variant;
  g.B = d->B;
  g.T = d->T;
  g.I = d->I;
  g.H = d->H;
  g.rw = d->w_rank;
  if (d->dtype != VMLMF_DT_F32 && d->dtype != VMLMF_DT_BF16) return fail(VMLMF_E_BADARG, "dtype must be VMLMF_DT_F32 or VMLMF_DT_BF16");
  g.bf = d->dtype == VMLMF_DT_BF16 ? 1 : 0;
  if (g.variant < 1 || g.variant > 6) return fail(VMLMF_E_BADARG, "variant must be 1..6");
  if (g.B < 1 || g.T < 1 || g.I < 1 || g.H < 1 || g.rw < 1)
    return fail(VMLMF_E_BADARG, "B, T, I, H, w_rank must be positive");
  const bool grouped = g.variant == VMLMF_V2_GROUP_CELL || g.variant == VMLMF_V4_LM_GROUP ||
                       g.variant == VMLMF_V6_GROUP_NOVM;
  const bool lm = g.variant == VMLMF_V3_LM || g.variant == VMLMF_V4_LM_GROUP;
  g.novm = (g.variant == VMLMF_V5_LMF_CELL || g.variant == VMLMF_V6_GROUP_NOVM) ? 1 : 0;
  g.pergate = g.variant == VMLMF_V5_LMF_CELL ? 1 : 0;
  g.xperm = g.variant == VMLMF_V6_GROUP_NOVM ? 1 : 0;
  g.G = grouped ? d->g : 1;
  if (grouped && g.G < 1) return fail(VMLMF_E_BADARG, "g must be positive");
  if (g.G > VMLMF_MAX_G)
    return fail(VMLMF_E_UNSUPPORTED, "g > 2 is not covered by the HIP kernels (the reference never builds it)");
  if (g.H % g.G != 0) return fail(VMLMF_E_SHAPE, "hidden_size must be divisible by g (vmlmf_group.py:73)");
  // the reference fails on these shapes too (vmlmf.py:94 / vmlmf_lm.py:243)
  if (!lm && !g.novm && g.I > g.H)
    return fail(VMLMF_E_SHAPE, "input_size > hidden_size: the reference cell raises (vmlmf.py:94,103)");

  if (lm && g.I != g.H) return fail(VMLMF_E_SHAPE, "LM layers need input_size == hidden_size (vmlmf_lm.py:243)");
  g.ru0 = d->u_ranks[0];
  g.ru1 = g.G == 2 ? d->u_ranks[1] : 0;
  if (g.ru0 < 1 || (g.G == 2 && g.ru1 < 1)) return fail(VMLMF_E_BADARG, "u_ranks must be positive");
  g.Hg = g.H / g.G;
  g.W = (g.Hg + 63) / 64;
  if (force_W > g.W) g.W = force_W;
  g.NW = g.G * g.W;
  g.NT = g.NW * 64;
  g.off1 = vg_pad8(g.ru0);
  g.KH = g.off1 + (g.G == 2 ? vg_pad8(g.ru1) : 0);
  g.KX = vg_pad8(g.rw);
  g.NP = (g.KH + 15) / 16;
  g.KQ = g.NP * 16;
  g.NPX = (g.KX + 15) / 16;
  g.KQX = g.NPX * 16;
  g.flat = g.variant == VMLMF_V4_LM_GROUP ? 1 : 0;
  g.hperm = (g.variant == VMLMF_V2_GROUP_CELL || g.variant == VMLMF_V6_GROUP_NOVM) ? 1 : 0;
  g.time_major = d->time_major ? 1 : 0;
  g.training = d->training ? 1 : 0;
  if (g.time_major) {
    g.sxT = (long long)g.B * g.I;
    g.sxB = g.I;
    g.syT = (long long)g.B * g.H;
    g.syB = g.H;
  } else {
    g.sxT = g.I;
    g.sxB = (long long)g.T * g.I;
    g.syT = g.H;
    g.syB = (long long)g.T * g.H;
  }
  // register-resident persistent kernels need <= 32 ranks per unit and <= 512 thread slots; larger layers
  // (e.g. H = 650, ranks [32,32]) run the step-wise path of vmlmf_generic.hip
  // (the cells without vm accept input_size > hidden_size; the persistent kernels keep x-side quantities in the slots of the
  // first I units, so such a layer takes the step-wise path, whose x side is indexed by input)
  g.generic = (g.KH > 32 || g.NT > 512 || g.I > g.H) ? 1 : 0;
  // Wide layers (padded w_rank > 32, or padded hidden rank summed over groups > 128, e.g. the reference LM's default ranks 300 / 300):
  // the step-wise family only, with the x side and the weight gradients as rank-agnostic GEMMs.  The register-resident kernels keep
  // x-side factor images in registers; a wide x side there stays refused (the message keeps its historical start).
  g.wide = (g.KX > 32 || g.G * g.KH > 128) ? 1 : 0;
  if (g.wide) {
    if (!g.generic) {
      if (g.KX > 32)
        return fail(VMLMF_E_UNSUPPORTED, "padded w_rank > 32 is not covered by the HIP kernels on a register-resident layer "
                                         "(wide ranks need the step-wise path: padded u_rank > 32, more than 512 thread slots or I > H)");
      return fail(VMLMF_E_UNSUPPORTED, "padded hidden rank (summed over groups) > 128 is not covered on a register-resident layer");
    }
    if (g.rw > g.I) return fail(VMLMF_E_UNSUPPORTED, "wide ranks: w_rank larger than input_size (an over-complete factorisation) is not covered");
    if (g.ru0 > g.Hg || (g.G == 2 && g.ru1 > g.Hg))
      return fail(VMLMF_E_UNSUPPORTED, "wide ranks: a u_rank larger than the units it factors (hidden_size / g) is not covered");
    if (g.bf) return fail(VMLMF_E_UNSUPPORTED, "wide ranks: dtype bf16 is not covered (fp32 only)");
    if (g.KX > 1024 || g.KH > 1024)
      return fail(VMLMF_E_UNSUPPORTED, "wide ranks: padded w_rank and padded hidden rank (summed over shifts) are capped at 1024, the "
                                       "bound of the step-wise workspace");
  }
  // One batch row per workgroup, whatever the batch: with more rows than CUs the workgroups queue up, which
  // measured at least as fast as two rows per workgroup at every size (H = 180, T = 128: B = 512 0.49 vs 0.55 ms,
  // 768 0.71 vs 0.78, 1024 0.98 vs 0.96, 2048 1.84 vs 2.00); the kernels keep their R template parameter.
  g.R = 1;
  g.nwg = (g.B + g.R - 1) / g.R;
  g.Bp = g.nwg * g.R;
  if ((long long)g.T * g.Bp * g.NT * 4 >= (1LL << 31) || (long long)g.T * g.B * g.H >= (1LL << 31))
    return fail(VMLMF_E_UNSUPPORTED, "T*B*H too large for the 32-bit element offsets of the kernels");
  // backward, parallel part: dqx_dx works on RC rows per workgroup (groups of 8 per barrier); wgrad keeps
  // register accumulators over RC2 rows per chunk, 5 parts per chunk
  const int TB = g.T * g.B;
  // (measured at the headline shape: ~1024 dqx_dx workgroups 12.9 us, 512 14.0, 256 16.7; 64 wgrad chunks:
  // 128 chunks gain 2 us there and lose them again in reduce_cg_kernel, 32 chunks cost 10 us)
  int rc = ((TB + 1023) / 1024 + 7) / 8 * 8;
  if (rc < 8) rc = 8;
  if (g_rc > 0) rc = g_rc;
  g.RC = rc;
  g.nblk = (TB + rc - 1) / rc;
  int rc2 = (TB + g_wchunks - 1) / g_wchunks;
  if (rc2 < g_wmin) rc2 = g_wmin;
  g.RC2 = rc2;
  g.nchunk = (TB + rc2 - 1) / rc2;
  g.foldx = (!g.generic && g.I <= g.KX) ? 1 : 0;
  g.NA = 5 * g.KX + 5 * g.KH + 12;
  // row-block MFMA recurrence?
  {
    RbGeo q;
    memset(&q, 0, sizeof(q));
    g.rb = 0;
    if (g.bf) {   // the bf16 variant IS the row-block family
      if (!g.generic && g.I <= g.H && rb_geometry(g, 1, &q, g_rb_rows)) g.rb = 1;
      else return fail(VMLMF_E_UNSUPPORTED, "dtype bf16: implemented by the row-block MFMA kernels for one-group layers (V1, V3, V5) "
                                            "with padded rank <= 32 and <= 512 thread slots");
    } else if (g_rb_mode != 0 && g.I <= g.H && !g.wide) {   // (wide layers: the step-wise recurrence only)
      if (g.generic) {          // factors beyond one CU's registers: a cluster of S workgroups per 16-row block
        // measured at H = 650, B = 256 (members of a cluster on one XCD): group layer (ranks 32+32) 2.98 / 2.21 / 2.09 ms with
        // clusters of 4 / 8 / 16, plain layer (rank 32) 1.84 / 1.64 / 1.60 ms: the largest cluster first
        const int cand[] = {g_rb_S, 16, 8, 4, 2};
        for (int i = (g_rb_S > 0 ? 0 : 1); i < 5 && g.rb == 0; ++i)
          if (cand[i] > 1 && rb_geometry(g, cand[i], &q, g_rb_rows)) g.rb = cand[i];
      } else if ((g_rb_mode == 1 || (g_rb_minB > 0 && g.B >= g_rb_minB)) && rb_geometry(g, 1, &q, g_rb_rows)) {
        g.rb = 1;
      }
    }
    if (g.rb != 0) g.foldx = 0;   // the x-fold belongs to the x-projection wave's layers; here qx always exists
    if (rbout != nullptr) *rbout = q;
  }
  {
    const long long GK = (long long)g.G * g.KH;
    const long long nb1 = (vg_nb1(g) + 31) / 32 * 32, nb2 = (GK + 31) / 32 * 32, nb3 = (g.KX + 31) / 32 * 32;
    g.PCH = (long long)g.NT * 4 * nb1 + (long long)((g.H + 31) / 32) * 32 * nb2 +
            (long long)((g.I + 31) / 32) * 32 * nb3 + 3LL * g.NT * 4;
  }
  *out = g;
  return 0;
}

// ---- buffer layouts (float offsets) ----
// split-K scratch of a step-wise layer's GEMMs (GenericBuf::part): VG_GEMM_SPLIT partial copies of the largest skinny product (B x G*KH)
static long long gemm_part_floats(const VGeo& g) { return (long long)VG_GEMM_SPLIT * ((g.B + 63) / 64 * 64) * ((g.G * g.KH + 63) / 64 * 64); }
Layout make_layout(const VGeo& g, const VPack& P, const RbGeo& q) {
  Layout L;
  const long long TB = (long long)g.T * g.B;
  const long long TS = (long long)g.T * g.Bp * g.NT;   // (t, padded row, thread slot)
  long long o = 0;
  L.r_pack = o, o += align64(P.total);
  // (16 spare rows behind qx, Q, dQ, dqx of the layers wgrad_ring_kernel may take: its last stage fetches whole 16-row pieces)
  const long long TBp = TB + (g.NT >= 256 ? 16 : 0);
  L.r_qx = o, o += align64(TBp * g.KX);
  L.r_gates = o, o += align64(TS * 4);
  L.r_cs = o, o += align64(TS + (long long)g.Bp * g.NT);   // slice 0 = c0, slice t+1 = c_t
  L.r_Qs = o, o += align64(TBp * g.G * g.KH);
  L.r_prog = o, o += align64((long long)g.B * WR_PROG_STRIDE);   // progress words of the backward rows (zero between launches: cleared by the forward kernel)
  L.r_total = o;
  o = 0;
  L.f_pack = o, o += align64(P.total);
  L.f_gx = o, o += align64(TS * 4);
  L.f_qx = o, o += align64(g.generic ? TB * g.KX : 0);   // qx of an inference call on a large layer (the MFMA x-side expansion reads it)
  L.f_trash = o, o += 64;
  {
    const long long gen = (g.generic && !g.rb) ? 1 : 0, BN = (long long)g.B * g.NT;
    L.f_Qtmp = o, o += align64(gen * g.B * g.G * g.KH);
    L.f_P = o, o += align64(gen * BN * 4);
    L.f_ccar = o, o += align64(gen * BN);
    L.f_zeros = o, o += align64(gen * (long long)g.B * g.H);
    L.f_part = o, o += align64(gen * gemm_part_floats(g));
  }
  L.f_xq = o, o += align64(g.rb ? q.xq_floats : 0);
  L.f_flag = o, o += align64(g.rb ? q.flag_words : 0);
  L.f_xrows = o, o += align64((g.wide && !g.time_major) ? TB * g.I : 0);   // x in (t, b) row order for a wide layer's x-side GEMM
  L.f_total = o;
  o = 0;
  L.b_dpre = o, o += align64(TS * 4);
  L.b_dQs = o, o += align64(TBp * g.G * g.KH);
  L.b_dqx = o, o += align64(TBp * g.KX);
  // (one partial block per chunk of rows, or - backward with the weight gradients formed in the rows' workgroups - per workgroup)
  {
    long long blocks = g.nchunk;
    if (!g.generic && !g.rb && rec4_bwd_supported(g) && g.nwg > blocks) blocks = g.nwg;
    L.b_wpart = o, o += align64(g.wide ? 0 : blocks * g.PCH);   // (wide layers: dense products in b_wide instead)
  }
  L.b_cgrad = o, o += align64((long long)g.NA * g.NT + (g.I > g.H ? (long long)g.I * g.KX : 0));   // + dU_x by input when I > H
  L.b_trash = o, o += 64;
  {
    const long long gen = (g.generic && !g.rb) ? 1 : 0, BN = (long long)g.B * g.NT;
    L.b_dHrec = o, o += align64(gen * (long long)g.B * g.H);
    L.b_ehterm = o, o += align64(gen * BN);
    L.b_dcar = o, o += align64(gen * BN);
    // (the dqx product of large layers keeps its split-K scratch under the row-block kernels too)
    L.b_part = o, o += align64((g.generic ? 1 : 0) * gemm_part_floats(g));
  }
  L.b_xq = o, o += align64(g.rb ? q.xq_floats : 0);
  L.b_flag = o, o += align64(g.rb ? q.flag_words : 0);
  L.b_headdh = o, o += align64((g.rb || g.generic) ? (long long)g.B * g.H : 0);   // d(hT) of a classifier on the row-block / step-wise families
  // the riding workers' shares of d(u_x) (finish2_kernel): [worker index][task][16 x 16]
  L.b_dux = o, o += align64((!g.generic && !g.rb && finish2_ok(g)) ? (long long)g.nchunk * (g.NT / 8) * 256 : 0);
  L.b_wide = o, o += wide_scratch_floats(g);
  L.b_total = o;
  return L;
}

// vmlmf_params and vmlmf_grads have the same members; one check serves both
template <class P>
static int check_pointers(const VGeo& g, const P* p, const char* what) {
  if (p == nullptr) return fail(VMLMF_E_BADARG, std::string("null ") + what);
  bool ok = p->u_x && p->u_h[0];
  if (g.pergate) {
    for (int k = 0; k < 4; ++k) ok = ok && p->w_gate[k] && p->u_gate[k] && p->b_gate[k];
  } else {
    ok = ok && p->v_x && p->b_x && p->b_h && p->v_h[0];
    if (!g.novm) ok = ok && p->dia_x && p->dia_h;
  }
  if (!ok) return fail(VMLMF_E_BADARG, std::string("null pointer in ") + what);
  if (g.G == 2 && (!p->u_h[1] || !p->v_h[1]))
    return fail(VMLMF_E_BADARG, std::string(what) + ": group variant needs u_h[1], v_h[1]");
  return 0;
}

int check_params(const VGeo& g, const vmlmf_params* p) { return check_pointers(g, p, "params"); }
int check_grads(const VGeo& g, const vmlmf_grads* gr) { return check_pointers(g, gr, "grads"); }
int check_head(const VGeo& g, const vmlmf_head* hd, bool fwd) {
  if (hd == nullptr || hd->classes == 0) return 0;
  if (hd->classes < 0 || hd->classes > head_max_classes()) return fail(VMLMF_E_UNSUPPORTED, "head: 1..32 classes");
  if (hd->weight == nullptr || (fwd ? hd->logits == nullptr : hd->dlogits == nullptr)) return fail(VMLMF_E_BADARG, "head: null pointer");
  return 0;
}

// ---- the kernels of one layer call (LayerPlan: vmlmf_host.h) ----
// Do the weight-gradient products ride on the recurrent backward launch?  Layers of the persistent VALU kernels whose x-side
// gradient folds into the dpre product (no dqx operand, which only exists after that launch), with few enough batch rows that
// most of the chip is idle during the recurrence.  Fills the worker counts of w (K = 0: no).
// (g.flat: a V4 layer small enough for the x-fold - hidden_size <= 16 - takes the stand-alone weight-gradient kernel: the riding
//  instantiations of the flat layout left the library in round 5 as unreachable, and such a layer's backward was refused since -
//  found by tools/fuzz_parity.py in round 6)
static void plan_wride(const VGeo& g, WRide* w) {
  const int n1 = (vg_nb1(g) + 31) / 32, n2 = (g.G * g.KH + 31) / 32;
  if (!g_wride || g_wride_tripped.load() != 0 || !g.foldx || g.flat || g.R != 1 || g.NT > 256 || g.B > g_wride_maxb || n1 > 2 || n2 > 2) return;
  // rows per chunk: a part of a step's batch rows when they divide evenly (one batch of loads per chunk: the last chunk's
  // latency is the tail of the launch), else whole steps of at least 64 rows
  const int S = (g.B % g_wride_rc == 0 && g_wride_rc % 2 == 0) ? g_wride_rc : g.B * (g.B >= 64 ? 1 : (64 + g.B - 1) / g.B);
  const int nck = (g.T * g.B + S - 1) / S;
  int K = g_wride_k < g.nchunk ? g_wride_k : g.nchunk;         // partial blocks: the workspace holds nchunk of them
  K = K < nck ? K : nck;
  const int tasks = g.NT / 8 + (g.H + 31) / 32;
  const int wpw = (g.NT + 128) / 64;
  const int ntg = (tasks + wpw - 1) / wpw;
  // every workgroup of the launch has a CU of its own (the launch asks for more than half a CU's LDS): rows + workers must
  // fit the chip at once, or the workers behind the last CU would only start when the others have finished
  // (the CU count of THIS device, less a margin of eight for whatever else is resident: on a partitioned or masked device a
  // fixed 248 would queue workers behind the rows, and a queued worker can only give up)
  const int room = (device_cus() - 8 - g.nwg) / ntg;
  K = K < room ? K : room;
  if (K < 4) return;
  w->K = K, w->S = S, w->tasks = tasks, w->ntg = ntg;
  w->lag = g_wride_lag < 8 ? g_wride_lag : 8;
  w->spin = (unsigned)g_wride_spin;
}

LayerPlan plan_layer(const VGeo& g, const vmlmf_params* p, bool packed, bool head, bool want_dx, PlanCtx ctx) {
  LayerPlan pl;
  memset(&pl, 0, sizeof(pl));
  pl.family = g.rb ? FAM_RB : (g.generic ? FAM_STEP : FAM_VALU);
  // narrow-input layers compute the x-projection inside rec_fwd_kernel (VMLMF_XWAVE=0: always the separate launch)
  pl.xwave = g_xwave && vg_xwave_ok(g);
  pl.head_inside = head && pl.family == FAM_VALU;
  pl.dqx = !(g.foldx && !want_dx);
  if (pl.family != FAM_VALU) return pl;
  const bool call = ctx == PLAN_CALL;
  if (pl.xwave && ((g_rec3 & 1) || ((g_rec3 & 4) && g.nwg > device_cus())) && rec3_fwd_supported(g)) pl.fwd = K_REC3;
  const bool rec3_bwd = (g_rec3 & 2) && rec3_bwd_supported(g);
  // weight gradients inside the rows' workgroups: layers it covers whose input needs no gradient; automatic: batches beyond the
  // riding workers' range (up to there the idle CUs form the products for free)
  if (call && g_inrow != 0 && !want_dx && rec4_bwd_supported(g) && (g_inrow > 0 || g.B > g_wride_maxb)) pl.bwd = K_REC4;
  else pl.bwd = rec3_bwd ? K_REC3 : K_REC;
  if (call && pl.bwd != K_REC4) plan_wride(g, &pl.ride);
  if (pl.ride.K > 0 && pl.bwd != K_REC3 && !rec_bwd_rides(g)) memset(&pl.ride, 0, sizeof(pl.ride));
  // one launch behind the riding workers finishes every gradient where it covers the layer: the workers then contract their
  // x-fold tiles with v_x themselves
  pl.finish2 = pl.ride.K > 0 && g_finish2 != 0 && finish2_ok(g) && p->v_x != nullptr;
  // direct mode: V1 / V3 layers of ranks 8 / 16 on rec_fwd_kernel's x-projection wave; a training call's backward must be one of the
  // kernels that can do the same (rec3_bwd_kernel / rec4_bwd_kernel); the reference's rows are read as 16-byte loads
  const uintptr_t al = (uintptr_t)p->v_h[0] | (uintptr_t)p->u_h[0] | (uintptr_t)p->v_x | (uintptr_t)p->u_x;
  pl.direct = call && !packed && g_direct != 0 && (g.variant == VMLMF_V1_CELL || g.variant == VMLMF_V3_LM) && g.G == 1 && g.R == 1 &&
              g.foldx && pl.xwave && pl.fwd == K_REC && (g.KH == 8 || g.KH == 16) && g.ru0 == g.KH && (g.KX == 8 || g.KX == 16) &&
              g.rw == g.KX && (!g.training || rec3_bwd) && (al & 15u) == 0;
  return pl;
}

static WgxArgs wgx_args(const Layout& L, const VPack& P, const float* pack, float* ws, float* dx) {
  WgxArgs wx;
  wx.dpre = ws + L.b_dpre, wx.VRX = pack + P.VRX, wx.UXO = pack + P.UXO, wx.EXI = pack + P.EXI;
  wx.dx = dx, wx.dqx = ws + L.b_dqx;
  return wx;
}
// split-K scratch and tickets of a step-wise call's GEMMs
static void split_k(GenericBuf* w, const VGeo& g, float* part, const float* pack, const VPack& P) {
  w->part = part, w->part_cap = gemm_part_floats(g);
  w->ticket = reinterpret_cast<int*>(const_cast<float*>(pack + P.TKT)), w->ticket_cap = VG_GEMM_TICKETS;
}
// the buffers of the plan's riding workers, or of the in-row weight gradients
static void ride_buffers(LayerPlan* pl, const Layout& L, const WghArgs& wh, const vmlmf_params* p, const float* rs, float* ws, hipStream_t s) {
  WRide* w = &pl->ride;
  if (pl->bwd == K_REC4) {
    w->a.x = wh.x, w->a.y = wh.y, w->a.h0 = wh.h0, w->a.Qs = wh.Qs, w->a.P = wh.wpart;
    return;
  }
  if (w->K == 0) return;
  w->a.dpre = wh.dpre, w->a.x = wh.x, w->a.y = wh.y, w->a.h0 = wh.h0, w->a.qx = wh.qx, w->a.dqx = wh.dqx, w->a.Qs = wh.Qs;
  w->a.dQs = wh.dQs, w->a.P = wh.wpart;
  w->prog = reinterpret_cast<unsigned*>(const_cast<float*>(rs + L.r_prog));
  w->status = status_word(s);
  if (pl->finish2) w->dux = ws + L.b_dux, w->vx = p->v_x;
}

int backward_tail(const VGeo& g, const LayerPlan& pl, const Layout& L, const vmlmf_params* p, const vmlmf_grads* gr, const float* x,
                  const float* y, const float* h0, const float* rs, float* ws, const HeadBwd& hb, hipStream_t s) {
  int rc;
  const WghArgs wh = wgrad_args(L, x, y, h0, rs, ws);
  const bool rode = pl.ride.K > 0, inrow = pl.bwd == K_REC4;
  int ring_nc[3] = {0, 0, 0};
  if (g.wide) {   // dense GEMMs straight into the canonical gradients (cgrad): no partial blocks, no reduce launch
    const long long TB = (long long)g.T * g.B, N4 = 4LL * g.NT, GK = (long long)g.G * g.KH;
    auto al = [](long long n) { return (n + 63) / 64 * 64; };
    WideBuf wb;
    wb.x = x, wb.y = y, wb.h0 = h0, wb.dpre = wh.dpre, wb.qx = wh.qx, wb.dqx = wh.dqx, wb.Qs = wh.Qs, wb.dQs = wh.dQs;
    float* o = ws + L.b_wide;   // (the order of wide_scratch_floats)
    wb.X = o, o += al(g.time_major ? 0 : TB * g.I);
    wb.Hp = o, o += al(TB * g.H);
    wb.dVd = o, o += al(N4 * GK);
    wb.dUd = o, o += al((long long)g.H * GK);
    wb.dVx = o, o += al(N4 * g.KX);
    wb.dUx = o, o += al((long long)g.I * g.KX);
    wb.csum = o;
    wb.cgrad = ws + L.b_cgrad;
    if ((rc = run(SL_WGRAD, s, "wgrad", [&] { return wide_wgrad(g, wb, s); })) != 0) return rc;
  } else if (!rode && !inrow) {
    Scope sc(SL_WGRAD, s);   // (covers both launches of the fallback)
    // large layers: operands through an LDS ring, long chunks (vmlmf_wgrad_ring.hip); -1: where it was measured faster
    const bool ring = g_wring != 0 && wgrad_ring_ok(g) && (g_wring > 0 || (g.generic && (long long)g.T * g.B >= 1024));
    int rr = ring ? launch_wgrad_ring(g, wh, device_cus(), ring_nc, s) : -3;
    if (rr == 0) ++g_ring_launches;
    if (rr == -3) {   // not taken, or no instantiation / no LDS for it on this device: the stand-alone products, one chunking for all
      ring_nc[0] = ring_nc[1] = ring_nc[2] = 0;
      rr = launch_wgrad_h(g, wh, s);
    }
    if ((rc = hip_fail(rr, "wgrad")) != 0) return rc;
  }
  const RefG og = to_refg(gr);
  if (rode && pl.finish2)   // the riding workers left their d(u_x) shares: ONE launch sums the K blocks and finishes
    return run(SL_FINISH2, s, "finish2", [&] {
      return launch_finish2(g, to_refp(p), ws + L.b_wpart, pl.ride.dux, pl.ride.K, og, hb, pl.ride.prog, s, health_word(s));
    });
  if (!g.wide) {
    VGeo gr_ = g;
    if (rode) gr_.nchunk = pl.ride.K;   // one partial block per worker index; the progress words go back to zero here
    if (inrow) gr_.nchunk = g.B;        // one partial block per workgroup of rec4_bwd_kernel
    if ((rc = run(SL_REDUCE, s, "reduce", [&] {
           return launch_reduce(gr_, ws + L.b_wpart, ws + L.b_cgrad, rode ? pl.ride.prog : nullptr, s, ReduceCounts{{ring_nc[0], ring_nc[1], ring_nc[2]}});
         })) != 0) return rc;
  }
  return run(SL_FINISH, s, "finish", [&] { return launch_finish(g, to_refp(p), ws + L.b_cgrad, og, hb, s, health_word(s)); });
}

int site_drop(const vmlmf_dropout* dr, bool forward, int B, DropArgs* out) {
  memset(out, 0, sizeof(*out));
  if (dr == nullptr) return 0;
  const int rc = drop_args(dr->p, dr->state, dr->site, forward ? dr->y_dropped : nullptr, out, B);
  if (rc != 0) return rc;
  if (dr->state == nullptr || (forward && dr->y_dropped == nullptr)) return fail(VMLMF_E_BADARG, "dropout: null state / y_dropped");
  return 0;
}

int valu_backward(const VGeo& g, LayerPlan* pl, const Layout& L, const VPack& P, const float* pack, const vmlmf_params* p, const LayerBwdIo& io,
                  const HeadBwd& hb, const float* rs, float* ws, hipStream_t s) {
  int rc;
  BwdArgs a;
  a.gates = rs + L.r_gates, a.cs = rs + L.r_cs, a.c0 = io.c0, a.dy = io.dy, a.dhT = io.dhT, a.dcT = io.dcT;
  a.VR = pack + P.VR, a.UE = pack + P.UE, a.EH = pack + P.EH, a.VE = pack + P.VE;
  a.dpre = ws + L.b_dpre, a.dQs = ws + L.b_dQs, a.dh0 = io.dh0, a.dc0 = io.dc0, a.trash = ws + L.b_trash;
  a.hd = hb;
  // (a PLAN_CHAINED plan rides nothing: the tape is a stack launch's, its progress words are not this path's)
  ride_buffers(pl, L, wgrad_args(L, io.x, io.y, io.h0, rs, ws), p, rs, ws, s);
  a.wr = pl->ride;
  if (pl->direct) {   // the forward of this call packed nothing
    // the backward builds its own images where its workgroups have a CU each (riding workers, weight gradients in the rows'
    // workgroups); elsewhere, and for the input's gradient (x-side images), this call packs after all
    const bool own = pl->bwd == K_REC4 || pl->ride.K > 0;
    if (own) a.VE = p->v_h[0], a.UE = p->u_h[0], a.EH = p->dia_h, a.wr.direct = 1;
    if ((!own || pl->dqx) &&
        (rc = run(SL_PACK, s, "pack", [&] { return launch_pack(g, to_refp(p), P, const_cast<float*>(pack), s); })) != 0) return rc;
  }
  {
    Scope sc(SL_REC_BWD, s);
    if (pl->bwd == K_REC4) {
      if ((rc = hip_fail(launch_rec4_bwd(g, a, s), "rec4_bwd")) != 0) return rc;
    } else if (pl->bwd == K_REC3) {
      if ((rc = hip_fail(launch_rec3_bwd(g, a, s), "rec3_bwd")) != 0) return rc;
    } else if ((rc = hip_fail(launch_rec_bwd(g, a, s), "rec_bwd")) != 0) return rc;
  }
  if (!pl->dqx) return 0;
  return run(SL_DQX_DX, s, "dqx_dx", [&] { return launch_wgrad_x(g, wgx_args(L, P, pack, ws, io.dx), s); });
}

}  // namespace vmlmf_host

extern "C" {

int vmlmf_query(const vmlmf_desc* d, vmlmf_sizes* out) {
  if (out == nullptr) return fail(VMLMF_E_BADARG, "null sizes");
  VGeo g;
  RbGeo q;
  const int rc = make_geo(d, &g, &q);
  if (rc != 0) return rc;
  const VPack P = vg_pack_layout(g, q.total);
  const Layout L = make_layout(g, P, q);
  out->workspace_bytes = (size_t)L.ws_total() * sizeof(float);
  out->reserve_bytes = (size_t)L.r_total * sizeof(float);
  out->rows_per_wg = g.rb ? q.rbl : g.R;
  out->threads_per_wg = g.rb ? 256 : g.NT;
  out->workgroups = g.rb ? q.nrb * q.S : g.nwg;
  out->kx = g.KX;
  out->kh = g.KH;
  return 0;
}

// ---- parameter images kept by the caller (vmlmf_pack_params / *_packed) ----
// An image is only valid for the geometry and the kernel selection (vmlmf_tune generation) it was packed for, and it lives in
// device memory, which the forward / backward calls never read back.  So the signature is kept ON THE HOST: vmlmf_pack_params
// records (device address -> signature) in a small registry, and a *_packed call whose image is unknown, or was packed for
// another geometry or under another kernel selection, returns VMLMF_E_BADARG instead of running kernels on a foreign layout
// (verdict r3: the header that used to sit in front of the image was written and never checked).  The registry holds the last
// PK_REG images per process; an image that fell out has to be packed again.  The 256 bytes in front of the image stay
// reserved (alignment of the images behind them).
constexpr int PK_HDR = 64;   // floats
struct PackSig {
  long long v[10];
  bool operator==(const PackSig& o) const { return memcmp(v, o.v, sizeof(v)) == 0; }
};
static PackSig pack_signature(const VGeo& g, const VPack& P, const RbGeo& q) {
  PackSig s;
  const long long v[10] = {g.variant, P.total, g.rb, g.generic * 2 + g.bf, g.NT, (long long)g.KH * 1000 + g.KX, q.total,
                           (long long)g.I * 100000 + g.H, (long long)g.G * 100000 + g.ru0 * 100 + g.ru1, g_tune_generation};
  memcpy(s.v, v, sizeof(v));
  return s;
}
constexpr int PK_REG = 256;
struct PackReg {
  std::mutex mu;
  const void* ptr[PK_REG] = {nullptr};
  PackSig sig[PK_REG];
  int next = 0;
  void put(const void* p, const PackSig& s) {
    std::lock_guard<std::mutex> lk(mu);
    for (int i = 0; i < PK_REG; ++i)
      if (ptr[i] == p) { sig[i] = s; return; }
    ptr[next] = p, sig[next] = s;
    next = (next + 1) % PK_REG;
  }
  // 0 = matches, 1 = unknown image, 2 = packed for something else
  int check(const void* p, const PackSig& s) {
    std::lock_guard<std::mutex> lk(mu);
    for (int i = 0; i < PK_REG; ++i)
      if (ptr[i] == p) return sig[i] == s ? 0 : 2;
    return 1;
  }
} g_packreg;
// (kept images are for the register-resident and row-block layers: the others' image carries per-call state)
static int refuse_kept(const char* why = "") {
  return fail(VMLMF_E_UNSUPPORTED, std::string("kept parameter images: not for the step-wise / clustered layers") + why);
}
static int check_packed(const void* packed, const VGeo& g, const VPack& P, const RbGeo& q) {
  if (g.generic) return refuse_kept();
  switch (g_packreg.check(packed, pack_signature(g, P, q))) {
    case 0: return 0;
    case 1: return fail(VMLMF_E_BADARG, "packed: not an image vmlmf_pack_params made at this address (or it left the registry of the last 256 images: pack it again)");
  }
  return fail(VMLMF_E_BADARG, "packed: the image was packed for another descriptor or under another kernel selection (vmlmf_tune): pack it again");
}

int vmlmf_pack_bytes(const vmlmf_desc* d, size_t* bytes) {
  if (bytes == nullptr) return fail(VMLMF_E_BADARG, "null size");
  VGeo g;
  RbGeo q;
  const int rc = make_geo(d, &g, &q);
  if (rc != 0) return rc;
  if (g.generic) return refuse_kept(" (their image carries per-call state)");
  const VPack P = vg_pack_layout(g, q.total);
  *bytes = sizeof(float) * (size_t)(PK_HDR + P.total);
  return 0;
}

int vmlmf_pack_params(const vmlmf_desc* d, const vmlmf_params* p, void* packed, void* stream) {
  VGeo g;
  RbGeo q;
  int rc = make_geo(d, &g, &q);
  if (rc != 0) return rc;
  if ((rc = check_params(g, p)) != 0) return rc;
  if (packed == nullptr) return fail(VMLMF_E_BADARG, "null packed buffer");
  if (g.generic) return refuse_kept();
  const VPack P = vg_pack_layout(g, q.total);
  hipStream_t s = (hipStream_t)stream;
  float* img = (float*)packed + PK_HDR;
  g_packreg.put(packed, pack_signature(g, P, q));
  const RefP rp = to_refp(p);
  Scope sc(SL_PACK, s);   // (both launches)
  if ((rc = hip_fail(launch_pack(g, rp, P, img, s), "pack")) != 0) return rc;
  if (g.rb && (rc = hip_fail(launch_rb_pack(g, q, rp, img + P.RB, s), "rb_pack")) != 0) return rc;
  return 0;
}

int vmlmf_seq_forward(const vmlmf_desc* d, const vmlmf_params* p, const float* x, const float* h0,
                      const float* c0, float* y, float* hT, float* cT, void* reserve, void* workspace,
                      size_t workspace_bytes, void* stream) {
  return vmlmf_seq_forward_packed(d, p, x, h0, c0, y, hT, cT, reserve, workspace, workspace_bytes, stream, nullptr);
}

int vmlmf_seq_forward_packed(const vmlmf_desc* d, const vmlmf_params* p, const float* x, const float* h0,
                             const float* c0, float* y, float* hT, float* cT, void* reserve, void* workspace,
                             size_t workspace_bytes, void* stream, const void* packed) {
  vmlmf_extra ex = {};   // every field the caller does not set is a null pointer (drop, ce, ...)
  ex.packed = packed, ex.head = nullptr, ex.ce = nullptr;
  return vmlmf_seq_forward_ex(d, p, x, h0, c0, y, hT, cT, reserve, workspace, workspace_bytes, stream, &ex);
}

// the criterion behind a classifier that is a launch of its own: a launch too (same values up to the mean's summation order)
static int ce_after(int B, const vmlmf_head* head, const vmlmf_ce* ce, hipStream_t s) {
  if (ce == nullptr) return 0;
  return run(SL_CE_FWD, s, "ce_fwd", [&] {
    return launch_ce_fwd(B, head->classes, head->logits, (const long long*)ce->target, (long long)ce->ignore_index, ce->loss, ce->lse,
                         ce->nvalid, ce->dlogits_unit, s);
  });
}
// behind the recurrence of the families that do not carry the classifier: the stand-alone head launch, then the criterion
static int head_and_ce_after(const VGeo& g, const vmlmf_head* head, const vmlmf_ce* ce, const float* hT, hipStream_t s) {
  int rc;
  if (head != nullptr && (rc = run(SL_HEAD_FWD, s, "head_fwd", [&] {
        return launch_head_fwd(g.B, g.H, head->classes, hT, g.H, head->weight, head->bias, head->logits, s);
      })) != 0) return rc;
  return ce_after(g.B, head, ce, s);
}

// vmlmf_dropout of a call -> kernel arguments (vmlmf_dropout.h); rc != 0: bad arguments / a layer whose kernels do not take it
static int make_drop(const vmlmf_dropout* dr, const VGeo& g, bool forward, DropArgs* out) {
  const int rc = site_drop(dr, forward, g.B, out);
  if (rc != 0 || dr == nullptr || drop_fused(g)) return rc;
  return fail(VMLMF_E_UNSUPPORTED, "dropout inside the layer's launches: row-block layers in the time-major layout (vmlmf_dropout_fused)");
}

int vmlmf_seq_forward_ex(const vmlmf_desc* d, const vmlmf_params* p, const float* x, const float* h0,
                         const float* c0, float* y, float* hT, float* cT, void* reserve, void* workspace,
                         size_t workspace_bytes, void* stream, const vmlmf_extra* ex) {
  const void* packed = ex != nullptr ? ex->packed : nullptr;
  const vmlmf_head* head = (ex != nullptr && ex->head != nullptr && ex->head->classes != 0) ? ex->head : nullptr;
  VGeo g;
  RbGeo q;
  int rc = take_status();
  if (rc != 0) return rc;
  if ((rc = make_geo(d, &g, &q)) != 0) return rc;
  if ((rc = check_params(g, p)) != 0) return rc;
  if (x == nullptr || y == nullptr || workspace == nullptr) return fail(VMLMF_E_BADARG, "null x / y / workspace");
  if (g.training && reserve == nullptr) return fail(VMLMF_E_BADARG, "training forward needs a reserve buffer");
  if ((rc = check_head(g, head, true)) != 0) return rc;
  // the classifier rides inside the VALU recurrent kernels; the other families run the stand-alone head kernel after
  // their recurrence (same values up to summation order)
  const LayerPlan pl = plan_layer(g, p, packed != nullptr, head != nullptr, true);
  if (head != nullptr && !pl.head_inside && hT == nullptr) return fail(VMLMF_E_BADARG, "head on this layer needs the hT output");
  DropArgs drop;
  if ((rc = make_drop(ex != nullptr ? ex->drop : nullptr, g, true, &drop)) != 0) return rc;
  const vmlmf_ce* ce = ex != nullptr ? ex->ce : nullptr;
  if (ce != nullptr) {
    if (head == nullptr) return fail(VMLMF_E_BADARG, "ce: the criterion rides on the classifier's logits (extra.head)");
    if (!ce->target || !ce->loss || !ce->nvalid || !ce->lse || !ce->ticket) return fail(VMLMF_E_BADARG, "ce: null pointer");
  }
  const VPack P = vg_pack_layout(g, q.total);
  const Layout L = make_layout(g, P, q);
  // (the size vmlmf_query reports serves either direction: a buffer short of it is refused by both, whichever needs less)
  if (workspace_bytes < (size_t)L.ws_total() * sizeof(float))
    return fail(VMLMF_E_WORKSPACE, "workspace smaller than vmlmf_query() reported");
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  float* rs = (float*)reserve;
  float* pack = g.training ? rs + L.r_pack : ws + L.f_pack;
  if (packed != nullptr) {   // the caller's image (vmlmf_pack_params): nothing is packed here
    if ((rc = check_packed(packed, g, P, q)) != 0) return rc;
    pack = const_cast<float*>((const float*)packed) + PK_HDR;
  }
  float* gx = ws + L.f_gx;
  const RefP rp = to_refp(p);
  if (packed == nullptr && !pl.direct && (rc = run(SL_PACK, s, "pack", [&] { return launch_pack(g, rp, P, pack, s); })) != 0) return rc;
  float* const qxbuf = g.training ? rs + L.r_qx : (g.generic ? ws + L.f_qx : nullptr);
  if (!pl.xwave && (rc = run(SL_XPROJ, s, "xproj", [&] {
        return g.wide ? wide_xproj(g, P, pack, x, ws + L.f_xrows, gx, qxbuf, s) : launch_xproj(g, P, pack, x, gx, qxbuf, s);
      })) != 0) return rc;
  if (pl.family == FAM_RB) {
    if (packed == nullptr && (rc = run(SL_PACK, s, "rb_pack", [&] {
          return launch_rb_pack(g, q, rp, pack + P.RB, s, reinterpret_cast<unsigned*>(ws + L.f_flag));
        })) != 0) return rc;
    RbIo io;
    memset(&io, 0, sizeof(io));
    io.flags_zeroed = packed == nullptr ? 1 : 0;
    io.gx = gx, io.EH = pack + P.EH, io.h0 = h0, io.c0 = c0, io.img = pack + P.RB, io.y = y, io.hT = hT, io.cT = cT;
    io.gates = g.training ? rs + L.r_gates : nullptr, io.cs = g.training ? rs + L.r_cs : nullptr;
    io.Qs = g.training ? rs + L.r_Qs : nullptr;
    io.xq = ws + L.f_xq, io.flag = reinterpret_cast<unsigned*>(ws + L.f_flag), io.status = status_word(s);
    io.drop = drop;
    if ((rc = run(SL_REC_FWD, s, "rb_fwd", [&] { return launch_rb_fwd(g, q, io, s); })) != 0) return rc;
    return head_and_ce_after(g, head, ce, hT, s);
  }
  if (pl.family == FAM_STEP) {
    GenericBuf w;
    memset(&w, 0, sizeof(w));
    w.gx = gx, w.EH = pack + P.EH, w.h0 = h0, w.c0 = c0, w.Ud = pack + P.UD, w.Vd = pack + P.VD;
    w.UdT = pack + P.UDT;   // the skinny products read both operands along k
    w.zeros = ws + L.f_zeros, w.y = y, w.hT = hT, w.cT = cT;
    w.gates = g.training ? rs + L.r_gates : nullptr, w.cs = g.training ? rs + L.r_cs : nullptr;
    w.Qs = g.training ? rs + L.r_Qs : nullptr, w.Qtmp = ws + L.f_Qtmp, w.P = ws + L.f_P, w.ccar = ws + L.f_ccar;
    split_k(&w, g, ws + L.f_part, pack, P);
    if (h0 == nullptr) {
      rc = (int)hipMemsetAsync(ws + L.f_zeros, 0, sizeof(float) * (size_t)g.B * g.H, s);
      if (rc != 0) return hip_fail(rc, "memset");
    }
    if ((rc = run(SL_REC_FWD, s, "generic_forward", [&] { return generic_forward(g, w, s); })) != 0) return rc;
    return head_and_ce_after(g, head, ce, hT, s);
  }
  FwdArgs a;
  a.gx = gx, a.VE = pack + P.VE, a.UR = pack + P.UR, a.EH = pack + P.EH, a.h0 = h0, a.c0 = c0;
  a.y = y, a.hT = hT, a.cT = cT, a.trash = ws + L.f_trash;
  a.gates = g.training ? rs + L.r_gates : nullptr;
  a.cs = g.training ? rs + L.r_cs : nullptr;
  a.Qs = g.training ? rs + L.r_Qs : nullptr;
  XwArgs xw;
  xw.x = x, xw.UXP = pack + P.UXP, xw.WXD = pack + P.WXD, xw.BBT = pack + P.BBT;
  memset(&xw.hd, 0, sizeof(xw.hd));
  if (pl.head_inside) xw.hd.W = head->weight, xw.hd.bias = head->bias, xw.hd.logits = head->logits, xw.hd.C = head->classes;
  memset(&xw.ce, 0, sizeof(xw.ce));
  if (pl.head_inside && ce != nullptr && g.R == 1 && g.B < 65536) {   // one batch row per workgroup: the row's terms are workgroup-local
    xw.ce.tgt = (const long long*)ce->target, xw.ce.ignore = (long long)ce->ignore_index, xw.ce.loss = ce->loss, xw.ce.nvalid = ce->nvalid;
    xw.ce.lse = ce->lse, xw.ce.dz = ce->dlogits_unit, xw.ce.ticket = (unsigned long long*)ce->ticket;
  }
  a.xwave = pl.xwave ? 1 : 0, a.qxw = g.training ? rs + L.r_qx : nullptr;
  xw.BH = nullptr, xw.DX = nullptr, xw.direct = 0, xw.pad = 0;
  if (pl.direct) {   // the reference's own tensors in the places of the images (vmlmf_direct.inc)
    a.VE = p->v_h[0], a.UR = p->u_h[0], a.EH = p->dia_h, a.xwave = 3;
    xw.UXP = p->u_x, xw.WXD = p->v_x, xw.BBT = p->b_x, xw.BH = p->b_h, xw.DX = p->dia_x, xw.direct = 1;
  }
  a.prog = g.training ? reinterpret_cast<unsigned*>(rs + L.r_prog) : nullptr;
  if ((rc = pl.fwd == K_REC3 ? run(SL_REC_FWD, s, "rec3_fwd", [&] { return launch_rec3_fwd(g, a, xw, s); })
                             : run(SL_REC_FWD, s, "rec_fwd", [&] { return launch_rec_fwd(g, a, xw, s); })) != 0) return rc;
  if (ce != nullptr && xw.ce.tgt == nullptr && (rc = ce_after(g.B, head, ce, s)) != 0) return rc;   // (a batch beyond the ticket's 16-bit row count)
  return debug_status(s);
}

int vmlmf_seq_backward(const vmlmf_desc* d, const vmlmf_params* p, const float* x, const float* h0,
                       const float* c0, const float* y, const void* reserve, const float* dy,
                       const float* dhT, const float* dcT, float* dx, float* dh0, float* dc0,
                       const vmlmf_grads* gr, void* workspace, size_t workspace_bytes, void* stream) {
  return vmlmf_seq_backward_packed(d, p, x, h0, c0, y, reserve, dy, dhT, dcT, dx, dh0, dc0, gr, workspace, workspace_bytes, stream,
                                   nullptr);
}

int vmlmf_seq_backward_packed(const vmlmf_desc* d, const vmlmf_params* p, const float* x, const float* h0,
                              const float* c0, const float* y, const void* reserve, const float* dy,
                              const float* dhT, const float* dcT, float* dx, float* dh0, float* dc0,
                              const vmlmf_grads* gr, void* workspace, size_t workspace_bytes, void* stream,
                              const void* packed) {
  vmlmf_extra ex = {};   // every field the caller does not set is a null pointer (drop, ce, ...)
  ex.packed = packed, ex.head = nullptr, ex.ce = nullptr;
  return vmlmf_seq_backward_ex(d, p, x, h0, c0, y, reserve, dy, dhT, dcT, dx, dh0, dc0, gr, workspace, workspace_bytes, stream, &ex);
}

int vmlmf_seq_backward_ex(const vmlmf_desc* d, const vmlmf_params* p, const float* x, const float* h0,
                          const float* c0, const float* y, const void* reserve, const float* dy,
                          const float* dhT, const float* dcT, float* dx, float* dh0, float* dc0,
                          const vmlmf_grads* gr, void* workspace, size_t workspace_bytes, void* stream,
                          const vmlmf_extra* ex) {
  const void* packed = ex != nullptr ? ex->packed : nullptr;
  const vmlmf_head* head = (ex != nullptr && ex->head != nullptr && ex->head->classes != 0) ? ex->head : nullptr;
  VGeo g;
  RbGeo q;
  int rc = take_status();
  if (rc != 0) return rc;
  if ((rc = make_geo(d, &g, &q)) != 0) return rc;
  if ((rc = check_params(g, p)) != 0) return rc;
  if (x == nullptr || y == nullptr || reserve == nullptr || workspace == nullptr || gr == nullptr)
    return fail(VMLMF_E_BADARG, "null x / y / reserve / workspace / grads");
  if ((rc = check_grads(g, gr)) != 0) return rc;
  if ((rc = check_head(g, head, false)) != 0) return rc;
  LayerPlan pl = plan_layer(g, p, packed != nullptr, head != nullptr, dx != nullptr);
  DropArgs drop;
  if ((rc = make_drop(ex != nullptr ? ex->drop : nullptr, g, false, &drop)) != 0) return rc;
  const VPack P = vg_pack_layout(g, q.total);
  const Layout L = make_layout(g, P, q);
  if (workspace_bytes < (size_t)L.ws_total() * sizeof(float))
    return fail(VMLMF_E_WORKSPACE, "workspace smaller than vmlmf_query() reported");
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const float* rs = (const float*)reserve;
  // final hidden state of the layer = last time slice of y
  const float* hlast = y + (size_t)(g.T - 1) * g.syT;
  const HeadBwd hb = head_bwd_args(pl.head_inside ? head : nullptr, g, y);
  if (head != nullptr && !pl.head_inside) {
    // stand-alone head kernel: dh into scratch, which then is the dhT of the recurrence
    if (dhT != nullptr) return fail(VMLMF_E_UNSUPPORTED, "head together with an explicit dhT: only on the VALU recurrent kernels");
    float* tmp = ws + L.b_headdh;
    if ((rc = run(SL_HEAD_BWD, s, "head_bwd", [&] {
           return launch_head_bwd(g.B, g.H, head->classes, hlast, g.syB, head->weight, head->dlogits, tmp, head->dweight, head->dbias, s);
         })) != 0) return rc;
    dhT = tmp;
  }
  const float* pack = rs + L.r_pack;
  if (packed != nullptr) {   // the image the matching forward was given
    if ((rc = check_packed(packed, g, P, q)) != 0) return rc;
    pack = (const float*)packed + PK_HDR;
  }
  if (pl.family == FAM_RB) {
    RbIo io;
    memset(&io, 0, sizeof(io));
    io.gates = const_cast<float*>(rs + L.r_gates), io.cs = const_cast<float*>(rs + L.r_cs), io.EH = pack + P.EH;
    io.img = pack + P.RB, io.dy = dy, io.dhT = dhT, io.dcT = dcT, io.dpre = ws + L.b_dpre, io.dQs = ws + L.b_dQs;
    io.dh0 = dh0, io.dc0 = dc0, io.xq = ws + L.b_xq, io.flag = reinterpret_cast<unsigned*>(ws + L.b_flag), io.status = status_word(s);
    io.drop = drop;
    if ((rc = run(SL_REC_BWD, s, "rb_bwd", [&] { return launch_rb_bwd(g, q, io, s); })) != 0) return rc;
    if (g.generic) {   // large layer: dqx as one skinny product over all rows, then dx
      GenericBuf w;
      memset(&w, 0, sizeof(w));
      w.dpre = ws + L.b_dpre, w.VxT = pack + P.VXTT, w.dqx = ws + L.b_dqx, w.dx = dx, w.UXP = pack + P.UXP, w.EXT = pack + P.EXT;
      split_k(&w, g, ws + L.b_part, pack, P);
      if ((rc = run(SL_DQX_DX, s, "dqx_dx", [&] { return generic_dqx_dx(g, w, s); })) != 0) return rc;
    } else if ((rc = run(SL_DQX_DX, s, "dqx_dx", [&] { return launch_wgrad_x(g, wgx_args(L, P, pack, ws, dx), s); })) != 0) {
      return rc;
    }
  } else if (pl.family == FAM_STEP) {
    GenericBuf w;
    memset(&w, 0, sizeof(w));
    w.EH = pack + P.EH, w.gates = const_cast<float*>(rs + L.r_gates), w.cs = const_cast<float*>(rs + L.r_cs);
    w.dy = dy, w.dhT = dhT, w.dcT = dcT, w.UdT = pack + P.UDT, w.VdT = pack + P.VDT, w.VxT = pack + P.VXTT;
    w.UXP = pack + P.UXP, w.EXT = pack + P.EXT, w.Vd = pack + P.VD;
    w.dpre = ws + L.b_dpre, w.dQs = ws + L.b_dQs, w.dHrec = ws + L.b_dHrec, w.ehterm = ws + L.b_ehterm;
    w.dcar = ws + L.b_dcar, w.dh0 = dh0, w.dc0 = dc0, w.dqx = ws + L.b_dqx, w.dx = dx;
    if (g.wide) {   // dqx U_x^T goes to the last piece of the wide scratch (wide_scratch_floats)
      w.UXT = pack + P.UXT;
      w.dxs = ws + L.b_total - ((long long)g.T * g.B * g.I + 63) / 64 * 64;
    }
    split_k(&w, g, ws + L.b_part, pack, P);
    if ((rc = run(SL_REC_BWD, s, "generic_backward", [&] { return generic_backward(g, w, s); })) != 0) return rc;
  } else if ((rc = valu_backward(g, &pl, L, P, pack, p, LayerBwdIo{x, y, h0, c0, dy, dhT, dcT, dx, dh0, dc0}, hb, rs, ws, s)) != 0) {
    return rc;
  }
  if ((rc = backward_tail(g, pl, L, p, gr, x, y, h0, rs, ws, hb, s)) != 0) return rc;
  return debug_status(s);
}

}  // extern "C"
