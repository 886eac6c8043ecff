// Process state of the C ABI: error text, the switch table and vmlmf_tune, the status and health words, profiling.
#include <atomic>
#include <cstdlib>

#include "vmlmf_host.h"

using namespace vmlmf_host;

int vmlmf_env_switch(const char* name, EnvRule rule, int dflt) {
  const char* e = getenv(name);
  if (e == nullptr) return dflt;
  switch (rule) {
    case ENV_SET: return 1;
    case ENV_ON: return e[0] != '0';
    case ENV_INT: return atoi(e);
    case ENV_POS: break;
  }
  const int v = atoi(e);
  return v >= 1 ? v : dflt;
}

namespace vmlmf_host {

static thread_local std::string g_err = "";

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

Prof g_prof;

// ---- process-wide switches: one row each in g_switches (the vmlmf_tune keys are documented in include/vmlmf_hip.h) ----
int g_debug_sync, g_adam_guard, g_xwave, g_wchunks, g_wmin, g_rc, g_wride, g_wride_k, g_wride_maxb, g_wride_lag, g_wride_rc, g_rb_mode,
    g_rb_minB, g_rb_S, g_rb_rows, g_rec3, g_inrow, g_wring, g_direct, g_finish2, g_wf_bwd, g_pack_slim, g_finish_units, g_rbx, g_ffb;
struct Switch {
  const char* env;
  const char* key;   // vmlmf_tune / vmlmf_tune_get key, or NULL (environment only)
  int dflt;
  EnvRule rule;
  int* var;
};
// ("wride" is no row's key: vmlmf_tune("wride") moves the trip latch below, not VMLMF_WRIDE's setting; vmlmf_tune clamps the rb_* keys)
const Switch g_switches[] = {
    // synchronise after every internal launch and name it on stderr (finds the kernel behind an asynchronous GPU fault; never set in
    // production: it serialises everything and breaks hipGraph capture)
    {"VMLMF_DEBUG_SYNC", nullptr, 0, ENV_SET, &g_debug_sync},
    {"VMLMF_ADAM_GUARD", "adam_guard", 1, ENV_INT, &g_adam_guard},
    {"VMLMF_XWAVE", nullptr, 1, ENV_ON, &g_xwave},   // 0: the x projection always as a launch of its own
    // weight-gradient chunking (A/B): target row chunks, fewest rows per chunk (config C, 3072 rows: 0.2546 ms at 32 or 48, 0.2428 at
    // 64, 0.243 at 96), dqx_dx rows per workgroup (0: from the row count).  Positive or the default: a zero divides by zero in make_geo
    {"VMLMF_WCHUNKS", nullptr, 64, ENV_POS, &g_wchunks},
    {"VMLMF_WMIN", nullptr, 64, ENV_POS, &g_wmin},
    {"VMLMF_RC", nullptr, 0, ENV_POS, &g_rc},
    // weight-gradient workers riding on the recurrent backward launch (vmlmf_atb.inc): on / off, workers per task, the largest batch
    // that rides (round 3, H = 180, T = 128, ride on / off: B 32 0.158 / 0.165 ms, 64 0.160 / 0.173, 72 0.185 / 0.178, 96 0.192 /
    // 0.181 - beyond 64 the faster rows outrun the workers), segments a progress word trails, rows per chunk
    {"VMLMF_WRIDE", nullptr, 1, ENV_ON, &g_wride},
    {"VMLMF_WRIDE_K", nullptr, 32, ENV_POS, &g_wride_k},
    {"VMLMF_WRIDE_MAXB", nullptr, 64, ENV_POS, &g_wride_maxb},
    {"VMLMF_WRIDE_LAG", nullptr, WR_LAG_DEFAULT, ENV_POS, &g_wride_lag},
    {"VMLMF_WRIDE_RC", nullptr, 32, ENV_POS, &g_wride_rc},
    // row-block MFMA kernels (vmlmf_rb.hip).  rb_min_batch 0 = never: measured the one-row-per-CU kernels win
    // at every batch up to 2048 - sixteen rows' tape traffic through ONE CU's memory pipe costs more than the MFMAs save
    {"VMLMF_RB", "rb", -1, ENV_INT, &g_rb_mode},
    {"VMLMF_RB_MINB", "rb_min_batch", 0, ENV_POS, &g_rb_minB},
    {"VMLMF_RB_S", "rb_cluster", 0, ENV_POS, &g_rb_S},
    {"VMLMF_RB_ROWS", "rb_rows", 0, ENV_POS, &g_rb_rows},
    // bit 4: rec3_fwd_kernel needs ~170 VGPRs (two workgroups share a CU), rec_fwd_kernel's x-projection wave 256 (its workgroups run
    // in rounds): B = 512 138 -> 104 us, 0.402 -> 0.370 ms per step; up to B = 256 the two tie
    {"VMLMF_REC3", "rec3", 6, ENV_INT, &g_rec3},
    {"VMLMF_INROW", "inrow", -1, ENV_INT, &g_inrow},
    {"VMLMF_WRING", "wring", -1, ENV_INT, &g_wring},
    {"VMLMF_DIRECT", "direct", 1, ENV_INT, &g_direct},
    {"VMLMF_FINISH2", "finish2", 1, ENV_INT, &g_finish2},
    // stacks (A/B; 0 = off): the wavefront backward (else the per-layer kernels, chained), the slim pack launch (else every image of
    // pack_kernel), the one finishing launch (else reduce_cg_stack_kernel + finish_stack_kernel)
    {"VMLMF_WF_BWD", nullptr, 1, ENV_INT, &g_wf_bwd},
    {"VMLMF_PACK_SLIM", nullptr, 1, ENV_INT, &g_pack_slim},
    {"VMLMF_FINISH_UNITS", nullptr, 1, ENV_INT, &g_finish_units},
    {"VMLMF_RBX", "rbx", 1, ENV_INT, &g_rbx},
    // ffb 0 by default: measured slower - config C's finish_stack_kernel 25.5 us against reduce 8.1 + finish 6.2 (the repeated block sums
    // of the d(ex) / d(eh) rows); two PTB group layers at 32 rows 0.710 ms with, 0.702 without
    {"VMLMF_FFB", "ffb", 0, ENV_INT, &g_ffb},
};
static int read_switches() {
  for (const Switch& w : g_switches) *w.var = vmlmf_env_switch(w.env, w.rule, w.dflt);
  return 0;
}
static const int g_switches_read = read_switches();
static const Switch* find_switch(const std::string& key) {
  for (const Switch& w : g_switches)
    if (w.key != nullptr && key == w.key) return &w;
  return nullptr;
}

// ---- protocol failures inside a launch ----
// The riding weight-gradient workers, the clusters of the row-block kernels and the wavefront hand-overs all wait for other
// workgroups with a bounded number of looks; a wait that gives up leaves NaN in the results (never a plausible wrong number)
// and a code in a status word.  The word lives in host memory mapped into the device (one per device, allocated at the first
// call): the kernel's store costs nothing unless it happens, and the host reads it without a copy or a synchronisation.
// Every forward / backward entry point looks at it first: a failure of an EARLIER launch on the device comes back as
// VMLMF_E_PROTOCOL from the next call (under VMLMF_DEBUG_SYNC from the failing call itself); vmlmf_check_status() after a
// synchronisation tells at once.
constexpr int MAX_DEV = 16;
static std::atomic<unsigned*> g_status[MAX_DEV];
static std::atomic<bool> g_status_failed[MAX_DEV];   // the allocation itself failed (not: was skipped because of a capture)
static std::mutex g_status_mu;
// beside it, in DEVICE memory: the gradient-health word.  finish_kernel sets it when a parameter gradient it writes is not
// finite (the NaN partial products of a launch that gave up a wait); the package's Adam reads it in its tick launch and skips
// that step, then clears it (vmlmf_optim.hip).  Device memory, because the tick launch reads it in every step.
static std::atomic<unsigned*> g_health[MAX_DEV];

// `s`: the stream the caller is about to launch on.  The first call on a device allocates the word; that allocation is not
// capturable, so a first call made while `s` is being captured returns NULL WITHOUT remembering anything (the launch simply
// carries no word; the next call outside a capture allocates it).  Torch captures on a side stream, never the null stream:
// the caller's own stream is what has to be asked.
unsigned* status_word(hipStream_t s) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) return nullptr;
  unsigned* w = g_status[dev].load(std::memory_order_acquire);
  if (w != nullptr || g_status_failed[dev].load(std::memory_order_acquire)) return w;
  std::lock_guard<std::mutex> lk(g_status_mu);
  w = g_status[dev].load(std::memory_order_acquire);
  if (w != nullptr || g_status_failed[dev].load(std::memory_order_acquire)) return w;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  if (cs != hipStreamCaptureStatusNone) return nullptr;          // not now; nothing is latched
  // another thread of the process may be capturing in global mode: the allocation must not invalidate its capture
  hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
  const bool swapped = hipThreadExchangeStreamCaptureMode(&mode) == hipSuccess;
  void* p = nullptr;
  const bool ok = hipHostMalloc(&p, 64, hipHostMallocMapped) == hipSuccess && p != nullptr;
  void* hw = nullptr;
  if (ok && hipMalloc(&hw, 256) == hipSuccess && hw != nullptr) {
    if (hipMemset(hw, 0, 256) == hipSuccess) g_health[dev].store((unsigned*)hw, std::memory_order_release);
  } else {
    (void)hipGetLastError();
  }
  if (swapped) (void)hipThreadExchangeStreamCaptureMode(&mode);
  if (ok) {
    memset(p, 0, 64);
    g_status[dev].store((unsigned*)p, std::memory_order_release);
    return (unsigned*)p;
  }
  (void)hipGetLastError();
  g_status_failed[dev].store(true, std::memory_order_release);
  return nullptr;
}
unsigned* health_word(hipStream_t s) {   // allocated together with the status word
  (void)status_word(s);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) return nullptr;
  return g_health[dev].load(std::memory_order_acquire);
}
// the word if it exists already (host-side readers: never allocates)
static unsigned* status_word_if_any() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) return nullptr;
  return g_status[dev].load(std::memory_order_acquire);
}

// looks a riding weight-gradient worker takes at its rows' progress words before it gives up (vmlmf_tune "test_wride_spin": tests)
constexpr int WRIDE_SPIN_DEFAULT = 1 << 16;
int g_wride_spin = WRIDE_SPIN_DEFAULT;
// set when a worker gave up under the production bound: the workers wait for row workgroups of their own launch, which a GPU
// shared with other processes / launches can keep from getting a CU.  From then on the process takes the
// stand-alone weight-gradient kernel (plan_wride) instead of failing every step; vmlmf_tune("wride", 1) re-arms the riding form.
// (Launches already captured into a hipGraph stay what they are.)
std::atomic<int> g_wride_tripped{0};
std::atomic<int> g_ring_launches{0};

static const char* status_text(unsigned code) {
  switch (code) {
    case VMLMF_ST_WRIDE: return "a weight-gradient worker riding on the backward launch never saw its rows' progress words (parameter gradients of that call are NaN); the workers wait for workgroups of their own launch and need them resident: when the GPU is shared with other processes or launches that fill its CUs, run with VMLMF_WRIDE=0 (after this report the process does so by itself for eager launches)";
    case VMLMF_ST_CLUSTER: return "a member of a row-block cluster never published its partial (outputs of that call are NaN)";
    case VMLMF_ST_WF_FWD: return "a layer of a wavefront forward launch never received the rows of the layer below (outputs are NaN)";
    case VMLMF_ST_WF_BWD: return "a layer of a wavefront backward launch never received the gradient rows of the layer above (gradients are NaN)";
    case VMLMF_ST_P2P: return "a rank of the peer-to-peer all-reduce never wrote its buffer into this rank's staging area (the reduced buffer is NaN)";
  }
  return "unknown status code";
}

// 0, or VMLMF_E_PROTOCOL with the text of the failure an earlier launch on this device reported (the word is cleared)
int g_tune_generation = 0;                        // bumped by every vmlmf_tune() and by the automatic switch below: kept parameter images / captured graphs of an older one are stale
int take_status() {
  unsigned* w = status_word_if_any();
  if (w == nullptr) return 0;
  const unsigned code = *(volatile unsigned*)w;
  if (code == 0) return 0;
  *(volatile unsigned*)w = 0;
  if (code == VMLMF_ST_WRIDE && g_wride_spin == WRIDE_SPIN_DEFAULT && g_wride_tripped.exchange(1) == 0) ++g_tune_generation;
  return fail(VMLMF_E_PROTOCOL, std::string("an earlier launch on this device gave up a bounded wait: ") + status_text(code));
}
// at the end of an entry point under VMLMF_DEBUG_SYNC: the failure of THIS call
int debug_status(hipStream_t s) {
  if (!g_debug_sync) return 0;
  (void)hipStreamSynchronize(s);
  return take_status();
}

static int g_cus[MAX_DEV] = {0};   // compute units of the device (hipDeviceProp_t::multiProcessorCount), looked up once
int device_cus() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) return 256;
  if (g_cus[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    g_cus[dev] = n;
  }
  return g_cus[dev];
}

int hip_fail(int rc, const char* what) {
  if (rc == 0) return 0;
  if (rc == -3) return fail(VMLMF_E_UNSUPPORTED, std::string(what) + ": no kernel instantiation for this geometry");
  return fail(rc, std::string(what) + ": " + hipGetErrorString((hipError_t)rc));
}

}  // namespace vmlmf_host

unsigned* vmlmf_health_word_if_any() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) return nullptr;
  return g_health[dev].load(std::memory_order_acquire);
}
int vmlmf_adam_guard_mode() { return g_adam_guard; }

// error text for the other translation units of the C ABI (vmlmf_comm.cpp)
int vmlmf_set_error(int code, const std::string& msg) { return fail(code, msg); }
unsigned* vmlmf_status_word(void* stream) { return status_word((hipStream_t)stream); }   // (vmlmf_p2p.hip)

extern "C" {

int vmlmf_abi_version(void) { return VMLMF_ABI_VERSION; }

const char* vmlmf_build_info(void) { return "vmlmf_hip gfx950 fp32 persistent-rnn (register-resident U/V, DPP rank reduce)"; }

const char* vmlmf_last_error(void) { return g_err.c_str(); }

int vmlmf_tune_generation(void) { return g_tune_generation; }

int vmlmf_check_status(void) { return take_status(); }

int vmlmf_tune(const char* key, int value) {
  if (key == nullptr) return fail(VMLMF_E_BADARG, "tune: null key");
  const std::string k(key);
  const Switch* sw = find_switch(k);
  if (k == "test_wride_spin") g_wride_spin = value < 1 ? WRIDE_SPIN_DEFAULT : value;
  else if (k == "clear_health") {   // forget a non-finite gradient no guarded optimizer step has consumed (synchronises the device)
    unsigned* hw = vmlmf_health_word_if_any();
    if (hw != nullptr && hipMemset(hw, 0, sizeof(unsigned)) != hipSuccess) (void)hipGetLastError();
  }
  else if (k == "wride") g_wride_tripped.store(value != 0 ? 0 : 1);   // 0: stand-alone weight-gradient kernel; 1: ride again (where VMLMF_WRIDE allows)
  else if (k == "rb_min_batch" || k == "rb_cluster" || k == "rb_rows") *sw->var = value < 0 ? 0 : value;   // (rb_min_batch: 0 = never, the default)
  else if (sw != nullptr) *sw->var = value;
  else return fail(VMLMF_E_BADARG, "tune: unknown key " + k);
  ++g_tune_generation;
  return 0;
}

int vmlmf_tune_get(const char* key, int* value) {
  if (key == nullptr || value == nullptr) return fail(VMLMF_E_BADARG, "tune_get: null pointer");
  const std::string k(key);
  const Switch* sw = find_switch(k);
  if (k == "wride") *value = (g_wride && g_wride_tripped.load() == 0) ? 1 : 0;   // 0 also after a bounded wait gave up (VMLMF_ST_WRIDE)
  else if (k == "wring_launches") *value = g_ring_launches.load();   // read-only: how often wgrad_ring_kernel itself was launched
  else if (sw != nullptr) *value = *sw->var;
  else return fail(VMLMF_E_BADARG, "tune_get: unknown key " + k);
  return 0;
}

int vmlmf_profile_enable(int mask) {
  std::lock_guard<std::mutex> lk(g_prof.mu);
  g_prof.mask = (unsigned)mask;
  return 0;
}

int vmlmf_profile_read(float* usec_sum, int32_t* count, int reset) {
  std::lock_guard<std::mutex> lk(g_prof.mu);
  for (int k = 0; k < NKERN; ++k) {
    float sum = 0.f;
    for (auto& pr : g_prof.ev[k]) {
      (void)hipEventSynchronize(pr.second);
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, pr.first, pr.second);
      sum += ms * 1000.f;
    }
    if (usec_sum != nullptr) usec_sum[k] = sum;
    if (count != nullptr) count[k] = (int32_t)g_prof.ev[k].size();
    if (reset) {
      for (auto& pr : g_prof.ev[k]) {
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
      }
      g_prof.ev[k].clear();
    }
  }
  return 0;
}

const char* vmlmf_kernel_name(int k) { return kernel_label(k); }

}  // extern "C"
