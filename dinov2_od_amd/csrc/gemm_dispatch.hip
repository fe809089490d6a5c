// Executor of the inference GEMM plans (gemm_plan.h): the one place that gathers what the dispatch policy reads -- the device's CU count, the
// scratch reserved, the test options, the tuning-build overrides, the policy-relevant facts of the epilogue -- and runs a plan's steps through
// the run_* function of each form (dod_common.h).  launch_gemm_bf16 / _x3 / _h2 / _fp8 / _f32 check their arguments and end here.
// The dispatch's per-device process state lives here too: the CU counts and the two scratch pools (SlabPool).
#include "dod_common.h"
#include "gemm_epi.h"
#include "gemm_plan.h"
#include "stream_slabs.h"
#include <atomic>
#include <cstring>
#include <mutex>

int current_device_slot() {
  int dev = 0;
  return hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 16 ? dev : -1;
}

int device_cus() {
  static std::atomic<int> cus[16];
  const int dev = current_device_slot();
  if (dev < 0) return 256;
  int c = cus[dev].load();
  if (!c) { (void)hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev); c = c > 0 ? c : 256; cus[dev].store(c); }
  return c;
}

void gemm_lds_attr_once(bool* done, const KernelLds* k, int n) {
  const int dev = current_device_slot();
  if (dev < 0 || done[dev]) return;
  for (int i = 0; i < n; ++i) (void)hipFuncSetAttribute(k[i].fn, hipFuncAttributeMaxDynamicSharedMemorySize, k[i].bytes);
  done[dev] = true;
}

// ---- stream-slab pool: per device, blocks of SLAB_SLOTS slabs, one slab per launching stream (stream_slabs.h holds the rule).  reserve()
// runs outside any stream capture.  A pool only ever GROWS, by adding a block (at most max_gens of them), and never frees one: captured
// hipGraphs keep slab addresses.  The newest block is the one handed out; growing forgets the owners.
#define SLAB_SLOTS 4
struct SlabPool {
  const int max_gens;          // blocks a device may ever get
  const bool zero_fill;        // the block starts zeroed (a pool whose kernels leave their counters zero between launches)
  std::mutex mu;               // autograd / DataLoader threads may launch GEMMs beside the main thread
  struct Dev { char* block; int gens; size_t bytes; StreamSlabs<SLAB_SLOTS> slots; } dev[16] = {};

  // 0: every slab of the current device holds `bytes`; 3: no device, the generation limit, or the allocation failed
  int reserve(size_t bytes) {
    const int d = current_device_slot();
    if (d < 0) return 3;
    std::lock_guard<std::mutex> lk(mu);
    Dev& v = dev[d];
    if (v.bytes >= bytes) return 0;
    if (v.gens >= max_gens) return 3;  // never free a block a captured graph may still reference: refuse instead
    char* blk = nullptr;
    if (hipMalloc((void**)&blk, bytes * SLAB_SLOTS) != hipSuccess) return 3;
    if (zero_fill && hipMemset(blk, 0, bytes * SLAB_SLOTS) != hipSuccess) { (void)hipFree(blk); return 3; }
    v.block = blk; ++v.gens; v.bytes = bytes;
    v.slots.reset();
    return 0;
  }
  size_t reserved() {                  // bytes per slab on the current device (0: none)
    const int d = current_device_slot();
    if (d < 0) return 0;
    std::lock_guard<std::mutex> lk(mu);
    return dev[d].bytes;
  }
  char* slab(hipStream_t s) {          // the launching stream's slab (null: nothing reserved)
    const int d = current_device_slot();
    if (d < 0) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    Dev& v = dev[d];
    return v.block ? v.block + (size_t)v.slots.pick(s) * v.bytes : nullptr;
  }
};
static SlabPool g_tail_pool{4, false};      // tail split's K-split partials (gemm_pp.hip): sized by the caller, growable
// fp32 K split (gemm_f32.hip): one fixed size -- F32K_TILES counters (zero between launches) + partials of at most F32K_PARTS (tile, slice)
// pairs; the planner (gemm_plan.h) drops the split beyond them
static SlabPool g_f32k_pool{1, true};
static constexpr size_t F32K_SLAB = (size_t)F32K_TILES * 4 + (size_t)F32K_PARTS * 16 * 256 * 4;
int gemm_tail_reserve(size_t bytes) { return g_tail_pool.reserve(bytes); }
size_t gemm_tail_reserved() { return g_tail_pool.reserved(); }
float* gemm_tail_slab(hipStream_t s) { return reinterpret_cast<float*>(g_tail_pool.slab(s)); }
int gemm_f32_ksplit_reserve() { return g_f32k_pool.reserve(F32K_SLAB); }
bool gemm_f32_ksplit_reserved() { return g_f32k_pool.reserved() != 0; }
char* gemm_f32_ksplit_slab(hipStream_t s) { return g_f32k_pool.slab(s); }

// Every tuning-build switch that steers the dispatch (include/dinodet_tuning.h).  The release build reads no environment: DOD_TUNE_ENV is a null
// constant there and this folds to GemmTune's defaults.  The tile overrides are read per call (tools/ flip them between launches), the rest once.
static GemmTune gemm_tune() {
  static const GemmTune once = [] {
    GemmTune t;
    if (const char* v = DOD_TUNE_ENV("DINODET_GEMM_REMCUT")) t.rem_div = atoi(v);
    if (const char* v = DOD_TUNE_ENV("DINODET_GEMM_M16_BIAS")) t.m16_bias = atof(v);
    if (const char* v = DOD_TUNE_ENV("DINODET_GEMM_RING")) t.ring = atoi(v);
    if (const char* v = DOD_TUNE_ENV("DINODET_GEMM_KSPLIT0")) t.k0frac = atoi(v);
    if (const char* v = DOD_TUNE_ENV("DINODET_GEMM_TAILSPLIT")) t.tailsplit = v[0] == '0' ? 0 : (v[0] == '2' ? 2 : 1);
    if (const char* v = DOD_TUNE_ENV("DINODET_FP8_TILE")) t.fp8_big = atoi(v);
    if (const char* v = DOD_TUNE_ENV("DINODET_F32_KSPLIT")) t.f32_ksplit = atoi(v);
    return t;
  }();
  GemmTune t = once;
  if (const char* v = DOD_TUNE_ENV("DINODET_GEMM_TILE")) t.tile = v[0];
  if (const char* v = DOD_TUNE_ENV("DINODET_X3_TILE")) t.x3_tile = v[0];
  return t;
}

// the policy inputs that are process state: test options and tuning overrides (what dod_test_gemm_plan shares with the launchers)
GemmPolicy gemm_policy(int cus, size_t tail_bytes, bool f32_slab) {
  GemmPolicy p;
  p.cus = cus; p.tail_bytes = tail_bytes; p.f32_slab = f32_slab;
  p.opt_tailsplit = dod_option(DOD_OPT_TAILSPLIT); p.opt_f32_ksplit = dod_option(DOD_OPT_F32_KSPLIT); p.opt_epi_regmath = dod_option(DOD_OPT_EPI_REGMATH);
  p.tune = gemm_tune();
  return p;
}

static unsigned plan_epi_flags(const GemmEpi& e, int N, bool allow_ksplit) {
  return (e.act == ACT_GELU ? PE_GELU : 0) | (e.act == ACT_SIGMOID ? PE_SIGMOID : 0) | (e.rows_per_img != 0 ? PE_ROWMAP : 0) | (e.a_scale ? PE_A_SCALE : 0) |
         (e.out_split > 0 ? PE_OUT_SPLIT3 : 0) | (e.ksplit > 1 ? PE_KSPLIT : 0) | (gemm_epi_rows_ok(e) ? PE_ROWS_OK : 0) | (epi_regmath_ok(e, N) ? PE_REGMATH_OK : 0) |
         (e.a_bs ? PE_A_BS : 0) | (e.w_bs ? PE_W_BS : 0) | (e.out_bs ? PE_OUT_BS : 0) | (allow_ksplit ? PE_ALLOW_KSPLIT : 0);
}

static std::atomic<long> g_rem_cuts{0}, g_tail_splits{0}, g_f32k_count{0}, g_epi_regmath{0};
long gemm_rem_cut_count() { return g_rem_cuts.load(); }
long gemm_tail_split_count() { return g_tail_splits.load(); }
long gemm_f32_ksplit_count() { return g_f32k_count.load(); }
long gemm_epi_regmath_count() { return g_epi_regmath.load(); }

int gemm_dispatch(int family, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const GemmEpi& e, hipStream_t s, bool allow_ksplit) {
  const GemmPolicy pol = gemm_policy(device_cus(), family <= GEMM_H2 ? gemm_tail_reserved() : 0, family == GEMM_F32 && gemm_f32_ksplit_reserved());
  const GemmPlan plan = gemm_plan(family, M, N, K, plan_epi_flags(e, N, allow_ksplit), pol);
  if (!gemm_plan_tiles(plan, M)) return 2;
  const size_t row_bytes = (size_t)lda * (family == GEMM_BF16 || family == GEMM_X3 ? 2 : (family == GEMM_F32 ? 4 : 1));      // lda: elements (bf16, fp32) or bytes
  float* scratch = nullptr;
  for (int i = 0; i < plan.n; ++i) {
    const GemmStep& st = plan.step[i];
    if (st.form == FORM_KSPLIT_REDUCE) {      // + the caller's epilogue on global rows row0 .. row0 + rows - 1
      ++g_tail_splits;
      if (const int rc = run_gemm_ksplit_reduce(scratch, st.kslices, st.rows, N, e, st.row0, M, K, s)) return rc;
      continue;
    }
    const char* Ar = (const char*)A + (size_t)st.row0 * row_bytes;
    GemmEpi er;
    if (st.kslices > 1 && family != GEMM_F32) {      // K-split launch of the tail split: fp32 partial slabs, no epilogue term
      if (K % (st.kslices * (family == GEMM_BF16 ? 64 : 32)) != 0) return 2;                  // whole K-tiles per slice
      if (gemm_tail_reserved() < (size_t)st.rows * N * st.kslices * 4 || !(scratch = gemm_tail_slab(s))) return 2;      // the slabs fit the scratch
      memset(&er, 0, sizeof er);
      er.out_f32 = scratch; er.ldc = N; er.h2_wexp = e.h2_wexp;
      er.ksplit = st.kslices; er.kslice_len = K / st.kslices; er.kslice_stride = (long long)st.rows * N;
    } else if (st.row0 > 0) {                        // the cut rows of a remainder cut: a launch of their own
      if (!gemm_epi_rows_ok(e)) return 2;
      ++g_rem_cuts;
      er = gemm_epi_rows(e, st.row0);
    } else er = e;
    gemm_form_launched(st.form);
    int rc;
    switch (st.form) {
      case FORM_BF16_128_R2: case FORM_BF16_128_R3:
        rc = run_gemm_bf16_128((const bf16_t*)Ar, lda, (const bf16_t*)W, ldw, st.rows, N, K, er, st.form == FORM_BF16_128_R3 ? 3 : 2, s); break;
      case FORM_BF16_M16: rc = run_gemm_bf16_m16((const bf16_t*)Ar, lda, (const bf16_t*)W, ldw, st.rows, N, K, er, st.gm, s); break;
      case FORM_K64:
        if (st.regmath) ++g_epi_regmath;
        rc = run_gemm_k64((const bf16_t*)Ar, lda, (const bf16_t*)W, ldw, st.rows, N, K, er, st.regmath != 0, s); break;
      case FORM_PPM: case FORM_X3_PP: rc = run_gemm_pp(st.form == FORM_X3_PP, (const bf16_t*)Ar, lda, (const bf16_t*)W, ldw, st.rows, N, K, er, s); break;
      case FORM_X3_16W: rc = run_gemm_x3_16w((const bf16_t*)Ar, lda, (const bf16_t*)W, ldw, st.rows, N, K, er, s); break;
      case FORM_H2: rc = run_gemm_h2(Ar, lda, W, ldw, st.rows, N, K, er, s); break;
      case FORM_F32:
        if (st.kslices > 1) ++g_f32k_count;
        rc = run_gemm_f32((const float*)Ar, lda, (const float*)W, ldw, st.rows, N, K, er, st.kslices, s); break;
      default: rc = run_gemm_fp8(st.form, (const unsigned char*)Ar, lda, (const unsigned char*)W, ldw, st.rows, N, K, er, st.gm, s); break;
    }
    if (rc) return rc;
  }
  return 0;
}
