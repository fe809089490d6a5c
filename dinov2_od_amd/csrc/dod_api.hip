// C ABI of libdinodet.so: handle life cycle, the forward entry points and the stateless dod_op_* operators.
// See include/dinodet.h for the contract; dod_pack.hip packs the weights, dod_forward.hip holds the forward schedules.
#include "dod_internal.h"
#include "gemm_plan.h"

#include <cstdarg>
#include <cstdio>
#include <atomic>
#include <cstdlib>

using namespace dod;

// The calling thread's message slot (include/dinodet.h "Errors"): every handle-less failure of the library is written here.
static thread_local std::string t_err;

static int vfail(const dod_handle* h, int code, const char* fmt, va_list ap, int launch_rc = 0) {
  char buf[512];
  const int n = vsnprintf(buf, sizeof buf, fmt, ap);
  if (launch_rc && n >= 0 && (size_t)n < sizeof buf) snprintf(buf + n, sizeof buf - n, " rejected (rc %d)", launch_rc);
  if (h) h->err = buf; else t_err = buf;
  return code;
}
int dod_fail(int code, const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); code = vfail(nullptr, code, fmt, ap); va_end(ap);
  return code;
}
int dod::fail(const dod_handle* h, int code, const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); code = vfail(h, code, fmt, ap); va_end(ap);
  return code;
}
int dod::rejected(const dod_handle* h, int r, const char* fmt, ...) {
  if (!r) return DOD_OK;
  va_list ap; va_start(ap, fmt); const int code = vfail(h, r == 3 ? DOD_ERR_HIP : DOD_ERR_INVALID, fmt, ap, r); va_end(ap);
  return code;
}

static bool check_common(dod_handle* h, int B, int H, int W, int* rc) {
  if (!h) { *rc = fail(nullptr, DOD_ERR_INVALID, "null handle"); return false; }
  if (!h->finalized) { *rc = fail(h, DOD_ERR_STATE, "dod_finalize_weights has not been called"); return false; }
  if (B <= 0) { *rc = fail(h, DOD_ERR_INVALID, "batch must be positive (got %d)", B); return false; }
  if (H < h->cfg.patch || W < h->cfg.patch) { *rc = fail(h, DOD_ERR_INVALID, "image %dx%d smaller than one %dx%d patch", H, W, h->cfg.patch, h->cfg.patch); return false; }
  return true;
}

// ---- test hooks (dod_common.h DOD_OPT_*)
static std::atomic<int> g_options[DOD_OPT_COUNT] = {{-1}, {-1}, {-1}, {-1}, {-1}, {-1}, {-1}, {-1}, {-1}, {-1}, {-1}, {-1}};
int dod_option(int which) { return which >= 0 && which < DOD_OPT_COUNT ? g_options[which].load() : -1; }
static const char* const k_option_names[DOD_OPT_COUNT] = {"tailsplit", "dec_fused_split", "mha_chunk_images", "no_fused_patch", "ln_fold", "deterministic", "f32_ksplit",
                                                       "attn_bwd_flash", "epi_regmath", "f32x3_tile", "attn_diet", "attn_fixed_ref"};

static std::atomic<long> g_form_launches[FORM_COUNT];
static const char* const k_form_names[FORM_COUNT] = {"bf16_128_r2", "bf16_128_r3", "bf16_m16", "k64", "ppm", "x3_16w", "x3_pp", "h2", "fp8_rows", "fp8mx_256x128",
                                                     "fp8mx2_256x128", "fp8mx2_256x256", "f32", "patch_fused"};
void gemm_form_launched(int form) { if (form >= 0 && form < FORM_COUNT) ++g_form_launches[form]; }

extern "C" {

int dod_test_set_option(const char* name, int value) {
  if (!name) return fail(nullptr, DOD_ERR_INVALID, "null option name");
  for (int i = 0; i < DOD_OPT_COUNT; ++i)
    if (!strcmp(name, k_option_names[i])) { g_options[i].store(value); return DOD_OK; }
  return fail(nullptr, DOD_ERR_INVALID, "unknown test option '%s'", name);
}
long dod_test_counter(const char* name) {
  if (name && !strcmp(name, "tail_splits")) return gemm_tail_split_count();
  if (name && !strcmp(name, "rem_cuts")) return gemm_rem_cut_count();
  if (name && !strcmp(name, "f32_ksplits")) return gemm_f32_ksplit_count();
  if (name && !strcmp(name, "epi_regmath")) return gemm_epi_regmath_count();
  if (name && !strcmp(name, "attn_diet")) return attn_half_tile_count();
  if (name && !strcmp(name, "attn_rerun")) return attn_rerun_count();
  if (name && !strcmp(name, "f32x3_launches")) return gemm_f32x3_count(0);
  if (name && !strcmp(name, "f32x3_wide_launches")) return gemm_f32x3_count(1);
  if (name && !strcmp(name, "optim_launches")) return optim_launch_count();
  if (name && !strcmp(name, "optim_chunk_elems")) return optim_constant(0);
  if (name && !strcmp(name, "optim_table_tensors")) return optim_constant(1);
  if (name && !strcmp(name, "optim_norm_table_tensors")) return optim_constant(2);
  if (name && !strcmp(name, "optim_ema_table_tensors")) return optim_constant(3);
  if (name && !strncmp(name, "form_", 5))
    for (int i = 0; i < FORM_COUNT; ++i)
      if (!strcmp(name + 5, k_form_names[i])) return g_form_launches[i].load();
  return -1;
}

int dod_test_gemm_plan(int family, int M, int N, int K, unsigned epi_flags, int cus, size_t scratch_bytes, dod_gemm_step* steps, int max_steps) {
  if (family < GEMM_BF16 || family > GEMM_F32 || M <= 0 || N <= 0 || K <= 0 || cus <= 0 || !steps) return -1;
  const GemmPlan pl = gemm_plan(family, M, N, K, epi_flags, gemm_policy(cus, scratch_bytes, scratch_bytes > 0));
  if (pl.n > 4 || pl.n > max_steps) return -1;
  for (int i = 0; i < pl.n; ++i) {
    const GemmStep& st = pl.step[i];
    steps[i].form = st.form; steps[i].row0 = st.row0; steps[i].rows = st.rows; steps[i].kslices = st.kslices; steps[i].regmath = st.regmath; steps[i].gm = st.gm;
  }
  return pl.n;
}

const char* dod_version(void) { return "dinodet 0.3 (gfx950)"; }
int dod_abi_version(void) { return DOD_ABI_VERSION; }

int dod_device_count(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : -1;
}

const char* dod_last_error(const dod_handle* h) { return h ? h->err.c_str() : t_err.c_str(); }
const char* dod_decoder_train_last_error(void) { return t_err.c_str(); }
const char* dod_optim_last_error(void) { return t_err.c_str(); }

int dod_create(const dod_config* cfg, dod_handle** out) {
  if (!cfg || !out) return fail(nullptr, DOD_ERR_INVALID, "null argument");
  const dod_config& c = *cfg;
  if (c.hidden <= 0 || c.layers <= 0 || c.heads <= 0 || c.hidden % c.heads) return fail(nullptr, DOD_ERR_INVALID, "bad backbone dims hidden=%d heads=%d layers=%d", c.hidden, c.heads, c.layers);
  if (c.hidden % 64) return fail(nullptr, DOD_ERR_INVALID, "hidden (%d) must be a multiple of 64", c.hidden);
  {
    const int fm = c.precision == DOD_PREC_FP32 ? 4 : 64;
    if (c.ffn_hidden <= 0 || c.ffn_hidden % fm) return fail(nullptr, DOD_ERR_INVALID, "ffn_hidden (%d) must be a multiple of %d in this precision", c.ffn_hidden, fm);
  }
  if (c.patch <= 0 || c.pos_grid <= 0) return fail(nullptr, DOD_ERR_INVALID, "bad patch/pos_grid");
  if (c.num_queries <= 0 || c.dec_hidden <= 0 || c.dec_heads <= 0 || c.dec_layers <= 0 || c.num_classes <= 0 || c.dim_feedforward <= 0) return fail(nullptr, DOD_ERR_INVALID, "bad decoder dims");
  if (c.dec_hidden % 64 || c.dim_feedforward % 4) return fail(nullptr, DOD_ERR_INVALID, "decoder hidden (%d) must be a multiple of 64, dim_feedforward (%d) of 4", c.dec_hidden, c.dim_feedforward);
  if (c.target_dim && c.target_dim != c.dec_hidden) return fail(nullptr, DOD_ERR_INVALID, "projection dim %d != decoder hidden %d", c.target_dim, c.dec_hidden);
  if (!c.target_dim && c.hidden != c.dec_hidden) return fail(nullptr, DOD_ERR_INVALID, "backbone width %d != decoder hidden %d and no projection", c.hidden, c.dec_hidden);
  if (c.use_deformable && (c.n_points <= 0 || c.n_points > 8)) return fail(nullptr, DOD_ERR_INVALID, "n_points must be 1..8");
  if (c.dec_layers > 64) return fail(nullptr, DOD_ERR_INVALID, "at most 64 decoder layers");
  if (c.precision != DOD_PREC_FP32 && c.precision != DOD_PREC_BF16 && c.precision != DOD_PREC_FP8 && c.precision != DOD_PREC_BF16X3 && c.precision != DOD_PREC_FP16X2) return fail(nullptr, DOD_ERR_INVALID, "unknown precision %d", c.precision);
  dod_handle* h = new (std::nothrow) dod_handle();
  if (!h) return fail(nullptr, DOD_ERR_STATE, "out of host memory");
  h->cfg = c;
  *out = h;
  return DOD_OK;
}

void dod_destroy(dod_handle* h) {
  if (!h) return;
  for (auto& r : h->prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  for (auto e : h->evpool) (void)hipEventDestroy(e);
  for (void* p : h->owned) (void)hipFree(p);
  delete h;
}

int dod_set_weight(dod_handle* h, const char* key, const void* dev_ptr, const int64_t* shape, int ndim, int dtype) {
  if (!h || !key || !dev_ptr || ndim < 0 || ndim > 8 || (ndim && !shape)) return fail(h, DOD_ERR_INVALID, "dod_set_weight: bad argument");
  if (dtype != DOD_F32 && dtype != DOD_BF16) return fail(h, DOD_ERR_INVALID, "dod_set_weight('%s'): dtype %d is neither DOD_F32 nor DOD_BF16", key, dtype);
  std::string k(key);
  if (k.rfind("module.", 0) == 0) k = k.substr(7);   // DDP prefix, train.py:700-709
  WRef r; r.raw = dev_ptr; r.dtype = dtype; r.ptr = dtype == DOD_F32 ? (const float*)dev_ptr : nullptr; r.shape.assign(shape, shape + ndim);
  h->w[k] = r;
  h->finalized = false;
  return DOD_OK;
}

int dod_reserve_gemm_scratch(size_t bytes) { return (gemm_tail_reserve(bytes) || gemm_f32_ksplit_reserve()) ? fail(nullptr, DOD_ERR_HIP, "scratch allocation of %zu bytes failed", bytes) : DOD_OK; }

int dod_finalize_weights(dod_handle* h, void* stream) {
  if (!h) return fail(nullptr, DOD_ERR_INVALID, "null handle");
  { static const size_t mb = [] { const char* v = getenv("DINODET_GEMM_SCRATCH_MB"); return v && atoi(v) > 0 ? (size_t)atoi(v) : (size_t)64; }();
    (void)gemm_tail_reserve(mb << 20);
    (void)gemm_f32_ksplit_reserve(); }     // K-split scratch of the GEMMs' wave-quantisation tail (gemm_pp.hip): never allocated inside a forward
  int rc = finalize_impl(h, (hipStream_t)stream);
  if (rc || !h->has_dec) return rc;
  // layer 0's image-independent prefix (dod_handle::l0_tgt / l0_proj) through the forward's own code path, one image, scratch freed afterwards
  hipStream_t s = (hipStream_t)stream;
  const dod_config& g = h->cfg;
  const size_t Q = g.num_queries, Dd = g.dec_hidden;
  h->l0_tgt = h->l0_proj = nullptr;
  Carver sz(nullptr);
  const size_t bytes = carve_decoder(h, sz, 1, 1, nullptr, false) + 256;
  void* tmp = nullptr;
  float *t0 = nullptr, *p0 = nullptr;
  HIPCHK(h, hipMalloc(&tmp, bytes));
  if (hipMalloc((void**)&t0, Q * Dd * 4) != hipSuccess || (g.use_deformable && hipMalloc((void**)&p0, Q * (size_t)h->ncat * 4) != hipSuccess)) {
    (void)hipFree(tmp); if (t0) (void)hipFree(t0);
    return fail(h, DOD_ERR_HIP, "allocation of the decoder's layer-0 constants failed");
  }
  h->owned.push_back(t0); if (p0) h->owned.push_back(p0);
  Carver cv((void*)(((uintptr_t)tmp + 255) & ~(uintptr_t)255));
  DecWS dw;
  carve_decoder(h, cv, 1, 1, &dw, false);
  rc = decoder_impl(h, nullptr, 1, 1, dw, nullptr, s, true);
  if (!rc) {
    hipError_t e1 = hipMemcpyAsync(t0, dw.tgt, Q * Dd * 4, hipMemcpyDeviceToDevice, s);
    hipError_t e2 = p0 ? hipMemcpyAsync(p0, dw.proj, Q * (size_t)h->ncat * 4, hipMemcpyDeviceToDevice, s) : hipSuccess;
    hipError_t e3 = hipStreamSynchronize(s);
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) rc = fail(h, DOD_ERR_HIP, "decoder layer-0 constants: %s", hipGetErrorString(e3 != hipSuccess ? e3 : (e1 != hipSuccess ? e1 : e2)));
  } else (void)hipStreamSynchronize(s);
  (void)hipFree(tmp);
  if (rc) return rc;
  h->l0_tgt = t0; h->l0_proj = p0;
  return DOD_OK;
}

int dod_prepare(dod_handle* h, int H, int W, void* stream) {
  if (!h) return fail(nullptr, DOD_ERR_INVALID, "null handle");
  return prepare_impl(h, H, W, (hipStream_t)stream);
}

int dod_num_tokens(const dod_handle* h, int H, int W) { return h ? (H / h->cfg.patch) * (W / h->cfg.patch) + 1 : 0; }

size_t dod_workspace_bytes(const dod_handle* h, int B, int H, int W) {
  if (!h || B <= 0 || H < h->cfg.patch || W < h->cfg.patch) return 0;
  const int N = dod_num_tokens(h, H, W);
  Carver c(nullptr);
  carve_backbone(h, c, B, N, nullptr);
  carve_decoder(h, c, B, N, nullptr, false);
  return c.off + 256;
}

size_t dod_decoder_workspace_bytes(const dod_handle* h, int B, int N) {
  if (!h || B <= 0 || N <= 0) return 0;
  Carver c(nullptr);
  carve_decoder(h, c, B, N, nullptr, true);
  return c.off + 256;
}

int dod_set_tap(dod_handle* h, int stage, float* dst) {
  if (!h) return fail(nullptr, DOD_ERR_INVALID, "null handle");
  if (dst) h->taps[stage] = dst; else h->taps.erase(stage);
  return DOD_OK;
}

int dod_forward(dod_handle* h, const float* pixels, int B, int H, int W, float* det, void* workspace, size_t wsb, void* stream) {
  int rc;
  if (!check_common(h, B, H, W, &rc)) return rc;
  if (!pixels || !det || !workspace) return fail(h, DOD_ERR_INVALID, "null buffer");
  if (wsb < dod_workspace_bytes(h, B, H, W)) return fail(h, DOD_ERR_STATE, "workspace too small: %zu < %zu", wsb, dod_workspace_bytes(h, B, H, W));
  const int N = dod_num_tokens(h, H, W);
  Carver c(align_ws(workspace));
  BbWS bw; DecWS dw;
  carve_backbone(h, c, B, N, &bw);
  carve_decoder(h, c, B, N, &dw, false);
  CARVE_FITS(h, c, workspace, wsb)
  rc = backbone_impl(h, pixels, B, H, W, bw, nullptr, true, (hipStream_t)stream); if (rc) return rc;
  return decoder_impl(h, bw.mem, B, N, dw, det, (hipStream_t)stream);
}

// dod_forward that also hands out the decoder's memory: an entry of its own, so that dod_forward's path has no branch for it.  The copy sits
// where tap 1000 reads, between the two schedules, before the decoder can reuse the workspace.
int dod_forward_mem(dod_handle* h, const float* pixels, int B, int H, int W, float* det, float* memory, void* workspace, size_t wsb, void* stream) {
  int rc;
  if (h && (!pixels || !det || !memory || !workspace)) return fail(h, DOD_ERR_INVALID, "null buffer");      // an argument error whatever the handle's state
  if (!check_common(h, B, H, W, &rc)) return rc;
  if (wsb < dod_workspace_bytes(h, B, H, W)) return fail(h, DOD_ERR_STATE, "workspace too small: %zu < %zu", wsb, dod_workspace_bytes(h, B, H, W));
  const int N = dod_num_tokens(h, H, W);
  Carver c(align_ws(workspace));
  BbWS bw; DecWS dw;
  carve_backbone(h, c, B, N, &bw);
  carve_decoder(h, c, B, N, &dw, false);
  CARVE_FITS(h, c, workspace, wsb)
  hipStream_t s = (hipStream_t)stream;
  rc = backbone_impl(h, pixels, B, H, W, bw, nullptr, true, s); if (rc) return rc;
  const size_t n = (size_t)B * N * h->cfg.dec_hidden;
  if (is_bf16(h)) KCHK(h, launch_widen_bf16((const bf16_t*)bw.mem, memory, n, s));
  else HIPCHK(h, hipMemcpyAsync(memory, bw.mem, n * 4, hipMemcpyDeviceToDevice, s));
  return decoder_impl(h, bw.mem, B, N, dw, det, s);
}

int dod_forward_u8(dod_handle* h, const uint8_t* pixels_hwc, int B, int H, int W, float* det, void* workspace, size_t wsb, void* stream) {
  int rc;
  if (!check_common(h, B, H, W, &rc)) return rc;
  if (!pixels_hwc || !det || !workspace) return fail(h, DOD_ERR_INVALID, "null buffer");
  if (wsb < dod_workspace_bytes(h, B, H, W)) return fail(h, DOD_ERR_STATE, "workspace too small: %zu < %zu", wsb, dod_workspace_bytes(h, B, H, W));
  const int N = dod_num_tokens(h, H, W);
  Carver c(align_ws(workspace));
  BbWS bw; DecWS dw;
  carve_backbone(h, c, B, N, &bw);
  carve_decoder(h, c, B, N, &dw, false);
  CARVE_FITS(h, c, workspace, wsb)
  rc = backbone_impl(h, nullptr, B, H, W, bw, nullptr, true, (hipStream_t)stream, -1, nullptr, pixels_hwc); if (rc) return rc;
  return decoder_impl(h, bw.mem, B, N, dw, det, (hipStream_t)stream);
}

int dod_backbone_forward(dod_handle* h, const float* pixels, int B, int H, int W, float* features, void* workspace, size_t wsb, void* stream) {
  int rc;
  if (!check_common(h, B, H, W, &rc)) return rc;
  if (!pixels || !features || !workspace) return fail(h, DOD_ERR_INVALID, "null buffer");
  if (wsb < dod_workspace_bytes(h, B, H, W)) return fail(h, DOD_ERR_STATE, "workspace too small: %zu < %zu", wsb, dod_workspace_bytes(h, B, H, W));
  const int N = dod_num_tokens(h, H, W);
  Carver c(align_ws(workspace));
  BbWS bw;
  carve_backbone(h, c, B, N, &bw);
  CARVE_FITS(h, c, workspace, wsb)
  return backbone_impl(h, pixels, B, H, W, bw, features, false, (hipStream_t)stream);
}

int dod_backbone_prefix(dod_handle* h, const float* pixels, int B, int H, int W, int nblocks, float* x_out, void* workspace, size_t wsb, void* stream) {
  int rc;
  if (!check_common(h, B, H, W, &rc)) return rc;
  if (!pixels || !x_out || !workspace) return fail(h, DOD_ERR_INVALID, "null buffer");
  if (nblocks < 0 || nblocks > h->cfg.layers) return fail(h, DOD_ERR_INVALID, "nblocks %d outside 0..%d", nblocks, h->cfg.layers);
  if (wsb < dod_workspace_bytes(h, B, H, W)) return fail(h, DOD_ERR_STATE, "workspace too small: %zu < %zu", wsb, dod_workspace_bytes(h, B, H, W));
  const int N = dod_num_tokens(h, H, W);
  Carver c(align_ws(workspace));
  BbWS bw;
  carve_backbone(h, c, B, N, &bw);
  CARVE_FITS(h, c, workspace, wsb)
  return backbone_impl(h, pixels, B, H, W, bw, nullptr, false, (hipStream_t)stream, nblocks, x_out);
}

int dod_decoder_forward(dod_handle* h, const float* memory, int B, int N, float* det, void* workspace, size_t wsb, void* stream) {
  if (!h) return fail(nullptr, DOD_ERR_INVALID, "null handle");
  if (!h->finalized) return fail(h, DOD_ERR_STATE, "dod_finalize_weights has not been called");
  if (B <= 0 || N <= 0) return fail(h, DOD_ERR_INVALID, "bad B=%d N=%d", B, N);
  if (!memory || !det || !workspace) return fail(h, DOD_ERR_INVALID, "null buffer");
  if (wsb < dod_decoder_workspace_bytes(h, B, N)) return fail(h, DOD_ERR_STATE, "workspace too small");
  Carver c(align_ws(workspace));
  DecWS dw;
  carve_decoder(h, c, B, N, &dw, true);
  CARVE_FITS(h, c, workspace, wsb)
  hipStream_t s = (hipStream_t)stream;
  const void* mem_op = memory;
  if (is_bf16(h)) {
    KCHK(h, launch_cast_bf16(memory, (bf16_t*)dw.mem_op, (size_t)B * N * h->cfg.dec_hidden, s));
    mem_op = dw.mem_op;
  }
  return decoder_impl(h, mem_op, B, N, dw, det, s);
}

int dod_profile(dod_handle* h, int enable) {
  if (!h) return fail(nullptr, DOD_ERR_INVALID, "null handle");
  for (auto& r : h->prof) { h->evpool.push_back(r.a); h->evpool.push_back(r.b); }
  h->prof.clear();
  h->prof_on = enable != 0;
  return DOD_OK;
}

int dod_profile_read(dod_handle* h, int cls, double* ms, double* flops, int* launches) {
  if (!h || cls < 0 || cls >= PC_COUNT) return fail(h, DOD_ERR_INVALID, "bad profile class");
  double t = 0, f = 0; int n = 0;
  for (auto& r : h->prof) {
    if (r.cls != cls) continue;
    HIPCHK(h, hipEventSynchronize(r.b));
    float e = 0.f;
    HIPCHK(h, hipEventElapsedTime(&e, r.a, r.b));
    t += e; f += r.flops; ++n;
  }
  if (ms) *ms = t; if (flops) *flops = f; if (launches) *launches = n;
  return DOD_OK;
}

// ---- stateless ops
int dod_op_linear(int in_dtype, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const float* bias,
                  const float* scale, const float* resid, int ldr, void* out, int out_dtype, int ldc, int act, void* stream) {
  if (!A || !W || !out) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  GemmEpi e = epi(bias, out_dtype == DOD_F32 ? (float*)out : nullptr, out_dtype == DOD_BF16 ? out : nullptr, ldc, act, scale, resid, ldr);
  if (act == DOD_ACT_SWIGLU_PAIRS) {      // interleaved (x1_i, x2_i) columns -> silu(x1_i) * x2_i at column i (bf16 operands and output only)
    if (in_dtype != DOD_BF16 || out_dtype != DOD_BF16 || scale || resid || (N & 7)) return fail(nullptr, DOD_ERR_INVALID, "DOD_ACT_SWIGLU_PAIRS: bf16 in / out, N %% 8 == 0, no scale / residual");
    e.act = ACT_NONE; e.glu = 1;
  }
  int r = in_dtype == DOD_BF16 ? launch_gemm_bf16((const bf16_t*)A, lda, (const bf16_t*)W, ldw, M, N, K, e, (hipStream_t)stream)
                               : launch_gemm_f32((const float*)A, lda, (const float*)W, ldw, M, N, K, e, (hipStream_t)stream);
  return rejected(nullptr, r, "dod_op_linear M=%d N=%d K=%d", M, N, K);
}
int dod_op_gemm_f32x(const float* A, int lda, int a_kmajor, long long a_sb, long long a_sh, const float* W, int ldw, int w_kmajor, long long w_sb,
                     long long w_sh, float* C, int ldc, long long c_sb, long long c_sh, int M, int N, int K, int batch, int hb, float alpha,
                     int accumulate, int ksplit, void* stream) {
  if (!A || !W || !C) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  GemmF32X g; memset(&g, 0, sizeof g);
  g.A = A; g.lda = lda; g.a_kmajor = a_kmajor; g.a_sb = a_sb; g.a_sh = a_sh;
  g.W = W; g.ldw = ldw; g.w_kmajor = w_kmajor; g.w_sb = w_sb; g.w_sh = w_sh;
  g.C = C; g.ldc = ldc; g.c_sb = c_sb; g.c_sh = c_sh;
  g.M = M; g.N = N; g.K = K; g.batch = batch; g.hb = hb; g.alpha = alpha; g.accumulate = accumulate; g.ksplit = ksplit;
  return rejected(nullptr, launch_gemm_f32x(g, (hipStream_t)stream), "dod_op_gemm_f32x M=%d N=%d K=%d batch=%d", M, N, K, batch);
}
int dod_op_gemm_f32x3(const float* A, int lda, int a_kmajor, long long a_sb, long long a_sh, const float* W, int ldw, int w_kmajor, long long w_sb,
                      long long w_sh, float* C, int ldc, long long c_sb, long long c_sh, int M, int N, int K, int batch, int hb, float alpha,
                      int accumulate, int ksplit, void* stream) {
  if (!A || !W || !C) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  GemmF32X g; memset(&g, 0, sizeof g);
  g.A = A; g.lda = lda; g.a_kmajor = a_kmajor; g.a_sb = a_sb; g.a_sh = a_sh;
  g.W = W; g.ldw = ldw; g.w_kmajor = w_kmajor; g.w_sb = w_sb; g.w_sh = w_sh;
  g.C = C; g.ldc = ldc; g.c_sb = c_sb; g.c_sh = c_sh;
  g.M = M; g.N = N; g.K = K; g.batch = batch; g.hb = hb; g.alpha = alpha; g.accumulate = accumulate; g.ksplit = ksplit;
  return rejected(nullptr, launch_gemm_f32x3(g, (hipStream_t)stream), "dod_op_gemm_f32x3 M=%d N=%d K=%d batch=%d", M, N, K, batch);
}
int dod_op_linear_f32x3(const float* X, int ldx, const float* W, const float* bias, const float* scale, const float* resid, int ldr, int M, int N, int K,
                        float* Y, int ldy, int act, void* stream) {
  if (!X || !W || !Y) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  if (act < DOD_ACT_NONE || act > DOD_ACT_SIGMOID) return fail(nullptr, DOD_ERR_INVALID, "dod_op_linear_f32x3: activation %d", act);
  GemmF32X g; memset(&g, 0, sizeof g);
  g.A = X; g.lda = ldx; g.W = W; g.ldw = K; g.C = Y; g.ldc = ldy; g.M = M; g.N = N; g.K = K; g.batch = 1; g.hb = 1; g.alpha = 1.0f; g.ksplit = 1;
  g.bias = bias; g.scale = scale; g.resid = resid; g.ldr = ldr; g.act = act;
  return rejected(nullptr, launch_gemm_f32x3(g, (hipStream_t)stream), "dod_op_linear_f32x3 M=%d N=%d K=%d", M, N, K);
}
int dod_op_linear_fp8(const void* A, int lda, const float* a_scale, const void* W, int ldw, const float* w_scale, int M, int N, int K,
                      const float* bias, const float* scale, const float* resid, int ldr, void* out, int out_dtype, int ldc, int act,
                      void* stream) {
  if (!A || !W || !out || !a_scale || !w_scale) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  GemmEpi e = epi(bias, out_dtype == DOD_F32 ? (float*)out : nullptr, out_dtype == DOD_BF16 ? out : nullptr, ldc, act, scale, resid, ldr);
  e.a_scale = a_scale; e.w_scale = w_scale;
  return rejected(nullptr, launch_gemm_fp8((const unsigned char*)A, lda, (const unsigned char*)W, ldw, M, N, K, e, (hipStream_t)stream), "dod_op_linear_fp8 M=%d N=%d K=%d", M, N, K);
}
int dod_op_linear_fp8_mx(const void* A, int lda, const void* a_block_scales, const void* W, int ldw, const float* w_scale, int M, int N, int K,
                         const float* bias, const float* scale, const float* resid, int ldr, void* out, int out_dtype, int ldc, int act,
                         void* stream) {
  if (!A || !W || !out || !a_block_scales || !w_scale) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  GemmEpi e = epi(bias, out_dtype == DOD_F32 ? (float*)out : nullptr, out_dtype == DOD_BF16 ? out : nullptr, ldc, act, scale, resid, ldr);
  e.a_bs = (const unsigned char*)a_block_scales; e.w_scale = w_scale;
  return rejected(nullptr, launch_gemm_fp8((const unsigned char*)A, lda, (const unsigned char*)W, ldw, M, N, K, e, (hipStream_t)stream), "dod_op_linear_fp8_mx M=%d N=%d K=%d", M, N, K);
}
int dod_op_linear_fp8_glu_mx(const void* A, int lda, const float* a_scale, const void* W, int ldw, const float* w_scale, int M, int N, int K,
                             const float* bias, void* out_q, int ldq, void* out_block_scales, void* stream) {
  if (!A || !W || !a_scale || !w_scale || !out_q || !out_block_scales) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  GemmEpi e = epi(bias, nullptr, out_q, ldq);
  e.a_scale = a_scale; e.w_scale = w_scale; e.glu = 1; e.out_bs = (unsigned char*)out_block_scales;
  return rejected(nullptr, launch_gemm_fp8((const unsigned char*)A, lda, (const unsigned char*)W, ldw, M, N, K, e, (hipStream_t)stream), "dod_op_linear_fp8_glu_mx M=%d N=%d K=%d", M, N, K);
}
// both operands block-scaled (round 4: the fp8 mode's linears); glu_out_block_scales: the weights_in form -- interleaved (x1, x2) columns, the
// epilogue gates and quantises (out = e4m3 rows of N / 2 columns at pitch ldc BYTES, their e8m0 bytes to glu_out_block_scales)
int dod_op_linear_fp8_mx2(const void* A, int lda, const void* a_block_scales, const void* W, int ldw, const void* w_block_scales, int M, int N, int K,
                          const float* bias, const float* scale, const float* resid, int ldr, void* out, int out_dtype, int ldc, int act,
                          void* glu_out_block_scales, void* stream) {
  if (!A || !W || !out || !a_block_scales || !w_block_scales) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  GemmEpi e = epi(bias, out_dtype == DOD_F32 ? (float*)out : nullptr, out_dtype == DOD_BF16 ? out : nullptr, ldc, act, scale, resid, ldr);
  e.a_bs = (const unsigned char*)a_block_scales; e.w_bs = (const unsigned char*)w_block_scales;
  if (glu_out_block_scales) { e.out_f32 = nullptr; e.out_bf16 = (bf16_t*)out; e.glu = 1; e.out_bs = (unsigned char*)glu_out_block_scales; }
  return rejected(nullptr, launch_gemm_fp8((const unsigned char*)A, lda, (const unsigned char*)W, ldw, M, N, K, e, (hipStream_t)stream), "dod_op_linear_fp8_mx2 M=%d N=%d K=%d", M, N, K);
}
int dod_op_quant_mx_fp8(const void* x, int in_dtype, int ld, int rows, int cols, void* q, int ldq, void* block_scales, void* stream) {
  if (!x || !q || !block_scales) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  return rejected(nullptr, launch_quant_mx_fp8(x, in_dtype == DOD_BF16, ld, rows, cols, (unsigned char*)q, ldq, (unsigned char*)block_scales, (hipStream_t)stream), "dod_op_quant_mx_fp8 rows=%d cols=%d", rows, cols);
}
int dod_op_split_pair(const float* x, int ld, int rows, int cols, void* out, void* stream) {
  if (!x || !out) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  return launch_split2(x, ld, (bf16_t*)out, rows, cols, (hipStream_t)stream) ? fail(nullptr, DOD_ERR_HIP, "launch failed") : DOD_OK;
}
int dod_op_linear_x3(const void* A2, const void* W2, int M, int N, int K, const float* bias, const float* scale, const float* resid, int ldr,
                     void* out, int out_layout, int ldc, int act, void* stream) {
  if (!A2 || !W2 || !out) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  GemmEpi e = epi(bias, out_layout == 0 ? (float*)out : nullptr, out_layout != 0 ? out : nullptr, ldc, act, scale, resid, ldr);
  if (out_layout == 2) e.out_split = -N;       // pair layout [hi | lo]
  return rejected(nullptr, launch_gemm_x3((const bf16_t*)A2, 2 * K, (const bf16_t*)W2, 2 * K, M, N, K, e, (hipStream_t)stream), "dod_op_linear_x3 M=%d N=%d K=%d", M, N, K);
}
int dod_op_split_h2(const float* x, int ld, int rows, int cols, void* out, void* wexp, void* stream) {
  if (!x || !out) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  return rejected(nullptr, launch_split_h2(x, ld, out, rows, cols, (unsigned char*)wexp, (hipStream_t)stream), "dod_op_split_h2 rows=%d cols=%d", rows, cols);
}
int dod_op_linear_h2(const void* A, const void* W, const void* wexp, int M, int N, int K, const float* bias, const float* scale, const float* resid,
                     int ldr, void* out, int out_layout, int ldc, int act, void* stream) {
  if (!A || !W || !wexp || !out) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  GemmEpi e = epi(bias, out_layout == 0 ? (float*)out : nullptr, out_layout != 0 ? out : nullptr, ldc, act, scale, resid, ldr);
  if (out_layout == 2) e.out_split = -N;       // bf16 pair layout [hi | lo]
  if (out_layout == 3) e.out_h2 = 1;           // H2 operand rows
  e.h2_wexp = (const unsigned char*)wexp;
  return rejected(nullptr, launch_gemm_h2(A, 4 * K, W, 3 * K, M, N, K, e, (hipStream_t)stream), "dod_op_linear_h2 M=%d N=%d K=%d", M, N, K);
}
// Block linears with the LayerNorm folded into them (GemmEpi::ln_*): family = DOD_PREC_BF16 / DOD_PREC_BF16X3 / DOD_PREC_FP16X2 picks the operand
// format (and the kernel family) exactly as the forward does
int dod_op_linear_ln(int family, const void* A, const void* W, const void* wexp, int M, int N, int K, const float* bias, const float* scale,
                     const float* resid, int ldr, void* out, int out_layout, int ldc, int act, const dod_ln_fold* ln, void* stream) {
  if (!A || !W || !out || !ln) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  if (family != DOD_PREC_BF16 && family != DOD_PREC_BF16X3 && family != DOD_PREC_FP16X2) return fail(nullptr, DOD_ERR_INVALID, "family must be a bf16 / bf16x3 / fp16x2 precision");
  if ((ln->stats == nullptr) != (ln->csum == nullptr)) return fail(nullptr, DOD_ERR_INVALID, "stats and csum go together");
  if (ln->stats && scale) return fail(nullptr, DOD_ERR_INVALID, "the folded consumer has no LayerScale");
  if (ln->part && !(resid && out_layout == 0)) return fail(nullptr, DOD_ERR_INVALID, "the folded producer is the fp32 residual epilogue");
  GemmEpi e = epi(bias, out_layout == 0 ? (float*)out : nullptr, out_layout != 0 ? out : nullptr, ldc, act, scale, resid, ldr);
  if (out_layout == 2) e.out_split = -N;
  if (out_layout == 3) e.out_h2 = 1;
  e.ln_stats = (const float2*)ln->stats; e.ln_c = ln->csum;
  if (ln->part_in) {
    if (!ln->stats || ln->stats_out == ln->stats) return fail(nullptr, DOD_ERR_INVALID, "part_in needs stats (the shift) and a DIFFERENT stats_out buffer");
    e.ln_part_in = (const float2*)ln->part_in; e.ln_npart = (K + 127) / 128; e.ln_stats_out = (float2*)ln->stats_out; e.ln_eps = ln->eps;
  }
  if (ln->part) {
    e.ln_part = (float2*)ln->part; e.ln_npart = (N + 127) / 128; e.ln_op = ln->op_out; e.ln_shift = (const float2*)ln->shift;
    e.ln_op_kind = family == DOD_PREC_FP16X2 ? LNOP_H2 : (family == DOD_PREC_BF16X3 ? LNOP_PAIR : LNOP_BF16);
    e.ln_op_ld = family == DOD_PREC_BF16 ? N : 2 * N;
  }
  int r;
  if (family == DOD_PREC_FP16X2) {
    if (!wexp) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
    e.h2_wexp = (const unsigned char*)wexp;
    r = launch_gemm_h2(A, 4 * K, W, 3 * K, M, N, K, e, (hipStream_t)stream);
  } else if (family == DOD_PREC_BF16X3) r = launch_gemm_x3((const bf16_t*)A, 2 * K, (const bf16_t*)W, 2 * K, M, N, K, e, (hipStream_t)stream);
  else r = launch_gemm_bf16((const bf16_t*)A, K, (const bf16_t*)W, K, M, N, K, e, (hipStream_t)stream);
  return rejected(nullptr, r, "dod_op_linear_ln M=%d N=%d K=%d", M, N, K);
}
int dod_op_rowstats(const float* x, int rows, int D, float eps, void* op_out, int family, void* stats, void* stream) {
  if (!x || !op_out || !stats) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  const int kind = family == DOD_PREC_FP16X2 ? LNOP_H2 : (family == DOD_PREC_BF16X3 ? LNOP_PAIR : (family == DOD_PREC_BF16 ? LNOP_BF16 : 0));
  return rejected(nullptr, launch_rowstats(x, rows, D, eps, op_out, kind, (float2*)stats, (hipStream_t)stream), "dod_op_rowstats rows=%d D=%d", rows, D);
}
int dod_op_ln_finalize(const void* part, int rows, int D, float eps, void* stats, void* stream) {
  if (!part || !stats) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  return rejected(nullptr, launch_ln_finalize((const float2*)part, (D + 127) / 128, rows, D, eps, (float2*)stats, (hipStream_t)stream), "dod_op_ln_finalize rows=%d D=%d", rows, D);
}
int dod_op_attention_x3(const void* qkv2, void* ctx2, int B, int N, int heads, float scale, void* stream) {
  if (!qkv2 || !ctx2) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  return rejected(nullptr, launch_attn_x3((const bf16_t*)qkv2, (bf16_t*)ctx2, B, N, heads, scale, (hipStream_t)stream), "dod_op_attention_x3");
}
// both flash kernels index their grid (8-padded (image, head) pairs x query blocks of at least 128 rows, plus one tail block per pair) with an int
static bool attn_grid_fits(int B, int N, int heads) {
  return (((long long)B * heads + 7) / 8 * 8) * (((long long)N + 127) / 128 + 1) <= 0x7fffffffLL;
}
// the H2 epilogue of the same kernel (ctx_h2 = 1): what the fp16x2 forward launches
int dod_op_attention_x3_h2(const void* qkv2, void* ctx_h2, int B, int N, int heads, float scale, void* stream) {
  if (!qkv2 || !ctx_h2) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  if (B <= 0 || N <= 0 || heads <= 0) return fail(nullptr, DOD_ERR_INVALID, "dod_op_attention_x3_h2: B=%d N=%d heads=%d must be positive", B, N, heads);
  if (!attn_grid_fits(B, N, heads)) return fail(nullptr, DOD_ERR_INVALID, "dod_op_attention_x3_h2: B=%d N=%d heads=%d is more workgroups than one launch holds", B, N, heads);
  return rejected(nullptr, launch_attn_x3((const bf16_t*)qkv2, (bf16_t*)ctx_h2, B, N, heads, scale, (hipStream_t)stream, 1), "dod_op_attention_x3_h2");
}
int dod_op_quant_rows_fp8(const void* x, int in_dtype, int ld, int rows, int cols, void* q, int ldq, float* scale, void* stream) {
  if (!x || !q || !scale) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  return rejected(nullptr, launch_quant_rows_fp8(x, in_dtype == DOD_BF16, ld, rows, cols, (unsigned char*)q, ldq, scale, (hipStream_t)stream), "dod_op_quant_rows_fp8 rows=%d cols=%d", rows, cols);
}
int dod_op_layernorm(const float* x, const float* add, const float* gamma, const float* beta, float eps, int rows, int D, void* out, int out_dtype, void* stream) {
  if (!x || !gamma || !beta || !out) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  return rejected(nullptr, launch_layernorm(x, add, gamma, beta, eps, rows, D, ln_out(out_dtype == DOD_F32 ? (float*)out : nullptr, out_dtype == DOD_BF16 ? (bf16_t*)out : nullptr), (hipStream_t)stream), "dod_op_layernorm rows=%d D=%d", rows, D);
}
// every output form of launch_layernorm, as the forward schedules fill LnOut
int dod_op_layernorm_form(const float* x, const float* add, const float* gamma, const float* beta, float eps, int rows, int D, int form, void* out, void* out2,
                          void* stream) {
  if (!x || !gamma || !beta || !out) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  if (form < DOD_LN_F32 || form > DOD_LN_F32_S3) return fail(nullptr, DOD_ERR_INVALID, "dod_op_layernorm_form: unknown form %d", form);
  const bool two = form == DOD_LN_F32_BF16 || form == DOD_LN_FP8 || form == DOD_LN_FP8_MX || form == DOD_LN_F32_S3;
  if (two && !out2) return fail(nullptr, DOD_ERR_INVALID, "null buffer (form %d writes out2)", form);
  if (!two && out2) return fail(nullptr, DOD_ERR_INVALID, "dod_op_layernorm_form: form %d has no second output, out2 must be NULL", form);
  if (rows <= 0 || D <= 0) return fail(nullptr, DOD_ERR_INVALID, "dod_op_layernorm_form: rows=%d D=%d must be positive", rows, D);
  if (D % 4 != 0 || D > 2048) return fail(nullptr, DOD_ERR_INVALID, "dod_op_layernorm_form: D=%d must be a multiple of 4 and at most 2048", D);
  if (form == DOD_LN_H2 && D % 32 != 0) return fail(nullptr, DOD_ERR_INVALID, "dod_op_layernorm_form: H2 rows need D %% 32 == 0 (D=%d)", D);
  if (form == DOD_LN_FP8_MX && D % 64 != 0) return fail(nullptr, DOD_ERR_INVALID, "dod_op_layernorm_form: block-scaled rows need D %% 64 == 0 (D=%d)", D);
  LnOut o;
  switch (form) {
    case DOD_LN_F32: o.f32 = (float*)out; break;
    case DOD_LN_BF16: o.bf16 = (bf16_t*)out; break;
    case DOD_LN_F32_BF16: o.f32 = (float*)out; o.bf16 = (bf16_t*)out2; break;
    case DOD_LN_PAIR: case DOD_LN_H2: o.split = (bf16_t*)out; break;
    case DOD_LN_FP8: o.fp8 = (unsigned char*)out; o.scale = (float*)out2; break;
    case DOD_LN_FP8_MX: o.fp8 = (unsigned char*)out; o.bs = (unsigned char*)out2; break;
    default: o.f32 = (float*)out; o.a3 = (bf16_t*)out2; break;
  }
  return rejected(nullptr, launch_layernorm(x, add, gamma, beta, eps, rows, D, o, (hipStream_t)stream, form == DOD_LN_H2 ? 1 : 0), "dod_op_layernorm_form rows=%d D=%d form=%d", rows, D, form);
}
int dod_op_swiglu(const void* x, void* out, int dtype, int rows, int Fh, void* stream) {
  if (!x || !out) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  if (dtype != DOD_F32 && dtype != DOD_BF16) return fail(nullptr, DOD_ERR_INVALID, "dod_op_swiglu: dtype must be DOD_F32 or DOD_BF16");
  if (rows <= 0 || Fh <= 0) return fail(nullptr, DOD_ERR_INVALID, "dod_op_swiglu: rows=%d Fh=%d must be positive", rows, Fh);
  const bool bf = dtype == DOD_BF16;
  return rejected(nullptr, launch_swiglu(bf ? nullptr : (const float*)x, bf ? (const bf16_t*)x : nullptr, rows, Fh, bf ? nullptr : (float*)out, bf ? (bf16_t*)out : nullptr, (hipStream_t)stream),
                  "dod_op_swiglu rows=%d Fh=%d", rows, Fh);
}
int dod_op_split3(const float* x, int ld, int rows, int cols, int weight_order, void* out, void* stream) {
  if (!x || !out) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  if (rows <= 0 || cols <= 0) return fail(nullptr, DOD_ERR_INVALID, "dod_op_split3: rows=%d cols=%d must be positive", rows, cols);
  if (ld < cols) return fail(nullptr, DOD_ERR_INVALID, "dod_op_split3: pitch %d is less than cols=%d", ld, cols);
  if (weight_order != 0 && weight_order != 1) return fail(nullptr, DOD_ERR_INVALID, "dod_op_split3: weight_order must be 0 or 1");
  return rejected(nullptr, launch_split3(x, ld, (bf16_t*)out, rows, cols, weight_order, (hipStream_t)stream), "dod_op_split3 rows=%d cols=%d", rows, cols);
}
int dod_op_attention_bf16(const void* qkv, void* ctx, int B, int N, int heads, float scale, void* stream) {
  if (!qkv || !ctx) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  return rejected(nullptr, launch_attn_bf16((const bf16_t*)qkv, (bf16_t*)ctx, B, N, heads, scale, (hipStream_t)stream), "dod_op_attention_bf16");
}
// the block-scaled e4m3 epilogue of the same kernel (ctx_bs set): what the fp8 forward launches
int dod_op_attention_bf16_mx(const void* qkv, void* ctx_q8, void* ctx_bs, int B, int N, int heads, float scale, void* stream) {
  if (!qkv || !ctx_q8 || !ctx_bs) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  if (B <= 0 || N <= 0 || heads <= 0) return fail(nullptr, DOD_ERR_INVALID, "dod_op_attention_bf16_mx: B=%d N=%d heads=%d must be positive", B, N, heads);
  if (!attn_grid_fits(B, N, heads)) return fail(nullptr, DOD_ERR_INVALID, "dod_op_attention_bf16_mx: B=%d N=%d heads=%d is more workgroups than one launch holds", B, N, heads);
  return rejected(nullptr, launch_attn_bf16((const bf16_t*)qkv, (bf16_t*)ctx_q8, B, N, heads, scale, (hipStream_t)stream, (unsigned char*)ctx_bs), "dod_op_attention_bf16_mx");
}
int dod_op_attention_f32(const float* q, const float* k, const float* v, float* o, int ldq, int ldk, int ldv, int ldo, int Lq, int Lk,
                         int B, int heads, int dh, float scale, void* stream) {
  if (!q || !k || !v || !o) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  AttnF32 a; a.q = q; a.k = k; a.v = v; a.o = o; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.Lq = Lq; a.Lk = Lk; a.B = B; a.heads = heads; a.dh = dh; a.scale = scale;
  return rejected(nullptr, launch_attn_f32(a, (hipStream_t)stream), "dod_op_attention_f32 (dh=%d)", dh);
}
int dod_op_deform_sample(const float* proj, int ldp, const float* values, int B, int Q, int N, int Hd, int P, int dh, int hh, int ww, float* out, void* stream) {
  if (!proj || !values || !out) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  if (hh * ww != N) return fail(nullptr, DOD_ERR_INVALID, "Cannot reshape input of size %d into a %dx%d feature map", N, hh, ww);
  return rejected(nullptr, launch_deform_sample(proj, ldp, values, B, Q, N, Hd, P, dh, hh, ww, out, (hipStream_t)stream), "dod_op_deform_sample");
}
// the decoder's own launch: projections shared by all images (layer 0) and / or the fused [hi | hi | lo] operand copy
int dod_op_deform_sample_ex(const float* proj, int ldp, int proj_shared, const float* values, int B, int Q, int N, int Hd, int P, int dh, int hh, int ww, float* out,
                            void* out3, void* stream) {
  if (!proj || !values || !out) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  if (B <= 0 || Q <= 0 || N <= 0 || Hd <= 0 || hh <= 0 || ww <= 0) return fail(nullptr, DOD_ERR_INVALID, "dod_op_deform_sample_ex: B=%d Q=%d N=%d Hd=%d h=%d w=%d must be positive", B, Q, N, Hd, hh, ww);
  if (P < 1 || P > 8) return fail(nullptr, DOD_ERR_INVALID, "dod_op_deform_sample_ex: 1..8 sampling points (got %d)", P);
  if (dh < 1 || dh > 128) return fail(nullptr, DOD_ERR_INVALID, "dod_op_deform_sample_ex: head_dim 1..128 (got %d)", dh);
  if ((long long)hh * ww != N) return fail(nullptr, DOD_ERR_INVALID, "Cannot reshape input of size %d into a %dx%d feature map", N, hh, ww);
  if (ldp < 2 + 3LL * Hd * P) return fail(nullptr, DOD_ERR_INVALID, "dod_op_deform_sample_ex: pitch %d is less than 2 + 3*Hd*P = %lld", ldp, 2 + 3LL * Hd * P);
  if ((long long)B * Q * Hd > 0x7fffffffLL) return fail(nullptr, DOD_ERR_INVALID, "dod_op_deform_sample_ex: B*Q*Hd is more items than one launch holds");
  return rejected(nullptr, launch_deform_sample(proj, ldp, values, B, Q, N, Hd, P, dh, hh, ww, out, (hipStream_t)stream, proj_shared ? 1 : 0, (bf16_t*)out3), "dod_op_deform_sample_ex");
}
int dod_op_pos_resize(const float* pos_in, int G, int gh, int gw, int D, float* pos_out, void* stream) {
  if (!pos_in || !pos_out) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  return launch_pos_resize(pos_in, G, gh, gw, D, pos_out, (hipStream_t)stream) ? fail(nullptr, DOD_ERR_HIP, "launch failed") : DOD_OK;
}
int dod_op_im2col(const float* img, int B, int H, int W, int patch, int Kp, void* out, int out_dtype, void* stream) {
  if (!img || !out) return fail(nullptr, DOD_ERR_INVALID, "null buffer");
  int r = launch_im2col(img, B, H, W, patch, Kp, out_dtype == DOD_F32 ? (float*)out : nullptr, out_dtype == DOD_BF16 ? (bf16_t*)out : nullptr, (hipStream_t)stream);
  return r ? fail(nullptr, DOD_ERR_INVALID, "dod_op_im2col rejected") : DOD_OK;
}

}  // extern "C"
