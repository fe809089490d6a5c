// Host-side internals of the native training step, shared by train_ops.hip (the training kernels, their launchers, the fp32 linear
// helpers and the dod_op_* operator entry points), dec_train.hip (the two decoder schedules) and tail_train.hip (the backbone-tail
// schedule): error helpers, entry checks, the tape / scratch carver and the declaration of every launcher a schedule calls.
// Launchers return 0, 2 (shape not taken) or 3 (the HIP runtime refused) unless stated otherwise; TK turns that into a dod_status.
#pragma once
#include "dod_internal.h"

#include <cstdlib>

namespace dtrain {

inline size_t up4(size_t x) { return (x + 3) & ~(size_t)3; }
inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// ------------------------------------------------------------------------------------------------ errors (dod_common.h dod_fail)
#define TK(x) do { int r_ = (x); if (r_) return dod_fail(r_ == 3 ? DOD_ERR_HIP : DOD_ERR_INVALID, "decoder train: %s failed (%d)", #x, r_); } while (0)
#define TH(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return dod_fail(DOD_ERR_HIP, "decoder train: %s: %s", #x, hipGetErrorString(e_)); } while (0)
#define OPFAIL(...) return dod_fail(DOD_ERR_INVALID, __VA_ARGS__)

// ------------------------------------------------------------------------------------------------ entry checks, tape / scratch carve
// What every step's entry point checks once its configuration is taken: `buffers` = none of its pointers is null; the backward passes
// dropout_p = 0 (the forward has checked the rate both calls are given); *_need = what the step's carve from the caller's pointer
// reports + 256 (a null pointer carves as the sizing pass does, and fails the first check).  Returns a dod_status.
inline int entry_check(const char* step, bool buffers, float dropout_p, size_t tape_bytes, size_t tape_need, size_t ws_bytes, size_t ws_need) {
  if (!buffers) return dod_fail(DOD_ERR_INVALID, "%s: null buffer / mismatched parameters", step);
  if (dropout_p < 0.f || dropout_p >= 1.f) return dod_fail(DOD_ERR_INVALID, "%s: dropout %g outside [0, 1)", step, dropout_p);
  if (tape_bytes < tape_need || ws_bytes < ws_need) return dod_fail(DOD_ERR_STATE, "%s: tape / workspace too small", step);
  return DOD_OK;
}
// The tape and scratch layouts are carved by dod::Carver (256-byte slots; a null base is the sizing pass and yields null pointers) from
// the caller's pointer rounded up to 256 bytes -- the *_bytes queries add that slack.
inline dod::Carver carver(const void* base) { return dod::Carver(base ? dod::align_ws(const_cast<void*>(base)) : nullptr); }
inline float* takef(dod::Carver& c, size_t floats) { return (float*)c.take(floats * 4); }

// ------------------------------------------------------------------------------------------------ dropout keys, modes
inline unsigned long long site_key(unsigned long long seed, int layer, int site) {
  return seed * 0xD1342543DE82EF95ull + (unsigned long long)(layer * 8 + site + 1) * 0x9E3779B97F4A7C15ull;
}
bool det_mode();      // DINODET_DETERMINISTIC=1 / test option "deterministic": ordered reductions (train_ops.hip)

// ------------------------------------------------------------------------------------------------ batched-GEMM attention scratch
#define MHA_MAXQ 1408      // decoder queries, and the 1370 tokens of a 518x518 image in the backbone-tail backward
// Images per pass: the score / adjoint scratch ([images*Hd, Q, Qp] fp32, two of them in the backward) is capped at 1 GB per buffer
// (DINODET_MHA_CHUNK_MB) instead of growing with the batch (1 370 tokens x 12 heads: 90 MB per image per buffer).  Passes small
// enough to keep the scores in the 256 MB Infinity Cache between launches were measured and do not pay: ViT-B 518x518, batch 8,
// one image per pass 23.0 ms per step, two 22.0, the whole batch in one pass 21.7.
inline int mha_chunk_images(int B, int Hd, int Lq, int Lk) {
  const int forced = dod_option(DOD_OPT_MHA_CHUNK_IMAGES);      // tests: force several (ragged) passes on small shapes
  if (forced > 0) return forced > B ? B : forced;
  const char* e = getenv("DINODET_MHA_CHUNK_MB");
  const size_t mb = e && atoi(e) > 0 ? (size_t)atoi(e) : (size_t)1024;
  const size_t per = (size_t)Hd * Lq * up4((size_t)Lk) * 4;
  size_t c = (mb << 20) / (per ? per : 1);
  if (c < 1) c = 1;
  return c > (size_t)B ? B : (int)c;
}
inline size_t mha_scratch_floats(int B, int Hd, int Lq, int Lk) { return (size_t)mha_chunk_images(B, Hd, Lq, Lk) * Hd * Lq * up4((size_t)Lk); }

// ------------------------------------------------------------------------------------------------ GEMM descriptors
inline GemmEpi gepi(const float* bias, float* out, int ldc, int act = ACT_NONE, const float* resid = nullptr, int ldr = 0) {
  GemmEpi e; memset(&e, 0, sizeof e);
  e.bias = bias; e.out_f32 = out; e.ldc = ldc; e.act = act; e.resid = resid; e.ldr = ldr;
  return e;
}
inline GemmF32X xgemm(const float* A, int lda, bool a_km, const float* W, int ldw, bool w_km, float* C, int ldc, int M, int N, int K, float alpha, bool accumulate) {
  GemmF32X g; memset(&g, 0, sizeof g);
  g.A = A; g.lda = lda; g.a_kmajor = a_km; g.W = W; g.ldw = ldw; g.w_kmajor = w_km; g.C = C; g.ldc = ldc;
  g.M = M; g.N = N; g.K = K; g.batch = 1; g.hb = 1; g.alpha = alpha; g.accumulate = accumulate; g.ksplit = 1;
  return g;
}

// ------------------------------------------------------------------------------------------------ launchers (train_ops.hip)
// The arithmetic of a linear's product: the exact-fp32 MFMA kernels (gemm_f32.hip), or -- DOD_PREC_BF16X3 in the step's configuration -- the
// bf16 split product on fp32 operands (gemm_f32x3.hip: same operands, tape and scratch; a few 1e-6 from the exact product).  An ARGUMENT of every
// linear, taken from the configuration each entry point is given: forward and backward of one step run on different threads, and two models of
// one process may train in different modes -- nothing thread-local or global could carry it.
enum Mm { MM_F32 = 0, MM_X3 = 1 };
inline Mm mm_of(const dod_config* c) { return c && c->precision == DOD_PREC_BF16X3 ? MM_X3 : MM_F32; }
// Linears.  Y[M,N] = act(X[M,K] W[N,K]^T + b) (* scale[n]) (+ resid[M, ldr]), never K-split;  dX[M,K] (+)= dY[M,N] W[N,K];
// dW[N,K] += dY^T X, db[N] += colsum(dY)
int lin_fwd(const float* X, int ldx, const float* W, const float* b, int M, int N, int K, float* Y, int ldy, int act, Mm mm, hipStream_t s,
            const float* scale = nullptr, const float* resid = nullptr, int ldr = 0);
int lin_bwd_x(const float* dY, int ldy, const float* W, int M, int N, int K, float* dX, bool accumulate, Mm mm, hipStream_t s);
int lin_bwd_w(const float* dY, int ldy, const float* X, int ldx, int M, int N, int K, float* dW, float* db, Mm mm, hipStream_t s);
// pointwise: each wrapper owns its kernel's grid formula
int colsum_add(const float* src, int ld, int rows, int cols, float* dst, hipStream_t s);                                         // dst[c] += sum_r src[r][c]
int dropout_add(const float* a, const float* b, float* out, size_t n, float p, unsigned long long key, hipStream_t s);            // out = a + keep(b) / (1 - p); a may be null
int add_inplace(float* a, const float* b, size_t n, hipStream_t s);
int relu_drop_bwd(const float* dy, const float* y, float* g, size_t n, float p, unsigned long long key, hipStream_t s);           // g = keep(dy) / (1 - p) where y > 0
int gelu_fwd(const float* pre, float* h, size_t n, hipStream_t s);
int gelu_bwd(const float* dy, const float* pre, float* g, size_t n, hipStream_t s);
int swiglu_fwd(const float* pre, float* h, size_t rows, int F, hipStream_t s);                                                    // pre [rows, 2F] = [x1 | x2] -> h [rows, F]
int swiglu_bwd(const float* dh, const float* pre, float* dpre, size_t rows, int F, hipStream_t s);
int colscale(const float* a, const float* v, float* out, size_t n, int D, hipStream_t s);                                         // out[i] = a[i] * v[i % D]
int sigmoid_bwd4(const float* dbox, int ldd, const float* box, int ldb, float* dz, int rows, hipStream_t s);                      // dz [rows, 4] = dbox * box (1 - box)
int batch_sum(const float* d, float* dq, int B, size_t per, hipStream_t s);                                                       // dq[i] += sum_b d[b][i]
int ln_bwd(const float* x, const float* gamma, const float* dy, float eps, int rows, int D, float* dx, float* dgamma, float* dbeta, hipStream_t s);
// batched-GEMM attention (dropout on the probabilities): rectangular and packed q | k | v forms.  S, dS, Pd: mha_scratch_floats() each
int launch_mha_fwd_rect(const float* q, int ldq, const float* k, const float* v, int ldkv, float* out, int ldo, float* S, int B, int Lq, int Lk, int Hd, int dh,
                        float scale, float p, unsigned long long key, hipStream_t s);
int launch_mha_bwd_rect(const float* q, int ldq, const float* k, const float* v, int ldkv, const float* dO, int ldo, float* dq, int lddq, float* dk, float* dv,
                        int lddkv, float* dS, float* Pd, int B, int Lq, int Lk, int Hd, int dh, float scale, float p, unsigned long long key, hipStream_t s);
// the packed self-attention forms: qkv [B*Q, ld] = [q | k | v]
inline int launch_mha_fwd_train(const float* qkv, int ld, float* out, int ldo, float* S, int B, int Q, int Hd, int Dd, int dh, float scale, float p,
                                unsigned long long key, hipStream_t s) {
  return launch_mha_fwd_rect(qkv, ld, qkv + Dd, qkv + 2 * Dd, ld, out, ldo, S, B, Q, Q, Hd, dh, scale, p, key, s);
}
inline int launch_mha_bwd(const float* qkv, int ld, const float* dO, int ldo, float* dqkv, float* dS, float* Pd, int B, int Q, int Hd, int Dd, int dh, float scale,
                          float p, unsigned long long key, hipStream_t s) {
  return launch_mha_bwd_rect(qkv, ld, qkv + Dd, qkv + 2 * Dd, ld, dO, ldo, dqkv, ld, dqkv + Dd, dqkv + 2 * Dd, ld, dS, Pd, B, Q, Q, Hd, dh, scale, p, key, s);
}
// adjoint of the deformable gather: dproj zero on entry, dvalues accumulated.  Returns a dod_status.
int launch_deform_bwd(const float* proj, int ldp, const float* values, const float* dout, int B, int Q, int N, int Hd, int P, int dh, int h, int w, float* dproj, float* dvalues, hipStream_t s);
// gradients of one LoRA pair for out = X W'^T over M rows: dB [out, r] += alpha dY^T (X A^T), dA [r, in] += alpha (dY B)^T X;  T, U: [M, up4(r)] scratch
int lora_grads(const float* X, int in_f, const float* dY, int ldy, int out_f, const float* A, const float* Bm, int M, int r, float alpha, float* dA, float* dB, float* T, float* U, hipStream_t s);

}  // namespace dtrain
