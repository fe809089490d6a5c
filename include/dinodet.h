/* dinodet.h -- C ABI of the MI355X-native dino_detector forward path (libdinodet.so).
 *
 * The reference (mudit1729/dinov2-od) is pure Python and has no FFI of its own; this ABI is the
 * boundary SURVEY.md section 8b defines for the path
 *     DINOv2ObjectDetector.forward   dino_detector/models/detector.py:58-69
 *       DINOv2Backbone.forward       dino_detector/models/dinov2_backbone.py:58-67
 *       DETRDecoder.forward          dino_detector/models/detr_decoder.py:47-83
 * and is what the reference-side binding (a ctypes stub) calls.
 *
 * Conventions
 *  - plain pointers and sizes only; every tensor pointer is a DEVICE pointer (HIP), row-major, fp32
 *    unless stated; `stream` is a hipStream_t passed as void* (NULL = default stream).
 *  - every call returns 0 on success, a non-zero dod_status otherwise; no C++ exception crosses
 *    the ABI.
 *  - errors: a failing call that is given a handle leaves its message on that handle, read with
 *    dod_last_error(handle).  Every other failing call (dod_create, a NULL handle, every stateless
 *    entry point: ops, training steps, optimizer, pre / post-processing, tracking, evaluation)
 *    has written the CALLING THREAD's message slot before it returns non-zero; a successful call
 *    leaves the slot alone.  The message begins with the entry point's name (the training steps:
 *    with the step's; dod_create and the dod_op_* operators name the offending argument only).
 *    dod_last_error(NULL), dod_decoder_train_last_error() and
 *    dod_optim_last_error() all return the calling thread's slot: the pointer is valid until that
 *    thread's next failing call.
 *  - all work is enqueued on the caller's stream; forward calls never synchronise and never
 *    allocate once dod_prepare() has been called for that (H, W).
 *  - a handle is re-entrant across handles but not thread-safe on one handle (the reference is
 *    one Python thread per process, one process per GPU: train.py:1501-1506).
 *  - ownership: I/O buffers, the workspace and the weight tensors passed to dod_set_weight are
 *    caller-owned; weights are only read during dod_finalize_weights(), which builds the handle's
 *    private packed copy (LoRA merged, QKV concatenated, bf16 casts).
 */
#ifndef DINODET_H
#define DINODET_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dod_handle dod_handle;

enum dod_dtype { DOD_F32 = 0, DOD_BF16 = 1 };

enum dod_status {
  DOD_OK = 0,
  DOD_ERR_INVALID = 1,      /* bad argument / unsupported shape  (Python raises ValueError)   */
  DOD_ERR_MISSING = 2,      /* a required state-dict key was never set (KeyError)             */
  DOD_ERR_STATE = 3,        /* call order: not finalized, workspace too small (RuntimeError)  */
  DOD_ERR_HIP = 4           /* HIP runtime error (RuntimeError)                               */
};

enum dod_precision {
  DOD_PREC_FP32 = 0,        /* exact-fp32 MFMA/VALU everywhere: the mode gated at 1e-3 parity  */
  DOD_PREC_BF16 = 1,        /* bf16 MFMA operands in the backbone + value projection, fp32
                               accumulate / residual stream / LayerNorm / softmax / decoder     */
  DOD_PREC_BF16X3 = 3,      /* backbone linears as bf16x3 split products on the bf16 MFMA kernels (A = Ah + Al, W = Wh + Wl,
                               Ah Wh + Ah Wl + Al Wh: ~1e-5 relative, fp32-class accuracy at a third of the bf16 rate);
                               everything else as FP32.  A parity-gated mode that runs on the bf16 matrix cores   */
  DOD_PREC_FP8 = 2,         /* as BF16, with the QKV / MLP-in (/ SwiGLU MLP-out) linears on OCP e4m3 MFMA operands:
                               per-token activation scales from the producing LayerNorm / SwiGLU kernel, per-output-
                               feature weight scales (BASELINE configs[4]: ViT-g/14 fp8)          */
  DOD_PREC_FP16X2 = 4       /* as BF16X3, with the four linears of every backbone block as fp16 main product + both cross terms
                               on ONE block-scaled e4m3 MFMA (x = fp16(x) + remainder; 2.0 bf16-MFMA-equivalents per product
                               instead of 3; ~2e-5 relative per linear).  Parity-gated like BF16X3; operands limited to the
                               fp16 range (|x| <= 65504, clamped beyond)                          */
};

/* Shapes.  Backbone fields mirror HF Dinov2Config as used by dinov2_backbone.py:11-27; decoder
 * fields mirror the DETRDecoder constructor (detr_decoder.py:8-9) / config.py:21-35. */
typedef struct dod_config {
  int32_t hidden;           /* D: 384 / 768 / 1024 / 1536 */
  int32_t layers;
  int32_t heads;            /* head_dim must be 64 in bf16 mode */
  int32_t swiglu;           /* 1 for giant (Dinov2SwiGLUFFN) */
  int32_t patch;            /* 14 */
  int32_t pos_grid;         /* 37: pretrained position grid side */
  int32_t ffn_hidden;       /* 4*D, or the SwiGLU hidden size (4096 for giant) */
  float   ln_eps;           /* 1e-6 */
  int32_t lora_r;           /* informational; LoRA presence is detected per linear from the keys */
  float   lora_alpha;
  int32_t target_dim;       /* 0 = no projection (dinov2_backbone.py:33-37) */
  int32_t num_queries;
  int32_t dec_hidden;       /* Dd */
  int32_t dec_heads;
  int32_t dec_layers;
  int32_t num_classes;
  int32_t dim_feedforward;
  int32_t n_points;
  int32_t use_deformable;
  float   dec_ln_eps;       /* 1e-5 */
  int32_t precision;        /* dod_precision */
} dod_config;

int dod_create(const dod_config* cfg, dod_handle** out);
void dod_destroy(dod_handle* h);
const char* dod_last_error(const dod_handle* h);

/* Register one device tensor (dtype DOD_F32, or DOD_BF16 for half-width checkpoints: widened to fp32 while packing) under its reference state-dict key
 * (e.g. "backbone.dino.encoder.layer.3.attention.attention.query.weight",
 *  "...layer.11.mlp.fc1.lora_A.weight", "decoder.decoder.layers.0.cross_attn.value_proj.bias").
 * A leading "module." (DDP, train.py:700-709) is ignored.  Unknown keys are accepted and unused. */
int dod_set_weight(dod_handle* h, const char* key, const void* dev_ptr, const int64_t* shape, int ndim, int dtype /* dod_dtype */);

/* Build the packed weights (merges W + alpha*B*A, concatenates q/k/v, casts).  Synchronises `stream`
 * once at the end; after it returns the caller's weight tensors are no longer referenced.
 * May be called again after new dod_set_weight calls (e.g. after load_state_dict / an optimizer step). */
int dod_finalize_weights(dod_handle* h, void* stream);

/* Precompute (and cache in the handle) the position table for an H x W input -- bicubic resize of the
 * pretrained grid when (H/patch, W/patch) != (pos_grid, pos_grid), modeling_dinov2.py:57-95.
 * Forward calls do this lazily; call it first when the forward is to be captured in a hipGraph. */
int dod_prepare(dod_handle* h, int H, int W, void* stream);

/* Bytes of scratch a forward of batch B at H x W needs. 0 on error. */
size_t dod_workspace_bytes(const dod_handle* h, int B, int H, int W);
int dod_num_tokens(const dod_handle* h, int H, int W);     /* N = (H/p)*(W/p) + 1 */

/* DINOv2ObjectDetector.forward: pixels [B,3,H,W] -> detections [B, Q, C+4] packed
 * (columns 0..C-1 = pred_logits, C..C+3 = pred_boxes cx,cy,w,h after sigmoid). */
int dod_forward(dod_handle* h, const float* pixels, int B, int H, int W, float* detections,
                void* workspace, size_t workspace_bytes, void* stream);

/* dod_forward that also hands out the decoder's memory -- the DINOv2 patch tokens after the final LayerNorm and projection, which the
 * forward leaves in HBM anyway -- into `memory` [B, N, Dd] fp32 (caller-owned; token 0 of an image is CLS).  It is filled where tap 1000
 * reads, between the backbone and the decoder schedule: one device-to-device copy in the fp32 and bf16x3 modes, one widening pass in the
 * bf16 / fp8 modes.  Detections are bit-identical to dod_forward's on the same input, mode and workspace; the workspace query is the
 * same.  memory == NULL returns DOD_ERR_INVALID.  What dod_roi_embed pools from. */
int dod_forward_mem(dod_handle* h, const float* pixels, int B, int H, int W, float* detections, float* memory,
                    void* workspace, size_t workspace_bytes, void* stream);

/* The same forward from the device input pipeline's bytes: pixels_hwc = uint8 [B, H, W, 3] (dod_preprocess_u8: the resampled
 * image before ToTensor); the patch-embedding kernel applies ToTensor's x / 255 in its load stage, so the fp32 CHW batch of
 * train.py:584-587 never exists in HBM.  Same detections, bit for bit, as dod_forward on dod_preprocess's output.
 * bf16 / bf16x3 / fp8 precision only (the fused patch embedding). */
int dod_forward_u8(dod_handle* h, const uint8_t* pixels_hwc, int B, int H, int W, float* detections,
                   void* workspace, size_t workspace_bytes, void* stream);

/* DINOv2Backbone.forward: pixels -> features [B, N, out_dim] fp32 (CLS token at index 0). */
int dod_backbone_forward(dod_handle* h, const float* pixels, int B, int H, int W, float* features,
                         void* workspace, size_t workspace_bytes, void* stream);
/* The frozen prefix of the backbone: embeddings (modeling_dinov2.py:97-116) and the first `nblocks` encoder blocks
 * (:361-380) -> the fp32 residual stream x_out [B, N, hidden].  Training only touches the last two blocks (LoRA,
 * dinov2_backbone.py:47-51), so the blocks before them need no autograd: the train()-mode composite runs them here. */
int dod_backbone_prefix(dod_handle* h, const float* pixels, int B, int H, int W, int nblocks, float* x_out,
                        void* workspace, size_t workspace_bytes, void* stream);

/* DETRDecoder.forward: memory [B, N, Dd] fp32 -> detections [B, Q, C+4] packed. */
int dod_decoder_forward(dod_handle* h, const float* memory, int B, int N, float* detections,
                        void* workspace, size_t workspace_bytes, void* stream);
size_t dod_decoder_workspace_bytes(const dod_handle* h, int B, int N);

/* Debug taps: if set, the next forwards copy that stage (fp32) into `dst` (caller-sized).
 * stage: 0 = embeddings [B,N,D]; 1+i = output of encoder block i [B,N,D]; 1000 = decoder memory
 * [B,N,Dd] (final LayerNorm / projection); 2000 = value projection [B,N,Dd]; 3000+j = decoder layer j
 * output [B,Q,Dd].  dst = NULL clears the tap. */
int dod_set_tap(dod_handle* h, int stage, float* dst);

/* Per-kernel-class timing with HIP events recorded on the caller's stream around each launch of the
 * forward (used by bench.py's roofline leg; adds an event pair per launch, so it is off in the timed
 * region).  dod_profile(h, 1) clears and enables, forwards accumulate, dod_profile_read() waits for the
 * events and returns summed milliseconds, algorithmic FLOPs (2*M*N*K resp. 4*B*N*N*D) and launches.
 * cls: 0 bf16 MFMA GEMM, 1 bf16 flash attention, 2 fp32 MFMA GEMM, 3 fp32 attention, 4 backbone LayerNorm, 6 fp8 MFMA GEMM. */
int dod_profile(dod_handle* h, int enable);
int dod_profile_read(dod_handle* h, int cls, double* ms, double* flops, int* launches);

/* ---- stateless operator entry points (the same kernels the forward uses; for parity tests) ------ */
enum dod_act { DOD_ACT_NONE = 0, DOD_ACT_RELU = 1, DOD_ACT_GELU = 2, DOD_ACT_SIGMOID = 3,
               DOD_ACT_SWIGLU_PAIRS = 4 };   /* dod_op_linear only: the N columns are interleaved SwiGLU pairs (2i: x1_i, 2i+1: x2_i); the
                                                 output has N / 2 columns silu(x1_i) * x2_i at row pitch ldc (bf16 in / out) */

/* out[M,N] = act(A[M,K] W[N,K]^T + bias) * scale + resid ; A, W of dtype `in_dtype`; bias/scale/resid fp32 or NULL */
int dod_op_linear(int in_dtype, const void* A, int lda, const void* W, int ldw, int M, int N, int K,
                  const float* bias, const float* scale, const float* resid, int ldr,
                  void* out, int out_dtype, int ldc, int act, void* stream);
/* The fp32 product in the forms the native training step uses (train.py:1079-1109):
 *   C[z] (+)= alpha * A[z] W[z]^T,  z = zb * hb + zh over `batch` strided views (X[z] = X + zb * x_sb + zh * x_sh, in floats);
 * a_kmajor / w_kmajor: that operand is stored [K, rows] (the transposed products of a backward, no transposed copies);
 * ksplit > 1 splits K over the grid and accumulates atomically (C must already hold the addend).
 * Operands whose pointer, pitch and batch strides are multiples of 4 floats are read as float4: such a buffer must hold whole
 * pitches (rows * ld floats), as any [rows, ld] allocation does. */
int dod_op_gemm_f32x(const float* A, int lda, int a_kmajor, long long a_sb, long long a_sh,
                     const float* W, int ldw, int w_kmajor, long long w_sb, long long w_sh,
                     float* C, int ldc, long long c_sb, long long c_sh,
                     int M, int N, int K, int batch, int hb, float alpha, int accumulate, int ksplit, void* stream);
/* The same product, argument for argument, as a bf16 split product on the fp32 operands (csrc/gemm_f32x3.hip): each operand is split
 * x = h + l (h = bf16_rne(x), l = bf16_rne(x - h), as dod_op_split_pair) on its way into LDS and
 *   C[z] (+)= alpha * (Ah Wh^T + Ah Wl^T + Al Wh^T),  fp32 accumulation on the bf16 MFMA
 * -- what the training step's linears run on when its configuration says DOD_PREC_BF16X3 (see "training precision" below). */
int dod_op_gemm_f32x3(const float* A, int lda, int a_kmajor, long long a_sb, long long a_sh,
                      const float* W, int ldw, int w_kmajor, long long w_sb, long long w_sh,
                      float* C, int ldc, long long c_sb, long long c_sh,
                      int M, int N, int K, int batch, int hb, float alpha, int accumulate, int ksplit, void* stream);
/* The forward linear of that mode, with the kernel's whole epilogue: Y[M,N] = act(X[M,K] W[N,K]^T + bias) * scale + resid (bias / scale / resid
 * fp32 or NULL; ldw = K; act: DOD_ACT_NONE / RELU / GELU / SIGMOID). */
int dod_op_linear_f32x3(const float* X, int ldx, const float* W, const float* bias, const float* scale, const float* resid, int ldr,
                        int M, int N, int K, float* Y, int ldy, int act, void* stream);
/* fp8 (OCP e4m3) operands, one byte per element: out = act((Aq Wq^T) * a_scale[m] * w_scale[n] + bias) * scale + resid.
 * K % 64 == 0, lda / ldw in bytes, % 16 == 0.  The ViT-g fp8 configuration's linears (BASELINE configs[4]). */
int dod_op_linear_fp8(const void* A, int lda, const float* a_scale, const void* W, int ldw, const float* w_scale,
                      int M, int N, int K, const float* bias, const float* scale, const float* resid, int ldr,
                      void* out, int out_dtype, int ldc, int act, void* stream);
/* x [rows, cols] (fp32 or bf16, ld in elements) -> q e4m3 [rows, ldq] and scale[rows] = amax_row / 448 (1 for an all-zero
 * row); q = round-to-nearest-even e4m3 of x / scale */
int dod_op_quant_rows_fp8(const void* x, int in_dtype, int ld, int rows, int cols, void* q, int ldq, float* scale,
                          void* stream);
/* Block-scaled ("MX") activations of the fp8 GEMM: x [rows, cols] (cols % 64 == 0) -> q e4m3 [rows, ldq] and one e8m0 byte per 32 elements
 * (value 2^(byte - 127): the smallest power of two >= amax_block / 448), laid out [rows][2][cols / 64]: block b of a row at byte
 * (b & 1) * (cols / 64) + (b >> 1).  dod_op_linear_fp8_mx: the linear on such an A (K % 256 == 0), W as in dod_op_linear_fp8. */
int dod_op_quant_mx_fp8(const void* x, int in_dtype, int ld, int rows, int cols, void* q, int ldq, void* block_scales, void* stream);
int dod_op_linear_fp8_mx(const void* A, int lda, const void* a_block_scales, const void* W, int ldw, const float* w_scale,
                         int M, int N, int K, const float* bias, const float* scale, const float* resid, int ldr,
                         void* out, int out_dtype, int ldc, int act, void* stream);
/* The ViT-g fp8 MLP-in linear with the SwiGLU gate AND the block-scaled quantisation of the gated row in its epilogue: W [N, K] holds the
 * (x1_i, x2_i) rows interleaved (N = 2F, N % 128 == 0); out_q [M, F] e4m3 (pitch ldq bytes) = silu(x1) * x2 / 2^e per 32 columns, the
 * e8m0 bytes in out_block_scales in the dod_op_quant_mx_fp8 layout -- the A operand of dod_op_linear_fp8_mx. */
int dod_op_linear_fp8_glu_mx(const void* A, int lda, const float* a_scale, const void* W, int ldw, const float* w_scale,
                             int M, int N, int K, const float* bias, void* out_q, int ldq, void* out_block_scales, void* stream);
/* Both operands block-scaled (what the fp8 mode's linears run since round 4): W [N, K] e4m3 with e8m0 bytes in the same [N][2][K / 64] layout
 * (dod_op_quant_mx_fp8 on the weight matrix).  glu_out_block_scales != NULL: the weights_in form of dod_op_linear_fp8_glu_mx (out = e4m3 rows
 * of N / 2 gated columns at pitch ldc bytes, out_dtype DOD_BF16 as a byte buffer). */
int dod_op_linear_fp8_mx2(const void* A, int lda, const void* a_block_scales, const void* W, int ldw, const void* w_block_scales,
                          int M, int N, int K, const float* bias, const float* scale, const float* resid, int ldr,
                          void* out, int out_dtype, int ldc, int act, void* glu_out_block_scales, void* stream);
/* bf16x3 (parity-gated mode) operators.  Pair layout: [rows, 2*cols] bf16 = [hi | lo], hi = bf16(x), lo = bf16(x - hi).
 * dod_op_split_pair: fp32 x [rows, cols] (ld) -> pair layout.
 * dod_op_linear_x3: A2 [M, 2K], W2 [N, 2K] pair layouts -> act(A W^T + bias) * scale + resid as the split product
 *   Ah Wh^T + Ah Wl^T + Al Wh^T; out_layout 0: fp32 [M, ldc], 1: bf16 [M, ldc], 2: pair layout [M, 2N] (ldc = 2N).
 * dod_op_attention_x3: qkv2 [B*N, 6*D] = [hi(q|k|v) | lo(q|k|v)] -> ctx2 [B*N, 2*D] pair layout, head_dim 64. */
int dod_op_split_pair(const float* x, int ld, int rows, int cols, void* out, void* stream);
int dod_op_linear_x3(const void* A2, const void* W2, int M, int N, int K, const float* bias, const float* scale,
                     const float* resid, int ldr, void* out, int out_layout, int ldc, int act, void* stream);
int dod_op_attention_x3(const void* qkv2, void* ctx2, int B, int N, int heads, float scale, void* stream);
/* The same attention with the fp16x2 mode's epilogue: ctx_h2 [B*N] H2 activation rows of D = heads*64 columns (4*D bytes per row, the A
 * operand of dod_op_linear_h2 with K = D): [ fp16(x) x D | per 16-column group: 16 x e4m3(h), 16 x e4m3((x - h) 2^11) ], h = fp16(x). */
int dod_op_attention_x3_h2(const void* qkv2, void* ctx_h2, int B, int N, int heads, float scale, void* stream);
/* fp16x2 (parity-gated mode) operators.  H2 operand format of a [rows, cols] matrix (cols % 32 == 0), 4*cols bytes per row:
 *   [ fp16(x) x cols | per 32-column block: 32 x e4m3(h 2^e), 32 x e4m3((x - h) 2^(e+11)) ],  h = fp16(x);
 *   activations: e = 0; weights (wexp != NULL): per row e = floor(log2(448 / max|h|)), wexp[row] = 127 - e (E8M0 byte) and the
 *   two 32-byte halves of a block swapped, so that k-slot by k-slot main meets remainder.
 * dod_op_linear_h2: act(A W^T + bias) * scale + resid with A W^T ~ fp16(A) fp16(W)^T + the two cross terms on block-scaled e4m3
 *   MFMA operands; out_layout 0: fp32, 1: bf16, 2: bf16 pair layout [M, 2N], 3: H2 rows (ldc in 2-byte units, >= 2N). */
int dod_op_split_h2(const float* x, int ld, int rows, int cols, void* out, void* wexp, void* stream);
int dod_op_linear_h2(const void* A, const void* W, const void* wexp, int M, int N, int K, const float* bias, const float* scale,
                     const float* resid, int ldr, void* out, int out_layout, int ldc, int act, void* stream);
/* LayerNorm folded into the GEMMs around it (the fast modes' schedule of modeling_dinov2.py:361-380, x -> LN -> linear): with
 * W' = W diag(gamma), c[n] = sum_k W'[n][k] and b' = b + W beta,   LN(x) W^T + b = rstd (x W'^T - mean c) + b'.
 *   consumer (stats, csum set): A holds the residual rows x themselves in the family's operand format, W holds W', bias holds b'; with part_in
 *     (a producer's group sums [M][ceil(K / 128)][2]; stats[m][0] = the shift it used) the consumer finishes the statistics itself in its
 *     epilogue (eps: the LayerNorm's) and the tiles of output column 0 write them to stats_out [M][2] (a different buffer than stats) -- what the
 *     forward does since round 4: no launch of its own merges the groups;
 *   producer (part set; out_layout 0 with a residual): beside the fp32 rows it writes them in the family's operand format to op_out
 *     ([M, N] bf16 / pair layout [M, 2N] / H2 rows) and (sum, sum of squares) of (row - shift[m][0]) per 128-column group to
 *     part [M][ceil(N / 128)][2]; shift [M][2] (or NULL = 0): a value near the row's mean -- the forward passes the row's previous
 *     statistics, which makes the one-pass sums free of cancellation;
 * dod_op_ln_finalize turns the groups into stats [M][2] = (mean, rstd); on entry stats[m][0] must hold the shift the producer used
 * (the same buffer, or zeros); dod_op_rowstats: x -> operand copy + stats (the first block).
 * family: DOD_PREC_BF16 / DOD_PREC_BF16X3 / DOD_PREC_FP16X2; A / W / wexp / out_layout as in dod_op_linear / _x3 / _h2 (bf16: lda = ldw = K). */
typedef struct dod_ln_fold {
  const void* stats;
  const float* csum;
  void* op_out;
  void* part;
  const void* shift;
  const void* part_in;
  void* stats_out;
  float eps;
} dod_ln_fold;
int dod_op_linear_ln(int family, const void* A, const void* W, const void* wexp, int M, int N, int K, const float* bias, const float* scale,
                     const float* resid, int ldr, void* out, int out_layout, int ldc, int act, const dod_ln_fold* ln, void* stream);
int dod_op_rowstats(const float* x, int rows, int D, float eps, void* op_out, int family, void* stats, void* stream);
int dod_op_ln_finalize(const void* part, int rows, int D, float eps, void* stats, void* stream);
/* out = LayerNorm(x + add) ; add may be NULL */
int dod_op_layernorm(const float* x, const float* add, const float* gamma, const float* beta, float eps,
                     int rows, int D, void* out, int out_dtype, void* stream);
/* The same LayerNorm in every output form the forward schedules launch (D % 4 == 0, D <= 2048).  `form` says what out / out2 are:
 *   DOD_LN_F32       out fp32 [rows, D]                                          out2 NULL
 *   DOD_LN_BF16      out bf16 [rows, D]                                          out2 NULL
 *   DOD_LN_F32_BF16  out fp32 [rows, D]                                          out2 bf16 [rows, D], the rounding of out
 *   DOD_LN_PAIR      out bf16 [rows, 2 D] = [hi | lo], as dod_op_split_pair      out2 NULL
 *   DOD_LN_H2        out H2 operand rows of 4 D bytes, as dod_op_split_h2 (D % 32 == 0)        out2 NULL
 *   DOD_LN_FP8       out e4m3 [rows, D], value = q * scale                       out2 fp32 scale [rows] = amax / 448 (1.0 for a zero row)
 *   DOD_LN_FP8_MX    out e4m3 [rows, D] (D % 64 == 0)                            out2 e8m0 bytes [rows][2][D / 64], as dod_op_quant_mx_fp8
 *   DOD_LN_F32_S3    out fp32 [rows, D]                                          out2 bf16 [rows, 3 D] = [hi | hi | lo], the split of out */
enum { DOD_LN_F32 = 0, DOD_LN_BF16 = 1, DOD_LN_F32_BF16 = 2, DOD_LN_PAIR = 3, DOD_LN_H2 = 4, DOD_LN_FP8 = 5, DOD_LN_FP8_MX = 6, DOD_LN_F32_S3 = 7 };
int dod_op_layernorm_form(const float* x, const float* add, const float* gamma, const float* beta, float eps,
                          int rows, int D, int form, void* out, void* out2, void* stream);
/* SwiGLU gate of [rows, 2 Fh] rows whose halves are chunked, not interleaved: out[r][c] = silu(x[r][c]) * x[r][Fh + c].  dtype DOD_F32 or
 * DOD_BF16 is the type of x and of out alike. */
int dod_op_swiglu(const void* x, void* out, int dtype, int rows, int Fh, void* stream);
/* x [rows, cols] fp32 at pitch ld -> bf16 [rows, 3 cols]: hi = bf16(x), lo = bf16(x - hi); weight_order 0: the activation operand
 * [hi | hi | lo], 1: the weight operand [hi | lo | hi] */
int dod_op_split3(const float* x, int ld, int rows, int cols, int weight_order, void* out, void* stream);
/* qkv [B*N, 3*heads*64] bf16 -> ctx [B*N, heads*64] bf16 */
int dod_op_attention_bf16(const void* qkv, void* ctx, int B, int N, int heads, float scale, void* stream);
/* The same attention with the fp8 mode's epilogue: the context leaves block-scaled, ctx_q8 [B*N, D] e4m3 bytes (D = heads*64; a head's 64
 * columns are two blocks of 32) and ctx_bs [B*N][2][D / 64] e8m0 bytes in the dod_op_quant_mx_fp8 order: block b of a row (columns
 * 32 b .. 32 b + 31) at byte (b & 1) * (D / 64) + (b >> 1); value = q * 2^(byte - 127), an all-zero block has byte 1.  Together they are
 * the A operand of dod_op_linear_fp8_mx / _mx2 with K = D. */
int dod_op_attention_bf16_mx(const void* qkv, void* ctx_q8, void* ctx_bs, int B, int N, int heads, float scale, void* stream);
int dod_op_attention_f32(const float* q, const float* k, const float* v, float* o, int ldq, int ldk, int ldv,
                         int ldo, int Lq, int Lk, int B, int heads, int dh, float scale, void* stream);
/* proj [B*Q, ldp] = [ref logits(2) | offsets(Hd*P*2) | weight logits(Hd*P)], values [B*N, Hd*dh] -> out [B*Q, Hd*dh] */
int dod_op_deform_sample(const float* proj, int ldp, const float* values, int B, int Q, int N, int Hd, int P,
                         int dh, int h, int w, float* out, void* stream);
/* The same gather as the decoder launches it: proj_shared != 0: proj has Q rows only, shared by every image (layer 0, whose queries do not
 * depend on the image); out3 != NULL: out is written a second time as the bf16 operand [B*Q, 3*Hd*dh] = [hi | hi | lo] of the output
 * projection.  1 <= P <= 8, dh <= 128, h*w == N, ldp >= 2 + 3*Hd*P. */
int dod_op_deform_sample_ex(const float* proj, int ldp, int proj_shared, const float* values, int B, int Q, int N, int Hd, int P,
                            int dh, int h, int w, float* out, void* out3, void* stream);
/* pos_in [G*G+1, D] -> pos_out [gh*gw+1, D] */
int dod_op_pos_resize(const float* pos_in, int G, int gh, int gw, int D, float* pos_out, void* stream);
/* img [B,3,H,W] -> cols [B*(H/p)*(W/p), Kp] of out_dtype */
int dod_op_im2col(const float* img, int B, int H, int W, int patch, int Kp, void* out, int out_dtype, void* stream);

/* ---- detection post-processing on device ---------------------------------------
 * Replaces the per-image / per-class / per-query loop of evaluate_coco, dino_detector/utils.py:195-233:
 * sigmoid scores (:198), background class 0 skipped (:211-212), score > threshold (0.05 at :215), cxcywh -> xyxy
 * (:86-87) -> COCO [x, y, w, h] (:225), one record per kept (image, class, query) in the reference's order
 * (image-major, then class 1..C-1, then query).  `query` is extra (the reference drops it). */
typedef struct dod_detection {
  int64_t image_id;       /* image_ids[b], or b when image_ids is NULL (target.get('image_id', i), utils.py:203) */
  int32_t category_id;    /* class index c, 1..C-1 */
  int32_t query;          /* query index q */
  float bbox[4];          /* x1, y1, x2 - x1, y2 - y1 (normalised, as the reference emits them) */
  float score;            /* sigmoid(logit) */
  int32_t reserved;
} dod_detection;          /* 40 bytes */
size_t dod_postprocess_workspace_bytes(int B, int Q, int C);
/* det: packed detections [B, Q, C+4] fp32 (the output of dod_forward), image_ids: device int64 [B] or NULL.
 * Writes min(total, max_out) records to `out` (device) and the TOTAL number of kept detections to *count (device
 * int64; > max_out means truncated).  Enqueued on `stream`; no host synchronisation. */
int dod_postprocess(const float* det, int B, int Q, int C, const int64_t* image_ids, float threshold,
                    dod_detection* out, int64_t max_out, int64_t* count, void* workspace, size_t workspace_bytes,
                    void* stream);

/* ---- detection output on device: top-k, pixel boxes, optional NMS -----------------------------------
 * What a caller that is not running COCO eval wants from the packed detections: per image the K best (query, class) pairs as xyxy
 * boxes in pixels with score and label, duplicates optionally removed.  Fixed-shape outputs, one launch on `stream`, no host
 * synchronisation, no atomics on global memory: the results are a function of the input bits and bit-identical from run to run.
 *   candidates of image b   all (q, c) with c >= first_class (1 skips the background class as dod_postprocess does; 0 keeps it) whose
 *                           logit is not NaN and for which threshold < 0 or sigmoid(logit) > threshold, sigmoid = 1 / (1 + expf(-x)).
 *   order                   logit descending, ties by flat index q*C + c ascending.  Ranking is on the logit's bits (sign-flipped
 *                           to an order-preserving integer: +0.0 ranks before -0.0, +inf first, -inf last), never on the fp32 score, so
 *                           it is a total order where the sigmoid saturates.  The first K candidates in that order are selected.
 *   box                     x1 = cx - 0.5 w, y1 = cy - 0.5 h, x2 = cx + 0.5 w, y2 = cy + 0.5 h (as dod_postprocess), then x *= width_b,
 *                           y *= height_b with sizes[b] = (height, width) fp32 (device [B, 2]; NULL = 1 x 1: boxes stay normalised),
 *                           then with clamp != 0 every coordinate v becomes v < 0 ? 0 : (v > limit ? limit : v), limit = width_b or
 *                           height_b.  One fp32 rounding per operation.
 *   NMS (iou_threshold >= 0)  greedy over the selected candidates in their order, on the output boxes: j is suppressed by an earlier
 *                           survivor i when (class_agnostic or label_i == label_j) and inter > iou_threshold * union, in fp32 and in
 *                           this order: iw = max(0, min(x2i, x2j) - max(x1i, x1j)), ih likewise, inter = iw * ih,
 *                           area = max(0, x2 - x1) * max(0, y2 - y1), union = (area_i + area_j) - inter; min(a, b) = a < b ? a : b,
 *                           max(a, b) = a > b ? a : b.  No division: the decision can be reproduced bit for bit on the host.
 *                           Survivors are compacted to the front in order.  NMS needs K <= 512 (its K x K bit matrix lives in LDS).
 *   outputs                 scores [B, K] f32 (the sigmoid), labels [B, K] i32 (c), queries [B, K] i32 (q), boxes [B, K, 4] f32 xyxy
 *                           (16-byte aligned), counts [B] i32.  Rows at and beyond counts[b] are padding: score 0, label -1, query -1,
 *                           box 0.
 * Limits: 1 <= K <= 1024, Q*C <= 2^20, C >= 1, 0 <= first_class < C, B, Q >= 1; outside them, for a NULL det / output pointer or a
 * workspace below dod_detect_workspace_bytes(B, Q, C, K) (which is 0 outside the limits) the call returns DOD_ERR_INVALID before
 * any launch.  All pointers are device pointers. */
size_t dod_detect_workspace_bytes(int B, int Q, int C, int K);
int dod_detect(const float* det, int B, int Q, int C, int first_class, const float* sizes, float threshold, int K,
               float iou_threshold, int class_agnostic, int clamp, float* scores, int32_t* labels, int32_t* queries, float* boxes,
               int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* ---- sliced and flip-augmented inference: the detections of several views of an image merged on device ---------
 * A fixed-square forward gives a small object one or two patches; the remedy is to run the model on overlapping tiles of the source
 * image next to the whole image, optionally on mirrored copies, and to merge the answers in source-image coordinates.  dod_detect_views
 * is that merge: dod_detect over ALL views of an image at once, every box mapped back through its view's rectangle and mirror flag.
 * Fixed-shape outputs, one launch on `stream`, no host synchronisation, no atomics on global memory: the results are a function of
 * the input bits, bit-identical from run to run and on any stream.
 *   det            fp32 [V, Q, C+4]: the packed forward output of all V views of all B images, view-major.
 *   view_offsets   int32 [B+1], non-decreasing, view_offsets[0] = 0, view_offsets[B] = V: the views of image b are rows
 *                  view_offsets[b] .. view_offsets[b+1] - 1; v below is the index LOCAL to the image, v0 = view_offsets[b].  An image
 *                  may have no view: it gets count 0 and padding rows.
 *   view_rects     int32 [V, 4]: (left, top, width, height) = (vl, vt, vw, vh) of the view in source pixels;  view_flips uint8 [V]:
 *                  non-zero = the view was mirrored left-right.  The tensors, in the format, that dod_preprocess_aug* reads as `crops`
 *                  and `flips`.
 *   sizes          fp32 [B, 2]: (height_b, width_b) of the source images, as dod_detect takes them; not optional here.
 *   candidates of image b   every (v, q, c) over its views with c >= first_class whose logit is not NaN and for which threshold < 0
 *                  or sigmoid(logit) > threshold (dod_detect's rule), and whose (v, q) passes the edge filter below.
 *   order          logit descending on the logit's bits with dod_detect's key image (+0.0 before -0.0, +inf first, -inf last); ties by
 *                  flat index (v*Q + q)*C + c ascending.  The first K candidates are selected.
 *   box            fp32, one rounding per operation, in this order:  x1 = cx - 0.5f*w, x2 = cx + 0.5f*w, y1 = cy - 0.5f*h,
 *                  y2 = cy + 0.5f*h;  with the flip set  t = 1.0f - x2; x2 = 1.0f - x1; x1 = t;  then  x = x * (float)vw, then
 *                  x = x + (float)vl  for x1 and x2, and  y = y * (float)vh, then y = y + (float)vt  for y1 and y2;  then the edge
 *                  filter;  then with clamp != 0 dod_detect's clamp to [0, width_b] and [0, height_b].
 *   edge filter    edge_margin m > 0 (m <= 0 or NaN: off) drops partial objects cut by a tile border.  A (v, q) is no candidate when
 *                  any of  vl > 0 && x1 < (float)vl + m;  (float)(vl + vw) < width_b && x2 > (float)(vl + vw) - m;
 *                  vt > 0 && y1 < (float)vt + m;  (float)(vt + vh) < height_b && y2 > (float)(vt + vh) - m  holds, on the box before
 *                  the clamp (vl + vw is the integer sum).  Every comparison is false on NaN.  A border of the view that is also a
 *                  border of the source image never filters.
 *   NMS (iou_threshold >= 0)  greedy over the selected candidates in their order, on the output boxes, with dod_detect's iw, ih,
 *                  inter, area and union arithmetic and its class rule; pairs of one view are treated like any other.
 *                  nms_metric 0 (IoU): j is suppressed by an earlier survivor i when inter > iou_threshold * union;
 *                  nms_metric 1 (intersection over the smaller box, what slicing tools use across views): when
 *                  inter > iou_threshold * min(area_i, area_j), min(a, b) = a < b ? a : b.  No division in either form.
 *                  Survivors are compacted to the front in order.  K may be 1024 here: the relation is kept upper-triangular in LDS.
 *   outputs        scores [B, K] f32, labels [B, K] i32, views [B, K] i32 (v, local to the image), queries [B, K] i32, boxes
 *                  [B, K, 4] f32 xyxy in source pixels (16-byte aligned), counts [B] i32.  Rows at and beyond counts[b] are padding:
 *                  score 0, label, view and query -1, box 0.
 * Limits: 1 <= K <= 1024 with or without NMS, Q*C <= 2^20, C >= 1, 0 <= first_class < C, B, Q >= 1, V >= 0, nms_metric 0 or 1;
 * outside them, for a NULL pointer (det, view_rects and view_flips may be NULL only when V == 0), a boxes pointer that is not 16-byte
 * aligned or a workspace below dod_detect_views_workspace_bytes(V, Q, C, K) (which is 0 outside the limits and never 0 inside them)
 * the call returns DOD_ERR_INVALID before any launch.  (views of one image) * Q * C <= 2^20 is a limit on device data, which the
 * call does not read on the host: the caller keeps it (dinov2_od_amd.slicing.plan_views raises), and an image whose offsets break
 * it, decrease or leave [0, V] is treated as an image without views.  All pointers are device pointers. */
size_t dod_detect_views_workspace_bytes(int V, int Q, int C, int K);
int dod_detect_views(const float* det, int B, int V, int Q, int C, const int32_t* view_offsets, const int32_t* view_rects,
                     const uint8_t* view_flips, const float* sizes, int first_class, float threshold, int K, float iou_threshold,
                     int nms_metric, int class_agnostic, int clamp, float edge_margin, float* scores, int32_t* labels, int32_t* views,
                     int32_t* queries, float* boxes, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the same merge by weighted boxes fusion instead of NMS ---------------------------------------------
 * NMS keeps the best of the views' answers for an object and discards the rest.  dod_fuse_views averages the boxes that agree, with
 * their scores as weights, and lowers the fused score when fewer views agree than could have seen the box.  Arguments, candidates,
 * order, box, edge filter, limits and error codes are dod_detect_views' (there is no nms_metric: the match measure is IoU); the n <= K
 * selected candidates 0 .. n-1, in their order, then pass ONCE through the following, in fp32 with one rounding per operation.
 *   cluster        label, member count T, five running sums  S_x1 = sum s*x1, S_y1, S_x2, S_y2, S_s = sum s  over its members (score s,
 *                  box x1 y1 x2 y2), its fused box, and its founder = first member.  Clusters are numbered in founding order.
 *   match          candidate i (score s, box b, label l) matches cluster c when (class_agnostic or label_c == l) and
 *                  inter > iou_threshold * union, with dod_detect's iw, ih, inter, area and union arithmetic between the cluster's
 *                  CURRENT fused box (in the place of the earlier survivor i of NMS) and b.  Among several matching clusters the one
 *                  with the largest quotient inter / union (one fp32 division) takes the candidate; equal quotients go to the lowest
 *                  cluster number.  Every comparison is false on NaN: a NaN box founds a cluster nothing joins.  iou_threshold < 0 or
 *                  NaN, like iou_threshold >= 1 (inter <= union), matches nothing: the result is dod_detect_views' without NMS.
 *   update         on a match  S_k = S_k + s * coord_k  (the product rounds, then the sum),  S_s = S_s + s,  T = T + 1,  fused box
 *                  = S_k / S_s (four divisions), then with clamp != 0 dod_detect's clamp again.  Without a match the candidate founds
 *                  a cluster: S_k = s * coord_k, S_s = s, fused box = b itself, T = 1.
 *   coverage       view v of the image covers a fused box f when  f.x1 >= (float)vl, f.y1 >= (float)vt, f.x2 <= (float)(vl + vw),
 *                  f.y2 <= (float)(vt + vh)  and, with edge_margin > 0, the edge filter's predicate is false for f against v.
 *                  Mirrored views count like plain ones.  N = max(1, number of covering views of the image).
 *   score          conf 0 ("max"): the founder's score.  conf 1 ("avg"):  mean = S_s / (float)T;  mean if T >= N, else
 *                  mean * (float)T / (float)N  evaluated left to right.  Scores are NOT thresholded again after fusion: `threshold`
 *                  acts on the candidates only, and an "avg" score may lie below it.
 *   output order   conf 0: founding order (descending in the founder's logit).  conf 1: fused score descending, ties by cluster number.
 *   outputs        scores (fused score), labels (the cluster's), views and queries (the founder's), boxes (the fused box),
 *                  members [B, K] i32 (T), counts [B] (the number of clusters).  Padding rows as dod_detect_views', members 0.
 * The fused box a candidate meets depends on all earlier candidates: the pass is serial over the candidates (about half a
 * microsecond each on an MI355X) and parallel over the clusters.  conf outside {0, 1} or a NULL members returns DOD_ERR_INVALID like the other argument errors, before any launch. */
size_t dod_fuse_views_workspace_bytes(int V, int Q, int C, int K);
int dod_fuse_views(const float* det, int B, int V, int Q, int C, const int32_t* view_offsets, const int32_t* view_rects,
                   const uint8_t* view_flips, const float* sizes, int first_class, float threshold, int K, float iou_threshold,
                   int class_agnostic, int clamp, float edge_margin, int conf, float* scores, int32_t* labels, int32_t* views,
                   int32_t* queries, float* boxes, int32_t* members, int32_t* counts, void* workspace, size_t workspace_bytes,
                   void* stream);

/* ---- detections and ground truth drawn into the image batch on device ---------------------------------
 * The counterpart of the reference's log_images (dino_detector/utils.py:360-384, whose box drawing is a TODO) and of
 * visualize_predictions (analyze_results.py:81-203, matplotlib on the host): up to two LAYERS of boxes -- `below` (ground truth) first,
 * `above` (predictions) over it -- are rendered into a fresh uint8 batch as outlined, optionally filled and captioned rectangles.  One
 * launch on `stream`, no host synchronisation, no atomics, no data-dependent shape: every output byte is a function of the input bits,
 * identical from run to run and on any stream.  All integer arithmetic below is exact; every fp32 operation rounds once.
 *   images      images_fp32 == 0: uint8 [B, H, W, 3] (the buffer dod_forward_u8 takes); 1: fp32 [B, 3, H, W] in [0, 1], each value x
 *               becoming the byte  v = x * 255.0f; v = v + 0.5f; NaN -> 0; v < 0 -> 0; v > 255 -> 255; truncate.
 *   out         uint8 [B, H, W, 3], never the input buffer.  Any byte alignment; nothing outside its B*H*W*3 bytes is written.
 *   a layer     struct dod_draw_layer, or NULL / boxes == NULL / K == 0 for "absent".  boxes fp32 [B, K, 4] (16-byte aligned), counts
 *               int32 [B] (NULL = K rows everywhere), labels int32 [B, K], scores fp32 [B, K] or NULL: the tensors dod_detect writes.
 *               Rows at and beyond min(max(counts[b], 0), K) are ignored.  format 0: x1, y1, x2, y2 in pixels of this image.  format 1:
 *               normalised cx, cy, w, h converted as dod_detect does with sizes = (H, W) and no clamp:  x1 = cx - 0.5f * w, then
 *               x1 = x1 * (float)W  (y with h and H, x2 / y2 with +).  A row with scores != NULL is skipped when score_threshold is
 *               not below 0 and score <= score_threshold.
 *   rectangle   a row with a NaN coordinate is skipped.  xa = I(floorf(x1)), ya = I(floorf(y1)), xb = I(ceilf(x2)) - 1,
 *               yb = I(ceilf(y2)) - 1 with I(v) = (int) of v saturated to [-32768, 32767] first (infinities saturate).  The row is
 *               skipped when xb < xa or yb < ya, or when the rectangle [xa, xb] x [ya, yb] (bounds included) has no pixel in the
 *               image [0, W) x [0, H).  Only pixels inside the image are ever touched.
 *   colour      use_palette != 0: palette[m] with m = label mod palette_size taken non-negative (uint8 [palette_size, 3] device table);
 *               otherwise the layer's own color[0..2] (r, g, b).
 *   outline     thickness t: a pixel (x, y) of the rectangle with min(x - xa, xb - x, y - ya, yb - y) < t takes the colour, opaque.
 *               (For sides >= 2 t this is Pillow's ImageDraw.rectangle([xa, ya, xb, yb], outline = c, width = t).)
 *   fill        fill_alpha a > 0: every other pixel of the rectangle becomes, per channel,  div255(dst * (255 - a) + c * a)  with
 *               div255(u) = ((u + 128) + ((u + 128) >> 8)) >> 8   (Pillow's RGBA-mode rectangle(fill = (r, g, b, a))).  a == 0: untouched.
 *   caption     font_scale s > 0.  Text: the row's class name -- the bytes of names[label] (uint8 [n_names, name_len] device table,
 *               zero padded) up to the first zero byte -- when names != NULL, 0 <= label < n_names and that name is not empty;
 *               otherwise the decimal label ('-' first when negative).  With scores != NULL a space, the decimal of
 *               p = floorf(score * 100.0f + 0.5f) (NaN -> 0, then clamped to [0, 999]) and '%' follow.  n = number of characters.
 *               Rectangle: cw = min(6 s n + s, W), ch = min(9 s, H); cy0 = ya - ch when that is >= 0 (above the box), else ya
 *               (inside it); then cy0 = min(max(cy0, 0), H - ch), cx0 = min(max(xa, 0), W - cw): the caption never leaves the image,
 *               and one wider or higher than the image is cut at its right / bottom edge.  Pixel (x, y) of [cx0, cx0 + cw) x
 *               [cy0, cy0 + ch): u = x - cx0 - s, v = y - cy0 - s (a margin of s pixels); for u, v >= 0: character i = u / (6 s), glyph
 *               column gx = (u mod 6 s) / s, glyph row gy = v / s; the pixel is TEXT when i < n, gx < 5, gy < 7 and bit (4 - gx) of
 *               font[g][gy] is set, g = byte - 0x20 for a byte in 0x20..0x7F, else 95.  font: uint8 [96, 7] device table, 5 low bits per
 *               row, bit 4 the leftmost column (dinov2_od_amd/visualize.py FONT_5X7 is the one copy; glyph 95 and every glyph the
 *               font does not design are solid).  Text pixels are black (0) when 299 r + 587 g + 114 b >= 128000 for the box colour, else
 *               white (255); every other caption pixel takes the box colour.  Both opaque.
 *   order       painter's algorithm: layer `below`, then `above`; inside a layer rows count - 1 down to 0, so row 0 ends on top; for a
 *               row the fill and outline, then its caption.
 * Limits: 1 <= B <= 65535, 1 <= H, W <= 16384, 0 <= K <= 1024 per layer, thickness 1..8, fill_alpha 0..255, font_scale 0..4 (0: no
 * captions; > 0 needs font), format 0 or 1, name_len 1..64 and n_names >= 1 when names is given, palette with palette_size >= 1 when a
 * present layer asks for it, labels != NULL for a present layer.  Outside them, for a NULL images / out / style pointer, out == images or
 * images_fp32 not 0 / 1 the call returns DOD_ERR_INVALID before any launch.  All data pointers are device pointers; the structs are
 * host memory read during the call. */
typedef struct dod_draw_layer {
  const float* boxes;
  const int32_t* counts;
  const int32_t* labels;
  const float* scores;
  int32_t K;
  int32_t format;
  float score_threshold;
  int32_t use_palette;
  uint8_t color[4];           /* r, g, b, unused */
} dod_draw_layer;
typedef struct dod_draw_style {
  int32_t thickness;
  int32_t fill_alpha;
  int32_t font_scale;
  int32_t palette_size;
  const uint8_t* palette;
  const uint8_t* names;
  int32_t n_names;
  int32_t name_len;
  const uint8_t* font;
} dod_draw_style;
int dod_draw_detections(const void* images, int images_fp32, int B, int H, int W, const dod_draw_layer* below,
                        const dod_draw_layer* above, const dod_draw_style* style, uint8_t* out, void* stream);

/* ---- input pipeline on device -------------------------------------------------------
 * Replaces the per-image host transform of dino_detector/train.py:584-587 -- torchvision Resize((R,R)) + ToTensor() on a
 * PIL image, i.e. Pillow's Image.resize(BILINEAR) (two-pass 8-bit fixed-point resample, antialiased when downscaling)
 * followed by uint8 -> float32 / 255 in CHW order -- for a ragged batch.  Bit-exact against Pillow.
 * src: concatenated uint8 HWC RGB images, image b at src + src_offs[b] with heights[b] x widths[b] pixels; tmp: the
 * horizontal-pass images, image b at tmp + tmp_offs[b] (heights[b] * out_w * 3 bytes); out: fp32 [B, 3, out_h, out_w].
 * All pointers are device pointers; max_h / max_w (host) bound the grid and the filter width (scale <= 15). */
int dod_preprocess(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int B,
                   int max_h, int max_w, int out_h, int out_w, uint8_t* tmp, const int64_t* tmp_offs, float* out,
                   void* stream);

/* as dod_preprocess, stopping before ToTensor: out_hwc = uint8 [B, out_h, out_w, 3], the input of dod_forward_u8 */
int dod_preprocess_u8(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int B,
                      int max_h, int max_w, int out_h, int out_w, uint8_t* tmp, const int64_t* tmp_offs, uint8_t* out_hwc,
                      void* stream);

/* Train-time augmentation in the same two passes (Python mirror: dinov2_od_amd/augment.py), Pillow-exact and in this order per
 * image b:  img.crop(box) -> ImageEnhance.Brightness / .Contrast / .Color (in that order) -> resize((out_w, out_h), BILINEAR) ->
 * transpose(FLIP_LEFT_RIGHT) -> ToTensor.
 *   crops   int32 [B, 4]: (left, top, width, height), a box inside image b (0 <= left, left + width <= widths[b], width >= 1,
 *           likewise vertically).  The kernels skip an image whose box is not, leaving its output unwritten; the caller validates.
 *           Pixels outside the box never enter a filter window (crop-then-resize).
 *   flips   uint8 [B]: non-zero mirrors the resized image left-right.
 *   jitter  float [B, 3]: the brightness, contrast and saturation factors, each finite and >= 0, 1.0 = identity; NULL = no jitter
 *           (the geometric-only call: no more bytes read than dod_preprocess on the same boxes).
 *   lsum    uint64 [B] caller-owned workspace of the contrast step: the call zeroes it on `stream` and sums every crop's luma into
 *           it before the horizontal pass.  It may be NULL when every contrast factor is 1.0 (host-known to the caller): the
 *           reduction is then not launched and the contrast step is skipped.
 *   max_crop_h / max_crop_w (host): the largest crop height / width; they bound the grid and the filter width
 *           (ceil(crop / out) * 2 + 1 <= 32 taps, else DOD_ERR_INVALID).
 * tmp: image b at tmp + tmp_offs[b]: (crop height of b) * out_w * 3 bytes when jitter is NULL, (crop height) * (out_w + crop
 * width) * 3 bytes otherwise -- the jittered crop is written once behind the horizontal pass's rows, so that every source pixel is
 * jittered once and not once per filter tap.  All pointers are device pointers; heights / widths are those of the source images, as
 * in dod_preprocess. */
int dod_preprocess_aug(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int B,
                       const int32_t* crops, const uint8_t* flips, const float* jitter, uint64_t* lsum, int max_crop_h,
                       int max_crop_w, int out_h, int out_w, uint8_t* tmp, const int64_t* tmp_offs, float* out, void* stream);

/* as dod_preprocess_aug, stopping before ToTensor: out_hwc = uint8 [B, out_h, out_w, 3], the input of dod_forward_u8 */
int dod_preprocess_aug_u8(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int B,
                          const int32_t* crops, const uint8_t* flips, const float* jitter, uint64_t* lsum, int max_crop_h,
                          int max_crop_w, int out_h, int out_w, uint8_t* tmp, const int64_t* tmp_offs, uint8_t* out_hwc,
                          void* stream);

/* Composed canvases (mosaic, zoom-out; Python mirror: dinov2_od_amd/augment.py compose_batch): N canvases of out_h x out_w, each a
 * fill colour with disjoint rectangular pieces pasted into it, every piece the chain of dod_preprocess_aug at its own output size.
 * Pillow-exact, per canvas n:
 *   canvas = Image.new("RGB", (out_w, out_h), fill);   for each piece p of n:
 *     im = source[p.src].crop(box) -> Brightness / Contrast / Color -> resize((dw, dh), BILINEAR) -> transpose(FLIP_LEFT_RIGHT) if flip
 *     canvas.paste(im, (dx, dy))                        -> ToTensor
 *   src, src_offs, heights, widths: S staged sources, as in dod_preprocess; several pieces may read one source.
 *   pieces         int32 [P, 10]: (source index, crop left, top, width, height, flip, dest dx, dy, dw, dh), sorted by canvas.  The contrast
 *                  mean is that of the piece's crop; the flip mirrors inside the dest rect.
 *   piece_offsets  int32 [N + 1]: canvas n owns pieces piece_offsets[n] .. piece_offsets[n + 1] - 1, at most 16 of them (a canvas may
 *                  own none: it is all fill); piece_offsets[N] = P.
 *   jitter         float [P, 3] or NULL, lsum uint64 [P] or NULL: as in dod_preprocess_aug, per piece.
 *   fills          uint8 [N, 3] when fill_per_canvas is non-zero, else uint8 [3]: the RGB fill colour.
 *   max_crop_h / max_crop_w / max_dw (host): the largest crop height and width and the largest dest width; they bound the grids.
 *   tmp            piece p at tmp + tmp_offs[p]: (crop height) * dw * 3 bytes when jitter is NULL, (crop height) * (dw + crop width) * 3
 *                  bytes otherwise (the jittered crop behind the horizontal pass's rows).
 * Every output byte of every canvas is written exactly once (one vertical + compose pass; no fill pre-pass, no atomics but the luma
 * sums).  A piece is treated as absent -- its area takes the fill -- when its source index is not in [0, S), its crop is not inside
 * its source, its dest rect is empty or not inside the canvas, it needs more than 32 filter taps (ceil(crop / dest) * 2 + 1) in
 * either direction, it exceeds one of the three host bounds, or it is the 17th or later of its canvas: a caller's mistake does not
 * fault.  The dest rects of one canvas must be pairwise disjoint (the caller checks): overlapping pieces give an unspecified but
 * in-bounds result.  DOD_ERR_INVALID when a pointer is missing, N or P <= 0, or the largest crop would need more than 32 taps even
 * for a piece as large as the canvas. */
int dod_preprocess_compose(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int S,
                           const int32_t* pieces, const int32_t* piece_offsets, int N, int P, const float* jitter, uint64_t* lsum,
                           const uint8_t* fills, int fill_per_canvas, int max_crop_h, int max_crop_w, int max_dw, int out_h,
                           int out_w, uint8_t* tmp, const int64_t* tmp_offs, float* out, void* stream);

/* as dod_preprocess_compose, stopping before ToTensor: out_hwc = uint8 [N, out_h, out_w, 3], the input of dod_forward_u8 */
int dod_preprocess_compose_u8(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int S,
                              const int32_t* pieces, const int32_t* piece_offsets, int N, int P, const float* jitter, uint64_t* lsum,
                              const uint8_t* fills, int fill_per_canvas, int max_crop_h, int max_crop_w, int max_dw, int out_h,
                              int out_w, uint8_t* tmp, const int64_t* tmp_offs, uint8_t* out_hwc, void* stream);

/* Geometric warp (random affine, perspective; Python mirror: dinov2_od_amd/augment.py warp_batch): per image b
 *   Image.transform((out_w, out_h), PERSPECTIVE, coeffs[b], BILINEAR, fillcolor=fill)  ->  ToTensor
 * Pillow-exact (src/libImaging/Geometry.c, generic transform + bilinear filter).  An affine is the 8 coefficients with a6 = a7 = 0: the
 * bytes are those of Image.AFFINE.  For output pixel (x, y), a source of W x H RGB bytes p and coefficients a[0..7], all in double,
 * one rounding per operation, no FMA contraction:
 *   xin = x + 0.5;  yin = y + 0.5
 *   den = a6*xin + a7*yin + 1
 *   sx  = (a0*xin + a1*yin + a2) / den          (left to right; the division is skipped when a6 == 0 and a7 == 0: den is exactly 1)
 *   sy  = (a3*xin + a4*yin + a5) / den
 *   outside  <=>  not (sx >= 0.0 and sx < W and sy >= 0.0 and sy < H)     -> the pixel is the fill colour (a NaN coordinate too)
 *   sx -= 0.5; sy -= 0.5;  ix = floor(sx); iy = floor(sy);  dx = sx - ix;  dy = sy - iy
 *   x0 = clamp(ix, 0, W-1);  x1 = clamp(ix+1, 0, W-1);  r0 = clamp(iy, 0, H-1)
 *   per channel:  v1 = p[r0][x0] + (p[r0][x1] - p[r0][x0]) * dx
 *                 v2 = (0 <= iy+1 < H) ? p[iy+1][x0] + (p[iy+1][x1] - p[iy+1][x0]) * dx : v1
 *                 byte = (uint8) (v1 + (v2 - v1) * dy)        (truncation; the value is always within [0, 255])
 * There is no blending with the fill at the border: a pixel is either the fill or a sample with edge clamping.
 *   src, src_offs, heights, widths: B ragged uint8 HWC sources, as in dod_preprocess (the uniform [B, h, w, 3] output of
 *           dod_preprocess_aug_u8 / dod_preprocess_compose_u8 is src_offs[b] = b * h * w * 3).  An image with heights[b] < 1 or
 *           widths[b] < 1 is all fill.
 *   coeffs  double [B, 8].  Any value is safe: the coordinates become integers only after the inside test has passed.
 *   fills   uint8 [B, 3] when fill_per_image is non-zero, else uint8 [3].
 * One launch, no workspace, no atomics, no host synchronisation; every element of out is written exactly once and nothing else is.
 * All pointers are device pointers.  DOD_ERR_INVALID when a pointer is missing, B <= 0, B > 65535, out_h <= 0 or out_w <= 0 (or
 * out_h > 524 280: past one launch). */
int dod_preprocess_warp(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int B,
                        const double* coeffs, const uint8_t* fills, int fill_per_image, int out_h, int out_w, float* out, void* stream);

/* as dod_preprocess_warp, stopping before ToTensor: out_hwc = uint8 [B, out_h, out_w, 3], the input of dod_forward_u8 */
int dod_preprocess_warp_u8(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int B,
                           const double* coeffs, const uint8_t* fills, int fill_per_image, int out_h, int out_w, uint8_t* out_hwc,
                           void* stream);

/* Baseline JPEG decode (Python mirror: dinov2_od_amd/jpeg.py decode_jpeg_batch; specification in numpy: tests/jpeg_cases.py): a batch
 * of JPEG files as bytes -> the packed uint8 RGB sources (src, src_offs, heights, widths) every dod_preprocess* entry reads, bit for
 * bit what libjpeg-turbo gives Pillow's Image.open(f).convert("RGB") (JDCT_ISLOW, fancy upsampling).  Streams taken: SOF0 / SOF1
 * Huffman, 8 bits, one interleaved scan, 8-bit quantisation tables, 3 components YCbCr with luma 1x1 / 2x1 / 2x2 and chroma 1x1, or
 * 1 component; with or without restart markers.  The header parse stays with the caller, who hands over tables of plain integers
 * (layouts: dinov2_od_amd/csrc/jpeg_entropy.h, which a host compiler can include by itself):
 *   images     int64 [B, 32], the DOD_JI_* row of every image: size, sampling, MCU counts, restart interval, the scan's byte range,
 *              and per component its first block, blocks per row, plane offset, quantisation / DC / AC table, then the output offset
 *              and the first work item of the colour stage (4 pixels of one row each; H * ceil(W / 4) per image)
 *   intervals  int64 [V, 5]: image, byte begin and end, first MCU, MCU count of one restart interval
 *   htabs      int32 [T, 802] Huffman tables: 9-bit look-up, largest code / symbol offset per length, symbols
 *   qtabs      uint16 [Q, 64] quantisation tables in natural order
 *   comps      int64 [C, 4] per component in coefficient order: first block, blocks per row, plane offset, quantisation table
 *   coef       int16 [n_blocks, 64], natural order, 16-byte aligned; zero before the entropy stage (the device stage writes non-zero
 *              coefficients only; the host entry zeroes its images' blocks itself)
 *   planes     one uint8 plane per component, padded to whole blocks (8 * blocks_w bytes per row), offsets multiples of 8
 *   status     int32 [B]: DOD_JPEG_F_* flags of a stream that ran out of bytes (1), used an undefined code (2), ran past a block's
 *              end (4), lacked a restart marker (8), left whole bytes unread behind an interval's last MCU (32), or of a descriptor naming
 *              a table or block outside its array (16)
 * The entropy stage is one function, memory-safe on any bytes: reads stay inside the interval (zero bits and flag 1 behind it), every
 * store is bounds-checked, an undefined code ends the interval.  What follows the flagged point keeps its zeros, so the pixels are
 * a function of the bytes either way.
 *   dod_jpeg_entropy_host    host code, no HIP call: decodes the whole scans of images [first, first + count) (restart markers
 *                            handled) into host memory -- meant for pinned memory and one call per thread on disjoint image ranges.
 *   dod_jpeg_entropy_device  one thread per restart interval; bytes / images / intervals / htabs / coef / status on the device.
 *   dod_jpeg_idct            dequantise + jpeg_idct_islow (CONST_BITS 13, PASS1_BITS 2, 64-bit sums, int workspace, descale by 11
 *                            and 18, + 128, range limit on the low 10 bits): every plane byte of every block written once.
 *   dod_jpeg_color           h2v1 / h2v2 fancy upsampling (plain replication for a component no wider than 2 samples; the edge
 *                            rows and columns of the ceil(W h / h_max) x ceil(H v / v_max) component replicated; block padding is
 *                            never read) + jdcolor's 16-bit tables: R = Y + ((91881 Cr' + 32768) >> 16), B = Y + ((116130 Cb' +
 *                            32768) >> 16), G = Y + ((-22554 Cb' + 32768 - 46802 Cr') >> 16), clamped; one component is replicated
 *                            to R = G = B.  Every output byte of every image with work items is written exactly once, no atomics.
 * One launch each on `stream`, no workspace, no host synchronisation.  DOD_ERR_INVALID before any launch for a NULL pointer, a
 * non-positive count or a misaligned coef / qtabs / planes. */
int dod_jpeg_entropy_host(const uint8_t* bytes, int64_t nbytes, const int64_t* images, int first, int count, const int32_t* htabs,
                          int n_htabs, int16_t* coef, int64_t coef_blocks, int32_t* status);
int dod_jpeg_entropy_device(const uint8_t* bytes, int64_t nbytes, const int64_t* images, int n_images, const int64_t* intervals,
                            int n_intervals, const int32_t* htabs, int n_htabs, int16_t* coef, int64_t coef_blocks, int32_t* status,
                            void* stream);
int dod_jpeg_idct(const int16_t* coef, int64_t n_blocks, const int64_t* comps, int n_comps, const uint16_t* qtabs, int n_qtabs,
                  uint8_t* planes, void* stream);
int dod_jpeg_color(const uint8_t* planes, const int64_t* images, int n_images, int64_t n_items, uint8_t* out, void* stream);

/* ---- Hungarian-matcher cost matrices on device -------------------------------------
 * Replaces the per-image cost computation of HungarianMatcher.forward, dino_detector/matching.py:79-98 (focal class
 * cost :80-86, L1 box cost :89, GIoU cost :92-95 with utils.py:124-164, weighted sum :98) for the whole batch.
 * Targets are concatenated: labels int64 [G], gt_boxes fp32 [G,4] (cx,cy,w,h), gt_offsets int32 [B+1] (device).
 * cost (device fp32, G*Q floats): image b's matrix [Q, n_b] row-major at cost + gt_offsets[b]*Q -- exactly the C_valid
 * the reference hands to scipy (:102-105).  rows_from: -1 = image b's own predictions; k >= 0 = the predictions of
 * image k for EVERY image (the reference slices C[:num_queries] of a matrix built over all B*Q rows, i.e. k = 0). */
int dod_match_cost(const float* det, int B, int Q, int C, const int64_t* labels, const float* gt_boxes,
                   const int32_t* gt_offsets, int G, float w_class, float w_bbox, float w_giou, float alpha, float gamma,
                   int rows_from, float* cost, void* stream);

/* ---- Hungarian assignment on device (the matcher's linear_sum_assignment, matching.py:105) ---------------------------
 * scipy.optimize.linear_sum_assignment of every image's [Q, n_b] matrix in the cost buffer dod_match_cost writes (image b at
 * cost + gt_offsets[b]*Q), one workgroup per image.  Bit-identical to scipy's result, ties included: the same shortest
 * augmenting path (Crouse) with the same double-precision operations in the same order.  All pointers
 * are DEVICE pointers; one launch on `stream`, no sync, no allocation.
 *   gt_offsets  int32 [B+1], as for dod_match_cost; G = gt_offsets[B] is the cost buffer's target count
 *   labels      int64 [G] or NULL (NULL skips the label check); C the class count it is checked against
 *   match       int32 [B*Q] out: entry b*Q + q = gt_offsets[b] + target, or -1 when query q is unmatched (the table
 *               SetCriterion consumes); every row of an image whose status is not 0 is -1
 *   status      int32 [B] out, per image:
 *                 0  solved (an image without targets is solved, all rows -1)
 *                 1  the matrix holds NaN or -inf: scipy raises ValueError("matrix contains invalid numeric entries");
 *                    also for offsets outside [0, G] or decreasing (nothing of the image is read)
 *                 2  infeasible: scipy raises ValueError("cost matrix is infeasible")
 *                 3  a label of the image lies outside [0, C) (checked before the costs): the matcher raises IndexError
 *   workspace   dod_match_assign_workspace_bytes(B, Q, G) bytes (DOD_ERR_STATE if smaller or NULL): state of the images too
 *               large for LDS
 * DOD_ERR_INVALID: a NULL offsets / match / status pointer, NULL cost with G > 0, non-positive B / Q, negative G, labels
 * with C <= 0.  Argument errors return before any HIP call. */
size_t dod_match_assign_workspace_bytes(int B, int Q, int G);
int dod_match_assign(const float* cost, const int32_t* gt_offsets, int B, int Q, int G, const int64_t* labels, int C,
                     int32_t* match, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* ---- multi-object tracking on device: ByteTrack association behind dod_detect -----------------------------------------
 * One launch per frame for S independent streams (cameras), the track table resident on the device: no host sync, no allocation,
 * no global atomics, the result a function of the input bits.  It equals the numpy + scipy restatement in tests/track_cases.py
 * bit for bit.  A tracker owns S streams of T slots each (S >= 1, T in 1..512); a frame brings K <= 1024 rows per stream, the
 * tensors dod_detect writes: scores fp32 [S, K], labels int32 [S, K], boxes fp32 [S, K, 4] pixel xyxy, counts int32 [S].
 * A slot is FREE (0), TENTATIVE (1), TRACKED (2) or LOST (3).  Every stream keeps frame (0 after reset), next_id (1 after reset:
 * the first id is 1) and an overflow counter.  One update of stream s does, in this order:
 *   0. frame += 1.  Row j < counts[s] (counts clamped to 0..K) is VALID when its score and four coordinates are finite and
 *      x2 > x1, y2 > y1, compared in fp32; every other row is ignored and gets id -1.  The measurement, in double from the widened
 *      fp32 values:  w = x2 - x1, h = y2 - y1, z = (x1 + 0.5 w, y1 + 0.5 h, w / h, h).
 *   1. Predict every TRACKED, LOST and TENTATIVE slot; a LOST slot's velocity of h is set to 0 first, as ByteTrack does.  The
 *      filter is ByteTrack's constant-velocity Kalman filter over (cx, cy, a, h), std weights 1/20 and 1/160, aspect-ratio constants
 *      1e-2 / 1e-5 / 1e-1, carried in its block form: with a diagonal initial covariance and diagonal noise the 8 x 8 covariance
 *      never leaves four independent 2 x 2 blocks (p, c, v) = (var x, cov(x, x'), var x'), and the innovation is a scalar per component:
 *        predict  q_p = (h/20)^2, q_v = (h/160)^2 from h BEFORE the step (component a: 1e-2^2, 1e-5^2);
 *                 x += x';  p = (((p + c) + c) + v) + q_p;  c = c + v;  v = v + q_v          (p from the old c and v, c from the old v)
 *        update   r = (h/20)^2 from the predicted h (component a: 1e-1^2);  s = p + r;  k_p = p / s;  k_v = c / s;  y = z - x;
 *                 x += k_p y;  x' += k_v y;  p -= (k_p k_p) s;  c -= (k_p k_v) s;  v -= (k_v k_v) s
 *        init     x = z, x' = 0, p = (2 h/20)^2, c = 0, v = (10 h/160)^2 from the measured h (component a: 1e-2^2, 1e-5^2)
 *      all in double, every operation rounded once (no FMA contraction), in the order tests/track_cases.py spells out.
 *   2. high = the valid rows with score > track_thresh, low = those with low_thresh < score <= track_thresh, both in row order.
 *   3. First association: rows = the TRACKED and LOST slots in slot order, columns = high.  cost = 1 - iou * score with fuse_score,
 *      else 1 - iou, in double, narrowed once to fp32.  iou is taken between the slot's predicted mean as xyxy (w = a h, x1 = cx - 0.5 w,
 *      y1 = cy - 0.5 h, x2 = cx + 0.5 w, y2 = cy + 0.5 h) and the row's box: widths and heights clamped at 0, union = (area_a + area_b) -
 *      inter, 0 unless union > 0; with class_aware it counts as 0 when the slot's label differs from the row's.  The rectangular
 *      problem is solved exactly as scipy.optimize.linear_sum_assignment solves the fp32 matrix (the solver of dod_match_assign, ties
 *      included); pairs with cost <= match_thresh (fp32) are kept.  A kept pair is a HIT: Kalman update, state TRACKED, last_frame =
 *      frame, the slot takes the row's score and label, the row gets the slot's id.
 *   4. Second association: the TRACKED slots (not LOST) still without a hit against low, cost 1 - iou, threshold second_thresh.
 *      Slots still without a hit become LOST.
 *   5. Tentative: the TENTATIVE slots against the high rows left over from step 3, threshold tentative_thresh, fuse_score as in
 *      step 3.  Hits become TRACKED, misses FREE.
 *   6. Expire: a LOST slot with frame - last_frame > max_age becomes FREE.
 *   7. Birth: every high row still without a slot and with score >= new_thresh takes the lowest FREE slot, in row order: filter
 *      initialised from z, id = next_id++, score, label, last_frame = frame.  At frame 1 the state is TRACKED and the row gets the id;
 *      later the state is TENTATIVE and the row keeps -1.  Without a free slot the row is dropped and overflow += 1.
 * A slot that becomes FREE keeps its other fields until a birth overwrites them: only `state` says whether they mean anything.
 * Left out on purpose: ByteTrack's remove_duplicate_stracks (duplicate removal) and camera-motion compensation; appearance costs are
 * dod_track_update_app's, below.  Two choices differ
 * from ByteTrack: association is "scipy, then filter by the threshold" (what Ultralytics does without `lap`; ByteTrack calls lapjv
 * with a cost limit), and tentative slots are predicted too.
 * Outputs per row: ids int32 [S, K] (-1 where untracked or padding), track_boxes fp32 [S, K, 4] = the slot's post-update mean as
 * xyxy, narrowed once, 0 where the id is -1.  Nothing else of the input is copied or changed.
 *   state       dod_track_state_bytes(S, T) bytes, 8-byte aligned, owned by the caller; dod_track_reset before the first update.
 *               stream_mask: int32 [S] (DEVICE), non-zero = reset that stream, or NULL = all; a stream that is not reset is not touched.
 *   workspace   dod_track_workspace_bytes(S, T, K) bytes, 8-byte aligned: per stream the compacted cost matrix (T * K floats) and the
 *               solver's state for the problems with rows + columns > 1024 (smaller ones keep it in LDS).
 *   export      the table as typed arrays (DEVICE): mean fp64 [S, T, 8] (cx, cy, a, h and their velocities), cov fp64 [S, T, 12]
 *               (component-major: p, c, v of cx, then cy, a, h), state / id / label / last_frame int32 [S, T], score fp32 [S, T],
 *               frame / next_id / overflow int32 [S].  Ten copies on `stream`.
 * The byte queries return 0 outside the limits.  DOD_ERR_INVALID before any launch: a NULL or misaligned pointer (stream_mask may be
 * NULL), S outside 1..65535, T outside 1..512, K outside 1..1024, a NaN threshold, low_thresh > track_thresh, max_age < 0, a
 * workspace smaller than the query's answer.  All data pointers are DEVICE pointers; params is read on the host. */
typedef struct dod_track_params {
  float track_thresh, low_thresh, new_thresh, match_thresh, second_thresh, tentative_thresh;
  int32_t max_age, fuse_score, class_aware;
} dod_track_params;
size_t dod_track_state_bytes(int S, int T);
size_t dod_track_workspace_bytes(int S, int T, int K);
int dod_track_reset(void* state, int S, int T, const int32_t* stream_mask, void* stream);
int dod_track_update(void* state, int S, int T, const float* scores, const int32_t* labels, const float* boxes, const int32_t* counts,
                     int K, const dod_track_params* params, int32_t* ids, float* track_boxes, void* workspace, size_t workspace_bytes,
                     void* stream);
int dod_track_export(const void* state, int S, int T, double* mean, double* cov, int32_t* slot_state, int32_t* id, int32_t* label,
                     int32_t* last_frame, float* score, int32_t* frame, int32_t* next_id, int32_t* overflow, void* stream);

/* ---- ROI embeddings from the backbone tokens -------------------------------------------------------------------------
 * One unit vector per box, pooled from features [B, N, D] fp32 (dod_forward_mem's memory, or dod_backbone_forward's features) by
 * torchvision's aligned ROIAlign rules.  One launch, no host sync, no atomics; tests/roi_embed_cases.py restates it in numpy.
 *   tokens      the tokens first_token + r * gw + c of image b form a gh x gw map (first_token = 1 skips CLS); the centre of token
 *               (r, c) is at (c + 0.5, r + 0.5) in map units.
 *   valid rows  row (b, k) is VALID when k < counts[b] (counts clamped to 0..K; NULL = K), its four coordinates are finite and x2 > x1,
 *               y2 > y1, compared in fp32 -- dod_track_update's rule.
 *   box         xyxy in the pixel frame sizes[b] = (height, width) (NULL = 1 x 1: normalised boxes).  In double from the widened values:
 *               u = (x * gw) / width clipped to [0, gw], v = (y * gh) / height clipped to [0, gh]; a box that is empty after clipping
 *               (not u2 > u1 and v2 > v1, which a size that is not a positive number ends in as well) is invalid.
 *   samples     grid x grid points u_i = u1 + (i + 0.5) (u2 - u1) / grid, v_j likewise; each is sampled bilinearly at (u_i - 0.5, v_j - 0.5):
 *               the coordinate is clamped to [0, gw - 1] / [0, gh - 1], the lower neighbour is its floor, the upper neighbour is clamped
 *               to the last index.
 *   pooled      the mean of the grid^2 samples.  Bilinear sampling on a product grid is separable, so this is
 *                 p = sum_r sum_c wy[r] wx[c] f[r, c, :]
 *               with wx[c] = (sum over the samples i of the weight they give column c, lower neighbour before upper) / grid and wy likewise:
 *               non-negative, each set sums to 1, at most 2 * grid of each are non-zero.  The weights are computed in double and narrowed
 *               once; w = wy[r] * wx[c] is one fp32 product; p accumulates in fp32 as p = fmaf(w, f, p) over the tokens with w != 0 in
 *               row-major order.  A token with w == 0 is not read.
 *   output      emb [B, K, D] = p / |p| (|p| from the fp32 p, in double; the quotient narrowed once), all zeros when |p| == 0.  Invalid
 *               and padding rows are zeros.  Every element is written exactly once; nothing outside the gh * gw tokens of the row's own
 *               image is read.
 * DOD_ERR_INVALID before any launch: a NULL features / boxes / emb, features or emb not 16-byte aligned, B < 1, K outside 1..1024,
 * D outside 4..2048 or not a multiple of 4, grid outside 1..8, gh or gw < 1, first_token < 0, first_token + gh * gw > N. */
int dod_roi_embed(const float* features, int B, int N, int D, int first_token, int gh, int gw,
                  const float* boxes /* [B, K, 4] xyxy */, const int32_t* counts /* [B] or NULL = K */,
                  const float* sizes /* [B, 2] (height, width) or NULL = 1 x 1 */, int K, int grid,
                  float* emb /* [B, K, D] */, void* stream);

/* ---- appearance in the tracker's association: BoT-SORT's fusion on dod_roi_embed's vectors -----------------------------
 * The track table keeps its layout; the slots' embeddings live in a tensor of the caller's, slot_emb [S, T, D] fp32 (zeros at the start;
 * the row of a FREE slot is never read).  One frame is three launches behind dod_detect and dod_roi_embed (emb [S, K, D]):
 *   dod_track_embed_dots     dots[s, t, j] = <slot_emb[s, t], emb[s, j]> for every t < T, j < K, fp32 [S, T, K]: the strided-batched fp32
 *                            product of dod_op_gemm_f32x.
 *   dod_track_update_app     dod_track_update with another cost in steps 3 and 5 (first and tentative association); steps 0..7 are
 *                            otherwise the ones above, word for word, and step 4 stays pure IoU.  In double:
 *                              d_iou = 1 - iou                               (iou as above, class_aware included)
 *                              base  = fuse_score ? 1 - iou * score : d_iou  (dod_track_update's cost)
 *                              d_app = 0.5 * max(0, 1 - (double) dots[s, slot, row])          (x > 0 ? x : 0)
 *                              if (d_app > appearance_thresh) d_app = 1;   if (d_iou > proximity_thresh) d_app = 1
 *                              cost  = (float) min(base, d_app)                               (d_app < base ? d_app : base)
 *                            With appearance_thresh < 0 every d_app is 1, and while base <= 1 (scores >= 0) ids, track boxes and the table equal
 *                            dod_track_update's bit for bit.  One more output, assoc int32 [S, K]: -1, or slot + 1024 * kind with
 *                              kind 0  hit in step 4: the embedding is left alone (low-score boxes are the occluded ones)
 *                              kind 1  hit in step 3 or 5: blend
 *                              kind 2  birth in step 7: store -- at every frame, also where the birth is TENTATIVE and the row's id stays -1
 *   dod_track_embed_commit   kind 2: slot_emb[s, slot] = emb[s, row].  kind 1: x = m E + (1 - m) e per element in double (m the widened
 *                            fp32 momentum, one rounding per operation), E' = (float)(x / sqrt(sum x^2)), zeros when the sum is 0.  The
 *                            rows of a frame name distinct slots: one wave per row, plain stores.
 * DOD_ERR_INVALID before any launch: what dod_track_update rejects, a NULL app_params / dots / assoc / slot_emb / emb, a NaN threshold,
 * a momentum outside [0, 1] (NaN included), D outside 4..2048 or not a multiple of 4. */
typedef struct dod_track_app_params {
  float appearance_thresh, proximity_thresh, momentum;      /* BoT-SORT's 0.25, 0.5, 0.9 */
} dod_track_app_params;
int dod_track_embed_dots(const float* slot_emb, const float* emb, int S, int T, int K, int D, float* dots, void* stream);
int dod_track_update_app(void* state, int S, int T, const float* scores, const int32_t* labels, const float* boxes, const int32_t* counts,
                         int K, const dod_track_params* params, const dod_track_app_params* app_params, const float* dots, int32_t* ids,
                         float* track_boxes, int32_t* assoc, void* workspace, size_t workspace_bytes, void* stream);
int dod_track_embed_commit(float* slot_emb, const float* emb, const int32_t* assoc, int S, int T, int K, int D, float momentum, void* stream);

/* ---- COCO bbox evaluation on device (compute_coco_metrics, dino_detector/utils.py:243-276) ---------------------------
 * pycocotools' COCOeval (iouType 'bbox', useCats = 1, default parameters: 10 IoU thresholds, 101 recall thresholds, area
 * ranges all / small / medium / large, maxDets 1 / 10 / 100) restated operation for operation in double precision
 * (csrc/cocoeval.hip): precision / recall are bit-identical to the host library's, the 12 statistics
 * equal up to the summation order of a mean.
 *
 * The evaluator's state lives in ONE caller-owned device workspace of dod_coco_eval_workspace_bytes(max_dets, I, K, G) bytes
 * (0 for unsupported sizes); every call names the same four sizes.  I / K: the annotation file's unique image / category ids;
 * G: its ground truths.  Limits: max_dets <= 2^24, I and K <= 2^24, G <= 2^26, at most 1024 ground truths in one (image,
 * category) group; any number of groups and of detections per group (the 100 best of a group are kept, as maxDets[-1]
 * keeps them).  Beyond a limit a call returns DOD_ERR_INVALID; a short or NULL workspace is DOD_ERR_STATE.
 *
 * dod_coco_eval_set_gt   HOST arrays: image_ids [I] / category_ids [K] sorted and unique; the ground truths sorted STABLY by
 *                        gt_group = category index * I + image index (so a group keeps the file's order): bbox [G,4] xywh,
 *                        the annotation's `area`, iscrowd bytes; iou_thrs [10] / rec_thrs [101] = np.linspace(.5, .95, 10) /
 *                        np.linspace(0, 1, 101) (uploaded as given, never recomputed).  Clears the detections.  Synchronises.
 * dod_coco_eval_append   `*count` (device int64) records of a device dod_detection buffer of capacity max_records -- what
 *                        dod_postprocess writes -- are appended.  Two launches on `stream`, no host synchronisation.
 * dod_coco_eval_append_host  n HOST detections with double boxes and scores (a results list).  Synchronises.
 * dod_coco_eval_reset    forgets the detections (one launch).
 * dod_coco_eval_evaluate stats: HOST double [12] = COCOeval.stats; precision / recall: DEVICE double [10,101,K,4,3] /
 *                        [10,K,4,3] or NULL; n_dets / n_groups: HOST out or NULL (detections held, ground-truth groups).
 *                        Synchronises (it reads the detection count and returns the statistics).  DOD_ERR_INVALID: more than
 *                        max_dets detections were appended or a source buffer was truncated; a detection's image id is not
 *                        in image_ids; a score is not finite; a label of dod_coco_eval_append_detections was outside its
 *                        category map.  Detections of a category the annotations lack are not
 *                        evaluated (COCOeval's catIds come from the ground truth).
 * dod_coco_eval_matches  after evaluate, copies out (DEVICE, each may be NULL) per sorted detection position [n_dets]: the
 *                        input index, the rank in its (image, category) group, and bit a*10+t of matched / ignored for area
 *                        range a and IoU threshold t (meaningful for rank < 100); per ground-truth group [n_groups]: its key
 *                        and the non-ignored ground truths per area range [n_groups, 4].
 * dod_coco_eval_append_detections  what dod_detect / dod_detect_views / dod_fuse_views write (all DEVICE): boxes [B,Kd,4] pixel
 *                        xyxy, scores [B,Kd], labels [B,Kd], counts [B]; image_ids [B] int64; category_map [n_map] int64 or NULL.
 *                        Rows 0 .. counts[b]-1 of every image are appended in (image ascending, row ascending) order -- the order
 *                        of the host list built the same way, which the stable score sort keeps for ties -- as records with
 *                        x = (double)x1, y = (double)y1, w = (double)x2 - (double)x1, h = (double)y2 - (double)y1, the score widened,
 *                        category_id = category_map[label] (the label itself without a map).  Rows at and beyond counts[b] are
 *                        never read.  Two launches on `stream` (every image's workgroup sums the counts before it; one
 *                        workgroup advances the count), no host synchronisation, no float atomics.  Records past max_dets are
 *                        not written and the count still grows, so evaluate refuses.  A counts[b] outside [0, Kd] contributes
 *                        clamp(counts[b], 0, Kd) rows and evaluate / confusion report the truncated source; a label outside
 *                        [0, n_map) with a map makes them report DOD_ERR_INVALID with a message of its own (reset clears both).
 *                        DOD_ERR_INVALID before any launch: a NULL boxes / scores / labels / counts / image_ids, B < 1 or
 *                        B > 65536, Kd < 1, n_map < 1 with a map.
 * dod_coco_eval_confusion  matrix: DEVICE int64 [K+1, K+1], overwritten; matrix[p][g] counts (predicted category index p,
 *                        ground-truth category index g) pairs at one operating point, index K standing for "background".  Per
 *                        image of the annotations the candidates are its appended detections of a category the annotations
 *                        hold with score >= score_threshold, in evaluate's stable (score descending, append order) order; the
 *                        ground truths are its non-crowd ones of ALL categories in (category index, file) order.  Each
 *                        candidate in turn takes, among the ground truths not yet taken, the one of the highest IoU (bbIou's
 *                        non-crowd form, double) that is >= min(iou_threshold, 1 - 1e-10), the LATER one on a tie (a NaN IoU
 *                        matches nothing): evaluateImg's greedy loop without ignore flags, across classes.  A match adds 1 to
 *                        matrix[pred][gt], a candidate left over to matrix[pred][K], a ground truth left over to
 *                        matrix[K][gt]; other detections and crowd ground truths appear nowhere.  Needs no evaluate before it and
 *                        leaves a later evaluate's results (and dod_coco_eval_matches' after an earlier one) as they are.
 *                        Synchronises (the count, then the input flags); integer atomics only.  DOD_ERR_INVALID: evaluate's
 *                        input errors; K > 2048; an image with more than 1024 non-crowd ground truths; a NaN threshold; a NULL
 *                        matrix. */
typedef struct dod_coco_det {
  int64_t image_id;
  int64_t category_id;
  double bbox[4];         /* x, y, w, h */
  double score;
} dod_coco_det;           /* 56 bytes */
size_t dod_coco_eval_workspace_bytes(int64_t max_dets, int n_images, int n_categories, int64_t n_gt);
int dod_coco_eval_set_gt(void* workspace, size_t workspace_bytes, int64_t max_dets, int n_images, int n_categories, int64_t n_gt,
                         const int64_t* image_ids, const int64_t* category_ids, const int64_t* gt_group, const double* gt_bbox,
                         const double* gt_area, const uint8_t* gt_iscrowd, const double* iou_thrs, const double* rec_thrs, void* stream);
int dod_coco_eval_reset(void* workspace, size_t workspace_bytes, int64_t max_dets, int n_images, int n_categories, int64_t n_gt, void* stream);
int dod_coco_eval_append(void* workspace, size_t workspace_bytes, int64_t max_dets, int n_images, int n_categories, int64_t n_gt,
                         const dod_detection* records, const int64_t* count, int64_t max_records, void* stream);
int dod_coco_eval_append_host(void* workspace, size_t workspace_bytes, int64_t max_dets, int n_images, int n_categories, int64_t n_gt,
                              const dod_coco_det* dets, int64_t n, void* stream);
int dod_coco_eval_evaluate(void* workspace, size_t workspace_bytes, int64_t max_dets, int n_images, int n_categories, int64_t n_gt,
                           double* stats, double* precision, double* recall, int64_t* n_dets, int32_t* n_groups, void* stream);
int dod_coco_eval_matches(const void* workspace, size_t workspace_bytes, int64_t max_dets, int n_images, int n_categories, int64_t n_gt,
                          int64_t n_dets, int32_t* det_index, int32_t* det_rank, uint64_t* matched, uint64_t* ignored, int32_t n_groups,
                          uint64_t* group_keys, int32_t* npig, void* stream);
int dod_coco_eval_append_detections(void* workspace, size_t workspace_bytes, int64_t max_dets, int n_images, int n_categories, int64_t n_gt,
                                    const float* boxes, const float* scores, const int32_t* labels, const int32_t* counts, int B, int Kd,
                                    const int64_t* image_ids, const int64_t* category_map, int n_map, void* stream);
int dod_coco_eval_confusion(void* workspace, size_t workspace_bytes, int64_t max_dets, int n_images, int n_categories, int64_t n_gt,
                            double score_threshold, double iou_threshold, int64_t* matrix, void* stream);

/* Stable LSD radix sort (8-bit digits) of n <= 2^24 (64-bit key, 32-bit payload) pairs on key bits [begin_bit, end_bit), both
 * multiples of 8: equal keys keep their input order.  Sorts (keys, vals) in place; keys_alt / vals_alt [n] are scratch.
 * workspace: dod_op_sort_pairs_workspace_bytes(n) bytes (0 for unsupported n).  All DEVICE pointers; no sync. */
size_t dod_op_sort_pairs_workspace_bytes(int64_t n);
int dod_op_sort_pairs_u64(uint64_t* keys, uint32_t* vals, uint64_t* keys_alt, uint32_t* vals_alt, int64_t n, int begin_bit, int end_bit,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- set-prediction loss and its gradient on device (the training criterion) ----------------------------------------
 * Replaces SetCriterion.forward, dino_detector/losses.py:204-242: the focal loss over every [B, Q, C] logit with unmatched
 * queries as background (loss_labels :100-146), the L1 and GIoU losses of the matched boxes (loss_boxes :148-185), each
 * divided by max(num_boxes, 1).  The Hungarian assignment arrives as a match table.  Stateless; all pointers are DEVICE
 * pointers owned by the caller; everything is enqueued on `stream`, no hidden sync, no allocation, no atomics (results are
 * bit-identical from run to run).
 *   pred_logits   fp32, row r = b*Q + q at pred_logits + r * logits_row_stride (>= C): a view of the packed [B, Q, C+4]
 *                 detections (stride C+4) is read in place
 *   pred_boxes    fp32 (cx, cy, w, h), row r at pred_boxes + r * boxes_row_stride (>= 4); NULL = no box terms
 *   labels        int64 [G]; gt_boxes fp32 [G, 4] cxcywh: the targets of all images, concatenated
 *   match         int32 [M = B*Q]: the global target row matched to query r, or -1 (background).  An entry outside [0, G)
 *                 is background; a label equal to C (the reference's dropped one-hot column) or outside [0, C] only
 *                 removes the focal positive -- no label or entry is ever used as an address unchecked.
 *                 NULL = row r's target is labels[r] (then G must equal B*Q): nn FocalLoss, losses.py:9-68
 *   num_boxes     fp32 device scalar (all-reduced by the caller when distributed); NULL = 1
 * Forward: losses = fp32[3] {loss_ce, loss_bbox, loss_giou}, unweighted.  elem_loss (nullable, fp32 [B*Q, C] dense): the
 * un-normalised per-element focal term (FocalLoss reduction='none').  workspace: dod_set_criterion_workspace_bytes(B, Q, C)
 * bytes (DOD_ERR_STATE if smaller).  Two launches.
 * Backward (one launch, recomputed from the inputs): d_losses = fp32[3] upstream gradient of `losses` (weights and
 * accumulation arrive through it) -- d_losses[i] / max(num_boxes, 1) reaches loss i's terms; d_elem (nullable, fp32 [B*Q, C]) is
 * the upstream gradient of elem_loss and replaces d_losses[0] element-wise (reduction='none'): d_logits = d_elem * d(elem_loss),
 * NOT divided by num_boxes, as elem_loss is not; with both given the boxes still take d_losses[1..2] / max(num_boxes, 1).
 * Writes dense d_logits fp32 [B*Q, C] and, when pred_boxes and d_boxes are given, dense d_boxes fp32 [B*Q, 4] (zero on
 * unmatched rows).  Tie rules are those of torch autograd on the reference formula.
 * DOD_ERR_INVALID: a NULL required pointer, non-positive B / Q / C, negative G, a row stride below C (logits) or 4 (boxes),
 * M != B*Q, gamma < 0. */
size_t dod_set_criterion_workspace_bytes(int B, int Q, int C);
int dod_set_criterion_forward(const float* pred_logits, int64_t logits_row_stride, const float* pred_boxes,
                              int64_t boxes_row_stride, int B, int Q, int C, const int64_t* labels, const float* gt_boxes,
                              int G, const int32_t* match, int M, const float* num_boxes, float alpha, float gamma,
                              float* losses, float* elem_loss, void* workspace, size_t workspace_bytes, void* stream);
int dod_set_criterion_backward(const float* pred_logits, int64_t logits_row_stride, const float* pred_boxes,
                               int64_t boxes_row_stride, int B, int Q, int C, const int64_t* labels, const float* gt_boxes,
                               int G, const int32_t* match, int M, const float* num_boxes, float alpha, float gamma,
                               const float* d_losses, const float* d_elem, float* d_logits, float* d_boxes, void* stream);
/* The same loss over `layers` decoder outputs against ONE set of targets (deep supervision: DETR's aux_outputs), all layers
 * in the same two / one launches.  Row r = (l*B + b)*Q + q at base + r * row_stride -- the packed [L, B, Q, C+4] detections
 * of dod_decoder_train_aux_forward are read in place; match int32 [M = layers*B*Q] holds each layer's own assignment as
 * global target rows into the one labels / gt_boxes array; losses and d_losses are fp32 [layers, 3]; d_logits / d_boxes /
 * elem_loss / d_elem are dense over all layers*B*Q rows.  Workgroups are partitioned per layer exactly as the single-layer
 * call partitions B*Q rows, so layer l's losses and gradients are bit-identical to that call on the layer's slice
 * (layers = 1 IS the single-layer call). */
size_t dod_set_criterion_layers_workspace_bytes(int layers, int B, int Q, int C);
int dod_set_criterion_layers_forward(const float* pred_logits, int64_t logits_row_stride, const float* pred_boxes,
                                     int64_t boxes_row_stride, int layers, int B, int Q, int C, const int64_t* labels,
                                     const float* gt_boxes, int G, const int32_t* match, int M, const float* num_boxes,
                                     float alpha, float gamma, float* losses, float* elem_loss, void* workspace,
                                     size_t workspace_bytes, void* stream);
int dod_set_criterion_layers_backward(const float* pred_logits, int64_t logits_row_stride, const float* pred_boxes,
                                      int64_t boxes_row_stride, int layers, int B, int Q, int C, const int64_t* labels,
                                      const float* gt_boxes, int G, const int32_t* match, int M, const float* num_boxes,
                                      float alpha, float gamma, const float* d_losses, const float* d_elem, float* d_logits,
                                      float* d_boxes, void* stream);

/* ---- native training step of the decoder + heads (first slice) ---------------------------------------
 * What `loss.backward()` at dino_detector/train.py:1101 needs from DETRDecoder.forward (detr_decoder.py:47-83) over the
 * weight-tied DeformableDecoderLayer (deformable_attention.py:215-268, tied at :284): a train-mode forward (dropout at the
 * reference's five sites, masks from a counter-based hash of `seed`) that tapes its activations, and the backward producing
 * the gradients of every decoder / head parameter and of `memory` (which the caller feeds on into the projection and the
 * LoRA-adapted blocks).  Stateless: the shapes come from `cfg`, the fp32 parameters from the caller's own tensors.
 * All pointers are device pointers.  `grads` has the layout of the parameters; its tensors are float ACCUMULATORS (the layers
 * share one set of weights; zero them for a plain gradient).  The same `dropout_p` / `seed` must be given to both calls.
 * Training precision: cfg->precision = DOD_PREC_BF16X3 runs the linears of every training step below as bf16 split products on their fp32
 * operands (dod_op_gemm_f32x3) -- the backbone tail's every linear, forward and backward; the decoders' every backward linear and their
 * forward products over the B*N memory rows (value_proj / the cross-attention k | v projection; the query-side forward stays fp32, it feeds
 * floor()).  Attention, the deformable gather, LayerNorm, the LoRA rank-r products, dropout and the deterministic mode are the fp32 step's.
 * Every other precision value behaves as DOD_PREC_FP32, and the *_tape_bytes / *_workspace_bytes answers do not depend on it. */
typedef struct dod_dec_train_params {
  const float *query_embed;                      /* [Q, Dd]            detr_decoder.py:15 */
  const float *class_w, *class_b;                /* [C, Dd], [C]       :40 */
  const float *bb0_w, *bb0_b, *bb2_w, *bb2_b;    /* bbox_embed.mlp.{0,2}  :39-41 */
  const float *in_proj_w, *in_proj_b, *out_proj_w, *out_proj_b;          /* self_attn (nn.MultiheadAttention) */
  const float *norm1_w, *norm1_b, *norm2_w, *norm2_b, *norm3_w, *norm3_b;
  const float *lin1_w, *lin1_b, *lin2_w, *lin2_b;
  const float *refp_w, *refp_b;                  /* reference_points_proj [2, Dd] */
  const float *off_w, *off_b, *aw_w, *aw_b;      /* cross_attn.sampling_offsets / attention_weights */
  const float *vp_w, *vp_b, *op_w, *op_b;        /* cross_attn.value_proj / output_proj */
} dod_dec_train_params;
size_t dod_decoder_train_tape_bytes(const dod_config* cfg, int B, int N);
size_t dod_decoder_train_workspace_bytes(const dod_config* cfg, int B, int N);
/* memory [B, N, Dd] -> detections [B, Q, C+4] (as dod_decoder_forward), activations into `tape` (keep it until the backward) */
int dod_decoder_train_forward(const dod_config* cfg, const dod_dec_train_params* params, const float* memory, int B, int N,
                              float dropout_p, uint64_t seed, float* detections, void* tape, size_t tape_bytes,
                              void* workspace, size_t workspace_bytes, void* stream);
/* d_detections [B, Q, C+4] -> grads (accumulated) and d_memory [B, N, Dd] (overwritten; may be NULL) */
int dod_decoder_train_backward(const dod_config* cfg, const dod_dec_train_params* params, const float* memory, int B, int N,
                               float dropout_p, uint64_t seed, const float* d_detections, const void* tape, size_t tape_bytes,
                               const dod_dec_train_params* grads, float* d_memory, void* workspace, size_t workspace_bytes,
                               void* stream);
/* The same step with every decoder layer's output supervised (DETR's aux_loss): detections / d_detections are
 * [L, B, Q, C+4], slice j = the shared heads on decoder layer j's output, slice L-1 = what dod_decoder_train_forward
 * returns.  Same schedule, dropout sites and keys; the heads run once over all L*B*Q rows in either direction.  Tape and
 * workspace have their own sizes. */
size_t dod_decoder_train_aux_tape_bytes(const dod_config* cfg, int B, int N);
size_t dod_decoder_train_aux_workspace_bytes(const dod_config* cfg, int B, int N);
int dod_decoder_train_aux_forward(const dod_config* cfg, const dod_dec_train_params* params, const float* memory, int B, int N,
                                  float dropout_p, uint64_t seed, float* detections, void* tape, size_t tape_bytes,
                                  void* workspace, size_t workspace_bytes, void* stream);
int dod_decoder_train_aux_backward(const dod_config* cfg, const dod_dec_train_params* params, const float* memory, int B, int N,
                                   float dropout_p, uint64_t seed, const float* d_detections, const void* tape, size_t tape_bytes,
                                   const dod_dec_train_params* grads, float* d_memory, void* workspace, size_t workspace_bytes,
                                   void* stream);
const char* dod_decoder_train_last_error(void);

/* The nn.TransformerDecoder branch of DETRDecoder (use_deformable = False; detr_decoder.py:28-35, 62-69) in train() mode:
 * post-norm nn.TransformerDecoderLayer x L with UNTIED weights -- query self-attention, dense cross-attention of the Q queries over
 * all N memory tokens, ReLU FFN, three LayerNorms, dropout at torch's six sites (both attentions' probabilities, dropout1/2/3 and
 * the FFN's inner dropout) -- and the same heads.  Same contract as dod_decoder_train_*: `grads` has the layout of the parameters
 * (float accumulators), `layers` is a HOST array of nlayers entries holding device pointers. */
typedef struct dod_dense_layer_params {
  const float *sa_in_w, *sa_in_b, *sa_out_w, *sa_out_b;      /* self_attn: in_proj [3Dd, Dd], out_proj [Dd, Dd] */
  const float *ca_in_w, *ca_in_b, *ca_out_w, *ca_out_b;      /* multihead_attn: in_proj [3Dd, Dd] = q (queries) | k | v (memory) */
  const float *lin1_w, *lin1_b, *lin2_w, *lin2_b;            /* [F, Dd], [Dd, F] */
  const float *norm1_w, *norm1_b, *norm2_w, *norm2_b, *norm3_w, *norm3_b;
} dod_dense_layer_params;
typedef struct dod_dense_dec_train_params {
  int32_t nlayers, reserved;
  const dod_dense_layer_params* layers;
  const float *query_embed, *class_w, *class_b, *bb0_w, *bb0_b, *bb2_w, *bb2_b;
} dod_dense_dec_train_params;
size_t dod_dense_decoder_train_tape_bytes(const dod_config* cfg, int B, int N);
size_t dod_dense_decoder_train_workspace_bytes(const dod_config* cfg, int B, int N);
int dod_dense_decoder_train_forward(const dod_config* cfg, const dod_dense_dec_train_params* params, const float* memory, int B, int N,
                                    float dropout_p, uint64_t seed, float* detections, void* tape, size_t tape_bytes,
                                    void* workspace, size_t workspace_bytes, void* stream);
int dod_dense_decoder_train_backward(const dod_config* cfg, const dod_dense_dec_train_params* params, const float* memory, int B, int N,
                                     float dropout_p, uint64_t seed, const float* d_detections, const void* tape, size_t tape_bytes,
                                     const dod_dense_dec_train_params* grads, float* d_memory, void* workspace,
                                     size_t workspace_bytes, void* stream);

/* The rest of the trainable subset: the LoRA-adapted encoder blocks (the last two, dinov2_backbone.py:45-51), the final
 * LayerNorm and the projection (dinov2_backbone.py:33-37, 64-65) in train() mode.  x_in [B, N, D] is the residual stream in
 * front of the first adapted block (dod_backbone_prefix: everything before it is frozen and needs no autograd); the forward
 * writes the decoder memory [B, N, Dd] and tapes its activations, the backward turns d(memory) into the gradients of every
 * lora_A / lora_B (dino_detector/utils.py:46-70) and of the projection.  Frozen tensors (w, b, LayerNorm, LayerScale) are read
 * only; in `grads` only A, Bm, proj_w, proj_b are written (float accumulators, same layout).  GELU MLP (ViT-S/B/L) or SwiGLU
 * (ViT-g, cfg->swiglu: the fc1 / fc2 slots then hold mlp.weights_in [2F, D] / mlp.weights_out [D, F]); hidden <= 2048;
 */
typedef struct dod_lora_linear { const float *w, *b, *A, *Bm; } dod_lora_linear;        /* [out,in], [out], [r,in], [out,r] */
typedef struct dod_bb_block_params {
  const float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *ls1, *ls2;                              /* frozen */
  dod_lora_linear q, k, v, o, fc1, fc2;                                                /* attention.attention.{query,key,value}, attention.output.dense, mlp.fc1, mlp.fc2 */
} dod_bb_block_params;
typedef struct dod_bb_tail_params {
  int32_t nblocks, reserved;
  const dod_bb_block_params* blocks;             /* HOST array of nblocks entries (device pointers inside) */
  const float *lnf_w, *lnf_b;                    /* final LayerNorm (frozen) */
  const float *proj_w, *proj_b;                  /* [Dd, D], [Dd]; NULL when the backbone has no projection */
} dod_bb_tail_params;
size_t dod_backbone_tail_tape_bytes(const dod_config* cfg, int B, int N, int nblocks);
size_t dod_backbone_tail_workspace_bytes(const dod_config* cfg, int B, int N, int nblocks);
int dod_backbone_tail_train_forward(const dod_config* cfg, const dod_bb_tail_params* params, const float* x_in, int B, int N,
                                    float* memory_out, void* tape, size_t tape_bytes, void* workspace, size_t workspace_bytes,
                                    void* stream);
int dod_backbone_tail_train_backward(const dod_config* cfg, const dod_bb_tail_params* params, int B, int N, const float* d_memory,
                                     const void* tape, size_t tape_bytes, const dod_bb_tail_params* grads, void* workspace,
                                     size_t workspace_bytes, void* stream);

/* ---- training-step operators: the adjoint kernels of the three steps above, one at a time ---------------------------------
 * What dod_decoder_train_*, dod_dense_decoder_train_* and dod_backbone_tail_train_* are made of (train_ops.hip, attn_f32m.hip), each
 * behind a thin entry that validates its arguments and calls the launcher the step calls -- for parity tests at shapes the steps never
 * run.  Stateless; every pointer is a caller-owned fp32 DEVICE buffer; enqueued on `stream`, no sync.  The "deterministic" test
 * option / DINODET_DETERMINISTIC selects the ordered reductions exactly as in the steps (that mode keeps a library-owned partial-sum
 * buffer).  DOD_ERR_INVALID before any launch for a NULL pointer or a shape outside the stated limits, DOD_ERR_STATE for a
 * workspace that is too small.
 *
 * LayerNorm backward: x, dy, dx [rows, D] dense, D <= 2048.  dx is written; dgamma / dbeta [D] ACCUMULATE. */
int dod_op_layernorm_bwd(const float* x, const float* gamma, const float* dy, float eps, int rows, int D, float* dx, float* dgamma,
                         float* dbeta, void* stream);
/* Attention forward + vector-Jacobian product in one call: o = dropout(softmax(scale q k^T)) v per (image, head), then dq, dk, dv
 * for the upstream gradient d_o.  q [B*Lq, ldq], k / v [B*Lk, ldkv], o / d_o [B*Lq, ldo], dq [B*Lq, lddq], dk / dv [B*Lk, lddkv]: head h
 * at columns h*dh of each, pitches multiples of 4 (q | k | v of one packed buffer: k = q + heads*dh, v = q + 2*heads*dh, ldq = ldkv).
 * All four outputs are WRITTEN.
 *   form 0  batched fp32 GEMMs around the softmax row kernels (the decoders' attention): head_dim <= 128, Lk <= 1408, dropout_p in
 *           [0, 1) with the keep mask  u01(key, ((b*heads + h)*Lq + i)*Lk + j) >= dropout_p,  kept probabilities scaled by 1/(1-p);
 *           u01(key, n) = (z >> 40) * 2^-24 for z = the splitmix64 finaliser of key + n * 0x9E3779B97F4A7C15 (mod 2^64)
 *   form 1  the flash kernels (the backbone tail at >= 1 024 tokens): head_dim 64, dropout_p == 0; o comes from the forward that
 *           also writes the log-sum-exp the adjoint recomputes its probabilities from
 * workspace: dod_op_attention_f32_vjp_workspace_bytes(...) bytes (0 for a shape the form does not take; form 0 sizes it by the
 * "mha_chunk_images" option in force at the time). */
size_t dod_op_attention_f32_vjp_workspace_bytes(int B, int Lq, int Lk, int heads, int dh, int form);
int dod_op_attention_f32_vjp(const float* q, int ldq, const float* k, const float* v, int ldkv, const float* d_o, float* o, int ldo,
                             float* dq, int lddq, float* dk, float* dv, int lddkv, int B, int Lq, int Lk, int heads, int dh,
                             float scale, int form, float dropout_p, uint64_t key, void* workspace, size_t workspace_bytes,
                             void* stream);
/* Adjoint of dod_op_deform_sample (same proj / values layout; dout [B*Q, Hd*dh]): dproj [B*Q, ldp] is zeroed and WRITTEN (columns
 * 0..1 the reference logits, shared by all heads; then offsets; then point-weight logits), dvalues [B*N, Hd*dh] ACCUMULATES.
 * 1 <= P <= 8, dh <= 128, hh*ww == N, ldp >= 2 + 3*Hd*P. */
int dod_op_deform_sample_bwd(const float* proj, int ldp, const float* values, const float* dout, int B, int Q, int N, int Hd, int P,
                             int dh, int hh, int ww, float* dproj, float* dvalues, void* stream);
/* Gradients of one LoRA pair of out = X (W + alpha Bm A)^T:  dB [out_f, r] += alpha dY^T (X A^T),  dA [r, in_f] += alpha (dY Bm)^T X.
 * X [M, in_f] dense, dY [M, out_f] with pitch ldy (a column block of a wider buffer), A [r, in_f], Bm [out_f, r]; 1 <= r <= 64
 * (r <= 8: the rank-r kernels; above: the fp32 GEMMs, which take any pitch).  Both outputs ACCUMULATE. */
size_t dod_op_lora_grads_workspace_bytes(int M, int r);
int dod_op_lora_grads(const float* X, int in_f, const float* dY, int ldy, int out_f, const float* A, const float* Bm, int M, int r,
                      float alpha, float* dA, float* dB, void* workspace, size_t workspace_bytes, void* stream);
/* Element-wise adjoints; `out` is written (it may alias `a`).  keep(i) = u01(key, i) >= p as above; p in [0, 1).
 *   DOD_PW_GELU_BWD       out[i] = a[i] * d/dx gelu_erf(b[i])                         a = dy, b = pre-activation, n elements
 *   DOD_PW_SWIGLU_BWD     b = pre [n, 2*cols] = [x1 | x2], a = dh [n, cols] -> out [n, 2*cols] = [d x1 | d x2] of silu(x1) * x2
 *   DOD_PW_RELU_DROP_BWD  out[i] = b[i] > 0 ? keep(i) a[i] / (1 - p) : 0            a = dy, b = the ReLU output
 *   DOD_PW_DROPOUT_ADD    out[i] = a[i] + keep(i) b[i] / (1 - p)                      a may be NULL (out = dropped b)
 *   DOD_PW_SIGMOID_BWD4   out[r][c] = a[r*cols + c] * s (1 - s), s = b[r*4 + c], c < 4   n rows, a with pitch cols >= 4 */
enum dod_pointwise_op { DOD_PW_GELU_BWD = 0, DOD_PW_SWIGLU_BWD = 1, DOD_PW_RELU_DROP_BWD = 2, DOD_PW_DROPOUT_ADD = 3, DOD_PW_SIGMOID_BWD4 = 4 };
int dod_op_train_pointwise(int op, const float* a, const float* b, float* out, size_t n, int cols, float p, uint64_t key, void* stream);
/* dst[c] += sum_r src[r*ld + c], c < cols (the bias gradient) */
int dod_op_colsum_add(const float* src, int ld, int rows, int cols, float* dst, void* stream);

/* ---- optimizer step on device: gradient-norm clip + Adam (train.py:1000-1004, 1101-1110 of the reference) ----------------
 * torch.nn.utils.clip_grad_norm_ (2-norm) followed by torch.optim.Adam (L2 weight_decay, no amsgrad) over a list of dense
 * fp32 tensors, in two kinds of launch (csrc/optim.hip): the gradients' sum of squares, accumulated in
 * double, one partial per workgroup; then the update, in which every workgroup adds the partials in a fixed order, forms
 *   total_norm = (float)sqrt(sum),  coef = min(1, max_norm / (sqrt(sum) + 1e-6))          (a NaN norm gives a NaN coef)
 * and updates its chunk once:
 *   g = coef * g_raw + weight_decay * p;  m += (g - m)(1 - beta1);  v = beta2 v + (1 - beta2) g g;
 *   p -= step_size * m / (sqrt(v) / bc2_sqrt + eps)
 * with step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) formed by the caller in double PER TENSOR (a parameter
 * whose gradient was None on some step has a smaller t).  g, m and v are evaluated in double and rounded once when stored.
 * beta1 / beta2 / weight_decay are doubles: 1 - (float)0.999 is 1.3e-5 away from 0.001, 36 times the bound on v by itself, and where
 * coef * g_raw and weight_decay * p cancel, a rounded weight_decay would leave g with no correct digit.
 * The tensor descriptors travel in the kernel arguments: a list longer than one argument table (56 tensors for the update, 128
 * for the norm) takes more launches; tensors with n = 0 are skipped.  16-byte accesses where all pointers of a tensor are
 * 16-byte aligned, 4-byte ones otherwise and for the n mod 4 tail; nothing past n is read or written.  No atomics: two runs of
 * the same input give the same bits.  Everything is enqueued on `stream`; no synchronisation, no allocation.
 *   dod_optim_clip_grad_norm  scales every g in place (only g and n of a descriptor are read) and stores total_norm; gradients
 *                             keep their bits when the norm is below max_norm
 *   dod_optim_adam_step       max_norm > 0: clip and update fused, the clipped gradient is NOT written back, total_norm is stored.
 *                             max_norm <= 0: no clip, no norm launch, total_norm_dev and ws are not touched (may be NULL)
 *   workspace                 dod_optim_workspace_bytes(n_tensors, total elements) bytes, monotone in both (0 for a negative one)
 * n_tensors == 0 (or no elements at all) succeeds and stores total_norm = 0.  DOD_ERR_INVALID, before any HIP call: n_tensors < 0, a NULL list, a negative n, a NULL pointer of a tensor with
 * n > 0, NULL total_norm_dev, a NULL or short workspace, betas outside [0, 1), negative eps / weight_decay.
 * dod_test_counter("optim_launches") counts the launches of both entries; "optim_chunk_elems" / "optim_table_tensors" /
 * "optim_norm_table_tensors" report the elements per workgroup and the tensors per update / norm launch. */
typedef struct dod_optim_tensor { float* p; float* g; float* m; float* v; int64_t n; float step_size; float bc2_sqrt; } dod_optim_tensor;
size_t dod_optim_workspace_bytes(int n_tensors, int64_t total_elems);
int dod_optim_clip_grad_norm(const dod_optim_tensor* t, int n_tensors, float max_norm, float* total_norm_dev, void* ws, size_t ws_bytes,
                             void* stream);
int dod_optim_adam_step(const dod_optim_tensor* t, int n_tensors, double beta1, double beta2, float eps, double weight_decay, float max_norm,
                        float* total_norm_dev, void* ws, size_t ws_bytes, void* stream);
const char* dod_optim_last_error(void);

/* ---- the same step with decoupled weight decay (AdamW), a fused moving average of the weights and a skip on a non-finite norm ----
 * dod_optim_step is dod_optim_adam_step (above: lists, workspace, alignment, errors, determinism) plus three things, each optional.
 *   decay    NULL, or one double per tensor: p is multiplied by decay[i] = 1 - lr * weight_decay BEFORE the Adam update (PyTorch's
 *            AdamW order), with options.weight_decay = 0.  A double, because 1 - 1e-8 is 1.0f.  With delta = step_size * m' / den the
 *            fp32 term of the L2 form, p' = (float)((double)p * decay[i] - (double)delta): rounded once.  decay[i] == 1.0 is the L2
 *            form's fp32 subtraction bit for bit.  A launch holds 4 runs of equal consecutive factors; a fifth starts another launch.
 *   ema      NULL, or one pointer per tensor (NULL entries allowed): the thread that stores p' also stores
 *            e' = (float)((double)e + ((double)p' - (double)e) * ema_w), ema_w = 1 - d a double (1 - (float)0.9999 is 3e-4 relative away
 *            from 1e-4), p' the fp32 value just stored, every double operation rounded by itself (no fused multiply-add, so float64
 *            arithmetic on the host gives the same bits).  The 16-byte path needs all five pointers aligned.  e must not alias p, m, v.
 *   skip_nonfinite  the norm launch runs even with max_norm <= 0 (coefficient 1 then), and when the fp32 total_norm is inf or NaN every
 *            workgroup returns before any store: p, m, v and e keep their bits.  total_norm is still stored, and thread 0 of workgroup 0
 *            of the first update launch adds 1 to *skipped_dev (int32, may be NULL; one writer, a plain load and store).
 *            norm_ready = 1 (with skip_nonfinite and max_norm <= 0): no norm launch; *total_norm_dev already holds the norm of an earlier
 *            dod_optim_clip_grad_norm over the WHOLE list and is only read -- for several dod_optim_step calls that share one norm; pass
 *            skipped_dev to one of them.
 * With decay and ema NULL and skip_nonfinite 0 the call IS dod_optim_adam_step.  dod_optim_ema_update is the average alone over a list
 * of (e, p, n), the same arithmetic in one launch per 96 tensors ("optim_ema_table_tensors"): for tensors that had no gradient this step
 * and for callers with another optimizer.  Additional DOD_ERR_INVALID: NULL options, ema_w or w outside [0, 1], a NaN decay factor, an
 * average that aliases its tensor, norm_ready without skip_nonfinite or with max_norm > 0. */
typedef struct dod_optim_options {
  double beta1, beta2;
  double weight_decay;          /* L2: added to the gradient; 0 with a decay list */
  double ema_w;                 /* 1 - d; read only with an ema list */
  float eps, max_norm;          /* max_norm <= 0: no clip */
  int32_t skip_nonfinite, norm_ready;
  float* total_norm_dev;        /* needed with max_norm > 0 or skip_nonfinite */
  int32_t* skipped_dev;
} dod_optim_options;
typedef struct dod_optim_ema_tensor { float* e; const float* p; int64_t n; } dod_optim_ema_tensor;
int dod_optim_step(const dod_optim_tensor* t, float* const* ema, const double* decay, int n_tensors, const dod_optim_options* options,
                   void* ws, size_t ws_bytes, void* stream);
int dod_optim_ema_update(const dod_optim_ema_tensor* t, int n_tensors, double w, void* stream);

/* Scratch of the GEMMs' wave-quantisation tail split (K-split partial slabs; gemm_pp.hip) and of the fp32 GEMM's K split (gemm_f32.hip, fixed size).  dod_finalize_weights reserves 64 MiB on the
 * current device; operator-level callers (tests, tools) reserve it themselves.  Never allocated inside a forward / stream capture. */
int dod_reserve_gemm_scratch(size_t bytes);
/* Test hooks.  Process-wide integer options a parity test sets for its own cases and hands back with -1 (= the shipped behaviour); they
 * are NOT environment variables -- nothing outside the calling process can change which kernel runs:
 *   "tailsplit"        GEMM wave-quantisation tail split: 0 off, 1 the shipped heuristic, 2 every qualifying shape
 *   "dec_fused_split"  0 = a split3 launch per decoder query-side linear (the round-2 schedule; bit-identical to the shipped one)
 *   "mha_chunk_images" training-step attention: images per pass (forces ragged passes on small shapes)
 *   "no_fused_patch"   1 = the explicit im2col + GEMM patch embedding (read by dod_finalize_weights)
 *   "ln_fold"          0 = LayerNorm kernels instead of the folded form (read by dod_finalize_weights)
 *   "deterministic"    1 = ordered reductions instead of fp32 atomics in the training step's weight gradients (also DINODET_DETERMINISTIC=1)
 *   "f32_ksplit"       fp32 GEMM K split across workgroups (gemm_f32.hip): 0 = never, 1 = also in dod_op_linear (shipped: the decoder's small linears in
 *                      every mode but the strict fp32 one)
 *   "attn_bwd_flash"   backbone-tail attention adjoint: 0 = never the flash form, 1 = whenever head_dim is 64 (shipped: from 1 024 tokens up;
 *                      wins over DINODET_ATTN_BWD_FLASH).  Read when the tape and workspace are sized and in both passes: set it around a whole step
 *   "epi_regmath"      16-wave bf16 GEMM with plain bf16 output rows (QKV, fc1 of the bf16 mode; gemm_x3.hip): 0 = the LDS-staged fp32 epilogue,
 *                      1 = the epilogue math on the accumulators (shipped; bit-identical).  Read once per launch
 *   "f32x3_tile"       fp32-in bf16 split GEMM (gemm_f32x3.hip): 64 / 128 = that tile for every product; 0 = the shipped rule (128x128 from 256 such
 *                      tiles up, one per CU)
 *   "attn_diet"        bf16 flash attention (attn_bf16.hip): 0 = the last key tile at full width and per-lane global pointers for the K/V staging,
 *                      1 = a last tile of at most 32 keys computes one 32-key block, staging through a buffer descriptor (shipped; bit-identical)
 * dod_test_counter("tail_splits"): GEMM calls that took the tail-split path so far; "rem_cuts": GEMM calls whose short last round ran as a
 * launch of its own (gemm_bf16.hip); "f32_ksplits": fp32 GEMM launches that split K across workgroups (gemm_f32.hip); "epi_regmath": launches
 * of the 16-wave bf16 GEMM that took the register epilogue; "f32x3_launches": launches of the fp32-in bf16 split GEMM, "f32x3_wide_launches": those
 * that took its 128x128 tile; "attn_diet": bf16 attention launches whose last key tile ran at half width; -1 for an unknown name.
 * Kernel launches per inference GEMM form, counted by the launchers (a call the heuristics cut in two counts each part under its own form; a
 * tail split's K-split launch counts under its family's ping-pong form, its reduce launch under none):
 *   "form_bf16_128_r2" / "form_bf16_128_r3"  gemm_bf16.hip 128x128 tile on a 2- / 3-slot ring;  "form_bf16_m16"  its 256x128 tile
 *   "form_k64"  16-wave 256x256 plain bf16 (gemm_x3.hip, either epilogue);  "form_ppm"  ping-pong 256x256 plain bf16 (gemm_pp.hip)
 *   "form_x3_16w" / "form_x3_pp"  split product on the 16-wave / the ping-pong kernel;  "form_h2"  the H2 kernel
 *   "form_fp8_rows"  per-row scaled e4m3;  "form_fp8mx_256x128"  block-scaled A;  "form_fp8mx2_256x128" / "form_fp8mx2_256x256"  both operands
 *   block-scaled on the 256x128 / the 256x256 tile;  "form_f32"  gemm_f32.hip;  "form_patch_fused"  the fused patch embedding (patch_embed.hip)
 * The in-kernel time stamps, the register-only MFMA probes and every tile / schedule override of the tuning rounds exist only in
 * -DDINODET_TUNING builds (include/dinodet_tuning.h); the release library exports none of them. */
int dod_test_set_option(const char* name, int value);
long dod_test_counter(const char* name);
/* What the inference GEMM launchers WOULD do, without a device (the planner of csrc/gemm_plan.h, which the launchers execute): the launches of one
 * linear in order -- at most main rows cut in two by the remainder cut, then a tail split's K-split launch and its reduce launch.  Returns the number
 * of steps written (1..4), -1 for a bad argument or max_steps too small.  The caller chooses the CU count and the scratch bytes reserved
 * (dod_reserve_gemm_scratch; > 0 also means the fp32 K split's slab exists); the "tailsplit" / "f32_ksplit" / "epi_regmath" test options are read
 * as the launchers read them.
 *   family     0 plain bf16 operands (dod_op_linear), 1 split product (dod_op_linear_x3), 2 H2 (dod_op_linear_h2), 3 fp8, 4 fp32
 *   epi_flags  what the policy reads of the epilogue, nothing else of it matters:  1 GELU, 2 sigmoid, 4 patch-embed row map, 8 fp8 per-row A scales,
 *              16 [hi | hi | lo] output, 32 K-sliced epilogue, 64 the epilogue of a row range can run as a launch of its own (no row map, K slices or fp8
 *              scales), 128 plain bf16 rows the register epilogue can write (bf16 out, N and pitch multiples of 8, no residual / pair / H2 / gated form, act
 *              none / relu / gelu), 256 / 512 / 1024 fp8 block scales of A / W / the gated output, 2048 the fp32 caller allows the K split
 *   step.form  index of the form in the dod_test_counter("form_*") list below, in that order (0 = bf16_128_r2 ... 12 = f32), or 14 = the tail
 *              split's reduce launch;  row0, rows: the rows it computes;  kslices: K slices of a K-split launch and its reduce (1 otherwise);
 *              regmath: the k64 form takes the register epilogue;  gm: grouped-order depth of the bf16_m16 and fp8 forms (0 otherwise)
 * Executing the steps moves the counters so: one per form; "tail_splits" per reduce step; "rem_cuts" per step with row0 > 0 and kslices == 1;
 * "f32_ksplits" per f32 step with kslices > 1; "epi_regmath" per step with regmath. */
typedef struct dod_gemm_step { int form, row0, rows, kslices, regmath, gm; } dod_gemm_step;
int dod_test_gemm_plan(int family, int M, int N, int K, unsigned epi_flags, int cus, size_t scratch_bytes, dod_gemm_step* steps, int max_steps);
/* What dod_finalize_weights stored, read-only (tests/test_gpu_pack.py holds every packed operand to its float64 definition).  Neither call
 * changes the handle.  dod_test_packed_info describes the operand `name`; dod_test_packed_copy enqueues a device-to-device copy of one of its
 * arrays (enum dod_packed_array) into dst, a device buffer of dst_bytes >= info.bytes[array], on `stream`.
 *   names   "Wpatch" (im2col order, K = 3 p^2 padded to pitch), "Wpatch2" (bf16x3 / fp16x2: pair layout, K padded to a multiple of 32), "Wpe" (fused
 *           patch embed: k' order of csrc/patch_embed.hip, 3 (p / 2) 32 columns), "bpatch", "cls", "pos", "lnfw", "lnfb", "Wproj", "bproj";
 *           "block.<i>.qkv" / ".o" / ".fc1" / ".fc2" (with their bias / csum / wscale / wbs / wexp arrays), ".ln1w" ".ln1b" ".ln2w" ".ln2b" ".ls1" ".ls2";
 *           "query", "cls_w", "cls_b", "bb0_w", "bb0_b", "bb0_w3", "bb2_w", "bb2_b", "l0_tgt", "l0_proj";
 *           "dec.<j>." + in_w in_b out_w out_b n1w n1b n2w n2b n3w n3b l1w l1b l2w l2b, the split3 copies in_w3 out_w3 l1w3 l2w3 op_w3 ca_q_w3
 *           ca_out_w3, deformable: cat_w cat_b op_w op_b vp_w vp_w2 vp_b, dense: ca_q_w ca_q_b ca_kv_w ca_kv_w2 ca_kv_b ca_out_w ca_out_b.
 *   format  DOD_PK_ABSENT: the name is valid but this configuration / precision keeps no such operand (arrays == 0 unless a block linear kept
 *           only its bias);  F32 / BF16: [rows, pitch / 4 or / 2] elements of which the first `cols` are data and the rest zero padding;
 *           PAIR: bf16 [hi | lo], each plane pitch / 4 elements wide;  SPLIT3W: bf16 [hi | lo | hi], three planes of `cols`;  H2W: H2 weight
 *           rows of 3 cols bytes with the WEXP array;  E4M3_ROWS: e4m3 [rows, cols] with the WSCALE array;  E4M3_MX: e4m3 [rows, cols] with the
 *           WBS array in the [rows][2][cols / 64] order of dod_op_quant_mx_fp8.  Vectors report rows = 1.
 *   glu, fold   the flags of block <i> (SwiGLU rows interleaved in fc1; LayerNorm folded into qkv / fc1), 0 for every other name
 *   vp_alias    of decoder layer <j>: the earlier layer whose value projection it shares, or -1 (also for every other name)
 * DOD_ERR_INVALID: NULL handle / name / info / dst, a name that no configuration has, an array the operand does not have, dst_bytes too small;
 * DOD_ERR_STATE: the handle is not finalized. */
enum dod_packed_format { DOD_PK_ABSENT = -1, DOD_PK_F32 = 0, DOD_PK_BF16 = 1, DOD_PK_PAIR = 2, DOD_PK_H2W = 3, DOD_PK_E4M3_ROWS = 4, DOD_PK_E4M3_MX = 5,
                         DOD_PK_SPLIT3W = 6 };
enum dod_packed_array { DOD_PK_W = 0, DOD_PK_BIAS = 1, DOD_PK_CSUM = 2, DOD_PK_WSCALE = 3, DOD_PK_WBS = 4, DOD_PK_WEXP = 5, DOD_PK_ARRAYS = 6 };
typedef struct dod_packed_info {
  int32_t format;           /* dod_packed_format */
  int32_t rows, cols;
  int32_t arrays;           /* bit a set: array a (dod_packed_array) exists */
  int64_t pitch;            /* bytes per row of the W array */
  int64_t bytes[6];         /* bytes of each array, 0 when absent */
  int32_t glu, fold, vp_alias, reserved;
} dod_packed_info;
int dod_test_packed_info(const dod_handle* h, const char* name, dod_packed_info* info);
int dod_test_packed_copy(const dod_handle* h, const char* name, int array, void* dst, size_t dst_bytes, void* stream);

const char* dod_version(void);
/* ABI revision of this header: bumped whenever an exported signature or struct layout changes (round 2's dod_set_weight gained its
 * dtype argument at revision 2; revision 4 = this file: the dod_debug_* entry points left the release library, dod_test_* replaced the three
 * the tests use, the folded-LayerNorm operators arrived; revision 5: the dod_set_criterion_* entry points; revision 6: dod_match_assign*).
 * New entry points alone change no signature and no layout: dod_coco_eval_* and dod_op_sort_pairs_* joined revision 6, and a caller that
 * needs them resolves them by name (the Python binding fails at load when one is missing).  The training-step operators
 * (dod_op_layernorm_bwd ... dod_op_colsum_add) joined revision 6 the same way.  So did the optimizer step (dod_optim_*), the deep-supervision
 * step (dod_decoder_train_aux_*), the layered criterion (dod_set_criterion_layers_*) and the split-product operators (dod_op_gemm_f32x3,
 * dod_op_linear_f32x3; the training entry points reading cfg->precision changes no signature either) and the train-time augmentation
 * (dod_preprocess_aug, dod_preprocess_aug_u8), the host-side dispatch query (dod_test_gemm_plan), the detection output (dod_detect*)
 * and the drawing entry (dod_draw_detections with its two new structs, which no earlier entry reads) and the merge of sliced
 * inference (dod_detect_views*) and its fusing form (dod_fuse_views*) and the composed canvases (dod_preprocess_compose,
 * dod_preprocess_compose_u8).
 * dod_coco_eval_append_detections and dod_coco_eval_confusion joined revision 6 the same way; the evaluator's workspace grew with them (the
 * per-image ground-truth lists), which a caller learns from dod_coco_eval_workspace_bytes as before.  The geometric warp
 * (dod_preprocess_warp, dod_preprocess_warp_u8) joined revision 6 by name as well, and so did the JPEG decode (dod_jpeg_*).
 * Revision 7: the packed-operand accessor (dod_test_packed_info, dod_test_packed_copy, struct dod_packed_info) -- additive like the above, but it
 * publishes the layout of what dod_finalize_weights keeps (the dod_packed_format / dod_packed_array numbering), which a tool built against this
 * header reads through the struct: the revision is raised so that such a tool and the library agree on it.
 * dod_optim_step and dod_optim_ema_update (with struct dod_optim_options and struct dod_optim_ema_tensor, which no earlier entry reads)
 * joined revision 7 by name: no earlier signature or layout moved.  So did the tracker (dod_track_* with struct dod_track_params), and
 * after it dod_forward_mem, dod_roi_embed and the appearance entries (dod_track_embed_dots, dod_track_update_app, dod_track_embed_commit with
 * struct dod_track_app_params, which no earlier entry reads).
 * A C caller compiled against DOD_ABI_VERSION checks it once at load. */
#define DOD_ABI_VERSION 7
int dod_abi_version(void);
/* Devices visible to the HIP runtime libdinodet.so is bound to (<= 0: none / error).  The host uses it to
 * verify the library shares PyTorch's HIP runtime (pointers and streams cross this ABI). */
int dod_device_count(void);

#ifdef __cplusplus
}
#endif
#endif
