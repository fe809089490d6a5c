// Host-side internals of libdinodet.so shared by dod_pack.hip (weight packing), dod_forward.hip (workspace + the two forward schedules)
// and dod_api.hip (C ABI): the handle, the packed layers, error / profiling helpers and the precision predicates.
#pragma once
#include "dod_common.h"
#include "../../include/dinodet.h"

#include <cstring>
#include <map>
#include <string>
#include <vector>

// ptr: the fp32 view the packer reads (== raw for fp32 tensors; a widened temporary made by finalize for bf16 ones)
struct WRef { const float* ptr; std::vector<int64_t> shape; const void* raw = nullptr; int dtype = DOD_F32; size_t numel() const { size_t n = 1; for (auto s : shape) n *= (size_t)s; return n; } };

// One block linear as the packer left it.  Which fields are set names the GEMM family that runs it (dod_forward.hip block_linear).
struct PackedLinear {
  void* W = nullptr;                     // bf16 or fp32 by precision; pair layout (bf16x3), H2 rows (fp16x2), e4m3 (fp8 mode; GELU-MLP fc2 stays bf16)
  float* bias = nullptr;
  const unsigned char* wexp = nullptr;   // fp16x2 mode: per-row E8M0 exponent bytes of the H2 weight rows
  const float* wscale = nullptr;         // fp8 mode: per-output-feature dequant scales
  const unsigned char* wbs = nullptr;    // fp8 mode, block-scaled weights: e8m0 bytes [rows][2][K / 64] (then wscale stays null)
  const float* csum = nullptr;           // folded LayerNorm: column sums of the packed rows
};
struct BLayer {
  PackedLinear qkv, o, fc1, fc2;
  float *ln1w = nullptr, *ln1b = nullptr, *ln2w = nullptr, *ln2b = nullptr, *ls1 = nullptr, *ls2 = nullptr;
  bool glu = false;      // SwiGLU: fc1 holds weights_in with the (x1_i, x2_i) rows INTERLEAVED; the gate runs in the GEMM epilogue
  // folded LayerNorm (GemmEpi::ln_*): qkv / fc1 hold W diag(gamma), their biases b + W beta, their csum the column sums of the packed rows
  bool fold = false;
};
struct DLayer {
  float *in_w = nullptr, *in_b = nullptr, *out_w = nullptr, *out_b = nullptr;
  float *n1w = nullptr, *n1b = nullptr, *n2w = nullptr, *n2b = nullptr, *n3w = nullptr, *n3b = nullptr;
  float *l1w = nullptr, *l1b = nullptr, *l2w = nullptr, *l2b = nullptr;
  // bf16x3-split copies [out, 3*in] of the query-side weights (bf16 mode only; see rowops.hip split3_kernel)
  bf16_t *in_w3 = nullptr, *out_w3 = nullptr, *l1w3 = nullptr, *l2w3 = nullptr, *op_w3 = nullptr, *ca_q_w3 = nullptr, *ca_out_w3 = nullptr;
  // deformable
  float *cat_w = nullptr, *cat_b = nullptr, *op_w = nullptr, *op_b = nullptr, *vp_b = nullptr;
  void* vp_w = nullptr;            // bf16 / fp32
  bf16_t* vp_w2 = nullptr;         // bf16x3 mode: pair layout
  bf16_t* ca_kv_w2 = nullptr;
  int vp_alias = -1;               // index of an earlier layer with the same (tied) value_proj, or -1
  // standard branch cross attention
  float *ca_q_w = nullptr, *ca_q_b = nullptr, *ca_kv_b = nullptr, *ca_out_w = nullptr, *ca_out_b = nullptr;
  void* ca_kv_w = nullptr;         // bf16 / fp32 [2Dd, Dd]
};

struct dod_handle {
  dod_config cfg;
  std::map<std::string, WRef> w;
  mutable std::string err;
  bool finalized = false;
  bool has_bb = false, has_dec = false;   // which halves of the state dict were registered
  std::vector<void*> owned;
  // packed
  std::vector<BLayer> L;
  void* Wpatch = nullptr; int Kp = 0;
  bf16_t* Wpatch2 = nullptr; int Kp2 = 0;   // bf16x3 mode: pair-layout patch weight, K padded to a multiple of 32
  bf16_t* Wpe = nullptr;                    // fused patch embed (patch_embed.hip): weight in the kernel's k order (pair layout in bf16x3 mode)
  float *bpatch = nullptr, *cls = nullptr, *pos = nullptr, *lnfw = nullptr, *lnfb = nullptr, *bproj = nullptr;
  void* Wproj = nullptr;
  std::vector<DLayer> DL;
  bf16_t* bb0_w3 = nullptr;
  float *query = nullptr, *cls_w = nullptr, *cls_b = nullptr, *bb0_w = nullptr, *bb0_b = nullptr, *bb2_w = nullptr, *bb2_b = nullptr;
  int ncat = 0;
  // Layer 0 of the decoder starts from tgt = query_embed for EVERY image (detr_decoder.py:59): its self-attention block and (deformable branch)
  // its reference-point / offset / weight projections are functions of the weights alone -- computed once when the weights are packed, by the
  // forward's own code path (decoder_impl, l0_only), and reused by every forward (five launches of ~25 us each on 2..72 workgroups otherwise)
  float *l0_tgt = nullptr, *l0_proj = nullptr;
  // position-table cache
  // one table per distinct (H, W), kept until the next finalize / destroy: alternating input sizes neither leak nor
  // re-allocate, and hipGraphs captured for an earlier shape keep valid pointers
  std::map<std::pair<int, int>, float*> pos_cache;
  int pos_H = -1, pos_W = -1; float* pos_hw = nullptr;
  std::map<int, float*> taps;
  // optional per-kernel-class timing with HIP events on the caller's stream (bench.py roofline leg)
  bool prof_on = false;
  struct ProfRec { hipEvent_t a, b; int cls; double flops; };
  std::vector<ProfRec> prof;
  std::vector<hipEvent_t> evpool;
};

namespace dod {

// ------------------------------------------------------------------------------------------- errors
int fail(const dod_handle* h, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));   // dod_api.hip; h null: dod_fail's slot of the calling thread
// a launcher's return code (0 ok, 3 = the HIP runtime refused the launch, else a rejected shape / argument) as DOD_ERR_* with "<what> rejected (rc r)"
int rejected(const dod_handle* h, int r, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
#define HIPCHK(h, x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return dod::fail(h, DOD_ERR_HIP, "%s: %s", #x, hipGetErrorString(e_)); } while (0)
#define KCHK(h, x) do { int r_ = (x); if (r_) return dod::rejected(h, r_, "%s", #x); } while (0)

// ------------------------------------------------------------------------------------------- profiling
enum { PC_GEMM_BF16 = 0, PC_ATTN_BF16 = 1, PC_GEMM_F32 = 2, PC_ATTN_F32 = 3, PC_LAYERNORM = 4, PC_OTHER = 5, PC_GEMM_FP8 = 6, PC_COUNT = 7 };
struct ProfScope {
  dod_handle* h; hipStream_t s; int cls; double flops; hipEvent_t a = nullptr;
  ProfScope(dod_handle* h_, hipStream_t s_, int cls_, double flops_) : h(h_), s(s_), cls(cls_), flops(flops_) {
    if (!h->prof_on) return;
    a = take();
    if (a) (void)hipEventRecord(a, s);
  }
  hipEvent_t take() {
    hipEvent_t e = nullptr;
    if (!h->evpool.empty()) { e = h->evpool.back(); h->evpool.pop_back(); return e; }
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
  }
  ~ProfScope() {
    if (!h->prof_on || !a) return;
    hipEvent_t b = take();
    if (!b) { h->evpool.push_back(a); return; }
    (void)hipEventRecord(b, s);
    h->prof.push_back({a, b, cls, flops});
  }
};

// ------------------------------------------------------------------------------------------- precision
inline bool is_fp8(const dod_handle* h) { return h->cfg.precision == DOD_PREC_FP8; }
// bf16x3: the backbone block linears run as split products on the bf16 kernels; every other choice follows the fp32 mode
inline bool is_x3(const dod_handle* h) { return h->cfg.precision == DOD_PREC_BF16X3 || h->cfg.precision == DOD_PREC_FP16X2; }
// fp16x2: as bf16x3, with the four linears of every backbone block on H2-format operands (gemm_pp.hip gemm_h2_256x256_kernel)
inline bool is_h2(const dod_handle* h) { return h->cfg.precision == DOD_PREC_FP16X2; }
// operand dtype of everything that is not an fp8 GEMM: bf16 in both the bf16 and the fp8 mode
inline bool is_bf16(const dod_handle* h) { return h->cfg.precision == DOD_PREC_BF16 || is_fp8(h); }
inline size_t esz(const dod_handle* h) { return is_x3(h) ? 6 : (is_bf16(h) ? 2 : 4); }   // x3: [hi | hi | lo] bf16 per element
// norm1 / norm2 can be folded into the QKV / MLP-in GEMMs (bf16 and the compensated modes; the strict fp32 and the fp8 schedule keep the
// LayerNorm kernel).  The ONE predicate behind the workspace's statistics buffers, BLayer::fold and the forward's choice of schedule.
inline bool ln_foldable(const dod_handle* h) { return !is_fp8(h) && (is_bf16(h) || is_x3(h)) && h->cfg.hidden % 32 == 0; }

inline GemmEpi epi(const float* bias, float* of32, void* obf, int ldc, int act = ACT_NONE, const float* scale = nullptr, const float* resid = nullptr, int ldr = 0) {
  GemmEpi e; memset(&e, 0, sizeof e);
  e.bias = bias; e.out_f32 = of32; e.out_bf16 = (bf16_t*)obf; e.ldc = ldc; e.act = act; e.scale = scale; e.resid = resid; e.ldr = ldr;
  return e;
}

// ------------------------------------------------------------------------------------------- workspace (dod_forward.hip)
struct Carver {
  char* base; size_t off = 0;
  explicit Carver(void* b) : base((char*)b) {}
  void* take(size_t bytes) { void* p = base ? base + off : nullptr; off += align_up(bytes); return p; }
};
inline void* align_ws(void* p) { return (void*)(((uintptr_t)p + 255) & ~(uintptr_t)255); }
// the real carve must fit what the sizing pass (a carve from a null base) reported: a buffer taken only when another POINTER is non-null
// is invisible to the sizing pass -- fail loudly instead of writing past the caller's workspace
#define CARVE_FITS(h, c, workspace, wsb)                                                                                      \
  if ((size_t)((c).base - (char*)(workspace)) + (c).off > (wsb))                                                              \
    return dod::fail(h, DOD_ERR_STATE, "internal: workspace carve %zu exceeds the %zu bytes provided", (size_t)((c).base - (char*)(workspace)) + (c).off, (size_t)(wsb));
struct DecWS { float *tgt, *t2, *att, *samp, *qkv, *proj, *ffn, *hb, *qd; void* mem_op; float* values; float* kv; bf16_t* a3; bf16_t* a3b; bf16_t* mem2; };   // mem2: bf16x3 mode, memory in the pair layout [M, 2*Dd]
struct BbWS { float* x; void *y, *qkv, *ctx, *hbuf, *gated, *mem; float* rs; unsigned char* bs; unsigned char* bsx; float2 *lnp, *lns, *lns2; };   // bsx: fp8 mode, e8m0 block scales of the D-wide operand rows in ws.y   // rs: fp8 mode, per-row activation scales [M]; lnp / lns: folded LayerNorm group / row statistics
size_t carve_decoder(const dod_handle* h, Carver& c, int B, int N, DecWS* w, bool need_mem_op);
size_t carve_backbone(const dod_handle* h, Carver& c, int B, int N, BbWS* w);

// ------------------------------------------------------------------------------------------- schedules
int finalize_impl(dod_handle* h, hipStream_t s);      // dod_pack.hip
int launch_widen_bf16(const bf16_t* in, float* out, size_t n, hipStream_t s);   // dod_pack.hip: bf16 weights, debug taps
int prepare_impl(dod_handle* h, int H, int W, hipStream_t s);
// DINOv2Backbone.forward (dinov2_backbone.py:58-67) -> ws.mem (operand dtype) and/or feat_f32
// stop_blocks >= 0: run the embeddings and the first stop_blocks encoder blocks only and copy the fp32 residual stream to x_out
int backbone_impl(dod_handle* h, const float* pixels, int B, int H, int W, const BbWS& ws, float* feat_f32, bool want_mem, hipStream_t s,
                  int stop_blocks = -1, float* x_out = nullptr, const unsigned char* pixels_u8 = nullptr);
// DETRDecoder.forward (detr_decoder.py:47-83).  mem_op: memory in the operand dtype (bf16 in fast mode).
// l0_only: run layer 0's image-independent prefix for ONE image (ws sized for B = 1) and leave it in ws.tgt / ws.proj (dod_finalize_weights)
int decoder_impl(dod_handle* h, const void* mem_op, int B, int N, const DecWS& ws, float* det, hipStream_t s, bool l0_only = false);

}  // namespace dod
