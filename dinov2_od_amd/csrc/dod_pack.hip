// Weight packing of libdinodet.so: dod_finalize_weights turns the registered state dict into the operand formats of the handle's precision.
#include "dod_internal.h"

#include <cstdlib>

using namespace dod;

namespace {

// Device allocations of one finalize: what the handle keeps goes to h->owned, temporaries live until the Packer goes (after the stream has
// drained: the packing kernels read them), whichever way finalize returns.
struct Packer {
  dod_handle* h; hipStream_t s; std::vector<void*> tmp; int rc = 0;
  Packer(dod_handle* h_, hipStream_t s_) : h(h_), s(s_) {}
  Packer(const Packer&) = delete;
  ~Packer() {
    if (tmp.empty()) return;
    (void)hipStreamSynchronize(s);
    for (void* t : tmp) (void)hipFree(t);
  }
  template <typename T> T* alloc(size_t n, bool temp = false) {
    void* p = nullptr;
    if (rc) return nullptr;   // keep the FIRST error
    hipError_t me = hipMalloc(&p, n * sizeof(T) ? n * sizeof(T) : 4);
    if (me != hipSuccess) { rc = fail(h, DOD_ERR_HIP, "hipMalloc of %zu bytes failed: %s", n * sizeof(T), hipGetErrorString(me)); return nullptr; }
    (temp ? tmp : h->owned).push_back(p);
    return (T*)p;
  }
  const WRef* find(const std::string& k) { auto it = h->w.find(k); return it == h->w.end() ? nullptr : &it->second; }
  const WRef* need(const std::string& k, std::initializer_list<int64_t> shape) {
    const WRef* r = find(k);
    if (!r) { if (!rc) rc = fail(h, DOD_ERR_MISSING, "missing weight '%s'", k.c_str()); return nullptr; }
    if (r->shape != std::vector<int64_t>(shape)) {
      if (!rc) { std::string got; for (auto d : r->shape) got += std::to_string(d) + ","; rc = fail(h, DOD_ERR_INVALID, "weight '%s' has shape [%s] (unexpected)", k.c_str(), got.c_str()); }
      return nullptr;
    }
    return r;
  }
  // owned fp32 copy of a vector/matrix parameter
  float* copy(const std::string& k, std::initializer_list<int64_t> shape) {
    const WRef* r = need(k, shape); if (!r) return nullptr;
    float* d = alloc<float>(r->numel()); if (!d) return nullptr;
    hipError_t ce = hipMemcpyAsync(d, r->ptr, r->numel() * 4, hipMemcpyDeviceToDevice, s);
    if (ce != hipSuccess && !rc) rc = fail(h, DOD_ERR_HIP, "copy of '%s' failed: %s", k.c_str(), hipGetErrorString(ce));
    return d;
  }
  // effective fp32 weight of a (possibly LoRA-wrapped) linear: returns a device pointer valid until finalize ends
  const float* eff_weight(const std::string& prefix, int out_f, int in_f) {
    if (find(prefix + ".linear.weight")) {   // LoraLinear, dino_detector/utils.py:46-70
      const WRef* W = need(prefix + ".linear.weight", {out_f, in_f});
      const WRef* A = find(prefix + ".lora_A.weight");
      const WRef* Bm = find(prefix + ".lora_B.weight");
      if (!W) return nullptr;
      if (!A || !Bm) { rc = fail(h, DOD_ERR_MISSING, "missing lora_A/lora_B for '%s'", prefix.c_str()); return nullptr; }
      const int r = (int)A->shape[0];
      if (A->shape != std::vector<int64_t>{r, in_f} || Bm->shape != std::vector<int64_t>{out_f, r}) { rc = fail(h, DOD_ERR_INVALID, "bad LoRA shapes for '%s'", prefix.c_str()); return nullptr; }
      float* m = alloc<float>((size_t)out_f * in_f, true); if (!m) return nullptr;
      if (launch_lora_merge(W->ptr, A->ptr, Bm->ptr, h->cfg.lora_alpha, out_f, in_f, r, m, s) && !rc) rc = fail(h, DOD_ERR_HIP, "lora merge launch failed: %s", hipGetErrorString(hipGetLastError()));
      return m;
    }
    const WRef* W = need(prefix + ".weight", {out_f, in_f});
    return W ? W->ptr : nullptr;
  }
  float* eff_bias(const std::string& prefix, int out_f) {
    if (find(prefix + ".linear.bias")) return copy(prefix + ".linear.bias", {out_f});
    return copy(prefix + ".bias", {out_f});
  }
  // bf16x3 split weight [rows, 3*cols] (bf16 mode, cols % 64 == 0), else nullptr
  bf16_t* split_w(const float* src, int rows, int cols) {
    if (!src || !(is_bf16(h) || is_x3(h)) || cols % 64) return nullptr;
    bf16_t* b = alloc<bf16_t>((size_t)rows * 3 * cols); if (!b) return nullptr;
    if (launch_split3(src, cols, b, rows, cols, 1, s)) { if (!rc) rc = fail(h, DOD_ERR_HIP, "split3 launch failed"); return nullptr; }
    return b;
  }
  // split-product weight in the pair layout [Wh | Wl] (bf16x3 mode, gemm_x3.hip)
  bf16_t* pair_w(const float* src, int rows, int cols) {
    if (!src || cols % 32) return nullptr;
    bf16_t* b = alloc<bf16_t>((size_t)rows * 2 * cols); if (!b) return nullptr;
    if (launch_split2(src, cols, b, rows, cols, s)) { if (!rc) rc = fail(h, DOD_ERR_HIP, "split2 launch failed"); return nullptr; }
    return b;
  }
  // pack fp32 [rows, cols] (ld = cols) into the precision's operand dtype, K padded to cols_pad
  void* pack_operand(const float* src, int rows, int cols, int cols_pad, bool force_f32 = false) {
    if (!src) return nullptr;
    const bool bf = is_bf16(h) && !force_f32;
    float* f = alloc<float>((size_t)rows * cols_pad, bf); if (!f) return nullptr;
    if (launch_copy2d(src, cols, f, cols_pad, rows, cols, cols_pad, s)) { if (!rc) rc = fail(h, DOD_ERR_HIP, "copy2d launch failed"); return nullptr; }
    if (!bf) return f;
    bf16_t* b = alloc<bf16_t>((size_t)rows * cols_pad); if (!b) return nullptr;
    if (launch_cast_bf16(f, b, (size_t)rows * cols_pad, s)) { if (!rc) rc = fail(h, DOD_ERR_HIP, "cast launch failed"); return nullptr; }
    return b;
  }
  // One block linear in the precision's operand format: H2 rows + exponent bytes (fp16x2), pair layout (bf16x3), e4m3 (fp8; fp8_ok false:
  // GELU-MLP fc2 stays bf16), else bf16 / fp32.
  // fp8 mode, round 4: BOTH operands of every fp8 linear block-scaled (one e8m0 byte per 32 elements along K; the per-row / per-feature fp32
  // scales of rounds 1-3 remain for widths that are not multiples of 256): on the reference's G8 golden the per-row form sat at 96.3 % top-1
  // agreement / 1.6e-1 logits rel-L2, the block-scaled form at 99.3 % / 1.4e-1
  PackedLinear pack_linear(const float* src, int rows, int cols, float* bias, const float* csum = nullptr, bool fp8_ok = true) {
    const dod_config& c = h->cfg;
    PackedLinear p; p.bias = bias; p.csum = csum;
    if (is_h2(h)) {            // H2 weight rows (3 bytes per element: fp16 | e4m3 remainder) + the rows' exponent bytes (dod_common.h)
      if (!src || cols % 32) return p;
      unsigned char* b = alloc<unsigned char>((size_t)rows * 3 * cols); unsigned char* ex = alloc<unsigned char>((size_t)rows);
      if (!b || !ex) return p;
      if (launch_split_h2(src, cols, b, rows, cols, ex, s)) { if (!rc) rc = fail(h, DOD_ERR_HIP, "split_h2 launch failed"); return p; }
      p.W = b; p.wexp = ex;
    } else if (is_x3(h)) p.W = pair_w(src, rows, cols);
    else if (is_fp8(h) && fp8_ok) {
      if (!src) return p;
      unsigned char* q = alloc<unsigned char>((size_t)rows * cols);
      if (c.hidden % 256 == 0 && (!c.swiglu || c.ffn_hidden % 256 == 0)) {   // e4m3 rows + one e8m0 byte per 32 columns (the activations' layout: quant_mx_fp8_kernel)
        unsigned char* bs = alloc<unsigned char>((size_t)rows * (cols >> 5));
        if (!q || !bs) return p;
        if (launch_quant_mx_fp8(src, 0, cols, rows, cols, q, cols, bs, s)) { if (!rc) rc = fail(h, DOD_ERR_HIP, "fp8 block-scaled weight quantisation launch failed"); return p; }
        p.W = q; p.wbs = bs;
      } else {                                                               // e4m3 rows + per-row (output feature) scales
        float* sc = alloc<float>(rows);
        if (!q || !sc) return p;
        if (launch_quant_rows_fp8(src, 0, cols, rows, cols, q, cols, sc, s)) { if (!rc) rc = fail(h, DOD_ERR_HIP, "fp8 weight quantisation launch failed"); return p; }
        p.W = q; p.wscale = sc;
      }
    } else p.W = pack_operand(src, rows, cols, cols);
    return p;
  }
  // norm folded into the linear behind it: W' = W diag(gamma) as a temporary fp32 copy, bias <- bias + W beta in place
  float* fold_ln(const float* w, int rows, const float* gamma, const float* beta, float* bias) {
    const int D = h->cfg.hidden;
    float* wf = alloc<float>((size_t)rows * D, true);
    if (!w || !wf || !gamma || !beta || !bias) return nullptr;
    if (launch_ln_fold(w, rows, D, gamma, beta, bias, wf, bias, s)) { if (!rc) rc = fail(h, DOD_ERR_HIP, "LayerNorm fold launch failed"); return nullptr; }
    return wf;
  }
  // c = row sums of what the MFMAs multiply
  float* col_sums(const float* wf, int rows) {
    float* cs = alloc<float>((size_t)rows);
    if (!wf || !cs) return nullptr;
    if (launch_rowsum(wf, rows, h->cfg.hidden, (is_bf16(h) && !is_x3(h)) ? 1 : 0, cs, s)) { if (!rc) rc = fail(h, DOD_ERR_HIP, "row sum launch failed"); return nullptr; }
    return cs;
  }
};

// bf16 tensors (dod_set_weight dtype DOD_BF16): widen once per distinct storage so that tied parameters stay tied
int widen_bf16_weights(Packer& P) {
  dod_handle* h = P.h;
  std::map<const void*, float*> widened;
  for (auto& kv : h->w) {
    WRef& r = kv.second;
    if (r.dtype == DOD_F32) { r.ptr = (const float*)r.raw; continue; }
    auto it = widened.find(r.raw);
    if (it == widened.end()) {
      float* f = P.alloc<float>(r.numel(), true);
      if (!f || launch_widen_bf16((const bf16_t*)r.raw, f, r.numel(), P.s)) return P.rc ? P.rc : fail(h, DOD_ERR_HIP, "widening of a bf16 weight failed");
      it = widened.emplace(r.raw, f).first;
    }
    r.ptr = it->second;
  }
  return DOD_OK;
}

int pack_backbone(Packer& P) {
  dod_handle* h = P.h; hipStream_t s = P.s;
  const dod_config& c = h->cfg;
  const int D = c.hidden, F = c.ffn_hidden, G = c.pos_grid, p = c.patch;
  const std::string bb = "backbone.dino.", e = bb + "embeddings.";
  // ---- embeddings
  h->cls = P.copy(e + "cls_token", {1, 1, D});
  h->pos = P.copy(e + "position_embeddings", {1, (int64_t)G * G + 1, D});
  h->bpatch = P.copy(e + "patch_embeddings.projection.bias", {D});
  {
    const WRef* W = P.need(e + "patch_embeddings.projection.weight", {D, 3, p, p});
    const int K = 3 * p * p;
    h->Kp = is_bf16(h) ? (K + 63) / 64 * 64 : K;
    if (W) h->Wpatch = P.pack_operand(W->ptr, D, K, h->Kp);
    h->Wpe = nullptr;
    if (W && (is_bf16(h) || is_x3(h)) && (p == 14 || p == 16) && D % 4 == 0 && dod_option(DOD_OPT_NO_FUSED_PATCH) <= 0) {
      bf16_t* wp = P.alloc<bf16_t>((size_t)D * 3 * (p / 2) * 32 * (is_x3(h) ? 2 : 1));
      if (wp && !launch_patch_pack(W->ptr, D, p, wp, is_x3(h) ? 1 : 0, s)) h->Wpe = wp;
    }
    if (W && is_x3(h)) {
      h->Kp2 = (K + 31) / 32 * 32;
      float* padded = P.alloc<float>((size_t)D * h->Kp2, true);
      if (padded && !launch_copy2d(W->ptr, K, padded, h->Kp2, D, K, h->Kp2, s)) h->Wpatch2 = P.pair_w(padded, D, h->Kp2);
    }
  }
  // ---- encoder blocks
  // norm1 / norm2 folded into the QKV / MLP-in GEMMs (ln_foldable): W' = W diag(gamma), b' = b + W beta, c = row sums of what the MFMAs
  // multiply.  DINODET_LN_FOLD=0 (or the test option): the round-3 schedule.
  static const bool fold_env = [] { const char* v = getenv("DINODET_LN_FOLD"); return !(v && v[0] == '0'); }();
  const int fold_opt = dod_option(DOD_OPT_LN_FOLD);
  const bool fold = (fold_opt >= 0 ? fold_opt != 0 : fold_env) && ln_foldable(h);
  h->L.resize(c.layers);
  for (int i = 0; i < c.layers && !P.rc; ++i) {
    BLayer& L = h->L[i];
    const std::string lp = bb + "encoder.layer." + std::to_string(i) + ".";
    L.ln1w = P.copy(lp + "norm1.weight", {D}); L.ln1b = P.copy(lp + "norm1.bias", {D});
    L.ln2w = P.copy(lp + "norm2.weight", {D}); L.ln2b = P.copy(lp + "norm2.bias", {D});
    L.ls1 = P.copy(lp + "layer_scale1.lambda1", {D}); L.ls2 = P.copy(lp + "layer_scale2.lambda1", {D});
    L.fold = fold;
    // fused QKV: rows [q | k | v]
    float* cat = P.alloc<float>((size_t)3 * D * D, true);
    float* bqkv = P.alloc<float>((size_t)3 * D);
    const char* names[3] = {"query", "key", "value"};
    for (int t = 0; t < 3 && !P.rc; ++t) {
      const std::string q = lp + "attention.attention." + names[t];
      const float* w = P.eff_weight(q, D, D);
      float* b = P.eff_bias(q, D);
      if (!w || !b || !cat || !bqkv) break;
      HIPCHK(h, hipMemcpyAsync(cat + (size_t)t * D * D, w, (size_t)D * D * 4, hipMemcpyDeviceToDevice, s));
      HIPCHK(h, hipMemcpyAsync(bqkv + (size_t)t * D, b, (size_t)D * 4, hipMemcpyDeviceToDevice, s));
    }
    if (P.rc) break;
    float* cqkv = nullptr;
    if (fold) {
      float* cf = P.fold_ln(cat, 3 * D, L.ln1w, L.ln1b, bqkv);
      if (cf) { cat = cf; cqkv = P.col_sums(cat, 3 * D); }
      if (!cf || !cqkv) { if (!P.rc) P.rc = fail(h, DOD_ERR_HIP, "LayerNorm fold failed"); break; }
    }
    L.qkv = P.pack_linear(cat, 3 * D, D, bqkv, cqkv);
    const float* wo = P.eff_weight(lp + "attention.output.dense", D, D);
    L.o = P.pack_linear(wo, D, D, nullptr);
    L.o.bias = P.eff_bias(lp + "attention.output.dense", D);
    float* c1 = nullptr;
    if (c.swiglu) {
      const float* w_in = P.eff_weight(lp + "mlp.weights_in", 2 * F, D);
      float* b1 = P.eff_bias(lp + "mlp.weights_in", 2 * F);
      // bf16 / fp8 operands: hidden = silu(x1) * x2 (modeling_dinov2.py:310-314) is evaluated in the weights_in GEMM's epilogue
      // (GemmEpi::glu) on interleaved column pairs -- rows of the weight and the bias re-ordered once here (x1_i, x2_i adjacent; the
      // fp8 per-feature scales are computed on the re-ordered rows).  The strict fp32 mode keeps the separate gate kernel.
      static const bool glu_off = DOD_TUNE_ENV("DINODET_NO_FUSED_GLU") != nullptr;
      // (round 3b: the compensated modes too -- their gate was three passes over fp32 [M, 2F] / [M, F] buffers: 4.9 GB per ViT-g block at 32
      // images; the epilogue now writes the pair / H2 operand rows of weights_out directly.  H2 rows need F % 32 == 0 and whole quads.)
      const bool glu_ok = is_x3(h) ? (F % 32 == 0) : is_bf16(h);
      if (fold) w_in = P.fold_ln(w_in, 2 * F, L.ln2w, L.ln2b, b1);
      if (w_in && b1 && glu_ok && !glu_off) {
        float* wi = P.alloc<float>((size_t)2 * F * D, true);
        float* bi = P.alloc<float>((size_t)2 * F);
        if (wi && bi && !launch_interleave_halves(w_in, wi, F, D, s) && !launch_interleave_halves(b1, bi, F, 1, s)) { w_in = wi; b1 = bi; L.glu = true; }
      }
      if (fold) c1 = P.col_sums(w_in, 2 * F);
      L.fc1 = P.pack_linear(w_in, 2 * F, D, b1, c1);
      L.fc2 = P.pack_linear(P.eff_weight(lp + "mlp.weights_out", D, F), D, F, nullptr);
      L.fc2.bias = P.eff_bias(lp + "mlp.weights_out", D);
    } else {
      const float* w1 = P.eff_weight(lp + "mlp.fc1", F, D);
      float* b1 = P.eff_bias(lp + "mlp.fc1", F);
      if (fold) { w1 = P.fold_ln(w1, F, L.ln2w, L.ln2b, b1); c1 = P.col_sums(w1, F); }
      L.fc1 = P.pack_linear(w1, F, D, b1, c1);
      L.fc2 = P.pack_linear(P.eff_weight(lp + "mlp.fc2", D, F), D, F, nullptr, nullptr, false);
      L.fc2.bias = P.eff_bias(lp + "mlp.fc2", D);
    }
  }
  if (!P.rc) for (auto& L : h->L) if (L.fold && (!L.qkv.csum || !L.fc1.csum || !L.fc1.W)) { P.rc = fail(h, DOD_ERR_HIP, "LayerNorm fold failed"); break; }
  if (P.rc) return P.rc;
  h->lnfw = P.copy(bb + "layernorm.weight", {D}); h->lnfb = P.copy(bb + "layernorm.bias", {D});
  if (c.target_dim) {
    const WRef* W = P.need("backbone.projection.weight", {c.target_dim, D});
    if (W) h->Wproj = is_x3(h) ? (void*)P.pair_w(W->ptr, c.target_dim, D) : P.pack_operand(W->ptr, c.target_dim, D, D);
    h->bproj = P.copy("backbone.projection.bias", {c.target_dim});
  }
  return DOD_OK;
}

// decoder (fp32 except the memory-side projections in bf16 mode)
int pack_decoder(Packer& P) {
  dod_handle* h = P.h; hipStream_t s = P.s;
  const dod_config& c = h->cfg;
  const int Dd = c.dec_hidden, Q = c.num_queries, Hd = c.dec_heads, Pn = c.n_points, Fd = c.dim_feedforward, C = c.num_classes;
  const std::string dp = "decoder.";
  h->query = P.copy(dp + "query_embed.weight", {Q, Dd});
  h->cls_w = P.copy(dp + "class_embed.weight", {C, Dd}); h->cls_b = P.copy(dp + "class_embed.bias", {C});
  h->bb0_w = P.copy(dp + "bbox_embed.mlp.0.weight", {Dd / 2, Dd}); h->bb0_b = P.copy(dp + "bbox_embed.mlp.0.bias", {Dd / 2});
  h->bb0_w3 = P.split_w(h->bb0_w, Dd / 2, Dd);
  h->bb2_w = P.copy(dp + "bbox_embed.mlp.2.weight", {4, Dd / 2}); h->bb2_b = P.copy(dp + "bbox_embed.mlp.2.bias", {4});
  h->ncat = 2 + 3 * Hd * Pn;
  h->DL.resize(c.dec_layers);
  for (int j = 0; j < c.dec_layers && !P.rc; ++j) {
    DLayer& L = h->DL[j];
    const std::string lp = dp + "decoder.layers." + std::to_string(j) + ".";
    L.in_w = P.copy(lp + "self_attn.in_proj_weight", {3 * Dd, Dd}); L.in_b = P.copy(lp + "self_attn.in_proj_bias", {3 * Dd});
    L.out_w = P.copy(lp + "self_attn.out_proj.weight", {Dd, Dd}); L.out_b = P.copy(lp + "self_attn.out_proj.bias", {Dd});
    L.n1w = P.copy(lp + "norm1.weight", {Dd}); L.n1b = P.copy(lp + "norm1.bias", {Dd});
    L.n2w = P.copy(lp + "norm2.weight", {Dd}); L.n2b = P.copy(lp + "norm2.bias", {Dd});
    L.n3w = P.copy(lp + "norm3.weight", {Dd}); L.n3b = P.copy(lp + "norm3.bias", {Dd});
    L.l1w = P.copy(lp + "linear1.weight", {Fd, Dd}); L.l1b = P.copy(lp + "linear1.bias", {Fd});
    L.l2w = P.copy(lp + "linear2.weight", {Dd, Fd}); L.l2b = P.copy(lp + "linear2.bias", {Dd});
    L.in_w3 = P.split_w(L.in_w, 3 * Dd, Dd); L.out_w3 = P.split_w(L.out_w, Dd, Dd);
    L.l1w3 = P.split_w(L.l1w, Fd, Dd); L.l2w3 = P.split_w(L.l2w, Dd, Fd);
    if (c.use_deformable) {
      // one fused small linear: [reference_points_proj (2) | sampling_offsets (Hd*P*2) | attention_weights (Hd*P)]
      const WRef* rw = P.need(lp + "reference_points_proj.weight", {2, Dd});
      const WRef* rb = P.need(lp + "reference_points_proj.bias", {2});
      const WRef* ow = P.need(lp + "cross_attn.sampling_offsets.weight", {(int64_t)Hd * Pn * 2, Dd});
      const WRef* ob = P.need(lp + "cross_attn.sampling_offsets.bias", {(int64_t)Hd * Pn * 2});
      const WRef* aw = P.need(lp + "cross_attn.attention_weights.weight", {(int64_t)Hd * Pn, Dd});
      const WRef* ab = P.need(lp + "cross_attn.attention_weights.bias", {(int64_t)Hd * Pn});
      L.cat_w = P.alloc<float>((size_t)h->ncat * Dd); L.cat_b = P.alloc<float>(h->ncat);
      if (P.rc || !rw || !rb || !ow || !ob || !aw || !ab || !L.cat_w || !L.cat_b) break;
      HIPCHK(h, hipMemcpyAsync(L.cat_w, rw->ptr, (size_t)2 * Dd * 4, hipMemcpyDeviceToDevice, s));
      HIPCHK(h, hipMemcpyAsync(L.cat_w + (size_t)2 * Dd, ow->ptr, (size_t)Hd * Pn * 2 * Dd * 4, hipMemcpyDeviceToDevice, s));
      HIPCHK(h, hipMemcpyAsync(L.cat_w + (size_t)(2 + Hd * Pn * 2) * Dd, aw->ptr, (size_t)Hd * Pn * Dd * 4, hipMemcpyDeviceToDevice, s));
      HIPCHK(h, hipMemcpyAsync(L.cat_b, rb->ptr, 2 * 4, hipMemcpyDeviceToDevice, s));
      HIPCHK(h, hipMemcpyAsync(L.cat_b + 2, ob->ptr, (size_t)Hd * Pn * 2 * 4, hipMemcpyDeviceToDevice, s));
      HIPCHK(h, hipMemcpyAsync(L.cat_b + 2 + Hd * Pn * 2, ab->ptr, (size_t)Hd * Pn * 4, hipMemcpyDeviceToDevice, s));
      L.op_w = P.copy(lp + "cross_attn.output_proj.weight", {Dd, Dd}); L.op_b = P.copy(lp + "cross_attn.output_proj.bias", {Dd});
      L.op_w3 = P.split_w(L.op_w, Dd, Dd);
      // value projection: layers are weight-tied in the reference (deformable_attention.py:284): when the
      // caller registered the same storage for several layers the projection is computed once per forward
      const WRef* vw = P.need(lp + "cross_attn.value_proj.weight", {Dd, Dd});
      const WRef* vb = P.need(lp + "cross_attn.value_proj.bias", {Dd});
      if (!vw || !vb) break;
      for (int k = 0; k < j; ++k) {
        const std::string kp = dp + "decoder.layers." + std::to_string(k) + ".";
        if (h->w[kp + "cross_attn.value_proj.weight"].ptr == vw->ptr && h->w[kp + "cross_attn.value_proj.bias"].ptr == vb->ptr) { L.vp_alias = h->DL[k].vp_alias >= 0 ? h->DL[k].vp_alias : k; break; }
      }
      if (L.vp_alias < 0) {
        L.vp_w = P.pack_operand(vw->ptr, Dd, Dd, Dd); L.vp_b = P.copy(lp + "cross_attn.value_proj.bias", {Dd});
        if (is_x3(h)) L.vp_w2 = P.pair_w(vw->ptr, Dd, Dd);
      }
    } else {
      const WRef* iw = P.need(lp + "multihead_attn.in_proj_weight", {3 * Dd, Dd});
      const WRef* ib = P.need(lp + "multihead_attn.in_proj_bias", {3 * Dd});
      if (!iw || !ib) break;
      L.ca_q_w = (float*)P.pack_operand(iw->ptr, Dd, Dd, Dd, true);
      L.ca_kv_w = P.pack_operand(iw->ptr + (size_t)Dd * Dd, 2 * Dd, Dd, Dd);
      if (is_x3(h)) L.ca_kv_w2 = P.pair_w(iw->ptr + (size_t)Dd * Dd, 2 * Dd, Dd);
      L.ca_q_b = P.alloc<float>(Dd); L.ca_kv_b = P.alloc<float>(2 * Dd);
      if (P.rc) break;
      HIPCHK(h, hipMemcpyAsync(L.ca_q_b, ib->ptr, (size_t)Dd * 4, hipMemcpyDeviceToDevice, s));
      HIPCHK(h, hipMemcpyAsync(L.ca_kv_b, ib->ptr + Dd, (size_t)2 * Dd * 4, hipMemcpyDeviceToDevice, s));
      L.ca_out_w = P.copy(lp + "multihead_attn.out_proj.weight", {Dd, Dd}); L.ca_out_b = P.copy(lp + "multihead_attn.out_proj.bias", {Dd});
      L.ca_q_w3 = P.split_w(L.ca_q_w, Dd, Dd); L.ca_out_w3 = P.split_w(L.ca_out_w, Dd, Dd);
    }
  }
  return DOD_OK;
}

}  // namespace

// bf16 -> fp32 widening (bf16 weights, debug taps)
__global__ void widen_bf16_kernel(const bf16_t* __restrict__ in, float* __restrict__ out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = bf2f(in[i]);
}
int dod::launch_widen_bf16(const bf16_t* in, float* out, size_t n, hipStream_t s) {
  const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(widen_bf16_kernel, dim3(blocks), dim3(256), 0, s, in, out, n);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

int dod::finalize_impl(dod_handle* h, hipStream_t s) {
  for (void* p : h->owned) (void)hipFree(p);
  h->owned.clear(); h->L.clear(); h->DL.clear(); h->finalized = false;
  h->pos_H = h->pos_W = -1; h->pos_hw = nullptr; h->pos_cache.clear();
  Packer P(h, s);
  int rc = widen_bf16_weights(P); if (rc) return rc;
  h->has_bb = h->has_dec = false;
  for (auto& kv : h->w) {
    if (kv.first.rfind("backbone.", 0) == 0) h->has_bb = true;
    if (kv.first.rfind("decoder.", 0) == 0) h->has_dec = true;
  }
  if (!h->has_bb && !h->has_dec) return fail(h, DOD_ERR_MISSING, "no 'backbone.*' or 'decoder.*' weights were registered");
  if (h->has_bb) { rc = pack_backbone(P); if (rc) return rc; }
  if (h->has_dec) { rc = pack_decoder(P); if (rc) return rc; }
  hipError_t se = hipStreamSynchronize(s);
  if (P.rc) return P.rc;
  if (se != hipSuccess) return fail(h, DOD_ERR_HIP, "finalize: %s", hipGetErrorString(se));
  h->finalized = true;
  return DOD_OK;
}

// ----------------------------------------------------------------------------- read-only views of what finalize stored (dod_test_packed_*)
namespace {

// arrays of one packed operand in the order of enum dod_packed_array
struct PackedView {
  const void* p[DOD_PK_ARRAYS] = {};
  size_t bytes[DOD_PK_ARRAYS] = {};
  int format = DOD_PK_ABSENT, rows = 0, cols = 0;
  size_t pitch = 0;
  int glu = 0, fold = 0, vp_alias = -1;
};

void view_plain(PackedView& v, const void* p, int format, int rows, int cols, int cols_pad = 0) {
  if (!p) return;
  const int cp = cols_pad ? cols_pad : cols;
  const size_t per = format == DOD_PK_F32 ? 4 : format == DOD_PK_BF16 ? 2 : format == DOD_PK_PAIR ? 4 : format == DOD_PK_SPLIT3W ? 6 : 1;
  v.format = format; v.rows = rows; v.cols = cols; v.pitch = per * cp;
  v.p[DOD_PK_W] = p; v.bytes[DOD_PK_W] = (size_t)rows * v.pitch;
}

void view_linear(const dod_handle* h, PackedView& v, const PackedLinear& L, int rows, int cols) {
  if (L.W) {
    const int format = L.wexp ? DOD_PK_H2W : L.wbs ? DOD_PK_E4M3_MX : L.wscale ? DOD_PK_E4M3_ROWS : is_x3(h) ? DOD_PK_PAIR : is_bf16(h) ? DOD_PK_BF16 : DOD_PK_F32;
    if (format == DOD_PK_H2W) { v.format = format; v.rows = rows; v.cols = cols; v.pitch = (size_t)3 * cols; v.p[DOD_PK_W] = L.W; v.bytes[DOD_PK_W] = (size_t)rows * v.pitch; }
    else view_plain(v, L.W, format, rows, cols);
  } else { v.rows = rows; v.cols = cols; }
  if (L.bias) { v.p[DOD_PK_BIAS] = L.bias; v.bytes[DOD_PK_BIAS] = (size_t)rows * 4; }
  if (L.csum) { v.p[DOD_PK_CSUM] = L.csum; v.bytes[DOD_PK_CSUM] = (size_t)rows * 4; }
  if (L.wscale) { v.p[DOD_PK_WSCALE] = L.wscale; v.bytes[DOD_PK_WSCALE] = (size_t)rows * 4; }
  if (L.wbs) { v.p[DOD_PK_WBS] = L.wbs; v.bytes[DOD_PK_WBS] = (size_t)rows * (cols >> 5); }
  if (L.wexp) { v.p[DOD_PK_WEXP] = L.wexp; v.bytes[DOD_PK_WEXP] = (size_t)rows; }
}

// "<prefix>.<index>.<field>" -> index and field; false when name has another form
bool indexed(const char* name, const char* prefix, int* idx, const char** field) {
  const size_t n = strlen(prefix);
  if (strncmp(name, prefix, n) || name[n] != '.') return false;
  char* end = nullptr;
  const long i = strtol(name + n + 1, &end, 10);
  if (end == name + n + 1 || *end != '.' || i < 0 || i > 1 << 20) return false;
  *idx = (int)i; *field = end + 1;
  return true;
}

// false: no operand of that name exists in any configuration
bool packed_view(const dod_handle* h, const char* name, PackedView& v) {
  const dod_config& c = h->cfg;
  const int D = c.hidden, F = c.ffn_hidden, p = c.patch, Dd = c.dec_hidden, Q = c.num_queries, Fd = c.dim_feedforward;
  const int wfmt = is_bf16(h) ? DOD_PK_BF16 : DOD_PK_F32;     // operand dtype outside the block linears
  auto is = [&](const char* s) { return !strcmp(name, s); };
  struct Plain { const char* name; const void* p; int format, rows, cols, cols_pad; };
  int i = 0; const char* f = nullptr;
  if (indexed(name, "block", &i, &f)) {
    if (i >= (int)h->L.size()) return false;
    const BLayer& L = h->L[i];
    v.glu = L.glu; v.fold = L.fold;
    const int F1 = c.swiglu ? 2 * F : F;
    if (!strcmp(f, "qkv")) { view_linear(h, v, L.qkv, 3 * D, D); return true; }
    if (!strcmp(f, "o")) { view_linear(h, v, L.o, D, D); return true; }
    if (!strcmp(f, "fc1")) { view_linear(h, v, L.fc1, F1, D); return true; }
    if (!strcmp(f, "fc2")) { view_linear(h, v, L.fc2, D, F); return true; }
    const Plain t[] = {{"ln1w", L.ln1w, DOD_PK_F32, 1, D, 0}, {"ln1b", L.ln1b, DOD_PK_F32, 1, D, 0}, {"ln2w", L.ln2w, DOD_PK_F32, 1, D, 0},
                       {"ln2b", L.ln2b, DOD_PK_F32, 1, D, 0}, {"ls1", L.ls1, DOD_PK_F32, 1, D, 0}, {"ls2", L.ls2, DOD_PK_F32, 1, D, 0}};
    for (const Plain& e : t) if (!strcmp(f, e.name)) { view_plain(v, e.p, e.format, e.rows, e.cols, e.cols_pad); return true; }
    return false;
  }
  if (indexed(name, "dec", &i, &f)) {
    if (i >= (int)h->DL.size()) return false;
    const DLayer& L = h->DL[i];
    v.vp_alias = L.vp_alias;
    const int S3 = DOD_PK_SPLIT3W, F32 = DOD_PK_F32, nc = h->ncat;
    const Plain t[] = {
      {"in_w", L.in_w, F32, 3 * Dd, Dd, 0}, {"in_b", L.in_b, F32, 1, 3 * Dd, 0}, {"out_w", L.out_w, F32, Dd, Dd, 0}, {"out_b", L.out_b, F32, 1, Dd, 0},
      {"n1w", L.n1w, F32, 1, Dd, 0}, {"n1b", L.n1b, F32, 1, Dd, 0}, {"n2w", L.n2w, F32, 1, Dd, 0}, {"n2b", L.n2b, F32, 1, Dd, 0},
      {"n3w", L.n3w, F32, 1, Dd, 0}, {"n3b", L.n3b, F32, 1, Dd, 0},
      {"l1w", L.l1w, F32, Fd, Dd, 0}, {"l1b", L.l1b, F32, 1, Fd, 0}, {"l2w", L.l2w, F32, Dd, Fd, 0}, {"l2b", L.l2b, F32, 1, Dd, 0},
      {"in_w3", L.in_w3, S3, 3 * Dd, Dd, 0}, {"out_w3", L.out_w3, S3, Dd, Dd, 0}, {"l1w3", L.l1w3, S3, Fd, Dd, 0}, {"l2w3", L.l2w3, S3, Dd, Fd, 0},
      {"op_w3", L.op_w3, S3, Dd, Dd, 0}, {"ca_q_w3", L.ca_q_w3, S3, Dd, Dd, 0}, {"ca_out_w3", L.ca_out_w3, S3, Dd, Dd, 0},
      {"cat_w", L.cat_w, F32, nc, Dd, 0}, {"cat_b", L.cat_b, F32, 1, nc, 0}, {"op_w", L.op_w, F32, Dd, Dd, 0}, {"op_b", L.op_b, F32, 1, Dd, 0},
      {"vp_w", L.vp_w, wfmt, Dd, Dd, 0}, {"vp_w2", L.vp_w2, DOD_PK_PAIR, Dd, Dd, 0}, {"vp_b", L.vp_b, F32, 1, Dd, 0},
      {"ca_q_w", L.ca_q_w, F32, Dd, Dd, 0}, {"ca_q_b", L.ca_q_b, F32, 1, Dd, 0}, {"ca_kv_w", L.ca_kv_w, wfmt, 2 * Dd, Dd, 0},
      {"ca_kv_w2", L.ca_kv_w2, DOD_PK_PAIR, 2 * Dd, Dd, 0}, {"ca_kv_b", L.ca_kv_b, F32, 1, 2 * Dd, 0},
      {"ca_out_w", L.ca_out_w, F32, Dd, Dd, 0}, {"ca_out_b", L.ca_out_b, F32, 1, Dd, 0}};
    for (const Plain& e : t) if (!strcmp(f, e.name)) { view_plain(v, e.p, e.format, e.rows, e.cols, e.cols_pad); return true; }
    return false;
  }
  const int K = 3 * p * p, kpe = 3 * (p / 2) * 32, G = c.pos_grid;
  const Plain t[] = {
    {"Wpatch", h->Wpatch, wfmt, D, K, h->Kp}, {"Wpatch2", h->Wpatch2, DOD_PK_PAIR, D, K, h->Kp2}, {"Wpe", h->Wpe, is_x3(h) ? DOD_PK_PAIR : DOD_PK_BF16, D, kpe, 0},
    {"bpatch", h->bpatch, DOD_PK_F32, 1, D, 0}, {"cls", h->cls, DOD_PK_F32, 1, D, 0}, {"pos", h->pos, DOD_PK_F32, G * G + 1, D, 0},
    {"lnfw", h->lnfw, DOD_PK_F32, 1, D, 0}, {"lnfb", h->lnfb, DOD_PK_F32, 1, D, 0},
    {"Wproj", h->Wproj, is_x3(h) ? DOD_PK_PAIR : wfmt, c.target_dim, D, 0}, {"bproj", h->bproj, DOD_PK_F32, 1, c.target_dim, 0},
    {"query", h->query, DOD_PK_F32, Q, Dd, 0}, {"cls_w", h->cls_w, DOD_PK_F32, c.num_classes, Dd, 0}, {"cls_b", h->cls_b, DOD_PK_F32, 1, c.num_classes, 0},
    {"bb0_w", h->bb0_w, DOD_PK_F32, Dd / 2, Dd, 0}, {"bb0_b", h->bb0_b, DOD_PK_F32, 1, Dd / 2, 0}, {"bb0_w3", h->bb0_w3, DOD_PK_SPLIT3W, Dd / 2, Dd, 0},
    {"bb2_w", h->bb2_w, DOD_PK_F32, 4, Dd / 2, 0}, {"bb2_b", h->bb2_b, DOD_PK_F32, 1, 4, 0},
    {"l0_tgt", h->l0_tgt, DOD_PK_F32, Q, Dd, 0}, {"l0_proj", h->l0_proj, DOD_PK_F32, Q, h->ncat, 0}};
  for (const Plain& e : t) if (is(e.name)) { view_plain(v, e.p, e.format, e.rows, e.cols, e.cols_pad); return true; }
  return false;
}

int packed_lookup(const dod_handle* h, const char* name, PackedView& v, const char* who) {
  if (!h) return fail(nullptr, DOD_ERR_INVALID, "%s: null handle", who);
  if (!name) return fail(h, DOD_ERR_INVALID, "%s: null name", who);
  if (!h->finalized) return fail(h, DOD_ERR_STATE, "%s: dod_finalize_weights has not been called", who);
  if (!packed_view(h, name, v)) return fail(h, DOD_ERR_INVALID, "%s: no packed operand named '%s'", who, name);
  return DOD_OK;
}

}  // namespace

extern "C" {

int dod_test_packed_info(const dod_handle* h, const char* name, dod_packed_info* info) {
  PackedView v;
  const int rc = packed_lookup(h, name, v, "dod_test_packed_info"); if (rc) return rc;
  if (!info) return fail(h, DOD_ERR_INVALID, "dod_test_packed_info: null info");
  info->format = v.format; info->rows = v.rows; info->cols = v.cols; info->pitch = (int64_t)v.pitch;
  info->glu = v.glu; info->fold = v.fold; info->vp_alias = v.vp_alias; info->reserved = 0; info->arrays = 0;
  for (int a = 0; a < DOD_PK_ARRAYS; ++a) { info->bytes[a] = (int64_t)v.bytes[a]; if (v.p[a]) info->arrays |= 1 << a; }
  return DOD_OK;
}

int dod_test_packed_copy(const dod_handle* h, const char* name, int array, void* dst, size_t dst_bytes, void* stream) {
  PackedView v;
  const int rc = packed_lookup(h, name, v, "dod_test_packed_copy"); if (rc) return rc;
  if (array < 0 || array >= DOD_PK_ARRAYS) return fail(h, DOD_ERR_INVALID, "dod_test_packed_copy: array %d is not a dod_packed_array", array);
  if (!dst) return fail(h, DOD_ERR_INVALID, "dod_test_packed_copy: null destination");
  if (!v.p[array]) return fail(h, DOD_ERR_INVALID, "dod_test_packed_copy: '%s' has no array %d in this configuration", name, array);
  if (dst_bytes < v.bytes[array]) return fail(h, DOD_ERR_INVALID, "dod_test_packed_copy: '%s' array %d holds %zu bytes, the destination %zu", name, array, v.bytes[array], dst_bytes);
  HIPCHK(h, hipMemcpyAsync(dst, v.p[array], v.bytes[array], hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return DOD_OK;
}

}  // extern "C"
