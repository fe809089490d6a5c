// Backbone tail: the LoRA-adapted encoder blocks (dinov2_backbone.py:45-51: the last two), the final LayerNorm and the projection
// (dinov2_backbone.py:33-37, 64-65) in train() mode -- the rest of what `loss.backward()` (train.py:1101) reaches: gradients of every
// lora_A / lora_B (utils.py:46-70) and of the projection.  The DINOv2 weights, LayerNorms, LayerScales and biases are frozen
// (dinov2_backbone.py:40-41), and so is everything in front of the first adapted block (it runs in the inference kernels,
// dod_backbone_prefix): the backward stops at the tail's input.  GELU MLP (ViT-S/B/L) or SwiGLU (ViT-g: modeling_dinov2.py:300-314; the
// fc1 / fc2 slots of dod_bb_block_params then hold mlp.weights_in [2F, D] / mlp.weights_out [D, F]).
//   forward : x -> LN1 -> q|k|v (W' = W + alpha B A, merged in fp32 as the eval path does) -> softmax(q k^T / sqrt(dh)) v -> dense
//             -> x + ls1 * . -> LN2 -> fc1 -> GELU(erf) -> fc2 -> + ls2 * .  ->  final LN -> projection
//   backward: dX = dY W' on the fp32 MFMA GEMM (the bf16 split GEMM under DOD_PREC_BF16X3, like every linear here: train_internal.h Mm); per LoRA linear  dB += alpha dY^T (X A^T),  dA += alpha (dY B)^T X  (rank-r GEMMs);
//             attention backward = the row / column passes of the decoder's self-attention with Q := N tokens.
// Schedule only: the kernels and their launchers are in train_ops.hip, attn_f32m.hip and gemm_f32.hip.
#include "train_internal.h"

using namespace dtrain;

namespace {

struct TDims { int B, N, M, D, H, dh, F, F1, Dd, nb, r, swiglu; float alpha, eps; };   // F1: width of the first MLP linear (2F for SwiGLU)
bool make_tdims(const dod_config* c, int B, int N, int nblocks, TDims* d) {
  if (!c || B <= 0 || N <= 0 || nblocks <= 0 || nblocks > 8) return false;
  d->B = B; d->N = N; d->M = B * N; d->D = c->hidden; d->H = c->heads; d->dh = d->D / d->H; d->F = c->ffn_hidden;
  d->swiglu = c->swiglu ? 1 : 0; d->F1 = c->swiglu ? 2 * c->ffn_hidden : c->ffn_hidden;
  d->Dd = c->target_dim ? c->target_dim : c->hidden; d->nb = nblocks; d->r = c->lora_r; d->alpha = c->lora_alpha; d->eps = c->ln_eps;
  if (d->D % d->H || d->dh > 128 || d->dh % 4 || d->D % 4 || d->F % 4 || d->D > 2048 || N > MHA_MAXQ || d->r < 1 || d->r > 64) return false;   // D: ln_bwd / launch_layernorm
  return true;
}
struct TTape {
  float* xout; float* f;
  struct Blk { float *x, *y1, *qkv, *ctx, *x1, *y2, *pre, *h, *Wqkv, *Wo, *W1, *W2, *bqkv, *lse; } b[8];
};
size_t carve_ttape(const TDims& d, const void* base, TTape& tt) {
  dod::Carver c = carver(base);
  const size_t M = d.M, D = d.D, F = d.F;
  tt.xout = takef(c, M * D); tt.f = takef(c, M * D);
  for (int i = 0; i < d.nb; ++i) {
    auto& b = tt.b[i];
    b.x = takef(c, M * D); b.y1 = takef(c, M * D); b.qkv = takef(c, M * 3 * D); b.ctx = takef(c, M * D); b.x1 = takef(c, M * D); b.y2 = takef(c, M * D);
    b.pre = takef(c, M * (size_t)d.F1); b.h = takef(c, M * F);
    b.Wqkv = takef(c, 3 * D * D); b.Wo = takef(c, D * D); b.W1 = takef(c, (size_t)d.F1 * D); b.W2 = takef(c, D * F); b.bqkv = takef(c, 3 * D);
    b.lse = takef(c, 2 * M * (size_t)d.H);             // (max, sum) of every score row [B, H, N, 2]: the flash-style attention adjoint
  }
  return c.off;
}
struct TScratch { float *dx, *da, *db, *dbig, *dqkv, *dS, *Pd, *T, *U, *dump, *dh, *delta; };
// head_dim 64 (every DINOv2 variant): the attention adjoint may recompute its scores tile by tile (attn_f32m.hip launch_attn_f32_bwd) -- no
// [B*H, N, N] score / adjoint scratch -- instead of the batched-GEMM form (which other head sizes always take).
// Taken from 1 024 tokens per image up (518x518 inputs: 19.8 vs 21.9 ms per ViT-B batch-8 step, and no 2 x 720 MB of scratch); below
// that the batched form is as fast (224x224: 10.0 vs 9.9 ms) and sits closer to a float64 evaluation -- the flash form takes
// delta = <dO, O> from the forward's rounded output instead of sum_j P dP over the probabilities it multiplies (1.7e-5 vs 5.3e-5 from
// float64 on the worst LoRA gradient at 1 370 tokens, the PyTorch composite 2.3e-5).  DINODET_ATTN_BWD_FLASH = 0 / 1 forces either, and so
// does the test option "attn_bwd_flash" (which wins over the variable).
// This is the SINGLE predicate: the scratch carve (no dS / Pd when it holds), the forward's log-sum-exp tape and the backward all ask it, and it
// contains everything launch_attn_f32_bwd itself checks (head_dim 64; q / k / v / o pitches 3D and D multiples of 4: D = heads * 64) -- so that
// launcher's "not taken" return (2) cannot occur behind it; there is no second scratch layout to fall back to.
inline bool tail_flash_bwd(const TDims& d) {
  static const char* e = getenv("DINODET_ATTN_BWD_FLASH");
  if (d.dh != 64 || d.D != d.H * 64 || d.D % 4 != 0 || d.B <= 0 || d.N <= 0) return false;
  const int o = dod_option(DOD_OPT_ATTN_BWD_FLASH);      // tests choose the form per case; set around a whole forward + backward
  if (o >= 0) return o != 0;
  if (e && e[0] == '0') return false;
  return (e && e[0] == '1') || d.N >= 1024;
}
size_t carve_tscratch(const TDims& d, const void* base, TScratch& s) {
  dod::Carver c = carver(base);
  const size_t M = d.M, D = d.D, F = d.F1, big = F > 3 * D ? F : 3 * D;
  s.dx = takef(c, M * D); s.da = takef(c, M * D); s.db = takef(c, M * D); s.dbig = takef(c, M * big); s.dqkv = takef(c, M * 3 * D);
  const bool flash = tail_flash_bwd(d);
  s.dS = takef(c, flash ? 0 : mha_scratch_floats(d.B, d.H, d.N, d.N)); s.Pd = takef(c, flash ? 0 : mha_scratch_floats(d.B, d.H, d.N, d.N));
  s.delta = takef(c, M * (size_t)d.H);
  s.T = takef(c, M * up4(d.r)); s.U = takef(c, M * up4(d.r)); s.dump = takef(c, 2 * big);
  s.dh = d.swiglu ? takef(c, M * (size_t)d.F) : nullptr;        // SwiGLU: d(h) [M, F] beside d(pre) [M, 2F] (the tape stays read-only)
  return c.off;
}
}  // namespace

extern "C" {

size_t dod_backbone_tail_tape_bytes(const dod_config* cfg, int B, int N, int nblocks) {
  TDims d; TTape t; if (!make_tdims(cfg, B, N, nblocks, &d)) return 0;
  return carve_ttape(d, nullptr, t) + 256;
}
size_t dod_backbone_tail_workspace_bytes(const dod_config* cfg, int B, int N, int nblocks) {
  TDims d; TScratch sc; if (!make_tdims(cfg, B, N, nblocks, &d)) return 0;
  return carve_tscratch(d, nullptr, sc) + 256;
}

int dod_backbone_tail_train_forward(const dod_config* cfg, const dod_bb_tail_params* p, const float* x_in, int B, int N, float* mem_out,
                                    void* tape, size_t tape_bytes, void* ws, size_t ws_bytes, void* stream) {
  if (!p || !p->blocks) return dod_fail(DOD_ERR_INVALID, "backbone tail: null parameters");
  TDims d;
  if (!make_tdims(cfg, B, N, p->nblocks, &d)) return dod_fail(DOD_ERR_INVALID, "backbone tail: unsupported configuration (head_dim <= 128, N <= %d, 1 <= lora_r <= 64, at most 8 blocks)", MHA_MAXQ);
  TTape t; TScratch sc;      // carved first: the carve itself says how many bytes each buffer must hold
  int rc = entry_check("backbone tail", x_in && mem_out && tape && ws, 0.f, tape_bytes, carve_ttape(d, tape, t) + 256, ws_bytes, carve_tscratch(d, ws, sc) + 256); if (rc) return rc;
  if (cfg->target_dim && (!p->proj_w || !p->proj_b)) return dod_fail(DOD_ERR_MISSING, "backbone tail: projection weights missing");
  hipStream_t s = (hipStream_t)stream;
  const Mm mm = mm_of(cfg);      // DOD_PREC_BF16X3: every linear of the tail, forward and backward, as a bf16 split product (attention, LoRA rank-r products and LayerNorm stay)
  const int M = d.M, D = d.D, F = d.F, F1 = d.F1;
  const float scale = 1.0f / sqrtf((float)d.dh);
  TH(hipMemcpyAsync(t.b[0].x, x_in, (size_t)M * D * 4, hipMemcpyDeviceToDevice, s));
  for (int i = 0; i < d.nb; ++i) {
    const dod_bb_block_params& bp = p->blocks[i];
    auto& tb = t.b[i];
    // merged weights W' = W + alpha B A (utils.py:68-70), q | k | v concatenated
    const dod_lora_linear* qkv3[3] = {&bp.q, &bp.k, &bp.v};
    for (int c = 0; c < 3; ++c) {
      TK(launch_lora_merge(qkv3[c]->w, qkv3[c]->A, qkv3[c]->Bm, d.alpha, D, D, d.r, tb.Wqkv + (size_t)c * D * D, s));
      TH(hipMemcpyAsync(tb.bqkv + (size_t)c * D, qkv3[c]->b, (size_t)D * 4, hipMemcpyDeviceToDevice, s));
    }
    TK(launch_lora_merge(bp.o.w, bp.o.A, bp.o.Bm, d.alpha, D, D, d.r, tb.Wo, s));
    TK(launch_lora_merge(bp.fc1.w, bp.fc1.A, bp.fc1.Bm, d.alpha, F1, D, d.r, tb.W1, s));
    TK(launch_lora_merge(bp.fc2.w, bp.fc2.A, bp.fc2.Bm, d.alpha, D, F, d.r, tb.W2, s));
    TK(launch_layernorm(tb.x, nullptr, bp.ln1_w, bp.ln1_b, d.eps, M, D, ln_out(tb.y1), s));
    TK(lin_fwd(tb.y1, D, tb.Wqkv, tb.bqkv, M, 3 * D, D, tb.qkv, 3 * D, ACT_NONE, mm, s));
    {
      AttnF32 a; a.q = tb.qkv; a.k = tb.qkv + D; a.v = tb.qkv + 2 * D; a.o = tb.ctx; a.ldq = a.ldk = a.ldv = 3 * D; a.ldo = D;
      a.Lq = a.Lk = N; a.B = B; a.heads = d.H; a.dh = d.dh; a.scale = scale;
      if (d.dh == 64) a.lse = tb.lse;            // fp32-MFMA flash kernel: the adjoint's log-sum-exp comes for free
      TK(launch_attn_f32(a, s));
    }
    TK(lin_fwd(tb.ctx, D, tb.Wo, bp.o.b, M, D, D, tb.x1, D, ACT_NONE, mm, s, bp.ls1, tb.x, D));      // x1 = x + ls1 * (ctx Wo'^T + bo)
    TK(launch_layernorm(tb.x1, nullptr, bp.ln2_w, bp.ln2_b, d.eps, M, D, ln_out(tb.y2), s));
    TK(lin_fwd(tb.y2, D, tb.W1, bp.fc1.b, M, F1, D, tb.pre, F1, ACT_NONE, mm, s));      // taped: the backward needs the pre-activation
    if (d.swiglu) TK(swiglu_fwd(tb.pre, tb.h, (size_t)M, F, s));      // fc1 / fc2 = weights_in / weights_out
    else TK(gelu_fwd(tb.pre, tb.h, (size_t)M * F, s));
    float* xnext = i + 1 < d.nb ? t.b[i + 1].x : t.xout;
    TK(lin_fwd(tb.h, F, tb.W2, bp.fc2.b, M, D, F, xnext, D, ACT_NONE, mm, s, bp.ls2, tb.x1, D));     // x2 = x1 + ls2 * (h W2'^T + b2)
  }
  if (cfg->target_dim) {
    TK(launch_layernorm(t.xout, nullptr, p->lnf_w, p->lnf_b, d.eps, M, D, ln_out(t.f), s));
    TK(lin_fwd(t.f, D, p->proj_w, p->proj_b, M, d.Dd, D, mem_out, d.Dd, ACT_NONE, mm, s));
  } else {
    TK(launch_layernorm(t.xout, nullptr, p->lnf_w, p->lnf_b, d.eps, M, D, ln_out(mem_out), s));
  }
  return DOD_OK;
}

int dod_backbone_tail_train_backward(const dod_config* cfg, const dod_bb_tail_params* p, int B, int N, const float* d_mem, const void* tape,
                                     size_t tape_bytes, const dod_bb_tail_params* grads, void* ws, size_t ws_bytes, void* stream) {
  if (!p || !p->blocks || !grads || !grads->blocks || grads->nblocks != p->nblocks) return dod_fail(DOD_ERR_INVALID, "backbone tail: null / mismatched parameters");
  TDims d;
  if (!make_tdims(cfg, B, N, p->nblocks, &d)) return dod_fail(DOD_ERR_INVALID, "backbone tail: unsupported configuration");
  TTape t; TScratch sc;      // carved first: the carve itself says how many bytes each buffer must hold
  int rc = entry_check("backbone tail", d_mem && tape && ws, 0.f, tape_bytes, carve_ttape(d, tape, t) + 256, ws_bytes, carve_tscratch(d, ws, sc) + 256); if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const Mm mm = mm_of(cfg);
  auto G = [](const float* q) { return const_cast<float*>(q); };
  const int M = d.M, D = d.D, F = d.F, F1 = d.F1;
  const size_t nMD = (size_t)M * D;
  const float scale = 1.0f / sqrtf((float)d.dh);
  // ---- projection + final LayerNorm (frozen affine: its parameter gradients go to a dump)
  if (cfg->target_dim) {
    TK(lin_bwd_w(d_mem, d.Dd, t.f, D, M, d.Dd, D, G(grads->proj_w), G(grads->proj_b), mm, s));
    TK(lin_bwd_x(d_mem, d.Dd, p->proj_w, M, d.Dd, D, sc.da, false, mm, s));
    TK(ln_bwd(t.xout, p->lnf_w, sc.da, d.eps, M, D, sc.dx, sc.dump, sc.dump + D, s));
  } else {
    TK(ln_bwd(t.xout, p->lnf_w, d_mem, d.eps, M, D, sc.dx, sc.dump, sc.dump + D, s));
  }
  // sc.dx = d(block output)
  for (int i = d.nb - 1; i >= 0; --i) {
    const dod_bb_block_params& bp = p->blocks[i];
    const dod_bb_block_params& gp = grads->blocks[i];
    const auto& tb = t.b[i];
    // x2 = x1 + ls2 * (h W2'^T + b2)
    TK(colscale(sc.dx, bp.ls2, sc.da, nMD, D, s));                                                                        // da = d(fc2 out)
    TK(lora_grads(tb.h, F, sc.da, D, D, bp.fc2.A, bp.fc2.Bm, M, d.r, d.alpha, G(gp.fc2.A), G(gp.fc2.Bm), sc.T, sc.U, s));
    if (d.swiglu) {     // d(h) [M, F], then d(pre) = [d(x1) | d(x2)] in dbig
      TK(lin_bwd_x(sc.da, D, tb.W2, M, D, F, sc.dh, false, mm, s));
      TK(swiglu_bwd(sc.dh, tb.pre, sc.dbig, (size_t)M, F, s));
    } else {
      TK(lin_bwd_x(sc.da, D, tb.W2, M, D, F, sc.dbig, false, mm, s));                                                     // d(h)
      TK(gelu_bwd(sc.dbig, tb.pre, sc.dbig, (size_t)M * F, s));
    }
    TK(lora_grads(tb.y2, D, sc.dbig, F1, F1, bp.fc1.A, bp.fc1.Bm, M, d.r, d.alpha, G(gp.fc1.A), G(gp.fc1.Bm), sc.T, sc.U, s));
    TK(lin_bwd_x(sc.dbig, F1, tb.W1, M, F1, D, sc.da, false, mm, s));                                                     // d(y2)
    TK(ln_bwd(tb.x1, bp.ln2_w, sc.da, d.eps, M, D, sc.db, sc.dump, sc.dump + D, s));
    TK(add_inplace(sc.dx, sc.db, nMD, s));                                                                                // dx = d(x1)
    // x1 = x + ls1 * (ctx Wo'^T + bo)
    TK(colscale(sc.dx, bp.ls1, sc.da, nMD, D, s));
    TK(lora_grads(tb.ctx, D, sc.da, D, D, bp.o.A, bp.o.Bm, M, d.r, d.alpha, G(gp.o.A), G(gp.o.Bm), sc.T, sc.U, s));
    TK(lin_bwd_x(sc.da, D, tb.Wo, M, D, D, sc.db, false, mm, s));                                                         // db = d(ctx)
    if (tail_flash_bwd(d)) {
      AttnF32Bwd g;
      g.q = tb.qkv; g.k = tb.qkv + D; g.v = tb.qkv + 2 * D; g.o = tb.ctx; g.d_o = sc.db; g.lse = tb.lse;
      g.dq = sc.dqkv; g.dk = sc.dqkv + D; g.dv = sc.dqkv + 2 * D; g.delta = sc.delta;
      g.ldq = g.ldk = g.ldv = g.lddq = g.lddk = g.lddv = 3 * D; g.ldo = D;
      g.Lq = g.Lk = N; g.B = B; g.heads = d.H; g.dh = d.dh; g.scale = scale;
      TK(launch_attn_f32_bwd(g, s));
    } else {
      TK(launch_mha_bwd(tb.qkv, 3 * D, sc.db, D, sc.dqkv, sc.dS, sc.Pd, B, N, d.H, D, d.dh, scale, 0.f, 0ull, s));
    }
    const dod_lora_linear* qkv3[3] = {&bp.q, &bp.k, &bp.v};
    const dod_lora_linear* gqkv3[3] = {&gp.q, &gp.k, &gp.v};
    for (int c = 0; c < 3; ++c)
      TK(lora_grads(tb.y1, D, sc.dqkv + (size_t)c * D, 3 * D, D, qkv3[c]->A, qkv3[c]->Bm, M, d.r, d.alpha, G(gqkv3[c]->A), G(gqkv3[c]->Bm), sc.T, sc.U, s));
    if (i > 0) {        // the tail's input is the frozen prefix's output: nothing below block 0 needs a gradient
      TK(lin_bwd_x(sc.dqkv, 3 * D, tb.Wqkv, M, 3 * D, D, sc.da, false, mm, s));                                           // d(y1)
      TK(ln_bwd(tb.x, bp.ln1_w, sc.da, d.eps, M, D, sc.db, sc.dump, sc.dump + D, s));
      TK(add_inplace(sc.dx, sc.db, nMD, s));                                                                              // dx = d(x): the block below's output
    }
  }
  return DOD_OK;
}

}  // extern "C"
