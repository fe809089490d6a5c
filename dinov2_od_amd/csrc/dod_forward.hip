// Workspace carving and the two forward schedules of libdinodet.so: the DINOv2 backbone and the DETR decoder.
// Reference call stack being replaced: SURVEY.md section 3.1.
#include "dod_internal.h"

#include <cmath>
#include <cstdlib>

using namespace dod;

size_t dod::carve_decoder(const dod_handle* h, Carver& c, int B, int N, DecWS* w, bool need_mem_op) {
  const dod_config& g = h->cfg;
  const size_t BQ = (size_t)B * g.num_queries, Dd = g.dec_hidden, M = (size_t)B * N;
  DecWS t;
  t.tgt = (float*)c.take(BQ * Dd * 4); t.t2 = (float*)c.take(BQ * Dd * 4); t.att = (float*)c.take(BQ * Dd * 4);
  t.samp = (float*)c.take(BQ * Dd * 4); t.qkv = (float*)c.take(BQ * 3 * Dd * 4);
  t.proj = (float*)c.take(BQ * (size_t)(h->ncat > 0 ? h->ncat : 4) * 4);
  t.ffn = (float*)c.take(BQ * (size_t)g.dim_feedforward * 4); t.hb = (float*)c.take(BQ * (Dd / 2) * 4);
  t.qd = (float*)c.take(BQ * Dd * 4);
  { const size_t kmax = Dd > (size_t)g.dim_feedforward ? Dd : (size_t)g.dim_feedforward;
    const bool want3 = is_bf16(h) || is_x3(h);      // (not "t.a3 != null": the sizing pass carves from a null base)
    t.a3 = want3 ? (bf16_t*)c.take(BQ * 3 * kmax * 2) : nullptr;
    t.a3b = want3 ? (bf16_t*)c.take(BQ * 3 * kmax * 2) : nullptr; }     // second operand buffer: a GEMM that reads a3 may write the next GEMM's operand
  t.mem2 = is_x3(h) ? (bf16_t*)c.take(M * 2 * Dd * 2) : nullptr;
  t.mem_op = need_mem_op ? c.take(M * Dd * esz(h)) : nullptr;
  if (g.use_deformable) {
    int uniq = 0; for (auto& L : h->DL) if (L.vp_alias < 0) ++uniq;
    if (!h->finalized) uniq = g.dec_layers;
    t.values = (float*)c.take(M * Dd * 4 * (size_t)(uniq > 0 ? uniq : 1)); t.kv = nullptr;
  } else {
    t.values = nullptr; t.kv = (float*)c.take(M * 2 * Dd * 4);
  }
  if (w) *w = t;
  return c.off;
}

size_t dod::carve_backbone(const dod_handle* h, Carver& c, int B, int N, BbWS* w) {
  const dod_config& g = h->cfg;
  const size_t M = (size_t)B * N, D = g.hidden, es = esz(h), Np = N - 1;
  const size_t F1 = g.swiglu ? 2 * (size_t)g.ffn_hidden : (size_t)g.ffn_hidden;
  size_t hb = M * F1; const size_t col = (size_t)B * Np * (size_t)(h->Kp ? h->Kp : (3 * g.patch * g.patch + 63) / 64 * 64);
  if (col > hb) hb = col;
  BbWS t;
  t.x = (float*)c.take(M * D * 4); t.y = c.take(M * D * es); t.qkv = c.take(M * 3 * D * es); t.ctx = c.take(M * D * es);
  t.hbuf = c.take(hb * es); t.gated = g.swiglu ? c.take(M * (size_t)g.ffn_hidden * es) : nullptr;
  t.mem = c.take(M * (size_t)(g.target_dim ? g.target_dim : g.hidden) * es);
  t.rs = is_fp8(h) ? (float*)c.take(M * 4) : nullptr;
  t.bs = (is_fp8(h) && g.swiglu && g.ffn_hidden % 256 == 0) ? (unsigned char*)c.take(M * (size_t)(g.ffn_hidden / 32)) : nullptr;     // e8m0 block scales of the gated rows
  t.bsx = (is_fp8(h) && D % 256 == 0) ? (unsigned char*)c.take(M * (D / 32)) : nullptr;
  const bool foldable = ln_foldable(h);      // (not "L.fold": the sizing pass may run before finalize)
  t.lnp = foldable ? (float2*)c.take(M * ((D + 127) / 128) * 8) : nullptr;
  t.lns = foldable ? (float2*)c.take(M * 8) : nullptr;
  t.lns2 = foldable ? (float2*)c.take(M * 8) : nullptr;
  if (w) *w = t;
  return c.off;
}

int dod::prepare_impl(dod_handle* h, int H, int W, hipStream_t s) {
  const dod_config& g = h->cfg;
  if (!h->finalized || !h->has_bb) return fail(h, DOD_ERR_STATE, "backbone weights not finalized");
  if (H < g.patch || W < g.patch) return fail(h, DOD_ERR_INVALID, "image %dx%d smaller than one patch", H, W);
  if (h->pos_H == H && h->pos_W == W) return DOD_OK;
  const int gh = H / g.patch, gw = W / g.patch;
  // modeling_dinov2.py:71-72: used as is only when num_patches == num_positions and H == W
  if (gh * gw == g.pos_grid * g.pos_grid && H == W) { h->pos_hw = h->pos; h->pos_H = H; h->pos_W = W; return DOD_OK; }
  // the table depends on (gh, gw) only -- and on H != W for the square-count case above
  const std::pair<int, int> key(gh, gw);
  auto it = h->pos_cache.find(key);
  if (it == h->pos_cache.end()) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (s && hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
      return fail(h, DOD_ERR_STATE, "first forward at %dx%d inside a stream capture: call dod_prepare(h, %d, %d) before capturing", H, W, H, W);
    const size_t need = (size_t)(gh * gw + 1) * g.hidden;
    float* buf = nullptr;
    HIPCHK(h, hipMalloc((void**)&buf, need * 4));
    h->owned.push_back(buf);
    KCHK(h, launch_pos_resize(h->pos, g.pos_grid, gh, gw, g.hidden, buf, s));
    it = h->pos_cache.emplace(key, buf).first;
  }
  h->pos_hw = it->second; h->pos_H = H; h->pos_W = W;
  return DOD_OK;
}

namespace {

void spatial_factor(int hw, int* h, int* w) {   // deformable_attention.py:241-256
  int s = (int)std::sqrt((double)hw);
  while ((s + 1) * (s + 1) <= hw) ++s;
  while (s * s > hw) --s;
  if (s * s != hw) {
    for (int i = s; i > 0; --i) if (hw % i == 0) { *h = i; *w = hw / i; return; }
  }
  *h = s; *w = s;
}

int tap(dod_handle* h, int stage, const void* src, bool src_bf16, size_t n, hipStream_t s) {
  auto it = h->taps.find(stage);
  if (it == h->taps.end() || !it->second) return 0;
  if (!src_bf16) { (void)hipMemcpyAsync(it->second, src, n * 4, hipMemcpyDeviceToDevice, s); return 0; }
  return launch_widen_bf16((const bf16_t*)src, it->second, n, s);
}

// generic linear on bf16 or fp32 operands
// flops_K: the ALGORITHMIC reduction length booked for the roofline (0 = K; the split-3 form executes 3K for K)
int linear(dod_handle* h, bool bf, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const GemmEpi& e, hipStream_t s, int flops_K = 0) {
  ProfScope ps(h, s, bf ? PC_GEMM_BF16 : PC_GEMM_F32, 2.0 * M * N * (e.rows_per_img > 0 ? 3.0 * h->cfg.patch * h->cfg.patch : (double)(flops_K ? flops_K : K)));
  int r = bf ? launch_gemm_bf16((const bf16_t*)A, lda, (const bf16_t*)W, ldw, M, N, K, e, s)
             : launch_gemm_f32((const float*)A, lda, (const float*)W, ldw, M, N, K, e, s, h->cfg.precision != DOD_PREC_FP32);      // (the strict mode keeps one k-ordered chain per output)
  return rejected(h, r, "linear launch (M=%d N=%d K=%d bf16=%d)", M, N, K, (int)bf);
}
// bf16x3 linear on pair-layout operands A2 [M, 2K] = [Ah | Al], W2 [N, 2K] = [Wh | Wl] (gemm_x3.hip; algorithmic FLOPs reported)
int linear3(dod_handle* h, const void* A3, const void* W3, int M, int N, int K, const GemmEpi& e, hipStream_t s) {
  ProfScope ps(h, s, PC_GEMM_BF16, 2.0 * M * N * (double)K);
  int r = launch_gemm_x3((const bf16_t*)A3, 2 * K, (const bf16_t*)W3, 2 * K, M, N, K, e, s);
  return rejected(h, r, "bf16x3 linear launch (M=%d N=%d K=%d)", M, N, K);
}

// ------------------------------------------------------------------------------------------- backbone block
// Activation rows as a block linear reads them, in the precision's operand format (bf16 / fp32 rows, pair layout, H2 rows, e4m3 bytes)
struct Operand {
  const void* rows;
  const float* row_scale = nullptr;      // fp8 mode: per-row dequant scales [M], or
  const unsigned char* bs = nullptr;     // e8m0 block scales [M][2][K / 64]
};

// One linear of a backbone block, Y[M, N] = A[M, K] W^T with epilogue e, on the GEMM family of the handle's precision and of what the packer
// left in W: H2 (fp16x2), split product (bf16x3), fp8 (W carries scales), else bf16 / fp32.  Algorithmic FLOPs booked.
int block_linear(dod_handle* h, const Operand& a, const PackedLinear& W, int M, int N, int K, GemmEpi e, hipStream_t s) {
  if (is_h2(h)) {      // activation rows 4K bytes, weight rows 3K bytes + exponent bytes
    ProfScope ps(h, s, PC_GEMM_BF16, 2.0 * M * N * (double)K);
    e.h2_wexp = W.wexp;
    return rejected(h, launch_gemm_h2(a.rows, 4 * K, W.W, 3 * K, M, N, K, e, s), "fp16x2 linear launch (M=%d N=%d K=%d)", M, N, K);
  }
  if (is_x3(h)) return linear3(h, a.rows, W.W, M, N, K, e, s);
  if (W.wscale || W.wbs) {      // A_q [M, K] e4m3 with per-row or block scales, W_q [N, K] e4m3 with per-row (output feature) or block scales
    ProfScope ps(h, s, PC_GEMM_FP8, 2.0 * M * N * (double)K);
    e.a_scale = a.row_scale; e.w_scale = W.wscale; e.a_bs = a.bs; e.w_bs = W.wbs;
    return rejected(h, launch_gemm_fp8((const unsigned char*)a.rows, K, (const unsigned char*)W.W, K, M, N, K, e, s), "fp8 linear launch (M=%d N=%d K=%d)", M, N, K);
  }
  return linear(h, is_bf16(h), a.rows, K, W.W, K, M, N, K, e, s);
}

// The per-block stages that differ by precision.  One instance per forward: it carries the folded-LayerNorm statistics state across blocks.
struct BlockRun {
  dod_handle* h; const BbWS& ws; hipStream_t s;
  int B, N, M, D, F;
  bool bf, f8, x3, h2, fold;
  float scale;
  // Folded LayerNorm (BLayer::fold; modeling_dinov2.py:361-380): no norm1 / norm2 pass.  ws.y always holds the CURRENT residual rows in the
  // operand format (written by rowstats for block 0, then by the out-proj / fc2 epilogues), ws.lns their (mean, rstd).
  // Row statistics ping-pong between two [M] buffers: stat[cur] holds the rows' latest (mean, rstd) -- the shift of the next producer; the consumer
  // behind a producer reads that shift from stat[cur] with the producer's group sums, finishes the statistics in its epilogue and publishes them
  // to stat[cur ^ 1] (its other tiles still read the shift): no launch merges the groups
  float2* stat[2];
  int cur = 0;
  bool fresh = false;      // a producer wrote group sums since the last consumer
  int op_kind, npart;

  BlockRun(dod_handle* h_, const BbWS& ws_, hipStream_t s_, int B_, int N_, bool fold_)
      : h(h_), ws(ws_), s(s_), B(B_), N(N_), M(B_ * N_), D(h_->cfg.hidden), F(h_->cfg.ffn_hidden), bf(is_bf16(h_)), f8(is_fp8(h_)), x3(is_x3(h_)),
        h2(is_h2(h_)), fold(fold_), scale(1.0f / std::sqrt((float)(h_->cfg.hidden / h_->cfg.heads))), stat{ws_.lns, ws_.lns2},
        op_kind(is_h2(h_) ? LNOP_H2 : (is_x3(h_) ? LNOP_PAIR : LNOP_BF16)), npart((h_->cfg.hidden + 127) / 128) {}

  // fp8 mode, block-scaled on both operands (round 4): every e4m3 activation row carries one e8m0 byte per 32 columns, written by its
  // producer -- LayerNorm, the attention epilogue, the SwiGLU epilogue of weights_in; no per-row maxima anywhere.  Else (widths that are
  // not multiples of 256) per-row scales in ws.rs.
  bool mx(const BLayer& L) const { return f8 && L.qkv.wbs && ws.bsx; }

  // out-proj / fc2: act(...) * LayerScale + residual, in place on the fp32 stream; folded: + the operand copy of the new rows + their group statistics
  GemmEpi residual_epi(const PackedLinear& W, const float* layer_scale, bool next_norm_reads) {
    GemmEpi e = epi(W.bias, ws.x, nullptr, D, ACT_NONE, layer_scale, ws.x, D);
    if (fold && next_norm_reads) {
      e.ln_op = ws.y; e.ln_op_kind = op_kind; e.ln_op_ld = (op_kind == LNOP_BF16 ? D : 2 * D); e.ln_part = ws.lnp; e.ln_npart = npart; e.ln_shift = stat[cur];
      fresh = true;
    }
    return e;
  }
  // QKV / MLP-in behind a folded norm: normalise in the epilogue (and finish the producer's statistics)
  GemmEpi normed_epi(GemmEpi e, const PackedLinear& W) {
    if (fold) {
      e.ln_stats = stat[cur]; e.ln_c = W.csum;
      if (fresh) { e.ln_part_in = ws.lnp; e.ln_npart = npart; e.ln_stats_out = stat[cur ^ 1]; e.ln_eps = h->cfg.ln_eps; cur ^= 1; fresh = false; }
    }
    return e;
  }
  // stages 1 / 5: the normalised residual rows as the operand of QKV / MLP-in.  Folded: ws.y already holds the rows, the consumer normalises.
  int norm(const BLayer& L, const float* gamma, const float* beta, Operand* y) {
    *y = Operand{ws.y, f8 && !mx(L) ? ws.rs : nullptr, mx(L) ? ws.bsx : nullptr};
    if (fold) return 0;
    LnOut o;
    if (x3) o.split = (bf16_t*)ws.y;       // pair layout [hi | lo] (bf16x3) or H2 rows (fp16x2): 4 bytes per element either way
    else if (f8) { o.fp8 = (unsigned char*)ws.y; o.scale = (float*)y->row_scale; o.bs = (unsigned char*)y->bs; }
    else if (bf) o.bf16 = (bf16_t*)ws.y;
    else o.f32 = (float*)ws.y;
    ProfScope ps(h, s, PC_LAYERNORM, 0);
    KCHK(h, launch_layernorm(ws.x, nullptr, gamma, beta, h->cfg.ln_eps, M, D, o, s, h2 ? 1 : 0));
    return 0;
  }
  // stages 2 + 3: QKV and attention -> the context rows as out-proj's operand
  int attention(const BLayer& L, const Operand& y, Operand* ctx) {
    const int heads = h->cfg.heads;
    const bool flash = D / heads == 64;      // x3: split-product flash attention on the bf16 MFMA cores (both modes: its q / k / v stay bf16 pairs)
    GemmEpi eq = epi(L.qkv.bias, bf ? nullptr : (float*)ws.qkv, bf ? ws.qkv : nullptr, 3 * D);
    if (x3 && flash) { eq = epi(L.qkv.bias, nullptr, ws.qkv, 6 * D); eq.out_split = -3 * D; }      // [hi(q|k|v) | lo(q|k|v)]
    int rc = block_linear(h, y, L.qkv, M, 3 * D, D, normed_epi(eq, L.qkv), s); if (rc) return rc;
    const double flops = 4.0 * B * (double)N * N * D;
    *ctx = Operand{ws.ctx};
    if (x3 && flash) {
      ProfScope ps(h, s, PC_ATTN_BF16, flops);
      KCHK(h, launch_attn_x3((const bf16_t*)ws.qkv, (bf16_t*)ws.ctx, B, N, heads, scale, s, h2 ? 1 : 0));
    } else if (bf && mx(L)) {   // the attention epilogue quantises its own tiles (a head's 64 context columns = two blocks): e4m3 bytes into ws.y, scales into ws.bsx
      ProfScope ps(h, s, PC_ATTN_BF16, flops);
      KCHK(h, launch_attn_bf16((const bf16_t*)ws.qkv, (bf16_t*)ws.y, B, N, heads, scale, s, ws.bsx));
      *ctx = Operand{ws.y, nullptr, ws.bsx};
    } else if (bf) {
      { ProfScope ps(h, s, PC_ATTN_BF16, flops); KCHK(h, launch_attn_bf16((const bf16_t*)ws.qkv, (bf16_t*)ws.ctx, B, N, heads, scale, s)); }
      if (f8) {   // out-proj on e4m3 operands too: the bf16 context rows are quantised by one pass (the attention kernel writes them head-wise)
        KCHK(h, launch_quant_rows_fp8(ws.ctx, 1, D, M, D, (unsigned char*)ws.y, D, ws.rs, s));
        *ctx = Operand{ws.y, ws.rs};
      }
    } else {                    // generic fp32 attention; x3 with other head sizes (micro test models): then split
      float* o = x3 ? (float*)ws.hbuf : (float*)ws.ctx;
      {
        ProfScope ps(h, s, PC_ATTN_F32, flops);
        AttnF32 a; const float* q = (const float*)ws.qkv;
        a.q = q; a.k = q + D; a.v = q + 2 * D; a.o = o; a.ldq = a.ldk = a.ldv = 3 * D; a.ldo = D;
        a.Lq = a.Lk = N; a.B = B; a.heads = heads; a.dh = D / heads; a.scale = scale;
        KCHK(h, launch_attn_f32(a, s));
      }
      if (x3) KCHK(h, split(o, D, ws.ctx));
    }
    return 0;
  }
  // fp32 rows -> the compensated modes' operand rows
  int split(const float* src, int cols, void* dst) {
    return h2 ? launch_split_h2(src, cols, dst, M, cols, nullptr, s) : launch_split2(src, cols, (bf16_t*)dst, M, cols, s);
  }
  // stage 6: MLP-in with its activation / gate -> the hidden rows as MLP-out's operand
  int mlp_in(const BLayer& L, const Operand& y, Operand* hidden) {
    const dod_config& g = h->cfg;
    // fp8 SwiGLU: block-scaled gated rows written by the weights_in epilogue (F % 256 == 0; tuning builds, DINODET_FP8_MX_GATE=0: bf16 rows + a quantisation pass)
    static const bool mx_gate_env = [] { const char* v = DOD_TUNE_ENV("DINODET_FP8_MX_GATE"); return !(v && v[0] == '0'); }();
    const PackedLinear& W = L.fc1;
    int rc;
    if (!g.swiglu) {            // GELU in the epilogue.  fp8 mode: fc2 stays bf16 (its input is produced tile-wise by fc1's epilogue: no per-row scale)
      GemmEpi e1 = epi(W.bias, bf ? nullptr : (float*)ws.hbuf, bf ? ws.hbuf : nullptr, F, ACT_GELU);
      if (x3) { e1 = epi(W.bias, nullptr, ws.hbuf, 2 * F, ACT_GELU); if (h2) e1.out_h2 = 1; else e1.out_split = -F; }      // H2 rows / pair layout [hi | lo]
      *hidden = Operand{ws.hbuf};
      return block_linear(h, y, W, M, F, D, normed_epi(e1, W), s);
    }
    if (L.glu) {                // gate in the weights_in epilogue (interleaved columns), written in weights_out's operand format
      GemmEpi eg = epi(W.bias, nullptr, ws.gated, F);
      *hidden = Operand{ws.gated};
      const bool gate_mx = f8 && ws.bs && (mx(L) || (mx_gate_env && F % 256 == 0));
      if (x3) { eg = epi(W.bias, nullptr, ws.hbuf, 2 * F); if (h2) eg.out_h2 = 1; else eg.out_split = -F; *hidden = Operand{ws.hbuf}; }
      else if (gate_mx) { eg.out_bs = ws.bs; *hidden = Operand{ws.gated, nullptr, ws.bs}; }      // AND block-scaled quantisation: e4m3 gated rows, no bf16 hidden rows
      else if (f8) eg = epi(W.bias, nullptr, ws.hbuf, F);                                          // [M, F] bf16, then the row quantisation below
      eg.glu = 1;
      rc = block_linear(h, y, W, M, 2 * F, D, normed_epi(eg, W), s); if (rc) return rc;
      if (f8 && !gate_mx) {
        KCHK(h, launch_quant_rows_fp8(ws.hbuf, 1, F, M, F, (unsigned char*)ws.gated, F, ws.rs, s));
        *hidden = Operand{ws.gated, ws.rs};
      }
      return 0;
    }
    // gate as a kernel of its own over the [M, 2F] rows
    rc = block_linear(h, y, W, M, 2 * F, D, normed_epi(epi(W.bias, bf ? nullptr : (float*)ws.hbuf, bf ? ws.hbuf : nullptr, 2 * F), W), s); if (rc) return rc;
    *hidden = Operand{ws.gated};
    if (f8) { KCHK(h, launch_swiglu_fp8((const bf16_t*)ws.hbuf, M, F, (unsigned char*)ws.gated, ws.rs, s)); *hidden = Operand{ws.gated, ws.rs}; }
    else KCHK(h, launch_swiglu(bf ? nullptr : (const float*)ws.hbuf, bf ? (const bf16_t*)ws.hbuf : nullptr, M, F, bf ? nullptr : (float*)ws.gated, bf ? (bf16_t*)ws.gated : nullptr, s));
    if (x3) { KCHK(h, split((const float*)ws.gated, F, ws.hbuf)); *hidden = Operand{ws.hbuf}; }
    return 0;
  }
  // one transformer block (modeling_dinov2.py:361-380) on the fp32 residual stream ws.x
  int block(const BLayer& L, bool more) {      // more: another block reads the residual after this one (the final LayerNorm is a kernel of its own)
    if (mx(L) && h->cfg.swiglu && !(L.glu && ws.bs)) return fail(h, DOD_ERR_STATE, "fp8 SwiGLU MLP needs the fused gate (block-scaled rows)");
    Operand y, ctx, hidden;
    int rc = norm(L, L.ln1w, L.ln1b, &y); if (rc) return rc;                                                    // 1    K3
    rc = attention(L, y, &ctx); if (rc) return rc;                                                              // 2, 3 K4, K5
    rc = block_linear(h, ctx, L.o, M, D, D, residual_epi(L.o, L.ls1, true), s); if (rc) return rc;              // 4    K6
    rc = norm(L, L.ln2w, L.ln2b, &y); if (rc) return rc;                                                        // 5
    rc = mlp_in(L, y, &hidden); if (rc) return rc;                                                              // 6    K7 / K7g
    return block_linear(h, hidden, L.fc2, M, D, F, residual_epi(L.fc2, L.ls2, more), s);                        // 7
  }
};

}  // namespace

int dod::backbone_impl(dod_handle* h, const float* pixels, int B, int H, int W, const BbWS& ws, float* feat_f32, bool want_mem, hipStream_t s,
                       int stop_blocks, float* x_out, const unsigned char* pixels_u8) {
  const dod_config& g = h->cfg;
  const bool bf = is_bf16(h);
  const int D = g.hidden, p = g.patch;
  const int gh = H / p, gw = W / p, Np = gh * gw, N = Np + 1, M = B * N;
  if (!h->has_bb) return fail(h, DOD_ERR_STATE, "no backbone weights were registered");
  if (bf && D / g.heads != 64) return fail(h, DOD_ERR_INVALID, "bf16 attention kernel needs head_dim 64 (got %d)", D / g.heads);
  int rc = prepare_impl(h, H, W, s); if (rc) return rc;
  // K1 + K2.  Fused form (patch_embed.hip): implicit im2col in the GEMM's load stage, bias + position add in its epilogue; the
  // uint8 HWC input of the device input pipeline (dod_forward_u8) exists only there.
  if (pixels_u8 && !h->Wpe) return fail(h, DOD_ERR_INVALID, "uint8 input needs the fused patch embed (bf16 / bf16x3 / fp8 precision, patch size 14 or 16)");
  if (h->Wpe && (pixels_u8 || W % 2 == 0)) {
    ProfScope ps(h, s, PC_GEMM_BF16, 2.0 * B * Np * (double)D * 3.0 * p * p);
    KCHK(h, launch_patch_embed(pixels_u8 ? (const void*)pixels_u8 : (const void*)pixels, pixels_u8 ? 1 : 0, B, H, W, p, h->Wpe, is_x3(h) ? 1 : 0,
                               h->bpatch, h->pos_hw, ws.x, D, s));
  } else if (is_x3(h) && h->Wpatch2 && (size_t)3 * D * 6 >= (size_t)h->Kp2 * 4) {   // split-product patch embed (pair operand staged in ws.qkv)
    const int K2 = h->Kp2;
    KCHK(h, launch_im2col(pixels, B, H, W, p, K2, (float*)ws.hbuf, nullptr, s));
    KCHK(h, launch_split2((const float*)ws.hbuf, K2, (bf16_t*)ws.qkv, B * Np, K2, s));
    GemmEpi e = epi(h->bpatch, ws.x, nullptr, D);
    e.pos = h->pos_hw; e.rows_per_img = Np; e.out_rows_per_img = N;
    ProfScope ps(h, s, PC_GEMM_BF16, 2.0 * B * Np * (double)D * 3.0 * p * p);
    KCHK(h, launch_gemm_x3((const bf16_t*)ws.qkv, 2 * K2, h->Wpatch2, 2 * K2, B * Np, D, K2, e, s));
  } else {
    KCHK(h, launch_im2col(pixels, B, H, W, p, h->Kp, bf ? nullptr : (float*)ws.hbuf, bf ? (bf16_t*)ws.hbuf : nullptr, s));
    GemmEpi e = epi(h->bpatch, ws.x, nullptr, D);
    e.pos = h->pos_hw; e.rows_per_img = Np; e.out_rows_per_img = N;
    rc = linear(h, bf, ws.hbuf, h->Kp, h->Wpatch, h->Kp, B * Np, D, h->Kp, e, s); if (rc) return rc;
  }
  KCHK(h, launch_cls_row(h->cls, h->pos_hw, ws.x, B, N, D, s));
  tap(h, 0, ws.x, false, (size_t)M * D, s);
  float* yf = bf ? nullptr : (float*)ws.y; bf16_t* yb = bf ? (bf16_t*)ws.y : nullptr;
  const bool x3 = is_x3(h);
  const int nblocks = stop_blocks >= 0 ? (stop_blocks < g.layers ? stop_blocks : g.layers) : g.layers;
  const bool fold = ln_foldable(h) && !h->L.empty() && h->L[0].fold;
  if (fold && !(ws.lnp && ws.lns && ws.lns2)) return fail(h, DOD_ERR_STATE, "internal: the weights were packed with the LayerNorm folded but the workspace has no statistics buffers");
  BlockRun run(h, ws, s, B, N, fold);
  if (fold && nblocks > 0) { ProfScope ps(h, s, PC_LAYERNORM, 0); KCHK(h, launch_rowstats(ws.x, M, D, g.ln_eps, ws.y, run.op_kind, run.stat[0], s)); }
  for (int i = 0; i < nblocks; ++i) {
    rc = run.block(h->L[i], i + 1 < g.layers); if (rc) return rc;
    tap(h, 1 + i, ws.x, false, (size_t)M * D, s);                                                               // 8
  }
  if (stop_blocks >= 0) {
    HIPCHK(h, hipMemcpyAsync(x_out, ws.x, (size_t)M * D * 4, hipMemcpyDeviceToDevice, s));
    return DOD_OK;
  }
  // final LayerNorm (+ projection K9)
  if (!g.target_dim) {
    float* of = feat_f32 ? feat_f32 : (bf ? nullptr : (want_mem ? (float*)ws.mem : nullptr));
    bf16_t* ob = (bf && want_mem) ? (bf16_t*)ws.mem : nullptr;
    KCHK(h, launch_layernorm(ws.x, nullptr, h->lnfw, h->lnfb, g.ln_eps, M, D, ln_out(of, ob), s));
    if (!bf && want_mem && feat_f32) HIPCHK(h, hipMemcpyAsync(ws.mem, feat_f32, (size_t)M * D * 4, hipMemcpyDeviceToDevice, s));
  } else {
    const int Dd = g.target_dim;
    if (x3) {
      { LnOut o; o.split = (bf16_t*)ws.y; KCHK(h, launch_layernorm(ws.x, nullptr, h->lnfw, h->lnfb, g.ln_eps, M, D, o, s)); }
      float* dst = feat_f32 ? feat_f32 : (float*)ws.mem;
      rc = linear3(h, ws.y, h->Wproj, M, Dd, D, epi(h->bproj, dst, nullptr, Dd), s); if (rc) return rc;
      if (feat_f32 && want_mem) HIPCHK(h, hipMemcpyAsync(ws.mem, feat_f32, (size_t)M * Dd * 4, hipMemcpyDeviceToDevice, s));
      return DOD_OK;
    }
    KCHK(h, launch_layernorm(ws.x, nullptr, h->lnfw, h->lnfb, g.ln_eps, M, D, ln_out(yf, yb), s));
    if (feat_f32) { rc = linear(h, bf, ws.y, D, h->Wproj, D, M, Dd, D, epi(h->bproj, feat_f32, nullptr, Dd), s); if (rc) return rc; }
    if (want_mem) { rc = linear(h, bf, ws.y, D, h->Wproj, D, M, Dd, D, epi(h->bproj, bf ? nullptr : (float*)ws.mem, bf ? ws.mem : nullptr, Dd), s); if (rc) return rc; }
  }
  return DOD_OK;
}

int dod::decoder_impl(dod_handle* h, const void* mem_op, int B, int N, const DecWS& ws, float* det, hipStream_t s, bool l0_only) {
  const dod_config& g = h->cfg;
  const bool bf = is_bf16(h);
  const int Dd = g.dec_hidden, Q = g.num_queries, Hd = g.dec_heads, Pn = g.n_points, Fd = g.dim_feedforward, C = g.num_classes;
  const int BQ = B * Q, M = B * N, dh = Dd / Hd;
  if (!h->has_dec) return fail(h, DOD_ERR_STATE, "no decoder weights were registered");
  if (Dd % Hd) return fail(h, DOD_ERR_INVALID, "decoder hidden %d not divisible by heads %d", Dd, Hd);
  if (dh > 128 || dh % 4) return fail(h, DOD_ERR_INVALID, "decoder head_dim %d unsupported (<=128, multiple of 4)", dh);
  int rc;
  if (!l0_only) tap(h, 1000, mem_op, bf, (size_t)M * Dd, s);
  const bool x3 = is_x3(h) && ws.mem2;
  if (x3 && !l0_only) KCHK(h, launch_split2((const float*)mem_op, Dd, ws.mem2, M, Dd, s));   // memory-side projections as split products
  const bool l0_const = !l0_only && h->l0_tgt && (!g.use_deformable || h->l0_proj);          // layer 0's prefix comes from the pack-time constants
  if (!l0_const) KCHK(h, launch_bcast_rows(h->query, ws.tgt, 1, Q, Dd, s));                                  // K10 (image 0; broadcast after layer 0's shared part)
  int fh = 0, fw = 0;
  if (g.use_deformable && !l0_only) {
    spatial_factor(N, &fh, &fw);                                                                                // K16
    int u = 0;
    for (int j = 0; j < g.dec_layers; ++j) {                                                                    // K14 (once per distinct weight)
      DLayer& L = h->DL[j];
      if (L.vp_alias >= 0) continue;
      float* dst = ws.values + (size_t)u * M * Dd; ++u;
      if (x3 && L.vp_w2) rc = linear3(h, ws.mem2, L.vp_w2, M, Dd, Dd, epi(L.vp_b, dst, nullptr, Dd), s);
      else rc = linear(h, bf, mem_op, Dd, L.vp_w, Dd, M, Dd, Dd, epi(L.vp_b, dst, nullptr, Dd), s);
      if (rc) return rc;
    }
    tap(h, 2000, ws.values, false, (size_t)M * Dd, s);
  }
  const float sscale = 1.0f / std::sqrt((float)dh);
  // query-side linear: fp32 MFMA kernel, or (bf16 mode, large enough, N % 4 == 0) the bf16x3-split form on the bf16 kernel
  static const int qrows = DOD_TUNE_ENV("DINODET_QSPLIT_ROWS") ? atoi(DOD_TUNE_ENV("DINODET_QSPLIT_ROWS")) : 1024;
  // test option DOD_OPT_DEC_FUSED_SPLIT = 0: every query-side linear splits its own operand with a split3 launch (the round-2 schedule: the
  // bit-identity test)
  const bool fuse3 = dod_option(DOD_OPT_DEC_FUSED_SPLIT) != 0;
  // will this linear take the split form?  (then its producer writes the [hi | hi | lo] operand itself -- LayerNorm, the attention and
  // sampling kernels, the ReLU epilogue -- instead of a split3 launch over its fp32 output: 15 launches per forward)
  auto splits = [&](const bf16_t* W3, int rows, int Nout, int ldc, int act) {
    return (bf || x3) && W3 && ws.a3 && rows >= qrows && Nout >= 128 && Nout % 4 == 0 && ldc % 4 == 0 && act != ACT_SIGMOID;
  };
  // A3: the operand already in the split layout (written by the producer), or null -> split3 of A into ws.a3
  auto qlinear = [&](const float* A, int K, const float* Wf, const bf16_t* W3, int rows, int Nout, const GemmEpi& e, const bf16_t* A3 = nullptr) -> int {
    if (splits(W3, rows, Nout, e.ldc, e.act)) {
      if (!A3) { KCHK(h, launch_split3(A, K, ws.a3, rows, K, 0, s)); A3 = ws.a3; }
      return linear(h, true, A3, 3 * K, W3, 3 * K, rows, Nout, 3 * K, e, s, K);
    }
    return linear(h, false, A, K, Wf, K, rows, Nout, K, e, s);
  };
  const bf16_t* tgt3 = nullptr;      // non-null: ws.a3 holds the split form of ws.tgt (written by the LayerNorm that produced it)
  // post-norm of a sub-block: ws.t2 -> ws.tgt, also as the split operand in ws.a3 when the next reader of tgt takes the split form
  auto post_norm = [&](const float* gamma, const float* beta, int rows, bool next_splits) -> int {
    KCHK(h, launch_layernorm(ws.t2, nullptr, gamma, beta, g.dec_ln_eps, rows, Dd, ln_out(ws.tgt, nullptr, next_splits ? ws.a3 : nullptr), s));
    tgt3 = next_splits ? ws.a3 : nullptr;
    return 0;
  };
  // nb = number of images the query rows are computed for: B, or 1 in layer 0 where tgt = query_embed for every image
  // (detr_decoder.py:59), so the self-attention block and the sampling projections are image-independent there --
  // same kernels, same per-row arithmetic, computed once and broadcast (bit-identical to the per-image evaluation).
  auto self_attn = [&](const DLayer& L, int nb) -> int {                                                       // K11
    const int rows = nb * Q;
    int r = qlinear(ws.tgt, Dd, L.in_w, L.in_w3, rows, 3 * Dd, epi(L.in_b, ws.qkv, nullptr, 3 * Dd), tgt3); if (r) return r;
    tgt3 = nullptr;
    AttnF32 a; a.q = ws.qkv; a.k = ws.qkv + Dd; a.v = ws.qkv + 2 * Dd; a.o = ws.att; a.ldq = a.ldk = a.ldv = 3 * Dd; a.ldo = Dd;
    a.Lq = a.Lk = Q; a.B = nb; a.heads = Hd; a.dh = dh; a.scale = sscale;
    const bool o3 = fuse3 && splits(L.out_w3, rows, Dd, Dd, ACT_NONE);
    if (o3) a.o3 = ws.a3;
    KCHK(h, launch_attn_f32(a, s));
    r = qlinear(ws.att, Dd, L.out_w, L.out_w3, rows, Dd, epi(L.out_b, ws.t2, nullptr, Dd, ACT_NONE, nullptr, ws.tgt, Dd), o3 ? ws.a3 : nullptr); if (r) return r;
    // dense branch: the next reader of tgt is the cross-attention's query projection
    const bool n3 = fuse3 && !g.use_deformable && nb == B && splits(L.ca_q_w3, rows, Dd, Dd, ACT_NONE);
    return post_norm(L.n1w, L.n1b, rows, n3);
  };
  auto ffn = [&](const DLayer& L, bool last_layer, const bf16_t* L_next_in_w3) -> int {                         // K18
    // linear1's ReLU epilogue writes linear2's operand [hi | hi | lo] (GemmEpi::out_split) into the second operand buffer when both take
    // the split form; the fp32 ffn buffer is then not written at all
    const bool f3 = fuse3 && splits(L.l1w3, BQ, Fd, Fd, ACT_RELU) && splits(L.l2w3, BQ, Dd, Dd, ACT_NONE) && Fd % 4 == 0;
    int r;
    if (f3) {
      GemmEpi e1 = epi(L.l1b, nullptr, nullptr, 3 * Fd, ACT_RELU);
      e1.out_bf16 = ws.a3b; e1.out_split = Fd;
      r = qlinear(ws.tgt, Dd, L.l1w, L.l1w3, BQ, Fd, e1, tgt3);
    } else r = qlinear(ws.tgt, Dd, L.l1w, L.l1w3, BQ, Fd, epi(L.l1b, ws.ffn, nullptr, Fd, ACT_RELU), tgt3);
    if (r) return r;
    tgt3 = nullptr;
    r = qlinear(ws.ffn, Fd, L.l2w, L.l2w3, BQ, Dd, epi(L.l2b, ws.t2, nullptr, Dd, ACT_NONE, nullptr, ws.tgt, Dd), f3 ? ws.a3b : nullptr); if (r) return r;
    // the next split reader of tgt: the next layer's self-attention input projection (all B images from layer 1 on), or the box head
    const bool n3 = fuse3 && (last_layer ? splits(h->bb0_w3, BQ, Dd / 2, Dd / 2, ACT_RELU) : splits(L_next_in_w3, BQ, 3 * Dd, 3 * Dd, ACT_NONE));
    return post_norm(L.n3w, L.n3b, BQ, n3);
  };
  int uniq_idx[64]; { int u = 0; for (int j = 0; j < g.dec_layers && j < 64; ++j) uniq_idx[j] = h->DL[j].vp_alias < 0 ? u++ : -1; }
  for (int j = 0; j < g.dec_layers; ++j) {
    const DLayer& L = h->DL[j];
    const bool const0 = j == 0 && l0_const;          // layer 0's self-attention block (+ sampling projections): precomputed
    const bool shared0 = (j == 0 && (B > 1 || const0));          // layer 0: query rows identical for every image
    if (const0) { KCHK(h, launch_bcast_rows(h->l0_tgt, ws.tgt, B, Q, Dd, s)); tgt3 = nullptr; }
    else { rc = self_attn(L, shared0 ? 1 : B); if (rc) return rc; }
    if (g.use_deformable) {
      // K12 + K13 fused small linear, then K15 gather
      if (!const0) { rc = linear(h, false, ws.tgt, Dd, L.cat_w, Dd, shared0 ? Q : BQ, h->ncat, Dd, epi(L.cat_b, ws.proj, nullptr, h->ncat), s); if (rc) return rc; }
      if (l0_only) return DOD_OK;                                                                   // ws.tgt rows 0..Q-1 and ws.proj hold the prefix
      if (shared0 && !const0) KCHK(h, launch_bcast_rows(ws.tgt, ws.tgt + (size_t)Q * Dd, B - 1, Q, Dd, s));   // rows of image 0 -> images 1..B-1
      const int src = L.vp_alias >= 0 ? L.vp_alias : j;
      const float* vals = ws.values + (size_t)uniq_idx[src] * M * Dd;
      const bool s3 = fuse3 && splits(L.op_w3, BQ, Dd, Dd, ACT_NONE);
      KCHK(h, launch_deform_sample(const0 ? h->l0_proj : ws.proj, h->ncat, vals, B, Q, N, Hd, Pn, dh, fh, fw, ws.samp, s, shared0 ? 1 : 0, s3 ? ws.a3 : nullptr));
      rc = qlinear(ws.samp, Dd, L.op_w, L.op_w3, BQ, Dd, epi(L.op_b, ws.t2, nullptr, Dd, ACT_NONE, nullptr, ws.tgt, Dd), s3 ? ws.a3 : nullptr); if (rc) return rc;   // K17
      const bool n3 = fuse3 && splits(L.l1w3, BQ, Fd, Fd, ACT_RELU);      // next reader of tgt: linear1
      rc = post_norm(L.n2w, L.n2b, BQ, n3); if (rc) return rc;
    } else {
      // K20: dense cross-attention over all N memory tokens
      if (l0_only) return DOD_OK;
      if (shared0 && !const0) KCHK(h, launch_bcast_rows(ws.tgt, ws.tgt + (size_t)Q * Dd, B - 1, Q, Dd, s));
      rc = qlinear(ws.tgt, Dd, L.ca_q_w, L.ca_q_w3, BQ, Dd, epi(L.ca_q_b, ws.qd, nullptr, Dd), tgt3); if (rc) return rc;
      tgt3 = nullptr;
      if (x3 && L.ca_kv_w2) rc = linear3(h, ws.mem2, L.ca_kv_w2, M, 2 * Dd, Dd, epi(L.ca_kv_b, ws.kv, nullptr, 2 * Dd), s);
      else rc = linear(h, bf, mem_op, Dd, L.ca_kv_w, Dd, M, 2 * Dd, Dd, epi(L.ca_kv_b, ws.kv, nullptr, 2 * Dd), s);
      if (rc) return rc;
      AttnF32 a; a.q = ws.qd; a.k = ws.kv; a.v = ws.kv + Dd; a.o = ws.att; a.ldq = Dd; a.ldk = a.ldv = 2 * Dd; a.ldo = Dd;
      a.Lq = Q; a.Lk = N; a.B = B; a.heads = Hd; a.dh = dh; a.scale = sscale;
      const bool o3 = fuse3 && splits(L.ca_out_w3, BQ, Dd, Dd, ACT_NONE);
      if (o3) a.o3 = ws.a3;
      KCHK(h, launch_attn_f32(a, s));
      rc = qlinear(ws.att, Dd, L.ca_out_w, L.ca_out_w3, BQ, Dd, epi(L.ca_out_b, ws.t2, nullptr, Dd, ACT_NONE, nullptr, ws.tgt, Dd), o3 ? ws.a3 : nullptr); if (rc) return rc;
      const bool n3 = fuse3 && splits(L.l1w3, BQ, Fd, Fd, ACT_RELU);
      rc = post_norm(L.n2w, L.n2b, BQ, n3); if (rc) return rc;
    }
    rc = ffn(L, j + 1 == g.dec_layers, j + 1 < g.dec_layers ? h->DL[j + 1].in_w3 : nullptr); if (rc) return rc;
    tap(h, 3000 + j, ws.tgt, false, (size_t)BQ * Dd, s);
  }
  // K19 heads -> packed [B, Q, C+4]
  rc = linear(h, false, ws.tgt, Dd, h->cls_w, Dd, BQ, C, Dd, epi(h->cls_b, det, nullptr, C + 4), s); if (rc) return rc;
  rc = qlinear(ws.tgt, Dd, h->bb0_w, h->bb0_w3, BQ, Dd / 2, epi(h->bb0_b, ws.hb, nullptr, Dd / 2, ACT_RELU), tgt3); if (rc) return rc;
  rc = linear(h, false, ws.hb, Dd / 2, h->bb2_w, Dd / 2, BQ, 4, Dd / 2, epi(h->bb2_b, det + C, nullptr, C + 4, ACT_SIGMOID), s); if (rc) return rc;
  return DOD_OK;
}
