// Native training step of the decoder + heads (first slice): train-mode forward with a tape and
// the backward of DETRDecoder.forward (detr_decoder.py:47-83) -- what `loss.backward()` at train.py:1101 computes for the decoder, the
// heads and d(memory) (which then flows into the projection / LoRA blocks, tail_train.hip).  fp32 throughout (master weights, exact-fp32
// MFMA GEMMs) unless the configuration asks for DOD_PREC_BF16X3 (Ctx::mm below).  Two schedules over shared sub-blocks; every kernel and launcher is in train_ops.hip.
//
// Deformable (weight-tied DeformableDecoderLayer, deformable_attention.py:215-268, :284):
//   forward  : query tiling -> per layer { MHA self-attention (dropout on the probabilities, nn.MultiheadAttention) -> +dropout1
//              -> LN1 -> sigmoid reference points, offsets, point weights -> bilinear gather -> output_proj -> +dropout2 -> LN2
//              -> linear1 -> ReLU -> dropout3 -> linear2 -> +dropout4 -> LN3 } -> class / box heads.
//   backward : the exact adjoint of each step; weight gradients ACCUMULATE (the layers share one set of weights, and the
//              caller may accumulate over micro-batches); d(values) is a float-atomic scatter-add of the same four corners the
//              forward gathered (floor / clamp carry no gradient; torch.clamp passes it inside [0, 1] inclusive).
// Dense (the nn.TransformerDecoder branch, detr_decoder.py:28-35, 62-69; torch's TransformerDecoderLayer, post-norm, ReLU; layers untied):
//   x  = LN1(x + drop1(MHA(x, x, x)))              self-attention over the Q queries (probabilities dropped inside the MHA)
//   x  = LN2(x + drop2(MHA(x, memory, memory)))    dense cross-attention: Q queries x N memory tokens per head
//   x  = LN3(x + drop3(lin2(drop(relu(lin1(x))))))
// Dropout sites per layer: 0 self-attn probabilities, 1 dropout1, 2 dropout2, 3 the FFN's inner dropout, 4 the FFN's outer dropout, 5 the
// dense cross-attn probabilities.  Self-attention and FFN are the same sub-block in both; the middle of a layer is each decoder's own.
#include "train_internal.h"

using namespace dtrain;

namespace {

// ------------------------------------------------------------------------------------------------ what both decoders share
struct QDims { int B, N, Q, Dd, Hd, F, C, L, dh, BQ, M; };
bool make_qdims(const dod_config* c, int B, int N, QDims* d) {
  if (!c || B <= 0 || N <= 0) return false;
  d->B = B; d->N = N; d->Q = c->num_queries; d->Dd = c->dec_hidden; d->Hd = c->dec_heads; d->F = c->dim_feedforward; d->C = c->num_classes;
  d->L = c->dec_layers; d->dh = d->Dd / d->Hd; d->BQ = B * d->Q; d->M = B * N;
  return !(d->Dd % d->Hd || d->dh > 128 || d->dh % 4 || d->Dd % 4 || d->F % 4 || (d->Dd / 2) % 4 || d->Dd > 1024 || d->Q > MHA_MAXQ);
}
// one call of a step: shapes, the rate and seed both directions are given, the stream
// mm: the step's product mode (train_internal.h Mm), which every BACKWARD linear and the forward products over the B*N memory rows take.  The
// query-side FORWARD linears pass MM_F32 whatever the mode: they feed the reference points and offsets, whose floor() (deformable_attention.py:114-115)
// turns a last-bit difference into another sampling cell -- the rows eval() keeps in fp32 in every precision mode, for the same reason.
struct Ctx { QDims d; float eps, p, scale; unsigned long long seed; hipStream_t s; Mm mm; };
// gradients are written through the const-qualified structs' pointers (same layout as the parameters, float accumulators)
inline float* G(const float* q) { return const_cast<float*>(q); }

// Parameter views: the few tensors a sub-block reads, filled from dod_dec_train_params or dod_dense_layer_params -- and from `grads` the same way.
struct PostW { const float *w, *b, *norm_w, *norm_b; };      // a linear whose (dropped) output joins the residual, and the LayerNorm behind the sum
struct AttnW { const float *in_w, *in_b; PostW post; };      // self-attention: in_proj, then out_proj + LN1
struct FfnW { const float *lin1_w, *lin1_b; PostW post; };   // linear1, then linear2 + LN3
struct HeadW { const float *class_w, *class_b, *bb0_w, *bb0_b, *bb2_w, *bb2_b; };
AttnW attn_view(const dod_dec_train_params& p) { return {p.in_proj_w, p.in_proj_b, {p.out_proj_w, p.out_proj_b, p.norm1_w, p.norm1_b}}; }
AttnW attn_view(const dod_dense_layer_params& p) { return {p.sa_in_w, p.sa_in_b, {p.sa_out_w, p.sa_out_b, p.norm1_w, p.norm1_b}}; }
FfnW ffn_view(const dod_dec_train_params& p) { return {p.lin1_w, p.lin1_b, {p.lin2_w, p.lin2_b, p.norm3_w, p.norm3_b}}; }
FfnW ffn_view(const dod_dense_layer_params& p) { return {p.lin1_w, p.lin1_b, {p.lin2_w, p.lin2_b, p.norm3_w, p.norm3_b}}; }
HeadW head_view(const dod_dec_train_params& p) { return {p.class_w, p.class_b, p.bb0_w, p.bb0_b, p.bb2_w, p.bb2_b}; }
HeadW head_view(const dod_dense_dec_train_params& p) { return {p.class_w, p.class_b, p.bb0_w, p.bb0_b, p.bb2_w, p.bb2_b}; }

// Taped activations of the shared sub-blocks, and the scratch they work in (each decoder's layout extends these)
struct AttnTape { float *in, *qkv, *att, *t1, *out; };      // layer input, q | k | v, attention output, pre-norm sum, LN1 output
struct FfnTape { float *in, *hid, *t3; };                   // LN2 output, post-ReLU (pre-dropout) hidden, pre-norm sum; LN3 writes the next layer's input
struct QScratch { float *y, *dx, *dt, *dbr, *dbig, *dqkv, *dS, *Pd, *dhb, *dz; };      // dx / dt: the two d(activation) buffers a backward alternates between
void carve_attn(dod::Carver& c, const QDims& d, AttnTape* a, bool own_in = true) {      // own_in false: the caller points a->in at the layer below's output
  const size_t n = (size_t)d.BQ * d.Dd;
  a->in = own_in ? takef(c, n) : nullptr; a->qkv = takef(c, 3 * n); a->att = takef(c, n); a->t1 = takef(c, n); a->out = takef(c, n);
}

// The linear's input where the forward dropped it (the FFN's inner dropout, untaped): regenerated from x [BQ, K] into sc.y; p == 0: x itself.
// Forward and adjoint both come here, so they cannot disagree on the mask.
int dropped_input(const Ctx& c, int j, int site, const float* x, int K, const QScratch& sc, const float** xd) {
  *xd = x;
  if (c.p > 0.f) { TK(dropout_add(nullptr, x, sc.y, (size_t)c.d.BQ * K, c.p, site_key(c.seed, j, site), c.s)); *xd = sc.y; }
  return DOD_OK;
}
// out = LN(resid + dropout_site(x W^T + b)), x [BQ, K].  t receives the pre-norm sum (taped); ybuf [BQ, Dd] is clobbered.
int postnorm_fwd(const Ctx& c, int j, int site, const PostW& w, const float* x, int K, const float* resid, float* t, float* out, float* ybuf) {
  const int BQ = c.d.BQ, Dd = c.d.Dd;
  TK(lin_fwd(x, K, w.w, w.b, BQ, Dd, K, ybuf, Dd, ACT_NONE, MM_F32, c.s));
  TK(dropout_add(resid, ybuf, t, (size_t)BQ * Dd, c.p, site_key(c.seed, j, site), c.s));
  TK(launch_layernorm(t, nullptr, w.norm_w, w.norm_b, c.eps, BQ, Dd, ln_out(out), c.s));
  return DOD_OK;
}
// Its adjoint.  dy = d(out).  dt receives d(t) -- which is also the residual's gradient -- and dx [BQ, K] is WRITTEN with d(x); dx may be dy.
// in_site >= 0: the forward dropped x at that site (dropped_input).  g accumulates the gradients of w.  Clobbers sc.dbr (and sc.y with in_site).
int postnorm_bwd(const Ctx& c, int j, int site, const PostW& w, const PostW& g, const float* t, const float* x, int K, int in_site, const float* dy, float* dt,
                 float* dx, const QScratch& sc) {
  const int BQ = c.d.BQ, Dd = c.d.Dd;
  TK(ln_bwd(t, w.norm_w, dy, c.eps, BQ, Dd, dt, G(g.norm_w), G(g.norm_b), c.s));
  TK(dropout_add(nullptr, dt, sc.dbr, (size_t)BQ * Dd, c.p, site_key(c.seed, j, site), c.s));      // d(linear output)
  if (in_site >= 0) { int rc = dropped_input(c, j, in_site, x, K, sc, &x); if (rc) return rc; }
  TK(lin_bwd_w(sc.dbr, Dd, x, K, BQ, Dd, K, G(g.w), G(g.b), c.mm, c.s));
  TK(lin_bwd_x(sc.dbr, Dd, w.w, BQ, Dd, K, dx, false, c.mm, c.s));
  return DOD_OK;
}

// a.out = LN1(a.in + dropout1(out_proj(MHA(a.in)))); tapes a.qkv, a.att, a.t1.  Clobbers sc.Pd, sc.y.
int self_attn_fwd(const Ctx& c, int j, const AttnW& w, const AttnTape& a, const QScratch& sc) {
  const QDims& d = c.d;
  TK(lin_fwd(a.in, d.Dd, w.in_w, w.in_b, d.BQ, 3 * d.Dd, d.Dd, a.qkv, 3 * d.Dd, ACT_NONE, MM_F32, c.s));
  TK(launch_mha_fwd_train(a.qkv, 3 * d.Dd, a.att, d.Dd, sc.Pd, d.B, d.Q, d.Hd, d.Dd, d.dh, c.scale, c.p, site_key(c.seed, j, 0), c.s));
  return postnorm_fwd(c, j, 1, w.post, a.att, d.Dd, a.in, a.t1, a.out, sc.y);
}
// sc.dx = d(a.out) on entry; on return sc.dx (and sc.dt) = d(a.in), the d(output) of the layer below.  Clobbers sc.dbr, sc.dqkv, sc.dS, sc.Pd.
int self_attn_bwd(const Ctx& c, int j, const AttnW& w, const AttnW& g, const AttnTape& a, const QScratch& sc) {
  const QDims& d = c.d;
  int rc = postnorm_bwd(c, j, 1, w.post, g.post, a.t1, a.att, d.Dd, -1, sc.dx, sc.dt, sc.dx, sc); if (rc) return rc;      // dt = d(t1), dx = d(att)
  TK(launch_mha_bwd(a.qkv, 3 * d.Dd, sc.dx, d.Dd, sc.dqkv, sc.dS, sc.Pd, d.B, d.Q, d.Hd, d.Dd, d.dh, c.scale, c.p, site_key(c.seed, j, 0), c.s));
  TK(lin_bwd_w(sc.dqkv, 3 * d.Dd, a.in, d.Dd, d.BQ, 3 * d.Dd, d.Dd, G(g.in_w), G(g.in_b), c.mm, c.s));
  TK(lin_bwd_x(sc.dqkv, 3 * d.Dd, w.in_w, d.BQ, 3 * d.Dd, d.Dd, sc.dt, true, c.mm, c.s));                                        // dt = d(in): residual + q | k | v input
  TH(hipMemcpyAsync(sc.dx, sc.dt, (size_t)d.BQ * d.Dd * 4, hipMemcpyDeviceToDevice, c.s));
  return DOD_OK;
}

// out = LN3(f.in + dropout4(linear2(dropout3(relu(linear1(f.in)))))); tapes f.hid (post-ReLU, pre-dropout), f.t3.  Clobbers sc.y, sc.dbig.
int ffn_fwd(const Ctx& c, int j, const FfnW& w, const FfnTape& f, float* out, const QScratch& sc) {
  const QDims& d = c.d;
  TK(lin_fwd(f.in, d.Dd, w.lin1_w, w.lin1_b, d.BQ, d.F, d.Dd, f.hid, d.F, ACT_RELU, MM_F32, c.s));
  const float* hin;
  int rc = dropped_input(c, j, 3, f.hid, d.F, sc, &hin); if (rc) return rc;
  return postnorm_fwd(c, j, 4, w.post, hin, d.F, f.in, f.t3, out, sc.dbig);                                                // dbig: free during the forward
}
// sc.dx = d(out) on entry; on return sc.dt = d(f.in); sc.dx is only read.  Clobbers sc.dbr, sc.dbig, sc.y.
int ffn_bwd(const Ctx& c, int j, const FfnW& w, const FfnW& g, const FfnTape& f, const QScratch& sc) {
  const QDims& d = c.d;
  int rc = postnorm_bwd(c, j, 4, w.post, g.post, f.t3, f.hid, d.F, 3, sc.dx, sc.dt, sc.dbig, sc); if (rc) return rc;       // dt = d(t3), dbig = d(dropped hidden)
  TK(relu_drop_bwd(sc.dbig, f.hid, sc.dbig, (size_t)d.BQ * d.F, c.p, site_key(c.seed, j, 3), c.s));
  TK(lin_bwd_w(sc.dbig, d.F, f.in, d.Dd, d.BQ, d.F, d.Dd, G(g.lin1_w), G(g.lin1_b), c.mm, c.s));
  TK(lin_bwd_x(sc.dbig, d.F, w.lin1_w, d.BQ, d.F, d.Dd, sc.dt, true, c.mm, c.s));                                               // dt = d(in): residual + FFN input
  return DOD_OK;
}

// class logits and sigmoid boxes into det [BQ, C+4] (detr_decoder.py:80-81; utils.py:14-30); tapes hb (post-ReLU) and boxes.
// BQ = rows: B*Q, or L*B*Q when every layer's output is supervised (the heads are shared, so all layers go through one pass).
int heads_fwd(const Ctx& c, const HeadW& w, int BQ, const float* hs, float* hb, float* boxes, float* det) {
  const int Dd = c.d.Dd, C = c.d.C;
  TK(launch_gemm_f32(hs, Dd, w.class_w, Dd, BQ, C, Dd, gepi(w.class_b, det, C + 4), c.s));
  TK(lin_fwd(hs, Dd, w.bb0_w, w.bb0_b, BQ, Dd / 2, Dd, hb, Dd / 2, ACT_RELU, MM_F32, c.s));
  TK(launch_gemm_f32(hb, Dd / 2, w.bb2_w, Dd / 2, BQ, 4, Dd / 2, gepi(w.bb2_b, det + C, C + 4, ACT_SIGMOID), c.s));
  TK(launch_copy2d(det + C, C + 4, boxes, 4, BQ, 4, 4, c.s));
  return DOD_OK;
}
// dhs [BQ, Dd] is WRITTEN with d(hs) (BQ = rows, as heads_fwd).  Clobbers sc.dz, sc.dhb.
int heads_bwd(const Ctx& c, const HeadW& w, const HeadW& g, int BQ, const float* d_det, const float* hs, const float* hb, const float* boxes, float* dhs, const QScratch& sc) {
  const int Dd = c.d.Dd, C = c.d.C;
  TK(sigmoid_bwd4(d_det + C, C + 4, boxes, 4, sc.dz, BQ, c.s));
  TK(lin_bwd_w(sc.dz, 4, hb, Dd / 2, BQ, 4, Dd / 2, G(g.bb2_w), G(g.bb2_b), c.mm, c.s));
  TK(lin_bwd_x(sc.dz, 4, w.bb2_w, BQ, 4, Dd / 2, sc.dhb, false, c.mm, c.s));
  TK(relu_drop_bwd(sc.dhb, hb, sc.dhb, (size_t)BQ * (Dd / 2), 0.f, 0ull, c.s));
  TK(lin_bwd_w(sc.dhb, Dd / 2, hs, Dd, BQ, Dd / 2, Dd, G(g.bb0_w), G(g.bb0_b), c.mm, c.s));
  TK(lin_bwd_x(sc.dhb, Dd / 2, w.bb0_w, BQ, Dd / 2, Dd, dhs, false, c.mm, c.s));
  TK(lin_bwd_w(d_det, C + 4, hs, Dd, BQ, C, Dd, G(g.class_w), G(g.class_b), c.mm, c.s));
  TK(lin_bwd_x(d_det, C + 4, w.class_w, BQ, C, Dd, dhs, true, c.mm, c.s));
  return DOD_OK;
}

// ------------------------------------------------------------------------------------------------ deformable decoder
struct Dims : QDims { int P, ncat, ncp, fh, fw; };
bool make_dims(const dod_config* c, int B, int N, Dims* d) {
  if (!c || !c->use_deformable || !make_qdims(c, B, N, d)) return false;
  d->P = c->n_points; d->ncat = 2 + 3 * d->Hd * d->P; d->ncp = (int)up4(d->ncat);
  if (d->P > 8 || d->P < 1 || d->L < 1 || d->L > 64) return false;      // Tape::l
  int s = 1; while ((s + 1) * (s + 1) <= N) ++s;          // (h, w) of deformable_attention.py:241-256
  d->fh = s; d->fw = s;
  if (s * s != N) for (int i = s; i > 0; --i) if (N % i == 0) { d->fh = i; d->fw = N / i; break; }
  return true;
}
// nh = layers the heads see: 1 (the last layer's output only) or L (deep supervision: detections [L, B, Q, C+4]).
// hs_all [L, BQ, Dd]: slot j is layer j's LN3 output and (j + 1 < L) layer j+1's sa.in; hs = the last slot, or all nh = L of them.
struct Tape {
  float *values, *hs_all, *hb, *boxes;
  struct Layer { AttnTape sa; float *proj, *samp, *t2; FfnTape ffn; } l[64];      // sa.out = tgt1, ffn.in = tgt2
};
size_t carve_tape(const Dims& d, int nh, const void* base, Tape& tt) {
  dod::Carver c = carver(base);
  const size_t BQ = d.BQ, Dd = d.Dd;
  tt.values = takef(c, (size_t)d.M * Dd); tt.hs_all = takef(c, d.L * BQ * Dd); tt.hb = takef(c, nh * BQ * (Dd / 2)); tt.boxes = takef(c, nh * BQ * 4);
  for (int j = 0; j < d.L; ++j) {
    auto& L = tt.l[j];
    carve_attn(c, d, &L.sa, j == 0);
    if (j && tt.hs_all) L.sa.in = tt.hs_all + (j - 1) * BQ * Dd;
    L.proj = takef(c, BQ * d.ncp); L.samp = takef(c, BQ * Dd); L.t2 = takef(c, BQ * Dd);
    L.ffn.in = takef(c, BQ * Dd); L.ffn.hid = takef(c, BQ * (size_t)d.F); L.ffn.t3 = takef(c, BQ * Dd);
  }
  return c.off;
}
struct Scratch : QScratch {
  float *cat_w, *cat_b;                                     // fused [ref | offsets | weights] linear
  float *dproj, *dcat_w, *dcat_b, *dvalues;                 // backward
  float *dhs;                                               // d(hs_all) [nh, BQ, Dd]; its LAST slot is dx, where the layer loop starts
};
size_t carve_scratch(const Dims& d, int nh, const void* base, Scratch& s) {
  dod::Carver c = carver(base);
  const size_t BQ = d.BQ, Dd = d.Dd, F = d.F, M = d.M;
  const size_t maxcols = (size_t)(3 * Dd > F ? 3 * Dd : F);           // widest activation of the query side
  s.y = takef(c, BQ * maxcols); s.cat_w = takef(c, (size_t)d.ncp * Dd); s.cat_b = takef(c, d.ncp);
  s.dhs = takef(c, nh * BQ * Dd); s.dx = s.dhs ? s.dhs + (nh - 1) * BQ * Dd : nullptr;
  s.dt = takef(c, BQ * Dd); s.dbr = takef(c, BQ * Dd); s.dbig = takef(c, BQ * maxcols); s.dproj = takef(c, BQ * d.ncp);
  s.dcat_w = takef(c, (size_t)d.ncp * Dd); s.dcat_b = takef(c, d.ncp); s.dqkv = takef(c, BQ * 3 * Dd);
  s.dS = takef(c, mha_scratch_floats(d.B, d.Hd, d.Q, d.Q)); s.Pd = takef(c, mha_scratch_floats(d.B, d.Hd, d.Q, d.Q));
  s.dvalues = takef(c, M * Dd); s.dhb = takef(c, nh * BQ * (Dd / 2)); s.dz = takef(c, nh * BQ * 4);
  return c.off;
}
int build_cat(const Dims& d, const dod_dec_train_params* p, const Scratch& sc, hipStream_t s) {
  const int Dd = d.Dd, HP = d.Hd * d.P;
  TH(hipMemsetAsync(sc.cat_w, 0, (size_t)d.ncp * Dd * 4, s));
  TH(hipMemsetAsync(sc.cat_b, 0, (size_t)d.ncp * 4, s));
  TH(hipMemcpyAsync(sc.cat_w, p->refp_w, (size_t)2 * Dd * 4, hipMemcpyDeviceToDevice, s));
  TH(hipMemcpyAsync(sc.cat_w + (size_t)2 * Dd, p->off_w, (size_t)HP * 2 * Dd * 4, hipMemcpyDeviceToDevice, s));
  TH(hipMemcpyAsync(sc.cat_w + (size_t)(2 + HP * 2) * Dd, p->aw_w, (size_t)HP * Dd * 4, hipMemcpyDeviceToDevice, s));
  TH(hipMemcpyAsync(sc.cat_b, p->refp_b, 2 * 4, hipMemcpyDeviceToDevice, s));
  TH(hipMemcpyAsync(sc.cat_b + 2, p->off_b, (size_t)HP * 2 * 4, hipMemcpyDeviceToDevice, s));
  TH(hipMemcpyAsync(sc.cat_b + 2 + HP * 2, p->aw_b, (size_t)HP * 4, hipMemcpyDeviceToDevice, s));
  return 0;
}

// The deformable step, for both forms of supervision.  aux: the heads run over every layer's output -- det / d_det are [L, B, Q, C+4],
// slice j = decoder layer j, slice L-1 = what the plain step returns -- and d(layer j's output) gains d_hs_all[j] on the way down.
int deform_forward(const dod_config* cfg, bool aux, const dod_dec_train_params* p, const float* memory, int B, int N, float dropout_p, uint64_t seed, float* det,
                   void* tape, size_t tape_bytes, void* ws, size_t ws_bytes, void* stream) {
  Dims d;
  if (!make_dims(cfg, B, N, &d)) return dod_fail(DOD_ERR_INVALID, "decoder train: unsupported configuration (deformable branch, head_dim <= 128, Dd <= 1024, Q <= %d)", MHA_MAXQ);
  const int nh = aux ? d.L : 1;
  Tape t; Scratch sc;      // carved first: the carve itself says how many bytes each buffer must hold
  int rc = entry_check("decoder train", p && memory && det && tape && ws, dropout_p, tape_bytes, carve_tape(d, nh, tape, t) + 256, ws_bytes, carve_scratch(d, nh, ws, sc) + 256); if (rc) return rc;
  const Ctx c = {d, cfg->dec_ln_eps, dropout_p, 1.0f / sqrtf((float)d.dh), seed, (hipStream_t)stream, mm_of(cfg)};
  hipStream_t s = c.s;
  const int BQ = d.BQ, Dd = d.Dd, Q = d.Q;
  const AttnW aw = attn_view(*p);
  const FfnW fw = ffn_view(*p);
  const PostW ow = {p->op_w, p->op_b, p->norm2_w, p->norm2_b};
  rc = build_cat(d, p, sc, s); if (rc) return rc;
  TK(lin_fwd(memory, Dd, p->vp_w, p->vp_b, d.M, Dd, Dd, t.values, Dd, ACT_NONE, c.mm, s));                       // tied layers: once.  The B*N memory rows: the step's mode
  TK(launch_bcast_rows(p->query_embed, t.l[0].sa.in, B, Q, Dd, s));
  for (int j = 0; j < d.L; ++j) {
    auto& L = t.l[j];
    rc = self_attn_fwd(c, j, aw, L.sa, sc); if (rc) return rc;
    // reference points, offsets, point weights -> bilinear gather -> output_proj -> +dropout2 -> LN2
    TH(hipMemsetAsync(L.proj, 0, (size_t)BQ * d.ncp * 4, s));
    TK(launch_gemm_f32(L.sa.out, Dd, sc.cat_w, Dd, BQ, d.ncat, Dd, gepi(sc.cat_b, L.proj, d.ncp), s));
    TK(launch_deform_sample(L.proj, d.ncp, t.values, B, Q, N, d.Hd, d.P, d.dh, d.fh, d.fw, L.samp, s, 0));
    rc = postnorm_fwd(c, j, 2, ow, L.samp, Dd, L.sa.out, L.t2, L.ffn.in, sc.y); if (rc) return rc;
    rc = ffn_fwd(c, j, fw, L.ffn, t.hs_all + (size_t)j * BQ * Dd, sc); if (rc) return rc;               // = layer j+1's sa.in
  }
  return heads_fwd(c, head_view(*p), nh * BQ, t.hs_all + (size_t)(d.L - nh) * BQ * Dd, t.hb, t.boxes, det);
}

int deform_backward(const dod_config* cfg, bool aux, const dod_dec_train_params* p, const float* memory, int B, int N, float dropout_p, uint64_t seed,
                    const float* d_det, const void* tape, size_t tape_bytes, const dod_dec_train_params* grads, float* d_memory, void* ws, size_t ws_bytes,
                    void* stream) {
  Dims d;
  if (!make_dims(cfg, B, N, &d)) return dod_fail(DOD_ERR_INVALID, "decoder train: unsupported configuration");
  const int nh = aux ? d.L : 1;
  Tape t; Scratch sc;      // carved first: the carve itself says how many bytes each buffer must hold
  int rc = entry_check("decoder train", p && memory && d_det && tape && grads && ws, 0.f, tape_bytes, carve_tape(d, nh, tape, t) + 256, ws_bytes, carve_scratch(d, nh, ws, sc) + 256); if (rc) return rc;
  const Ctx c = {d, cfg->dec_ln_eps, dropout_p, 1.0f / sqrtf((float)d.dh), seed, (hipStream_t)stream, mm_of(cfg)};
  hipStream_t s = c.s;
  const int BQ = d.BQ, Dd = d.Dd, Q = d.Q, HP = d.Hd * d.P;
  // weights tied: every layer adds into the same gradient tensors
  const AttnW aw = attn_view(*p), ag = attn_view(*grads);
  const FfnW fw = ffn_view(*p), fg = ffn_view(*grads);
  const PostW ow = {p->op_w, p->op_b, p->norm2_w, p->norm2_b}, og = {grads->op_w, grads->op_b, grads->norm2_w, grads->norm2_b};
  rc = build_cat(d, p, sc, s); if (rc) return rc;
  TH(hipMemsetAsync(sc.dcat_w, 0, (size_t)d.ncp * Dd * 4, s));
  TH(hipMemsetAsync(sc.dcat_b, 0, (size_t)d.ncp * 4, s));
  TH(hipMemsetAsync(sc.dvalues, 0, (size_t)d.M * Dd * 4, s));
  // one pass over the nh * BQ supervised rows; the last slot of dhs is dx = d(last layer's output)
  rc = heads_bwd(c, head_view(*p), head_view(*grads), nh * BQ, d_det, t.hs_all + (size_t)(d.L - nh) * BQ * Dd, t.hb, t.boxes, sc.dhs, sc); if (rc) return rc;
  for (int j = d.L - 1; j >= 0; --j) {
    const auto& L = t.l[j];
    if (aux && j + 1 < d.L) TK(add_inplace(sc.dx, sc.dhs + (size_t)j * BQ * Dd, (size_t)BQ * Dd, s));             // + the heads' own d(layer j's output)
    rc = ffn_bwd(c, j, fw, fg, L.ffn, sc); if (rc) return rc;                                                   // dt = d(tgt2)
    // LN2 <- tgt1 + dropout2(output_proj(samp)): dx = d(t2), dt = d(samp)
    rc = postnorm_bwd(c, j, 2, ow, og, L.t2, L.samp, Dd, -1, sc.dt, sc.dx, sc.dt, sc); if (rc) return rc;
    TH(hipMemsetAsync(sc.dproj, 0, (size_t)BQ * d.ncp * 4, s));
    rc = launch_deform_bwd(L.proj, d.ncp, t.values, sc.dt, B, Q, N, d.Hd, d.P, d.dh, d.fh, d.fw, sc.dproj, sc.dvalues, s); if (rc) return rc;
    TK(lin_bwd_w(sc.dproj, d.ncp, L.sa.out, Dd, BQ, d.ncat, Dd, sc.dcat_w, sc.dcat_b, c.mm, s));
    TK(lin_bwd_x(sc.dproj, d.ncp, sc.cat_w, BQ, d.ncat, Dd, sc.dx, true, c.mm, s));                                   // dx = d(tgt1)
    rc = self_attn_bwd(c, j, aw, ag, L.sa, sc); if (rc) return rc;                                              // dx = d(tgt_in)
  }
  TK(batch_sum(sc.dx, G(grads->query_embed), B, (size_t)Q * Dd, s));      // tgt_0[b] = query_embed for every image (detr_decoder.py:59)
  // fused small linear -> its three parameters
  float* dw = sc.dcat_w; float* dbv = sc.dcat_b;
  TK(add_inplace(G(grads->refp_w), dw, (size_t)2 * Dd, s));
  TK(add_inplace(G(grads->off_w), dw + (size_t)2 * Dd, (size_t)HP * 2 * Dd, s));
  TK(add_inplace(G(grads->aw_w), dw + (size_t)(2 + HP * 2) * Dd, (size_t)HP * Dd, s));
  TK(add_inplace(G(grads->refp_b), dbv, 2, s));
  TK(add_inplace(G(grads->off_b), dbv + 2, (size_t)HP * 2, s));
  TK(add_inplace(G(grads->aw_b), dbv + 2 + HP * 2, (size_t)HP, s));
  // value projection (computed once for the tied layers: d(values) is the sum over layers)
  TK(lin_bwd_w(sc.dvalues, Dd, memory, Dd, d.M, Dd, Dd, G(grads->vp_w), G(grads->vp_b), c.mm, s));
  if (d_memory) TK(lin_bwd_x(sc.dvalues, Dd, p->vp_w, d.M, Dd, Dd, d_memory, false, c.mm, s));
  return DOD_OK;
}
size_t deform_bytes(const dod_config* cfg, bool aux, bool tape, int B, int N) {
  Dims d; Tape t; Scratch sc; if (!make_dims(cfg, B, N, &d)) return 0;
  return (tape ? carve_tape(d, aux ? d.L : 1, nullptr, t) : carve_scratch(d, aux ? d.L : 1, nullptr, sc)) + 256;
}

}  // namespace

extern "C" {

size_t dod_decoder_train_tape_bytes(const dod_config* cfg, int B, int N) { return deform_bytes(cfg, false, true, B, N); }
size_t dod_decoder_train_workspace_bytes(const dod_config* cfg, int B, int N) { return deform_bytes(cfg, false, false, B, N); }
size_t dod_decoder_train_aux_tape_bytes(const dod_config* cfg, int B, int N) { return deform_bytes(cfg, true, true, B, N); }
size_t dod_decoder_train_aux_workspace_bytes(const dod_config* cfg, int B, int N) { return deform_bytes(cfg, true, false, B, N); }

int dod_decoder_train_forward(const dod_config* cfg, const dod_dec_train_params* p, const float* memory, int B, int N, float dropout_p,
                              uint64_t seed, float* det, void* tape, size_t tape_bytes, void* ws, size_t ws_bytes, void* stream) {
  return deform_forward(cfg, false, p, memory, B, N, dropout_p, seed, det, tape, tape_bytes, ws, ws_bytes, stream);
}
int dod_decoder_train_backward(const dod_config* cfg, const dod_dec_train_params* p, const float* memory, int B, int N, float dropout_p,
                               uint64_t seed, const float* d_det, const void* tape, size_t tape_bytes, const dod_dec_train_params* grads,
                               float* d_memory, void* ws, size_t ws_bytes, void* stream) {
  return deform_backward(cfg, false, p, memory, B, N, dropout_p, seed, d_det, tape, tape_bytes, grads, d_memory, ws, ws_bytes, stream);
}
int dod_decoder_train_aux_forward(const dod_config* cfg, const dod_dec_train_params* p, const float* memory, int B, int N, float dropout_p,
                                  uint64_t seed, float* det, void* tape, size_t tape_bytes, void* ws, size_t ws_bytes, void* stream) {
  return deform_forward(cfg, true, p, memory, B, N, dropout_p, seed, det, tape, tape_bytes, ws, ws_bytes, stream);
}
int dod_decoder_train_aux_backward(const dod_config* cfg, const dod_dec_train_params* p, const float* memory, int B, int N, float dropout_p,
                                   uint64_t seed, const float* d_det, const void* tape, size_t tape_bytes, const dod_dec_train_params* grads,
                                   float* d_memory, void* ws, size_t ws_bytes, void* stream) {
  return deform_backward(cfg, true, p, memory, B, N, dropout_p, seed, d_det, tape, tape_bytes, grads, d_memory, ws, ws_bytes, stream);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ dense decoder
namespace {

bool make_ddims(const dod_config* c, int B, int N, QDims* d) { return c && !c->use_deformable && make_qdims(c, B, N, d) && N <= MHA_MAXQ && d->L >= 1 && d->L <= 16; }
struct DTape {
  float *hs, *hb, *boxes;
  struct Layer { AttnTape sa; float *cq, *ckv, *catt, *t2; FfnTape ffn; } l[16];      // sa.out = x1, ffn.in = x2
};
size_t carve_dtape(const QDims& d, const void* base, DTape& tt) {
  dod::Carver c = carver(base);
  const size_t BQ = d.BQ, Dd = d.Dd;
  tt.hs = takef(c, BQ * Dd); tt.hb = takef(c, BQ * (Dd / 2)); tt.boxes = takef(c, BQ * 4);
  for (int j = 0; j < d.L; ++j) {
    auto& L = tt.l[j];
    carve_attn(c, d, &L.sa);
    L.cq = takef(c, BQ * Dd); L.ckv = takef(c, (size_t)d.M * 2 * Dd); L.catt = takef(c, BQ * Dd); L.t2 = takef(c, BQ * Dd);
    L.ffn.in = takef(c, BQ * Dd); L.ffn.hid = takef(c, BQ * (size_t)d.F); L.ffn.t3 = takef(c, BQ * Dd);
  }
  return c.off;
}
struct DScratch : QScratch { float *dcq, *dckv, *dmem; };
size_t carve_dscratch(const QDims& d, const void* base, DScratch& s) {
  dod::Carver c = carver(base);
  const size_t BQ = d.BQ, Dd = d.Dd, F = d.F;
  const size_t maxcols = (size_t)(3 * Dd > F ? 3 * Dd : F);
  const size_t sq = mha_scratch_floats(d.B, d.Hd, d.Q, d.Q), sr = mha_scratch_floats(d.B, d.Hd, d.Q, d.N);
  s.y = takef(c, BQ * maxcols); s.dx = takef(c, BQ * Dd); s.dt = takef(c, BQ * Dd); s.dbr = takef(c, BQ * Dd); s.dbig = takef(c, BQ * maxcols);
  s.dqkv = takef(c, BQ * 3 * Dd); s.dcq = takef(c, BQ * Dd); s.dckv = takef(c, (size_t)d.M * 2 * Dd);
  s.dS = takef(c, sq > sr ? sq : sr); s.Pd = takef(c, sq > sr ? sq : sr); s.dhb = takef(c, BQ * (Dd / 2)); s.dz = takef(c, BQ * 4);
  s.dmem = takef(c, (size_t)d.M * Dd);
  return c.off;
}
bool dense_params_ok(const dod_dense_dec_train_params* p, int L) { return p && p->layers && p->nlayers == L; }      // else: reported with the null buffers

}  // namespace

extern "C" {

size_t dod_dense_decoder_train_tape_bytes(const dod_config* cfg, int B, int N) {
  QDims d; DTape t; if (!make_ddims(cfg, B, N, &d)) return 0;
  return carve_dtape(d, nullptr, t) + 256;
}
size_t dod_dense_decoder_train_workspace_bytes(const dod_config* cfg, int B, int N) {
  QDims d; DScratch sc; if (!make_ddims(cfg, B, N, &d)) return 0;
  return carve_dscratch(d, nullptr, sc) + 256;
}

int dod_dense_decoder_train_forward(const dod_config* cfg, const dod_dense_dec_train_params* p, const float* memory, int B, int N, float dropout_p,
                                    uint64_t seed, float* det, void* tape, size_t tape_bytes, void* ws, size_t ws_bytes, void* stream) {
  QDims d;
  if (!make_ddims(cfg, B, N, &d)) return dod_fail(DOD_ERR_INVALID, "dense decoder train: unsupported configuration (nn.TransformerDecoder branch, head_dim <= 128, Dd <= 1024, Q and N <= %d, <= 16 layers)", MHA_MAXQ);
  DTape t; DScratch sc;      // carved first: the carve itself says how many bytes each buffer must hold
  int rc = entry_check("dense decoder train", dense_params_ok(p, d.L) && memory && det && tape && ws, dropout_p, tape_bytes, carve_dtape(d, tape, t) + 256, ws_bytes,
                       carve_dscratch(d, ws, sc) + 256); if (rc) return rc;
  const Ctx c = {d, cfg->dec_ln_eps, dropout_p, 1.0f / sqrtf((float)d.dh), seed, (hipStream_t)stream, mm_of(cfg)};
  hipStream_t s = c.s;
  const int BQ = d.BQ, Dd = d.Dd, Q = d.Q;
  TK(launch_bcast_rows(p->query_embed, t.l[0].sa.in, B, Q, Dd, s));
  for (int j = 0; j < d.L; ++j) {
    const dod_dense_layer_params& W = p->layers[j];
    auto& L = t.l[j];
    rc = self_attn_fwd(c, j, attn_view(W), L.sa, sc); if (rc) return rc;
    // dense cross-attention: q from the queries, k | v from the memory (in_proj rows 0..Dd-1 / Dd..3Dd-1)
    TK(lin_fwd(L.sa.out, Dd, W.ca_in_w, W.ca_in_b, BQ, Dd, Dd, L.cq, Dd, ACT_NONE, MM_F32, s));
    TK(lin_fwd(memory, Dd, W.ca_in_w + (size_t)Dd * Dd, W.ca_in_b + Dd, d.M, 2 * Dd, Dd, L.ckv, 2 * Dd, ACT_NONE, c.mm, s));      // the B*N memory rows: the step's mode
    TK(launch_mha_fwd_rect(L.cq, Dd, L.ckv, L.ckv + Dd, 2 * Dd, L.catt, Dd, sc.Pd, B, Q, N, d.Hd, d.dh, c.scale, dropout_p, site_key(seed, j, 5), s));
    rc = postnorm_fwd(c, j, 2, {W.ca_out_w, W.ca_out_b, W.norm2_w, W.norm2_b}, L.catt, Dd, L.sa.out, L.t2, L.ffn.in, sc.y); if (rc) return rc;
    rc = ffn_fwd(c, j, ffn_view(W), L.ffn, j + 1 < d.L ? t.l[j + 1].sa.in : t.hs, sc); if (rc) return rc;
  }
  return heads_fwd(c, head_view(*p), BQ, t.hs, t.hb, t.boxes, det);
}

int dod_dense_decoder_train_backward(const dod_config* cfg, const dod_dense_dec_train_params* p, const float* memory, int B, int N, float dropout_p,
                                     uint64_t seed, const float* d_det, const void* tape, size_t tape_bytes, const dod_dense_dec_train_params* grads,
                                     float* d_memory, void* ws, size_t ws_bytes, void* stream) {
  QDims d;
  if (!make_ddims(cfg, B, N, &d)) return dod_fail(DOD_ERR_INVALID, "dense decoder train: unsupported configuration");
  DTape t; DScratch sc;      // carved first: the carve itself says how many bytes each buffer must hold
  int rc = entry_check("dense decoder train", dense_params_ok(p, d.L) && dense_params_ok(grads, d.L) && memory && d_det && tape && ws, 0.f, tape_bytes,
                       carve_dtape(d, tape, t) + 256, ws_bytes, carve_dscratch(d, ws, sc) + 256); if (rc) return rc;
  const Ctx c = {d, cfg->dec_ln_eps, dropout_p, 1.0f / sqrtf((float)d.dh), seed, (hipStream_t)stream, mm_of(cfg)};
  hipStream_t s = c.s;
  const int BQ = d.BQ, Dd = d.Dd, Q = d.Q;
  float* dmem = d_memory ? d_memory : sc.dmem;                 // d(memory): the sum over the layers' k | v projections
  TH(hipMemsetAsync(dmem, 0, (size_t)d.M * Dd * 4, s));
  rc = heads_bwd(c, head_view(*p), head_view(*grads), BQ, d_det, t.hs, t.hb, t.boxes, sc.dx, sc); if (rc) return rc;      // dx = d(last layer's output)
  for (int j = d.L - 1; j >= 0; --j) {
    const dod_dense_layer_params& W = p->layers[j];
    const dod_dense_layer_params& Gw = grads->layers[j];
    const auto& L = t.l[j];
    rc = ffn_bwd(c, j, ffn_view(W), ffn_view(Gw), L.ffn, sc); if (rc) return rc;                                // dt = d(x2)
    // LN2 <- x1 + drop2(ca_out(catt)): dx = d(t2), dt = d(catt)
    rc = postnorm_bwd(c, j, 2, {W.ca_out_w, W.ca_out_b, W.norm2_w, W.norm2_b}, {Gw.ca_out_w, Gw.ca_out_b, Gw.norm2_w, Gw.norm2_b}, L.t2, L.catt, Dd, -1,
                      sc.dt, sc.dx, sc.dt, sc);
    if (rc) return rc;
    TK(launch_mha_bwd_rect(L.cq, Dd, L.ckv, L.ckv + Dd, 2 * Dd, sc.dt, Dd, sc.dcq, Dd, sc.dckv, sc.dckv + Dd, 2 * Dd, sc.dS, sc.Pd, B, Q, N, d.Hd, d.dh,
                           c.scale, dropout_p, site_key(seed, j, 5), s));
    // in_proj of the cross-attention: rows 0..Dd-1 see the queries, rows Dd..3Dd-1 the memory
    TK(lin_bwd_w(sc.dcq, Dd, L.sa.out, Dd, BQ, Dd, Dd, G(Gw.ca_in_w), G(Gw.ca_in_b), c.mm, s));
    TK(lin_bwd_w(sc.dckv, 2 * Dd, memory, Dd, d.M, 2 * Dd, Dd, G(Gw.ca_in_w) + (size_t)Dd * Dd, G(Gw.ca_in_b) + Dd, c.mm, s));
    TK(lin_bwd_x(sc.dckv, 2 * Dd, W.ca_in_w + (size_t)Dd * Dd, d.M, 2 * Dd, Dd, dmem, true, c.mm, s));                // d(memory) += d(k | v) W_kv
    TK(lin_bwd_x(sc.dcq, Dd, W.ca_in_w, BQ, Dd, Dd, sc.dx, true, c.mm, s));                                           // dx = d(x1): residual + query input
    rc = self_attn_bwd(c, j, attn_view(W), attn_view(Gw), L.sa, sc); if (rc) return rc;                         // dx = d(x_in)
  }
  TK(batch_sum(sc.dx, G(grads->query_embed), B, (size_t)Q * Dd, s));      // x_0[b] = query_embed for every image (detr_decoder.py:59)
  return DOD_OK;
}

}  // extern "C"
