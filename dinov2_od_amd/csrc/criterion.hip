// Set-prediction loss on device: SetCriterion.forward of dino_detector/losses.py:204-242 (loss_labels :100-146,
// loss_boxes :148-185) and its gradient, for the whole batch, given the Hungarian assignment as a per-query match table.
//   row r = b*Q + q, m = match[r] (a global target row, or -1 = background)
//   t[r, c]    = (m valid and labels[m] == c)  for c < C; a label of C (the dropped one-hot column, :125-128) or outside
//                [0, C] is background -- never an address
//   loss_ce    = sum_{r,c} a_t (1 - p_t)^gamma bce(x, t) / max(num_boxes, 1)                               :130-138
//                p = sigmoid(x), p_t = t ? p : 1 - p, a_t = t ? alpha : 1 - alpha,
//                bce = max(x, 0) - x t + log1p(exp(-|x|))   (binary_cross_entropy_with_logits)
//   loss_bbox  = sum_{matched r} |pred_r - gt_m|_1 / max(num_boxes, 1)                                       :170-171
//   loss_giou  = sum_{matched r} (1 - giou(xyxy(pred_r), xyxy(gt_m))) / max(num_boxes, 1)                  :174-178
// Forward: one wave64 per row striding over C, the matched pair's L1 / GIoU on lane 0 of the same wave; each workgroup
// writes ONE partial per loss, a one-workgroup launch sums the partials in a fixed order and divides by the device-resident
// normaliser.  No atomics, no cross-workgroup handoff: bit-identical from run to run.
// Backward: one launch, recomputed from the inputs (no tape), scaled by the upstream d_losses[3] read from device memory;
// the tie rules are those of torch autograd on the reference formula (maximum / minimum of equal values: half to each
// side; clamp(min=0) passes at 0; l1_loss: 0 where pred == target; (1 - p_t)**0 has no pow gradient).
// The same row kernel serves FocalLoss (losses.py:9-68): match == NULL means "row r's target is labels[r]", pred_boxes ==
// NULL skips the box terms, num_boxes == NULL normalises by 1, elem_loss / d_elem carry reduction='none': elem_loss is the
// un-normalised term and d_elem its upstream gradient, neither divided by num_boxes (only the d_losses path is).
// Layered form (deep supervision: `layers` decoder outputs against the same targets): rows r = (l*B + b)*Q + q, each layer has
// its own ceil(B*Q / 16) workgroups, partials and finalize workgroup, so layer l's losses and gradients are bit-identical to
// the single-layer call on that layer's slice; still two launches forward, one backward.
#include "dod_common.h"
#include "../../include/dinodet.h"

namespace {

constexpr int kWaves = 4;                      // waves per workgroup
constexpr int kRowsPerWave = 4;
constexpr int kRowsPerWg = kWaves * kRowsPerWave;

struct CritArgs {
  const float* logits; long long ls;           // row r's logits at logits + r * ls
  const float* boxes; long long bs;            // row r's (cx, cy, w, h) at boxes + r * bs, or NULL
  int R, C, G;                                 // R = rows of ONE layer; layer l's rows are l * R + (0 .. R-1)
  int wgl;                                     // workgroups per layer: a workgroup never straddles a layer
  const long long* labels;                     // [G]
  const float* gt;                             // [G, 4] cxcywh
  const int* match;                            // [R], or NULL = identity
  const float* num_boxes;                      // device scalar, or NULL = 1
  float alpha, gamma;
};

__device__ __forceinline__ int crit_target(const CritArgs& a, long long r) {
  return a.match ? a.match[r] : (int)r;
}

// class column of row r, -1 = background (no target, or a label outside [0, C))
__device__ __forceinline__ int crit_class(const CritArgs& a, int m) {
  if (m < 0 || m >= a.G) return -1;
  const long long lab = a.labels[m];
  return (lab >= 0 && lab < a.C) ? (int)lab : -1;
}

__device__ __forceinline__ float crit_norm(const CritArgs& a) {
  return a.num_boxes ? fmaxf(a.num_boxes[0], 1.0f) : 1.0f;
}

__device__ __forceinline__ float focal_pow(float base, float gamma) {
  return gamma == 2.0f ? base * base : powf(base, gamma);
}

__device__ __forceinline__ float bce_logits(float x, float t) {
  return fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
}

// a_t (1 - p_t)^gamma bce
__device__ __forceinline__ float focal_elem(float x, bool pos, float alpha, float gamma) {
  const float p = 1.0f / (1.0f + expf(-x));
  const float t = pos ? 1.f : 0.f;
  const float w = pos ? 1.f - p : p;                     // 1 - p_t
  const float at = pos ? alpha : 1.f - alpha;
  return at * focal_pow(w, gamma) * bce_logits(x, t);
}

// d/dx of focal_elem: a_t [gamma (1-p_t)^(gamma-1) (-(2t-1) p (1-p)) bce + (1-p_t)^gamma (p - t)]
__device__ __forceinline__ float focal_grad(float x, bool pos, float alpha, float gamma) {
  const float p = 1.0f / (1.0f + expf(-x));
  const float t = pos ? 1.f : 0.f;
  const float w = pos ? 1.f - p : p;
  const float at = pos ? alpha : 1.f - alpha;
  float dpow = 0.f;                                      // gamma == 0: no pow gradient; base 0: the p (1-p) factor is 0 too
  if (gamma != 0.f && w != 0.f) {
    const float wg1 = gamma == 2.0f ? w : powf(w, gamma - 1.f);
    dpow = gamma * wg1 * (-(2.f * t - 1.f) * p * (1.f - p)) * bce_logits(x, t);
  }
  return at * (dpow + focal_pow(w, gamma) * (p - t));
}

// torch.maximum / torch.minimum backward: the share of the gradient that reaches `a`
__device__ __forceinline__ float max_share(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }
__device__ __forceinline__ float min_share(float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); }

struct Giou {
  float ax1, ay1, ax2, ay2, bx1, by1, bx2, by2;
  float iwr, ihr, iw, ih, inter, uni, ewr, ehr, ew, eh, earea, giou;
};

// generalized_box_iou (utils.py:124-164) of one pair, boxes in cxcywh (box_cxcywh_to_xyxy, utils.py:73-88)
__device__ __forceinline__ Giou giou_pair(const float* p, const float* t) {
  Giou s;
  s.ax1 = p[0] - 0.5f * p[2]; s.ay1 = p[1] - 0.5f * p[3]; s.ax2 = p[0] + 0.5f * p[2]; s.ay2 = p[1] + 0.5f * p[3];
  s.bx1 = t[0] - 0.5f * t[2]; s.by1 = t[1] - 0.5f * t[3]; s.bx2 = t[0] + 0.5f * t[2]; s.by2 = t[1] + 0.5f * t[3];
  const float area1 = (s.ax2 - s.ax1) * (s.ay2 - s.ay1), area2 = (s.bx2 - s.bx1) * (s.by2 - s.by1);
  s.iwr = fminf(s.ax2, s.bx2) - fmaxf(s.ax1, s.bx1);
  s.ihr = fminf(s.ay2, s.by2) - fmaxf(s.ay1, s.by1);
  s.iw = fmaxf(s.iwr, 0.f); s.ih = fmaxf(s.ihr, 0.f);
  s.inter = s.iw * s.ih;
  s.uni = area1 + area2 - s.inter;
  s.ewr = fmaxf(s.ax2, s.bx2) - fminf(s.ax1, s.bx1);
  s.ehr = fmaxf(s.ay2, s.by2) - fminf(s.ay1, s.by1);
  s.ew = fmaxf(s.ewr, 0.f); s.eh = fmaxf(s.ehr, 0.f);
  s.earea = s.ew * s.eh;
  s.giou = s.inter / s.uni - (s.earea - s.uni) / s.earea;
  return s;
}

// dp[0..3] = g * d giou / d (cx, cy, w, h) of the prediction, with torch autograd's tie rules
__device__ __forceinline__ void giou_pair_grad(const float* p, const float* t, float g, float* dp) {
  const Giou s = giou_pair(p, t);
  // giou = I / U - N / E, N = E - U
  const float N = s.earea - s.uni;
  const float gT = -g;
  const float gN = gT / s.earea;
  const float gE = -gT * N / (s.earea * s.earea) + gN;
  float gU = -gN - g * s.inter / (s.uni * s.uni);
  const float gI = g / s.uni - gU;                       // U = A1 + A2 - I
  const float gA1 = gU;
  // I = iw * ih, clamp(min=0) passes at 0
  const float giw = s.iwr >= 0.f ? gI * s.ih : 0.f, gih = s.ihr >= 0.f ? gI * s.iw : 0.f;
  // E = ew * eh
  const float gew = s.ewr >= 0.f ? gE * s.eh : 0.f, geh = s.ehr >= 0.f ? gE * s.ew : 0.f;
  // A1 = (ax2 - ax1) (ay2 - ay1)
  const float gdx = gA1 * (s.ay2 - s.ay1), gdy = gA1 * (s.ax2 - s.ax1);
  const float gx2 = gdx + giw * min_share(s.ax2, s.bx2) + gew * max_share(s.ax2, s.bx2);
  const float gx1 = -gdx - giw * max_share(s.ax1, s.bx1) - gew * min_share(s.ax1, s.bx1);
  const float gy2 = gdy + gih * min_share(s.ay2, s.by2) + geh * max_share(s.ay2, s.by2);
  const float gy1 = -gdy - gih * max_share(s.ay1, s.by1) - geh * min_share(s.ay1, s.by1);
  dp[0] = gx1 + gx2;
  dp[1] = gy1 + gy2;
  dp[2] = 0.5f * (gx2 - gx1);
  dp[3] = 0.5f * (gy2 - gy1);
}

__device__ __forceinline__ float l1_sign(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

__global__ __launch_bounds__(256) void crit_forward_kernel(CritArgs a, float* __restrict__ part, float* __restrict__ elem) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float ce = 0.f, l1 = 0.f, gi = 0.f;
  const int layer = blockIdx.x / a.wgl, lwg = blockIdx.x - layer * a.wgl;
  for (int k = 0; k < kRowsPerWave; ++k) {
    const int rl = lwg * kRowsPerWg + wave * kRowsPerWave + k;
    if (rl >= a.R) break;
    const long long r = (long long)layer * a.R + rl;
    const int m = crit_target(a, r);
    const int tc = crit_class(a, m);
    const float* x = a.logits + r * a.ls;
    for (int c = lane; c < a.C; c += DOD_WAVE) {
      const float l = focal_elem(x[c], c == tc, a.alpha, a.gamma);
      ce += l;
      if (elem) elem[(long long)r * a.C + c] = l;
    }
    if (lane == 0 && a.boxes && m >= 0 && m < a.G) {
      const float* p = a.boxes + (long long)r * a.bs;
      const float* t = a.gt + (long long)m * 4;
      l1 += ((fabsf(p[0] - t[0]) + fabsf(p[1] - t[1])) + fabsf(p[2] - t[2])) + fabsf(p[3] - t[3]);
      gi += 1.f - giou_pair(p, t).giou;
    }
  }
  ce = wave_sum(ce);                                      // l1 / gi live on lane 0 only
  __shared__ float red[3][kWaves];
  if (lane == 0) { red[0][wave] = ce; red[1][wave] = l1; red[2][wave] = gi; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int i = threadIdx.x;
    float s = red[i][0];
    for (int w = 1; w < kWaves; ++w) s += red[i][w];
    part[((size_t)layer * 3 + i) * a.wgl + lwg] = s;
  }
}

// one workgroup per layer: losses[i] = (sum of the layer's nwg partials of loss i, in a fixed order) / max(num_boxes, 1)
__global__ __launch_bounds__(256) void crit_finalize_kernel(const float* __restrict__ part, int nwg,
                                                            const float* __restrict__ num_boxes,
                                                            float* __restrict__ losses) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  part += (size_t)blockIdx.x * 3 * nwg;
  losses += (size_t)blockIdx.x * 3;
  __shared__ float red[3][kWaves];
  for (int i = 0; i < 3; ++i) {
    float s = 0.f;
    for (int j = threadIdx.x; j < nwg; j += 256) s += part[(size_t)i * nwg + j];
    s = wave_sum(s);
    if (lane == 0) red[i][wave] = s;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int i = threadIdx.x;
    float s = red[i][0];
    for (int w = 1; w < kWaves; ++w) s += red[i][w];
    const float nb = num_boxes ? fmaxf(num_boxes[0], 1.0f) : 1.0f;
    losses[i] = s / nb;
  }
}

__global__ __launch_bounds__(256) void crit_backward_kernel(CritArgs a, const float* __restrict__ d_losses,
                                                            const float* __restrict__ d_elem,
                                                            float* __restrict__ d_logits, float* __restrict__ d_boxes) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float nb = crit_norm(a);
  const int layer = blockIdx.x / a.wgl, lwg = blockIdx.x - layer * a.wgl;
  if (d_losses) d_losses += layer * 3;
  const float gce = d_elem ? 0.f : d_losses[0] / nb;
  for (int k = 0; k < kRowsPerWave; ++k) {
    const int rl = lwg * kRowsPerWg + wave * kRowsPerWave + k;
    if (rl >= a.R) break;
    const long long r = (long long)layer * a.R + rl;
    const int m = crit_target(a, r);
    const int tc = crit_class(a, m);
    const float* x = a.logits + r * a.ls;
    float* dx = d_logits + r * a.C;
    for (int c = lane; c < a.C; c += DOD_WAVE) {
      const float up = d_elem ? d_elem[(long long)r * a.C + c] : gce;      // elem_loss is un-normalised, so is its gradient
      dx[c] = up * focal_grad(x[c], c == tc, a.alpha, a.gamma);
    }
    if (lane == 0 && a.boxes && d_boxes) {
      float g[4] = {0.f, 0.f, 0.f, 0.f};
      if (m >= 0 && m < a.G) {
        const float* p = a.boxes + (long long)r * a.bs;
        const float* t = a.gt + (long long)m * 4;
        const float gb = d_losses[1] / nb, gg = -(d_losses[2] / nb);
        giou_pair_grad(p, t, gg, g);
        for (int i = 0; i < 4; ++i) g[i] += gb * l1_sign(p[i] - t[i]);
      }
      float* db = d_boxes + (long long)r * 4;
      for (int i = 0; i < 4; ++i) db[i] = g[i];
    }
  }
}

int crit_nwg(int B, int Q) { return (int)(((long long)B * Q + kRowsPerWg - 1) / kRowsPerWg); }

// host-side shape / stride validation shared by forward and backward (who: the entry point, for the message)
int crit_args(const char* who, CritArgs& a, const float* pred_logits, long long logits_row_stride, const float* pred_boxes,
              long long boxes_row_stride, int layers, int B, int Q, int C, const int64_t* labels, const float* gt_boxes, int G,
              const int32_t* match, long long M, const float* num_boxes, float alpha, float gamma) {
  if (!pred_logits || layers <= 0 || B <= 0 || Q <= 0 || C <= 0 || G < 0) return dod_fail(DOD_ERR_INVALID, "%s: null pred_logits, non-positive layers / B / Q / C or negative G", who);
  const long long rows = (long long)layers * B * Q;
  if ((long long)B * Q > 0x7fffffffLL || rows > 0x7fffffffLL || rows * C > 0x7fffffffffffLL) return dod_fail(DOD_ERR_INVALID, "%s: layers=%d B=%d Q=%d C=%d beyond the index range", who, layers, B, Q, C);
  if ((long long)layers * crit_nwg(B, Q) > 0x7fffffffLL) return dod_fail(DOD_ERR_INVALID, "%s: layers=%d B=%d Q=%d beyond the grid range", who, layers, B, Q);
  if (logits_row_stride < C) return dod_fail(DOD_ERR_INVALID, "%s: logits row stride %lld below C = %d", who, logits_row_stride, C);
  if (pred_boxes && boxes_row_stride < 4) return dod_fail(DOD_ERR_INVALID, "%s: boxes row stride %lld below 4", who, boxes_row_stride);
  if (G > 0 && !labels) return dod_fail(DOD_ERR_INVALID, "%s: null labels with G > 0", who);
  if (G > 0 && pred_boxes && !gt_boxes) return dod_fail(DOD_ERR_INVALID, "%s: null gt_boxes with G > 0 and pred_boxes", who);
  if (match ? M != rows : G != rows) return dod_fail(DOD_ERR_INVALID, "%s: %lld match / target rows for %lld predictions", who, match ? M : (long long)G, rows);     // without a table, row r's target is labels[r]
  if (!(gamma >= 0.f) || !(alpha == alpha)) return dod_fail(DOD_ERR_INVALID, "%s: negative or NaN gamma, or NaN alpha", who);
  a.logits = pred_logits; a.ls = logits_row_stride;
  a.boxes = pred_boxes; a.bs = boxes_row_stride;
  a.R = B * Q; a.C = C; a.G = G; a.wgl = crit_nwg(B, Q);
  a.labels = (const long long*)labels; a.gt = gt_boxes; a.match = match; a.num_boxes = num_boxes;
  a.alpha = alpha; a.gamma = gamma;
  return DOD_OK;
}

}  // namespace

extern "C" size_t dod_set_criterion_layers_workspace_bytes(int layers, int B, int Q, int C) {
  if (layers <= 0 || B <= 0 || Q <= 0 || C <= 0) return 0;
  return (size_t)3 * layers * crit_nwg(B, Q) * sizeof(float);
}
extern "C" size_t dod_set_criterion_workspace_bytes(int B, int Q, int C) { return dod_set_criterion_layers_workspace_bytes(1, B, Q, C); }

// the two passes; their entry points are these with who = their own name (the one-layer forms: layers = 1)
static int crit_forward(const char* who, const float* pred_logits, int64_t logits_row_stride, const float* pred_boxes,
                        int64_t boxes_row_stride, int layers, int B, int Q, int C, const int64_t* labels,
                        const float* gt_boxes, int G, const int32_t* match, int M,
                        const float* num_boxes, float alpha, float gamma, float* losses, float* elem_loss,
                        void* workspace, size_t workspace_bytes, void* stream) {
  CritArgs a;
  const int rc = crit_args(who, a, pred_logits, logits_row_stride, pred_boxes, boxes_row_stride, layers, B, Q, C, labels, gt_boxes, G,
                           match, M, num_boxes, alpha, gamma);
  if (rc != DOD_OK) return rc;
  if (!losses || !workspace) return dod_fail(DOD_ERR_INVALID, "%s: null losses or workspace", who);
  if (workspace_bytes < dod_set_criterion_layers_workspace_bytes(layers, B, Q, C)) return dod_fail(DOD_ERR_STATE, "%s: workspace too small", who);
  float* part = (float*)workspace;
  hipLaunchKernelGGL(crit_forward_kernel, dim3((unsigned)(layers * a.wgl)), dim3(256), 0, (hipStream_t)stream, a, part, elem_loss);
  hipLaunchKernelGGL(crit_finalize_kernel, dim3((unsigned)layers), dim3(256), 0, (hipStream_t)stream, (const float*)part, a.wgl,
                     num_boxes, losses);
  return dod_launched(who);
}

static int crit_backward(const char* who, const float* pred_logits, int64_t logits_row_stride, const float* pred_boxes,
                         int64_t boxes_row_stride, int layers, int B, int Q, int C, const int64_t* labels,
                         const float* gt_boxes, int G, const int32_t* match, int M,
                         const float* num_boxes, float alpha, float gamma, const float* d_losses,
                         const float* d_elem, float* d_logits, float* d_boxes, void* stream) {
  CritArgs a;
  const int rc = crit_args(who, a, pred_logits, logits_row_stride, pred_boxes, boxes_row_stride, layers, B, Q, C, labels, gt_boxes, G,
                           match, M, num_boxes, alpha, gamma);
  if (rc != DOD_OK) return rc;
  if (!d_logits || (!d_losses && !d_elem) || (pred_boxes && d_boxes && !d_losses)) return dod_fail(DOD_ERR_INVALID, "%s: null d_logits, or no upstream gradient for an output asked for", who);
  hipLaunchKernelGGL(crit_backward_kernel, dim3((unsigned)(layers * a.wgl)), dim3(256), 0, (hipStream_t)stream, a, d_losses,
                     d_elem, d_logits, d_boxes);
  return dod_launched(who);
}

extern "C" int dod_set_criterion_layers_forward(const float* pred_logits, int64_t logits_row_stride, const float* pred_boxes,
                                                int64_t boxes_row_stride, int layers, int B, int Q, int C, const int64_t* labels,
                                                const float* gt_boxes, int G, const int32_t* match, int M,
                                                const float* num_boxes, float alpha, float gamma, float* losses, float* elem_loss,
                                                void* workspace, size_t workspace_bytes, void* stream) {
  return crit_forward("dod_set_criterion_layers_forward", pred_logits, logits_row_stride, pred_boxes, boxes_row_stride, layers, B, Q, C, labels, gt_boxes, G,
                      match, M, num_boxes, alpha, gamma, losses, elem_loss, workspace, workspace_bytes, stream);
}

extern "C" int dod_set_criterion_layers_backward(const float* pred_logits, int64_t logits_row_stride, const float* pred_boxes,
                                                 int64_t boxes_row_stride, int layers, int B, int Q, int C, const int64_t* labels,
                                                 const float* gt_boxes, int G, const int32_t* match, int M,
                                                 const float* num_boxes, float alpha, float gamma, const float* d_losses,
                                                 const float* d_elem, float* d_logits, float* d_boxes, void* stream) {
  return crit_backward("dod_set_criterion_layers_backward", pred_logits, logits_row_stride, pred_boxes, boxes_row_stride, layers, B, Q, C, labels, gt_boxes, G,
                       match, M, num_boxes, alpha, gamma, d_losses, d_elem, d_logits, d_boxes, stream);
}

extern "C" int dod_set_criterion_forward(const float* pred_logits, int64_t logits_row_stride, const float* pred_boxes,
                                         int64_t boxes_row_stride, int B, int Q, int C, const int64_t* labels,
                                         const float* gt_boxes, int G, const int32_t* match, int M, const float* num_boxes,
                                         float alpha, float gamma, float* losses, float* elem_loss, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  return crit_forward("dod_set_criterion_forward", pred_logits, logits_row_stride, pred_boxes, boxes_row_stride, 1, B, Q, C, labels, gt_boxes, G,
                      match, M, num_boxes, alpha, gamma, losses, elem_loss, workspace, workspace_bytes, stream);
}

extern "C" int dod_set_criterion_backward(const float* pred_logits, int64_t logits_row_stride, const float* pred_boxes,
                                          int64_t boxes_row_stride, int B, int Q, int C, const int64_t* labels,
                                          const float* gt_boxes, int G, const int32_t* match, int M,
                                          const float* num_boxes, float alpha, float gamma, const float* d_losses,
                                          const float* d_elem, float* d_logits, float* d_boxes, void* stream) {
  return crit_backward("dod_set_criterion_backward", pred_logits, logits_row_stride, pred_boxes, boxes_row_stride, 1, B, Q, C, labels, gt_boxes, G,
                       match, M, num_boxes, alpha, gamma, d_losses, d_elem, d_logits, d_boxes, stream);
}
