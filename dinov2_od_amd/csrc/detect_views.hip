// Merge of sliced / flip-augmented inference on device: the packed detections [V, Q, C+4] of all views (the whole image, overlapping
// tiles, mirrored copies) of B images become per image the K best (view, query, class) triples as xyxy boxes in SOURCE-image pixels,
// optionally after greedy NMS across the views (include/dinodet.h dod_detect_views states the contract; tests/detect_views_cases.py
// restates it in numpy).  Fixed-shape outputs [B, K], one launch, no host synchronisation, no global atomics.
//
// One workgroup of 1024 threads per image, the design of det_kernel (detect.hip) over the image's nv * Q rows:
//   0. with an edge margin, one pass over the rows (view, query): the box in source pixels and the edge predicate, one byte per row
//      into the workspace -- four box loads per row, not per class.
//   1 - 3. key pass (a filtered row reads as NaN: no candidate), radix select with the 20-bit index field over
//      i = ((v - v0) * Q + q) * C + c, gather and bitonic sort in LDS: detect_select.h, the code dod_detect runs.
//   4. thread t turns word t into score / label / view / query / box.
//   5. NMS with K up to 1024 (detect_select.h, the code dod_detect runs at 512): the suppression relation is stored upper-triangular,
//      so 1024 rows take 68 KiB instead of 128 KiB, and with boxes, areas, labels, select words and histograms the kernel declares about
//      109 KiB of the CU's 160 KiB of LDS.  K <= 512 runs an instance with an 18 KiB triangle.
// The box, edge and overlap arithmetic must round once per operation: this file is compiled with -ffp-contract=off (_build.EXTRA).
#include "detect_select.h"
#include "../../include/dinodet.h"

#define DV_NMS_MAX_K 1024

struct DvArgs {
  const float* det; const int* voffs; const int* rects; const unsigned char* flips; const float* sizes;
  unsigned* keys; unsigned char* cut;
  float* scores; int* labels; int* views; int* queries; float* boxes; int* counts;
  int V, Q, C, first_class, K;
  float threshold, iou, margin;
  int metric, agnostic, clamp;
};

struct DvRect { int l, t, w, h; };
struct DvBox { float x1, y1, x2, y2; };

__device__ __forceinline__ DvRect dv_rect(const DvArgs& a, int v) {
  const int* r = a.rects + 4 * (size_t)v;
  return DvRect{r[0], r[1], r[2], r[3]};
}
// cxcywh of one view -> xyxy in source pixels, before the edge filter and the clamp: the header's operations in the header's order
__device__ __forceinline__ DvBox dv_box(const float* p, const DvRect& r, bool flip) {
  const float cx = p[0], cy = p[1], w = p[2], h = p[3];
  float x1 = cx - 0.5f * w, y1 = cy - 0.5f * h, x2 = cx + 0.5f * w, y2 = cy + 0.5f * h;
  if (flip) { const float t = 1.0f - x2; x2 = 1.0f - x1; x1 = t; }
  const float vw = (float)r.w, vh = (float)r.h, vl = (float)r.l, vt = (float)r.t;
  x1 = x1 * vw; y1 = y1 * vh; x2 = x2 * vw; y2 = y2 * vh;
  x1 = x1 + vl; y1 = y1 + vt; x2 = x2 + vl; y2 = y2 + vt;
  return DvBox{x1, y1, x2, y2};
}
// a box cut by a border of its view that is not a border of the source image (every comparison is false on NaN)
__device__ __forceinline__ bool dv_cut(const DvBox& b, const DvRect& r, float m, float iw, float ih) {
  const float right = (float)(r.l + r.w), bottom = (float)(r.t + r.h);
  return (r.l > 0 && b.x1 < (float)r.l + m) || (right < iw && b.x2 > right - m) ||
         (r.t > 0 && b.y1 < (float)r.t + m) || (bottom < ih && b.y2 > bottom - m);
}
// NMSK: 0 = no NMS, else the largest K of this instance (512 or 1024)
template <int NMSK>
__global__ __launch_bounds__(DET_THREADS) void dv_kernel(const DvArgs a) {
  __shared__ DetSelectLds L;
  const int tid = threadIdx.x;
  const int b = blockIdx.x, C = a.C, Q = a.Q, K = a.K;
  int v0 = a.voffs[b], nv = a.voffs[b + 1] - v0;
  if (v0 < 0 || nv < 0 || v0 > a.V - nv || (long long)nv * Q * C > DET_MAX_PAIRS) { v0 = 0; nv = 0; }   // no view of this image is read
  const int R = nv * Q, N = R * C;
  const float* dp = a.det + (size_t)v0 * Q * (C + 4);
  unsigned* kp = a.keys + (size_t)v0 * Q * C;
  unsigned char* cut = a.cut + (size_t)v0 * Q;
  const float ih = a.sizes[2 * b], iw = a.sizes[2 * b + 1];
  const bool edge = a.margin > 0.0f;

  // ---- 0: the edge predicate of every row
  if (edge) {
    for (int r = tid; r < R; r += DET_THREADS) {
      const int vl = r / Q;
      const DvRect rc = dv_rect(a, v0 + vl);
      const DvBox bx = dv_box(dp + (size_t)r * (C + 4) + C, rc, a.flips[v0 + vl] != 0);
      cut[r] = dv_cut(bx, rc, a.margin, iw, ih) ? 1 : 0;
    }
    __syncthreads();
  }

  // ---- 1 - 3: keys, radix select, gather and sort (detect_select.h)
  const int n = det_select_sort(L, N, K, tid, kp,
    [&](int i) {
      const int r = i / C, c = i - r * C;
      const float x = dp[(size_t)r * (C + 4) + c];
      return (edge && cut[r]) ? __uint_as_float(0x7FC00000u) : x;
    },
    [&](int i, float x) {
      const int c = i % C;
      const bool cand = c >= a.first_class && x == x && (a.threshold < 0.0f || det_sigmoid(x) > a.threshold);
      return cand ? det_key(x) : 0u;
    });
  const unsigned long long* const sel = L.sel;

  // ---- 4: thread t decodes word t
  float sc = 0.0f, x1 = 0.0f, y1 = 0.0f, x2 = 0.0f, y2 = 0.0f;
  int lab = -1, qi = -1, vi = -1;
  if (tid < n) {
    const int idx = (int)(0xFFFFFu - (unsigned)((sel[tid] >> 4) & 0xFFFFFu));
    const int r = idx / C;
    lab = idx - r * C; vi = r / Q; qi = r - vi * Q;
    const float* row = dp + (size_t)r * (C + 4);
    sc = det_sigmoid(row[lab]);
    const DvBox bx = dv_box(row + C, dv_rect(a, v0 + vi), a.flips[v0 + vi] != 0);
    x1 = bx.x1; y1 = bx.y1; x2 = bx.x2; y2 = bx.y2;
    if (a.clamp) { x1 = det_clamp(x1, iw); y1 = det_clamp(y1, ih); x2 = det_clamp(x2, iw); y2 = det_clamp(y2, ih); }
  }
  const size_t o = (size_t)b * K;
  if constexpr (NMSK == 0) {
    if (tid < K) {
      a.scores[o + tid] = sc; a.labels[o + tid] = lab; a.views[o + tid] = vi; a.queries[o + tid] = qi;
      reinterpret_cast<float4*>(a.boxes)[o + tid] = make_float4(x1, y1, x2, y2);
    }
    if (tid == 0) a.counts[b] = n;
  } else {
    // ---- 5: greedy NMS over the n sorted candidates (n <= K <= NMSK: the host picks the instance), detect_select.h
    __shared__ DetNmsLds<NMSK> S;
    det_nms(S, n, tid, make_float4(x1, y1, x2, y2), lab, a.iou, a.agnostic != 0, a.metric != 0);
    int rank;
    const int total = det_nms_rank(S, n, tid, rank);
    if (tid >= total && tid < K) {                             // padding rows
      a.scores[o + tid] = 0.0f; a.labels[o + tid] = -1; a.views[o + tid] = -1; a.queries[o + tid] = -1;
      reinterpret_cast<float4*>(a.boxes)[o + tid] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    if (tid < n && !((S.rem[tid >> 6] >> (tid & 63)) & 1ull)) { // a survivor moves to row rank <= tid, rank < total
      a.scores[o + rank] = sc; a.labels[o + rank] = lab; a.views[o + rank] = vi; a.queries[o + rank] = qi;
      reinterpret_cast<float4*>(a.boxes)[o + rank] = make_float4(x1, y1, x2, y2);
    }
    if (tid == 0) a.counts[b] = total;
  }
}

static inline size_t dv_align(size_t x) { return (x + 255) & ~(size_t)255; }

static bool dv_shape_ok(int V, int Q, int C, int K) {
  return V >= 0 && Q > 0 && C >= 1 && K >= 1 && K <= DET_MAX_K && (long long)Q * C <= DET_MAX_PAIRS;
}
static size_t dv_keys_bytes(int V, int Q, int C) { return dv_align((size_t)V * Q * C * sizeof(unsigned) + 1); }

extern "C" size_t dod_detect_views_workspace_bytes(int V, int Q, int C, int K) {
  if (!dv_shape_ok(V, Q, C, K)) return 0;
  return dv_keys_bytes(V, Q, C) + dv_align((size_t)V * Q + 1);   // keys, then one edge byte per row; never 0 inside the limits
}

extern "C" int dod_detect_views(const float* det, int B, int V, int Q, int C, const int32_t* view_offsets, const int32_t* view_rects,
                                const uint8_t* view_flips, const float* sizes, int first_class, float threshold, int K,
                                float iou_threshold, int nms_metric, int class_agnostic, int clamp, float edge_margin, float* scores,
                                int32_t* labels, int32_t* views, int32_t* queries, float* boxes, int32_t* counts, void* workspace,
                                size_t workspace_bytes, void* stream) {
  if (!view_offsets || !sizes || !scores || !labels || !views || !queries || !boxes || !counts) return DOD_ERR_INVALID;
  if (B < 1 || !dv_shape_ok(V, Q, C, K) || first_class < 0 || first_class >= C) return DOD_ERR_INVALID;
  if (V > 0 && (!det || !view_rects || !view_flips)) return DOD_ERR_INVALID;
  if (nms_metric != 0 && nms_metric != 1) return DOD_ERR_INVALID;
  if (((uintptr_t)boxes & 15) != 0) return DOD_ERR_INVALID;      // rows are stored as float4
  if (!workspace || workspace_bytes < dod_detect_views_workspace_bytes(V, Q, C, K)) return DOD_ERR_INVALID;
  DvArgs a;
  a.det = det; a.voffs = view_offsets; a.rects = view_rects; a.flips = view_flips; a.sizes = sizes;
  a.keys = (unsigned*)workspace; a.cut = (unsigned char*)workspace + dv_keys_bytes(V, Q, C);
  a.scores = scores; a.labels = labels; a.views = views; a.queries = queries; a.boxes = boxes; a.counts = counts;
  a.V = V; a.Q = Q; a.C = C; a.first_class = first_class; a.K = K;
  a.threshold = threshold; a.iou = iou_threshold; a.margin = edge_margin;
  a.metric = nms_metric; a.agnostic = class_agnostic; a.clamp = clamp;
  hipStream_t s = (hipStream_t)stream;
  if (!(iou_threshold >= 0.0f)) hipLaunchKernelGGL(dv_kernel<0>, dim3(B), dim3(DET_THREADS), 0, s, a);
  else if (K <= 512) hipLaunchKernelGGL(dv_kernel<512>, dim3(B), dim3(DET_THREADS), 0, s, a);
  else hipLaunchKernelGGL(dv_kernel<DV_NMS_MAX_K>, dim3(B), dim3(DET_THREADS), 0, s, a);
  return hipGetLastError() == hipSuccess ? DOD_OK : DOD_ERR_HIP;
}
