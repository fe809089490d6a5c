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
//   5'. dod_fuse_views (fv_kernel, below): weighted boxes fusion in the place of NMS, on the same stages 0 - 4 (dv_candidates).
// The box, edge, overlap and fusion arithmetic must round once per operation: detect_select.h turns fp contraction off for the whole file.
#include "detect_select.h"
#include "../../include/dinodet.h"

#define DV_NMS_MAX_K 1024

struct DvArgs {
  const float* det; const int* voffs; const int* rects; const unsigned char* flips; const float* sizes;
  unsigned* keys; unsigned char* cut;
  DetOut out;                    // members null in dod_detect_views
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
// what stages 0 - 4 leave in thread t: candidate t of the image's n sorted candidates (the padding row for t >= n)
struct DvCand { DetRow row; int n, v0, nv; float ih, iw; };

// Stages 0 - 4 for image b by all DET_THREADS threads, shared by dv_kernel and fv_kernel; v0 / nv / ih / iw: the image's first view, view
// count (0 when its offsets are out of range) and size.  Ends behind det_select_sort's last barrier: L.sel holds the sorted words.
__device__ __forceinline__ DvCand dv_candidates(DetSelectLds& L, const DvArgs& a, int b, int tid) {
  const int C = a.C, Q = a.Q, K = a.K;
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
    [&](int i, float x) { return det_cand_key(i % C, x, a.first_class, a.threshold); });
  const unsigned long long* const sel = L.sel;

  // ---- 4: thread t decodes word t
  DvCand d{det_pad_row(), n, v0, nv, ih, iw};
  if (tid < n) {
    DetRow& o = d.row;
    const int idx = (int)(0xFFFFFu - (unsigned)((sel[tid] >> 4) & 0xFFFFFu));
    const int r = idx / C;
    o.label = idx - r * C; o.view = r / Q; o.query = r - o.view * Q;
    const float* p = dp + (size_t)r * (C + 4);
    o.score = det_sigmoid(p[o.label]);
    const DvBox bx = dv_box(p + C, dv_rect(a, v0 + o.view), a.flips[v0 + o.view] != 0);
    o.box = make_float4(bx.x1, bx.y1, bx.x2, bx.y2);
    if (a.clamp) o.box = make_float4(det_clamp(bx.x1, iw), det_clamp(bx.y1, ih), det_clamp(bx.x2, iw), det_clamp(bx.y2, ih));
  }
  return d;
}

// NMSK: 0 = no NMS, else the largest K of this instance (512 or 1024)
template <int NMSK>
__global__ __launch_bounds__(DET_THREADS) void dv_kernel(const DvArgs a) {
  __shared__ DetSelectLds L;
  const int tid = threadIdx.x, b = blockIdx.x;
  const DvCand d = dv_candidates(L, a, b, tid);
  // ---- 5 and the rows (detect_select.h)
  DetOut out = a.out;
  out.members = nullptr;                                         // known here, not only to the host: the store folds away
  det_finish<NMSK>(out, b, a.K, d.n, tid, d.row, a.iou, a.agnostic != 0, a.metric != 0);
}

// ---- weighted boxes fusion across the views (include/dinodet.h dod_fuse_views; tests/fuse_views_cases.py restates it) --------------
// Stages 0 - 4 as above, then in place of NMS one pass over the n sorted candidates that builds clusters: a candidate joins the
// cluster whose CURRENT fused box it overlaps best (IoU above the threshold, equal quotients to the lowest cluster number) or founds
// one.  The fused box a candidate meets depends on every earlier candidate, so the chain over the candidates is serial; what runs
// side by side is the comparison with the clusters.  Thread c holds cluster c in registers (box, area, label, five sums, members,
// founder).  Per candidate: the waves that hold clusters compute their lanes' match words (quotient bits, ~cluster), reduce them
// with one ballot and a readlane per matching lane, and post one word per wave; one barrier; every thread takes the largest of the
// posted words, so all agree on the winner, and the thread that owns it updates its registers.  The posted words are double
// buffered: a wave can overwrite a buffer only two barriers later, when every wave has read it.  One wave alone running the same
// comparison round by round over clusters in LDS took 1.2 times the whole call's time at K = 300 and 1.9 times at K = 1024: it is
// bound by the issue of its own VALU instructions, about 45 per round of 64 clusters.  About 76 KiB of LDS: 16 KiB select, 28 KiB candidates, 32 KiB for the clusters'
// results, which the sort of the output rows reads across threads.
struct FvLds {
  float4 cbox[DET_MAX_K];                 // the candidates: box, label, score, row (v * Q + q)
  int clab[DET_MAX_K];
  float csc[DET_MAX_K];
  int crow[DET_MAX_K];
  float4 kbox[DET_MAX_K];                 // the clusters after the chain: fused box, fused score, label, members, founder
  float kscore[DET_MAX_K];
  int klab[DET_MAX_K];
  int kcnt[DET_MAX_K];
  int kfirst[DET_MAX_K];
  unsigned long long post[2][DET_WAVES];  // the waves' best match words of the candidate, by candidate parity
};

__device__ __forceinline__ float fv_area(const float4& b) { return det_max(0.0f, b.z - b.x) * det_max(0.0f, b.w - b.y); }

__global__ __launch_bounds__(DET_THREADS) void fv_kernel(const DvArgs a, int conf) {
  __shared__ DetSelectLds L;
  __shared__ FvLds F;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, K = a.K;
  const DvCand d = dv_candidates(L, a, b, tid);
  const int n = d.n;                                           // uniform: det_select_sort reads it from LDS behind a barrier
  if (tid < n) {
    F.cbox[tid] = d.row.box;
    F.clab[tid] = d.row.label; F.csc[tid] = d.row.score; F.crow[tid] = d.row.view * a.Q + d.row.query;
  }
  __syncthreads();

  // ---- 5: the chain.  n, nc and the winner are the same in every thread, so every barrier is met by the whole workgroup
  const bool can = a.iou >= 0.0f, agnostic = a.agnostic != 0;
  float4 kb = make_float4(0.0f, 0.0f, 0.0f, 0.0f);             // cluster tid
  float ka = 0.0f, sx1 = 0.0f, sy1 = 0.0f, sx2 = 0.0f, sy2 = 0.0f, ss = 0.0f;
  int kl = -1, kT = 0, kf = 0;
  int nc = 0;
  float4 cb = kb;
  int cl = -1;
  float s = 0.0f;
  if (n > 0) { cb = F.cbox[0]; cl = F.clab[0]; s = F.csc[0]; }
  for (int i = 0; i < n; ++i) {
    const float ab = fv_area(cb);
    const int waves = (nc + 63) >> 6;                          // the waves that hold a cluster
    if (can && wave < waves) {
      unsigned long long best = 0;                             // (quotient bits, ~cluster): larger quotient first, then the lower cluster
      if (tid < nc) {
        const float iw = det_max(0.0f, det_min(kb.z, cb.z) - det_max(kb.x, cb.x));
        const float ih = det_max(0.0f, det_min(kb.w, cb.w) - det_max(kb.y, cb.y));
        const float inter = iw * ih;
        const float uni = (ka + ab) - inter;
        if ((agnostic || kl == cl) && inter > a.iou * uni)     // then 0 < inter <= uni: the quotient is positive and its bits are ordered
          best = ((unsigned long long)__float_as_uint(inter / uni) << 32) | (0xFFFFFFFFu - (unsigned)tid);
      }
      unsigned long long m = __ballot(best != 0), top = 0;
      while (m) {                                              // wave-uniform: one round per lane that holds a match
        const int l = __ffsll((long long)m) - 1;
        const unsigned lo = __builtin_amdgcn_readlane((unsigned)best, l), hi = __builtin_amdgcn_readlane((unsigned)(best >> 32), l);
        const unsigned long long k = ((unsigned long long)hi << 32) | lo;
        if (k > top) top = k;
        m &= m - 1;
      }
      if (lane == 0) F.post[i & 1][wave] = top;
    }
    float4 nb = cb;                                            // the next candidate, on its way while this one is decided
    int nl = cl;
    float ns = s;
    if (i + 1 < n) { nb = F.cbox[i + 1]; nl = F.clab[i + 1]; ns = F.csc[i + 1]; }
    __syncthreads();
    unsigned long long win = 0;
    if (can && waves > 0) {                                    // lane w reads wave w's word: the same reduction again, in every wave
      const unsigned long long k = lane < waves ? F.post[i & 1][lane] : 0ull;
      unsigned long long m = __ballot(k != 0);
      while (m) {
        const int l = __ffsll((long long)m) - 1;
        const unsigned lo = __builtin_amdgcn_readlane((unsigned)k, l), hi = __builtin_amdgcn_readlane((unsigned)(k >> 32), l);
        const unsigned long long kk = ((unsigned long long)hi << 32) | lo;
        if (kk > win) win = kk;
        m &= m - 1;
      }
    }
    const int c = win ? (int)(0xFFFFFFFFu - (unsigned)win) : nc;
    if (tid == c) {
      if (win) {                                               // each product rounds, then each sum (fp contract off)
        sx1 = sx1 + s * cb.x; sy1 = sy1 + s * cb.y; sx2 = sx2 + s * cb.z; sy2 = sy2 + s * cb.w; ss = ss + s;
        kb = make_float4(sx1 / ss, sy1 / ss, sx2 / ss, sy2 / ss);
        if (a.clamp) { kb.x = det_clamp(kb.x, d.iw); kb.y = det_clamp(kb.y, d.ih); kb.z = det_clamp(kb.z, d.iw); kb.w = det_clamp(kb.w, d.ih); }
        ka = fv_area(kb); kT += 1;
      } else {
        sx1 = s * cb.x; sy1 = s * cb.y; sx2 = s * cb.z; sy2 = s * cb.w; ss = s;
        kb = cb; ka = ab; kl = cl; kT = 1; kf = i;
      }
    }
    if (!win) ++nc;
    cb = nb; cl = nl; s = ns;
  }                                                            // nc <= n <= K

  // ---- 6: thread c scores cluster c: how many views could have seen its fused box
  if (tid < nc) {
    float score = F.csc[kf];
    if (conf != 0) {
      int N = 0;
      for (int v = 0; v < d.nv; ++v) {
        const DvRect r = dv_rect(a, d.v0 + v);
        const bool inside = kb.x >= (float)r.l && kb.y >= (float)r.t && kb.z <= (float)(r.l + r.w) && kb.w <= (float)(r.t + r.h);
        if (inside && !(a.margin > 0.0f && dv_cut(DvBox{kb.x, kb.y, kb.z, kb.w}, r, a.margin, d.iw, d.ih))) ++N;
      }
      if (N < 1) N = 1;
      const float mean = ss / (float)kT;
      score = kT >= N ? mean : mean * (float)kT / (float)N;
    }
    F.kbox[tid] = kb; F.kscore[tid] = score; F.klab[tid] = kl; F.kcnt[tid] = kT; F.kfirst[tid] = kf;
    if (conf != 0) L.sel[tid] = det_word(det_key(score), tid);
  }
  // ---- 7: order.  "max": founding order, which is descending in the founder's logit.  "avg": by fused score, ties by cluster number
  int c = tid;
  if (conf != 0) {
    det_sort_desc(L.sel, nc, tid);
    if (tid < nc) c = (int)(0xFFFFFu - (unsigned)((L.sel[tid] >> 4) & 0xFFFFFu));
  } else {
    __syncthreads();
  }
  const size_t o = (size_t)b * K;
  if (tid < nc) {
    const int row = F.crow[F.kfirst[c]], vi = row / a.Q;
    det_store(a.out, DetRow{F.kscore[c], F.klab[c], vi, row - vi * a.Q, F.kbox[c], F.kcnt[c]}, o + tid);
  } else if (tid < K) {
    det_store(a.out, det_pad_row(), o + tid);
  }
  if (tid == 0) a.out.counts[b] = nc;
}

static bool dv_shape_ok(int V, int Q, int C, int K) {
  return V >= 0 && Q > 0 && C >= 1 && K >= 1 && K <= DET_MAX_K && (long long)Q * C <= DET_MAX_PAIRS;
}
static size_t dv_keys_bytes(int V, int Q, int C) { return dod::align_up((size_t)V * Q * C * sizeof(unsigned) + 1); }

extern "C" size_t dod_detect_views_workspace_bytes(int V, int Q, int C, int K) {
  if (!dv_shape_ok(V, Q, C, K)) return 0;
  return dv_keys_bytes(V, Q, C) + dod::align_up((size_t)V * Q + 1);   // keys, then one edge byte per row; never 0 inside the limits
}
extern "C" size_t dod_fuse_views_workspace_bytes(int V, int Q, int C, int K) { return dod_detect_views_workspace_bytes(V, Q, C, K); }

// What dod_detect_views and dod_fuse_views check alike, and the DvArgs of both; a dod_status, its message under the entry point's
// name `who`.  `out` is complete: an entry point checks its own arguments (nms_metric, conf, members) itself.
static int dv_prepare(const char* who, DvArgs& a, const float* det, int B, int V, int Q, int C, const int32_t* view_offsets, const int32_t* view_rects,
                       const uint8_t* view_flips, const float* sizes, int first_class, float threshold, int K, float iou_threshold,
                       int nms_metric, int class_agnostic, int clamp, float edge_margin, const DetOut& out, void* workspace,
                       size_t workspace_bytes) {
  if (!view_offsets || !sizes || !out.scores || !out.labels || !out.views || !out.queries || !out.boxes || !out.counts)
    return dod_fail(DOD_ERR_INVALID, "%s: null view_offsets, sizes or output", who);
  if (B < 1 || !dv_shape_ok(V, Q, C, K) || first_class < 0 || first_class >= C)
    return dod_fail(DOD_ERR_INVALID, "%s: B=%d V=%d Q=%d C=%d K=%d outside the limits, or first_class = %d outside [0, C)", who, B, V, Q, C, K, first_class);
  if (V > 0 && (!det || !view_rects || !view_flips)) return dod_fail(DOD_ERR_INVALID, "%s: null det, view_rects or view_flips with V > 0", who);
  if (((uintptr_t)out.boxes & 15) != 0) return dod_fail(DOD_ERR_INVALID, "%s: boxes not 16-byte aligned", who);            // rows are stored as float4
  if (!workspace || workspace_bytes < dod_detect_views_workspace_bytes(V, Q, C, K)) return dod_fail(DOD_ERR_INVALID, "%s: null or short workspace", who);
  a.det = det; a.voffs = view_offsets; a.rects = view_rects; a.flips = view_flips; a.sizes = sizes;
  a.keys = (unsigned*)workspace; a.cut = (unsigned char*)workspace + dv_keys_bytes(V, Q, C);
  a.out = out;
  a.V = V; a.Q = Q; a.C = C; a.first_class = first_class; a.K = K;
  a.threshold = threshold; a.iou = iou_threshold; a.margin = edge_margin;
  a.metric = nms_metric; a.agnostic = class_agnostic; a.clamp = clamp;
  return DOD_OK;
}

extern "C" int dod_detect_views(const float* det, int B, int V, int Q, int C, const int32_t* view_offsets, const int32_t* view_rects,
                                const uint8_t* view_flips, const float* sizes, int first_class, float threshold, int K,
                                float iou_threshold, int nms_metric, int class_agnostic, int clamp, float edge_margin, float* scores,
                                int32_t* labels, int32_t* views, int32_t* queries, float* boxes, int32_t* counts, void* workspace,
                                size_t workspace_bytes, void* stream) {
  DvArgs a;
  if (nms_metric != 0 && nms_metric != 1) return dod_fail(DOD_ERR_INVALID, "dod_detect_views: nms_metric = %d is neither 0 nor 1", nms_metric);
  if (const int rc = dv_prepare("dod_detect_views", a, det, B, V, Q, C, view_offsets, view_rects, view_flips, sizes, first_class, threshold, K, iou_threshold, nms_metric,
                  class_agnostic, clamp, edge_margin, DetOut{scores, labels, views, queries, boxes, nullptr, counts}, workspace, workspace_bytes))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  if (!(iou_threshold >= 0.0f)) hipLaunchKernelGGL(dv_kernel<0>, dim3(B), dim3(DET_THREADS), 0, s, a);
  else if (K <= 512) hipLaunchKernelGGL(dv_kernel<512>, dim3(B), dim3(DET_THREADS), 0, s, a);
  else hipLaunchKernelGGL(dv_kernel<DV_NMS_MAX_K>, dim3(B), dim3(DET_THREADS), 0, s, a);
  return dod_launched("dod_detect_views");
}

extern "C" int dod_fuse_views(const float* det, int B, int V, int Q, int C, const int32_t* view_offsets, const int32_t* view_rects,
                              const uint8_t* view_flips, const float* sizes, int first_class, float threshold, int K,
                              float iou_threshold, int class_agnostic, int clamp, float edge_margin, int conf, float* scores,
                              int32_t* labels, int32_t* views, int32_t* queries, float* boxes, int32_t* members, int32_t* counts,
                              void* workspace, size_t workspace_bytes, void* stream) {
  DvArgs a;
  if (!members || (conf != 0 && conf != 1)) return dod_fail(DOD_ERR_INVALID, "dod_fuse_views: null members, or conf = %d is neither 0 nor 1", conf);
  if (const int rc = dv_prepare("dod_fuse_views", a, det, B, V, Q, C, view_offsets, view_rects, view_flips, sizes, first_class, threshold, K, iou_threshold, 0,
                  class_agnostic, clamp, edge_margin, DetOut{scores, labels, views, queries, boxes, members, counts}, workspace, workspace_bytes))
    return rc;
  hipLaunchKernelGGL(fv_kernel, dim3(B), dim3(DET_THREADS), 0, (hipStream_t)stream, a, conf);
  return dod_launched("dod_fuse_views");
}

