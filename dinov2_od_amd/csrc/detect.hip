// Detection output on device: the K best (query, class) pairs of every image as pixel xyxy boxes with score and label, optionally
// after greedy NMS -- what a caller who is not running COCO eval wants from the packed detections [B, Q, C+4] (include/dinodet.h
// dod_detect states the contract; tests/detect_cases.py restates it in numpy).  Fixed-shape outputs [B, K], one launch, no host
// synchronisation, no global atomics: results are a function of the input bits alone.
//
// One workgroup of 1024 threads per image:
//   1. key[i] of every flat index i = q*C + c: the order-preserving integer image of the logit (sign bit flipped for x >= 0, all bits
//      for x < 0), or 0 for a pair that is no candidate (c < first_class, NaN, score not above the threshold).  0 is the image of a
//      NaN only, so it is free.  Keys go to the workspace: the later passes read 4 contiguous bytes per pair.
//   2. radix select, 8 bits per pass, of the K-th largest 56-bit word  key << 24 | (0xFFFFF - i) << 4.  The index below the key makes
//      every word distinct and orders ties by ascending i, so "the first K in (logit descending, index ascending) order" is exactly
//      "word >= threshold word".  The passes stop as soon as the chosen bin holds no more words than are still wanted: four passes when
//      the K-th logit is distinct, up to seven when ties straddle it.  Histograms live in LDS, 8 copies by lane to spread the
//      same-bin atomics of clustered exponents.
//   3. the <= K selected words are gathered into LDS (slot order is arbitrary) and sorted descending by a bitonic network: the
//      order is a function of the words alone.
//   4. thread t turns word t into score / label / query / box; without NMS it stores row t.
//   5. NMS: a bit-matrix of the K x K suppression relation in LDS, upper-triangular (one ballot per 64 pairs), a serial sweep by one
//      wave that carries the removed set as one 64-bit word per lane, and an ordered compaction by population count.
// The box and IoU arithmetic must round once per operation: detect_select.h turns fp contraction off for the whole file.
#include "detect_select.h"       // stages 1 - 3 and 5, the output tail and the key / word helpers, shared with detect_views.hip
#include "../../include/dinodet.h"

#define DET_NMS_MAX_K 512        // dod_detect's documented limit with NMS

struct DetArgs {
  const float* det; const float* sizes; unsigned* keys;
  DetOut out;                    // views and members null
  int Q, C, first_class, K;
  float threshold, iou;
  int agnostic, clamp;
};

__device__ __forceinline__ float det_logit(const DetArgs& a, const float* dp, int i) {
  const int q = i / a.C, c = i - q * a.C;
  return dp[(size_t)q * (a.C + 4) + c];
}

template <bool NMS>
__global__ __launch_bounds__(DET_THREADS) void det_kernel(const DetArgs a) {
  __shared__ DetSelectLds L;
  const int tid = threadIdx.x;
  const int b = blockIdx.x, C = a.C, K = a.K;
  const int N = a.Q * C;
  const float* dp = a.det + (size_t)b * a.Q * (C + 4);
  unsigned* kp = a.keys + (size_t)b * N;

  // ---- 1 - 3: keys, radix select, gather and sort (detect_select.h)
  const int n = det_select_sort(L, N, K, tid, kp, [&](int i) { return det_logit(a, dp, i); },
                                [&](int i, float x) { return det_cand_key(i % C, x, a.first_class, a.threshold); });
  const unsigned long long* const sel = L.sel;

  // ---- 4: thread t decodes word t
  DetRow row = det_pad_row();
  if (tid < n) {
    const int idx = (int)(0xFFFFFu - (unsigned)((sel[tid] >> 4) & 0xFFFFFu));
    row.query = idx / C; row.label = idx - row.query * C;
    const float* p = dp + (size_t)row.query * (C + 4);
    row.score = det_sigmoid(p[row.label]);
    const float cx = p[C], cy = p[C + 1], w = p[C + 2], h = p[C + 3];
    const float ih = a.sizes ? a.sizes[2 * b] : 1.0f, iw = a.sizes ? a.sizes[2 * b + 1] : 1.0f;
    float x1 = cx - 0.5f * w, y1 = cy - 0.5f * h, x2 = cx + 0.5f * w, y2 = cy + 0.5f * h;
    x1 *= iw; y1 *= ih; x2 *= iw; y2 *= ih;
    if (a.clamp) { x1 = det_clamp(x1, iw); y1 = det_clamp(y1, ih); x2 = det_clamp(x2, iw); y2 = det_clamp(y2, ih); }
    row.box = make_float4(x1, y1, x2, y2);
  }
  // ---- 5 and the rows: with NMS n <= DET_NMS_MAX_K (the host refuses a larger K), detect_select.h
  DetOut out = a.out;
  out.views = out.members = nullptr;                             // known here, not only to the host: their stores fold away
  det_finish<NMS ? DET_NMS_MAX_K : 0>(out, b, K, n, tid, row, a.iou, a.agnostic != 0, false);
}

static bool det_shape_ok(int B, int Q, int C, int K) {
  return B > 0 && Q > 0 && C >= 1 && K >= 1 && K <= DET_MAX_K && (long long)Q * C <= DET_MAX_PAIRS;
}

extern "C" size_t dod_detect_workspace_bytes(int B, int Q, int C, int K) {
  if (!det_shape_ok(B, Q, C, K)) return 0;
  return dod::align_up((size_t)B * Q * C * sizeof(unsigned));
}

extern "C" int dod_detect(const float* det, int B, int Q, int C, int first_class, const float* sizes, float threshold, int K,
                          float iou_threshold, int class_agnostic, int clamp, float* scores, int32_t* labels, int32_t* queries,
                          float* boxes, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
  if (!det || !scores || !labels || !queries || !boxes || !counts) return dod_fail(DOD_ERR_INVALID, "dod_detect: null argument");
  if (!det_shape_ok(B, Q, C, K) || first_class < 0 || first_class >= C) return dod_fail(DOD_ERR_INVALID, "dod_detect: B=%d Q=%d C=%d K=%d outside the limits, or first_class = %d outside [0, C)", B, Q, C, K, first_class);
  const bool nms = iou_threshold >= 0.0f;
  if (nms && K > DET_NMS_MAX_K) return dod_fail(DOD_ERR_INVALID, "dod_detect: K = %d above the %d rows the NMS takes", K, DET_NMS_MAX_K);
  if (((uintptr_t)boxes & 15) != 0) return dod_fail(DOD_ERR_INVALID, "dod_detect: boxes not 16-byte aligned");      // rows are stored as float4
  if (!workspace || workspace_bytes < dod_detect_workspace_bytes(B, Q, C, K)) return dod_fail(DOD_ERR_INVALID, "dod_detect: null or short workspace");
  DetArgs a;
  a.det = det; a.sizes = sizes; a.keys = (unsigned*)workspace;
  a.out = DetOut{scores, labels, nullptr, queries, boxes, nullptr, counts};
  a.Q = Q; a.C = C; a.first_class = first_class; a.K = K;
  a.threshold = threshold; a.iou = iou_threshold;
  a.agnostic = class_agnostic; a.clamp = clamp;
  hipStream_t s = (hipStream_t)stream;
  if (nms) hipLaunchKernelGGL(det_kernel<true>, dim3(B), dim3(DET_THREADS), 0, s, a);
  else hipLaunchKernelGGL(det_kernel<false>, dim3(B), dim3(DET_THREADS), 0, s, a);
  return dod_launched("dod_detect");
}
