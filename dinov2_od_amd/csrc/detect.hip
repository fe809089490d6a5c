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
//   5. NMS: a bit-matrix of the K x K suppression relation in LDS (one ballot per 64 pairs), a serial sweep by one wave that carries
//      the removed set as one 64-bit word per lane, and an ordered compaction by population count.
// The box and IoU arithmetic must round once per operation: this file is compiled with -ffp-contract=off (_build.EXTRA).
#include "dod_common.h"
#include "../../include/dinodet.h"

#define DET_THREADS 1024
#define DET_WAVES (DET_THREADS / DOD_WAVE)
#define DET_MAX_K 1024           // one thread per output row
#define DET_NMS_MAX_K 512        // the suppression matrix: 512 x 512 bits = 32 KiB of LDS
#define DET_MAX_PAIRS (1 << 20)  // Q*C: the index field of the select word
#define DET_COPIES 8
#define DET_UNROLL 8
#define DET_HSTRIDE 257          // 256 bins + 1: the copies of one bin sit on different banks

struct DetArgs {
  const float* det; const float* sizes; unsigned* keys;
  float* scores; int* labels; int* queries; float* boxes; int* counts;
  int Q, C, first_class, K;
  float threshold, iou;
  int agnostic, clamp;
};

// torch.sigmoid in fp32, as pp_sigmoid (postproc.hip)
__device__ __forceinline__ float det_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
// larger logit <=> larger key; +0.0 (0x80000000) ranks above -0.0 (0x7FFFFFFF); 0 only for the all-ones NaN
__device__ __forceinline__ unsigned det_key(float x) {
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long det_word(unsigned key, int i) {
  return ((unsigned long long)key << 24) | ((unsigned long long)(0xFFFFFu - (unsigned)i) << 4);
}
__device__ __forceinline__ float det_logit(const DetArgs& a, const float* dp, int i) {
  const int q = i / a.C, c = i - q * a.C;
  return dp[(size_t)q * (a.C + 4) + c];
}
__device__ __forceinline__ unsigned det_make_key(const DetArgs& a, int i, float x) {
  const int c = i % a.C;
  const bool cand = c >= a.first_class && x == x && (a.threshold < 0.0f || det_sigmoid(x) > a.threshold);
  return cand ? det_key(x) : 0u;
}
// use(i, load(i)) for every i < N of this thread (i = tid, tid + 1024, ...), DET_UNROLL loads in flight before the first use: a pass is
// a few dozen elements per thread, and one L2 round trip per element would be most of its time
template <class Load, class Use>
__device__ __forceinline__ void det_for_each(int N, int tid, Load load, Use use) {
  for (int base = tid; base < N; base += DET_UNROLL * DET_THREADS) {
    decltype(load(0)) v[DET_UNROLL];
#pragma unroll
    for (int u = 0; u < DET_UNROLL; ++u) {
      const int i = base + u * DET_THREADS;
      v[u] = i < N ? load(i) : decltype(load(0))();
    }
#pragma unroll
    for (int u = 0; u < DET_UNROLL; ++u) {
      const int i = base + u * DET_THREADS;
      if (i < N) use(i, v[u]);
    }
  }
}
__device__ __forceinline__ float det_clamp(float v, float hi) { return v < 0.0f ? 0.0f : (v > hi ? hi : v); }
__device__ __forceinline__ float det_min(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float det_max(float a, float b) { return a > b ? a : b; }

template <bool NMS>
__global__ __launch_bounds__(DET_THREADS) void det_kernel(const DetArgs a) {
  __shared__ unsigned hist[DET_COPIES * DET_HSTRIDE];
  __shared__ unsigned long long sel[DET_MAX_K];
  __shared__ unsigned long long s_prefix;
  __shared__ unsigned s_kk, s_done, s_cnt;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, C = a.C, K = a.K;
  const int N = a.Q * C;
  const float* dp = a.det + (size_t)b * a.Q * (C + 4);
  unsigned* kp = a.keys + (size_t)b * N;
  if (tid == 0) s_cnt = 0;

  // ---- 1 + 2: keys, and the threshold word Tc: selected <=> key != 0 && word >= Tc
  unsigned long long Tc = 0;
  if (N < K) {                                   // everything that is a candidate is selected
    det_for_each(N, tid, [&](int i) { return det_logit(a, dp, i); }, [&](int i, float x) { kp[i] = det_make_key(a, i, x); });
    __syncthreads();
  } else {
    unsigned long long prefix = 0;
    unsigned kk = (unsigned)K;                   // rank still wanted among the words that share `prefix` above the current digit
    for (int shift = 48; shift >= 0; shift -= 8) {
      for (int j = tid; j < DET_COPIES * DET_HSTRIDE; j += DET_THREADS) hist[j] = 0;
      __syncthreads();
      unsigned* const hcopy = hist + (lane & (DET_COPIES - 1)) * DET_HSTRIDE;
      if (shift == 48)
        det_for_each(N, tid, [&](int i) { return det_logit(a, dp, i); }, [&](int i, float x) {
          const unsigned key = det_make_key(a, i, x);
          kp[i] = key;
          atomicAdd(&hcopy[key >> 24], 1u);
        });
      else
        det_for_each(N, tid, [&](int i) { return kp[i]; }, [&](int i, unsigned key) {
          const unsigned long long w = det_word(key, i);
          if ((w >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hcopy[(unsigned)((w >> shift) & 255u)], 1u);
        });
      __syncthreads();
      if (wave == 0) {                           // lane l owns digits 255-4l .. 252-4l: a prefix sum over lanes walks the digits downwards
        unsigned c4[4], s = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int d = 255 - (4 * lane + j);
          unsigned n = 0;
#pragma unroll
          for (int cp = 0; cp < DET_COPIES; ++cp) n += hist[cp * DET_HSTRIDE + d];
          c4[j] = n; s += n;
        }
        unsigned incl = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const unsigned v = __shfl_up(incl, o, 64); if (lane >= o) incl += v; }
        unsigned above = incl - s;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (above < kk && kk <= above + c4[j]) {
            s_prefix = prefix | ((unsigned long long)(255 - (4 * lane + j)) << shift);
            s_kk = kk - above;
            s_done = c4[j] == kk - above ? 1u : 0u;     // the whole bin is wanted: lower digits need no pass
          }
          above += c4[j];
        }
      }
      __syncthreads();
      prefix = s_prefix; kk = s_kk;
      if (s_done) break;
    }
    Tc = prefix;
  }

  // ---- 3: gather and sort
  det_for_each(N, tid, [&](int i) { return kp[i]; }, [&](int i, unsigned key) {
    const unsigned long long w = det_word(key, i);
    if (key != 0u && w >= Tc) {
      const unsigned slot = atomicAdd(&s_cnt, 1u);
      if (slot < DET_MAX_K) sel[slot] = w;
    }
  });
  __syncthreads();
  const int n = (int)(s_cnt < (unsigned)K ? s_cnt : (unsigned)K);
  int P = 1;
  while (P < n) P <<= 1;
  if (tid >= n && tid < P) sel[tid] = 0;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (tid < (P >> 1)) {
        const int lo = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), hi = lo + j;
        const unsigned long long x = sel[lo], y = sel[hi];
        const bool desc = (lo & k) == 0;
        if ((x < y) == desc) { sel[lo] = y; sel[hi] = x; }
      }
      __syncthreads();
    }

  // ---- 4: thread t decodes word t
  float sc = 0.0f, x1 = 0.0f, y1 = 0.0f, x2 = 0.0f, y2 = 0.0f;
  int lab = -1, qi = -1;
  if (tid < n) {
    const int idx = (int)(0xFFFFFu - (unsigned)((sel[tid] >> 4) & 0xFFFFFu));
    qi = idx / C; lab = idx - qi * C;
    const float* row = dp + (size_t)qi * (C + 4);
    sc = det_sigmoid(row[lab]);
    const float cx = row[C], cy = row[C + 1], w = row[C + 2], h = row[C + 3];
    const float ih = a.sizes ? a.sizes[2 * b] : 1.0f, iw = a.sizes ? a.sizes[2 * b + 1] : 1.0f;
    x1 = cx - 0.5f * w; y1 = cy - 0.5f * h; x2 = cx + 0.5f * w; y2 = cy + 0.5f * h;
    x1 *= iw; y1 *= ih; x2 *= iw; y2 *= ih;
    if (a.clamp) { x1 = det_clamp(x1, iw); y1 = det_clamp(y1, ih); x2 = det_clamp(x2, iw); y2 = det_clamp(y2, ih); }
  }
  const size_t o = (size_t)b * K;
  if constexpr (!NMS) {
    if (tid < K) {
      a.scores[o + tid] = sc; a.labels[o + tid] = lab; a.queries[o + tid] = qi;
      reinterpret_cast<float4*>(a.boxes)[o + tid] = make_float4(x1, y1, x2, y2);
    }
    if (tid == 0) a.counts[b] = n;
  } else {
    // ---- 5: greedy NMS over the n sorted candidates (n <= DET_NMS_MAX_K: the host refuses a larger K)
    __shared__ float4 nbox[DET_NMS_MAX_K];
    __shared__ float narea[DET_NMS_MAX_K];
    __shared__ int nlab[DET_NMS_MAX_K];
    __shared__ unsigned long long mat[DET_NMS_MAX_K * (DET_NMS_MAX_K / 64)];
    __shared__ unsigned long long remw[DET_NMS_MAX_K / 64];
    if (tid < n) {
      nbox[tid] = make_float4(x1, y1, x2, y2);
      narea[tid] = det_max(0.0f, x2 - x1) * det_max(0.0f, y2 - y1);
      nlab[tid] = lab;
    }
    __syncthreads();
    const int words = (n + 63) >> 6;
    for (int w = 0; w < words; ++w) {                          // word w of every row i with i >> 6 <= w: bit j - 64w says "i suppresses j", j > i only
      const int j = w * 64 + lane;                             // this lane's column stays in registers for all rows of the word
      const bool jin = j < n;
      const float4 bj = jin ? nbox[j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      const float aj = jin ? narea[j] : 0.0f;
      const int lj = jin ? nlab[j] : -2;
      const int rows = n < w * 64 + 64 ? n : w * 64 + 64;
      for (int i = wave; i < rows; i += DET_WAVES) {           // the row's box, area and label are wave-uniform reads that depend on nothing
        const float4 bi = nbox[i];
        const float ai = narea[i];
        const int li = nlab[i];
        bool bit = false;
        if (j > i && jin && (a.agnostic || li == lj)) {
          const float iw = det_max(0.0f, det_min(bi.z, bj.z) - det_max(bi.x, bj.x));
          const float ih = det_max(0.0f, det_min(bi.w, bj.w) - det_max(bi.y, bj.y));
          const float inter = iw * ih;
          const float uni = (ai + aj) - inter;
          bit = inter > a.iou * uni;
        }
        const unsigned long long m = __ballot(bit);
        if (lane == 0) mat[i * words + w] = m;
      }
    }
    __syncthreads();
    if (wave == 0) {                                           // lane l carries word l of the removed set
      unsigned long long rem = 0;
      for (int i0 = 0; i0 < n; i0 += 8) {                      // eight rows are loaded before the first decision: they do not depend on it
        unsigned long long row[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)                            // words below the diagonal were never written: they hold no bit
          row[u] = (lane < words && lane >= ((i0 + u) >> 6) && i0 + u < n) ? mat[(i0 + u) * words + lane] : 0ull;
#pragma unroll
        for (int u = 0; u < 8; ++u) {                          // a row past n is 0: it changes nothing
          const int i = i0 + u;
          const unsigned lo = __builtin_amdgcn_readlane((unsigned)rem, i >> 6), hi = __builtin_amdgcn_readlane((unsigned)(rem >> 32), i >> 6);
          const unsigned long long mine = ((unsigned long long)hi << 32) | lo;
          if (!((mine >> (i & 63)) & 1ull)) rem |= row[u];
        }
      }
      if (lane < DET_NMS_MAX_K / 64) remw[lane] = lane < words ? rem : 0ull;
    }
    __syncthreads();
    int total = 0, rank = 0;
    for (int w = 0; w < words; ++w) {
      const int left = n - 64 * w;
      const unsigned long long valid = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
      const unsigned long long kept = ~remw[w] & valid;
      total += __popcll(kept);
      if (w < (tid >> 6)) rank += __popcll(kept);
      else if (w == (tid >> 6)) rank += __popcll(kept & ((1ull << (tid & 63)) - 1ull));
    }
    if (tid >= total && tid < K) {                             // padding rows
      a.scores[o + tid] = 0.0f; a.labels[o + tid] = -1; a.queries[o + tid] = -1;
      reinterpret_cast<float4*>(a.boxes)[o + tid] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    if (tid < n && !((remw[tid >> 6] >> (tid & 63)) & 1ull)) { // a survivor moves to row rank <= tid, rank < total
      a.scores[o + rank] = sc; a.labels[o + rank] = lab; a.queries[o + rank] = qi;
      reinterpret_cast<float4*>(a.boxes)[o + rank] = make_float4(x1, y1, x2, y2);
    }
    if (tid == 0) a.counts[b] = total;
  }
}

static inline size_t det_align(size_t x) { return (x + 255) & ~(size_t)255; }

static bool det_shape_ok(int B, int Q, int C, int K) {
  return B > 0 && Q > 0 && C >= 1 && K >= 1 && K <= DET_MAX_K && (long long)Q * C <= DET_MAX_PAIRS;
}

extern "C" size_t dod_detect_workspace_bytes(int B, int Q, int C, int K) {
  if (!det_shape_ok(B, Q, C, K)) return 0;
  return det_align((size_t)B * Q * C * sizeof(unsigned));
}

extern "C" int dod_detect(const float* det, int B, int Q, int C, int first_class, const float* sizes, float threshold, int K,
                          float iou_threshold, int class_agnostic, int clamp, float* scores, int32_t* labels, int32_t* queries,
                          float* boxes, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
  if (!det || !scores || !labels || !queries || !boxes || !counts) return DOD_ERR_INVALID;
  if (!det_shape_ok(B, Q, C, K) || first_class < 0 || first_class >= C) return DOD_ERR_INVALID;
  const bool nms = iou_threshold >= 0.0f;
  if (nms && K > DET_NMS_MAX_K) return DOD_ERR_INVALID;
  if (((uintptr_t)boxes & 15) != 0) return DOD_ERR_INVALID;      // rows are stored as float4
  if (!workspace || workspace_bytes < dod_detect_workspace_bytes(B, Q, C, K)) return DOD_ERR_INVALID;
  DetArgs a;
  a.det = det; a.sizes = sizes; a.keys = (unsigned*)workspace;
  a.scores = scores; a.labels = labels; a.queries = queries; a.boxes = boxes; a.counts = counts;
  a.Q = Q; a.C = C; a.first_class = first_class; a.K = K;
  a.threshold = threshold; a.iou = iou_threshold;
  a.agnostic = class_agnostic; a.clamp = clamp;
  hipStream_t s = (hipStream_t)stream;
  if (nms) hipLaunchKernelGGL(det_kernel<true>, dim3(B), dim3(DET_THREADS), 0, s, a);
  else hipLaunchKernelGGL(det_kernel<false>, dim3(B), dim3(DET_THREADS), 0, s, a);
  return hipGetLastError() == hipSuccess ? DOD_OK : DOD_ERR_HIP;
}
