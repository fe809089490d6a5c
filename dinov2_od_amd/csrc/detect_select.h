// What dod_detect (detect.hip) and dod_detect_views (detect_views.hip) share: the order-preserving key image of a logit, the 56-bit
// select word, stages 1 - 3 of the one-workgroup-per-image design -- key pass, radix select of the K-th largest word, gather and
// bitonic sort in LDS (det_sort_desc, which the fusing merge of detect_views.hip runs a second time over its fused scores) -- and
// stage 5, greedy NMS through a bit matrix in LDS, and the output tail of every entry point: the row store, the padding row and
// det_finish (rows as sorted, or NMS and ordered compaction).
#pragma once
// The rounding contract of every file that includes this header, set here and not in the build script: no multiply-add is contracted
// from here to the end of the translation unit, so each fp32 operation rounds once.
//   dod_detect: `cx - 0.5 w` then `* width`; stage 5's `iou * union`.
//   dod_detect_views: the same, plus the view mapping (`x * vw` then `+ vl`) and the edge test (`vl + m`).
//   dod_fuse_views: `sum + s * x` is a rounded product, then a rounded sum, and `mean * T / N` rounds twice.
#pragma clang fp contract(off)
#include "dod_common.h"

#define DET_THREADS 1024
#define DET_WAVES (DET_THREADS / DOD_WAVE)
#define DET_MAX_K 1024           // one thread per output row
#define DET_MAX_PAIRS (1 << 20)  // candidates per image: the index field of the select word
#define DET_COPIES 8
#define DET_UNROLL 8
#define DET_HSTRIDE 257          // 256 bins + 1: the copies of one bin sit on different banks

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
// the key of logit x of class c, or 0 when the pair is no candidate: a class below first_class, a NaN, a score not above the threshold
__device__ __forceinline__ unsigned det_cand_key(int c, float x, int first_class, float threshold) {
  const bool cand = c >= first_class && x == x && (threshold < 0.0f || det_sigmoid(x) > threshold);
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

// the LDS of stages 1 - 3 (a __shared__ object of the calling kernel)
struct DetSelectLds {
  unsigned hist[DET_COPIES * DET_HSTRIDE];
  unsigned long long sel[DET_MAX_K];
  unsigned long long prefix;
  unsigned kk, done, cnt;
};

// The n <= DET_MAX_K words sel[0 .. n) (written, not yet fenced) sorted descending, by all DET_THREADS threads: a bitonic network over
// the next power of two, words n .. P - 1 filled with 0.  n is uniform over the workgroup; ends behind a barrier.
__device__ __forceinline__ void det_sort_desc(unsigned long long* sel, int n, int tid) {
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
}

// Stages 1 - 3 for the N flat indices of one image, by all DET_THREADS threads of the workgroup: kp[i] = make_key(i, load(i)) (0 = no
// candidate), the K largest words det_word(key, i) of the candidates into L.sel[0 .. n), sorted descending; returns n <= K.
template <class Load, class MakeKey>
__device__ __forceinline__ int det_select_sort(DetSelectLds& L, int N, int K, int tid, unsigned* kp, Load load, MakeKey make_key) {
  const int lane = tid & 63, wave = tid >> 6;
  if (tid == 0) L.cnt = 0;

  // ---- 1 + 2: keys, and the threshold word Tc: selected <=> key != 0 && word >= Tc
  unsigned long long Tc = 0;
  if (N < K) {                                   // everything that is a candidate is selected
    det_for_each(N, tid, load, [&](int i, float x) { kp[i] = make_key(i, x); });
    __syncthreads();
  } else {
    unsigned long long prefix = 0;
    unsigned kk = (unsigned)K;                   // rank still wanted among the words that share `prefix` above the current digit
    for (int shift = 48; shift >= 0; shift -= 8) {
      for (int j = tid; j < DET_COPIES * DET_HSTRIDE; j += DET_THREADS) L.hist[j] = 0;
      __syncthreads();
      unsigned* const hcopy = L.hist + (lane & (DET_COPIES - 1)) * DET_HSTRIDE;
      if (shift == 48)
        det_for_each(N, tid, load, [&](int i, float x) {
          const unsigned key = make_key(i, x);
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
          for (int cp = 0; cp < DET_COPIES; ++cp) n += L.hist[cp * DET_HSTRIDE + d];
          c4[j] = n; s += n;
        }
        unsigned incl = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const unsigned v = __shfl_up(incl, o, 64); if (lane >= o) incl += v; }
        unsigned above = incl - s;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (above < kk && kk <= above + c4[j]) {
            L.prefix = prefix | ((unsigned long long)(255 - (4 * lane + j)) << shift);
            L.kk = kk - above;
            L.done = c4[j] == kk - above ? 1u : 0u;     // the whole bin is wanted: lower digits need no pass
          }
          above += c4[j];
        }
      }
      __syncthreads();
      prefix = L.prefix; kk = L.kk;
      if (L.done) break;
    }
    Tc = prefix;
  }

  // ---- 3: gather and sort
  det_for_each(N, tid, [&](int i) { return kp[i]; }, [&](int i, unsigned key) {
    const unsigned long long w = det_word(key, i);
    if (key != 0u && w >= Tc) {
      const unsigned slot = atomicAdd(&L.cnt, 1u);
      if (slot < DET_MAX_K) L.sel[slot] = w;
    }
  });
  __syncthreads();
  const int n = (int)(L.cnt < (unsigned)K ? L.cnt : (unsigned)K);
  det_sort_desc(L.sel, n, tid);
  return n;
}

// ---- stage 5: greedy NMS over n <= MAXK sorted candidates.  The relation "i suppresses j" only has bits for j > i, so row i is kept
// from its 64-bit word i >> 6 on (upper-triangular): 64 * W (W + 1) / 2 words for W = MAXK / 64 -- 18 KiB at 512, 68 KiB at 1024, where
// the full matrix would take 128 KiB of the CU's 160.
template <int MAXK>
struct DetNmsLds {
  static constexpr int W = MAXK / 64;
  float4 box[MAXK];
  float area[MAXK];
  int lab[MAXK];
  unsigned long long mat[64 * (W * (W + 1) / 2)];
  unsigned long long rem[W];
};
// word w >= i >> 6 of row i: the rows of block g = i >> 6 hold W - g words each
template <int W>
__device__ __forceinline__ int det_tri(int i, int w) {
  const int g = i >> 6;
  return 64 * (W * g - ((g * (g - 1)) >> 1)) + (i & 63) * (W - g) + (w - g);
}
// By all DET_THREADS threads; thread t < n passes candidate t's output box and label.  j is suppressed by an earlier survivor i when
// (agnostic or label_i == label_j) and inter > iou * union, or with `ios` inter > iou * min(area_i, area_j).  Afterwards bit t of the
// words S.rem says "t was removed".  One ballot per 64 pairs, a serial sweep by one wave that carries the removed set as one 64-bit
// word per lane.
template <int MAXK>
__device__ __forceinline__ void det_nms(DetNmsLds<MAXK>& S, int n, int tid, float4 box, int lab, float iou, bool agnostic, bool ios) {
  constexpr int W = MAXK / 64;
  const int lane = tid & 63, wave = tid >> 6;
  if (tid < n) {
    S.box[tid] = box;
    S.area[tid] = det_max(0.0f, box.z - box.x) * det_max(0.0f, box.w - box.y);
    S.lab[tid] = lab;
  }
  __syncthreads();
  const int words = (n + 63) >> 6;
  for (int w = 0; w < words; ++w) {                          // word w of every row i with i >> 6 <= w: bit j - 64w says "i suppresses j", j > i only
    const int j = w * 64 + lane;                             // this lane's column stays in registers for all rows of the word
    const bool jin = j < n;
    const float4 bj = jin ? S.box[j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float aj = jin ? S.area[j] : 0.0f;
    const int lj = jin ? S.lab[j] : -2;
    const int rows = n < w * 64 + 64 ? n : w * 64 + 64;
    for (int i = wave; i < rows; i += DET_WAVES) {           // the row's box, area and label are wave-uniform reads that depend on nothing
      const float4 bi = S.box[i];
      const float ai = S.area[i];
      const int li = S.lab[i];
      bool bit = false;
      if (j > i && jin && (agnostic || li == lj)) {
        const float iw = det_max(0.0f, det_min(bi.z, bj.z) - det_max(bi.x, bj.x));
        const float ih = det_max(0.0f, det_min(bi.w, bj.w) - det_max(bi.y, bj.y));
        const float inter = iw * ih;
        const float uni = (ai + aj) - inter;
        bit = inter > iou * (ios ? det_min(ai, aj) : uni);
      }
      const unsigned long long m = __ballot(bit);
      if (lane == 0) S.mat[det_tri<W>(i, w)] = m;
    }
  }
  __syncthreads();
  if (wave == 0) {                                           // lane l carries word l of the removed set
    unsigned long long rem = 0;
    for (int i0 = 0; i0 < n; i0 += 8) {                      // eight rows are loaded before the first decision: they do not depend on it
      unsigned long long row[8];
      const int g = i0 >> 6, first = det_tri<W>(i0, lane);   // the eight rows lie in one block of 64: W - g words apart
#pragma unroll
      for (int u = 0; u < 8; ++u)                            // words below the diagonal do not exist: they hold no bit
        row[u] = (lane < words && lane >= g && i0 + u < n) ? S.mat[first + u * (W - g)] : 0ull;
#pragma unroll
      for (int u = 0; u < 8; ++u) {                          // a row past n is 0: it changes nothing
        const int i = i0 + u;
        const unsigned lo = __builtin_amdgcn_readlane((unsigned)rem, i >> 6), hi = __builtin_amdgcn_readlane((unsigned)(rem >> 32), i >> 6);
        const unsigned long long mine = ((unsigned long long)hi << 32) | lo;
        if (!((mine >> (i & 63)) & 1ull)) rem |= row[u];
      }
    }
    if (lane < W) S.rem[lane] = lane < words ? rem : 0ull;
  }
  __syncthreads();
}
// after det_nms: the number of survivors, and in `rank` how many of them stand in front of candidate tid (its output row if it survived)
template <int MAXK>
__device__ __forceinline__ int det_nms_rank(const DetNmsLds<MAXK>& S, int n, int tid, int& rank) {
  const int words = (n + 63) >> 6;
  int total = 0;
  rank = 0;
  for (int w = 0; w < words; ++w) {
    const int left = n - 64 * w;
    const unsigned long long valid = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
    const unsigned long long kept = ~S.rem[w] & valid;
    total += __popcll(kept);
    if (w < (tid >> 6)) rank += __popcll(kept);
    else if (w == (tid >> 6)) rank += __popcll(kept & ((1ull << (tid & 63)) - 1ull));
  }
  return total;
}

// ---- the output tail: where the rows of a call go ([B, K] each, boxes as float4 rows; views / members null in an entry point that has
// none), one row, and the row every padding position gets
struct DetOut { float* scores; int* labels; int* views; int* queries; float* boxes; int* members; int* counts; };
struct DetRow { float score; int label, view, query; float4 box; int members; };
__device__ __forceinline__ DetRow det_pad_row() { return DetRow{0.0f, -1, -1, -1, make_float4(0.0f, 0.0f, 0.0f, 0.0f), 0}; }
__device__ __forceinline__ void det_store(const DetOut& out, const DetRow& row, size_t r) {
  out.scores[r] = row.score; out.labels[r] = row.label; out.queries[r] = row.query;
  reinterpret_cast<float4*>(out.boxes)[r] = row.box;
  if (out.views) out.views[r] = row.view;
  if (out.members) out.members[r] = row.members;
}
// By all DET_THREADS threads, behind stage 4: thread t < n holds sorted candidate t in `row`, thread t >= n the padding row.  NMSK == 0
// writes the rows as they are and the count n.  Otherwise stage 5 (n <= K <= NMSK: the host picks the instance): greedy NMS, the
// survivors compacted in order into rows 0 .. total - 1, padding behind them, the count total.
template <int NMSK>
__device__ __forceinline__ void det_finish(const DetOut& out, int b, int K, int n, int tid, const DetRow& row, float iou, bool agnostic, bool ios) {
  const size_t o = (size_t)b * K;
  if constexpr (NMSK == 0) {
    if (tid < K) det_store(out, row, o + tid);
    if (tid == 0) out.counts[b] = n;
  } else {
    __shared__ DetNmsLds<NMSK> S;
    det_nms(S, n, tid, row.box, row.label, iou, agnostic, ios);
    int rank;
    const int total = det_nms_rank(S, n, tid, rank);
    if (tid >= total && tid < K) det_store(out, det_pad_row(), o + tid);
    if (tid < n && !((S.rem[tid >> 6] >> (tid & 63)) & 1ull)) det_store(out, row, o + rank);   // a survivor moves to row rank <= tid, rank < total
    if (tid == 0) out.counts[b] = total;
  }
}
