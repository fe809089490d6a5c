// COCO bbox evaluation on device: pycocotools' COCOeval (iouType 'bbox', useCats = 1, default parameters) restated operation
// for operation, from the records dod_postprocess compacts to the 12 summary numbers.  All evaluation arithmetic is double and
// no multiply-add is contracted anywhere in this file (the pragma below), so `da + ga - i` rounds twice as maskApi.c's does and
// every count, quotient and comparison equals the host library's.  DESIGN.md section 6b states the algorithm.
//
//   sort      stable LSD radix sort of (64-bit key, 32-bit payload) pairs, 8-bit digits: histogram -> scan -> scatter.  One wave
//             per 2048-key tile; inside a tile the keys are ranked 64 at a time in input order (ballot peers), so equal keys keep
//             their order: numpy's kind='mergesort'.  Descending doubles go through the order-preserving bit map.
//   group     detections ordered by (category index, image index), score descending, input order (two sorts); the rank inside a
//             group is the distance to the group's first position (binary search); ranks >= 100 (maxDets[-1]) drop out.
//   match     one wave per (image, category) group that has ground truth; lane a * 10 + t runs evaluateImg's greedy loop for area
//             range a and IoU threshold t serially over detections x ground truths, IoUs recomputed from LDS boxes (bbIou), so no
//             IoU matrix is stored and 1024 ground truths per group fit.  A ballot packs the 40 matched / 40 ignored bits.
//             Groups without ground truth need no matching: their detections are unmatched, ignored by area alone.
//   accumulate  detections re-ordered by (category, score descending), stable on (image, rank); one thread per (category, area,
//             maxDet, threshold) runs the integer cumulative sums forward (searchsorted positions) and backward (running maximum).
//   summarize one workgroup per statistic, a fixed-order tree sum.
//   append_detections  the fixed-shape output of dod_detect*: one workgroup per image sums the clamped counts of the images before it
//             (the exclusive scan, as a block reduction) and writes its rows behind them; one more workgroup advances the count.
//   confusion detections ordered by (image index, score descending, input order) with the same two sorts; one workgroup of four waves
//             per image holds the image's non-crowd ground truths of all categories in LDS (<= 1024), walks the candidates serially
//             and takes, lanes parallel over the ground truths, the arg-max IoU under a total order (IoU, then the later ground
//             truth), so the reduction's shape cannot change the answer.  Counts go to the matrix by integer atomics.
// No atomics on results, no float atomics anywhere: two evaluations of the same input are bit-identical.
#pragma clang fp contract(off)
#include "dod_internal.h"

using namespace dod;

namespace {

typedef unsigned long long u64;
typedef long long i64;

constexpr int kT = 10, kR = 101, kA = 4, kM = 3;
constexpr int kMaxDet = 100;                      // maxDets[-1]
constexpr int kMaxGt = 1024;                      // ground truths per (image, category) group
constexpr i64 kMaxDets = (i64)1 << 24;            // detections held by one evaluator
constexpr i64 kMaxGts = (i64)1 << 26;
constexpr int kMaxIds = 1 << 24;                  // images, categories
constexpr int kTile = 2048;                       // keys per sort workgroup
constexpr int kMagic = 0x0c0c0e7a;
constexpr u64 kBits40 = ((u64)1 << 40) - 1;
constexpr int kMaxAppendImages = 1 << 16;         // images of one append_detections call (every workgroup sums the counts before it)
constexpr int kCfThreads = 256;                   // confusion: four waves per image
constexpr int kCfMaxGt = 1024;                    // non-crowd ground truths per image
constexpr int kCfSlots = kCfMaxGt / kCfThreads;   // ground truths a lane owns: g = tid + kCfThreads * slot
constexpr int kCfMaxK = 2048;
constexpr int kErrImage = 1, kErrScore = 2, kErrTruncated = 4, kErrLabel = 8;

struct Hdr {
  i64 count;            // detections appended so far (may exceed max_dets: then evaluate refuses)
  u64 score_or;         // OR of the scores' bit patterns: its trailing zero digits are skipped by the score sorts
  int err;              // 1 image id not in the annotations, 2 non-finite score, 4 a source buffer was truncated, 8 a label outside its map
  int ng;               // ground-truth groups
  int magic;
  int nbig;             // ground-truth groups of more than 64
  int max_img_gt;       // the most non-crowd ground truths one image has (all categories)
  int reserved;
};

struct CocoDet { i64 image_id; i64 category_id; double bbox[4]; double score; };      // == dod_coco_det
static_assert(sizeof(CocoDet) == sizeof(dod_coco_det) && sizeof(CocoDet) == 56, "dod_coco_det layout");

__device__ __constant__ double c_area_lo[kA] = {0.0, 0.0, 1024.0, 9216.0};
__device__ __constant__ double c_area_hi[kA] = {1e10, 1024.0, 9216.0, 1e10};

// ------------------------------------------------------------------------------------------------ workspace layout
struct Lay {
  size_t hdr, img_ids, cat_ids, iou_thr, rec_thr, gbox, garea, gcrowd, gkey, gstart, catg, npig, dets, keyA, keyB, valA, valB, hist,
      sidx, rank, catk, dm, dig, prec, rec, stats, istart, ilist, icat, total;
  int nb;
};

Lay layout(i64 cap, int I, int K, i64 G) {
  Lay L;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += align_up(bytes ? bytes : 1); return at; };
  const size_t c = (size_t)cap, g = (size_t)(G > 0 ? G : 1);
  L.nb = (int)((c + kTile - 1) / kTile);
  L.hdr = take(sizeof(Hdr));
  L.img_ids = take((size_t)I * 8);
  L.cat_ids = take((size_t)K * 8);
  L.iou_thr = take(kT * 8);
  L.rec_thr = take(kR * 8);
  L.gbox = take(g * 32);
  L.garea = take(g * 8);
  L.gcrowd = take(g);
  L.gkey = take(g * 8);
  L.gstart = take((g + 1) * 4);
  L.catg = take(((size_t)K + 1) * 4);
  L.npig = take(g * kA * 4);
  L.dets = take(c * sizeof(CocoDet));
  L.keyA = take(c * 8);
  L.keyB = take(c * 8);
  L.valA = take(c * 4);
  L.valB = take(c * 4);
  L.hist = take((size_t)L.nb * 256 * 4);
  L.sidx = take(c * 4);
  L.rank = take(c * 4);
  L.catk = take(c * 4);
  L.dm = take(c * 8);
  L.dig = take(c * 8);
  L.prec = take((size_t)kT * kR * K * kA * kM * 8);
  L.rec = take((size_t)kT * K * kA * kM * 8);
  L.stats = take(12 * 8);
  L.istart = take(((size_t)I + 1) * 4);      // per image: its non-crowd ground truths of all categories, (category index, file) order
  L.ilist = take(g * 4);                     //   their positions in gbox
  L.icat = take(g * 4);                      //   their category indices
  L.total = o;
  return L;
}

bool sizes_ok(i64 cap, int I, int K, i64 G) {
  return cap >= 1 && cap <= kMaxDets && I >= 1 && I <= kMaxIds && K >= 1 && K <= kMaxIds && G >= 0 && G <= kMaxGts;
}

template <class T> inline T* at(void* ws, size_t off) { return reinterpret_cast<T*>((char*)ws + off); }

// ------------------------------------------------------------------------------------------------ radix sort
__global__ __launch_bounds__(DOD_WAVE) void rs_hist_kernel(const u64* __restrict__ keys, i64 n, int shift, unsigned* __restrict__ hist,
                                                           int nb) {
  __shared__ unsigned h[256];
  const int lane = threadIdx.x;
  for (int d = lane; d < 256; d += DOD_WAVE) h[d] = 0;
  __syncthreads();
  const i64 base = (i64)blockIdx.x * kTile, end = base + kTile < n ? base + kTile : n;
  for (i64 i = base + lane; i < end; i += DOD_WAVE) atomicAdd(&h[(unsigned)(keys[i] >> shift) & 255u], 1u);      // integer counts: order-free
  __syncthreads();
  for (int d = lane; d < 256; d += DOD_WAVE) hist[(size_t)d * nb + blockIdx.x] = h[d];
}

// exclusive scan, in place, of the m = 256 * nb digit-major counts by one workgroup (totals <= 2^24 fit 32 bits)
__global__ __launch_bounds__(1024) void rs_scan_kernel(unsigned* __restrict__ hist, int m) {
  __shared__ unsigned part[1024];
  const int tid = threadIdx.x;
  const int per = (m + 1023) / 1024;
  const int lo = tid * per < m ? tid * per : m, hi = lo + per < m ? lo + per : m;
  unsigned s = 0;
  for (int i = lo; i < hi; ++i) s += hist[i];
  part[tid] = s;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const unsigned v = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  unsigned run = part[tid] - s;
  for (int i = lo; i < hi; ++i) { const unsigned c = hist[i]; hist[i] = run; run += c; }
}

__global__ __launch_bounds__(DOD_WAVE) void rs_scatter_kernel(const u64* __restrict__ kin, const unsigned* __restrict__ vin,
                                                              u64* __restrict__ kout, unsigned* __restrict__ vout, i64 n, int shift,
                                                              const unsigned* __restrict__ hist, int nb) {
  __shared__ unsigned off[256];
  const int lane = threadIdx.x;
  for (int d = lane; d < 256; d += DOD_WAVE) off[d] = hist[(size_t)d * nb + blockIdx.x];
  __syncthreads();
  const i64 base = (i64)blockIdx.x * kTile, end = base + kTile < n ? base + kTile : n;
  const u64 below = ((u64)1 << lane) - 1;
  for (i64 c = base; c < end; c += DOD_WAVE) {            // 64 keys at a time, in input order
    const i64 i = c + lane;
    const bool valid = i < end;
    const u64 k = valid ? kin[i] : 0;
    const unsigned d = (unsigned)(k >> shift) & 255u;
    u64 peers = __ballot(valid);                          // the lanes of this step that hold the same digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const u64 bm = __ballot(bit);
      peers &= bit ? bm : ~bm;
    }
    const unsigned r = (unsigned)__popcll(peers & below), cnt = (unsigned)__popcll(peers);
    const unsigned at0 = valid ? off[d] : 0;
    __syncthreads();
    if (valid && r == cnt - 1) off[d] = at0 + cnt;        // one lane per digit present
    __syncthreads();
    if (valid && at0 + r < (u64)n) { kout[at0 + r] = k; vout[at0 + r] = vin[i]; }
  }
}

__global__ __launch_bounds__(256) void rs_copy_kernel(const u64* __restrict__ kin, const unsigned* __restrict__ vin, u64* __restrict__ kout,
                                                      unsigned* __restrict__ vout, i64 n) {
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) { kout[i] = kin[i]; vout[i] = vin[i]; }
}

inline int grid_for(i64 n, int block) {
  const i64 g = (n + block - 1) / block;
  return (int)(g < 1 ? 1 : g > 65536 ? 65536 : g);
}

// sorts the pairs on key bits [b0, b1); ping-pongs between the two buffer pairs and returns which one holds the result
int sort_pairs(u64* k[2], unsigned* v[2], i64 n, int b0, int b1, unsigned* hist, hipStream_t s) {
  int cur = 0;
  const int nb = (int)((n + kTile - 1) / kTile);
  for (int shift = b0; shift < b1; shift += 8, cur ^= 1) {
    hipLaunchKernelGGL(rs_hist_kernel, dim3(nb), dim3(DOD_WAVE), 0, s, k[cur], n, shift, hist, nb);
    hipLaunchKernelGGL(rs_scan_kernel, dim3(1), dim3(1024), 0, s, hist, 256 * nb);
    hipLaunchKernelGGL(rs_scatter_kernel, dim3(nb), dim3(DOD_WAVE), 0, s, k[cur], v[cur], k[cur ^ 1], v[cur ^ 1], n, shift, hist, nb);
  }
  return cur;
}

inline int bits_for(u64 maxval) {      // digits (in bits) needed for keys <= maxval
  int b = 8;
  while (b < 64 && (maxval >> b)) b += 8;
  return b;
}

// ------------------------------------------------------------------------------------------------ detections
__device__ __forceinline__ int find_id(const i64* __restrict__ ids, int n, i64 x) {      // index of x in the sorted unique ids, or -1
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (ids[mid] < x) lo = mid + 1; else hi = mid; }
  return lo < n && ids[lo] == x ? lo : -1;
}

__device__ __forceinline__ i64 lower_bound_u64(const u64* __restrict__ a, i64 n, u64 x) {
  i64 lo = 0, hi = n;
  while (lo < hi) { const i64 mid = (lo + hi) >> 1; if (a[mid] < x) lo = mid + 1; else hi = mid; }
  return lo;
}

// the key whose ascending unsigned order is the DESCENDING order of the doubles; -0.0 ties with +0.0 as it does for numpy
__device__ __forceinline__ u64 score_key(double sc) {
  if (sc == 0.0) sc = 0.0;
  const u64 b = (u64)__double_as_longlong(sc);
  const u64 asc = (b >> 63) ? ~b : b | ((u64)1 << 63);
  return ~asc;
}

__global__ __launch_bounds__(256) void ce_append_kernel(const dod_detection* __restrict__ src, const i64* __restrict__ src_count, i64 max_n,
                                                        const Hdr* __restrict__ hdr, CocoDet* __restrict__ dets, i64 cap) {
  const i64 have = *src_count, n = have < max_n ? have : max_n, base = hdr->count;
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
    if (base < 0 || base + i >= cap) break;
    const dod_detection r = src[i];
    CocoDet d;
    d.image_id = r.image_id; d.category_id = r.category_id;
    for (int c = 0; c < 4; ++c) d.bbox[c] = (double)r.bbox[c];
    d.score = (double)r.score;
    dets[base + i] = d;
  }
}

__global__ void ce_bump_kernel(Hdr* hdr, const i64* __restrict__ src_count, i64 max_n) {
  const i64 have = *src_count;
  if (have < 0) { hdr->err |= 4; return; }
  if (have > max_n) hdr->err |= 4;
  hdr->count += have < max_n ? have : max_n;
}

__global__ void ce_reset_kernel(Hdr* hdr) { hdr->count = 0; hdr->score_or = 0; hdr->err = 0; }

struct DetSrc {      // the fixed-shape output of dod_detect / dod_detect_views / dod_fuse_views
  const float* boxes;        // [B, Kd, 4] xyxy
  const float* scores;       // [B, Kd]
  const int* labels;         // [B, Kd]
  const int* counts;         // [B]
  const i64* image_ids;      // [B]
  const i64* map;            // [n_map] or null
  int B, Kd, n_map;
};

__device__ __forceinline__ i64 clamped_count(int c, int Kd) { return c < 0 ? 0 : c > Kd ? Kd : c; }

// sum of v over the workgroup (blockDim.x == 256), in every thread; integers, so the order is free
__device__ __forceinline__ i64 block_sum_256(i64 v, i64* part) {
  const int tid = threadIdx.x;
  part[tid] = v;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (tid < d) part[tid] += part[tid + d];
    __syncthreads();
  }
  return part[0];
}

// workgroup b: rows 0 .. counts[b]-1 of image b go behind the evaluator's records and the rows of the images before b
__global__ __launch_bounds__(256) void ce_append_det_kernel(DetSrc p, Hdr* hdr, CocoDet* __restrict__ dets, i64 cap) {
  __shared__ i64 part[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  i64 before = 0;
  for (int j = tid; j < b; j += 256) before += clamped_count(p.counts[j], p.Kd);
  before = block_sum_256(before, part);
  const i64 have = hdr->count, base = have + before;
  const int cnt = (int)clamped_count(p.counts[b], p.Kd);
  const i64 img = p.image_ids[b];
  bool bad = false;
  for (int r = tid; r < cnt; r += 256) {
    const size_t row = (size_t)b * p.Kd + r;
    const int lab = p.labels[row];
    i64 cat = lab;
    if (p.map) {
      if (lab < 0 || lab >= p.n_map) bad = true; else cat = p.map[lab];
    }
    if (have < 0 || base + r >= cap) continue;
    const float* bx = p.boxes + row * 4;
    const double x1 = (double)bx[0], y1 = (double)bx[1], x2 = (double)bx[2], y2 = (double)bx[3];
    CocoDet d;
    d.image_id = img; d.category_id = cat;
    d.bbox[0] = x1; d.bbox[1] = y1; d.bbox[2] = x2 - x1; d.bbox[3] = y2 - y1;
    d.score = (double)p.scores[row];
    dets[base + r] = d;
  }
  if (bad) atomicOr(&hdr->err, kErrLabel);
}

__global__ __launch_bounds__(256) void ce_bump_det_kernel(Hdr* hdr, const int* __restrict__ counts, int B, int Kd) {
  __shared__ i64 part[256];
  i64 sum = 0, odd = 0;
  for (int j = threadIdx.x; j < B; j += 256) {
    const int c = counts[j];
    sum += clamped_count(c, Kd);
    odd += c < 0 || c > Kd;
  }
  sum = block_sum_256(sum, part);
  __syncthreads();
  odd = block_sum_256(odd, part);
  if (threadIdx.x == 0) {
    if (odd) hdr->err |= kErrTruncated;
    hdr->count += sum;
  }
}

// score keys with the input index as payload; checks image ids and scores
__global__ __launch_bounds__(256) void ce_key_kernel(const CocoDet* __restrict__ dets, i64 n, const i64* __restrict__ img_ids, int I,
                                                     u64* __restrict__ key, unsigned* __restrict__ val, Hdr* hdr) {
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  u64 bits = 0;
  int err = 0;
  if (i < n) {
    const double sc = dets[i].score;
    if (!(sc - sc == 0.0)) err |= 2;
    if (find_id(img_ids, I, dets[i].image_id) < 0) err |= 1;
    key[i] = score_key(sc);
    val[i] = (unsigned)i;
    bits = (u64)__double_as_longlong(sc);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { bits |= __shfl_xor(bits, o, DOD_WAVE); err |= __shfl_xor(err, o, DOD_WAVE); }
  if ((threadIdx.x & (DOD_WAVE - 1)) == 0) {
    if (bits) atomicOr(&hdr->score_or, bits);
    if (err) atomicOr(&hdr->err, err);
  }
}

// group key of the detection at each sorted position: category index * I + image index; K * I for a category the annotations lack
__global__ __launch_bounds__(256) void ce_gkey_kernel(const CocoDet* __restrict__ dets, const unsigned* __restrict__ val, i64 n,
                                                      const i64* __restrict__ img_ids, int I, const i64* __restrict__ cat_ids, int K,
                                                      u64* __restrict__ key) {
  const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const CocoDet* d = dets + val[j];
  const int ii = find_id(img_ids, I, d->image_id), kk = find_id(cat_ids, K, d->category_id);
  key[j] = ii < 0 || kk < 0 ? (u64)K * I : (u64)kk * I + ii;
}

// rank inside the group, the kept flag as a category key, and the bits of a detection no ground truth matches
__global__ __launch_bounds__(256) void ce_rank_kernel(const CocoDet* __restrict__ dets, const u64* __restrict__ skey,
                                                      const unsigned* __restrict__ sval, i64 n, int I, int K, int* __restrict__ sidx,
                                                      int* __restrict__ rank, int* __restrict__ catk, u64* __restrict__ dm,
                                                      u64* __restrict__ dig) {
  const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const u64 key = skey[j];
  const i64 r = j - lower_bound_u64(skey, n, key);
  const unsigned idx = sval[j];
  const bool kept = key < (u64)K * I && r < kMaxDet;
  sidx[j] = (int)idx;
  rank[j] = r < 0x7fffffff ? (int)r : 0x7fffffff;
  catk[j] = kept ? (int)(key / (u64)I) : K;
  const double area = dets[idx].bbox[2] * dets[idx].bbox[3];
  u64 ig = 0;
  for (int a = 0; a < kA; ++a)
    if (area < c_area_lo[a] || area > c_area_hi[a]) ig |= (u64)0x3ff << (a * kT);
  dm[j] = 0;
  dig[j] = ig;
}

// maskApi.c bbIou on xywh doubles
__device__ __forceinline__ double bb_iou(const double* __restrict__ d, const double* __restrict__ g, bool crowd) {
  const double ga = g[2] * g[3], da = d[2] * d[3];
  const double w = __builtin_fmin(d[2] + d[0], g[2] + g[0]) - __builtin_fmax(d[0], g[0]);
  if (w <= 0) return 0.0;
  const double h = __builtin_fmin(d[3] + d[1], g[3] + g[1]) - __builtin_fmax(d[1], g[1]);
  if (h <= 0) return 0.0;
  const double i = w * h;
  const double u = crowd ? da : da + ga - i;
  return i / u;
}

struct MatchArgs {
  const CocoDet* dets;
  const u64* skey;
  const int* sidx;
  i64 n;
  const u64* gkey;
  const int* gstart;
  const double* gbox;
  const double* garea;
  const unsigned char* gcrowd;
  const double* iou_thr;
  u64* dm;
  u64* dig;
  int* npig;
};

// One wave per ground-truth group; groups of at most 64 ground truths run in the GMAX = 64 instance (4 KB of LDS), the rest in the
// GMAX = 1024 one (60 KB): the launch of the other class returns at once.
template <int GMAX>
__global__ __launch_bounds__(DOD_WAVE) void ce_match_kernel(MatchArgs p) {
  __shared__ double gb[GMAX][4];
  __shared__ double ga[GMAX];
  __shared__ double db[kMaxDet][4];
  __shared__ unsigned gm[(GMAX + 31) / 32][DOD_WAVE];      // matched flags of the ground truths, one bit column per lane
  __shared__ unsigned short ord[kA][GMAX];                 // per area range: non-ignored ground truths first, each part in input order
  __shared__ int nn[kA];                                   // non-ignored ground truths per area range
  __shared__ unsigned char gc[GMAX];
  const int grp = blockIdx.x, lane = threadIdx.x;
  const int g0 = p.gstart[grp], G = p.gstart[grp + 1] - g0;
  if (G <= 0 || G > GMAX || (GMAX > 64 && G <= 64)) return;
  const u64 key = p.gkey[grp];
  const i64 d0 = lower_bound_u64(p.skey, p.n, key), d1 = lower_bound_u64(p.skey, p.n, key + 1);
  const int D = d1 - d0 < kMaxDet ? (int)(d1 - d0) : kMaxDet;
  for (int g = lane; g < G; g += DOD_WAVE) {
    for (int c = 0; c < 4; ++c) gb[g][c] = p.gbox[(size_t)(g0 + g) * 4 + c];
    ga[g] = p.garea[g0 + g];
    gc[g] = p.gcrowd[g0 + g];
  }
  for (int d = lane; d < D; d += DOD_WAVE) {
    const CocoDet* r = p.dets + p.sidx[d0 + d];
    for (int c = 0; c < 4; ++c) db[d][c] = r->bbox[c];
  }
  for (int w = 0; w < (G + 31) / 32; ++w) gm[w][lane] = 0;
  __syncthreads();
  if (lane < kA) {                                         // gtind = argsort(gtIg, kind='mergesort')
    const double lo = c_area_lo[lane], hi = c_area_hi[lane];
    int c = 0;
    for (int g = 0; g < G; ++g)
      if (!(gc[g] || ga[g] < lo || ga[g] > hi)) ord[lane][c++] = (unsigned short)g;
    nn[lane] = c;
    for (int g = 0; g < G; ++g)
      if (gc[g] || ga[g] < lo || ga[g] > hi) ord[lane][c++] = (unsigned short)g;
    p.npig[(size_t)grp * kA + lane] = nn[lane];
  }
  __syncthreads();
  const bool active = lane < kA * kT;
  const int a = active ? lane / kT : 0, t = active ? lane - a * kT : 0;
  const double thr = __builtin_fmin(p.iou_thr[t], 1 - 1e-10);
  const double alo = c_area_lo[a], ahi = c_area_hi[a];
  const int nnig = nn[a];
  for (int d = 0; d < D; ++d) {
    bool matched = false, ignored = false;
    if (active) {
      double iou = thr;
      int m = -1;
      bool mig = false;
      for (int q = 0; q < G; ++q) {
        const int g = ord[a][q];
        const bool gig = q >= nnig;
        if (((gm[g >> 5][lane] >> (g & 31)) & 1u) && !gc[g]) continue;      // already matched at this threshold, and not a crowd
        if (m > -1 && !mig && gig) break;                                   // matched to a regular gt, and on the ignored ones now
        const double v = bb_iou(db[d], gb[g], gc[g] != 0);
        if (v < iou) continue;
        iou = v; m = g; mig = gig;
      }
      if (m >= 0) {
        matched = true; ignored = mig;
        gm[m >> 5][lane] |= 1u << (m & 31);
      } else {
        const double area = db[d][2] * db[d][3];
        ignored = area < alo || area > ahi;
      }
    }
    const u64 mb = __ballot(matched), ib = __ballot(ignored);
    if (lane == 0) { p.dm[d0 + d] = mb & kBits40; p.dig[d0 + d] = ib & kBits40; }
  }
}

// ------------------------------------------------------------------------------------------------ confusion matrix
// image key of the detection at each score-sorted position: the image index of a candidate (known category, score >= threshold), I for
// the rest (an unknown image id was refused before this runs)
__global__ __launch_bounds__(256) void ce_ikey_kernel(const CocoDet* __restrict__ dets, const unsigned* __restrict__ val, i64 n,
                                                      const i64* __restrict__ img_ids, int I, const i64* __restrict__ cat_ids, int K,
                                                      double score_thr, u64* __restrict__ key) {
  const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const CocoDet* d = dets + val[j];
  const int ii = find_id(img_ids, I, d->image_id), kk = find_id(cat_ids, K, d->category_id);
  key[j] = ii >= 0 && kk >= 0 && d->score >= score_thr ? (u64)ii : (u64)I;
}

struct ConfArgs {
  const CocoDet* dets;
  const u64* skey;           // image keys, sorted
  const unsigned* sval;      // input positions in (image, score descending, input order) order
  i64 n;
  const i64* cat_ids;
  int K;
  const int* istart;
  const int* ilist;
  const int* icat;
  const double* gbox;
  double thr;                // min(iou_threshold, 1 - 1e-10)
  u64* matrix;               // [K+1, K+1]
};

// (v, g) beats (bv, bg): a higher IoU, or the same IoU at a later ground truth; g < 0 is "none".  A total order on distinct g, so any
// reduction tree finds the same maximum.
__device__ __forceinline__ bool cf_better(double v, int g, double bv, int bg) { return g >= 0 && (bg < 0 || v > bv || (v == bv && g > bg)); }

// One workgroup per image.  Lane tid owns the ground truths tid + 256 * slot and keeps their taken bits in a register; the candidates
// come 256 at a time through LDS and are matched one after the other: a wave-level butterfly, then the four waves' winners through LDS
// (two alternating rows, so one barrier per candidate is enough).
__global__ __launch_bounds__(kCfThreads) void ce_confusion_kernel(ConfArgs p) {
  __shared__ double gb[kCfMaxGt][4];
  __shared__ int gk[kCfMaxGt];
  __shared__ double cb[kCfThreads][4];
  __shared__ int ck[kCfThreads];
  __shared__ double wv[2][kCfThreads / DOD_WAVE];
  __shared__ int wg[2][kCfThreads / DOD_WAVE];
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & (DOD_WAVE - 1), wave = tid / DOD_WAVE;
  const int g0 = p.istart[img];
  int G = p.istart[img + 1] - g0;
  if (G > kCfMaxGt) G = kCfMaxGt;                          // the host refuses such an image before the launch
  for (int g = tid; g < G; g += kCfThreads) {
    const size_t at = (size_t)p.ilist[g0 + g] * 4;
    for (int c = 0; c < 4; ++c) gb[g][c] = p.gbox[at + c];
    gk[g] = p.icat[g0 + g];
  }
  const i64 d0 = lower_bound_u64(p.skey, p.n, (u64)img), d1 = lower_bound_u64(p.skey, p.n, (u64)img + 1);
  const size_t W = (size_t)p.K + 1;
  unsigned taken = 0;
  for (i64 c0 = d0; c0 < d1; c0 += kCfThreads) {
    const int m = d1 - c0 < kCfThreads ? (int)(d1 - c0) : kCfThreads;
    __syncthreads();                                       // the ground truths are staged; the chunk before this one is used up
    if (tid < m) {
      const CocoDet* r = p.dets + p.sval[c0 + tid];
      for (int c = 0; c < 4; ++c) cb[tid][c] = r->bbox[c];
      ck[tid] = find_id(p.cat_ids, p.K, r->category_id);
    }
    __syncthreads();
    if (G == 0) {                                          // nothing to match: every candidate is left over
      if (tid < m && ck[tid] >= 0) atomicAdd(&p.matrix[(size_t)ck[tid] * W + p.K], (u64)1);
      continue;
    }
    for (int d = 0; d < m; ++d) {
      double bv = 0.0;
      int bg = -1;
#pragma unroll
      for (int s = 0; s < kCfSlots; ++s) {
        const int g = tid + s * kCfThreads;
        if (g < G && !((taken >> s) & 1u)) {
          const double v = bb_iou(cb[d], gb[g], false);
          if (v >= p.thr && cf_better(v, g, bv, bg)) { bv = v; bg = g; }
        }
      }
#pragma unroll
      for (int o = DOD_WAVE / 2; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o, DOD_WAVE);
        const int og = __shfl_xor(bg, o, DOD_WAVE);
        if (cf_better(ov, og, bv, bg)) { bv = ov; bg = og; }
      }
      const int row = d & 1;
      if (lane == 0) { wv[row][wave] = bv; wg[row][wave] = bg; }
      __syncthreads();
      bv = wv[row][0]; bg = wg[row][0];
#pragma unroll
      for (int w = 1; w < kCfThreads / DOD_WAVE; ++w)
        if (cf_better(wv[row][w], wg[row][w], bv, bg)) { bv = wv[row][w]; bg = wg[row][w]; }
      if (bg >= 0 && (bg & (kCfThreads - 1)) == tid) taken |= 1u << (bg / kCfThreads);
      if (tid == 0 && ck[d] >= 0) atomicAdd(&p.matrix[(size_t)ck[d] * W + (bg >= 0 ? gk[bg] : p.K)], (u64)1);
    }
  }
#pragma unroll
  for (int s = 0; s < kCfSlots; ++s) {                     // the ground truths nothing took
    const int g = tid + s * kCfThreads;
    if (g < G && !((taken >> s) & 1u)) atomicAdd(&p.matrix[(size_t)p.K * W + gk[g]], (u64)1);
  }
}

__global__ __launch_bounds__(256) void ce_gather_score_kernel(const CocoDet* __restrict__ dets, const int* __restrict__ sidx, i64 n,
                                                              u64* __restrict__ key, unsigned* __restrict__ val) {
  const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  key[j] = score_key(dets[sidx[j]].score);
  val[j] = (unsigned)j;
}

__global__ __launch_bounds__(256) void ce_gather_cat_kernel(const int* __restrict__ catk, const unsigned* __restrict__ val, i64 n,
                                                            u64* __restrict__ key) {
  const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) key[j] = (u64)catk[val[j]];
}

__global__ __launch_bounds__(256) void ce_fill_kernel(double* __restrict__ p, i64 n, double v) {
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) p[i] = v;
}

// COCOeval.accumulate: thread (a, m, t) of category k.  ckey / cval: the positions sorted by (category, score descending).
__global__ __launch_bounds__(128) void ce_accum_kernel(const u64* __restrict__ ckey, const unsigned* __restrict__ cval, i64 n, int K,
                                                       const int* __restrict__ rank, const u64* __restrict__ dm, const u64* __restrict__ dig,
                                                       const int* __restrict__ catg, const int* __restrict__ npig_g,
                                                       const double* __restrict__ rec_thr, double* __restrict__ prec,
                                                       double* __restrict__ rec) {
  const int k = blockIdx.x, tid = threadIdx.x;
  if (tid >= kA * kM * kT) return;
  const int a = tid / (kM * kT), m = (tid / kT) % kM, t = tid % kT;
  i64 npig = 0;
  for (int g = catg[k]; g < catg[k + 1]; ++g) npig += npig_g[(size_t)g * kA + a];
  if (npig == 0) return;                                   // the cells keep -1
  const int maxdet = m == 0 ? 1 : m == 1 ? 10 : kMaxDet;
  const u64 bit = (u64)1 << (a * kT + t);
  const i64 lo = lower_bound_u64(ckey, n, (u64)k), hi = lower_bound_u64(ckey, n, (u64)k + 1);
  const size_t pstride = (size_t)K * kA * kM;
  double* P = prec + (((size_t)t * kR * K + k) * kA + a) * kM + m;          // cell r at P[r * pstride]
  // forward: cumulative tp; P[r] <- searchsorted(rc, recThrs[r], 'left') as an index into the kept detections
  i64 tp = 0, fp = 0, nd = 0;
  int r = 0;
  double rc = 0.0;
  const double np_ = (double)npig;
  for (i64 j = lo; j < hi; ++j) {
    const unsigned pos = cval[j];
    if (rank[pos] >= maxdet) continue;
    ++nd;
    if (!(dig[pos] & bit)) {
      if (dm[pos] & bit) { ++tp; rc = (double)tp / np_; } else ++fp;
    }
    while (r < kR && rc >= rec_thr[r]) { P[(size_t)r * pstride] = (double)(nd - 1); ++r; }
  }
  for (int q = r; q < kR; ++q) P[(size_t)q * pstride] = 0.0;               // recall never reached: q stays 0
  rec[(((size_t)t * K + k) * kA + a) * kM + m] = nd ? (double)tp / np_ : 0.0;
  // backward: pr = tp / (fp + tp + eps), its running maximum from the right, read at the recorded positions
  int rr = r - 1;
  double best = -1.0;
  i64 idx = nd;
  for (i64 j = hi - 1; j >= lo && rr >= 0; --j) {
    const unsigned pos = cval[j];
    if (rank[pos] >= maxdet) continue;
    --idx;
    const double pr = (double)tp / (((double)fp + (double)tp) + 2.220446049250313e-16);
    if (pr > best) best = pr;
    while (rr >= 0 && P[(size_t)rr * pstride] == (double)idx) { P[(size_t)rr * pstride] = best; --rr; }
    if (!(dig[pos] & bit)) {
      if (dm[pos] & bit) --tp; else --fp;
    }
  }
}

// COCOeval.summarize: statistic blockIdx.x = mean of the entries > -1 of its slice, -1 without any
__global__ __launch_bounds__(256) void ce_summarize_kernel(const double* __restrict__ prec, const double* __restrict__ rec, int K,
                                                           double* __restrict__ stats) {
  __shared__ double ssum[256];
  __shared__ i64 scnt[256];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int a = s < 6 ? (s < 3 ? 0 : s - 2) : (s < 9 ? 0 : s - 8);
  const int m = s < 6 ? 2 : (s < 9 ? s - 6 : 2);
  const int t0 = s == 1 ? 0 : s == 2 ? 5 : 0, t1 = s == 1 ? 1 : s == 2 ? 6 : kT;
  const int R = s < 6 ? kR : 1;
  const double* src = s < 6 ? prec : rec;
  const i64 per_t = (i64)R * K, total = (i64)(t1 - t0) * per_t;
  double sum = 0.0;
  i64 cnt = 0;
  for (i64 e = tid; e < total; e += 256) {
    const i64 t = t0 + e / per_t, rk = e % per_t;                          // rk = r * K + k
    const double v = src[((size_t)(t * per_t + rk) * kA + a) * kM + m];
    if (v > -1.0) { sum += v; ++cnt; }
  }
  ssum[tid] = sum; scnt[tid] = cnt;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (tid < d) { ssum[tid] += ssum[tid + d]; scnt[tid] += scnt[tid + d]; }
    __syncthreads();
  }
  if (tid == 0) stats[s] = scnt[0] ? ssum[0] / (double)scnt[0] : -1.0;
}

int check_ws(const void* ws, size_t bytes, i64 cap, int I, int K, i64 G, Lay* L) {
  if (!sizes_ok(cap, I, K, G))
    return fail(nullptr, DOD_ERR_INVALID, "coco_eval: sizes outside the limits (max_dets %lld <= %lld, images %d, categories %d, ground truths %lld)",
                (long long)cap, (long long)kMaxDets, I, K, (long long)G);
  *L = layout(cap, I, K, G);
  if (!ws || bytes < L->total) return fail(nullptr, DOD_ERR_STATE, "coco_eval: workspace of %zu bytes, %zu needed", ws ? bytes : (size_t)0, L->total);
  return DOD_OK;
}

// what evaluate and confusion refuse from the header alone, before any launch
int check_appended(const char* who, const Hdr& h, i64 max_dets) {
  if (h.magic != kMagic) return fail(nullptr, DOD_ERR_STATE, "%s: dod_coco_eval_set_gt has not run on this workspace", who);
  if (h.err & kErrTruncated)
    return fail(nullptr, DOD_ERR_INVALID, "%s: an appended record buffer was truncated (its count exceeds its capacity)", who);
  if (h.err & kErrLabel) return fail(nullptr, DOD_ERR_INVALID, "%s: an appended detection's label is outside its category map", who);
  if (h.count < 0 || h.count > max_dets)
    return fail(nullptr, DOD_ERR_INVALID, "%s: %lld detections were appended, max_dets is %lld", who, (long long)h.count, (long long)max_dets);
  return DOD_OK;
}

// ... and from the flags ce_key_kernel leaves
int check_keyed(const char* who, const Hdr& h) {
  if (h.err & kErrImage) return fail(nullptr, DOD_ERR_INVALID, "%s: a detection's image id is not in the annotations", who);
  if (h.err & kErrScore) return fail(nullptr, DOD_ERR_INVALID, "%s: a detection's score is not finite", who);
  return DOD_OK;
}

}  // namespace

extern "C" {

size_t dod_op_sort_pairs_workspace_bytes(int64_t n) {
  if (n <= 0 || n > kMaxDets) return 0;
  return align_up((size_t)((n + kTile - 1) / kTile) * 256 * 4);
}

int dod_op_sort_pairs_u64(uint64_t* keys, uint32_t* vals, uint64_t* keys_alt, uint32_t* vals_alt, int64_t n, int begin_bit, int end_bit,
                          void* workspace, size_t workspace_bytes, void* stream) {
  if (n == 0) return DOD_OK;
  if (!keys || !vals || !keys_alt || !vals_alt || n < 0 || n > kMaxDets || begin_bit < 0 || end_bit > 64 || begin_bit > end_bit ||
      (begin_bit & 7) || (end_bit & 7))
    return fail(nullptr, DOD_ERR_INVALID, "sort_pairs_u64: null buffer, n outside [0, 2^24] or bits not whole digits of [0, 64]");
  if (!workspace || workspace_bytes < dod_op_sort_pairs_workspace_bytes(n)) return fail(nullptr, DOD_ERR_STATE, "sort_pairs_u64: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  u64* k[2] = {(u64*)keys, (u64*)keys_alt};
  unsigned* v[2] = {vals, vals_alt};
  if (sort_pairs(k, v, n, begin_bit, end_bit, (unsigned*)workspace, s))
    hipLaunchKernelGGL(rs_copy_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, k[1], v[1], k[0], v[0], (i64)n);
  return hipGetLastError() == hipSuccess ? DOD_OK : fail(nullptr, DOD_ERR_HIP, "sort_pairs_u64: launch failed");
}

size_t dod_coco_eval_workspace_bytes(int64_t max_dets, int n_images, int n_categories, int64_t n_gt) {
  return sizes_ok(max_dets, n_images, n_categories, n_gt) ? layout(max_dets, n_images, n_categories, n_gt).total : 0;
}

int dod_coco_eval_set_gt(void* ws, size_t ws_bytes, int64_t max_dets, int I, int K, int64_t G, const int64_t* image_ids,
                         const int64_t* category_ids, const int64_t* gt_group, const double* gt_bbox, const double* gt_area,
                         const uint8_t* gt_iscrowd, const double* iou_thrs, const double* rec_thrs, void* stream) {
  Lay L;
  if (!image_ids || !category_ids || !iou_thrs || !rec_thrs || (G > 0 && (!gt_group || !gt_bbox || !gt_area || !gt_iscrowd)))
    return fail(nullptr, DOD_ERR_INVALID, "coco_eval_set_gt: null argument");
  if (!sizes_ok(max_dets, I, K, G)) return check_ws(ws, ws_bytes, max_dets, I, K, G, &L);
  for (int i = 1; i < I; ++i)
    if (image_ids[i] <= image_ids[i - 1]) return fail(nullptr, DOD_ERR_INVALID, "coco_eval_set_gt: image ids must be sorted and unique");
  for (int i = 1; i < K; ++i)
    if (category_ids[i] <= category_ids[i - 1]) return fail(nullptr, DOD_ERR_INVALID, "coco_eval_set_gt: category ids must be sorted and unique");
  // groups: runs of equal keys (the caller sorted the ground truths stably by key = category index * I + image index)
  std::vector<u64> gkey;
  std::vector<int> gstart, catg((size_t)K + 1, 0);
  const i64 nkeys = (i64)K * I;
  int nbig = 0;
  for (i64 g = 0; g < G; ++g) {
    if (gt_group[g] < 0 || gt_group[g] >= nkeys || (g && gt_group[g] < gt_group[g - 1]))
      return fail(nullptr, DOD_ERR_INVALID, "coco_eval_set_gt: group keys must be non-decreasing in [0, categories * images)");
    if (!g || gt_group[g] != gt_group[g - 1]) { gkey.push_back((u64)gt_group[g]); gstart.push_back((int)g); }
    if (g + 1 - gstart.back() == 65) ++nbig;
    if (g + 1 - gstart.back() > kMaxGt)
      return fail(nullptr, DOD_ERR_INVALID, "coco_eval_set_gt: more than %d ground truths in one (image, category) group", kMaxGt);
  }
  const int ng = (int)gkey.size();
  gstart.push_back((int)G);
  for (int g = 0; g < ng; ++g) ++catg[(size_t)(gkey[g] / (u64)I) + 1];
  for (int k = 0; k < K; ++k) catg[k + 1] += catg[k];
  // per image: its non-crowd ground truths of all categories; ascending position = (category index, file) order
  std::vector<int> istart((size_t)I + 1, 0), ilist, icat;
  for (i64 g = 0; g < G; ++g)
    if (!gt_iscrowd[g]) ++istart[(size_t)(gt_group[g] % I) + 1];
  int max_img_gt = 0;
  for (int i = 0; i < I; ++i) {
    if (istart[i + 1] > max_img_gt) max_img_gt = istart[i + 1];
    istart[i + 1] += istart[i];
  }
  ilist.resize((size_t)istart[I]);
  icat.resize((size_t)istart[I]);
  {
    std::vector<int> fill(istart.begin(), istart.end() - 1);
    for (i64 g = 0; g < G; ++g) {
      if (gt_iscrowd[g]) continue;
      const int at = fill[(size_t)(gt_group[g] % I)]++;
      ilist[at] = (int)g;
      icat[at] = (int)(gt_group[g] / I);
    }
  }
  if (int rc = check_ws(ws, ws_bytes, max_dets, I, K, G, &L)) return rc;
  hipStream_t s = (hipStream_t)stream;
  Hdr h = {0, 0, 0, ng, kMagic, nbig, max_img_gt, 0};
#define CE_UP(off, src, bytes) \
  if ((bytes) > 0) HIPCHK(nullptr, hipMemcpyAsync((char*)ws + (off), (src), (bytes), hipMemcpyHostToDevice, s))
  CE_UP(L.hdr, &h, sizeof h);
  CE_UP(L.img_ids, image_ids, (size_t)I * 8);
  CE_UP(L.cat_ids, category_ids, (size_t)K * 8);
  CE_UP(L.iou_thr, iou_thrs, (size_t)kT * 8);
  CE_UP(L.rec_thr, rec_thrs, (size_t)kR * 8);
  CE_UP(L.gbox, gt_bbox, (size_t)G * 32);
  CE_UP(L.garea, gt_area, (size_t)G * 8);
  CE_UP(L.gcrowd, gt_iscrowd, (size_t)G);
  CE_UP(L.gkey, gkey.data(), (size_t)ng * 8);
  CE_UP(L.gstart, gstart.data(), ((size_t)ng + 1) * 4);
  CE_UP(L.catg, catg.data(), ((size_t)K + 1) * 4);
  CE_UP(L.istart, istart.data(), ((size_t)I + 1) * 4);
  CE_UP(L.ilist, ilist.data(), ilist.size() * 4);
  CE_UP(L.icat, icat.data(), icat.size() * 4);
#undef CE_UP
  HIPCHK(nullptr, hipStreamSynchronize(s));               // the host vectors above go out of scope
  return DOD_OK;
}

int dod_coco_eval_reset(void* ws, size_t ws_bytes, int64_t max_dets, int I, int K, int64_t G, void* stream) {
  Lay L;
  if (int rc = check_ws(ws, ws_bytes, max_dets, I, K, G, &L)) return rc;
  hipLaunchKernelGGL(ce_reset_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, at<Hdr>(ws, L.hdr));
  return hipGetLastError() == hipSuccess ? DOD_OK : fail(nullptr, DOD_ERR_HIP, "coco_eval_reset: launch failed");
}

int dod_coco_eval_append(void* ws, size_t ws_bytes, int64_t max_dets, int I, int K, int64_t G, const dod_detection* records,
                         const int64_t* count, int64_t max_records, void* stream) {
  Lay L;
  if (!records || !count || max_records < 0) return fail(nullptr, DOD_ERR_INVALID, "coco_eval_append: null records / count or a negative capacity");
  if (int rc = check_ws(ws, ws_bytes, max_dets, I, K, G, &L)) return rc;
  if (max_records == 0) return DOD_OK;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ce_append_kernel, dim3(grid_for(max_records, 256)), dim3(256), 0, s, records, (const i64*)count, (i64)max_records,
                     at<Hdr>(ws, L.hdr), at<CocoDet>(ws, L.dets), (i64)max_dets);
  hipLaunchKernelGGL(ce_bump_kernel, dim3(1), dim3(1), 0, s, at<Hdr>(ws, L.hdr), (const i64*)count, (i64)max_records);
  return hipGetLastError() == hipSuccess ? DOD_OK : fail(nullptr, DOD_ERR_HIP, "coco_eval_append: launch failed");
}

int dod_coco_eval_append_host(void* ws, size_t ws_bytes, int64_t max_dets, int I, int K, int64_t G, const dod_coco_det* dets, int64_t n,
                              void* stream) {
  Lay L;
  if (n < 0 || (n > 0 && !dets)) return fail(nullptr, DOD_ERR_INVALID, "coco_eval_append_host: null detections or a negative count");
  if (int rc = check_ws(ws, ws_bytes, max_dets, I, K, G, &L)) return rc;
  if (n == 0) return DOD_OK;
  hipStream_t s = (hipStream_t)stream;
  Hdr h;
  HIPCHK(nullptr, hipMemcpyAsync(&h, (char*)ws + L.hdr, sizeof h, hipMemcpyDeviceToHost, s));
  HIPCHK(nullptr, hipStreamSynchronize(s));
  if (h.magic != kMagic) return fail(nullptr, DOD_ERR_STATE, "coco_eval_append_host: dod_coco_eval_set_gt has not run on this workspace");
  if (h.count < 0 || h.count > max_dets || n > max_dets - h.count)
    return fail(nullptr, DOD_ERR_INVALID, "coco_eval_append_host: %lld + %lld detections exceed max_dets = %lld", (long long)h.count, (long long)n,
                (long long)max_dets);
  HIPCHK(nullptr, hipMemcpyAsync((char*)ws + L.dets + (size_t)h.count * sizeof(CocoDet), dets, (size_t)n * sizeof(CocoDet), hipMemcpyHostToDevice, s));
  h.count += n;
  HIPCHK(nullptr, hipMemcpyAsync((char*)ws + L.hdr, &h.count, sizeof h.count, hipMemcpyHostToDevice, s));
  HIPCHK(nullptr, hipStreamSynchronize(s));
  return DOD_OK;
}

int dod_coco_eval_append_detections(void* ws, size_t ws_bytes, int64_t max_dets, int I, int K, int64_t G, const float* boxes,
                                    const float* scores, const int32_t* labels, const int32_t* counts, int B, int Kd,
                                    const int64_t* image_ids, const int64_t* category_map, int n_map, void* stream) {
  Lay L;
  if (!boxes || !scores || !labels || !counts || !image_ids)
    return fail(nullptr, DOD_ERR_INVALID, "coco_eval_append_detections: null boxes / scores / labels / counts / image_ids");
  if (B < 1 || B > kMaxAppendImages || Kd < 1)
    return fail(nullptr, DOD_ERR_INVALID, "coco_eval_append_detections: need 1 <= B <= %d images and Kd >= 1 rows, got B=%d Kd=%d", kMaxAppendImages, B, Kd);
  if (category_map && n_map < 1) return fail(nullptr, DOD_ERR_INVALID, "coco_eval_append_detections: a category map of %d entries", n_map);
  if (int rc = check_ws(ws, ws_bytes, max_dets, I, K, G, &L)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const DetSrc src = {boxes, scores, labels, counts, (const i64*)image_ids, (const i64*)category_map, B, Kd, category_map ? n_map : 0};
  hipLaunchKernelGGL(ce_append_det_kernel, dim3(B), dim3(256), 0, s, src, at<Hdr>(ws, L.hdr), at<CocoDet>(ws, L.dets), (i64)max_dets);
  hipLaunchKernelGGL(ce_bump_det_kernel, dim3(1), dim3(256), 0, s, at<Hdr>(ws, L.hdr), counts, B, Kd);
  return hipGetLastError() == hipSuccess ? DOD_OK : fail(nullptr, DOD_ERR_HIP, "coco_eval_append_detections: launch failed");
}

int dod_coco_eval_confusion(void* ws, size_t ws_bytes, int64_t max_dets, int I, int K, int64_t G, double score_threshold,
                            double iou_threshold, int64_t* matrix, void* stream) {
  Lay L;
  if (!matrix) return fail(nullptr, DOD_ERR_INVALID, "coco_eval_confusion: null matrix");
  if (score_threshold != score_threshold || iou_threshold != iou_threshold)
    return fail(nullptr, DOD_ERR_INVALID, "coco_eval_confusion: a threshold is NaN");
  if (int rc = check_ws(ws, ws_bytes, max_dets, I, K, G, &L)) return rc;
  if (K > kCfMaxK) return fail(nullptr, DOD_ERR_INVALID, "coco_eval_confusion: %d categories, at most %d", K, kCfMaxK);
  hipStream_t s = (hipStream_t)stream;
  Hdr* hdr = at<Hdr>(ws, L.hdr);
  Hdr h;
  HIPCHK(nullptr, hipMemcpyAsync(&h, hdr, sizeof h, hipMemcpyDeviceToHost, s));
  HIPCHK(nullptr, hipStreamSynchronize(s));
  if (int rc = check_appended("coco_eval_confusion", h, max_dets)) return rc;
  if (h.max_img_gt > kCfMaxGt)
    return fail(nullptr, DOD_ERR_INVALID, "coco_eval_confusion: an image has %d non-crowd ground truths, at most %d", h.max_img_gt, kCfMaxGt);
  const i64 n = h.count;
  const CocoDet* dets = at<CocoDet>(ws, L.dets);
  u64* k[2] = {at<u64>(ws, L.keyA), at<u64>(ws, L.keyB)};
  unsigned* v[2] = {at<unsigned>(ws, L.valA), at<unsigned>(ws, L.valB)};
  unsigned* hist = at<unsigned>(ws, L.hist);
  const i64* img_ids = at<i64>(ws, L.img_ids);
  const i64* cat_ids = at<i64>(ws, L.cat_ids);
  const int nblk = (int)((n + 255) / 256);
  int cur = 0;
  if (n > 0) {      // (image index, score descending, input order): evaluate's score sort, then a stable sort on the image key
    hipLaunchKernelGGL(ce_key_kernel, dim3(nblk), dim3(256), 0, s, dets, n, img_ids, I, k[0], v[0], hdr);
    HIPCHK(nullptr, hipMemcpyAsync(&h, hdr, sizeof h, hipMemcpyDeviceToHost, s));
    HIPCHK(nullptr, hipStreamSynchronize(s));
    if (int rc = check_keyed("coco_eval_confusion", h)) return rc;
    const int score_b0 = h.score_or ? (__builtin_ctzll(h.score_or) / 8) * 8 : 56;
    cur = sort_pairs(k, v, n, score_b0, 64, hist, s);
    hipLaunchKernelGGL(ce_ikey_kernel, dim3(nblk), dim3(256), 0, s, dets, v[cur], n, img_ids, I, cat_ids, K, score_threshold, k[cur]);
    u64* k2[2] = {k[cur], k[cur ^ 1]};
    unsigned* v2[2] = {v[cur], v[cur ^ 1]};
    cur ^= sort_pairs(k2, v2, n, 0, bits_for((u64)I), hist, s);
  }
  const size_t cells = ((size_t)K + 1) * ((size_t)K + 1);
  HIPCHK(nullptr, hipMemsetAsync(matrix, 0, cells * 8, s));
  const ConfArgs a = {dets, k[cur], v[cur], n, cat_ids, K, at<int>(ws, L.istart), at<int>(ws, L.ilist), at<int>(ws, L.icat),
                      at<double>(ws, L.gbox), iou_threshold < 1 - 1e-10 ? iou_threshold : 1 - 1e-10, (u64*)matrix};
  hipLaunchKernelGGL(ce_confusion_kernel, dim3(I), dim3(kCfThreads), 0, s, a);
  return hipGetLastError() == hipSuccess ? DOD_OK : fail(nullptr, DOD_ERR_HIP, "coco_eval_confusion: launch failed");
}

int dod_coco_eval_evaluate(void* ws, size_t ws_bytes, int64_t max_dets, int I, int K, int64_t G, double* stats, double* precision,
                           double* recall, int64_t* n_dets, int32_t* n_groups, void* stream) {
  Lay L;
  if (!stats) return fail(nullptr, DOD_ERR_INVALID, "coco_eval_evaluate: null stats");
  if (int rc = check_ws(ws, ws_bytes, max_dets, I, K, G, &L)) return rc;
  hipStream_t s = (hipStream_t)stream;
  Hdr* hdr = at<Hdr>(ws, L.hdr);
  Hdr h;
  HIPCHK(nullptr, hipMemcpyAsync(&h, hdr, sizeof h, hipMemcpyDeviceToHost, s));
  HIPCHK(nullptr, hipStreamSynchronize(s));
  if (int rc = check_appended("coco_eval_evaluate", h, max_dets)) return rc;
  const i64 n = h.count;
  const CocoDet* dets = at<CocoDet>(ws, L.dets);
  u64* k[2] = {at<u64>(ws, L.keyA), at<u64>(ws, L.keyB)};
  unsigned* v[2] = {at<unsigned>(ws, L.valA), at<unsigned>(ws, L.valB)};
  unsigned* hist = at<unsigned>(ws, L.hist);
  const i64* img_ids = at<i64>(ws, L.img_ids);
  const i64* cat_ids = at<i64>(ws, L.cat_ids);
  int *sidx = at<int>(ws, L.sidx), *rank = at<int>(ws, L.rank), *catk = at<int>(ws, L.catk);
  u64 *dm = at<u64>(ws, L.dm), *dig = at<u64>(ws, L.dig);
  double *prec = at<double>(ws, L.prec), *rec = at<double>(ws, L.rec), *dstats = at<double>(ws, L.stats);
  const i64 nprec = (i64)kT * kR * K * kA * kM, nrec = (i64)kT * K * kA * kM;
  const int nblk = (int)((n + 255) / 256);
  int score_b0 = 0;
  hipLaunchKernelGGL(ce_fill_kernel, dim3(grid_for(nprec, 256)), dim3(256), 0, s, prec, nprec, -1.0);
  hipLaunchKernelGGL(ce_fill_kernel, dim3(grid_for(nrec, 256)), dim3(256), 0, s, rec, nrec, -1.0);
  int cur = 0;
  if (n > 0) {
    hipLaunchKernelGGL(ce_key_kernel, dim3(nblk), dim3(256), 0, s, dets, n, img_ids, I, k[0], v[0], hdr);
    HIPCHK(nullptr, hipMemcpyAsync(&h, hdr, sizeof h, hipMemcpyDeviceToHost, s));
    HIPCHK(nullptr, hipStreamSynchronize(s));
    if (int rc = check_keyed("coco_eval_evaluate", h)) return rc;
    score_b0 = h.score_or ? (__builtin_ctzll(h.score_or) / 8) * 8 : 56;      // digits in which every score agrees sort nothing
    cur = sort_pairs(k, v, n, score_b0, 64, hist, s);
    hipLaunchKernelGGL(ce_gkey_kernel, dim3(nblk), dim3(256), 0, s, dets, v[cur], n, img_ids, I, cat_ids, K, k[cur]);
    {
      u64* k2[2] = {k[cur], k[cur ^ 1]};
      unsigned* v2[2] = {v[cur], v[cur ^ 1]};
      cur ^= sort_pairs(k2, v2, n, 0, bits_for((u64)K * I), hist, s);
    }
    hipLaunchKernelGGL(ce_rank_kernel, dim3(nblk), dim3(256), 0, s, dets, k[cur], v[cur], n, I, K, sidx, rank, catk, dm, dig);
  }
  if (h.ng > 0) {
    MatchArgs a = {dets, k[cur], sidx, n, at<u64>(ws, L.gkey), at<int>(ws, L.gstart), at<double>(ws, L.gbox), at<double>(ws, L.garea),
                   at<unsigned char>(ws, L.gcrowd), at<double>(ws, L.iou_thr), dm, dig, at<int>(ws, L.npig)};
    hipLaunchKernelGGL(ce_match_kernel<64>, dim3(h.ng), dim3(DOD_WAVE), 0, s, a);
    if (h.nbig > 0) hipLaunchKernelGGL(ce_match_kernel<kMaxGt>, dim3(h.ng), dim3(DOD_WAVE), 0, s, a);
  }
  if (n > 0) {                                            // positions re-ordered by (category, score descending)
    hipLaunchKernelGGL(ce_gather_score_kernel, dim3(nblk), dim3(256), 0, s, dets, sidx, n, k[0], v[0]);
    cur = sort_pairs(k, v, n, score_b0, 64, hist, s);
    hipLaunchKernelGGL(ce_gather_cat_kernel, dim3(nblk), dim3(256), 0, s, catk, v[cur], n, k[cur]);
    u64* k2[2] = {k[cur], k[cur ^ 1]};
    unsigned* v2[2] = {v[cur], v[cur ^ 1]};
    cur ^= sort_pairs(k2, v2, n, 0, bits_for((u64)K), hist, s);
  }
  hipLaunchKernelGGL(ce_accum_kernel, dim3(K), dim3(128), 0, s, k[cur], v[cur], n, K, rank, dm, dig, at<int>(ws, L.catg), at<int>(ws, L.npig),
                     at<double>(ws, L.rec_thr), prec, rec);
  hipLaunchKernelGGL(ce_summarize_kernel, dim3(12), dim3(256), 0, s, prec, rec, K, dstats);
  if (hipGetLastError() != hipSuccess) return fail(nullptr, DOD_ERR_HIP, "coco_eval_evaluate: launch failed");
  HIPCHK(nullptr, hipMemcpyAsync(stats, dstats, 12 * 8, hipMemcpyDeviceToHost, s));
  if (precision) HIPCHK(nullptr, hipMemcpyAsync(precision, prec, (size_t)nprec * 8, hipMemcpyDeviceToDevice, s));
  if (recall) HIPCHK(nullptr, hipMemcpyAsync(recall, rec, (size_t)nrec * 8, hipMemcpyDeviceToDevice, s));
  HIPCHK(nullptr, hipStreamSynchronize(s));
  if (n_dets) *n_dets = n;
  if (n_groups) *n_groups = h.ng;
  return DOD_OK;
}

int dod_coco_eval_matches(const void* ws, size_t ws_bytes, int64_t max_dets, int I, int K, int64_t G, int64_t n_dets, int32_t* det_index,
                          int32_t* det_rank, uint64_t* matched, uint64_t* ignored, int32_t n_groups, uint64_t* group_keys, int32_t* npig,
                          void* stream) {
  Lay L;
  if (int rc = check_ws(ws, ws_bytes, max_dets, I, K, G, &L)) return rc;
  if (n_dets < 0 || n_dets > max_dets || n_groups < 0 || n_groups > G) return fail(nullptr, DOD_ERR_INVALID, "coco_eval_matches: counts outside the workspace");
  hipStream_t s = (hipStream_t)stream;
  const char* w = (const char*)ws;
  const size_t n = (size_t)n_dets, g = (size_t)n_groups;
#define CE_DN(dst, off, bytes) \
  if ((dst) && (bytes) > 0) HIPCHK(nullptr, hipMemcpyAsync((dst), w + (off), (bytes), hipMemcpyDeviceToDevice, s))
  CE_DN(det_index, L.sidx, n * 4);
  CE_DN(det_rank, L.rank, n * 4);
  CE_DN(matched, L.dm, n * 8);
  CE_DN(ignored, L.dig, n * 8);
  CE_DN(group_keys, L.gkey, g * 8);
  CE_DN(npig, L.npig, g * kA * 4);
#undef CE_DN
  return DOD_OK;
}

}  // extern "C"
