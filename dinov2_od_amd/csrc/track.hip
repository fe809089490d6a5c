// Multi-object tracking on device (dod_track_update): ByteTrack association behind dod_detect, one launch per frame for any number of
// independent streams, the track table resident on the device.  include/dinodet.h states the semantics; tests/track_cases.py restates
// them in numpy + scipy, and the result equals that restatement bit for bit: the filter arithmetic is double with one rounding per
// operation (the whole file is compiled without FMA contraction, as warp.hip is), the three association problems are solved by the
// solver assign.hip uses (lsap.h: scipy's linear_sum_assignment, ties included), and everything else is integer bookkeeping.
//
// One workgroup of one wave64 per stream -- the width lsap_solve is written for -- so the streams of a launch run side by side and
// nothing crosses a workgroup: no global atomics, no allocation, no host sync.  Inside the workgroup
//   lanes over rows    classify the detections (ignored / low / high); ordered compaction by ballot + prefix count keeps row order
//   lanes over slots   predict, the state changes between the passes, expiry; the same compaction keeps slot order
//   lanes over elements of the compacted cost matrix, written to the caller's workspace (at most T * K floats per stream); both sides
//                      (slot boxes, detection boxes, scores, labels) are staged in LDS first, so the element loop reads no global memory
//   lsap_solve         three times (high pass, low pass, tentative pass), its state in LDS when rows + columns fits, else in the workspace
//   lanes over matched pairs for the Kalman update: the pairs of one solution touch distinct slots and distinct rows
// The lists (slot list, high rows, low rows, the slot every row ended on) live in LDS.  Every loop is bounded by T or K; the solver's
// by the column count.
//
// dod_track_update_app is the same kernel instantiated a second time (template on a bool): the first and the tentative pass take
// min(that cost, the gated appearance distance) from the similarity matrix dod_track_embed_dots wrote (the strided-batched fp32 GEMM), and
// every row leaves with slot + 1024 * kind in `assoc`, which dod_track_embed_commit turns into the slots' smoothed embeddings.  The slots'
// embeddings are a tensor of the caller's; the table and the plain instantiation are what they were.
#include "dod_common.h"
#include "../../include/dinodet.h"
#include "lsap.h"
#include <type_traits>

#pragma clang fp contract(off)

namespace {

constexpr int kTrkMaxT = 512, kTrkMaxK = 1024, kTrkMaxS = 65535;
// LSAP state kept in LDS: 32 KiB beside the 16 KiB of lists below.  rows + columns above this (at most T + K = 1536) goes to the workspace.
constexpr int kTrkLdsUnits = 1024;
// Before the solver starts the same region stages both sides of the cost matrix: slot boxes (4 doubles), then per detection row 4 + 1
// floats and a label -- 16 + 24 KiB, which sizes the region
constexpr int kTrkSlotBoxBytes = kTrkMaxT * 4 * (int)sizeof(double);
constexpr int kTrkLdsBytes = kTrkSlotBoxBytes + kTrkMaxK * 6 * 4;
static_assert(kTrkLdsBytes >= kTrkLdsUnits * kUnitBytes, "the staging region also holds the solver state");
static_assert(kTrkLdsUnits <= kLdsUnits, "the tracker's LDS share of the solver state is bounded by the solver's own budget");
enum { TRK_FREE = 0, TRK_TENTATIVE = 1, TRK_TRACKED = 2, TRK_LOST = 3 };

// ByteTrack's KalmanFilter constants
constexpr double kStdPos = 1.0 / 20, kStdVel = 1.0 / 160;
constexpr double kInitPos = 2.0 * kStdPos, kInitVel = 10.0 * kStdVel;
constexpr double kAspInit = 1e-2, kAspVel = 1e-5, kAspMeas = 1e-1;

// the table: the arrays dod_track_export writes, in that order, every one starting 256 bytes apart
struct TrkTable {
  double *mean, *cov;                       // [S, T, 8] (cx, cy, a, h, and their velocities), [S, T, 4 x (p, c, v)]
  int *state, *id, *label, *last;           // [S, T]
  float* score;                             // [S, T]
  int *frame, *next_id, *overflow;          // [S]
};

__host__ __device__ inline size_t trk_up(size_t x) { return (x + 255) / 256 * 256; }

__host__ __device__ inline size_t trk_carve(unsigned char* base, int S, int T, TrkTable* t) {
  const size_t n = (size_t)S * T;
  size_t off = 0;
  auto take = [&](size_t bytes) { unsigned char* p = base ? base + off : nullptr; off += trk_up(bytes); return p; };
  unsigned char* p;
  p = take(n * 8 * sizeof(double)); if (t) t->mean = reinterpret_cast<double*>(p);
  p = take(n * 12 * sizeof(double)); if (t) t->cov = reinterpret_cast<double*>(p);
  p = take(n * 4); if (t) t->state = reinterpret_cast<int*>(p);
  p = take(n * 4); if (t) t->id = reinterpret_cast<int*>(p);
  p = take(n * 4); if (t) t->label = reinterpret_cast<int*>(p);
  p = take(n * 4); if (t) t->last = reinterpret_cast<int*>(p);
  p = take(n * 4); if (t) t->score = reinterpret_cast<float*>(p);
  p = take((size_t)S * 4); if (t) t->frame = reinterpret_cast<int*>(p);
  p = take((size_t)S * 4); if (t) t->next_id = reinterpret_cast<int*>(p);
  p = take((size_t)S * 4); if (t) t->overflow = reinterpret_cast<int*>(p);
  return off;
}

struct TrkArgs {
  TrkTable tab;
  int T, K;
  const float* scores; const int* labels; const float* boxes; const int* counts;
  dod_track_params p;
  int* ids; float* track_boxes;
  unsigned char* workspace;
  size_t cost_bytes, stream_bytes;          // of one stream's share of the workspace: the cost matrix, then the solver state
};

// dod_track_update_app: the same arguments, the similarity matrix, the two gates and the one new output
struct TrkAppArgs : TrkArgs {
  const float* dots;                        // [S, T, K]
  float app_thresh, prox_thresh;
  int* assoc;                               // [S, K]
};
constexpr int kTrkKind = 1024;              // assoc = slot + kTrkKind * kind; a slot is below kTrkMaxT
static_assert(kTrkMaxT <= kTrkKind, "a slot index fits below the kind");

__device__ __forceinline__ bool trk_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// ordered compaction, one 64-wide step: every lane calls it; returns the new count
__device__ __forceinline__ int trk_push(bool pred, int value, int* list, int count) {
  const unsigned long long m = __ballot(pred);
  if (pred) list[count + __popcll(m & ((1ull << threadIdx.x) - 1ull))] = value;
  return count + __popcll(m);
}

// the measurement (cx, cy, a, h) of an fp32 xyxy box, in double from the widened values
__device__ __forceinline__ void trk_measure(const float* __restrict__ b, double z[4]) {
  const double x1 = (double)b[0], y1 = (double)b[1], x2 = (double)b[2], y2 = (double)b[3];
  const double w = x2 - x1, h = y2 - y1;
  z[0] = x1 + 0.5 * w;
  z[1] = y1 + 0.5 * h;
  z[2] = w / h;
  z[3] = h;
}

__device__ __forceinline__ void trk_xyxy(const double* __restrict__ m, double b[4]) {
  const double w = m[2] * m[3];
  b[0] = m[0] - 0.5 * w;
  b[1] = m[1] - 0.5 * m[3];
  b[2] = m[0] + 0.5 * w;
  b[3] = m[1] + 0.5 * m[3];
}

__device__ __forceinline__ void trk_predict(double* __restrict__ m, double* __restrict__ P) {
  const double sp = kStdPos * m[3], sv = kStdVel * m[3];
  const double qp = sp * sp, qv = sv * sv;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const double qpc = c == 2 ? kAspInit * kAspInit : qp, qvc = c == 2 ? kAspVel * kAspVel : qv;
    const double p = P[3 * c], cc = P[3 * c + 1], v = P[3 * c + 2];
    m[c] = m[c] + m[4 + c];
    P[3 * c] = (((p + cc) + cc) + v) + qpc;
    P[3 * c + 1] = cc + v;
    P[3 * c + 2] = v + qvc;
  }
}

__device__ __forceinline__ void trk_correct(double* __restrict__ m, double* __restrict__ P, const double z[4]) {
  const double sp = kStdPos * m[3];
  const double r = sp * sp;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const double rc = c == 2 ? kAspMeas * kAspMeas : r;
    const double p = P[3 * c], cc = P[3 * c + 1], v = P[3 * c + 2];
    const double s = p + rc;
    const double kp = p / s, kv = cc / s;
    const double y = z[c] - m[c];
    m[c] = m[c] + kp * y;
    m[4 + c] = m[4 + c] + kv * y;
    P[3 * c] = p - (kp * kp) * s;
    P[3 * c + 1] = cc - (kp * kv) * s;
    P[3 * c + 2] = v - (kv * kv) * s;
  }
}

__device__ __forceinline__ void trk_init(double* __restrict__ m, double* __restrict__ P, const double z[4]) {
  const double sp = kInitPos * z[3], sv = kInitVel * z[3];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    m[c] = z[c];
    m[4 + c] = 0.0;
    P[3 * c] = c == 2 ? kAspInit * kAspInit : sp * sp;
    P[3 * c + 1] = 0.0;
    P[3 * c + 2] = c == 2 ? kAspVel * kAspVel : sv * sv;
  }
}

__device__ __forceinline__ double trk_iou(const double a[4], const double b[4]) {
  const double lx = a[0] < b[0] ? b[0] : a[0], ly = a[1] < b[1] ? b[1] : a[1];
  const double hx = a[2] < b[2] ? a[2] : b[2], hy = a[3] < b[3] ? a[3] : b[3];
  double iw = hx - lx, ih = hy - ly;
  iw = iw > 0.0 ? iw : 0.0;
  ih = ih > 0.0 ? ih : 0.0;
  double aw = a[2] - a[0], ah = a[3] - a[1], bw = b[2] - b[0], bh = b[3] - b[1];
  aw = aw > 0.0 ? aw : 0.0; ah = ah > 0.0 ? ah : 0.0; bw = bw > 0.0 ? bw : 0.0; bh = bh > 0.0 ? bh : 0.0;
  const double inter = iw * ih;
  const double uni = (aw * ah + bw * bh) - inter;
  return uni > 0.0 ? inter / uni : 0.0;
}

// One association pass of stream s: the slots rows[0 .. nr) against the detection rows cols[0 .. nc).  All lanes call it with uniform
// arguments.  A kept pair is a hit: Kalman update, TRACKED, last = frame, the slot takes the row's score and label, slot_of[row] = slot.
// APP (the first and the tentative pass of dod_track_update_app): the cost is min(today's cost, the gated appearance distance), and
// slot_of[row] carries kind 1 (slot + kTrkKind): the row's embedding is to be blended into the slot's.
template <bool APP>
__device__ __forceinline__ void trk_associate(const std::conditional_t<APP, TrkAppArgs, TrkArgs>& a, size_t s, const int* rows, int nr, const int* cols, int nc, bool fuse, float thresh,
                                              int frame, float* __restrict__ cost, unsigned char* lds, unsigned char* wstate, int* slot_of, int* slabel) {
  if (nr == 0 || nc == 0) return;
  const int lane = threadIdx.x;
  const size_t t0 = s * a.T, r0 = s * a.K;
  // both sides staged in LDS first -- the solver's region is free until lsap_solve starts -- so that the element loop reads no global
  // memory: slot boxes as doubles [nr][4] and labels, detection boxes [nc][4], scores and labels
  double* sbox = reinterpret_cast<double*>(lds);
  float* cbox = reinterpret_cast<float*>(lds + kTrkSlotBoxBytes);
  float* cscore = cbox + 4 * kTrkMaxK;
  int* clabel = reinterpret_cast<int*>(cscore + kTrkMaxK);
  for (int i = lane; i < nr; i += DOD_WAVE) {
    const int t = rows[i];
    trk_xyxy(a.tab.mean + (t0 + t) * 8, sbox + 4 * i);
    slabel[i] = a.tab.label[t0 + t];
  }
  for (int k = lane; k < nc; k += DOD_WAVE) {
    const int j = cols[k];
    const float* bx = a.boxes + (r0 + j) * 4;
    cbox[4 * k] = bx[0]; cbox[4 * k + 1] = bx[1]; cbox[4 * k + 2] = bx[2]; cbox[4 * k + 3] = bx[3];
    cscore[k] = a.scores[r0 + j];
    clabel[k] = a.labels[r0 + j];
  }
  __syncthreads();
  for (int e = lane; e < nr * nc; e += DOD_WAVE) {
    const int i = e / nc, k = e % nc;
    double db[4];
    db[0] = (double)cbox[4 * k]; db[1] = (double)cbox[4 * k + 1]; db[2] = (double)cbox[4 * k + 2]; db[3] = (double)cbox[4 * k + 3];
    double iou = trk_iou(sbox + 4 * i, db);
    if (a.p.class_aware && slabel[i] != clabel[k]) iou = 0.0;
    if constexpr (APP) {
      const double d_iou = 1.0 - iou;
      const double base = fuse ? 1.0 - iou * (double)cscore[k] : d_iou;
      const double gap = 1.0 - (double)a.dots[(t0 + rows[i]) * a.K + cols[k]];
      double d_app = 0.5 * (gap > 0.0 ? gap : 0.0);
      if (d_app > (double)a.app_thresh) d_app = 1.0;
      if (d_iou > (double)a.prox_thresh) d_app = 1.0;
      cost[e] = (float)(d_app < base ? d_app : base);
    } else {
      if (fuse) iou = iou * (double)cscore[k];
      cost[e] = (float)(1.0 - iou);
    }
  }
  __syncthreads();
  const bool tr = nc < nr;                   // scipy solves the transpose when columns < rows
  const int lr = tr ? nc : nr, lc = tr ? nr : nc;
  Lsap ls;
  int st;
  if (nr + nc <= kTrkLdsUnits) {
    ls = lsap_carve(lds, lr, lc);
    st = lsap_solve(ls, cost, nc, tr, lr, lc);
  } else {
    ls = lsap_carve(wstate, lr, lc);
    st = lsap_solve(ls, cost, nc, tr, lr, lc);
  }
  __syncthreads();
  if (st == 0) {
    for (int i = lane; i < nr; i += DOD_WAVE) {
      const int c = tr ? ls.row4col[i] : ls.col4row[i];
      if (c < 0 || !(cost[i * nc + c] <= thresh)) continue;
      const int t = rows[i], j = cols[c];
      double z[4];
      trk_measure(a.boxes + (r0 + j) * 4, z);
      trk_correct(a.tab.mean + (t0 + t) * 8, a.tab.cov + (t0 + t) * 12, z);
      a.tab.state[t0 + t] = TRK_TRACKED;
      a.tab.last[t0 + t] = frame;
      a.tab.score[t0 + t] = a.scores[r0 + j];
      a.tab.label[t0 + t] = a.labels[r0 + j];
      slot_of[j] = APP ? t + kTrkKind : t;
    }
  }
  __syncthreads();
}

// APP = dod_track_update_app: in that instantiation slot_of[row] holds slot + kTrkKind * kind (0: second pass, 1: first or tentative pass, 2: birth,
// at every frame), which the last loop writes out as `assoc` and takes apart again for the ids
template <bool APP>
__global__ __launch_bounds__(DOD_WAVE) void track_update_kernel(std::conditional_t<APP, TrkAppArgs, TrkArgs> a) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kTrkLdsBytes];
  __shared__ int hi[kTrkMaxK], lo[kTrkMaxK], slot_of[kTrkMaxK], rows[kTrkMaxT], slabel[kTrkMaxT];
  const int lane = threadIdx.x, T = a.T, K = a.K;
  const size_t s = blockIdx.x, t0 = s * T, r0 = s * K;
  const TrkTable& tab = a.tab;
  float* cost = reinterpret_cast<float*>(a.workspace + s * a.stream_bytes);
  unsigned char* wstate = a.workspace + s * a.stream_bytes + a.cost_bytes;
  // 0. count the frame; classify the rows
  const int frame = tab.frame[s] + 1;
  int cnt = a.counts[s];
  cnt = cnt < 0 ? 0 : (cnt > K ? K : cnt);
  int nhi = 0, nlo = 0;
  for (int base = 0; base < K; base += DOD_WAVE) {
    const int j = base + lane;
    int cls = 0;
    if (j < cnt) {
      const float sc = a.scores[r0 + j];
      const float* b = a.boxes + (r0 + j) * 4;
      const bool valid = trk_finite(sc) && trk_finite(b[0]) && trk_finite(b[1]) && trk_finite(b[2]) && trk_finite(b[3]) && b[2] > b[0] && b[3] > b[1];
      if (valid) cls = sc > a.p.track_thresh ? 2 : (sc > a.p.low_thresh ? 1 : 0);
    }
    if (j < K) slot_of[j] = -1;
    nhi = trk_push(cls == 2, j, hi, nhi);
    nlo = trk_push(cls == 1, j, lo, nlo);
  }
  // 1. predict; first pass rows = TRACKED and LOST slots
  int n = 0;
  for (int base = 0; base < T; base += DOD_WAVE) {
    const int t = base + lane;
    const int st = t < T ? tab.state[t0 + t] : TRK_FREE;
    if (st != TRK_FREE) {
      double* m = tab.mean + (t0 + t) * 8;
      if (st == TRK_LOST) m[7] = 0.0;
      trk_predict(m, tab.cov + (t0 + t) * 12);
    }
    n = trk_push(st == TRK_TRACKED || st == TRK_LOST, t, rows, n);
  }
  __syncthreads();
  // 3. high pass
  trk_associate<APP>(a, s, rows, n, hi, nhi, a.p.fuse_score != 0, a.p.match_thresh, frame, cost, lds, wstate, slot_of, slabel);
  // 4. low pass: the TRACKED slots without a hit against the low rows, plain IoU
  n = 0;
  for (int base = 0; base < T; base += DOD_WAVE) {
    const int t = base + lane;
    n = trk_push(t < T && tab.state[t0 + t] == TRK_TRACKED && tab.last[t0 + t] != frame, t, rows, n);
  }
  __syncthreads();
  trk_associate<false>(a, s, rows, n, lo, nlo, false, a.p.second_thresh, frame, cost, lds, wstate, slot_of, slabel);
  // ... the ones still without a hit become LOST; 5. tentative pass against the high rows left over (the low list's storage is free now)
  n = 0;
  for (int base = 0; base < T; base += DOD_WAVE) {
    const int t = base + lane;
    int st = t < T ? tab.state[t0 + t] : TRK_FREE;
    if (st == TRK_TRACKED && tab.last[t0 + t] != frame) tab.state[t0 + t] = st = TRK_LOST;
    n = trk_push(st == TRK_TENTATIVE, t, rows, n);
  }
  int nleft = 0;
  for (int base = 0; base < nhi; base += DOD_WAVE) {
    const int i = base + lane;
    const int j = i < nhi ? hi[i] : 0;
    nleft = trk_push(i < nhi && slot_of[j] < 0, j, lo, nleft);
  }
  __syncthreads();
  trk_associate<APP>(a, s, rows, n, lo, nleft, a.p.fuse_score != 0, a.p.tentative_thresh, frame, cost, lds, wstate, slot_of, slabel);
  // tentative misses are freed; 6. expiry; the free slots in slot order
  n = 0;
  for (int base = 0; base < T; base += DOD_WAVE) {
    const int t = base + lane;
    int st = t < T ? tab.state[t0 + t] : TRK_TRACKED;
    if (st == TRK_TENTATIVE || (st == TRK_LOST && frame - tab.last[t0 + t] > a.p.max_age)) tab.state[t0 + t] = st = TRK_FREE;
    n = trk_push(st == TRK_FREE, t, rows, n);
  }
  // 7. birth: the high rows still without a slot and with score >= new_thresh, in row order (the high list's storage is free now)
  int nb = 0;
  for (int base = 0; base < nleft; base += DOD_WAVE) {
    const int i = base + lane;
    const int j = i < nleft ? lo[i] : 0;
    nb = trk_push(i < nleft && slot_of[j] < 0 && a.scores[r0 + j] >= a.p.new_thresh, j, hi, nb);
  }
  __syncthreads();
  const int next = tab.next_id[s];
  const int born = nb < n ? nb : n;
  for (int i = lane; i < born; i += DOD_WAVE) {
    const int t = rows[i], j = hi[i];
    double z[4];
    trk_measure(a.boxes + (r0 + j) * 4, z);
    trk_init(tab.mean + (t0 + t) * 8, tab.cov + (t0 + t) * 12, z);
    tab.id[t0 + t] = next + i;
    tab.label[t0 + t] = a.labels[r0 + j];
    tab.score[t0 + t] = a.scores[r0 + j];
    tab.last[t0 + t] = frame;
    tab.state[t0 + t] = frame == 1 ? TRK_TRACKED : TRK_TENTATIVE;
    if constexpr (APP) slot_of[j] = t + 2 * kTrkKind;
    else if (frame == 1) slot_of[j] = t;
  }
  __syncthreads();
  // the rows' ids and boxes
  for (int j = lane; j < K; j += DOD_WAVE) {
    int t = slot_of[j];
    if constexpr (APP) {
      a.assoc[r0 + j] = t;
      if (t >= 0) t = (t >= 2 * kTrkKind && frame != 1) ? -1 : t % kTrkKind;      // a later birth is TENTATIVE: the row keeps id -1
    }
    float* o = a.track_boxes + (r0 + j) * 4;
    if (t < 0) {
      a.ids[r0 + j] = -1;
      o[0] = o[1] = o[2] = o[3] = 0.0f;
    } else {
      double b[4];
      trk_xyxy(tab.mean + (t0 + t) * 8, b);
      a.ids[r0 + j] = tab.id[t0 + t];
      o[0] = (float)b[0]; o[1] = (float)b[1]; o[2] = (float)b[2]; o[3] = (float)b[3];
    }
  }
  if (lane == 0) {
    tab.frame[s] = frame;
    tab.next_id[s] = next + born;
    tab.overflow[s] = tab.overflow[s] + (nb - born);
  }
}

__global__ __launch_bounds__(DOD_WAVE) void track_reset_kernel(TrkTable tab, int T, const int* __restrict__ mask) {
  const size_t s = blockIdx.x;
  if (mask && mask[s] == 0) return;
  for (int t = threadIdx.x; t < T; t += DOD_WAVE) {
    const size_t k = s * T + t;
    for (int c = 0; c < 8; ++c) tab.mean[k * 8 + c] = 0.0;
    for (int c = 0; c < 12; ++c) tab.cov[k * 12 + c] = 0.0;
    tab.state[k] = TRK_FREE; tab.id[k] = 0; tab.label[k] = 0; tab.last[k] = 0; tab.score[k] = 0.0f;
  }
  if (threadIdx.x == 0) { tab.frame[s] = 0; tab.next_id[s] = 1; tab.overflow[s] = 0; }
}

// dod_track_embed_commit: one wave per row (s, j).  Kind 2 stores the row's embedding in its slot; kind 1 blends it into the slot's,
// x = m E + (1 - m) e per element in double, and writes x / |x| (zeros when |x| is 0); kind 0 and -1 leave the table alone.  The rows of a
// frame name distinct slots, and a lane writes only the elements it read itself: plain stores, no atomics.
__global__ __launch_bounds__(DOD_WAVE) void track_embed_commit_kernel(float* __restrict__ slot_emb, const float* __restrict__ emb,
                                                                      const int* __restrict__ assoc, int T, int K, int D, float momentum) {
  const size_t s = blockIdx.y, j = blockIdx.x;
  const int lane = threadIdx.x;
  const int v = assoc[s * K + j];
  if (v < 0) return;
  const int kind = v / kTrkKind, t = v % kTrkKind;
  if (kind < 1 || kind > 2 || t >= T) return;
  float* E = slot_emb + (s * T + t) * D;
  const float* e = emb + (s * K + j) * D;
  if (kind == 2) {
    for (int c = lane; c < D; c += DOD_WAVE) E[c] = e[c];
    return;
  }
  const double m = (double)momentum, m1 = 1.0 - m;
  double ss = 0.0;
  for (int c = lane; c < D; c += DOD_WAVE) {
    const double x = m * (double)E[c] + m1 * (double)e[c];
    ss = ss + x * x;
  }
  for (int off = DOD_WAVE / 2; off > 0; off >>= 1) ss = ss + __shfl_xor(ss, off, DOD_WAVE);
  const double nrm = sqrt(ss);
  for (int c = lane; c < D; c += DOD_WAVE) {
    const double x = m * (double)E[c] + m1 * (double)e[c];
    E[c] = ss > 0.0 ? (float)(x / nrm) : 0.0f;
  }
}

constexpr int kTrkMaxD = 2048;
bool trk_shape_ok(int S, int T) { return S >= 1 && S <= kTrkMaxS && T >= 1 && T <= kTrkMaxT; }
bool trk_rows_ok(int K) { return K >= 1 && K <= kTrkMaxK; }

}  // namespace

extern "C" size_t dod_track_state_bytes(int S, int T) {
  if (!trk_shape_ok(S, T)) return 0;
  return trk_carve(nullptr, S, T, nullptr);
}

extern "C" size_t dod_track_workspace_bytes(int S, int T, int K) {
  if (!trk_shape_ok(S, T) || !trk_rows_ok(K)) return 0;
  return (size_t)S * (trk_up((size_t)T * K * sizeof(float)) + trk_up((size_t)(T + K) * kUnitBytes));
}

extern "C" int dod_track_reset(void* state, int S, int T, const int32_t* stream_mask, void* stream) {
  if (!state || ((uintptr_t)state & 7) != 0 || !trk_shape_ok(S, T)) return dod_fail(DOD_ERR_INVALID, "dod_track_reset: null or misaligned state, or S / T outside the limits");
  TrkTable tab;
  trk_carve((unsigned char*)state, S, T, &tab);
  hipLaunchKernelGGL(track_reset_kernel, dim3((unsigned)S), dim3(DOD_WAVE), 0, (hipStream_t)stream, tab, T, (const int*)stream_mask);
  return dod_launched("dod_track_reset");
}

// the argument check dod_track_update and dod_track_update_app share (who: the entry point, for the message), and the arguments both kernels take
static int trk_update_args(const char* who, void* state, int S, int T, const float* scores, const int32_t* labels, const float* boxes, const int32_t* counts, int K,
                           const dod_track_params* params, int32_t* ids, float* track_boxes, void* workspace, size_t workspace_bytes, TrkArgs& a) {
  if (!state || ((uintptr_t)state & 7) != 0 || !scores || !labels || !boxes || !counts || !params || !ids || !track_boxes)
    return dod_fail(DOD_ERR_INVALID, "%s: null argument or misaligned state", who);
  if (!trk_shape_ok(S, T) || !trk_rows_ok(K)) return dod_fail(DOD_ERR_INVALID, "%s: S=%d T=%d K=%d outside the limits", who, S, T, K);
  const dod_track_params& p = *params;
  const float th[6] = {p.track_thresh, p.low_thresh, p.new_thresh, p.match_thresh, p.second_thresh, p.tentative_thresh};
  for (float v : th)
    if (v != v) return dod_fail(DOD_ERR_INVALID, "%s: a NaN threshold", who);
  if (p.max_age < 0 || !(p.low_thresh <= p.track_thresh)) return dod_fail(DOD_ERR_INVALID, "%s: negative max_age, or low_thresh above track_thresh", who);
  if (!workspace || ((uintptr_t)workspace & 7) != 0 || workspace_bytes < dod_track_workspace_bytes(S, T, K))
    return dod_fail(DOD_ERR_INVALID, "%s: null, misaligned or short workspace", who);
  trk_carve((unsigned char*)state, S, T, &a.tab);
  a.T = T; a.K = K;
  a.scores = scores; a.labels = (const int*)labels; a.boxes = boxes; a.counts = (const int*)counts;
  a.p = p;
  a.ids = (int*)ids; a.track_boxes = track_boxes;
  a.workspace = (unsigned char*)workspace;
  a.cost_bytes = trk_up((size_t)T * K * sizeof(float));
  a.stream_bytes = a.cost_bytes + trk_up((size_t)(T + K) * kUnitBytes);
  return DOD_OK;
}

extern "C" int dod_track_update(void* state, int S, int T, const float* scores, const int32_t* labels, const float* boxes, const int32_t* counts,
                                int K, const dod_track_params* params, int32_t* ids, float* track_boxes, void* workspace, size_t workspace_bytes,
                                void* stream) {
  TrkArgs a;
  if (const int rc = trk_update_args("dod_track_update", state, S, T, scores, labels, boxes, counts, K, params, ids, track_boxes, workspace, workspace_bytes, a)) return rc;
  hipLaunchKernelGGL(track_update_kernel<false>, dim3((unsigned)S), dim3(DOD_WAVE), 0, (hipStream_t)stream, a);
  return dod_launched("dod_track_update");
}

static bool trk_app_params_ok(const dod_track_app_params* q) {
  return q && q->appearance_thresh == q->appearance_thresh && q->proximity_thresh == q->proximity_thresh && q->momentum >= 0.0f && q->momentum <= 1.0f;
}
static bool trk_embed_ok(int D) { return D >= 4 && D <= kTrkMaxD && D % 4 == 0; }

extern "C" int dod_track_update_app(void* state, int S, int T, const float* scores, const int32_t* labels, const float* boxes, const int32_t* counts,
                                    int K, const dod_track_params* params, const dod_track_app_params* app_params, const float* dots, int32_t* ids,
                                    float* track_boxes, int32_t* assoc, void* workspace, size_t workspace_bytes, void* stream) {
  TrkAppArgs a;
  if (!trk_app_params_ok(app_params) || !dots || !assoc) return dod_fail(DOD_ERR_INVALID, "dod_track_update_app: null dots / assoc, or app_params null or out of range");
  if (const int rc = trk_update_args("dod_track_update_app", state, S, T, scores, labels, boxes, counts, K, params, ids, track_boxes, workspace, workspace_bytes, a)) return rc;
  a.dots = dots; a.assoc = (int*)assoc;
  a.app_thresh = app_params->appearance_thresh; a.prox_thresh = app_params->proximity_thresh;
  hipLaunchKernelGGL(track_update_kernel<true>, dim3((unsigned)S), dim3(DOD_WAVE), 0, (hipStream_t)stream, a);
  return dod_launched("dod_track_update_app");
}

extern "C" int dod_track_embed_dots(const float* slot_emb, const float* emb, int S, int T, int K, int D, float* dots, void* stream) {
  if (!slot_emb || !emb || !dots || !trk_shape_ok(S, T) || !trk_rows_ok(K) || !trk_embed_ok(D))
    return dod_fail(DOD_ERR_INVALID, "dod_track_embed_dots: null argument, or S / T / K / D outside the limits");
  GemmF32X g = {};
  g.A = slot_emb; g.lda = D; g.a_sb = (long long)T * D;
  g.W = emb; g.ldw = D; g.w_sb = (long long)K * D;
  g.C = dots; g.ldc = K; g.c_sb = (long long)T * K;
  g.M = T; g.N = K; g.K = D; g.batch = S; g.hb = 1; g.alpha = 1.0f; g.ksplit = 1;
  const int rc = launch_gemm_f32x(g, (hipStream_t)stream);
  return rc == 0 ? DOD_OK : dod_fail(rc == 3 ? DOD_ERR_HIP : DOD_ERR_INVALID, "dod_track_embed_dots: launch_gemm_f32x rejected (rc %d)", rc);
}

extern "C" int dod_track_embed_commit(float* slot_emb, const float* emb, const int32_t* assoc, int S, int T, int K, int D, float momentum, void* stream) {
  if (!slot_emb || !emb || !assoc || !trk_shape_ok(S, T) || !trk_rows_ok(K) || !trk_embed_ok(D))
    return dod_fail(DOD_ERR_INVALID, "dod_track_embed_commit: null argument, or S / T / K / D outside the limits");
  if (!(momentum >= 0.0f && momentum <= 1.0f)) return dod_fail(DOD_ERR_INVALID, "dod_track_embed_commit: momentum %g outside [0, 1]", momentum);
  hipLaunchKernelGGL(track_embed_commit_kernel, dim3((unsigned)K, (unsigned)S), dim3(DOD_WAVE), 0, (hipStream_t)stream, slot_emb, emb, (const int*)assoc, T, K, D,
                     momentum);
  return dod_launched("dod_track_embed_commit");
}

extern "C" int dod_track_export(const void* state, int S, int T, double* mean, double* cov, int32_t* slot_state, int32_t* id, int32_t* label,
                                int32_t* last_frame, float* score, int32_t* frame, int32_t* next_id, int32_t* overflow, void* stream) {
  if (!state || ((uintptr_t)state & 7) != 0 || !trk_shape_ok(S, T)) return dod_fail(DOD_ERR_INVALID, "dod_track_export: null or misaligned state, or S / T outside the limits");
  if (!mean || !cov || !slot_state || !id || !label || !last_frame || !score || !frame || !next_id || !overflow) return dod_fail(DOD_ERR_INVALID, "dod_track_export: null output");
  TrkTable tab;
  trk_carve((unsigned char*)const_cast<void*>(state), S, T, &tab);
  const size_t n = (size_t)S * T;
  hipStream_t st = (hipStream_t)stream;
  const struct { void* dst; const void* src; size_t bytes; } parts[10] = {
      {mean, tab.mean, n * 8 * sizeof(double)}, {cov, tab.cov, n * 12 * sizeof(double)}, {slot_state, tab.state, n * 4}, {id, tab.id, n * 4},
      {label, tab.label, n * 4}, {last_frame, tab.last, n * 4}, {score, tab.score, n * 4}, {frame, tab.frame, (size_t)S * 4},
      {next_id, tab.next_id, (size_t)S * 4}, {overflow, tab.overflow, (size_t)S * 4}};
  for (const auto& c : parts)
    if (hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) return dod_fail(DOD_ERR_HIP, "dod_track_export: hipMemcpyAsync failed");
  return DOD_OK;
}
