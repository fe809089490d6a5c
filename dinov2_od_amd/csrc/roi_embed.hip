// ROI embeddings from the backbone tokens (dod_roi_embed): one unit vector per box, pooled from the patch tokens the forward already left
// in HBM.  include/dinodet.h states the semantics; tests/roi_embed_cases.py restates them in numpy.
//
// The mean of grid x grid bilinear samples on a product grid is separable: p = sum_r sum_c wy[r] wx[c] f[r, c, :], and one sample touches at
// most two rows and two columns, so a box has at most 2 * grid non-zero weights per axis whatever the size of the map.  One workgroup per
// box: lane 0 builds the column taps and lane 1 the row taps (index + weight, in double, narrowed once) in LDS, one barrier, then the lanes
// run over the channels as float4 and walk the touched tokens in row-major order -- every token row read is one coalesced line of D floats,
// served from L2 when boxes of one image share tokens.  The norm is one workgroup reduction (in double: it adds nothing to the error of
// the quotient).  Every output element is written exactly once, nothing is atomic, and no token outside the gh * gw map of the row's own
// image is ever addressed; a token whose weight is zero is not read either.
#include "dod_common.h"
#include "../../include/dinodet.h"

#pragma clang fp contract(off)

namespace {

constexpr int kRoiThreads = 256, kRoiMaxGrid = 8, kRoiTaps = 2 * kRoiMaxGrid, kRoiMaxD = 2048, kRoiMaxK = 1024;
constexpr int kRoiVec = kRoiMaxD / 4 / kRoiThreads;      // float4 accumulators per lane
static_assert(kRoiVec * kRoiThreads * 4 == kRoiMaxD, "the lanes' accumulators cover the widest row");

struct RoiArgs {
  const float* feat; int N, D, first, gh, gw;
  const float* boxes; const int* counts; const float* sizes;
  int K, grid;
  float* emb;
};

__device__ __forceinline__ bool roi_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ double roi_clip(double x, double hi) {
  x = x < 0.0 ? 0.0 : x;
  return x > hi ? hi : x;
}

// The taps of one axis of n tokens for the samples of [a1, a2]: indices ascending, weights summed in sample order (lower neighbour, then
// upper) and divided by grid once.  Called by one lane.  Returns the number of taps (<= 2 * grid).
__device__ int roi_axis(double a1, double a2, int n, int grid, int* idx, double* wd, float* wf) {
  int cnt = 0;
  const double step = (a2 - a1) / (double)grid;
  for (int i = 0; i < grid; ++i) {
    const double x = roi_clip((a1 + ((double)i + 0.5) * step) - 0.5, (double)(n - 1));
    const int c0 = (int)x;
    const int c1 = c0 + 1 < n ? c0 + 1 : n - 1;
    const double f = x - (double)c0;
    const int c[2] = {c0, c1};
    const double w[2] = {1.0 - f, f};
    for (int h = 0; h < 2; ++h) {
      int at = 0;
      while (at < cnt && idx[at] != c[h]) ++at;
      if (at == cnt) { idx[cnt] = c[h]; wd[cnt] = 0.0; ++cnt; }      // the samples ascend, so a new index is the largest so far
      wd[at] = wd[at] + w[h];
    }
  }
  for (int t = 0; t < cnt; ++t) wf[t] = (float)(wd[t] / (double)grid);
  return cnt;
}

__global__ __launch_bounds__(kRoiThreads) void roi_embed_kernel(RoiArgs a) {
  __shared__ int tap_i[2][kRoiTaps], tap_n[2];
  __shared__ float tap_w[2][kRoiTaps];
  __shared__ double tap_d[2][kRoiTaps], red[kRoiThreads / DOD_WAVE];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.K, k = blockIdx.x % a.K;
  const int D4 = a.D >> 2;
  float4* out = reinterpret_cast<float4*>(a.emb + (size_t)blockIdx.x * a.D);
  // the row's validity and its box on the token map: uniform over the workgroup
  int cnt = a.counts ? a.counts[b] : a.K;
  cnt = cnt < 0 ? 0 : (cnt > a.K ? a.K : cnt);
  bool valid = k < cnt;
  double u1 = 0.0, v1 = 0.0, u2 = 0.0, v2 = 0.0;
  if (valid) {
    const float* bx = a.boxes + (size_t)blockIdx.x * 4;
    const float x1 = bx[0], y1 = bx[1], x2 = bx[2], y2 = bx[3];
    valid = roi_finite(x1) && roi_finite(y1) && roi_finite(x2) && roi_finite(y2) && x2 > x1 && y2 > y1;
    if (valid) {
      const double hh = a.sizes ? (double)a.sizes[2 * b] : 1.0, ww = a.sizes ? (double)a.sizes[2 * b + 1] : 1.0;
      u1 = roi_clip(((double)x1 * (double)a.gw) / ww, (double)a.gw);
      u2 = roi_clip(((double)x2 * (double)a.gw) / ww, (double)a.gw);
      v1 = roi_clip(((double)y1 * (double)a.gh) / hh, (double)a.gh);
      v2 = roi_clip(((double)y2 * (double)a.gh) / hh, (double)a.gh);
      valid = u2 > u1 && v2 > v1;                       // empty after clipping, or a size that is not a positive number
    }
  }
  if (!valid) {
    for (int c4 = tid; c4 < D4; c4 += kRoiThreads) out[c4] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  if (tid == 0) tap_n[0] = roi_axis(u1, u2, a.gw, a.grid, tap_i[0], tap_d[0], tap_w[0]);
  if (tid == 1) tap_n[1] = roi_axis(v1, v2, a.gh, a.grid, tap_i[1], tap_d[1], tap_w[1]);
  __syncthreads();
  const int nx = tap_n[0], ny = tap_n[1];
  const float* base = a.feat + ((size_t)b * a.N + a.first) * a.D;
  float4 acc[kRoiVec];
#pragma unroll
  for (int q = 0; q < kRoiVec; ++q) acc[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (int j = 0; j < ny; ++j) {
    const float wyj = tap_w[1][j];
    const size_t row = (size_t)tap_i[1][j] * a.gw;
    for (int i = 0; i < nx; ++i) {
      const float w = wyj * tap_w[0][i];
      if (w == 0.0f) continue;
      const float4* src = reinterpret_cast<const float4*>(base + (row + tap_i[0][i]) * a.D);
#pragma unroll
      for (int q = 0; q < kRoiVec; ++q) {
        const int c4 = tid + q * kRoiThreads;
        if (c4 < D4) {
          const float4 f = src[c4];
          acc[q].x = fmaf(w, f.x, acc[q].x); acc[q].y = fmaf(w, f.y, acc[q].y);
          acc[q].z = fmaf(w, f.z, acc[q].z); acc[q].w = fmaf(w, f.w, acc[q].w);
        }
      }
    }
  }
  double ss = 0.0;
#pragma unroll
  for (int q = 0; q < kRoiVec; ++q) {
    if (tid + q * kRoiThreads < D4) {
      const double x = acc[q].x, y = acc[q].y, z = acc[q].z, w = acc[q].w;
      ss = (((ss + x * x) + y * y) + z * z) + w * w;
    }
  }
  for (int off = DOD_WAVE / 2; off > 0; off >>= 1) ss = ss + __shfl_down(ss, off, DOD_WAVE);
  if ((tid & (DOD_WAVE - 1)) == 0) red[tid / DOD_WAVE] = ss;
  __syncthreads();
  double tot = 0.0;
  for (int w = 0; w < kRoiThreads / DOD_WAVE; ++w) tot = tot + red[w];
  const double nrm = sqrt(tot);
#pragma unroll
  for (int q = 0; q < kRoiVec; ++q) {
    const int c4 = tid + q * kRoiThreads;
    if (c4 < D4) {
      float4 e = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (tot > 0.0) {
        e.x = (float)((double)acc[q].x / nrm); e.y = (float)((double)acc[q].y / nrm);
        e.z = (float)((double)acc[q].z / nrm); e.w = (float)((double)acc[q].w / nrm);
      }
      out[c4] = e;
    }
  }
}

}  // namespace

extern "C" int dod_roi_embed(const float* features, int B, int N, int D, int first_token, int gh, int gw, const float* boxes, const int32_t* counts,
                             const float* sizes, int K, int grid, float* emb, void* stream) {
  if (!features || !boxes || !emb || ((uintptr_t)features & 15) != 0 || ((uintptr_t)emb & 15) != 0) return dod_fail(DOD_ERR_INVALID, "dod_roi_embed: null features / boxes / emb, or features / emb not 16-byte aligned");
  if (B < 1 || K < 1 || K > kRoiMaxK || (long long)B * K > 0x7fffffffLL) return dod_fail(DOD_ERR_INVALID, "dod_roi_embed: B=%d K=%d outside the limits", B, K);
  if (D < 4 || D > kRoiMaxD || D % 4 != 0 || grid < 1 || grid > kRoiMaxGrid) return dod_fail(DOD_ERR_INVALID, "dod_roi_embed: D=%d or grid=%d outside the limits, or D no multiple of 4", D, grid);
  if (gh < 1 || gw < 1 || first_token < 0 || N < 1 || (long long)first_token + (long long)gh * gw > (long long)N) return dod_fail(DOD_ERR_INVALID, "dod_roi_embed: gh=%d gw=%d first_token=%d do not fit the N=%d tokens", gh, gw, first_token, N);
  RoiArgs a;
  a.feat = features; a.N = N; a.D = D; a.first = first_token; a.gh = gh; a.gw = gw;
  a.boxes = boxes; a.counts = (const int*)counts; a.sizes = sizes;
  a.K = K; a.grid = grid; a.emb = emb;
  hipLaunchKernelGGL(roi_embed_kernel, dim3((unsigned)(B * K)), dim3(kRoiThreads), 0, (hipStream_t)stream, a);
  return dod_launched("dod_roi_embed");
}
