// Geometric warp on device (dod_preprocess_warp): random affine (rotation, scale, shear, translation) and perspective as ONE
// inverse-map gather, Pillow-exact:
//   Image.transform((out_w, out_h), PERSPECTIVE, coeffs, BILINEAR, fillcolor=fill)  ->  ToTensor (or the uint8 HWC bytes)
// (AFFINE is the same arithmetic with a6 = a7 = 0: the denominator is exactly 1.0 and dividing by it changes no bit, so the
// division is skipped.)  The arithmetic is Pillow's src/libImaging/Geometry.c (third-party, restated -- see tests/warp_cases.py):
// perspective_transform on the pixel centre, then bilinear_filter32RGB, everything in DOUBLE with one rounding per operation.  The
// whole file is compiled without FMA contraction: a fused  a + (b - a) * dx  rounds once where the C code rounds twice, and the
// truncation to a byte makes that visible (tests/warp_cases.py fma_probe).
//
// A warp is a gather, not a separable resample: it cannot ride in the two resize passes and is a kernel of its own, one launch, no
// atomics, every output element written exactly once (fill included).  Workgroup = a WP_TX x WP_TY = 32 x 8 tile of output pixels of
// one image, one pixel per thread, lanes along x: a wave owns 32 x 2 pixels, so its planar fp32 stores are two full 128-byte lines per
// channel and its HWC byte stores two 96-byte runs, while under a rotation the tile's footprint in the source stays a compact patch of
// about 32 x 8 pixels (a 256 x 1 strip would walk diagonally through 256 sin(angle) source rows).  The coordinate arithmetic is about
// 45 fp64 operations per pixel against 15 (fp32) or 6 (uint8) bytes of traffic: DESIGN.md section 6b has the budget.
#include "dod_common.h"
#include "../../include/dinodet.h"

#pragma clang fp contract(off)

#define WP_TX 32
#define WP_TY 8

// a + (b - a) * d on bytes a, b: the difference is an int (exact), product and sum round separately
__device__ __forceinline__ double wp_lerp_u8(int a, int b, double d) {
#pragma clang fp contract(off)
  const double t = (double)(b - a) * d;
  return (double)a + t;
}

template <bool U8>
__global__ __launch_bounds__(WP_TX * WP_TY) void wp_warp_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ src_offs,
                                                                const int* __restrict__ hs, const int* __restrict__ ws,
                                                                const double* __restrict__ coeffs, const unsigned char* __restrict__ fills,
                                                                int fill_per_image, int out_h, int out_w, float* __restrict__ out,
                                                                unsigned char* __restrict__ out_u8) {
#pragma clang fp contract(off)
  const int b = blockIdx.z;
  const int x = blockIdx.x * WP_TX + (threadIdx.x & (WP_TX - 1));
  const int y = blockIdx.y * WP_TY + (threadIdx.x / WP_TX);
  if (x >= out_w || y >= out_h) return;
  const int H = hs[b], W = ws[b];
  const double* a = coeffs + (size_t)b * 8;
  const double a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5], a6 = a[6], a7 = a[7];
  const unsigned char* fill = fills + (fill_per_image ? 3 * b : 0);
  int v0 = fill[0], v1 = fill[1], v2 = fill[2];

  const double xin = (double)x + 0.5, yin = (double)y + 0.5;
  double sx = a0 * xin + a1 * yin + a2;
  double sy = a3 * xin + a4 * yin + a5;
  if (a6 != 0.0 || a7 != 0.0) {
    const double den = a6 * xin + a7 * yin + 1.0;
    sx = sx / den;
    sy = sy / den;
  }
  // written as the test for INSIDE, so that a NaN coordinate takes the fill; only then are the coordinates converted to integers
  if (H >= 1 && W >= 1 && sx >= 0.0 && sx < (double)W && sy >= 0.0 && sy < (double)H) {
    sx -= 0.5;
    sy -= 0.5;
    const double fx = floor(sx), fy = floor(sy);
    const int ix = (int)fx, iy = (int)fy;            // -1 .. W - 1, -1 .. H - 1
    const double dx = sx - fx, dy = sy - fy;
    const int x0 = ix < 0 ? 0 : ix;                  // ix <= W - 1
    const int x1 = ix + 1 > W - 1 ? W - 1 : ix + 1;  // ix + 1 >= 0
    const int r0 = iy < 0 ? 0 : iy;
    const bool two = iy + 1 < H;                     // iy + 1 >= 0 always
    const unsigned char* img = src + src_offs[b];
    const unsigned char* p0 = img + (size_t)r0 * W * 3;
    const unsigned char* p1 = img + (size_t)(two ? iy + 1 : r0) * W * 3;
    const unsigned char *p00 = p0 + 3 * x0, *p01 = p0 + 3 * x1, *p10 = p1 + 3 * x0, *p11 = p1 + 3 * x1;
    int v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double t1 = wp_lerp_u8(p00[c], p01[c], dx);
      const double t2 = two ? wp_lerp_u8(p10[c], p11[c], dx) : t1;
      const double d = (t2 - t1) * dy;
      v[c] = (int)(t1 + d);                          // within [0, 255]: truncation, as the (UINT8) cast
    }
    v0 = v[0]; v1 = v[1]; v2 = v[2];
  }
  if (U8) {
    unsigned char* o = out_u8 + (((size_t)b * out_h + y) * out_w + x) * 3;
    o[0] = (unsigned char)v0; o[1] = (unsigned char)v1; o[2] = (unsigned char)v2;
  } else {
    const size_t plane = (size_t)out_h * out_w;
    float* o = out + (size_t)b * 3 * plane + (size_t)y * out_w + x;
    o[0] = (float)v0 / 255.0f; o[plane] = (float)v1 / 255.0f; o[2 * plane] = (float)v2 / 255.0f;
  }
}

static int preprocess_warp_impl(const char* who, const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int B,
                                const double* coeffs, const uint8_t* fills, int fill_per_image, int out_h, int out_w, float* out,
                                uint8_t* out_u8, void* stream) {
  if (!src || !src_offs || !heights || !widths || !coeffs || !fills || (!out && !out_u8)) return dod_fail(DOD_ERR_INVALID, "%s: null argument", who);
  if (B <= 0 || B > 65535 || out_h <= 0 || out_w <= 0) return dod_fail(DOD_ERR_INVALID, "%s: B=%d out_h=%d out_w=%d outside the limits", who, B, out_h, out_w);
  const dim3 grid((out_w + WP_TX - 1) / WP_TX, (out_h + WP_TY - 1) / WP_TY, B);
  if (grid.y > 65535) return dod_fail(DOD_ERR_INVALID, "%s: out_h = %d past one launch", who, out_h);      // more than 524 280 output rows: past one launch
  hipStream_t s = (hipStream_t)stream;
  if (out_u8)
    hipLaunchKernelGGL(wp_warp_kernel<true>, grid, dim3(WP_TX * WP_TY), 0, s, (const unsigned char*)src, (const long long*)src_offs, heights,
                       widths, coeffs, (const unsigned char*)fills, fill_per_image, out_h, out_w, (float*)nullptr, (unsigned char*)out_u8);
  else
    hipLaunchKernelGGL(wp_warp_kernel<false>, grid, dim3(WP_TX * WP_TY), 0, s, (const unsigned char*)src, (const long long*)src_offs, heights,
                       widths, coeffs, (const unsigned char*)fills, fill_per_image, out_h, out_w, out, (unsigned char*)nullptr);
  return dod_launched(who);
}

extern "C" int dod_preprocess_warp(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int B,
                                   const double* coeffs, const uint8_t* fills, int fill_per_image, int out_h, int out_w, float* out,
                                   void* stream) {
  return preprocess_warp_impl("dod_preprocess_warp", src, src_offs, heights, widths, B, coeffs, fills, fill_per_image, out_h, out_w, out, nullptr, stream);
}
extern "C" int dod_preprocess_warp_u8(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int B,
                                      const double* coeffs, const uint8_t* fills, int fill_per_image, int out_h, int out_w,
                                      uint8_t* out_hwc, void* stream) {
  return preprocess_warp_impl("dod_preprocess_warp_u8", src, src_offs, heights, widths, B, coeffs, fills, fill_per_image, out_h, out_w, nullptr, out_hwc, stream);
}
