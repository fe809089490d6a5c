// Input pipeline on device: the reference's transform (dino_detector/train.py:584-587),
// torchvision Resize((R, R)) + ToTensor() on a PIL image, for a ragged batch of uint8 HWC RGB images:
//   Image.resize((R, R), BILINEAR)  ->  uint8 [R, R, 3]  ->  float32 CHW / 255.
// The arithmetic is Pillow's (src/libImaging/Resample.c; third-party, restated -- see oracle/preprocess_oracle.py): per output
// index a window [xmin, xmin + n) with bilinear weights computed in DOUBLE (support = max(scale, 1): the filter widens when
// downscaling), normalised, converted to int32 fixed point (22 bits, round half away from zero); a horizontal pass into a
// uint8 image (accumulator seeded with 1 << 21, >> 22, clipped), then a vertical pass on that uint8 image.  Integer / byte
// work, bit-exact: the double-precision weight arithmetic is compiled without FMA contraction so it rounds like the C code.
// (Pillow skips a pass whose size does not change; that pass is the identity here too -- weights (1 << 22, 0) -- so both
//  passes always run.)  HBM-bound byte work: each source byte is read once per pass (windows overlap in L2), lanes run along
// the contiguous output bytes.
#include "dod_common.h"
#include "../../include/dinodet.h"

#define PP_BITS 22
#define PP_MAXK 32          // window taps: ceil(max(scale, 1)) * 2 + 1 <= 32  (down-scaling up to 15x)

// window and fixed-point weights of output index xx (Resample.c precompute_coeffs + normalize_coeffs_8bpc)
__device__ void pil_coeffs(int in_size, int out_size, int xx, int* lo, int* n, int* kk) {
#pragma clang fp contract(off)
  const double scale = (double)in_size / (double)out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  const double center = 0.0 + ((double)xx + 0.5) * scale;
  const double ss = 1.0 / filterscale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  if (xmax > PP_MAXK) xmax = PP_MAXK;          // unreachable: the host wrapper bounds the scale
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) {
    double t = ((double)(x + xmin) - center + 0.5) * ss;
    if (t < 0.0) t = -t;
    ww += t < 1.0 ? 1.0 - t : 0.0;
  }
  for (int x = 0; x < xmax; ++x) {
    double t = ((double)(x + xmin) - center + 0.5) * ss;
    if (t < 0.0) t = -t;
    double w = t < 1.0 ? 1.0 - t : 0.0;
    if (ww != 0.0) w /= ww;
    const double v = w * (double)(1 << PP_BITS);
    kk[x] = w < 0.0 ? (int)(-0.5 + v) : (int)(0.5 + v);
  }
  *lo = xmin;
  *n = xmax;
}

__device__ __forceinline__ unsigned char pp_clip8(int acc) {
  const int v = acc >> PP_BITS;
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// horizontal pass: tmp[b][y][ox][c].  Block = 256 output columns x PP_ROWS source rows of one image.
#define PP_ROWS 16
__global__ __launch_bounds__(256) void pp_horizontal_kernel(const unsigned char* __restrict__ src,
                                                            const long long* __restrict__ src_offs,
                                                            const int* __restrict__ hs, const int* __restrict__ ws, int out_w,
                                                            unsigned char* __restrict__ tmp,
                                                            const long long* __restrict__ tmp_offs) {
  __shared__ int kk[256][PP_MAXK + 1];      // +1: odd pitch, conflict-free per-thread rows
  const int b = blockIdx.z;
  const int H = hs[b], W = ws[b];
  const int y0 = blockIdx.y * PP_ROWS;
  if (y0 >= H) return;
  const int ox = blockIdx.x * 256 + threadIdx.x;
  if (ox >= out_w) return;
  int lo, n;
  pil_coeffs(W, out_w, ox, &lo, &n, kk[threadIdx.x]);
  const unsigned char* img = src + src_offs[b];
  unsigned char* dst = tmp + tmp_offs[b];
  const int y1 = y0 + PP_ROWS < H ? y0 + PP_ROWS : H;
  for (int y = y0; y < y1; ++y) {
    const unsigned char* row = img + ((size_t)y * W + lo) * 3;
    int a0 = 1 << (PP_BITS - 1), a1 = a0, a2 = a0;
    for (int x = 0; x < n; ++x) {
      const int k = kk[threadIdx.x][x];
      a0 += (int)row[3 * x] * k; a1 += (int)row[3 * x + 1] * k; a2 += (int)row[3 * x + 2] * k;
    }
    unsigned char* o = dst + ((size_t)y * out_w + ox) * 3;
    o[0] = pp_clip8(a0); o[1] = pp_clip8(a1); o[2] = pp_clip8(a2);
  }
}

// vertical pass + ToTensor: out[b][c][oy][ox] = clip8(...) / 255.  Block = one output row; threads along its 3*out_w bytes.
// Image b's source height is hs[b * HS]: HS = 1 for the plain heights, 4 for the height column of the crop boxes.
template <int HS>
__global__ __launch_bounds__(256) void pp_vertical_kernel(const unsigned char* __restrict__ tmp,
                                                          const long long* __restrict__ tmp_offs,
                                                          const int* __restrict__ hs, int out_h, int out_w,
                                                          float* __restrict__ out, unsigned char* __restrict__ out_u8) {
  __shared__ int kk[PP_MAXK];
  __shared__ int s_lo, s_n;
  const int b = blockIdx.y, oy = blockIdx.x;
  const int H = hs[b * HS];
  if (threadIdx.x == 0) {
    int lo, n;
    pil_coeffs(H, out_h, oy, &lo, &n, kk);
    s_lo = lo; s_n = n;
  }
  __syncthreads();
  const int lo = s_lo, n = s_n;
  const unsigned char* img = tmp + tmp_offs[b];
  const int rowbytes = out_w * 3;
  for (int t = threadIdx.x; t < rowbytes; t += 256) {
    int acc = 1 << (PP_BITS - 1);
    for (int y = 0; y < n; ++y) acc += (int)img[(size_t)(lo + y) * rowbytes + t] * kk[y];
    const int ox = t / 3, c = t - ox * 3;
    if (out_u8) out_u8[((size_t)b * out_h + oy) * rowbytes + t] = pp_clip8(acc);      // resampled bytes, HWC: the fused patch embed divides by 255
    else out[(((size_t)b * 3 + c) * out_h + oy) * out_w + ox] = (float)pp_clip8(acc) / 255.0f;
  }
}

static int preprocess_impl(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int B,
                           int max_h, int max_w, int out_h, int out_w, uint8_t* tmp, const int64_t* tmp_offs, float* out, uint8_t* out_u8,
                           void* stream) {
  if (!src || !src_offs || !heights || !widths || !tmp || !tmp_offs || (!out && !out_u8)) return DOD_ERR_INVALID;
  if (B <= 0 || out_h <= 0 || out_w <= 0 || max_h <= 0 || max_w <= 0 || B > 65535) return DOD_ERR_INVALID;
  // window taps ceil(max(scale, 1)) * 2 + 1 must fit PP_MAXK
  const int kh = ((max_w + out_w - 1) / out_w) * 2 + 1, kv = ((max_h + out_h - 1) / out_h) * 2 + 1;
  if (kh > PP_MAXK || kv > PP_MAXK) return DOD_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pp_horizontal_kernel, dim3((out_w + 255) / 256, (max_h + PP_ROWS - 1) / PP_ROWS, B), dim3(256), 0, s,
                     (const unsigned char*)src, (const long long*)src_offs, heights, widths, out_w, (unsigned char*)tmp,
                     (const long long*)tmp_offs);
  hipLaunchKernelGGL(pp_vertical_kernel<1>, dim3(out_h, B), dim3(256), 0, s, (const unsigned char*)tmp, (const long long*)tmp_offs,
                     heights, out_h, out_w, out, (unsigned char*)out_u8);
  return hipGetLastError() == hipSuccess ? DOD_OK : DOD_ERR_HIP;
}

extern "C" int dod_preprocess(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int B,
                              int max_h, int max_w, int out_h, int out_w, uint8_t* tmp, const int64_t* tmp_offs, float* out,
                              void* stream) {
  return preprocess_impl(src, src_offs, heights, widths, B, max_h, max_w, out_h, out_w, tmp, tmp_offs, out, nullptr, stream);
}
extern "C" int dod_preprocess_u8(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int B,
                                 int max_h, int max_w, int out_h, int out_w, uint8_t* tmp, const int64_t* tmp_offs, uint8_t* out_hwc,
                                 void* stream) {
  return preprocess_impl(src, src_offs, heights, widths, B, max_h, max_w, out_h, out_w, tmp, tmp_offs, nullptr, out_hwc, stream);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Train-time augmentation in the same two passes (dod_preprocess_aug): per image a crop box (left, top, width, height), a
// colour jitter on the cropped source pixels, the resize above with in_size = the crop's width / height, and a horizontal flip
// of the resized image.  The semantics are Pillow's, in this order:
//   img.crop(box) -> ImageEnhance.Brightness -> .Contrast -> .Color -> resize(BILINEAR) -> transpose(FLIP_LEFT_RIGHT)
// Each enhancer is Image.blend(degenerate, img, f) (src/libImaging/Blend.c): per byte v = d + f * (p - d) in float, the product
// and the sum rounded separately; (uint8) truncation for 0 <= f <= 1, else clipped to [0, 255] first.  Degenerates: 0
// (brightness); the rounded mean m of the crop's luma after the brightness step, one integer per image (contrast); the pixel's
// own luma after both (saturation).  The mean comes from a reduction over the crop that runs first (integer sums: exact,
// order-independent, one 64-bit atomic per workgroup).  The jittered crop of every image that has a factor != 1 is then written
// once, behind that image's horizontal-pass rows in tmp, and the horizontal pass reads it from there: every source pixel is
// jittered once, not once per filter tap (2.4 - 3.6 taps per source pixel at 480x640 -> 224^2 / 518^2; measured 18 - 29 %
// faster than jittering in the tap loop).  Without jitter nothing of this runs and the horizontal pass
// reads the source image's crop directly.

// Image.convert("L") of one RGB pixel (src/libImaging/Convert.c, L24 >> 16)
__device__ __forceinline__ int pp_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Image.blend(d, p, f) on one byte; f >= 0 (the host wrapper checks)
__device__ __forceinline__ int pp_blend(int d, int p, float f) {
#pragma clang fp contract(off)
  const float t = f * (float)(p - d);
  const float v = (float)d + t;
  if (f <= 1.0f) return (int)v;
  return v <= 0.0f ? 0 : (v >= 255.0f ? 255 : (int)v);
}

// factors of one image (1.0 = skip the step); the contrast factor counts only when the luma sums exist
struct pp_jitter_t { float bf, cf, sf; };
__device__ __forceinline__ pp_jitter_t pp_factors(const float* jitter, const unsigned long long* lsum, int b) {
  pp_jitter_t j = {jitter[3 * b], lsum ? jitter[3 * b + 1] : 1.0f, jitter[3 * b + 2]};
  return j;
}
__device__ __forceinline__ bool pp_is_identity(const pp_jitter_t& j) { return j.bf == 1.0f && j.cf == 1.0f && j.sf == 1.0f; }

// a box that does not lie inside its image is never read (the host wrapper rejects it; a C caller's mistake must not fault)
__device__ __forceinline__ bool pp_box_ok(int H, int W, int l, int t, int cw, int ch) {
  return l >= 0 && t >= 0 && cw >= 1 && ch >= 1 && cw <= W - l && ch <= H - t;
}

// lsum[b] += sum of the luma of the crop's pixels after the brightness step, for every image whose contrast factor is not 1.
// Block = PP_SUM_ROWS rows of one crop, threads along its pixels.
#define PP_SUM_ROWS 8
__global__ __launch_bounds__(256) void pp_luma_sum_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ src_offs,
                                                          const int* __restrict__ hs, const int* __restrict__ ws,
                                                          const int* __restrict__ crops, const float* __restrict__ jitter,
                                                          unsigned long long* __restrict__ lsum) {
  __shared__ unsigned long long part[4];
  const int b = blockIdx.y;
  if (jitter[3 * b + 1] == 1.0f) return;            // the mean is not used
  const int W = ws[b], l = crops[4 * b], t = crops[4 * b + 1], cw = crops[4 * b + 2], ch = crops[4 * b + 3];
  if (!pp_box_ok(hs[b], W, l, t, cw, ch)) return;
  const int y0 = blockIdx.x * PP_SUM_ROWS;
  if (y0 >= ch) return;
  const int y1 = y0 + PP_SUM_ROWS < ch ? y0 + PP_SUM_ROWS : ch;
  const float bf = jitter[3 * b];
  const unsigned char* img = src + src_offs[b];
  unsigned long long acc = 0;
  for (int y = y0; y < y1; ++y) {
    const unsigned char* row = img + ((size_t)(t + y) * W + l) * 3;
    for (int x = threadIdx.x; x < cw; x += 256) {
      int r = row[3 * x], g = row[3 * x + 1], bl = row[3 * x + 2];
      if (bf != 1.0f) { r = pp_blend(0, r, bf); g = pp_blend(0, g, bf); bl = pp_blend(0, bl, bf); }
      acc += (unsigned long long)pp_luma(r, g, bl);
    }
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(&lsum[b], part[0] + part[1] + part[2] + part[3]);
}

// the jittered crop of image b, [ch][cw][3] bytes at tmp + tmp_offs[b] + ch * out_w * 3 (behind its horizontal-pass rows), for
// every image with a factor != 1.  Block = 256 crop columns x PP_SUM_ROWS crop rows, one pixel per thread and row.
__global__ __launch_bounds__(256) void pp_jitter_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ src_offs,
                                                        const int* __restrict__ hs, const int* __restrict__ ws,
                                                        const int* __restrict__ crops, const float* __restrict__ jitter,
                                                        const unsigned long long* __restrict__ lsum, int out_w,
                                                        unsigned char* __restrict__ tmp, const long long* __restrict__ tmp_offs) {
  const int b = blockIdx.z;
  const pp_jitter_t j = pp_factors(jitter, lsum, b);
  if (pp_is_identity(j)) return;                     // the horizontal pass reads the source
  const int W = ws[b], l = crops[4 * b], t = crops[4 * b + 1], cw = crops[4 * b + 2], ch = crops[4 * b + 3];
  if (!pp_box_ok(hs[b], W, l, t, cw, ch)) return;
  const int y0 = blockIdx.y * PP_SUM_ROWS;
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (y0 >= ch || x >= cw) return;
  int m = 0;
  if (j.cf != 1.0f) {
#pragma clang fp contract(off)
    m = (int)((double)lsum[b] / (double)((long long)cw * ch) + 0.5);      // ImageStat mean, rounded as ImageEnhance.Contrast does
  }
  const unsigned char* img = src + src_offs[b];
  unsigned char* dst = tmp + tmp_offs[b] + (size_t)ch * out_w * 3;
  const int y1 = y0 + PP_SUM_ROWS < ch ? y0 + PP_SUM_ROWS : ch;
  for (int y = y0; y < y1; ++y) {
    const unsigned char* p = img + ((size_t)(t + y) * W + l + x) * 3;
    int r = p[0], g = p[1], bl = p[2];
    if (j.bf != 1.0f) { r = pp_blend(0, r, j.bf); g = pp_blend(0, g, j.bf); bl = pp_blend(0, bl, j.bf); }
    if (j.cf != 1.0f) { r = pp_blend(m, r, j.cf); g = pp_blend(m, g, j.cf); bl = pp_blend(m, bl, j.cf); }
    if (j.sf != 1.0f) { const int lu = pp_luma(r, g, bl); r = pp_blend(lu, r, j.sf); g = pp_blend(lu, g, j.sf); bl = pp_blend(lu, bl, j.sf); }
    unsigned char* o = dst + ((size_t)y * cw + x) * 3;
    o[0] = (unsigned char)r; o[1] = (unsigned char)g; o[2] = (unsigned char)bl;
  }
}

// horizontal pass over the crop: tmp[b][y][ox'][c] for crop rows y, ox' = the flipped column when flips[b].  Block as in the plain
// kernel, and JIT = false is its loop on the crop's rows and columns; JIT = true reads the jittered crop where one was written.
// (tmp is read and written here, in disjoint parts: no __restrict__ on it.)
template <bool JIT>
__global__ __launch_bounds__(256) void pp_horizontal_aug_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ src_offs,
                                                                const int* __restrict__ hs, const int* __restrict__ ws,
                                                                const int* __restrict__ crops, const unsigned char* __restrict__ flips,
                                                                const float* __restrict__ jitter, const unsigned long long* __restrict__ lsum,
                                                                int out_w, unsigned char* tmp, const long long* __restrict__ tmp_offs) {
  __shared__ int kk[256][PP_MAXK + 1];
  const int b = blockIdx.z;
  int W = ws[b], l = crops[4 * b], t = crops[4 * b + 1];
  const int cw = crops[4 * b + 2], ch = crops[4 * b + 3];
  if (!pp_box_ok(hs[b], W, l, t, cw, ch)) return;
  const int y0 = blockIdx.y * PP_ROWS;
  if (y0 >= ch) return;
  const int ox = blockIdx.x * 256 + threadIdx.x;
  if (ox >= out_w) return;
  int lo, n;
  pil_coeffs(cw, out_w, ox, &lo, &n, kk[threadIdx.x]);
  unsigned char* dst = tmp + tmp_offs[b];
  const unsigned char* img = src + src_offs[b];
  if (JIT && !pp_is_identity(pp_factors(jitter, lsum, b))) {
    img = dst + (size_t)ch * out_w * 3;
    W = cw; l = 0; t = 0;
  }
  const int oxw = flips[b] ? out_w - 1 - ox : ox;
  const int y1 = y0 + PP_ROWS < ch ? y0 + PP_ROWS : ch;
  for (int y = y0; y < y1; ++y) {
    const unsigned char* row = img + ((size_t)(t + y) * W + l + lo) * 3;
    int a0 = 1 << (PP_BITS - 1), a1 = a0, a2 = a0;
    for (int x = 0; x < n; ++x) {
      const int k = kk[threadIdx.x][x];
      a0 += (int)row[3 * x] * k; a1 += (int)row[3 * x + 1] * k; a2 += (int)row[3 * x + 2] * k;
    }
    unsigned char* o = dst + ((size_t)y * out_w + oxw) * 3;
    o[0] = pp_clip8(a0); o[1] = pp_clip8(a1); o[2] = pp_clip8(a2);
  }
}

static int preprocess_aug_impl(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int B,
                               const int32_t* crops, const uint8_t* flips, const float* jitter, uint64_t* lsum, int max_crop_h,
                               int max_crop_w, int out_h, int out_w, uint8_t* tmp, const int64_t* tmp_offs, float* out, uint8_t* out_u8,
                               void* stream) {
  if (!src || !src_offs || !heights || !widths || !crops || !flips || !tmp || !tmp_offs || (!out && !out_u8)) return DOD_ERR_INVALID;
  if (B <= 0 || out_h <= 0 || out_w <= 0 || max_crop_h <= 0 || max_crop_w <= 0 || B > 65535) return DOD_ERR_INVALID;
  // window taps of the largest crop
  const int kh = ((max_crop_w + out_w - 1) / out_w) * 2 + 1, kv = ((max_crop_h + out_h - 1) / out_h) * 2 + 1;
  if (kh > PP_MAXK || kv > PP_MAXK) return DOD_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  const dim3 gh((out_w + 255) / 256, (max_crop_h + PP_ROWS - 1) / PP_ROWS, B);
  const int sum_blocks = (max_crop_h + PP_SUM_ROWS - 1) / PP_SUM_ROWS;
  if (jitter && lsum) {
    if (hipMemsetAsync(lsum, 0, (size_t)B * sizeof(uint64_t), s) != hipSuccess) return DOD_ERR_HIP;
    hipLaunchKernelGGL(pp_luma_sum_kernel, dim3(sum_blocks, B), dim3(256), 0, s, (const unsigned char*)src, (const long long*)src_offs,
                       heights, widths, crops, jitter, (unsigned long long*)lsum);
  }
  if (jitter) {
    hipLaunchKernelGGL(pp_jitter_kernel, dim3((max_crop_w + 255) / 256, sum_blocks, B), dim3(256), 0, s, (const unsigned char*)src,
                       (const long long*)src_offs, heights, widths, crops, jitter, (const unsigned long long*)lsum, out_w,
                       (unsigned char*)tmp, (const long long*)tmp_offs);
    hipLaunchKernelGGL(pp_horizontal_aug_kernel<true>, gh, dim3(256), 0, s, (const unsigned char*)src, (const long long*)src_offs, heights,
                       widths, crops, (const unsigned char*)flips, jitter, (const unsigned long long*)lsum, out_w, (unsigned char*)tmp,
                       (const long long*)tmp_offs);
  } else {
    hipLaunchKernelGGL(pp_horizontal_aug_kernel<false>, gh, dim3(256), 0, s, (const unsigned char*)src, (const long long*)src_offs, heights,
                       widths, crops, (const unsigned char*)flips, jitter, (const unsigned long long*)lsum, out_w, (unsigned char*)tmp,
                       (const long long*)tmp_offs);
  }
  hipLaunchKernelGGL(pp_vertical_kernel<4>, dim3(out_h, B), dim3(256), 0, s, (const unsigned char*)tmp, (const long long*)tmp_offs,
                     crops + 3, out_h, out_w, out, (unsigned char*)out_u8);
  return hipGetLastError() == hipSuccess ? DOD_OK : DOD_ERR_HIP;
}

extern "C" int dod_preprocess_aug(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int B,
                                  const int32_t* crops, const uint8_t* flips, const float* jitter, uint64_t* lsum, int max_crop_h,
                                  int max_crop_w, int out_h, int out_w, uint8_t* tmp, const int64_t* tmp_offs, float* out, void* stream) {
  return preprocess_aug_impl(src, src_offs, heights, widths, B, crops, flips, jitter, lsum, max_crop_h, max_crop_w, out_h, out_w, tmp,
                             tmp_offs, out, nullptr, stream);
}
extern "C" int dod_preprocess_aug_u8(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int B,
                                     const int32_t* crops, const uint8_t* flips, const float* jitter, uint64_t* lsum, int max_crop_h,
                                     int max_crop_w, int out_h, int out_w, uint8_t* tmp, const int64_t* tmp_offs, uint8_t* out_hwc,
                                     void* stream) {
  return preprocess_aug_impl(src, src_offs, heights, widths, B, crops, flips, jitter, lsum, max_crop_h, max_crop_w, out_h, out_w, tmp,
                             tmp_offs, nullptr, out_hwc, stream);
}
