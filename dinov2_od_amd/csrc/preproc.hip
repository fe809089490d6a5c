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

// the three per-crop loops, shared by the per-image kernels (dod_preprocess_aug) and the per-piece ones (dod_preprocess_compose); each
// is called by every thread of its block with block-uniform arguments.

// *dst += sum of the luma of the crop's pixels after the brightness step.  Block = PP_SUM_ROWS rows (blockIdx.x) of the crop, threads
// along its pixels.
#define PP_SUM_ROWS 8
__device__ __forceinline__ void pp_luma_sum_crop(const unsigned char* __restrict__ img, int W, int l, int t, int cw, int ch, float bf,
                                                 unsigned long long* __restrict__ dst) {
  __shared__ unsigned long long part[4];
  const int y0 = blockIdx.x * PP_SUM_ROWS;
  if (y0 >= ch) return;
  const int y1 = y0 + PP_SUM_ROWS < ch ? y0 + PP_SUM_ROWS : ch;
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
  if (threadIdx.x == 0) atomicAdd(dst, part[0] + part[1] + part[2] + part[3]);
}

// the jittered crop, [ch][cw][3] bytes at dst.  Block = 256 crop columns (blockIdx.x) x PP_SUM_ROWS crop rows (blockIdx.y), one pixel
// per thread and row; *ls is the crop's luma sum, read when the contrast factor is not 1.
__device__ __forceinline__ void pp_jitter_crop(const unsigned char* __restrict__ img, int W, int l, int t, int cw, int ch,
                                               const pp_jitter_t& j, const unsigned long long* __restrict__ ls,
                                               unsigned char* __restrict__ dst) {
  const int y0 = blockIdx.y * PP_SUM_ROWS;
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (y0 >= ch || x >= cw) return;
  int m = 0;
  if (j.cf != 1.0f) {
#pragma clang fp contract(off)
    m = (int)((double)*ls / (double)((long long)cw * ch) + 0.5);      // ImageStat mean, rounded as ImageEnhance.Contrast does
  }
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

// horizontal pass over the crop: dst[y][ox'][c] for crop rows y and out_w columns, ox' = the flipped column when flip.  Block = COLS
// output columns (blockIdx.x; COLS threads) x PP_ROWS crop rows (blockIdx.y), as in the plain kernel; kk = this thread's row of weights
// in LDS.  jittered: read the jittered crop behind the rows instead of the source.  (dst is then read and written, in disjoint parts.)
template <int COLS>
__device__ __forceinline__ void pp_horizontal_crop(const unsigned char* img, int W, int l, int t, int cw, int ch, bool jittered, bool flip,
                                                   int out_w, unsigned char* dst, int* kk) {
  const int y0 = blockIdx.y * PP_ROWS;
  if (y0 >= ch) return;
  const int ox = blockIdx.x * COLS + threadIdx.x;
  if (ox >= out_w) return;
  int lo, n;
  pil_coeffs(cw, out_w, ox, &lo, &n, kk);
  if (jittered) {
    img = dst + (size_t)ch * out_w * 3;
    W = cw; l = 0; t = 0;
  }
  const int oxw = flip ? out_w - 1 - ox : ox;
  const int y1 = y0 + PP_ROWS < ch ? y0 + PP_ROWS : ch;
  for (int y = y0; y < y1; ++y) {
    const unsigned char* row = img + ((size_t)(t + y) * W + l + lo) * 3;
    int a0 = 1 << (PP_BITS - 1), a1 = a0, a2 = a0;
    for (int x = 0; x < n; ++x) {
      const int k = kk[x];
      a0 += (int)row[3 * x] * k; a1 += (int)row[3 * x + 1] * k; a2 += (int)row[3 * x + 2] * k;
    }
    unsigned char* o = dst + ((size_t)y * out_w + oxw) * 3;
    o[0] = pp_clip8(a0); o[1] = pp_clip8(a1); o[2] = pp_clip8(a2);
  }
}

// lsum[b] += the luma sum of image b's crop, for every image whose contrast factor is not 1.  Grid (row blocks, B).
__global__ __launch_bounds__(256) void pp_luma_sum_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ src_offs,
                                                          const int* __restrict__ hs, const int* __restrict__ ws,
                                                          const int* __restrict__ crops, const float* __restrict__ jitter,
                                                          unsigned long long* __restrict__ lsum) {
  const int b = blockIdx.y;
  if (jitter[3 * b + 1] == 1.0f) return;            // the mean is not used
  const int W = ws[b], l = crops[4 * b], t = crops[4 * b + 1], cw = crops[4 * b + 2], ch = crops[4 * b + 3];
  if (!pp_box_ok(hs[b], W, l, t, cw, ch)) return;
  pp_luma_sum_crop(src + src_offs[b], W, l, t, cw, ch, jitter[3 * b], &lsum[b]);
}

// the jittered crop of image b at tmp + tmp_offs[b] + ch * out_w * 3 (behind its horizontal-pass rows), for every image with a
// factor != 1.  Grid (column blocks, row blocks, B).
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
  pp_jitter_crop(src + src_offs[b], W, l, t, cw, ch, j, lsum + b, tmp + tmp_offs[b] + (size_t)ch * out_w * 3);
}

// horizontal pass of image b's crop into tmp + tmp_offs[b].  JIT = false is the plain kernel's loop on the crop's rows and columns;
// JIT = true reads the jittered crop where one was written.  (tmp is read and written here, in disjoint parts: no __restrict__ on it.)
template <bool JIT>
__global__ __launch_bounds__(256) void pp_horizontal_aug_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ src_offs,
                                                                const int* __restrict__ hs, const int* __restrict__ ws,
                                                                const int* __restrict__ crops, const unsigned char* __restrict__ flips,
                                                                const float* __restrict__ jitter, const unsigned long long* __restrict__ lsum,
                                                                int out_w, unsigned char* tmp, const long long* __restrict__ tmp_offs) {
  __shared__ int kk[256][PP_MAXK + 1];
  const int b = blockIdx.z;
  const int W = ws[b], l = crops[4 * b], t = crops[4 * b + 1], cw = crops[4 * b + 2], ch = crops[4 * b + 3];
  if (!pp_box_ok(hs[b], W, l, t, cw, ch)) return;
  const bool jittered = JIT && !pp_is_identity(pp_factors(jitter, lsum, b));
  pp_horizontal_crop<256>(src + src_offs[b], W, l, t, cw, ch, jittered, flips[b] != 0, out_w, tmp + tmp_offs[b], kk[threadIdx.x]);
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

// ---------------------------------------------------------------------------------------------------------------------------
// Composed canvases (dod_preprocess_compose): mosaic, zoom-out and any other paste of disjoint pieces onto a fill colour.  A piece
// is the chain above (crop -> jitter -> resize -> flip) of one source at its own output size dw x dh, pasted at (dx, dy):
//   canvas = Image.new("RGB", (out_w, out_h), fill);  canvas.paste(chain(source[src], crop, jitter, (dw, dh), flip), (dx, dy)) ...
// The luma sum, the jittered crop and the horizontal pass run per piece (the loops above, indexed by piece: tmp holds
// [crop height][dw] rows per piece, the flip applied inside the piece).  ONE vertical + compose pass then writes every output byte of
// every canvas exactly once: a block owns one canvas row, finds the pieces covering it, and each byte takes the filtered value of
// the piece covering it or the fill.  No fill pre-pass, no races between pieces, no atomics but the luma sums.
#define PP_MAXP 16          // pieces per canvas: bounds the compose pass's LDS (16 x 33 weights)

struct pp_piece_t { int src, l, t, cw, ch, flip, dx, dy, dw, dh; };
struct pp_canvas_t { int S, P, out_h, out_w, max_ch, max_cw, max_dw; };

// piece p and its source's width; false = the piece is absent (include/dinodet.h lists the reasons): nothing of it is read or written
__device__ __forceinline__ bool pp_piece_load(const int* __restrict__ pieces, int p, const int* __restrict__ hs, const int* __restrict__ ws,
                                              const pp_canvas_t& cv, pp_piece_t* q, int* W) {
  const int* r = pieces + (size_t)p * 10;
  q->src = r[0]; q->l = r[1]; q->t = r[2]; q->cw = r[3]; q->ch = r[4]; q->flip = r[5]; q->dx = r[6]; q->dy = r[7]; q->dw = r[8]; q->dh = r[9];
  if (q->src < 0 || q->src >= cv.S) return false;
  *W = ws[q->src];
  if (!pp_box_ok(hs[q->src], *W, q->l, q->t, q->cw, q->ch)) return false;
  if (q->dx < 0 || q->dy < 0 || q->dw < 1 || q->dh < 1 || q->dw > cv.out_w - q->dx || q->dh > cv.out_h - q->dy) return false;
  if (q->cw > cv.max_cw || q->ch > cv.max_ch || q->dw > cv.max_dw) return false;      // the grids would not cover it
  return ((q->cw + q->dw - 1) / q->dw) * 2 + 1 <= PP_MAXK && ((q->ch + q->dh - 1) / q->dh) * 2 + 1 <= PP_MAXK;
}

// piece p's tmp: [ch][dw][3] horizontal-pass rows, then (with jitter) the [ch][cw][3] jittered crop
__global__ __launch_bounds__(256) void pp_piece_luma_sum_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ src_offs,
                                                                const int* __restrict__ hs, const int* __restrict__ ws,
                                                                const int* __restrict__ pieces, pp_canvas_t cv,
                                                                const float* __restrict__ jitter, unsigned long long* __restrict__ lsum) {
  const int p = blockIdx.y;
  if (jitter[3 * p + 1] == 1.0f) return;
  pp_piece_t q; int W;
  if (!pp_piece_load(pieces, p, hs, ws, cv, &q, &W)) return;
  pp_luma_sum_crop(src + src_offs[q.src], W, q.l, q.t, q.cw, q.ch, jitter[3 * p], &lsum[p]);
}

__global__ __launch_bounds__(256) void pp_piece_jitter_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ src_offs,
                                                              const int* __restrict__ hs, const int* __restrict__ ws,
                                                              const int* __restrict__ pieces, pp_canvas_t cv, const float* __restrict__ jitter,
                                                              const unsigned long long* __restrict__ lsum, unsigned char* __restrict__ tmp,
                                                              const long long* __restrict__ tmp_offs) {
  const int p = blockIdx.z;
  const pp_jitter_t j = pp_factors(jitter, lsum, p);
  if (pp_is_identity(j)) return;
  pp_piece_t q; int W;
  if (!pp_piece_load(pieces, p, hs, ws, cv, &q, &W)) return;
  pp_jitter_crop(src + src_offs[q.src], W, q.l, q.t, q.cw, q.ch, j, lsum + p, tmp + tmp_offs[p] + (size_t)q.ch * q.dw * 3);
}

// One wave per block (PP_PCOLS = 64 columns): a piece is narrower than its canvas, and a 256-column block whose upper waves leave at
// once still holds the whole block's 33 KB of weights in LDS -- at four blocks per CU that left two live waves per SIMD on quadrants
// of half the canvas width.
#define PP_PCOLS 64
template <bool JIT>
__global__ __launch_bounds__(PP_PCOLS) void pp_piece_horizontal_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ src_offs,
                                                                  const int* __restrict__ hs, const int* __restrict__ ws,
                                                                  const int* __restrict__ pieces, pp_canvas_t cv, const float* __restrict__ jitter,
                                                                  const unsigned long long* __restrict__ lsum, unsigned char* tmp,
                                                                  const long long* __restrict__ tmp_offs) {
  __shared__ int kk[PP_PCOLS][PP_MAXK + 1];
  const int p = blockIdx.z;
  pp_piece_t q; int W;
  if (!pp_piece_load(pieces, p, hs, ws, cv, &q, &W)) return;
  const bool jittered = JIT && !pp_is_identity(pp_factors(jitter, lsum, p));
  pp_horizontal_crop<PP_PCOLS>(src + src_offs[q.src], W, q.l, q.t, q.cw, q.ch, jittered, q.flip != 0, q.dw, tmp + tmp_offs[p], kk[threadIdx.x]);
}

// vertical pass + paste + ToTensor.  Block = PP_CROWS consecutive rows (blockIdx.x) of canvas n (blockIdx.y), one row per wave, the
// wave's lanes along the row's 3 * out_w bytes.  The wave first lists the pieces of the canvas that cover its row (at most PP_MAXP
// slots: byte range, weights, rows in tmp; one lane per piece).  It then filters slot by slot, its lanes along the piece's contiguous
// bytes (the weights are LDS broadcasts), and last writes the fill to the bytes no slot covers -- the pieces are disjoint, so every
// byte has one writer.  (One row per block left the listing -- three dependent global loads and the double-precision weights -- in
// front of at most 1.5 KB of work for the whole block: a row per wave measured 2 - 8 % faster end to end)
#define PP_CROWS 4
__global__ __launch_bounds__(64 * PP_CROWS) void pp_compose_kernel(const unsigned char* __restrict__ tmp, const long long* __restrict__ tmp_offs,
                                                                   const int* __restrict__ pieces, const int* __restrict__ piece_offsets,
                                                                   const int* __restrict__ hs, const int* __restrict__ ws, pp_canvas_t cv,
                                                                   const unsigned char* __restrict__ fills, int fill_per_canvas,
                                                                   float* __restrict__ out, unsigned char* __restrict__ out_u8) {
  __shared__ int s_kk[PP_CROWS][PP_MAXP][PP_MAXK + 1];
  __shared__ int s_x0[PP_CROWS][PP_MAXP], s_x1[PP_CROWS][PP_MAXP], s_n[PP_CROWS][PP_MAXP], s_pitch[PP_CROWS][PP_MAXP];
  __shared__ long long s_base[PP_CROWS][PP_MAXP];
  __shared__ int s_cnt[PP_CROWS];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = blockIdx.y, oy = blockIdx.x * PP_CROWS + w;
  const bool live = oy < cv.out_h;
  {
    const int p0 = piece_offsets[n];
    int np = piece_offsets[n + 1] - p0;
    if (p0 < 0 || np < 0 || np > cv.P - p0) np = 0;      // offsets that do not describe pieces: an empty canvas
    if (np > PP_MAXP) np = PP_MAXP;
    pp_piece_t q;
    bool act = false;
    if (live && lane < np) {
      int W;
      act = pp_piece_load(pieces, p0 + lane, hs, ws, cv, &q, &W) && oy >= q.dy && oy < q.dy + q.dh;
    }
    const unsigned long long m = __ballot(act);
    if (act) {
      const int slot = __popcll(m & ((1ull << lane) - 1ull));
      int lo, nn;
      pil_coeffs(q.ch, q.dh, oy - q.dy, &lo, &nn, s_kk[w][slot]);
      s_x0[w][slot] = q.dx * 3; s_x1[w][slot] = (q.dx + q.dw) * 3; s_n[w][slot] = nn; s_pitch[w][slot] = q.dw * 3;
      s_base[w][slot] = tmp_offs[p0 + lane] + (long long)lo * q.dw * 3;
    }
    if (lane == 0) s_cnt[w] = __popcll(m);
  }
  __syncthreads();
  if (!live) return;
  const int cnt = s_cnt[w];
  const int rowbytes = cv.out_w * 3;
  unsigned char* row_u8 = out_u8 ? out_u8 + ((size_t)n * cv.out_h + oy) * rowbytes : nullptr;
  float* row_f = out ? out + ((size_t)n * 3 * cv.out_h + oy) * cv.out_w : nullptr;          // channel c at + c * out_h * out_w
  const size_t plane = (size_t)cv.out_h * cv.out_w;
  // the pieces' bytes, slot by slot: the slot's geometry sits in registers and the loop is the plain vertical kernel's
  for (int i = 0; i < cnt; ++i) {
    const int x0 = s_x0[w][i], x1 = s_x1[w][i], pitch = s_pitch[w][i], nn = s_n[w][i];
    const long long base = s_base[w][i] - x0;
    const int* kk = s_kk[w][i];
    for (int t = x0 + lane; t < x1; t += 64) {
      int acc = 1 << (PP_BITS - 1);
      for (int y = 0; y < nn; ++y) acc += (int)tmp[base + (long long)y * pitch + t] * kk[y];
      const unsigned char v = pp_clip8(acc);
      const int ox = t / 3, c = t - ox * 3;
      if (row_u8) row_u8[t] = v;
      else row_f[c * plane + ox] = (float)v / 255.0f;
    }
  }
  // the bytes no piece covers take the fill
  const unsigned char* fill = fills + (fill_per_canvas ? 3 * n : 0);
  const unsigned char f0 = fill[0], f1 = fill[1], f2 = fill[2];
  for (int t = lane; t < rowbytes; t += 64) {
    bool covered = false;
    for (int i = 0; i < cnt; ++i) covered |= t >= s_x0[w][i] && t < s_x1[w][i];
    if (covered) continue;
    const int ox = t / 3, c = t - ox * 3;
    const unsigned char v = c == 0 ? f0 : (c == 1 ? f1 : f2);
    if (row_u8) row_u8[t] = v;
    else row_f[c * plane + ox] = (float)v / 255.0f;
  }
}

static int preprocess_compose_impl(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int S,
                                   const int32_t* pieces, const int32_t* piece_offsets, int N, int P, const float* jitter, uint64_t* lsum,
                                   const uint8_t* fills, int fill_per_canvas, int max_crop_h, int max_crop_w, int max_dw, int out_h, int out_w,
                                   uint8_t* tmp, const int64_t* tmp_offs, float* out, uint8_t* out_u8, void* stream) {
  if (!src || !src_offs || !heights || !widths || !pieces || !piece_offsets || !fills || !tmp || !tmp_offs || (!out && !out_u8))
    return DOD_ERR_INVALID;
  if (S <= 0 || N <= 0 || P <= 0 || N > 65535 || P > 65535 || out_h <= 0 || out_w <= 0 || max_crop_h <= 0 || max_crop_w <= 0 || max_dw <= 0 ||
      max_dw > out_w)
    return DOD_ERR_INVALID;
  // window taps of the largest crop in a piece as large as the canvas: a smaller piece needs more (the kernels check each piece)
  const int kh = ((max_crop_w + out_w - 1) / out_w) * 2 + 1, kv = ((max_crop_h + out_h - 1) / out_h) * 2 + 1;
  if (kh > PP_MAXK || kv > PP_MAXK) return DOD_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  const pp_canvas_t cv = {S, P, out_h, out_w, max_crop_h, max_crop_w, max_dw};
  const dim3 gh((max_dw + PP_PCOLS - 1) / PP_PCOLS, (max_crop_h + PP_ROWS - 1) / PP_ROWS, P);
  const int sum_blocks = (max_crop_h + PP_SUM_ROWS - 1) / PP_SUM_ROWS;
  const unsigned long long* ls = (const unsigned long long*)lsum;
  if (jitter && lsum) {
    if (hipMemsetAsync(lsum, 0, (size_t)P * sizeof(uint64_t), s) != hipSuccess) return DOD_ERR_HIP;
    hipLaunchKernelGGL(pp_piece_luma_sum_kernel, dim3(sum_blocks, P), dim3(256), 0, s, (const unsigned char*)src, (const long long*)src_offs,
                       heights, widths, pieces, cv, jitter, (unsigned long long*)lsum);
  }
  if (jitter) {
    hipLaunchKernelGGL(pp_piece_jitter_kernel, dim3((max_crop_w + 255) / 256, sum_blocks, P), dim3(256), 0, s, (const unsigned char*)src,
                       (const long long*)src_offs, heights, widths, pieces, cv, jitter, ls, (unsigned char*)tmp, (const long long*)tmp_offs);
    hipLaunchKernelGGL(pp_piece_horizontal_kernel<true>, gh, dim3(PP_PCOLS), 0, s, (const unsigned char*)src, (const long long*)src_offs, heights,
                       widths, pieces, cv, jitter, ls, (unsigned char*)tmp, (const long long*)tmp_offs);
  } else {
    hipLaunchKernelGGL(pp_piece_horizontal_kernel<false>, gh, dim3(PP_PCOLS), 0, s, (const unsigned char*)src, (const long long*)src_offs, heights,
                       widths, pieces, cv, jitter, ls, (unsigned char*)tmp, (const long long*)tmp_offs);
  }
  hipLaunchKernelGGL(pp_compose_kernel, dim3((out_h + PP_CROWS - 1) / PP_CROWS, N), dim3(64 * PP_CROWS), 0, s, (const unsigned char*)tmp, (const long long*)tmp_offs, pieces,
                     piece_offsets, heights, widths, cv, (const unsigned char*)fills, fill_per_canvas, out, (unsigned char*)out_u8);
  return hipGetLastError() == hipSuccess ? DOD_OK : DOD_ERR_HIP;
}

extern "C" int dod_preprocess_compose(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int S,
                                      const int32_t* pieces, const int32_t* piece_offsets, int N, int P, const float* jitter, uint64_t* lsum,
                                      const uint8_t* fills, int fill_per_canvas, int max_crop_h, int max_crop_w, int max_dw, int out_h,
                                      int out_w, uint8_t* tmp, const int64_t* tmp_offs, float* out, void* stream) {
  return preprocess_compose_impl(src, src_offs, heights, widths, S, pieces, piece_offsets, N, P, jitter, lsum, fills, fill_per_canvas,
                                 max_crop_h, max_crop_w, max_dw, out_h, out_w, tmp, tmp_offs, out, nullptr, stream);
}
extern "C" int dod_preprocess_compose_u8(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int S,
                                         const int32_t* pieces, const int32_t* piece_offsets, int N, int P, const float* jitter, uint64_t* lsum,
                                         const uint8_t* fills, int fill_per_canvas, int max_crop_h, int max_crop_w, int max_dw, int out_h,
                                         int out_w, uint8_t* tmp, const int64_t* tmp_offs, uint8_t* out_hwc, void* stream) {
  return preprocess_compose_impl(src, src_offs, heights, widths, S, pieces, piece_offsets, N, P, jitter, lsum, fills, fill_per_canvas,
                                 max_crop_h, max_crop_w, max_dw, out_h, out_w, tmp, tmp_offs, nullptr, out_hwc, stream);
}
