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
//
// Train-time augmentation runs in the same two passes (dod_preprocess_aug): per image a crop box (left, top, width, height), a
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
//
// There is ONE chain -- [luma sums] [jittered crops] horizontal pass -- over ITEMS (pp_item_t below).  The three entries differ in
// how item i is described: a whole image (dod_preprocess), a crop of image i (dod_preprocess_aug), a piece of a composed canvas
// (dod_preprocess_compose).  A vertical pass per entry finishes the resize and writes the output format.
#include "dod_common.h"
#include "../../include/dinodet.h"

#define PP_BITS 22
#define PP_MAXK 32          // window taps at most (down-scaling up to 15x)

// the window of `in` source pixels per `out` output pixels has ceil(max(scale, 1)) * 2 + 1 taps: they must fit PP_MAXK.  Both sizes
// are positive (every caller has checked that), so the division is the unsigned one.
__host__ __device__ __forceinline__ bool pp_taps_ok(unsigned in, unsigned out) { return ((in + out - 1) / out) * 2 + 1 <= PP_MAXK; }

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

// factors of one item (1.0 = skip the step); the contrast factor counts only when the luma sums exist
struct pp_jitter_t { float bf, cf, sf; };
__device__ __forceinline__ pp_jitter_t pp_factors(const float* jitter, const unsigned long long* lsum, int i) {
  pp_jitter_t j = {jitter[3 * i], lsum ? jitter[3 * i + 1] : 1.0f, jitter[3 * i + 2]};
  return j;
}
__device__ __forceinline__ bool pp_is_identity(const pp_jitter_t& j) { return j.bf == 1.0f && j.cf == 1.0f && j.sf == 1.0f; }

// ---------------------------------------------------------------------------------------------------------------------------
// One item of the chain: source image `src` with rows of W pixels, the box (l, t, cw, ch) of it that is resized, the flip, and dw =
// the width of the item's horizontal-pass rows.  Item i's tmp (at tmp_offs[i]) holds [ch][dw][3] horizontal-pass rows, then (with
// jitter) the [ch][cw][3] jittered crop.  A piece is an item with a place in its canvas.
struct pp_item_t { int src, W, l, t, cw, ch, flip, dw; };
struct pp_piece_t : pp_item_t { int dx, dy, dh; };

// a box that does not lie inside its image is never read (the host wrapper rejects it; a C caller's mistake must not fault)
__device__ __forceinline__ bool pp_box_ok(int H, int W, int l, int t, int cw, int ch) {
  return l >= 0 && t >= 0 && cw >= 1 && ch >= 1 && cw <= W - l && ch <= H - t;
}

// The three descriptions of item i, one per entry.  load() = false: the item is absent, nothing of it is read or written.  COLS = the
// output columns (= threads) of a horizontal-pass block; JITTERS = the entry has a colour jitter.

// image i as it is.  No box check: an image without rows or columns has no taps and comes out as zeros, like every other size.
struct pp_whole_t {
  typedef pp_item_t item; static constexpr int COLS = 256; static constexpr bool JITTERS = false;
  const int* hs; const int* ws; int out_w;
  __device__ __forceinline__ bool load(int i, item* q) const {
    q->src = i; q->W = ws[i]; q->l = 0; q->t = 0; q->cw = q->W; q->ch = hs[i]; q->flip = 0; q->dw = out_w;
    return true;
  }
};

// the box crops[i] of image i, flipped if flips[i]
struct pp_crops_t {
  typedef pp_item_t item; static constexpr int COLS = 256; static constexpr bool JITTERS = true;
  const int* hs; const int* ws; const int* crops; const unsigned char* flips; int out_w;
  __device__ __forceinline__ bool load(int i, item* q) const {
    q->src = i; q->W = ws[i]; q->l = crops[4 * i]; q->t = crops[4 * i + 1]; q->cw = crops[4 * i + 2]; q->ch = crops[4 * i + 3];
    q->flip = flips[i]; q->dw = out_w;
    return pp_box_ok(hs[i], q->W, q->l, q->t, q->cw, q->ch);
  }
};

// piece i of a composed canvas (include/dinodet.h lists the reasons a piece is absent).  One wave per block (PP_PCOLS = 64 columns): a
// piece is narrower than its canvas, and a 256-column block whose upper waves leave at once still holds the whole block's 33 KB of
// weights in LDS -- at four blocks per CU that left two live waves per SIMD on quadrants of half the canvas width.
#define PP_PCOLS 64
struct pp_canvas_t { int S, P, out_h, out_w, max_ch, max_cw, max_dw; };
struct pp_pieces_t {
  typedef pp_piece_t item; static constexpr int COLS = PP_PCOLS; static constexpr bool JITTERS = true;
  const int* hs; const int* ws; const int* pieces; pp_canvas_t cv;
  __device__ __forceinline__ bool load(int i, item* q) const {
    const int* r = pieces + (size_t)i * 10;
    q->src = r[0]; q->l = r[1]; q->t = r[2]; q->cw = r[3]; q->ch = r[4]; q->flip = r[5]; q->dx = r[6]; q->dy = r[7]; q->dw = r[8]; q->dh = r[9];
    if (q->src < 0 || q->src >= cv.S) return false;
    q->W = ws[q->src];
    if (!pp_box_ok(hs[q->src], q->W, q->l, q->t, q->cw, q->ch)) return false;
    if (q->dx < 0 || q->dy < 0 || q->dw < 1 || q->dh < 1 || q->dw > cv.out_w - q->dx || q->dh > cv.out_h - q->dy) return false;
    if (q->cw > cv.max_cw || q->ch > cv.max_ch || q->dw > cv.max_dw) return false;      // the grids would not cover it
    return pp_taps_ok(q->cw, q->dw) && pp_taps_ok(q->ch, q->dh);
  }
};

// The chain's kernels, each written once over the description G of an item.

// lsum[i] += the sum of the luma of item i's pixels after the brightness step, for every item whose contrast factor is not 1.
// Grid (row blocks, items); block = PP_SUM_ROWS rows of the box, threads along its pixels.
#define PP_SUM_ROWS 8
template <class G>
__global__ __launch_bounds__(256) void pp_luma_sum_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ src_offs, G items,
                                                          const float* __restrict__ jitter, unsigned long long* __restrict__ lsum) {
  __shared__ unsigned long long part[4];
  const int i = blockIdx.y;
  if (jitter[3 * i + 1] == 1.0f) return;            // the mean is not used
  typename G::item q;
  if (!items.load(i, &q)) return;
  const unsigned char* img = src + src_offs[q.src];
  const float bf = jitter[3 * i];
  const int y0 = blockIdx.x * PP_SUM_ROWS;
  if (y0 >= q.ch) return;
  const int y1 = y0 + PP_SUM_ROWS < q.ch ? y0 + PP_SUM_ROWS : q.ch;
  unsigned long long acc = 0;
  for (int y = y0; y < y1; ++y) {
    const unsigned char* row = img + ((size_t)(q.t + y) * q.W + q.l) * 3;
    for (int x = threadIdx.x; x < q.cw; x += 256) {
      int r = row[3 * x], g = row[3 * x + 1], bl = row[3 * x + 2];
      if (bf != 1.0f) { r = pp_blend(0, r, bf); g = pp_blend(0, g, bf); bl = pp_blend(0, bl, bf); }
      acc += (unsigned long long)pp_luma(r, g, bl);
    }
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(&lsum[i], part[0] + part[1] + part[2] + part[3]);
}

// the jittered box of item i, [ch][cw][3] bytes behind its horizontal-pass rows, for every item with a factor != 1.  Grid (column
// blocks, row blocks, items); block = 256 box columns x PP_SUM_ROWS box rows, one pixel per thread and row.  lsum[i] is the box's
// luma sum, read when the contrast factor is not 1.
template <class G>
__global__ __launch_bounds__(256) void pp_jitter_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ src_offs, G items,
                                                        const float* __restrict__ jitter, const unsigned long long* __restrict__ lsum,
                                                        unsigned char* __restrict__ tmp, const long long* __restrict__ tmp_offs) {
  const int i = blockIdx.z;
  const pp_jitter_t j = pp_factors(jitter, lsum, i);
  if (pp_is_identity(j)) return;                     // the horizontal pass reads the source
  typename G::item q;
  if (!items.load(i, &q)) return;
  const unsigned char* img = src + src_offs[q.src];
  unsigned char* dst = tmp + tmp_offs[i] + (size_t)q.ch * q.dw * 3;
  const int y0 = blockIdx.y * PP_SUM_ROWS;
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (y0 >= q.ch || x >= q.cw) return;
  int m = 0;
  if (j.cf != 1.0f) {
#pragma clang fp contract(off)
    m = (int)((double)lsum[i] / (double)((long long)q.cw * q.ch) + 0.5);      // ImageStat mean, rounded as ImageEnhance.Contrast does
  }
  const int y1 = y0 + PP_SUM_ROWS < q.ch ? y0 + PP_SUM_ROWS : q.ch;
  for (int y = y0; y < y1; ++y) {
    const unsigned char* p = img + ((size_t)(q.t + y) * q.W + q.l + x) * 3;
    int r = p[0], g = p[1], bl = p[2];
    if (j.bf != 1.0f) { r = pp_blend(0, r, j.bf); g = pp_blend(0, g, j.bf); bl = pp_blend(0, bl, j.bf); }
    if (j.cf != 1.0f) { r = pp_blend(m, r, j.cf); g = pp_blend(m, g, j.cf); bl = pp_blend(m, bl, j.cf); }
    if (j.sf != 1.0f) { const int lu = pp_luma(r, g, bl); r = pp_blend(lu, r, j.sf); g = pp_blend(lu, g, j.sf); bl = pp_blend(lu, bl, j.sf); }
    unsigned char* o = dst + ((size_t)y * q.cw + x) * 3;
    o[0] = (unsigned char)r; o[1] = (unsigned char)g; o[2] = (unsigned char)bl;
  }
}

// horizontal pass over the box of one item: dst[y][ox'][c] for box rows y and dw columns, ox' = the flipped column when flip.  Called
// by every thread of a block of COLS output columns (blockIdx.x; COLS threads) x PP_ROWS box rows (blockIdx.y), with block-uniform
// arguments; img = the item's source image, kk = this thread's row of weights in LDS.  jittered: read the jittered box behind the rows
// instead of the source.  (dst is then read and written, in disjoint parts.)  Kept apart from its one kernel on purpose: written into
// the kernel's body, the forms without jitter compiled to 1 % more instructions (profiles/preproc_refactor_ab.txt).
#define PP_ROWS 16
template <int COLS>
__device__ __forceinline__ void pp_horizontal_crop(const unsigned char* img, const pp_item_t& q, bool jittered, unsigned char* dst, int* kk) {
  const int y0 = blockIdx.y * PP_ROWS;
  if (y0 >= q.ch) return;
  const int ox = blockIdx.x * COLS + threadIdx.x;
  if (ox >= q.dw) return;
  int lo, n;
  pil_coeffs(q.cw, q.dw, ox, &lo, &n, kk);
  int W = q.W, l = q.l, t = q.t;
  if (jittered) {
    img = dst + (size_t)q.ch * q.dw * 3;
    W = q.cw; l = 0; t = 0;
  }
  const int oxw = q.flip ? q.dw - 1 - ox : ox;
  const int y1 = y0 + PP_ROWS < q.ch ? y0 + PP_ROWS : q.ch;
  for (int y = y0; y < y1; ++y) {
    const unsigned char* row = img + ((size_t)(t + y) * W + l + lo) * 3;
    int a0 = 1 << (PP_BITS - 1), a1 = a0, a2 = a0;
    for (int x = 0; x < n; ++x) {
      const int k = kk[x];
      a0 += (int)row[3 * x] * k; a1 += (int)row[3 * x + 1] * k; a2 += (int)row[3 * x + 2] * k;
    }
    unsigned char* o = dst + ((size_t)y * q.dw + oxw) * 3;
    o[0] = pp_clip8(a0); o[1] = pp_clip8(a1); o[2] = pp_clip8(a2);
  }
}

// horizontal pass of item i into tmp + tmp_offs[i].  Grid (column blocks, row blocks, items).  JIT = false reads the source; JIT = true
// reads the jittered box where one was written.  (tmp is read and written here, in disjoint parts: no __restrict__ on it.)
template <class G, bool JIT>
__global__ __launch_bounds__(G::COLS) void pp_horizontal_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ src_offs, G items,
                                                                const float* __restrict__ jitter, const unsigned long long* __restrict__ lsum,
                                                                unsigned char* tmp, const long long* __restrict__ tmp_offs) {
  __shared__ int kk[G::COLS][PP_MAXK + 1];      // +1: odd pitch, conflict-free per-thread rows
  const int i = blockIdx.z;
  typename G::item q;
  if (!items.load(i, &q)) return;
  const bool jittered = JIT && !pp_is_identity(pp_factors(jitter, lsum, i));
  pp_horizontal_crop<G::COLS>(src + src_offs[q.src], q, jittered, tmp + tmp_offs[i], kk[threadIdx.x]);
}

// the buffers every entry takes: sources, temporary, one of the two outputs; who: the entry point's name, for its messages
struct pp_io_t {
  const uint8_t* src; const int64_t* src_offs; const int32_t* hs; const int32_t* ws; uint8_t* tmp; const int64_t* tmp_offs;
  float* out; uint8_t* out_u8; hipStream_t s; const char* who;
};

// what every entry checks before it launches anything: its pointers, n items within the grid limit, and the window taps of the
// largest box at the output size
static bool pp_args_ok(const pp_io_t& io, int n, int max_h, int max_w, int out_h, int out_w) {
  if (!io.src || !io.src_offs || !io.hs || !io.ws || !io.tmp || !io.tmp_offs || (!io.out && !io.out_u8)) return false;
  if (n <= 0 || n > 65535 || out_h <= 0 || out_w <= 0 || max_h <= 0 || max_w <= 0) return false;
  return pp_taps_ok(max_w, out_w) && pp_taps_ok(max_h, out_h);
}

// [memset + luma sums] [jittered crops] horizontal pass of n items, the largest of them max_ch x max_cw into max_dw columns
template <class G>
static int pp_chain(const pp_io_t& io, const G& g, int n, int max_ch, int max_cw, int max_dw, const float* jitter, uint64_t* lsum) {
  const long long* so = (const long long*)io.src_offs;
  const long long* to = (const long long*)io.tmp_offs;
  const unsigned long long* ls = (const unsigned long long*)lsum;
  const dim3 gh((max_dw + G::COLS - 1) / G::COLS, (max_ch + PP_ROWS - 1) / PP_ROWS, n);
  if constexpr (G::JITTERS) {
    if (jitter) {
      const int sum_blocks = (max_ch + PP_SUM_ROWS - 1) / PP_SUM_ROWS;
      if (lsum) {
        if (hipMemsetAsync(lsum, 0, (size_t)n * sizeof(uint64_t), io.s) != hipSuccess) return dod_fail(DOD_ERR_HIP, "%s: hipMemsetAsync failed", io.who);
        hipLaunchKernelGGL(pp_luma_sum_kernel<G>, dim3(sum_blocks, n), dim3(256), 0, io.s, io.src, so, g, jitter, (unsigned long long*)lsum);
      }
      hipLaunchKernelGGL(pp_jitter_kernel<G>, dim3((max_cw + 255) / 256, sum_blocks, n), dim3(256), 0, io.s, io.src, so, g, jitter, ls, io.tmp, to);
      hipLaunchKernelGGL((pp_horizontal_kernel<G, true>), gh, dim3(G::COLS), 0, io.s, io.src, so, g, jitter, ls, io.tmp, to);
      return DOD_OK;
    }
  }
  hipLaunchKernelGGL((pp_horizontal_kernel<G, false>), gh, dim3(G::COLS), 0, io.s, io.src, so, g, jitter, ls, io.tmp, to);
  return DOD_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The vertical pass and the output format, shared by the per-image pass and the compose pass.

// filtered byte t of an output row: n rows of `pitch` bytes from `rows` on, weights kk
__device__ __forceinline__ unsigned char pp_vertical_byte(const unsigned char* __restrict__ rows, size_t pitch, int t, int n, const int* kk) {
  int acc = 1 << (PP_BITS - 1);
  for (int y = 0; y < n; ++y) acc += (int)rows[(size_t)y * pitch + t] * kk[y];
  return pp_clip8(acc);
}

// row oy of output b in either format, and the store of its byte t (of 3 * out_w): the resampled bytes uint8 HWC (the fused patch
// embed divides by 255), or ToTensor's float32 CHW
struct pp_out_row_t { unsigned char* u8; float* f; size_t plane; };
__device__ __forceinline__ pp_out_row_t pp_out_row(float* out, unsigned char* out_u8, int b, int oy, int out_h, int out_w) {
  pp_out_row_t r = {out_u8 ? out_u8 + ((size_t)b * out_h + oy) * out_w * 3 : nullptr,
                    out ? out + ((size_t)b * 3 * out_h + oy) * out_w : nullptr, (size_t)out_h * out_w};      // channel c at + c * plane
  return r;
}
__device__ __forceinline__ void pp_emit(const pp_out_row_t& r, int t, unsigned char v) {
  const int ox = t / 3, c = t - ox * 3;
  if (r.u8) r.u8[t] = v;
  else r.f[c * r.plane + ox] = (float)v / 255.0f;
}

// vertical pass + ToTensor of image b's horizontal-pass rows.  Block = one output row; threads along its 3*out_w bytes.
// Image b's source height is hs[b * HS]: HS = 1 for the plain heights, 4 for the height column of the crop boxes.
template <int HS>
__global__ __launch_bounds__(256) void pp_vertical_kernel(const unsigned char* __restrict__ tmp, const long long* __restrict__ tmp_offs,
                                                          const int* __restrict__ hs, int out_h, int out_w, float* __restrict__ out,
                                                          unsigned char* __restrict__ out_u8) {
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
  const int n = s_n;
  const int rowbytes = out_w * 3;
  const unsigned char* rows = tmp + tmp_offs[b] + (size_t)s_lo * rowbytes;
  const pp_out_row_t o = pp_out_row(out, out_u8, b, oy, out_h, out_w);
  for (int t = threadIdx.x; t < rowbytes; t += 256) pp_emit(o, t, pp_vertical_byte(rows, rowbytes, t, n, kk));
}

// the per-image vertical pass behind the chain; hs and HS as the kernel takes them
template <int HS>
static int pp_vertical(const pp_io_t& io, const int32_t* hs, int B, int out_h, int out_w) {
  hipLaunchKernelGGL(pp_vertical_kernel<HS>, dim3(out_h, B), dim3(256), 0, io.s, io.tmp, (const long long*)io.tmp_offs, hs, out_h, out_w, io.out,
                     io.out_u8);
  return dod_launched(io.who);
}

static int preprocess_impl(const pp_io_t& io, int B, int max_h, int max_w, int out_h, int out_w) {
  if (!pp_args_ok(io, B, max_h, max_w, out_h, out_w)) return dod_fail(DOD_ERR_INVALID, "%s: null argument, B or a size outside the limits, or more than 32 taps", io.who);
  const pp_whole_t g = {io.hs, io.ws, out_w};
  const int rc = pp_chain(io, g, B, max_h, max_w, out_w, nullptr, nullptr);
  return rc ? rc : pp_vertical<1>(io, io.hs, B, out_h, out_w);
}

extern "C" int dod_preprocess(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int B,
                              int max_h, int max_w, int out_h, int out_w, uint8_t* tmp, const int64_t* tmp_offs, float* out,
                              void* stream) {
  return preprocess_impl({src, src_offs, heights, widths, tmp, tmp_offs, out, nullptr, (hipStream_t)stream, "dod_preprocess"}, B, max_h, max_w, out_h, out_w);
}
extern "C" int dod_preprocess_u8(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int B,
                                 int max_h, int max_w, int out_h, int out_w, uint8_t* tmp, const int64_t* tmp_offs, uint8_t* out_hwc,
                                 void* stream) {
  return preprocess_impl({src, src_offs, heights, widths, tmp, tmp_offs, nullptr, out_hwc, (hipStream_t)stream, "dod_preprocess_u8"}, B, max_h, max_w, out_h, out_w);
}

static int preprocess_aug_impl(const pp_io_t& io, int B, const int32_t* crops, const uint8_t* flips, const float* jitter, uint64_t* lsum,
                               int max_crop_h, int max_crop_w, int out_h, int out_w) {
  if (!crops || !flips || !pp_args_ok(io, B, max_crop_h, max_crop_w, out_h, out_w))
    return dod_fail(DOD_ERR_INVALID, "%s: null argument, B or a size outside the limits, or more than 32 taps", io.who);
  const pp_crops_t g = {io.hs, io.ws, crops, flips, out_w};
  const int rc = pp_chain(io, g, B, max_crop_h, max_crop_w, out_w, jitter, lsum);
  return rc ? rc : pp_vertical<4>(io, crops + 3, B, out_h, out_w);
}

extern "C" int dod_preprocess_aug(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int B,
                                  const int32_t* crops, const uint8_t* flips, const float* jitter, uint64_t* lsum, int max_crop_h,
                                  int max_crop_w, int out_h, int out_w, uint8_t* tmp, const int64_t* tmp_offs, float* out, void* stream) {
  return preprocess_aug_impl({src, src_offs, heights, widths, tmp, tmp_offs, out, nullptr, (hipStream_t)stream, "dod_preprocess_aug"}, B, crops, flips, jitter, lsum,
                             max_crop_h, max_crop_w, out_h, out_w);
}
extern "C" int dod_preprocess_aug_u8(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int B,
                                     const int32_t* crops, const uint8_t* flips, const float* jitter, uint64_t* lsum, int max_crop_h,
                                     int max_crop_w, int out_h, int out_w, uint8_t* tmp, const int64_t* tmp_offs, uint8_t* out_hwc,
                                     void* stream) {
  return preprocess_aug_impl({src, src_offs, heights, widths, tmp, tmp_offs, nullptr, out_hwc, (hipStream_t)stream, "dod_preprocess_aug_u8"}, B, crops, flips, jitter, lsum,
                             max_crop_h, max_crop_w, out_h, out_w);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Composed canvases (dod_preprocess_compose): mosaic, zoom-out and any other paste of disjoint pieces onto a fill colour.  A piece
// is the chain above (crop -> jitter -> resize -> flip) of one source at its own output size dw x dh, pasted at (dx, dy):
//   canvas = Image.new("RGB", (out_w, out_h), fill);  canvas.paste(chain(source[src], crop, jitter, (dw, dh), flip), (dx, dy)) ...
// The chain runs per piece (tmp holds [crop height][dw] rows per piece, the flip applied inside the piece).  ONE vertical + compose
// pass then writes every output byte of every canvas exactly once: a block owns one canvas row, finds the pieces covering it, and
// each byte takes the filtered value of the piece covering it or the fill.  No fill pre-pass, no races between pieces, no atomics
// but the luma sums.
#define PP_MAXP 16          // pieces per canvas: bounds the compose pass's LDS (16 x 33 weights)

// vertical pass + paste + ToTensor.  Block = PP_CROWS consecutive rows (blockIdx.x) of canvas n (blockIdx.y), one row per wave, the
// wave's lanes along the row's 3 * out_w bytes.  The wave first lists the pieces of the canvas that cover its row (at most PP_MAXP
// slots: byte range, weights, rows in tmp; one lane per piece).  It then filters slot by slot, its lanes along the piece's contiguous
// bytes (the weights are LDS broadcasts), and last writes the fill to the bytes no slot covers -- the pieces are disjoint, so every
// byte has one writer.  (One row per block left the listing -- three dependent global loads and the double-precision weights -- in
// front of at most 1.5 KB of work for the whole block: a row per wave measured 2 - 8 % faster end to end)
#define PP_CROWS 4
__global__ __launch_bounds__(64 * PP_CROWS) void pp_compose_kernel(const unsigned char* __restrict__ tmp, const long long* __restrict__ tmp_offs,
                                                                   const int* __restrict__ piece_offsets, pp_pieces_t items,
                                                                   const unsigned char* __restrict__ fills, int fill_per_canvas,
                                                                   float* __restrict__ out, unsigned char* __restrict__ out_u8) {
  __shared__ int s_kk[PP_CROWS][PP_MAXP][PP_MAXK + 1];
  __shared__ int s_x0[PP_CROWS][PP_MAXP], s_x1[PP_CROWS][PP_MAXP], s_n[PP_CROWS][PP_MAXP], s_pitch[PP_CROWS][PP_MAXP];
  __shared__ long long s_base[PP_CROWS][PP_MAXP];
  __shared__ int s_cnt[PP_CROWS];
  const pp_canvas_t& cv = items.cv;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = blockIdx.y, oy = blockIdx.x * PP_CROWS + w;
  const bool live = oy < cv.out_h;
  {
    const int p0 = piece_offsets[n];
    int np = piece_offsets[n + 1] - p0;
    if (p0 < 0 || np < 0 || np > cv.P - p0) np = 0;      // offsets that do not describe pieces: an empty canvas
    if (np > PP_MAXP) np = PP_MAXP;
    pp_piece_t q;
    const bool act = live && lane < np && items.load(p0 + lane, &q) && oy >= q.dy && oy < q.dy + q.dh;
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
  const pp_out_row_t o = pp_out_row(out, out_u8, n, oy, cv.out_h, cv.out_w);
  // the pieces' bytes, slot by slot: the slot's geometry sits in registers and the loop is the per-image vertical kernel's
  for (int i = 0; i < cnt; ++i) {
    const int x0 = s_x0[w][i], x1 = s_x1[w][i], nn = s_n[w][i];
    const size_t pitch = s_pitch[w][i];
    const unsigned char* rows = tmp + (s_base[w][i] - x0);
    const int* kk = s_kk[w][i];
    for (int t = x0 + lane; t < x1; t += 64) pp_emit(o, t, pp_vertical_byte(rows, pitch, t, nn, kk));
  }
  // the bytes no piece covers take the fill
  const unsigned char* fill = fills + (fill_per_canvas ? 3 * n : 0);
  const unsigned char f0 = fill[0], f1 = fill[1], f2 = fill[2];
  for (int t = lane; t < cv.out_w * 3; t += 64) {
    bool covered = false;
    for (int i = 0; i < cnt; ++i) covered |= t >= s_x0[w][i] && t < s_x1[w][i];
    if (covered) continue;
    const int c = t % 3;
    pp_emit(o, t, c == 0 ? f0 : (c == 1 ? f1 : f2));
  }
}

static int preprocess_compose_impl(const pp_io_t& io, int S, const int32_t* pieces, const int32_t* piece_offsets, int N, int P, const float* jitter,
                                   uint64_t* lsum, const uint8_t* fills, int fill_per_canvas, int max_crop_h, int max_crop_w, int max_dw, int out_h,
                                   int out_w) {
  // the taps checked here are those of the largest crop in a piece as large as the canvas: a smaller piece needs more (the loader
  // checks each piece)
  if (!pieces || !piece_offsets || !fills || S <= 0 || N <= 0 || N > 65535 || max_dw <= 0 || max_dw > out_w ||
      !pp_args_ok(io, P, max_crop_h, max_crop_w, out_h, out_w))
    return dod_fail(DOD_ERR_INVALID, "%s: null argument, S / N / P / max_dw or a size outside the limits, or more than 32 taps", io.who);
  const pp_pieces_t g = {io.hs, io.ws, pieces, {S, P, out_h, out_w, max_crop_h, max_crop_w, max_dw}};
  const int rc = pp_chain(io, g, P, max_crop_h, max_crop_w, max_dw, jitter, lsum);
  if (rc) return rc;
  hipLaunchKernelGGL(pp_compose_kernel, dim3((out_h + PP_CROWS - 1) / PP_CROWS, N), dim3(64 * PP_CROWS), 0, io.s, io.tmp, (const long long*)io.tmp_offs,
                     piece_offsets, g, fills, fill_per_canvas, io.out, io.out_u8);
  return dod_launched(io.who);
}

extern "C" int dod_preprocess_compose(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int S,
                                      const int32_t* pieces, const int32_t* piece_offsets, int N, int P, const float* jitter, uint64_t* lsum,
                                      const uint8_t* fills, int fill_per_canvas, int max_crop_h, int max_crop_w, int max_dw, int out_h,
                                      int out_w, uint8_t* tmp, const int64_t* tmp_offs, float* out, void* stream) {
  return preprocess_compose_impl({src, src_offs, heights, widths, tmp, tmp_offs, out, nullptr, (hipStream_t)stream, "dod_preprocess_compose"}, S, pieces, piece_offsets, N, P,
                                 jitter, lsum, fills, fill_per_canvas, max_crop_h, max_crop_w, max_dw, out_h, out_w);
}
extern "C" int dod_preprocess_compose_u8(const uint8_t* src, const int64_t* src_offs, const int32_t* heights, const int32_t* widths, int S,
                                         const int32_t* pieces, const int32_t* piece_offsets, int N, int P, const float* jitter, uint64_t* lsum,
                                         const uint8_t* fills, int fill_per_canvas, int max_crop_h, int max_crop_w, int max_dw, int out_h,
                                         int out_w, uint8_t* tmp, const int64_t* tmp_offs, uint8_t* out_hwc, void* stream) {
  return preprocess_compose_impl({src, src_offs, heights, widths, tmp, tmp_offs, nullptr, out_hwc, (hipStream_t)stream, "dod_preprocess_compose_u8"}, S, pieces, piece_offsets, N,
                                 P, jitter, lsum, fills, fill_per_canvas, max_crop_h, max_crop_w, max_dw, out_h, out_w);
}
