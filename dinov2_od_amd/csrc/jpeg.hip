// Baseline JPEG decode on the device (dod_jpeg_*, include/dinodet.h; Python side: dinov2_od_amd/jpeg.py), bit-exact against
// libjpeg-turbo as Pillow drives it (JDCT_ISLOW, fancy upsampling): tests/jpeg_cases.py restates all of it in numpy.
//
//   entropy     jpeg_entropy.h: one thread per restart interval (device), or the host entry over whole scans.  Divergent by nature:
//               64-thread workgroups so that an image's intervals spread over many CUs, nothing clever.
//   IDCT        jidctint.c jpeg_idct_islow restated.  8 threads per 8 x 8 block, 32 blocks per workgroup.  A thread loads one ROW of
//               coefficients as one 16-byte load, multiplies by the quantisation row and parks it in LDS; pass 1 then works on the
//               thread's COLUMN (read from LDS, written back in place: nobody else touches that column), pass 2 on its row again, and
//               the row leaves as one 8-byte store into the component's plane.  Bytes that must move: 128 in, 64 out per block.
//   colour      jdsample.c (h2v1 / h2v2 fancy, plain replication for a component of width <= 2) + jdcolor.c restated.  A thread
//               owns 4 pixels of a row: it reads 4 luma bytes, the 2-4 chroma samples per row it needs, and writes 12 RGB bytes.
//               Bytes that must move per pixel: 1 + 2 / (h v) in, 3 out.  Every output byte is written exactly once.
// A flat grid over all blocks (all 4-pixel items) of the batch; the owner of an index is found by bisection over the batch's
// cumulative table (<= 3 B entries), so ragged batches waste no workgroups.
#include "dod_common.h"
#include "../../include/dinodet.h"
#include "jpeg_entropy.h"

#include <string.h>

// ------------------------------------------------------------------------------------------------------------------- entropy
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ images,
                                                           const int64_t* __restrict__ intervals, int n_intervals, int n_images,
                                                           const int32_t* __restrict__ htabs, int n_htabs, int16_t* __restrict__ coef,
                                                           int64_t coef_blocks, int64_t nbytes, int32_t* __restrict__ status) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= n_intervals) return;
  const int64_t* v = intervals + (size_t)t * DOD_JV_STRIDE;
  const int64_t b = v[DOD_JV_IMAGE];
  if (b < 0 || b >= n_images) return;
  int64_t begin = v[DOD_JV_BEGIN], end = v[DOD_JV_END];
  int flags;
  if (begin < 0 || end > nbytes || end < begin)
    flags = DOD_JPEG_F_TABLE;
  else
    flags = dod_jpeg_decode_interval(bytes, begin, end, images + (size_t)b * DOD_JI_STRIDE, htabs, n_htabs, v[DOD_JV_MCU0], v[DOD_JV_NMCU],
                                     coef, coef_blocks, nullptr);
  if (flags) atomicOr(status + b, flags);
}

// ---------------------------------------------------------------------------------------------------------------------- IDCT
#define JI_CONST_BITS 13
#define JI_PASS1_BITS 2
#define JI_BLOCKS 32      // blocks per workgroup: 256 threads
#define JI_PITCH 9        // ints per LDS row of a block: 8 + 1 so that a column's 8 reads fall on 8 banks

// component table of the IDCT: JC_STRIDE int64 per component of the batch, in coefficient-buffer order
enum { JC_BLOCK0 = 0, JC_BLOCKS_W, JC_PLANE, JC_QT, JC_STRIDE };

// the last row r with table[r * stride] <= g; rows are sorted, table[0] == 0
__device__ __forceinline__ int jpeg_owner(const int64_t* __restrict__ table, int stride, int n, int64_t g) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[(size_t)mid * stride] <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// jidctint.c: one 8-point pass on d[0..7] (already dequantised / from the workspace), results descaled by `shift`
__device__ __forceinline__ void jpeg_idct8(const int32_t* d, int shift, int64_t* o) {
  int64_t z2 = d[2], z3 = d[6];
  int64_t z1 = (z2 + z3) * 4433;                      // FIX_0_541196100
  int64_t tmp2 = z1 + z3 * (-15137);                  // FIX_1_847759065
  int64_t tmp3 = z1 + z2 * 6270;                      // FIX_0_765366865
  z2 = d[0]; z3 = d[4];
  int64_t tmp0 = (z2 + z3) * (1 << JI_CONST_BITS);
  int64_t tmp1 = (z2 - z3) * (1 << JI_CONST_BITS);
  const int64_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = d[7]; tmp1 = d[5]; tmp2 = d[3]; tmp3 = d[1];
  z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
  int64_t z4 = tmp1 + tmp3;
  const int64_t z5 = (z3 + z4) * 9633;               // FIX_1_175875602
  tmp0 *= 2446;                                       // FIX_0_298631336
  tmp1 *= 16819;                                      // FIX_2_053119869
  tmp2 *= 25172;                                      // FIX_3_072711026
  tmp3 *= 12299;                                      // FIX_1_501321110
  z1 *= -7373;                                        // FIX_0_899976223
  z2 *= -20995;                                       // FIX_2_562915447
  z3 *= -16069;                                       // FIX_1_961570560
  z4 *= -3196;                                        // FIX_0_390180644
  z3 += z5; z4 += z5;
  tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
  const int64_t half = (int64_t)1 << (shift - 1);
  o[0] = (tmp10 + tmp3 + half) >> shift; o[7] = (tmp10 - tmp3 + half) >> shift;
  o[1] = (tmp11 + tmp2 + half) >> shift; o[6] = (tmp11 - tmp2 + half) >> shift;
  o[2] = (tmp12 + tmp1 + half) >> shift; o[5] = (tmp12 - tmp1 + half) >> shift;
  o[3] = (tmp13 + tmp0 + half) >> shift; o[4] = (tmp13 - tmp0 + half) >> shift;
}

__global__ __launch_bounds__(JI_BLOCKS * 8) void jpeg_idct_kernel(const int16_t* __restrict__ coef, int64_t n_blocks,
                                                                  const int64_t* __restrict__ comps, int n_comps,
                                                                  const uint16_t* __restrict__ qtabs, int n_qtabs, uint8_t* __restrict__ planes) {
  __shared__ int32_t ws[JI_BLOCKS][8 * JI_PITCH];
  const int lb = threadIdx.x >> 3, t = threadIdx.x & 7;
  const int64_t g = (int64_t)blockIdx.x * JI_BLOCKS + lb;
  const bool live = g < n_blocks;
  const int64_t* cp = nullptr;
  int32_t* w = ws[lb];
  if (live) {
    cp = comps + (size_t)jpeg_owner(comps, JC_STRIDE, n_comps, g) * JC_STRIDE;
    int64_t q = cp[JC_QT];
    q = q < 0 ? 0 : (q >= n_qtabs ? n_qtabs - 1 : q);
    // row t of the block: 8 int16 = 16 bytes (the buffer is 16-byte aligned and a block is 128 bytes), times row t of the table
    const uint4 raw = *reinterpret_cast<const uint4*>(coef + g * 64 + t * 8);
    const uint4 qr = *reinterpret_cast<const uint4*>(qtabs + q * 64 + t * 8);
    const uint32_t cw[4] = {raw.x, raw.y, raw.z, raw.w}, qw[4] = {qr.x, qr.y, qr.z, qr.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      w[t * JI_PITCH + 2 * i] = (int32_t)(int16_t)(cw[i] & 0xffffu) * (int32_t)(qw[i] & 0xffffu);
      w[t * JI_PITCH + 2 * i + 1] = (int32_t)(int16_t)(cw[i] >> 16) * (int32_t)(qw[i] >> 16);
    }
  }
  __syncthreads();
  int32_t d[8];
  int64_t o[8];
  if (live) {
    // pass 1: column t, descale by CONST_BITS - PASS1_BITS; the workspace is int, as the library's
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = w[k * JI_PITCH + t];
    jpeg_idct8(d, JI_CONST_BITS - JI_PASS1_BITS, o);
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k * JI_PITCH + t] = (int32_t)(uint32_t)(uint64_t)o[k];
  }
  __syncthreads();
  if (live) {
    // pass 2: row t, descale by CONST_BITS + PASS1_BITS + 3, centre on 128, range_limit[x & 1023]: x as a 10-bit signed number
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = w[t * JI_PITCH + k];
    jpeg_idct8(d, JI_CONST_BITS + JI_PASS1_BITS + 3, o);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      int x = (int)(((uint32_t)(uint64_t)o[k] & 1023u) ^ 512u) - 512 + 128;
      x = x < 0 ? 0 : (x > 255 ? 255 : x);
      if (k < 4) lo |= (uint32_t)x << (8 * k); else hi |= (uint32_t)x << (8 * (k - 4));
    }
    const int64_t local = g - cp[JC_BLOCK0], bw = cp[JC_BLOCKS_W];
    const int64_t by = local / bw, bx = local - by * bw;
    // planes are 8-byte aligned: plane offsets are multiples of 64 (whole blocks) and a plane row is 8 * blocks_w bytes
    *reinterpret_cast<uint2*>(planes + cp[JC_PLANE] + (by * 8 + t) * (bw * 8) + bx * 8) = make_uint2(lo, hi);
  }
}

// ---------------------------------------------------------------------------------------------------------- upsample + colour
#define JC_THREADS 256

// chroma sample for output pixel (x, y) of a component of dw x dh samples at 1/hs x 1/vs of the luma; pitch = the plane's row bytes
__device__ __forceinline__ int jpeg_chroma(const uint8_t* __restrict__ p, int64_t pitch, int dw, int dh, int hs, int vs, int x, int y) {
  if (hs == 1) return p[(int64_t)y * pitch + x];      // (vs == 1 as well: 1 x 2 luma is not a supported stream)
  const int i = x >> 1;
  if (dw <= 2) return p[(int64_t)(vs == 2 ? y >> 1 : y) * pitch + i];      // the library's plain replication
  if (vs == 1) {
    const uint8_t* row = p + (int64_t)y * pitch;
    const int c = row[i];
    if (x & 1) return i == dw - 1 ? c : (3 * c + row[i + 1] + 2) >> 2;
    return i == 0 ? c : (3 * c + row[i - 1] + 1) >> 2;
  }
  const int r = y >> 1;
  int far = (y & 1) ? r + 1 : r - 1;                  // the neighbouring sample row, the component's edge rows replicated
  far = far < 0 ? 0 : (far > dh - 1 ? dh - 1 : far);
  const uint8_t* near_row = p + (int64_t)r * pitch;
  const uint8_t* far_row = p + (int64_t)far * pitch;
  const int s = 3 * near_row[i] + far_row[i];
  if (x & 1) return i == dw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * near_row[i + 1] + far_row[i + 1] + 7) >> 4;
  return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * near_row[i - 1] + far_row[i - 1] + 8) >> 4;
}

__device__ __forceinline__ int jpeg_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__global__ __launch_bounds__(JC_THREADS) void jpeg_color_kernel(const uint8_t* __restrict__ planes, const int64_t* __restrict__ images,
                                                                 int n_images, int64_t n_items, uint8_t* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * JC_THREADS + threadIdx.x;
  if (g >= n_items) return;
  const int64_t* ji = images + (size_t)jpeg_owner(images + DOD_JI_ITEM0, DOD_JI_STRIDE, n_images, g) * DOD_JI_STRIDE;
  const int W = (int)ji[DOD_JI_WIDTH], H = (int)ji[DOD_JI_HEIGHT];
  const int64_t local = g - ji[DOD_JI_ITEM0];
  const int per_row = (W + 3) >> 2;
  const int y = (int)(local / per_row), x0 = (int)(local - (int64_t)y * per_row) * 4;
  if (y >= H) return;
  const int n = W - x0 < 4 ? W - x0 : 4;
  const int hs = (int)ji[DOD_JI_HS], vs = (int)ji[DOD_JI_VS];
  const int64_t ypitch = ji[DOD_JI_BLOCKS_W] * 8;
  const uint8_t* yrow = planes + ji[DOD_JI_PLANE] + (int64_t)y * ypitch + x0;      // 4-byte aligned; the plane is padded to whole blocks
  const uint32_t y4 = *reinterpret_cast<const uint32_t*>(yrow);
  uint8_t px[12];
  if (ji[DOD_JI_NCOMP] == 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) px[3 * i] = px[3 * i + 1] = px[3 * i + 2] = (uint8_t)(y4 >> (8 * i));
  } else {
    const int dw = (W + hs - 1) / hs, dh = (H + vs - 1) / vs;
    const uint8_t* cbp = planes + ji[DOD_JI_PLANE + 1];
    const uint8_t* crp = planes + ji[DOD_JI_PLANE + 2];
    const int64_t cbpitch = ji[DOD_JI_BLOCKS_W + 1] * 8, crpitch = ji[DOD_JI_BLOCKS_W + 2] * 8;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int x = x0 + i < W ? x0 + i : W - 1;      // lanes past the row's end recompute its last pixel and store nothing
      const int Y = (int)((y4 >> (8 * i)) & 255u);
      const int cb = jpeg_chroma(cbp, cbpitch, dw, dh, hs, vs, x, y) - 128;
      const int cr = jpeg_chroma(crp, crpitch, dw, dh, hs, vs, x, y) - 128;
      px[3 * i] = (uint8_t)jpeg_clamp8(Y + ((91881 * cr + 32768) >> 16));
      px[3 * i + 1] = (uint8_t)jpeg_clamp8(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
      px[3 * i + 2] = (uint8_t)jpeg_clamp8(Y + ((116130 * cb + 32768) >> 16));
    }
  }
  uint8_t* o = out + ji[DOD_JI_OUT] + ((int64_t)y * W + x0) * 3;
  if (n == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
    uint32_t w3[3];
    memcpy(w3, px, 12);
    uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
    o4[0] = w3[0]; o4[1] = w3[1]; o4[2] = w3[2];
  } else {
    for (int i = 0; i < 3 * n; ++i) o[i] = px[i];
  }
}

// ------------------------------------------------------------------------------------------------------------ entry points
extern "C" int dod_jpeg_entropy_host(const uint8_t* bytes, int64_t nbytes, const int64_t* images, int first, int count, const int32_t* htabs,
                                     int n_htabs, int16_t* coef, int64_t coef_blocks, int32_t* status) {
  if (!bytes || !images || !htabs || !coef || !status || nbytes < 0 || first < 0 || count < 0 || n_htabs < 1 || coef_blocks < 0) return dod_fail(DOD_ERR_INVALID, "dod_jpeg_entropy_host: null argument, or a negative nbytes / first / count / coef_blocks, or n_htabs < 1");
  for (int b = first; b < first + count; ++b) {
    const int64_t* ji = images + (size_t)b * DOD_JI_STRIDE;
    const int ncomp = (int)ji[DOD_JI_NCOMP];
    int flags = 0;
    // the image's own blocks start from zero: components are adjacent in the buffer, so one range covers them
    if (ncomp == 1 || ncomp == 3) {
      for (int c = 0; c < ncomp && !flags; ++c) {
        const int64_t b0 = ji[DOD_JI_BLOCK0 + c], bw = ji[DOD_JI_BLOCKS_W + c], rows = ji[DOD_JI_MCUS_Y] * (c == 0 ? ji[DOD_JI_VS] : 1);
        if (b0 < 0 || bw < 1 || bw > 131072 || rows < 1 || rows > 131072 || b0 + bw * rows > coef_blocks) flags = DOD_JPEG_F_TABLE;
        else memset(coef + b0 * 64, 0, (size_t)(bw * rows) * 64 * sizeof(int16_t));
      }
    } else {
      flags = DOD_JPEG_F_TABLE;
    }
    if (!flags) flags = dod_jpeg_decode_scan(bytes, nbytes, ji, htabs, n_htabs, coef, coef_blocks);
    status[b] |= flags;
  }
  return DOD_OK;
}

extern "C" int dod_jpeg_entropy_device(const uint8_t* bytes, int64_t nbytes, const int64_t* images, int n_images, const int64_t* intervals,
                                       int n_intervals, const int32_t* htabs, int n_htabs, int16_t* coef, int64_t coef_blocks,
                                       int32_t* status, void* stream) {
  if (!bytes || !images || !intervals || !htabs || !coef || !status) return dod_fail(DOD_ERR_INVALID, "dod_jpeg_entropy_device: null argument");
  if (nbytes < 0 || n_images < 1 || n_intervals < 1 || n_htabs < 1 || coef_blocks < 1) return dod_fail(DOD_ERR_INVALID, "dod_jpeg_entropy_device: negative nbytes, or n_images / n_intervals / n_htabs / coef_blocks below 1");
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((n_intervals + 63) / 64), dim3(64), 0, (hipStream_t)stream, bytes, images, intervals,
                     n_intervals, n_images, htabs, n_htabs, coef, coef_blocks, nbytes, status);
  return dod_launched("dod_jpeg_entropy_device");
}

extern "C" int dod_jpeg_idct(const int16_t* coef, int64_t n_blocks, const int64_t* comps, int n_comps, const uint16_t* qtabs, int n_qtabs,
                             uint8_t* planes, void* stream) {
  if (!coef || !comps || !qtabs || !planes || n_blocks < 1 || n_comps < 1 || n_qtabs < 1) return dod_fail(DOD_ERR_INVALID, "dod_jpeg_idct: null argument, or n_blocks / n_comps / n_qtabs below 1");
  if ((reinterpret_cast<uintptr_t>(coef) & 15) || (reinterpret_cast<uintptr_t>(qtabs) & 15) || (reinterpret_cast<uintptr_t>(planes) & 7)) return dod_fail(DOD_ERR_INVALID, "dod_jpeg_idct: coef or qtabs not 16-byte aligned, or planes not 8-byte aligned");
  const int64_t groups = (n_blocks + JI_BLOCKS - 1) / JI_BLOCKS;
  if (groups > 0x7fffffff) return dod_fail(DOD_ERR_INVALID, "dod_jpeg_idct: n_blocks = %lld beyond the grid range", (long long)n_blocks);
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)groups), dim3(JI_BLOCKS * 8), 0, (hipStream_t)stream, coef, n_blocks, comps, n_comps,
                     qtabs, n_qtabs, planes);
  return dod_launched("dod_jpeg_idct");
}

extern "C" int dod_jpeg_color(const uint8_t* planes, const int64_t* images, int n_images, int64_t n_items, uint8_t* out, void* stream) {
  if (!planes || !images || !out || n_images < 1 || n_items < 1) return dod_fail(DOD_ERR_INVALID, "dod_jpeg_color: null argument, or n_images / n_items below 1");
  if (reinterpret_cast<uintptr_t>(planes) & 3) return dod_fail(DOD_ERR_INVALID, "dod_jpeg_color: planes not 4-byte aligned");
  const int64_t groups = (n_items + JC_THREADS - 1) / JC_THREADS;
  if (groups > 0x7fffffff) return dod_fail(DOD_ERR_INVALID, "dod_jpeg_color: n_items = %lld beyond the grid range", (long long)n_items);
  hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)groups), dim3(JC_THREADS), 0, (hipStream_t)stream, planes, images, n_images, n_items, out);
  return dod_launched("dod_jpeg_color");
}
