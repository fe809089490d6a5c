// The GEMM operand row formats the inference path hands from kernel to kernel besides fp32, each stated ONCE: the bf16 split and the byte
// placement of a row.  Producers (GEMM epilogues, LayerNorm / rowstats, the attention epilogues, the split kernels) call these and nothing else,
// so that two producers of one format agree bit for bit -- the tests compare them with dod_op_split_pair / dod_op_split3 / dod_op_split_h2.
//   bf16         plain rows
//   pair         [hi | lo]: the split-product operands (gemm_x3.hip, attn_x3.hip); the lo half starts lo_off columns after the hi half
//   s3           [hi | hi | lo], each section W columns wide: the bf16x3 activation operand of ONE bf16 GEMM with K' = 3K
//   H2           fp16, then per 16-k group the e4m3 main bytes and, 16 bytes on, the e4m3 remainder bytes (dod_common.h "H2")
// A row store takes the row's base, the column (a multiple of the store's width) and the values; the caller knows nothing of the layout.
#pragma once
#include "dod_common.h"

// ---- the split x = hi + lo: hi = bf16_rne(x), lo = bf16_rne(x - hi) (dod_op_split_pair's definition).  The heads come from ONE
// v_cvt_pk_bf16_f32, the remainders from the separately rounded differences x - float(hi): no fma, no reassociation.
// the two bf16 of a dword as floats (low half first)
__device__ __forceinline__ float2 bf16_unpack2(uint32_t u) { return make_float2(__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u)); }
__device__ __forceinline__ float4 bf16_unpack4(uint2 u) {
  const float2 a = bf16_unpack2(u.x), b = bf16_unpack2(u.y);
  return make_float4(a.x, a.y, b.x, b.y);
}
__device__ __forceinline__ void bf16_split1(float x, bf16_t& hi, bf16_t& lo) {
  hi = f2bf(x);
  lo = f2bf(x - bf2f(hi));
}
// the dword of the bf16 remainders of (x, y), given the dword of their heads h = pack2bf(x, y): for the producers that store the heads
// either way and the remainders under a condition (row_store_pair_lo* below; patch_embed.hip, whose bf16x3 kernel at patch 14 takes 260
// instead of 256 registers -- one wave per SIMD instead of two -- when it computes both dwords up front)
__device__ __forceinline__ uint32_t bf16_rem2(float x, float y, uint32_t h) {
  const float2 f = bf16_unpack2(h);
  return pack2bf(x - f.x, y - f.y);
}
// (x, y) -> the dword of their bf16 heads (x in the low half) and the dword of the bf16 remainders
__device__ __forceinline__ void bf16_split2(float x, float y, uint32_t& h, uint32_t& l) {
  h = pack2bf(x, y);
  l = bf16_rem2(x, y, h);
}
__device__ __forceinline__ uint2 bf16_pack4(const float4& v) { return make_uint2(pack2bf(v.x, v.y), pack2bf(v.z, v.w)); }
__device__ __forceinline__ void bf16_split4(const float4& v, uint2& hi, uint2& lo) {
  hi = bf16_pack4(v);
  lo = make_uint2(bf16_rem2(v.x, v.y, hi.x), bf16_rem2(v.z, v.w, hi.y));
}
__device__ __forceinline__ void bf16_split8(const float4& v, const float4& u, uint4& hi, uint4& lo) {
  uint2 h0, h1, l0, l1;
  bf16_split4(v, h0, l0);
  bf16_split4(u, h1, l1);
  hi = make_uint4(h0.x, h0.y, h1.x, h1.y);
  lo = make_uint4(l0.x, l0.y, l1.x, l1.y);
}

// ---- plain bf16 rows.  The stores return the heads they wrote: a pair row is a bf16 row plus its remainder half, and a producer that learns
// at run time which of the two it writes stores the heads once and completes the pair with row_store_pair_lo* -- the GEMM epilogues, which
// then branch around the remainders only.  (Measured on the ViT-B/14 518 forward: a whole store per format under a branch of its own, together
// with a branch on the activation per quad instead of per row, cost the bf16x3 mode 0.5 % and the fp16x2 mode 0.9 % of its images/s.)
__device__ __forceinline__ uint32_t row_store_bf16x2(bf16_t* row, int c, float x, float y) {
  const uint32_t hi = pack2bf(x, y);
  *reinterpret_cast<uint32_t*>(row + c) = hi;
  return hi;
}
__device__ __forceinline__ uint2 row_store_bf16x4(bf16_t* row, int c, const float4& v) {
  const uint2 hi = bf16_pack4(v);
  *reinterpret_cast<uint2*>(row + c) = hi;
  return hi;
}
__device__ __forceinline__ uint4 row_store_bf16x8(bf16_t* row, int c, const float4& v, const float4& u) {
  const uint2 a = bf16_pack4(v), b = bf16_pack4(u);
  const uint4 hi = make_uint4(a.x, a.y, b.x, b.y);
  *reinterpret_cast<uint4*>(row + c) = hi;
  return hi;
}

// ---- pair rows [hi | lo]
__device__ __forceinline__ void row_store_pair1(bf16_t* row, size_t c, size_t lo_off, float x) {
  bf16_t hi, lo;
  bf16_split1(x, hi, lo);
  row[c] = hi;
  row[c + lo_off] = lo;
}
// the remainder half alone, hi = what row_store_bf16x2 / x4 / x8 of the same values returned
__device__ __forceinline__ void row_store_pair_lo2(bf16_t* row, int c, int lo_off, float x, float y, uint32_t hi) {
  *reinterpret_cast<uint32_t*>(row + c + lo_off) = bf16_rem2(x, y, hi);
}
__device__ __forceinline__ void row_store_pair_lo4(bf16_t* row, int c, int lo_off, const float4& v, uint2 hi) {
  *reinterpret_cast<uint2*>(row + c + lo_off) = make_uint2(bf16_rem2(v.x, v.y, hi.x), bf16_rem2(v.z, v.w, hi.y));
}
__device__ __forceinline__ void row_store_pair_lo8(bf16_t* row, int c, int lo_off, const float4& v, const float4& u, uint4 hi) {
  *reinterpret_cast<uint4*>(row + c + lo_off) =
      make_uint4(bf16_rem2(v.x, v.y, hi.x), bf16_rem2(v.z, v.w, hi.y), bf16_rem2(u.x, u.y, hi.z), bf16_rem2(u.z, u.w, hi.w));
}
__device__ __forceinline__ void row_store_pair4(bf16_t* row, int c, int lo_off, const float4& v) {
  row_store_pair_lo4(row, c, lo_off, v, row_store_bf16x4(row, c, v));
}

// ---- bf16x3 activation rows [hi | hi | lo], sections of W columns
__device__ __forceinline__ void row_store_s3x1(bf16_t* row, int c, int W, float x) {
  bf16_t hi, lo;
  bf16_split1(x, hi, lo);
  row[c] = hi;
  row[W + c] = hi;
  row[2 * W + c] = lo;
}
__device__ __forceinline__ void row_store_s3x4(bf16_t* row, int c, int W, const float4& v) {
  uint2 hi, lo;
  bf16_split4(v, hi, lo);
  *reinterpret_cast<uint2*>(row + c) = hi;
  *reinterpret_cast<uint2*>(row + c + W) = hi;
  *reinterpret_cast<uint2*>(row + c + 2 * (size_t)W) = lo;
}

// ---- H2 rows (dod_common.h "H2").  Values are clamped to the fp16 / e4m3 finite ranges.
// four values -> fp16 (2 dwords), e4m3 of the fp16 value times 2^ehi and of the remainder times 2^(ehi + 11) (one dword each)
__device__ __forceinline__ void h2_quad(float4 v, float shi, uint2& f16, unsigned& hi8, unsigned& lo8) {
  v.x = clampf_(v.x, 65504.f); v.y = clampf_(v.y, 65504.f); v.z = clampf_(v.z, 65504.f); v.w = clampf_(v.w, 65504.f);
  const f16x2 p0 = {(_Float16)v.x, (_Float16)v.y}, p1 = {(_Float16)v.z, (_Float16)v.w};
  f16.x = __builtin_bit_cast(unsigned, p0); f16.y = __builtin_bit_cast(unsigned, p1);
  const float hx = (float)p0.x, hy = (float)p0.y, hz = (float)p1.x, hw = (float)p1.y;
  const float slo = shi * 2048.0f;
  hi8 = pack4_fp8(clampf_(hx * shi, 448.f), clampf_(hy * shi, 448.f), clampf_(hz * shi, 448.f), clampf_(hw * shi, 448.f));
  lo8 = pack4_fp8(clampf_((v.x - hx) * slo, 448.f), clampf_((v.y - hy) * slo, 448.f), clampf_((v.z - hz) * slo, 448.f), clampf_((v.w - hw) * slo, 448.f));
}
// byte offset of the e4m3(h) bytes of column c (c % 4 == 0) inside an H2 activation row of K elements; the remainder bytes follow 16 bytes on
__device__ __forceinline__ size_t h2_off8(int K, int c) { return (size_t)2 * K + (size_t)(c >> 4) * 32 + (c & 15); }
// activation row of K elements (4K bytes): four / eight values at column c
__device__ __forceinline__ void row_store_h2x4(void* row, int K, int c, const float4& v) {
  uint2 f16; unsigned hi8, lo8;
  h2_quad(v, 1.0f, f16, hi8, lo8);
  char* r = reinterpret_cast<char*>(row);
  *reinterpret_cast<uint2*>(r + 2 * c) = f16;
  char* p8 = r + h2_off8(K, c);
  *reinterpret_cast<unsigned*>(p8) = hi8;
  *reinterpret_cast<unsigned*>(p8 + 16) = lo8;
}
__device__ __forceinline__ void row_store_h2x8(void* row, int K, int c, const float4& v, const float4& u) {
  uint2 fa, fb; unsigned h0, l0, h1, l1;
  h2_quad(v, 1.0f, fa, h0, l0);
  h2_quad(u, 1.0f, fb, h1, l1);
  char* r = reinterpret_cast<char*>(row);
  *reinterpret_cast<uint4*>(r + 2 * c) = make_uint4(fa.x, fa.y, fb.x, fb.y);
  char* p8 = r + h2_off8(K, c);
  *reinterpret_cast<uint2*>(p8) = make_uint2(h0, h1);
  *reinterpret_cast<uint2*>(p8 + 16) = make_uint2(l0, l1);
}
// weight row of K elements (3K bytes; shi = the row's e4m3 scale 2^e): fp16, then the remainder bytes only
__device__ __forceinline__ void row_store_h2w4(void* row, int K, int c, const float4& v, float shi) {
  uint2 f16; unsigned hi8, lo8;
  h2_quad(v, shi, f16, hi8, lo8);
  char* r = reinterpret_cast<char*>(row);
  *reinterpret_cast<uint2*>(r + 2 * c) = f16;
  *reinterpret_cast<unsigned*>(r + 2 * K + c) = lo8;
}
