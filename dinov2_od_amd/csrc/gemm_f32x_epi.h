// The two epilogues of the GemmF32X products (dod_common.h), shared by the exact-fp32 kernel (gemm_f32.hip gemm_f32x_kernel) and the bf16
// split kernel (gemm_f32x3.hip): v_mfma_f32_32x32x2_f32 and v_mfma_f32_32x32x16_bf16 leave a 32x32 result in the same lanes and registers
// (col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)), and both kernels compute the tile transposed (D = W_tile A_tile^T): a lane
// owns an output row m, its register quads run along n.  Both act on ONE 64x64 tile at (m0, n0) of 256 threads = 2x2 waves of a 32x32
// accumulator each; a wider tile calls them once per 64x64 quadrant.
#pragma once
#include "dod_common.h"

// ---- host side, shared by the two launchers
// 16-byte loads are allowed: aligned base, row pitch and batch strides multiples of four floats
inline bool vec_ok(const void* p, long long ld, long long s1 = 0, long long s2 = 0) {
  return ((uintptr_t)p & 15) == 0 && ld >= 4 && ld % 4 == 0 && s1 % 4 == 0 && s2 % 4 == 0;
}
// Argument check and defaults of a GemmF32X launch (bk = the kernel's k-tile): 0, or the launcher's return code (1: nothing to do, 2: rejected)
inline int f32x_normalize(GemmF32X& g, int bk) {
  if (g.M <= 0 || g.N <= 0 || g.K <= 0 || !g.A || !g.W || !g.C) return 1;
  if (g.batch < 1) g.batch = 1;
  if (g.hb < 1) g.hb = 1;
  if (g.batch % g.hb || g.batch > 65535) return 2;
  if (g.ksplit < 1) g.ksplit = 1;
  if (g.ksplit > 1 && (g.act != ACT_NONE || g.scale || g.resid)) return 2;
  const int nkt = (g.K + bk - 1) / bk;
  if (g.ksplit > nkt) g.ksplit = nkt;
  return 0;
}

// C = alpha acc (+ bias) -> activation (-> * scale[n]) (+ resid) (+ C): every thread stores its own 16 values
__device__ __forceinline__ void f32x_epi_direct(const GemmF32X& g, float* cz, int m0, int n0, const f32x16& acc) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int lr = lane & 31, lh = lane >> 5;
  const int m = m0 + wm * 32 + lr;
  if (m >= g.M) return;
  float* crow = cz + (size_t)m * g.ldc;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int n = n0 + wn * 32 + 8 * q + 4 * lh + t;
      if (n >= g.N) continue;
      float v = acc[4 * q + t] * g.alpha;
      if (g.bias) v += g.bias[n];
      if (g.act == ACT_GELU) v = gelu_erf(v);
      else if (g.act == ACT_RELU) v = fmaxf(v, 0.f);
      else if (g.act == ACT_SIGMOID) v = sigmoidf_(v);
      if (g.scale) v *= g.scale[n];
      if (g.resid) v += g.resid[(size_t)m * g.ldr + n];
      crow[n] = g.accumulate ? crow[n] + v : v;
    }
  }
}

// K slices (g.ksplit > 1): atomic accumulate of the slice's partial tile, staged through LDS so that one wave instruction covers 64 consecutive
// columns of one row (a lane-owns-a-row scatter of 4-byte atomics ran at ~40 per ns: 80 us for a 384 x 768 gradient).  Only slice 0
// (add_bias) adds the bias.  T: [64][65] floats of LDS the main loop no longer needs; every thread of the workgroup calls this.
__device__ __forceinline__ void f32x_epi_atomic(const GemmF32X& g, float* cz, int m0, int n0, const f32x16& acc, float* T, bool add_bias) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int lr = lane & 31, lh = lane >> 5;
  __syncthreads();                                   // every wave is done reading the last stage (or the previous quadrant's T)
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int t = 0; t < 4; ++t) T[(wm * 32 + lr) * 65 + wn * 32 + 8 * q + 4 * lh + t] = acc[4 * q + t] * g.alpha;
  __syncthreads();
  const int n = n0 + lane;
  const float bv = (g.bias && add_bias && n < g.N) ? g.bias[n] : 0.f;
  for (int rr = 0; rr < 16; ++rr) {
    const int row = wid * 16 + rr, m = m0 + row;
    if (m < g.M && n < g.N) unsafeAtomicAdd(cz + (size_t)m * g.ldc + n, T[row * 65 + lane] + bv);
  }
}
