// The rectangular assignment solver the device kernels share: scipy.optimize.linear_sum_assignment (Crouse's shortest augmenting
// path, scipy/optimize/rectangular_lsap/rectangular_lsap.cpp) for one wave64, bit-identical to scipy's result, ties included: the
// solver performs the same double-precision additions, subtractions and comparisons in the same order on the same values (the fp32
// costs widened to double, as scipy widens them).  There are no products, so FMA contraction cannot change a result.
// assign.hip (one image of the matcher per workgroup) states the algorithm; track.hip (one stream of the tracker per workgroup)
// solves its three association problems with the same function.
#pragma once
#include "dod_common.h"

constexpr int kUnitBytes = 32;            // per (row + column) of a problem: 3 doubles, 4 int32, 2 flag bytes = 29 <= 32
constexpr int kLdsBytes = 48 * 1024;      // LDS state budget of one workgroup
constexpr int kLdsUnits = kLdsBytes / kUnitBytes;

struct Lsap {
  double *u, *v, *spc;
  int *path, *col4row, *row4col, *remaining;
  unsigned char *SR, *SC;
};

__device__ __forceinline__ Lsap lsap_carve(unsigned char* base, int nr, int nc) {
  Lsap s;
  s.u = reinterpret_cast<double*>(base);
  s.v = s.u + nr;
  s.spc = s.v + nc;
  s.path = reinterpret_cast<int*>(s.spc + nc);
  s.col4row = s.path + nc;
  s.row4col = s.col4row + nr;
  s.remaining = s.row4col + nc;
  s.SR = reinterpret_cast<unsigned char*>(s.remaining + nc);
  s.SC = s.SR + nr;
  return s;
}

// the argmin key of one position: smaller spc first; at equal spc a free column first, then among free columns the LATER
// position, among taken ones the EARLIER position -- a total order, so the wave reduction is order-independent
__device__ __forceinline__ bool key_better(double a, int afree, int apos, double b, int bfree, int bpos) {
  if (a < b) return true;
  if (b < a) return false;
  if (afree != bfree) return afree > bfree;
  return afree ? apos > bpos : apos < bpos;
}

// element (i, j) of the oriented matrix: image rows are queries ([Q, n] row-major); transposed, rows are targets
__device__ __forceinline__ double cost_at(const float* __restrict__ c, int i, int j, int n, bool tr) {
  return (double)(tr ? c[(size_t)j * n + i] : c[(size_t)i * n + j]);
}

// Solves one oriented nr x nc problem (nr <= nc).  Returns 0 or 2 (infeasible).  All lanes call it; every branch taken on
// a uniform value.
__device__ __forceinline__ int lsap_solve(const Lsap& s, const float* __restrict__ c, int n, bool tr, int nr, int nc) {
  const int lane = threadIdx.x;
  for (int k = lane; k < nr; k += DOD_WAVE) { s.u[k] = 0.0; s.col4row[k] = -1; }
  for (int k = lane; k < nc; k += DOD_WAVE) { s.v[k] = 0.0; s.row4col[k] = -1; }
  __syncthreads();
  for (int cur = 0; cur < nr; ++cur) {
    // 1. reset the search
    for (int k = lane; k < nr; k += DOD_WAVE) s.SR[k] = 0;
    for (int k = lane; k < nc; k += DOD_WAVE) {
      s.SC[k] = 0;
      s.spc[k] = __builtin_inf();
      s.remaining[k] = nc - 1 - k;
    }
    __syncthreads();
    double minVal = 0.0;
    int num_remaining = nc, i = cur, sink = -1;
    // 2. shortest augmenting path: one column leaves `remaining` per step
    while (sink == -1 && num_remaining > 0) {
      if (lane == 0) s.SR[i] = 1;
      const double ui = s.u[i];
      double best = __builtin_inf();
      int bfree = 0, bpos = 0x7fffffff;
      for (int it = lane; it < num_remaining; it += DOD_WAVE) {
        const int j = s.remaining[it];
        const double r = ((minVal + cost_at(c, i, j, n, tr)) - ui) - s.v[j];
        double sj = s.spc[j];
        if (r < sj) {
          s.path[j] = i;
          s.spc[j] = r;
          sj = r;
        }
        const int fr = s.row4col[j] == -1;
        if (key_better(sj, fr, it, best, bfree, bpos)) { best = sj; bfree = fr; bpos = it; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, DOD_WAVE);
        const int of = __shfl_xor(bfree, o, DOD_WAVE), op = __shfl_xor(bpos, o, DOD_WAVE);
        if (key_better(ob, of, op, best, bfree, bpos)) { best = ob; bfree = of; bpos = op; }
      }
      if (best == __builtin_inf()) return 2;
      minVal = best;
      const int j = s.remaining[bpos];
      if (s.row4col[j] == -1) sink = j;
      else i = s.row4col[j];
      __syncthreads();                      // every lane has read remaining[bpos] before lane 0 overwrites it
      if (lane == 0) {
        s.SC[j] = 1;
        s.remaining[bpos] = s.remaining[num_remaining - 1];
      }
      --num_remaining;
      __syncthreads();
    }
    if (sink == -1) return 2;               // unreachable for nr <= nc; keeps the loop bound explicit
    // 3. duals (u[cur] by itself; the other rows of the tree and the scanned columns in parallel)
    for (int k = lane; k < nr; k += DOD_WAVE)
      if (s.SR[k] && k != cur) s.u[k] = s.u[k] + (minVal - s.spc[s.col4row[k]]);
    for (int k = lane; k < nc; k += DOD_WAVE)
      if (s.SC[k]) s.v[k] = s.v[k] - (minVal - s.spc[k]);
    __syncthreads();
    // 4. augment along the path (lane 0; at most nr rows on it)
    if (lane == 0) {
      s.u[cur] = s.u[cur] + minVal;
      int j = sink;
      for (int k = 0; k <= nr; ++k) {
        const int r = s.path[j];
        s.row4col[j] = r;
        const int t = s.col4row[r];
        s.col4row[r] = j;
        j = t;
        if (r == cur) break;
      }
    }
    __syncthreads();
  }
  return 0;
}
