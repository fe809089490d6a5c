// Hungarian assignment on device: scipy.optimize.linear_sum_assignment (Crouse's shortest augmenting path,
// scipy/optimize/rectangular_lsap/rectangular_lsap.cpp) for every image of the batch in one launch, on the cost buffer
// dod_match_cost writes.  The result is bit-identical to scipy's, ties included: the solver performs the same double-precision
// additions, subtractions and comparisons in the same order on the same values (the fp32 costs widened to double, as scipy
// widens them).  There are no products, so FMA contraction cannot change a result; this file is built without fast-math.
//
// One workgroup of one wave64 per image.  Per augmenting row `cur` (DESIGN.md section 6b states the algorithm):
//   scan    lanes split the remaining columns by position: r = ((minVal + c(i,j)) - u[i]) - v[j] relaxes spc[j] / path[j]
//   argmin  a wave reduction over (spc, free, position) that selects what scipy's serial test
//           `spc[j] < lowest || (spc[j] == lowest && row4col[j] == -1)` selects: the LAST free position of the minimum if
//           there is one, else the FIRST position of the minimum (positions index `remaining`, not columns)
//   step    lane 0 removes that position from `remaining` (the other lanes track the same uniform scalars)
//   duals   lanes update u / v in parallel; augment on lane 0
// The per-image state (u, v, spc in double; path, col4row, row4col, remaining in int32; SR, SC as bytes) lives in LDS when
// it fits and in the caller's workspace otherwise; both regions are sized by rows + columns = Q + n_b, so no size limit
// beyond scipy's own is imposed.  Every loop is bounded by the column count.
#include "dod_common.h"
#include "../../include/dinodet.h"

namespace {

constexpr int kUnitBytes = 32;            // per (row + column) of an image: 3 doubles, 4 int32, 2 flag bytes = 29 <= 32
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

__global__ __launch_bounds__(DOD_WAVE) void match_assign_kernel(const float* __restrict__ cost, const int* __restrict__ gt_offsets,
                                                                 int Q, int G, const long long* __restrict__ labels, int C,
                                                                 int* __restrict__ match, int* __restrict__ status,
                                                                 unsigned char* __restrict__ workspace) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kLdsBytes];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int off = gt_offsets[b], n = gt_offsets[b + 1] - off;
  int* row = match + (size_t)b * Q;
  int st = 0;
  if (off < 0 || n < 0 || off > G - n) {
    st = 1;                                  // malformed offsets: nothing of this image is read
  } else if (n > 0) {
    int bad = 0;
    if (labels)
      for (int k = lane; k < n; k += DOD_WAVE) bad |= labels[off + k] < 0 || labels[off + k] >= C;
    if (__syncthreads_or(bad)) {
      st = 3;
    } else {
      const float* c = cost + (size_t)off * Q;
      bad = 0;
      for (long k = lane; k < (long)n * Q; k += DOD_WAVE) {
        const float x = c[k];
        bad |= x != x || x == -__builtin_inff();
      }
      if (__syncthreads_or(bad)) st = 1;
    }
  }
  if (st != 0 || n == 0) {
    for (int q = lane; q < Q; q += DOD_WAVE) row[q] = -1;
    if (lane == 0) status[b] = st;
    return;
  }
  const float* c = cost + (size_t)off * Q;
  const bool tr = n < Q;                     // scipy solves the transpose when columns < rows
  const int nr = tr ? n : Q, nc = tr ? Q : n;
  const int units = Q + n;
  Lsap s;
  if (units <= kLdsUnits) {
    s = lsap_carve(lds, nr, nc);
    st = lsap_solve(s, c, n, tr, nr, nc);
  } else {
    s = lsap_carve(workspace + ((size_t)b * Q + off) * kUnitBytes, nr, nc);
    st = lsap_solve(s, c, n, tr, nr, nc);
  }
  // match row: query q -> off + target, or -1
  if (st != 0) {
    for (int q = lane; q < Q; q += DOD_WAVE) row[q] = -1;
  } else if (tr) {                           // columns are queries
    for (int q = lane; q < Q; q += DOD_WAVE) row[q] = s.row4col[q] < 0 ? -1 : off + s.row4col[q];
  } else {                                   // rows are queries, every one matched (Q <= n)
    for (int q = lane; q < Q; q += DOD_WAVE) row[q] = off + s.col4row[q];
  }
  if (lane == 0) status[b] = st;
}

}  // namespace

extern "C" size_t dod_match_assign_workspace_bytes(int B, int Q, int G) {
  if (B <= 0 || Q <= 0 || G < 0) return 0;
  return ((size_t)B * Q + (size_t)G) * kUnitBytes;
}

extern "C" int dod_match_assign(const float* cost, const int32_t* gt_offsets, int B, int Q, int G, const int64_t* labels, int C,
                                int32_t* match, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  if (!gt_offsets || !match || !status || B <= 0 || Q <= 0 || G < 0 || (labels && C <= 0)) return DOD_ERR_INVALID;
  if (G > 0 && !cost) return DOD_ERR_INVALID;
  if (!workspace || workspace_bytes < dod_match_assign_workspace_bytes(B, Q, G)) return DOD_ERR_STATE;
  hipLaunchKernelGGL(match_assign_kernel, dim3((unsigned)B), dim3(DOD_WAVE), 0, (hipStream_t)stream, cost, gt_offsets, Q, G,
                     (const long long*)labels, C, match, status, (unsigned char*)workspace);
  return hipGetLastError() == hipSuccess ? DOD_OK : DOD_ERR_HIP;
}
