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
#include "lsap.h"

namespace {

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
  if (!gt_offsets || !match || !status || B <= 0 || Q <= 0 || G < 0 || (labels && C <= 0)) return dod_fail(DOD_ERR_INVALID, "dod_match_assign: null offsets / match / status, non-positive B / Q, negative G, or labels with C <= 0");
  if (G > 0 && !cost) return dod_fail(DOD_ERR_INVALID, "dod_match_assign: null cost with G > 0");
  if (!workspace || workspace_bytes < dod_match_assign_workspace_bytes(B, Q, G)) return dod_fail(DOD_ERR_STATE, "dod_match_assign: null or short workspace");
  hipLaunchKernelGGL(match_assign_kernel, dim3((unsigned)B), dim3(DOD_WAVE), 0, (hipStream_t)stream, cost, gt_offsets, Q, G,
                     (const long long*)labels, C, match, status, (unsigned char*)workspace);
  return dod_launched("dod_match_assign");
}
