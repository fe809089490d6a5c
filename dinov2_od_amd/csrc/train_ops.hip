// Kernels of the native training step and their launchers (train_internal.h): dropout RNG, deterministic-mode reductions, pointwise
// adjoints, LayerNorm backward, batched-GEMM attention, the deformable-gather adjoint, LoRA rank-r products, the fp32 linears -- and the
// dod_op_* operator entry points, thin wrappers over exactly these launchers.  Linear backward runs on the fp32 MFMA GEMM of the forward in
// its k-major-operand form (gemm_f32.hip, launch_gemm_f32x): dX = dY W reads W as the k-major operand, dW += dY^T X reads both operands
// k-major with the row dimension split over the grid (atomic accumulate) -- no transposed copies.  Dropout masks come from a counter-based
// hash of (seed, site, element): the backward regenerates them, nothing but activations is taped.
#include "train_internal.h"

#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <string>

namespace dtrain {

// one launch of 256-thread workgroups: 0, or 3 when the HIP runtime refused it
template <class K, class... A> static int launch256(K kernel, dim3 grid, hipStream_t s, A... args) {
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, args...);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

// ------------------------------------------------------------------------------------------------ RNG
__device__ __forceinline__ float u01(unsigned long long key, unsigned long long idx) {
  unsigned long long z = key + idx * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (float)(z >> 40) * (1.0f / 16777216.0f);
}

// ------------------------------------------------------------------------------------------------ deterministic mode
// DINODET_DETERMINISTIC=1 (or the test option "deterministic"): every reduction that the fast step spreads over workgroups and merges with
// fp32 atomics -- K-split weight / activation gradient products, bias column sums, LayerNorm and LoRA parameter gradients, the scatter of
// the deformable sampling adjoint and its shared reference-logit columns -- runs in a FIXED order instead: run-to-run bit-identical
// gradients (the fast step agrees with itself to ~1e-6: r3_t8.log), at roughly twice the step time.
bool det_mode() {
  const int o = dod_option(DOD_OPT_DETERMINISTIC);
  if (o >= 0) return o != 0;
  static const bool env = [] { const char* v = getenv("DINODET_DETERMINISTIC"); return v && v[0] == '1'; }();
  return env;
}
// partial-sum scratch of the ordered reductions (per device, grown on demand; the training step is never stream-captured)
static float* det_scratch(size_t floats) {
  static std::mutex mu;
  static float* buf[16] = {};
  static size_t cap[16] = {};
  const int dev = current_device_slot();
  if (dev < 0) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  if (cap[dev] < floats) {
    if (buf[dev]) { (void)hipDeviceSynchronize(); (void)hipFree(buf[dev]); buf[dev] = nullptr; cap[dev] = 0; }
    if (hipMalloc((void**)&buf[dev], floats * 4) != hipSuccess) return nullptr;
    cap[dev] = floats;
  }
  return buf[dev];
}
// dst[c] += part[0][c] + part[1][c] + ... in that order (part: [nparts][cols])
__global__ void ordered_add_kernel(const float* __restrict__ part, int nparts, int stride, int cols, float* __restrict__ dst) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  float acc = 0.f;
  for (int i = 0; i < nparts; ++i) acc += part[(size_t)i * stride + c];
  dst[c] += acc;
}

// ------------------------------------------------------------------------------------------------ small kernels
// dst[c] += sum_r src[r][c]
__global__ void colsum_kernel(const float* __restrict__ src, int ld, int rows, int cols, float* __restrict__ dst) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int w = threadIdx.x >> 6;
  float acc = 0.f;
  if (c < cols)
    for (int r = blockIdx.y * 4 + w; r < rows; r += gridDim.y * 4) acc += src[(size_t)r * ld + c];
  __shared__ float red[4][64];
  red[w][threadIdx.x & 63] = acc;
  __syncthreads();
  if (w == 0 && c < cols) atomicAdd(dst + c, red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
}
int colsum_add(const float* src, int ld, int rows, int cols, float* dst, hipStream_t s) {
  int gy = (rows + 63) / 64; gy = gy < 1 ? 1 : (gy > 128 ? 128 : gy);
  if (det_mode()) gy = 1;      // one workgroup per 64 columns walks every row: a single adder per column
  return launch256(colsum_kernel, dim3((cols + 63) / 64, gy), s, src, ld, rows, cols, dst);
}

// workgroups of a grid-stride pointwise kernel: one per 256 elements up to the launcher's cap
static unsigned pw_blocks(size_t n, size_t cap) { const size_t b = (n + 255) / 256; return (unsigned)(b < cap ? b : cap); }

// out = a + keep(b) / (1 - p)   (p == 0: plain add); also used with a == nullptr (out = dropped b)
__global__ void dropout_add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, size_t n,
                                   float p, unsigned long long key) {
  const float inv = 1.0f / (1.0f - p);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float v = b[i];
    if (p > 0.f) v = u01(key, i) >= p ? v * inv : 0.f;
    out[i] = a ? a[i] + v : v;
  }
}
int dropout_add(const float* a, const float* b, float* out, size_t n, float p, unsigned long long key, hipStream_t s) { return launch256(dropout_add_kernel, dim3(pw_blocks(n, 2048)), s, a, b, out, n, p, key); }
// g = dy * (y > 0 ? 1 : 0) [* dropout mask / (1 - p)]
__global__ void relu_drop_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ g, size_t n, float p,
                                     unsigned long long key) {
  const float inv = 1.0f / (1.0f - p);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float v = dy[i];
    if (p > 0.f) v = u01(key, i) >= p ? v * inv : 0.f;
    g[i] = y[i] > 0.f ? v : 0.f;
  }
}
int relu_drop_bwd(const float* dy, const float* y, float* g, size_t n, float p, unsigned long long key, hipStream_t s) { return launch256(relu_drop_bwd_kernel, dim3(pw_blocks(n, 2048)), s, dy, y, g, n, p, key); }
__global__ void add_inplace_kernel(float* __restrict__ a, const float* __restrict__ b, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) a[i] += b[i];
}
int add_inplace(float* a, const float* b, size_t n, hipStream_t s) { return launch256(add_inplace_kernel, dim3(pw_blocks(n, 2048)), s, a, b, n); }
// dz[r][0..3] = dbox[r][0..3] * s (1 - s), s = the forward's sigmoid output
__global__ void sigmoid_bwd4_kernel(const float* __restrict__ dbox, int ldd, const float* __restrict__ box, int ldb, float* __restrict__ dz, int rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * 4) return;
  const int r = i >> 2, c = i & 3;
  const float sg = box[(size_t)r * ldb + c];
  dz[i] = dbox[(size_t)r * ldd + c] * sg * (1.0f - sg);
}
int sigmoid_bwd4(const float* dbox, int ldd, const float* box, int ldb, float* dz, int rows, hipStream_t s) {
  return launch256(sigmoid_bwd4_kernel, dim3((unsigned)(((size_t)rows * 4 + 255) / 256)), s, dbox, ldd, box, ldb, dz, rows);
}
// exact-erf GELU backward (modeling_dinov2.py:288-296): g = dy * (Phi(x) + x phi(x))
__global__ void gelu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ pre, float* __restrict__ g, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float x = pre[i];
    const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
    const float pdf = 0.39894228040143267794f * expf(-0.5f * x * x);
    g[i] = dy[i] * (cdf + x * pdf);
  }
}
__global__ void gelu_fwd_kernel(const float* __restrict__ pre, float* __restrict__ h, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) h[i] = gelu_erf(pre[i]);
}
int gelu_fwd(const float* pre, float* h, size_t n, hipStream_t s) { return launch256(gelu_fwd_kernel, dim3(pw_blocks(n, 4096)), s, pre, h, n); }
int gelu_bwd(const float* dy, const float* pre, float* g, size_t n, hipStream_t s) { return launch256(gelu_bwd_kernel, dim3(pw_blocks(n, 4096)), s, dy, pre, g, n); }
// SwiGLU (Dinov2SwiGLUFFN, modeling_dinov2.py:300-314): pre [rows, 2F] = [x1 | x2] -> h = silu(x1) * x2
__global__ void swiglu_fwd_kernel(const float* __restrict__ pre, float* __restrict__ h, size_t rows, int F) {
  const size_t n = rows * (size_t)F;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / F; const int c = (int)(i - r * F);
    const float x1 = pre[r * 2 * F + c], x2 = pre[r * 2 * F + F + c];
    h[i] = x1 / (1.0f + expf(-x1)) * x2;
  }
}
// its adjoint: d(x1) = dh x2 s (1 + x1 (1 - s)), d(x2) = dh x1 s, s = sigmoid(x1); written as [d(x1) | d(x2)] rows of 2F
__global__ void swiglu_bwd_kernel(const float* __restrict__ dh, const float* __restrict__ pre, float* __restrict__ dpre, size_t rows, int F) {
  const size_t n = rows * (size_t)F;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / F; const int c = (int)(i - r * F);
    const float x1 = pre[r * 2 * F + c], x2 = pre[r * 2 * F + F + c], g = dh[i];
    const float sg = 1.0f / (1.0f + expf(-x1));
    dpre[r * 2 * F + c] = g * x2 * sg * (1.0f + x1 * (1.0f - sg));
    dpre[r * 2 * F + F + c] = g * x1 * sg;
  }
}
int swiglu_fwd(const float* pre, float* h, size_t rows, int F, hipStream_t s) { return launch256(swiglu_fwd_kernel, dim3(pw_blocks(rows * (size_t)F, 4096)), s, pre, h, rows, F); }
int swiglu_bwd(const float* dh, const float* pre, float* dpre, size_t rows, int F, hipStream_t s) { return launch256(swiglu_bwd_kernel, dim3(pw_blocks(rows * (size_t)F, 4096)), s, dh, pre, dpre, rows, F); }
// out[i] = a[i] * v[i % D]   (LayerScale on the gradient)
__global__ void colscale_kernel(const float* __restrict__ a, const float* __restrict__ v, float* __restrict__ out, size_t n, int D) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = a[i] * v[i % D];
}
int colscale(const float* a, const float* v, float* out, size_t n, int D, hipStream_t s) { return launch256(colscale_kernel, dim3(pw_blocks(n, 4096)), s, a, v, out, n, D); }
// dq[q][:] += sum_b d[b][q][:]
__global__ void batch_sum_kernel(const float* __restrict__ d, float* __restrict__ dq, int B, size_t per) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < per; i += (size_t)gridDim.x * blockDim.x) {
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc += d[(size_t)b * per + i];
    dq[i] += acc;
  }
}
int batch_sum(const float* d, float* dq, int B, size_t per, hipStream_t s) { return launch256(batch_sum_kernel, dim3((unsigned)((per + 255) / 256)), s, d, dq, B, per); }

// ------------------------------------------------------------------------------------------------ LayerNorm backward
// x: the pre-norm input (t = residual + branch), dy: gradient of the LayerNorm output.  dx per row; dgamma / dbeta accumulated
// per wave over its rows, then one float atomic per column and wave.
template <int MAXC>       // 64-column chunks per lane: 16 (D <= 1024) or 32 (D <= 2048: ViT-g's 1536)
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ dy,
                                                     float eps, int rows, int D, float* __restrict__ dx, float* __restrict__ dgamma,
                                                     float* __restrict__ dbeta, float* __restrict__ part, int nacc) {
  const int lane = threadIdx.x & 63, wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
  float dg[MAXC], db[MAXC];
#pragma unroll
  for (int c = 0; c < MAXC; ++c) { dg[c] = 0.f; db[c] = 0.f; }
  for (int r = wave; r < rows; r += nwaves) {
    const float* xr = x + (size_t)r * D;
    const float* dyr = dy + (size_t)r * D;
    float xv[MAXC], gv[MAXC];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) { const int k = c * 64 + lane; xv[c] = k < D ? xr[k] : 0.f; s += xv[c]; }
    const float mu = wave_sum(s) / (float)D;
    float v = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) { const int k = c * 64 + lane; const float d = k < D ? xv[c] - mu : 0.f; v += d * d; }
    const float rstd = rsqrtf(wave_sum(v) / (float)D + eps);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const int k = c * 64 + lane;
      if (k < D) {
        const float xh = (xv[c] - mu) * rstd, d = dyr[k];
        gv[c] = d * gamma[k];
        xv[c] = xh;
        s1 += gv[c]; s2 += gv[c] * xh;
        dg[c] += d * xh; db[c] += d;
      } else { gv[c] = 0.f; xv[c] = 0.f; }
    }
    s1 = wave_sum(s1) / (float)D; s2 = wave_sum(s2) / (float)D;
    float* dxr = dx + (size_t)r * D;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) { const int k = c * 64 + lane; if (k < D) dxr[k] = rstd * (gv[c] - s1 - xv[c] * s2); }
  }
  // the workgroup's four waves reduce their parameter-gradient partials in LDS: one atomic per column per workgroup
  __shared__ float sg[4][MAXC * 64], sb[4][MAXC * 64];
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) { sg[w][c * 64 + lane] = dg[c]; sb[w][c * 64 + lane] = db[c]; }
  __syncthreads();
  for (int k = threadIdx.x; k < D; k += 256) {
    const float g_ = (sg[0][k] + sg[1][k]) + (sg[2][k] + sg[3][k]), b_ = (sb[0][k] + sb[1][k]) + (sb[2][k] + sb[3][k]);
    if (part && !nacc) { part[((size_t)blockIdx.x * 2) * D + k] = g_; part[((size_t)blockIdx.x * 2 + 1) * D + k] = b_; }      // deterministic mode: merged in block order
    else if (part) { const size_t a = (size_t)(blockIdx.x % nacc) * 2; atomicAdd(part + a * D + k, g_); atomicAdd(part + (a + 1) * D + k, b_); }
    else { atomicAdd(dgamma + k, g_); atomicAdd(dbeta + k, b_); }
  }
}
#define LN_ACC 16            // interleaved accumulators of the fast mode's parameter gradients ...
#define LN_ACC_FROM 512      // ... from this many workgroups (2 048 rows) up: below, the chain is short and the two extra launches would show
int ln_bwd(const float* x, const float* gamma, const float* dy, float eps, int rows, int D, float* dx, float* dgamma, float* dbeta, hipStream_t s) {
  if (D > 2048) return 2;
  int blocks = (rows + 3) / 4; blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);      // one row per wave up to 8 192 rows
  float* part = nullptr;
  int nacc = 0;
  if (det_mode()) {
    blocks = blocks > 256 ? 256 : blocks;
    part = det_scratch((size_t)blocks * 2 * D);
    if (!part) return 3;
  } else if (blocks > LN_ACC_FROM) {
    // A float atomic per column and workgroup straight into dgamma / dbeta is a chain of `blocks` roundings at the size of the running sum: at
    // 2 048 workgroups its random walk reaches 1-2e-6 of the largest column, in an order that changes from run to run.  Long chains go through
    // LN_ACC interleaved accumulators instead (workgroup b adds into accumulator b % LN_ACC: chains and sums 1 / LN_ACC as long), merged in order.
    nacc = LN_ACC;
    part = det_scratch((size_t)nacc * 2 * D);
    if (!part) return 3;
    if (hipMemsetAsync(part, 0, (size_t)nacc * 2 * D * 4, s) != hipSuccess) return 3;
  }
  if (D <= 1024) hipLaunchKernelGGL(ln_bwd_kernel<16>, dim3(blocks), dim3(256), 0, s, x, gamma, dy, eps, rows, D, dx, dgamma, dbeta, part, nacc);
  else hipLaunchKernelGGL(ln_bwd_kernel<32>, dim3(blocks), dim3(256), 0, s, x, gamma, dy, eps, rows, D, dx, dgamma, dbeta, part, nacc);
  if (part) {      // part rows alternate (dgamma, dbeta) per block / accumulator: two strided ordered sums
    const int np = nacc ? nacc : blocks;
    hipLaunchKernelGGL(ordered_add_kernel, dim3((D + 255) / 256), dim3(256), 0, s, part, np, 2 * D, D, dgamma);
    hipLaunchKernelGGL(ordered_add_kernel, dim3((D + 255) / 256), dim3(256), 0, s, part + D, np, 2 * D, D, dbeta);
  }
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

// ------------------------------------------------------------------------------------------------ multi-head self-attention (Q x Q)
// nn.MultiheadAttention (deformable_attention.py:195, 233): softmax((q k^T) / sqrt(dh)), dropout on the probabilities, times v.
// qkv [B*Q, 3*Dd] = [q | k | v], head h at columns h*dh.  Scores, probabilities and their adjoints are [B*Hd, Q, Qp] fp32 scratch
// (Qp = Q rounded up to 4); every product is one batched fp32-MFMA GEMM over (image, head) on strided views of qkv / dO / dqkv, a chunk of images per pass:
//   forward : S = scale q k^T  ->  row kernel: Pd = dropout(softmax(S))  ->  O = Pd v
//   backward: S = scale q k^T, dP = dO v^T  ->  row kernel: Pd, dS = P (keep dP - sum_j keep dP P)
//             ->  dq = scale dS k,  dk = scale dS^T q,  dv = Pd^T dO
// (Round 2 first ran one wave per query row on the VALU -- 2.2 ms per ViT-B block backward at 16 x 257 tokens, every wave
// re-reading K and V from L2 -- and an LDS-resident workgroup per (image, head), which was 2x slower still: 192 workgroups of four
// waves left each SIMD one latency-bound wave.)
#define MHA_RT (MHA_MAXQ / 64)

// one wave per score row; item = (b*Hd + h)*Q + i is also the dropout counter base (mask element = item*Q + j)
__global__ __launch_bounds__(256) void mha_softmax_fwd_kernel(float* __restrict__ S, int Q, int Qp, long nrows, long item_base, float p,
                                                              unsigned long long key) {
  const int lane = threadIdx.x & 63;
  const long local = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (local >= nrows) return;
  const long item = item_base + local;            // rows of an image chunk; the dropout counter runs over the whole batch
  float* row = S + (size_t)local * Qp;
  float v[MHA_RT];
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < MHA_RT; ++t) { const int j = lane + 64 * t; v[t] = j < Q ? row[j] : -INFINITY; mx = fmaxf(mx, v[t]); }
  mx = wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < MHA_RT; ++t) { const int j = lane + 64 * t; v[t] = j < Q ? expf(v[t] - mx) : 0.f; sum += v[t]; }
  sum = wave_sum(sum);
  const float inv = 1.0f / sum, invk = 1.0f / (1.0f - p);
#pragma unroll
  for (int t = 0; t < MHA_RT; ++t) {
    const int j = lane + 64 * t;
    if (j < Qp) {
      float o = v[t] * inv;
      if (p > 0.f && j < Q) o = u01(key, (unsigned long long)item * Q + j) >= p ? o * invk : 0.f;
      row[j] = j < Q ? o : 0.f;
    }
  }
}
// SP: scores in, dropped probabilities out;  DD: d(loss)/d(dropped probabilities) in, d(loss)/d(scores) out
__global__ __launch_bounds__(256) void mha_softmax_bwd_kernel(float* __restrict__ SP, float* __restrict__ DD, int Q, int Qp, long nrows, long item_base,
                                                              float p, unsigned long long key) {
  const int lane = threadIdx.x & 63;
  const long local = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (local >= nrows) return;
  const long item = item_base + local;
  float* srow = SP + (size_t)local * Qp;
  float* drow = DD + (size_t)local * Qp;
  float v[MHA_RT], g[MHA_RT];
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < MHA_RT; ++t) { const int j = lane + 64 * t; v[t] = j < Q ? srow[j] : -INFINITY; g[t] = j < Q ? drow[j] : 0.f; mx = fmaxf(mx, v[t]); }
  mx = wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < MHA_RT; ++t) { const int j = lane + 64 * t; v[t] = j < Q ? expf(v[t] - mx) : 0.f; sum += v[t]; }
  sum = wave_sum(sum);
  const float inv = 1.0f / sum, invk = 1.0f / (1.0f - p);
  float dot = 0.f;
#pragma unroll
  for (int t = 0; t < MHA_RT; ++t) {
    const int j = lane + 64 * t;
    v[t] *= inv;
    float keepf = 1.0f;
    if (p > 0.f && j < Q) keepf = u01(key, (unsigned long long)item * Q + j) >= p ? invk : 0.f;
    g[t] *= keepf;                         // d(loss) / d(P_ij) through the dropout
    dot += g[t] * v[t];
    if (j < Qp) srow[j] = j < Q ? v[t] * keepf : 0.f;
  }
  dot = wave_sum(dot);
#pragma unroll
  for (int t = 0; t < MHA_RT; ++t) {
    const int j = lane + 64 * t;
    if (j < Qp) drow[j] = j < Q ? v[t] * (g[t] - dot) : 0.f;
  }
}

// batched product over z = (image, head); operands are strided views: per-image stride, per-head stride
GemmF32X mha_gemm(const float* A, int lda, long long a_sb, long long a_sh, bool a_km, const float* W, int ldw, long long w_sb, long long w_sh, bool w_km,
                  float* C, int ldc, long long c_sb, long long c_sh, int M, int N, int K, int B, int Hd, float alpha) {
  GemmF32X g; memset(&g, 0, sizeof g);
  g.A = A; g.lda = lda; g.a_sb = a_sb; g.a_sh = a_sh; g.a_kmajor = a_km;
  g.W = W; g.ldw = ldw; g.w_sb = w_sb; g.w_sh = w_sh; g.w_kmajor = w_km;
  g.C = C; g.ldc = ldc; g.c_sb = c_sb; g.c_sh = c_sh;
  g.M = M; g.N = N; g.K = K; g.batch = B * Hd; g.hb = Hd; g.alpha = alpha; g.ksplit = 1;
  return g;
}
// General (rectangular) form: queries q [B*Lq, ldq], keys / values k, v [B*Lk, ldkv] (head h at columns h*dh of each), Lk <= MHA_MAXQ.
// The decoder's self-attention passes q | k | v of one packed buffer (Lq = Lk = Q); the dense cross-attention of the
// nn.TransformerDecoder branch (detr_decoder.py:28-35) passes Lq = Q queries against the Lk = N memory tokens.
// S: mha_scratch_floats(B, Hd, Lq, Lk) of scratch
int launch_mha_fwd_rect(const float* q, int ldq, const float* k, const float* v, int ldkv, float* out, int ldo, float* S, int B, int Lq, int Lk,
                               int Hd, int dh, float scale, float p, unsigned long long key, hipStream_t s) {
  if (Lk > MHA_MAXQ) return 2;
  const int Lkp = (int)up4((size_t)Lk);
  const long long qs = (long long)Lq * ldq, ks = (long long)Lk * ldkv, ss = (long long)Lq * Lkp;
  const int cb = mha_chunk_images(B, Hd, Lq, Lk);
  for (int b0 = 0; b0 < B; b0 += cb) {
    const int nb = B - b0 < cb ? B - b0 : cb;
    const float* q0 = q + (size_t)b0 * qs;
    const float* k0 = k + (size_t)b0 * ks;
    const float* v0 = v + (size_t)b0 * ks;
    int rc = launch_gemm_f32x(mha_gemm(q0, ldq, qs, dh, false, k0, ldkv, ks, dh, false, S, Lkp, ss * Hd, ss, Lq, Lk, dh, nb, Hd, scale), s);
    if (rc) return rc;
    const long nrows = (long)nb * Hd * Lq;
    hipLaunchKernelGGL(mha_softmax_fwd_kernel, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, s, S, Lk, Lkp, nrows, (long)b0 * Hd * Lq, p, key);
    if (hipGetLastError() != hipSuccess) return 3;
    rc = launch_gemm_f32x(mha_gemm(S, Lkp, ss * Hd, ss, false, v0, ldkv, ks, dh, true, out + (size_t)b0 * Lq * ldo, ldo, (long long)Lq * ldo, dh, Lq, dh, Lk,
                                   nb, Hd, 1.0f), s);
    if (rc) return rc;
  }
  return 0;
}
// dS, Pd: mha_scratch_floats(B, Hd, Lq, Lk) of scratch each; dq [B*Lq, lddq], dk, dv [B*Lk, lddkv] are WRITTEN (not accumulated)
int launch_mha_bwd_rect(const float* q, int ldq, const float* k, const float* v, int ldkv, const float* dO, int ldo, float* dq, int lddq, float* dk,
                               float* dv, int lddkv, float* dS, float* Pd, int B, int Lq, int Lk, int Hd, int dh, float scale, float p,
                               unsigned long long key, hipStream_t s) {
  if (Lk > MHA_MAXQ) return 2;
  const int Lkp = (int)up4((size_t)Lk);
  const long long qs = (long long)Lq * ldq, ks = (long long)Lk * ldkv, os = (long long)Lq * ldo, ss = (long long)Lq * Lkp;
  const long long dqs = (long long)Lq * lddq, dks = (long long)Lk * lddkv;
  const int cb = mha_chunk_images(B, Hd, Lq, Lk);
  for (int b0 = 0; b0 < B; b0 += cb) {
    const int nb = B - b0 < cb ? B - b0 : cb;
    const float* q0 = q + (size_t)b0 * qs;
    const float* k0 = k + (size_t)b0 * ks;
    const float* v0 = v + (size_t)b0 * ks;
    const float* o0 = dO + (size_t)b0 * os;
    int rc = launch_gemm_f32x(mha_gemm(q0, ldq, qs, dh, false, k0, ldkv, ks, dh, false, Pd, Lkp, ss * Hd, ss, Lq, Lk, dh, nb, Hd, scale), s);
    if (rc) return rc;
    rc = launch_gemm_f32x(mha_gemm(o0, ldo, os, dh, false, v0, ldkv, ks, dh, false, dS, Lkp, ss * Hd, ss, Lq, Lk, dh, nb, Hd, 1.0f), s);
    if (rc) return rc;
    const long nrows = (long)nb * Hd * Lq;
    hipLaunchKernelGGL(mha_softmax_bwd_kernel, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, s, Pd, dS, Lk, Lkp, nrows, (long)b0 * Hd * Lq, p, key);
    if (hipGetLastError() != hipSuccess) return 3;
    // dq = scale dS k;  dk = scale dS^T q;  dv = Pd^T dO      (k, q, dO enter as the k-major operand: [token, dh] views)
    rc = launch_gemm_f32x(mha_gemm(dS, Lkp, ss * Hd, ss, false, k0, ldkv, ks, dh, true, dq + (size_t)b0 * dqs, lddq, dqs, dh, Lq, dh, Lk, nb, Hd, scale), s);
    if (rc) return rc;
    rc = launch_gemm_f32x(mha_gemm(dS, Lkp, ss * Hd, ss, true, q0, ldq, qs, dh, true, dk + (size_t)b0 * dks, lddkv, dks, dh, Lk, dh, Lq, nb, Hd, scale), s);
    if (rc) return rc;
    rc = launch_gemm_f32x(mha_gemm(Pd, Lkp, ss * Hd, ss, true, o0, ldo, os, dh, true, dv + (size_t)b0 * dks, lddkv, dks, dh, Lk, dh, Lq, nb, Hd, 1.0f), s);
    if (rc) return rc;
  }
  return 0;
}
// ------------------------------------------------------------------------------------------------ deformable gather backward
// Adjoint of deform_sample_kernel (deform.hip; deformable_attention.py:101-174).  One wave per (b, q, head), lanes along dh.
// dproj must be zero on entry (the two reference-logit columns are shared by all heads: float atomics); dvalues accumulates.
// DET (deterministic mode): no scatter and no atomics here -- the value gradient comes from deform_bwd_values_det_kernel (a gather in a
// fixed order), the heads' contributions to the two shared reference-logit columns go to dref_part [B*Q*Hd][2] and are summed head by head.
template <bool DET>
__global__ __launch_bounds__(256) void deform_bwd_kernel(const float* __restrict__ proj, int ldp, const float* __restrict__ values,
                                                         const float* __restrict__ dout, int B, int Q, int N, int Hd, int P, int dh, int h,
                                                         int w, float* __restrict__ dproj, float* __restrict__ dvalues, float* __restrict__ dref_part) {
  const int lane = threadIdx.x & 63;
  const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= (long)B * Q * Hd) return;
  const int hd = (int)(item % Hd);
  const long bq = item / Hd;
  const int b = (int)(bq / Q);
  const float* pr = proj + (size_t)bq * ldp;
  float* dpr = dproj + (size_t)bq * ldp;
  const float refx = sigmoidf_(pr[0]), refy = sigmoidf_(pr[1]);
  const float* off = pr + 2 + hd * P * 2;
  const float* awl = pr + 2 + Hd * P * 2 + hd * P;
  float mx = -INFINITY;
  for (int p = 0; p < P; ++p) mx = fmaxf(mx, awl[p]);
  float aw[8], den = 0.f;
#pragma unroll
  for (int p = 0; p < 8; ++p) { aw[p] = p < P ? expf(awl[p] - mx) : 0.f; den += aw[p]; }
  const int Dd = Hd * dh;
  const float* vb = values + (size_t)b * N * Dd + hd * dh;
  float* dvb = dvalues + (size_t)b * N * Dd + hd * dh;
  const float* g = dout + (size_t)bq * Dd + hd * dh;
  const bool d0ok = lane < dh, d1ok = lane + 64 < dh;
  const float g0 = d0ok ? g[lane] : 0.f, g1 = d1ok ? g[lane + 64] : 0.f;
  float da[8];
  float drefx = 0.f, drefy = 0.f;
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    da[p] = 0.f;
    if (p < P) {
      const float sx = refx + off[2 * p], sy = refy + off[2 * p + 1];
      float lx = fminf(fmaxf(sx, 0.f), 1.f), ly = fminf(fmaxf(sy, 0.f), 1.f);
      lx = lx * (float)(w - 1);
      ly = ly * (float)(h - 1);
      int x0 = (int)floorf(lx), y0 = (int)floorf(ly);
      int x1 = x0 + 1, y1 = y0 + 1;
      x0 = min(max(x0, 0), w - 1); x1 = min(max(x1, 0), w - 1);
      y0 = min(max(y0, 0), h - 1); y1 = min(max(y1, 0), h - 1);
      const float wx1 = lx - (float)x0, wx0 = 1.0f - wx1;
      const float wy1 = ly - (float)y0, wy0 = 1.0f - wy1;
      const float a = aw[p] / den;
      const size_t i00 = (size_t)(y0 * w + x0) * Dd, i01 = (size_t)(y1 * w + x0) * Dd, i10 = (size_t)(y0 * w + x1) * Dd, i11 = (size_t)(y1 * w + x1) * Dd;
      // <g, V_c> per corner
      float p00 = 0.f, p01 = 0.f, p10 = 0.f, p11 = 0.f;
      if (d0ok) { p00 += g0 * vb[i00 + lane]; p01 += g0 * vb[i01 + lane]; p10 += g0 * vb[i10 + lane]; p11 += g0 * vb[i11 + lane]; }
      if (d1ok) { p00 += g1 * vb[i00 + lane + 64]; p01 += g1 * vb[i01 + lane + 64]; p10 += g1 * vb[i10 + lane + 64]; p11 += g1 * vb[i11 + lane + 64]; }
      p00 = wave_sum(p00); p01 = wave_sum(p01); p10 = wave_sum(p10); p11 = wave_sum(p11);
      const float w00 = wx0 * wy0, w01 = wx0 * wy1, w10 = wx1 * wy0, w11 = wx1 * wy1;
      da[p] = p00 * w00 + p01 * w01 + p10 * w10 + p11 * w11;      // d out / d a_p
      // corner scatter: dV_c += a w_c g
      if (!DET && d0ok) {
        atomicAdd(dvb + i00 + lane, a * w00 * g0); atomicAdd(dvb + i01 + lane, a * w01 * g0);
        atomicAdd(dvb + i10 + lane, a * w10 * g0); atomicAdd(dvb + i11 + lane, a * w11 * g0);
      }
      if (!DET && d1ok) {
        atomicAdd(dvb + i00 + lane + 64, a * w00 * g1); atomicAdd(dvb + i01 + lane + 64, a * w01 * g1);
        atomicAdd(dvb + i10 + lane + 64, a * w10 * g1); atomicAdd(dvb + i11 + lane + 64, a * w11 * g1);
      }
      // bilinear weights -> pixel coordinates -> normalised location (clamp passes the gradient inside [0, 1] inclusive)
      const float dwx0 = a * (p00 * wy0 + p01 * wy1), dwx1 = a * (p10 * wy0 + p11 * wy1);
      const float dwy0 = a * (p00 * wx0 + p10 * wx1), dwy1 = a * (p01 * wx0 + p11 * wx1);
      float dsx = (dwx1 - dwx0) * (float)(w - 1), dsy = (dwy1 - dwy0) * (float)(h - 1);
      if (!(sx >= 0.f && sx <= 1.f)) dsx = 0.f;
      if (!(sy >= 0.f && sy <= 1.f)) dsy = 0.f;
      if (lane == 0) { dpr[2 + hd * P * 2 + 2 * p] = dsx; dpr[2 + hd * P * 2 + 2 * p + 1] = dsy; }
      drefx += dsx; drefy += dsy;
    }
  }
  // point-weight softmax backward
  float dotp = 0.f;
#pragma unroll
  for (int p = 0; p < 8; ++p) if (p < P) dotp += (aw[p] / den) * da[p];
  if (lane == 0) {
#pragma unroll
    for (int p = 0; p < 8; ++p) if (p < P) dpr[2 + Hd * P * 2 + hd * P + p] = (aw[p] / den) * (da[p] - dotp);
    if (DET) {
      dref_part[item * 2] = drefx * refx * (1.0f - refx);
      dref_part[item * 2 + 1] = drefy * refy * (1.0f - refy);
    } else {
      atomicAdd(dpr + 0, drefx * refx * (1.0f - refx));        // sigmoid of the reference logits
      atomicAdd(dpr + 1, drefy * refy * (1.0f - refy));
    }
  }
}
// deterministic mode: dproj[bq][0..1] = sum over heads, in head order, of dref_part
__global__ void deform_dref_det_kernel(const float* __restrict__ dref_part, int BQ, int Hd, int ldp, float* __restrict__ dproj) {
  const int bq = blockIdx.x * 256 + threadIdx.x;
  if (bq >= BQ) return;
  float ax = 0.f, ay = 0.f;
  for (int hd = 0; hd < Hd; ++hd) { ax += dref_part[((size_t)bq * Hd + hd) * 2]; ay += dref_part[((size_t)bq * Hd + hd) * 2 + 1]; }
  dproj[(size_t)bq * ldp] += ax;
  dproj[(size_t)bq * ldp + 1] += ay;
}
// deterministic mode: the adjoint of the bilinear gather as a GATHER -- one wave per (image, token, head) walks the image's Q x P samples
// in order (lanes along the samples: each recomputes its sample's corners as deform_bwd_kernel does and keeps its weight on THIS token),
// then adds the matching samples' a w g rows in ascending (q, p) order.  One writer per dvalues row: no atomics, a fixed order.
__global__ __launch_bounds__(256) void deform_bwd_values_det_kernel(const float* __restrict__ proj, int ldp, const float* __restrict__ dout, int B, int Q, int N,
                                                                    int Hd, int P, int dh, int h, int w, float* __restrict__ dvalues) {
  const int lane = threadIdx.x & 63;
  const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= (long)B * N * Hd) return;
  const int hd = (int)(item % Hd);
  const long bn = item / Hd;
  const int b = (int)(bn / N), n = (int)(bn % N);
  const int Dd = Hd * dh, QP = Q * P;
  float acc0 = 0.f, acc1 = 0.f;
  for (int s0 = 0; s0 < QP; s0 += 64) {
    const int sidx = s0 + lane;
    float wt = 0.f;
    if (sidx < QP) {
      const int q = sidx / P, p = sidx - q * P;
      const float* pr = proj + ((size_t)b * Q + q) * ldp;
      const float refx = sigmoidf_(pr[0]), refy = sigmoidf_(pr[1]);
      const float* awl = pr + 2 + Hd * P * 2 + hd * P;
      float mx = -INFINITY;
      for (int pp = 0; pp < P; ++pp) mx = fmaxf(mx, awl[pp]);
      float den = 0.f;                                            // the same 8-slot sum as deform_bwd_kernel
#pragma unroll
      for (int pp = 0; pp < 8; ++pp) den += pp < P ? expf(awl[pp] - mx) : 0.f;
      const float a = expf(awl[p] - mx) / den;
      const float* off = pr + 2 + hd * P * 2;
      const float sx = refx + off[2 * p], sy = refy + off[2 * p + 1];
      float lx = fminf(fmaxf(sx, 0.f), 1.f), ly = fminf(fmaxf(sy, 0.f), 1.f);
      lx = lx * (float)(w - 1);
      ly = ly * (float)(h - 1);
      int x0 = (int)floorf(lx), y0 = (int)floorf(ly);
      int x1 = x0 + 1, y1 = y0 + 1;
      x0 = min(max(x0, 0), w - 1); x1 = min(max(x1, 0), w - 1);
      y0 = min(max(y0, 0), h - 1); y1 = min(max(y1, 0), h - 1);
      const float wx1 = lx - (float)x0, wx0 = 1.0f - wx1;
      const float wy1 = ly - (float)y0, wy0 = 1.0f - wy1;
      // corners in the scatter kernel's order 00, 01, 10, 11 (clamped corners may coincide: their weights add, as their atomics did)
      if (y0 * w + x0 == n) wt += a * (wx0 * wy0);
      if (y1 * w + x0 == n) wt += a * (wx0 * wy1);
      if (y0 * w + x1 == n) wt += a * (wx1 * wy0);
      if (y1 * w + x1 == n) wt += a * (wx1 * wy1);
    }
    unsigned long long hit = __ballot(wt != 0.f);
    while (hit) {
      const int l = __ffsll((long long)hit) - 1;
      hit &= hit - 1;
      const float wl = __shfl(wt, l, 64);
      const int q = (s0 + l) / P;
      const float* g = dout + ((size_t)b * Q + q) * Dd + hd * dh;
      if (lane < dh) acc0 = fmaf(wl, g[lane], acc0);
      if (lane + 64 < dh) acc1 = fmaf(wl, g[lane + 64], acc1);
    }
  }
  float* dv = dvalues + ((size_t)b * N + n) * Dd + hd * dh;
  if (lane < dh) dv[lane] += acc0;
  if (lane + 64 < dh) dv[lane + 64] += acc1;
}

// dproj zero on entry, dvalues accumulated; the scatter kernel, or in deterministic mode the three ordered ones.  Returns a dod_status.
int launch_deform_bwd(const float* proj, int ldp, const float* values, const float* dout, int B, int Q, int N, int Hd, int P, int dh, int h, int w,
                      float* dproj, float* dvalues, hipStream_t s) {
  const int BQ = B * Q;
  if (det_mode()) {
    float* dref_part = det_scratch((size_t)BQ * Hd * 2);
    if (!dref_part) return dod_fail(DOD_ERR_HIP, "deterministic mode: scratch allocation failed");
    hipLaunchKernelGGL(deform_bwd_kernel<true>, dim3((unsigned)(((long)BQ * Hd + 3) / 4)), dim3(256), 0, s, proj, ldp, values, dout, B, Q, N, Hd, P, dh, h, w,
                       dproj, dvalues, dref_part);
    hipLaunchKernelGGL(deform_dref_det_kernel, dim3((BQ + 255) / 256), dim3(256), 0, s, dref_part, BQ, Hd, ldp, dproj);
    hipLaunchKernelGGL(deform_bwd_values_det_kernel, dim3((unsigned)(((long)B * N * Hd + 3) / 4)), dim3(256), 0, s, proj, ldp, dout, B, Q, N, Hd, P, dh, h, w,
                       dvalues);
  } else {
    hipLaunchKernelGGL(deform_bwd_kernel<false>, dim3((unsigned)(((long)BQ * Hd + 3) / 4)), dim3(256), 0, s, proj, ldp, values, dout, B, Q, N, Hd, P, dh, h, w,
                       dproj, dvalues, nullptr);
  }
  TH(hipGetLastError());
  return DOD_OK;
}

// ------------------------------------------------------------------------------------------------ linears
// K slices for a product whose 64x64 tiles leave most of the chip idle (the decoder's 1 600-row linears: 300 tiles, a lone
// workgroup's 16-k tile takes ~1 us): target ~768 workgroups of at least 8 k-tiles each; 1 = do not split.  The split kernel's k-tile is 32.
int ksplit_for(int rows, int cols, int K, Mm mm) {
  if (det_mode()) return 1;      // one workgroup owns an output tile: no atomic merge of K slices
  static const int target = [] { const char* e = DOD_TUNE_ENV("DINODET_F32_KSPLIT_WGS"); return e && atoi(e) > 0 ? atoi(e) : 768; }();
  const int tiles = ((rows + 63) / 64) * ((cols + 63) / 64), nkt = mm == MM_X3 ? (K + 31) / 32 : (K + 15) / 16;
  if (tiles >= target) return 1;
  int ks = (target + tiles - 1) / tiles;
  const int cap = nkt / 8 > 1 ? nkt / 8 : 1;
  return ks > cap ? cap : ks;
}
inline int xlaunch(const GemmF32X& g, Mm mm, hipStream_t s) { return mm == MM_X3 ? launch_gemm_f32x3(g, s) : launch_gemm_f32x(g, s); }
// Y[M,N] = act(X[M,K] W[N,K]^T + b) (* scale) (+ resid).  Never K-split: the forward stays a bit-reproducible function of (inputs, seed).
int lin_fwd(const float* X, int ldx, const float* W, const float* b, int M, int N, int K, float* Y, int ldy, int act, Mm mm, hipStream_t s,
            const float* scale, const float* resid, int ldr) {
  if (mm == MM_X3) {
    GemmF32X g = xgemm(X, ldx, false, W, K, false, Y, ldy, M, N, K, 1.0f, false);
    g.bias = b; g.act = act; g.scale = scale; g.resid = resid; g.ldr = ldr;
    return launch_gemm_f32x3(g, s);
  }
  GemmEpi e = gepi(b, Y, ldy, act, resid, ldr); e.scale = scale;
  return launch_gemm_f32(X, ldx, W, K, M, N, K, e, s);
}
// dX[M,K] (+)= dY[M,N] W[N,K]: W [N, K] is the k-major operand of the product over n
int lin_bwd_x(const float* dY, int ldy, const float* W, int M, int N, int K, float* dX, bool accumulate, Mm mm, hipStream_t s) {
  GemmF32X g = xgemm(dY, ldy, false, W, K, true, dX, K, M, K, N, 1.0f, accumulate);
  g.ksplit = ksplit_for(M, K, N, mm);
  if (g.ksplit > 1 && !accumulate) {
    if (hipMemsetAsync(dX, 0, (size_t)M * K * 4, s) != hipSuccess) return 3;
    g.accumulate = 1;
  }
  return xlaunch(g, mm, s);
}
// C[R,Cc] += alpha * Y[M,R]^T X[M,Cc]: both operands k-major over the M rows.  A small output (weight gradients: a few dozen to
// a few hundred tiles against a reduction over thousands of rows) splits the rows over grid.z and accumulates atomically.
int gemm_tn_acc(const float* Y, int ldy, const float* X, int ldx, int M, int R, int Cc, float* C, int ldc, float alpha, Mm mm, hipStream_t s) {
  GemmF32X g = xgemm(Y, ldy, true, X, ldx, true, C, ldc, R, Cc, M, alpha, true);
  g.ksplit = ksplit_for(R, Cc, M, mm);
  return xlaunch(g, mm, s);
}
// dW[N,K] += dY[M,N]^T X[M,K];  db[N] += colsum(dY)
int lin_bwd_w(const float* dY, int ldy, const float* X, int ldx, int M, int N, int K, float* dW, float* db, Mm mm, hipStream_t s) {
  int r = gemm_tn_acc(dY, ldy, X, ldx, M, N, K, dW, K, 1.0f, mm, s);
  if (r) return r;
  return db ? colsum_add(dY, ldy, M, N, db, s) : 0;
}

// ------------------------------------------------------------------------------------------------ LoRA
// Rank-r products of a LoRA pair, r <= 8 (the reference trains r = 2: dinov2_backbone.py:47-51): both are bound by reading the
// [M, features] activation once, which a 64x64-tile GEMM with r useful columns cannot do (12 workgroups walking 4 112 rows: 115 us).
//   down: T[m, c] = alpha * sum_k X[m, k] * A(c, k)            one wave per row, lanes along k;   A(c, k) = A[c * sa_c + k * sa_k]
//   up  : G(o, c) += sum_m Y[m, o] * T[m, c]                   one thread per column o, 64 rows per workgroup, atomic accumulate
#define LORA_RMAX 8
#define LORA_UP_ROWS 64
__global__ __launch_bounds__(256) void lora_down_kernel(const float* __restrict__ X, int ldx, const float* __restrict__ A, int sa_c, int sa_k, int M, int K,
                                                        int r, float alpha, float* __restrict__ T, int ldt) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const float* x = X + (size_t)m * ldx;
  float acc[LORA_RMAX];
#pragma unroll
  for (int c = 0; c < LORA_RMAX; ++c) acc[c] = 0.f;
#pragma unroll 4
  for (int k = lane; k < K; k += 64) {
    const float xv = x[k];
    const float* ak = A + (size_t)k * sa_k;
#pragma unroll
    for (int c = 0; c < LORA_RMAX; ++c)
      if (c < r) acc[c] = fmaf(xv, ak[(size_t)c * sa_c], acc[c]);
  }
#pragma unroll
  for (int c = 0; c < LORA_RMAX; ++c) {
    if (c < r) {
      const float v = wave_sum(acc[c]);
      if (lane == 0) T[(size_t)m * ldt + c] = alpha * v;
    }
  }
}
__global__ __launch_bounds__(256) void lora_up_kernel(const float* __restrict__ Y, int ldy, const float* __restrict__ T, int ldt, int M, int O, int r,
                                                      float* __restrict__ G, int sg_o, int sg_c) {
  __shared__ float sT[LORA_UP_ROWS][LORA_RMAX];
  const int o = blockIdx.x * 256 + threadIdx.x;
  float acc[LORA_RMAX];
#pragma unroll
  for (int c = 0; c < LORA_RMAX; ++c) acc[c] = 0.f;
  // a workgroup walks the row chunks blockIdx.y, blockIdx.y + gridDim.y, ...: gridDim.y = 1 (deterministic mode) makes it the only adder
  for (int m0 = blockIdx.y * LORA_UP_ROWS; m0 < M; m0 += gridDim.y * LORA_UP_ROWS) {
    const int nm = M - m0 < LORA_UP_ROWS ? M - m0 : LORA_UP_ROWS;
    __syncthreads();
    for (int i = threadIdx.x; i < LORA_UP_ROWS * LORA_RMAX; i += 256) {
      const int mm = i / LORA_RMAX, c = i % LORA_RMAX;
      sT[mm][c] = (mm < nm && c < r) ? T[(size_t)(m0 + mm) * ldt + c] : 0.f;
    }
    __syncthreads();
    if (o < O) {
      const float* y = Y + (size_t)m0 * ldy + o;
      for (int mm = 0; mm < nm; ++mm) {
        const float yv = y[(size_t)mm * ldy];
#pragma unroll
        for (int c = 0; c < LORA_RMAX; ++c) acc[c] = fmaf(yv, sT[mm][c], acc[c]);
      }
    }
  }
  if (o >= O) return;
#pragma unroll
  for (int c = 0; c < LORA_RMAX; ++c)
    if (c < r) unsafeAtomicAdd(G + (size_t)o * sg_o + (size_t)c * sg_c, acc[c]);
}
int lora_down(const float* X, int ldx, const float* A, int sa_c, int sa_k, int M, int K, int r, float alpha, float* T, int ldt, hipStream_t s) {
  return launch256(lora_down_kernel, dim3((M + 3) / 4), s, X, ldx, A, sa_c, sa_k, M, K, r, alpha, T, ldt);
}
int lora_up(const float* Y, int ldy, const float* T, int ldt, int M, int O, int r, float* G, int sg_o, int sg_c, hipStream_t s) {
  return launch256(lora_up_kernel, dim3((O + 255) / 256, det_mode() ? 1 : (M + LORA_UP_ROWS - 1) / LORA_UP_ROWS), s, Y, ldy, T, ldt, M, O, r, G, sg_o, sg_c);
}

// gradients of one LoRA pair for out = X W'^T: dB [out, r] += alpha dY^T (X A^T), dA [r, in] += alpha (dY B)^T X
int lora_grads(const float* X, int in_f, const float* dY, int ldy, int out_f, const float* A, const float* Bm, int M, int r, float alpha, float* dA, float* dB,
               float* T, float* U, hipStream_t s) {
  if (!dA || !dB) return 0;
  const int rp = (int)up4(r);
  int rc;
  if (r <= LORA_RMAX) {
    rc = lora_down(X, in_f, A, in_f, 1, M, in_f, r, alpha, T, rp, s); if (rc) return rc;            // T = alpha X A^T   [M, r]
    rc = lora_up(dY, ldy, T, rp, M, out_f, r, dB, r, 1, s); if (rc) return rc;                        // dB += dY^T T
    rc = lora_down(dY, ldy, Bm, 1, r, M, out_f, r, alpha, U, rp, s); if (rc) return rc;             // U = alpha dY B    [M, r]
    return lora_up(X, in_f, U, rp, M, in_f, r, dA, 1, in_f, s);                                       // dA += U^T X
  }
  rc = launch_gemm_f32x(xgemm(X, in_f, false, A, in_f, false, T, rp, M, r, in_f, alpha, false), s); if (rc) return rc;
  rc = gemm_tn_acc(dY, ldy, T, rp, M, out_f, r, dB, r, 1.0f, MM_F32, s); if (rc) return rc;
  rc = launch_gemm_f32x(xgemm(dY, ldy, false, Bm, r, true, U, rp, M, r, out_f, alpha, false), s); if (rc) return rc;
  return gemm_tn_acc(U, rp, X, in_f, M, r, in_f, dA, in_f, 1.0f, MM_F32, s);
}

}  // namespace dtrain

// =============================================================================================================================
// Operator entry points of the training kernels (include/dinodet.h "training-step operators"): each validates its arguments and calls
// the launcher the step itself calls, so a test reaches every adjoint kernel on its own, at shapes the three steps never run.
using namespace dtrain;

namespace {
inline size_t attn_vjp_ws(int B, int Lq, int Lk, int heads, int form) {
  if (form == 0) return 2 * al256(mha_scratch_floats(B, heads, Lq, Lk) * 4);                    // scores / probabilities, adjoint
  return al256((size_t)2 * B * heads * Lq * 4) + al256((size_t)B * heads * Lq * 4);             // (max, sum) per row, delta
}
inline bool attn_vjp_shape_ok(int B, int Lq, int Lk, int heads, int dh, int form) {
  if (B <= 0 || Lq <= 0 || Lk <= 0 || heads <= 0 || dh <= 0 || dh > 128 || dh % 4) return false;
  return form == 0 ? Lk <= MHA_MAXQ : (form == 1 && dh == 64);
}
}  // namespace

extern "C" {

int dod_op_layernorm_bwd(const float* x, const float* gamma, const float* dy, float eps, int rows, int D, float* dx, float* dgamma, float* dbeta,
                         void* stream) {
  if (!x || !gamma || !dy || !dx || !dgamma || !dbeta) OPFAIL("dod_op_layernorm_bwd: null buffer");
  if (rows <= 0 || D <= 0 || D > 2048) OPFAIL("dod_op_layernorm_bwd: rows=%d D=%d outside rows >= 1, 1 <= D <= 2048", rows, D);
  TK(ln_bwd(x, gamma, dy, eps, rows, D, dx, dgamma, dbeta, (hipStream_t)stream));
  return DOD_OK;
}

size_t dod_op_attention_f32_vjp_workspace_bytes(int B, int Lq, int Lk, int heads, int dh, int form) {
  return attn_vjp_shape_ok(B, Lq, Lk, heads, dh, form) ? attn_vjp_ws(B, Lq, Lk, heads, form) + 256 : 0;
}
int dod_op_attention_f32_vjp(const float* q, int ldq, const float* k, const float* v, int ldkv, const float* d_o, float* o, int ldo, float* dq, int lddq,
                             float* dk, float* dv, int lddkv, int B, int Lq, int Lk, int heads, int dh, float scale, int form, float dropout_p,
                             uint64_t key, void* workspace, size_t workspace_bytes, void* stream) {
  if (!q || !k || !v || !d_o || !o || !dq || !dk || !dv || !workspace) OPFAIL("dod_op_attention_f32_vjp: null buffer");
  if (form != 0 && form != 1) OPFAIL("dod_op_attention_f32_vjp: form %d (0 = batched GEMMs, 1 = flash)", form);
  if (!attn_vjp_shape_ok(B, Lq, Lk, heads, dh, form))
    OPFAIL("dod_op_attention_f32_vjp: B=%d Lq=%d Lk=%d heads=%d head_dim=%d not taken by form %d (head_dim <= 128, a multiple of 4; form 0: Lk <= %d; form 1: head_dim 64)",
           B, Lq, Lk, heads, dh, form, MHA_MAXQ);
  const int Dm = heads * dh;
  if (ldq < Dm || ldkv < Dm || ldo < Dm || lddq < Dm || lddkv < Dm || (ldq | ldkv | ldo | lddq | lddkv) % 4)
    OPFAIL("dod_op_attention_f32_vjp: every pitch must be a multiple of 4 and at least heads * head_dim = %d", Dm);
  if (dropout_p < 0.f || dropout_p >= 1.f || (form == 1 && dropout_p != 0.f)) OPFAIL("dod_op_attention_f32_vjp: dropout %g (form 0: [0, 1); form 1: 0)", dropout_p);
  if (workspace_bytes < attn_vjp_ws(B, Lq, Lk, heads, form) + 256) return dod_fail(DOD_ERR_STATE, "dod_op_attention_f32_vjp: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  dod::Carver c = carver(workspace);
  if (form == 0) {
    float* Pd = takef(c, mha_scratch_floats(B, heads, Lq, Lk));
    float* dS = takef(c, mha_scratch_floats(B, heads, Lq, Lk));
    TK(launch_mha_fwd_rect(q, ldq, k, v, ldkv, o, ldo, Pd, B, Lq, Lk, heads, dh, scale, dropout_p, key, s));
    TK(launch_mha_bwd_rect(q, ldq, k, v, ldkv, d_o, ldo, dq, lddq, dk, dv, lddkv, dS, Pd, B, Lq, Lk, heads, dh, scale, dropout_p, key, s));
    return DOD_OK;
  }
  float* lse = takef(c, (size_t)2 * B * heads * Lq);
  float* delta = takef(c, (size_t)B * heads * Lq);
  AttnF32 a; a.q = q; a.k = k; a.v = v; a.o = o; a.ldq = ldq; a.ldk = a.ldv = ldkv; a.ldo = ldo;
  a.Lq = Lq; a.Lk = Lk; a.B = B; a.heads = heads; a.dh = dh; a.scale = scale; a.lse = lse;
  TK(launch_attn_f32(a, s));
  AttnF32Bwd g;
  g.q = q; g.k = k; g.v = v; g.o = o; g.d_o = d_o; g.lse = lse; g.dq = dq; g.dk = dk; g.dv = dv; g.delta = delta;
  g.ldq = ldq; g.ldk = g.ldv = ldkv; g.ldo = ldo; g.lddq = lddq; g.lddk = g.lddv = lddkv;
  g.Lq = Lq; g.Lk = Lk; g.B = B; g.heads = heads; g.dh = dh; g.scale = scale;
  TK(launch_attn_f32_bwd(g, s));
  return DOD_OK;
}

int dod_op_deform_sample_bwd(const float* proj, int ldp, const float* values, const float* dout, int B, int Q, int N, int Hd, int P, int dh, int hh, int ww,
                             float* dproj, float* dvalues, void* stream) {
  if (!proj || !values || !dout || !dproj || !dvalues) OPFAIL("dod_op_deform_sample_bwd: null buffer");
  if (B <= 0 || Q <= 0 || N <= 0 || Hd <= 0 || P < 1 || P > 8 || dh <= 0 || dh > 128)
    OPFAIL("dod_op_deform_sample_bwd: B=%d Q=%d N=%d heads=%d points=%d head_dim=%d outside 1 <= points <= 8, 1 <= head_dim <= 128", B, Q, N, Hd, P, dh);
  if (hh <= 0 || ww <= 0 || hh * ww != N) OPFAIL("dod_op_deform_sample_bwd: a %dx%d feature map does not hold %d tokens", hh, ww, N);
  if (ldp < 2 + 3 * Hd * P) OPFAIL("dod_op_deform_sample_bwd: pitch %d below the %d columns of [ref | offsets | weights]", ldp, 2 + 3 * Hd * P);
  hipStream_t s = (hipStream_t)stream;
  TH(hipMemsetAsync(dproj, 0, (size_t)B * Q * ldp * 4, s));
  return launch_deform_bwd(proj, ldp, values, dout, B, Q, N, Hd, P, dh, hh, ww, dproj, dvalues, s);
}

size_t dod_op_lora_grads_workspace_bytes(int M, int r) {
  return M > 0 && r >= 1 && r <= 64 ? 2 * al256((size_t)M * up4(r) * 4) + 256 : 0;
}
int dod_op_lora_grads(const float* X, int in_f, const float* dY, int ldy, int out_f, const float* A, const float* Bm, int M, int r, float alpha, float* dA,
                      float* dB, void* workspace, size_t workspace_bytes, void* stream) {
  if (!X || !dY || !A || !Bm || !dA || !dB || !workspace) OPFAIL("dod_op_lora_grads: null buffer");
  if (r < 1 || r > 64) OPFAIL("dod_op_lora_grads: rank %d outside 1..64", r);
  if (M <= 0 || in_f <= 0 || out_f <= 0 || ldy < out_f) OPFAIL("dod_op_lora_grads: M=%d in=%d out=%d ldy=%d", M, in_f, out_f, ldy);
  if (workspace_bytes < dod_op_lora_grads_workspace_bytes(M, r)) return dod_fail(DOD_ERR_STATE, "dod_op_lora_grads: workspace too small");
  dod::Carver c = carver(workspace);
  float* T = takef(c, (size_t)M * up4(r));
  float* U = takef(c, (size_t)M * up4(r));
  TK(lora_grads(X, in_f, dY, ldy, out_f, A, Bm, M, r, alpha, dA, dB, T, U, (hipStream_t)stream));
  return DOD_OK;
}

int dod_op_train_pointwise(int op, const float* a, const float* b, float* out, size_t n, int cols, float p, uint64_t key, void* stream) {
  if (!b || !out || (!a && op != DOD_PW_DROPOUT_ADD)) OPFAIL("dod_op_train_pointwise: null buffer");
  if (n == 0 || p < 0.f || p >= 1.f) OPFAIL("dod_op_train_pointwise: n=%zu p=%g", n, p);
  hipStream_t s = (hipStream_t)stream;
  switch (op) {
    case DOD_PW_GELU_BWD: TK(gelu_bwd(a, b, out, n, s)); break;
    case DOD_PW_SWIGLU_BWD:
      if (cols <= 0) OPFAIL("dod_op_train_pointwise: swiglu_bwd needs cols = F > 0");
      TK(swiglu_bwd(a, b, out, n, cols, s)); break;
    case DOD_PW_RELU_DROP_BWD: TK(relu_drop_bwd(a, b, out, n, p, (unsigned long long)key, s)); break;
    case DOD_PW_DROPOUT_ADD: TK(dropout_add(a, b, out, n, p, (unsigned long long)key, s)); break;
    case DOD_PW_SIGMOID_BWD4:
      if (cols < 4 || n > (size_t)(1 << 29)) OPFAIL("dod_op_train_pointwise: sigmoid_bwd4 needs a pitch cols >= 4 and n <= 2^29 rows");
      TK(sigmoid_bwd4(a, cols, b, 4, out, (int)n, s)); break;
    default: OPFAIL("dod_op_train_pointwise: unknown op %d", op);
  }
  return DOD_OK;
}

int dod_op_colsum_add(const float* src, int ld, int rows, int cols, float* dst, void* stream) {
  if (!src || !dst) OPFAIL("dod_op_colsum_add: null buffer");
  if (rows <= 0 || cols <= 0 || ld < cols) OPFAIL("dod_op_colsum_add: rows=%d cols=%d ld=%d", rows, cols, ld);
  TK(colsum_add(src, ld, rows, cols, dst, (hipStream_t)stream));
  return DOD_OK;
}

}  // extern "C"
