// The optimizer step of the training loop on device: clip_grad_norm_ followed by Adam (L2 or decoupled weight decay, no amsgrad) over a
// list of fp32 tensors, train.py:1101-1110 of the reference, with an optional exponential moving average of the weights written by the
// thread that stores p' and an optional skip of the whole step on a non-finite norm.  DESIGN.md section 6b states the arithmetic and
// its error bounds.
//
//   sumsq    one workgroup per chunk of one tensor's gradient; squares are accumulated in double from the first add on and every
//            workgroup writes ONE partial sum to a workspace slot of its own.
//   adam     every workgroup first adds up ALL partials in a fixed order (double; a few thousand values, L2 resident), forms the norm and
//            the clip coefficient, then updates its own chunk once: one read of g, p, m, v and one write of p, m, v.
//   scale    the standalone clip: the same reduction, then g *= coef in place.
//   ema      the standalone moving average e += (p - e) w over a list of (e, p) pairs: the arithmetic of the fused form, one launch.
// Tensor descriptors travel BY VALUE in the kernel arguments (gradients are fresh allocations every step: a device table would need a
// staging buffer and an upload per step); a list longer than one table takes several launches.  The workgroup -> (tensor, chunk) map is a
// binary search over a prefix array in the same arguments: wave-uniform, scalar loads only.  No atomics: two runs give the same bits.
#include "dod_internal.h"

#include <atomic>
#include <cstdarg>
#include <cstdio>

namespace {

typedef long long i64;

constexpr int kThreads = 256;
constexpr int kSlots = 4;                                  // float4 per thread and chunk
constexpr int kChunk = kThreads * 4 * kSlots;              // 4096 elements per workgroup
constexpr int kNormT = 128;                                // tensors per sumsq / scale launch   (2.6 KB of arguments)
constexpr int kAdamT = 56;                                 // tensors per adam launch            (3.4 KB of arguments)
constexpr int kEmaT = 96;                                  // tensors per standalone ema launch  (2.7 KB of arguments)
constexpr int kRuns = 4;                                   // runs of equal decoupled decay factors per adam launch
constexpr int kMaxPartials = 4096;                         // sumsq workgroups take several chunks each beyond this many
constexpr int kMaxGrid = 1 << 30;

struct NormArgs {
  float* g[kNormT];
  i64 n[kNormT];
  int first[kNormT + 1];                                   // first workgroup of tensor i; first[nt] = grid size
  int nt;
  int per;                                                 // chunks per workgroup (sumsq), 1 for scale
};
struct AdamTensor { float* p; const float* g; float* m; float* v; float* e; i64 n; float step_size, bc2_sqrt; };      // e: NULL = no average
struct AdamArgs {
  AdamTensor t[kAdamT];
  int first[kAdamT + 1];
  int nt;
};
// w1 = 1 - beta1, w2 = 1 - beta2, formed from the caller's doubles; tensors run_first[r] .. run_first[r + 1] - 1 of the launch multiply p by
// decay[r] = 1 - lr wd before the update (1.0: no decoupled decay); ema_w = 1 - d of the average; skip: a non-finite norm leaves everything alone
struct Hyper { double w1, b2, w2, wd, max_norm, ema_w, decay[kRuns]; float eps; int run_first[kRuns + 1]; int nruns; int skip; };
struct EmaArgs {
  float* e[kEmaT];
  const float* p[kEmaT];
  i64 n[kEmaT];
  int first[kEmaT + 1];
  int nt;
};
static_assert(sizeof(NormArgs) <= 3072 && sizeof(EmaArgs) <= 3072 && sizeof(AdamArgs) + sizeof(Hyper) <= 3584, "kernel arguments stay well inside 4 KB");

// largest i with first[i] <= b: b is blockIdx.x, so the whole search runs on the scalar unit
template <int N> __device__ __forceinline__ int locate(const int (&first)[N], int nt, int b) {
  int lo = 0, hi = nt;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

// sum of s[0 .. 255] in a fixed tree order, the same value in every thread
__device__ __forceinline__ double block_sum(double x, double* s) {
  const int tid = threadIdx.x;
  s[tid] = x;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o) s[tid] += s[tid + o];
    __syncthreads();
  }
  const double r = s[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kThreads) void optim_sumsq_kernel(const NormArgs a, double* __restrict__ partial) {
  __shared__ double s[kThreads];
  const int b = blockIdx.x, t = locate(a.first, a.nt, b), tid = threadIdx.x;
  const float* __restrict__ g = a.g[t];
  const i64 n = a.n[t];
  const i64 span = (i64)a.per * kChunk, lo = (i64)(b - a.first[t]) * span, hi = lo + span < n ? lo + span : n;
  double acc = 0.0;
  if (((uintptr_t)g & 15) == 0) {
    for (i64 base = lo; base < hi; base += kChunk) {
#pragma unroll
      for (int k = 0; k < kSlots; ++k) {
        const i64 e = base + ((i64)k * kThreads + tid) * 4;
        if (e + 4 <= hi) {
          const float4 x = *reinterpret_cast<const float4*>(g + e);
          acc += (double)x.x * x.x; acc += (double)x.y * x.y; acc += (double)x.z * x.z; acc += (double)x.w * x.w;
        } else {
          for (i64 i = e; i < hi; ++i) acc += (double)g[i] * g[i];
        }
      }
    }
  } else {
    for (i64 i = lo + tid; i < hi; i += kThreads) acc += (double)g[i] * g[i];
  }
  const double r = block_sum(acc, s);
  if (tid == 0) partial[b] = r;
}

// norm and clip coefficient from the partial sums.  The norm a caller sees is fp32, as PyTorch's; the coefficient
// min(1, max_norm / (norm + 1e-6)) is formed from the double sum, so the scaled gradient is one rounding away from the exact one.
// A NaN norm gives a NaN coefficient (torch.clamp keeps NaN; fmin would not).
__device__ __forceinline__ double clip_coef(const double* __restrict__ partial, int np, double max_norm, double* s, float* norm_out) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < np; i += kThreads) acc += partial[i];
  const double norm = sqrt(block_sum(acc, s));
  *norm_out = (float)norm;
  const double c = max_norm / (norm + 1e-6);
  return c >= 1.0 ? 1.0 : c;
}

// PyTorch's Adam for one element; g, m and v in double (the fp64 rate is no limit behind 28 bytes of traffic per element), each state
// rounded once when stored; the quotient in fp32 from the stored values.  dec != 1: AdamW's p *= 1 - lr wd comes first, in double, and
// p' is rounded once from p dec - delta (delta the fp32 quotient term); dec == 1 is the fp32 subtraction of the L2 form, bit for bit.
__device__ __forceinline__ void adam1(float graw, float& p, float& m, float& v, double coef, const Hyper& h, double dec, float step_size,
                                      float bc2_sqrt) {
  double g = coef * (double)graw;
  if (h.wd != 0.0) g += h.wd * (double)p;
  const double md = (double)m + (g - (double)m) * h.w1;
  const double vd = h.b2 * (double)v + h.w2 * g * g;
  m = (float)md;
  v = (float)vd;
  const float den = sqrtf(v) / bc2_sqrt + h.eps;
  if (dec == 1.0) {
    p = p - step_size * (m / den);
  } else {
    const float delta = step_size * (m / den);
    p = (float)((double)p * dec - (double)delta);
  }
}

// the moving average of one element from the p just stored: e + (p - e) w in double, every operation rounded by itself (no fused
// multiply-add: torch's float64 operations on the same values give the same bits), the result rounded once to fp32
__device__ __forceinline__ float ema1(float e, float p, double w) {
#pragma clang fp contract(off)
  const double d = ((double)p - (double)e) * w;
  return (float)((double)e + d);
}

__device__ __forceinline__ bool nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// np >= 0: the norm comes from the partial sums (first: workgroup 0 stores it).  np < 0: no clip; with h.skip the norm of an earlier
// dod_optim_clip_grad_norm over the whole list is read from total_norm.  A skipped step returns before any store to p, m, v, e; the
// counter has one writer (thread 0 of workgroup 0 of the first launch): a plain load and store.
template <bool kEma>
__global__ __launch_bounds__(kThreads) void optim_adam_kernel(const AdamArgs a, const Hyper h, const double* __restrict__ partial, int np,
                                                              float* __restrict__ total_norm, int first, int* __restrict__ skipped) {
  __shared__ double s[kThreads];
  const int b = blockIdx.x, t = locate(a.first, a.nt, b), tid = threadIdx.x;
  double coef = 1.0;
  if (np >= 0 || h.skip) {
    float nf;
    if (np >= 0) {
      coef = clip_coef(partial, np, h.max_norm, s, &nf);
      if (first && b == 0 && tid == 0) *total_norm = nf;
    } else {
      nf = *total_norm;
    }
    if (h.skip && nonfinite(nf)) {
      if (first && b == 0 && tid == 0 && skipped) *skipped = *skipped + 1;
      return;
    }
  }
  const AdamTensor T = a.t[t];
  int r = 0;
  while (r + 1 < h.nruns && h.run_first[r + 1] <= t) ++r;
  const double dec = h.decay[r];
  const bool ema = kEma && T.e != nullptr;
  const i64 n = T.n, base = (i64)(b - a.first[t]) * kChunk;
  const bool vec = ((((uintptr_t)T.p) | ((uintptr_t)T.g) | ((uintptr_t)T.m) | ((uintptr_t)T.v) | (ema ? (uintptr_t)T.e : 0)) & 15) == 0;
  if (vec) {
    float4 G[kSlots], P[kSlots], M[kSlots], V[kSlots], E[kEma ? kSlots : 1];
    bool full[kSlots];
#pragma unroll
    for (int k = 0; k < kSlots; ++k) {
      const i64 e = base + ((i64)k * kThreads + tid) * 4;
      full[k] = e + 4 <= n;
      if (full[k]) {
        G[k] = *reinterpret_cast<const float4*>(T.g + e);
        P[k] = *reinterpret_cast<const float4*>(T.p + e);
        M[k] = *reinterpret_cast<const float4*>(T.m + e);
        V[k] = *reinterpret_cast<const float4*>(T.v + e);
        if constexpr (kEma) if (ema) E[k] = *reinterpret_cast<const float4*>(T.e + e);
      }
    }
#pragma unroll
    for (int k = 0; k < kSlots; ++k) {
      const i64 e = base + ((i64)k * kThreads + tid) * 4;
      if (full[k]) {
        adam1(G[k].x, P[k].x, M[k].x, V[k].x, coef, h, dec, T.step_size, T.bc2_sqrt);
        adam1(G[k].y, P[k].y, M[k].y, V[k].y, coef, h, dec, T.step_size, T.bc2_sqrt);
        adam1(G[k].z, P[k].z, M[k].z, V[k].z, coef, h, dec, T.step_size, T.bc2_sqrt);
        adam1(G[k].w, P[k].w, M[k].w, V[k].w, coef, h, dec, T.step_size, T.bc2_sqrt);
        *reinterpret_cast<float4*>(T.p + e) = P[k];
        *reinterpret_cast<float4*>(T.m + e) = M[k];
        *reinterpret_cast<float4*>(T.v + e) = V[k];
        if constexpr (kEma) if (ema) {
          float4 x = E[k];
          x.x = ema1(x.x, P[k].x, h.ema_w); x.y = ema1(x.y, P[k].y, h.ema_w); x.z = ema1(x.z, P[k].z, h.ema_w); x.w = ema1(x.w, P[k].w, h.ema_w);
          *reinterpret_cast<float4*>(T.e + e) = x;
        }
      } else {
        for (i64 i = e; i < n && i < e + 4; ++i) {      // the n mod 4 tail
          float p = T.p[i], m = T.m[i], v = T.v[i];
          adam1(T.g[i], p, m, v, coef, h, dec, T.step_size, T.bc2_sqrt);
          T.p[i] = p; T.m[i] = m; T.v[i] = v;
          if (ema) T.e[i] = ema1(T.e[i], p, h.ema_w);
        }
      }
    }
  } else {
    const i64 hi = base + kChunk < n ? base + kChunk : n;
    for (i64 i = base + tid; i < hi; i += kThreads) {
      float p = T.p[i], m = T.m[i], v = T.v[i];
      adam1(T.g[i], p, m, v, coef, h, dec, T.step_size, T.bc2_sqrt);
      T.p[i] = p; T.m[i] = m; T.v[i] = v;
      if (ema) T.e[i] = ema1(T.e[i], p, h.ema_w);
    }
  }
}

__global__ __launch_bounds__(kThreads) void optim_ema_kernel(const EmaArgs a, double w) {
  const int b = blockIdx.x, t = locate(a.first, a.nt, b), tid = threadIdx.x;
  float* __restrict__ e = a.e[t];
  const float* __restrict__ p = a.p[t];
  const i64 n = a.n[t], base = (i64)(b - a.first[t]) * kChunk, hi = base + kChunk < n ? base + kChunk : n;
  if (((((uintptr_t)e) | ((uintptr_t)p)) & 15) == 0) {
#pragma unroll
    for (int k = 0; k < kSlots; ++k) {
      const i64 i0 = base + ((i64)k * kThreads + tid) * 4;
      if (i0 + 4 <= n) {
        float4 x = *reinterpret_cast<const float4*>(e + i0);
        const float4 y = *reinterpret_cast<const float4*>(p + i0);
        x.x = ema1(x.x, y.x, w); x.y = ema1(x.y, y.y, w); x.z = ema1(x.z, y.z, w); x.w = ema1(x.w, y.w, w);
        *reinterpret_cast<float4*>(e + i0) = x;
      } else {
        for (i64 i = i0; i < n && i < i0 + 4; ++i) e[i] = ema1(e[i], p[i], w);
      }
    }
  } else {
    for (i64 i = base + tid; i < hi; i += kThreads) e[i] = ema1(e[i], p[i], w);
  }
}

__global__ __launch_bounds__(kThreads) void optim_scale_kernel(const NormArgs a, double max_norm, const double* __restrict__ partial, int np,
                                                               float* __restrict__ total_norm, int store_norm) {
  __shared__ double s[kThreads];
  const int b = blockIdx.x, t = locate(a.first, a.nt, b), tid = threadIdx.x;
  float nf;
  const double coef = clip_coef(partial, np, max_norm, s, &nf);
  if (store_norm && b == 0 && tid == 0) *total_norm = nf;
  if (coef >= 1.0) return;                                 // below max_norm: the gradients keep their bits (a NaN coefficient goes on)
  float* __restrict__ g = a.g[t];
  const i64 n = a.n[t], base = (i64)(b - a.first[t]) * kChunk, hi = base + kChunk < n ? base + kChunk : n;
  if (((uintptr_t)g & 15) == 0) {
#pragma unroll
    for (int k = 0; k < kSlots; ++k) {
      const i64 e = base + ((i64)k * kThreads + tid) * 4;
      if (e + 4 <= n) {
        float4 x = *reinterpret_cast<const float4*>(g + e);
        x.x = (float)(coef * x.x); x.y = (float)(coef * x.y); x.z = (float)(coef * x.z); x.w = (float)(coef * x.w);
        *reinterpret_cast<float4*>(g + e) = x;
      } else {
        for (i64 i = e; i < n && i < e + 4; ++i) g[i] = (float)(coef * g[i]);
      }
    }
  } else {
    for (i64 i = base + tid; i < hi; i += kThreads) g[i] = (float)(coef * g[i]);
  }
}

__global__ void optim_store_kernel(float* dst, float value) { *dst = value; }

// ------------------------------------------------------------------------------------------------ host
std::atomic<long> g_launches{0};

inline i64 chunks_of(i64 n, i64 span) { return (n + span - 1) / span; }

// arguments every entry point checks before it touches a device; *total = elements, *nz = tensors with n > 0
int check_list(const char* who, const dod_optim_tensor* t, int nt, bool adam, i64* total) {
  if (nt < 0) return dod_fail(DOD_ERR_INVALID, "%s: n_tensors = %d is negative", who, nt);
  if (nt > 0 && !t) return dod_fail(DOD_ERR_INVALID, "%s: null tensor list", who);
  i64 sum = 0;
  for (int i = 0; i < nt; ++i) {
    if (t[i].n < 0) return dod_fail(DOD_ERR_INVALID, "%s: tensor %d has n = %lld", who, i, (long long)t[i].n);
    if (t[i].n > (i64)kChunk * kMaxGrid) return dod_fail(DOD_ERR_INVALID, "%s: tensor %d has more than 2^42 elements", who, i);
    if (t[i].n > 0 && (!t[i].g || (adam && (!t[i].p || !t[i].m || !t[i].v)))) return dod_fail(DOD_ERR_INVALID, "%s: tensor %d has a null pointer", who, i);
    sum += t[i].n;
  }
  *total = sum;
  return DOD_OK;
}

int launched(const char* who) {
  ++g_launches;
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DOD_OK : dod_fail(DOD_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e));
}

// kernel 1 over the whole list: partial[0 .. *np)
int run_sumsq(const char* who, const dod_optim_tensor* t, int nt, i64 total, double* partial, int* np, hipStream_t s) {
  const int per = (int)chunks_of(chunks_of(total, kChunk) + nt, kMaxPartials);      // 1 up to 16 M elements
  const i64 span = (i64)per * kChunk;
  int done = 0, i = 0;
  while (i < nt) {
    NormArgs a;
    a.nt = 0; a.per = per; a.first[0] = 0;
    for (; i < nt && a.nt < kNormT; ++i) {
      if (t[i].n == 0) continue;
      const i64 c = chunks_of(t[i].n, span);
      if (a.first[a.nt] + c > kMaxGrid) break;
      a.g[a.nt] = t[i].g; a.n[a.nt] = t[i].n; a.first[a.nt + 1] = a.first[a.nt] + (int)c;
      ++a.nt;
    }
    if (!a.nt) continue;
    hipLaunchKernelGGL(optim_sumsq_kernel, dim3(a.first[a.nt]), dim3(kThreads), 0, s, a, partial + done);
    if (int rc = launched(who)) return rc;
    done += a.first[a.nt];
  }
  *np = done;
  return DOD_OK;
}

size_t ws_need(int nt, i64 total) { return ((size_t)chunks_of(total, kChunk) + (size_t)nt) * sizeof(double) + 256; }

int store_norm0(const char* who, float* total_norm_dev, hipStream_t s) {
  hipLaunchKernelGGL(optim_store_kernel, dim3(1), dim3(1), 0, s, total_norm_dev, 0.f);
  return launched(who);
}

// what both update entries run.  ema / decay: lists parallel to t, or NULL
int run_step(const char* who, const dod_optim_tensor* t, float* const* ema, const double* decay, int n_tensors, const dod_optim_options& o,
             void* ws, size_t ws_bytes, hipStream_t s) {
  i64 total = 0;
  if (int rc = check_list(who, t, n_tensors, true, &total)) return rc;
  const bool clip = o.max_norm > 0.f, skip = o.skip_nonfinite != 0, ready = o.norm_ready != 0, norm = clip || (skip && !ready);
  if (ready && (!skip || clip)) return dod_fail(DOD_ERR_INVALID, "%s: norm_ready goes with skip_nonfinite and max_norm <= 0 only", who);
  if ((norm || skip) && !o.total_norm_dev) return dod_fail(DOD_ERR_INVALID, "%s: null total_norm_dev with max_norm > 0 or skip_nonfinite", who);
  if (!(o.beta1 >= 0.0 && o.beta1 < 1.0 && o.beta2 >= 0.0 && o.beta2 < 1.0) || !(o.eps >= 0.f) || !(o.weight_decay >= 0.0) || !(o.max_norm == o.max_norm))
    return dod_fail(DOD_ERR_INVALID, "%s: betas outside [0, 1), negative eps / weight_decay or a NaN max_norm", who);
  if (ema && !(o.ema_w >= 0.0 && o.ema_w <= 1.0)) return dod_fail(DOD_ERR_INVALID, "%s: ema_w = %g outside [0, 1]", who, o.ema_w);
  if (decay)
    for (int i = 0; i < n_tensors; ++i)
      if (!(decay[i] == decay[i])) return dod_fail(DOD_ERR_INVALID, "%s: tensor %d has a NaN decay factor", who, i);
  if (total == 0) return norm ? store_norm0(who, o.total_norm_dev, s) : DOD_OK;
  if (norm && (!ws || ws_bytes < ws_need(n_tensors, total)))
    return dod_fail(DOD_ERR_INVALID, "%s: workspace of %zu bytes, %zu needed", who, ws ? ws_bytes : (size_t)0, ws_need(n_tensors, total));
  double* partial = norm ? reinterpret_cast<double*>(dod::align_ws(ws)) : nullptr;
  int np = -1;                                             // -1: no norm launch, the adam kernel skips the reduction
  if (norm) if (int rc = run_sumsq(who, t, n_tensors, total, partial, &np, s)) return rc;
  Hyper h;
  h.w1 = 1.0 - o.beta1; h.b2 = o.beta2; h.w2 = 1.0 - o.beta2; h.wd = o.weight_decay; h.eps = o.eps; h.ema_w = o.ema_w; h.skip = skip;
  h.max_norm = clip ? (double)o.max_norm : (double)INFINITY;      // the norm for the skip alone: the coefficient is 1
  int i = 0, first_launch = 1;
  while (i < n_tensors) {
    AdamArgs a;
    a.nt = 0; a.first[0] = 0;
    h.nruns = 0;
    for (int r = 0; r < kRuns; ++r) { h.decay[r] = 1.0; h.run_first[r] = 0; }
    h.run_first[kRuns] = 0;
    bool any_ema = false;
    for (; i < n_tensors && a.nt < kAdamT; ++i) {
      if (t[i].n == 0) continue;
      const i64 c = chunks_of(t[i].n, kChunk);
      if (a.first[a.nt] + c > kMaxGrid) break;
      const double dec = decay ? decay[i] : 1.0;
      if (h.nruns == 0 || dec != h.decay[h.nruns - 1]) {
        if (h.nruns == kRuns) break;                       // a fifth decay factor: the next launch
        h.decay[h.nruns] = dec; h.run_first[h.nruns] = a.nt;
        ++h.nruns;
      }
      AdamTensor& d = a.t[a.nt];
      d.p = t[i].p; d.g = t[i].g; d.m = t[i].m; d.v = t[i].v; d.e = ema ? ema[i] : nullptr; d.n = t[i].n;
      d.step_size = t[i].step_size; d.bc2_sqrt = t[i].bc2_sqrt;
      any_ema |= d.e != nullptr;
      a.first[a.nt + 1] = a.first[a.nt] + (int)c;
      ++a.nt;
    }
    if (!a.nt) continue;
    if (any_ema)
      hipLaunchKernelGGL(optim_adam_kernel<true>, dim3(a.first[a.nt]), dim3(kThreads), 0, s, a, h, partial, np, o.total_norm_dev, first_launch, o.skipped_dev);
    else
      hipLaunchKernelGGL(optim_adam_kernel<false>, dim3(a.first[a.nt]), dim3(kThreads), 0, s, a, h, partial, np, o.total_norm_dev, first_launch, o.skipped_dev);
    if (int rc = launched(who)) return rc;
    first_launch = 0;
  }
  return DOD_OK;
}

}  // namespace

long optim_launch_count() { return g_launches.load(); }
long optim_constant(int which) { return which == 0 ? kChunk : which == 1 ? kAdamT : which == 2 ? kNormT : kEmaT; }

extern "C" {

size_t dod_optim_workspace_bytes(int n_tensors, int64_t total_elems) {
  if (n_tensors < 0 || total_elems < 0) return 0;
  return ws_need(n_tensors, total_elems);
}

int dod_optim_clip_grad_norm(const dod_optim_tensor* t, int n_tensors, float max_norm, float* total_norm_dev, void* ws, size_t ws_bytes,
                             void* stream) {
  static const char* who = "dod_optim_clip_grad_norm";
  i64 total = 0;
  if (int rc = check_list(who, t, n_tensors, false, &total)) return rc;
  if (!total_norm_dev) return dod_fail(DOD_ERR_INVALID, "%s: null total_norm_dev", who);
  if (!(max_norm == max_norm)) return dod_fail(DOD_ERR_INVALID, "%s: max_norm is NaN", who);
  hipStream_t s = (hipStream_t)stream;
  if (total == 0) return store_norm0(who, total_norm_dev, s);
  if (!ws || ws_bytes < ws_need(n_tensors, total)) return dod_fail(DOD_ERR_INVALID, "%s: workspace of %zu bytes, %zu needed", who, ws ? ws_bytes : (size_t)0, ws_need(n_tensors, total));
  double* partial = reinterpret_cast<double*>(dod::align_ws(ws));
  int np = 0;
  if (int rc = run_sumsq(who, t, n_tensors, total, partial, &np, s)) return rc;
  int i = 0, first_launch = 1;
  while (i < n_tensors) {
    NormArgs a;
    a.nt = 0; a.per = 1; a.first[0] = 0;
    for (; i < n_tensors && a.nt < kNormT; ++i) {
      if (t[i].n == 0) continue;
      const i64 c = chunks_of(t[i].n, kChunk);
      if (a.first[a.nt] + c > kMaxGrid) break;
      a.g[a.nt] = t[i].g; a.n[a.nt] = t[i].n; a.first[a.nt + 1] = a.first[a.nt] + (int)c;
      ++a.nt;
    }
    if (!a.nt) continue;
    hipLaunchKernelGGL(optim_scale_kernel, dim3(a.first[a.nt]), dim3(kThreads), 0, s, a, (double)max_norm, partial, np, total_norm_dev, first_launch);
    if (int rc = launched(who)) return rc;
    first_launch = 0;
  }
  return DOD_OK;
}

int dod_optim_adam_step(const dod_optim_tensor* t, int n_tensors, double beta1, double beta2, float eps, double weight_decay, float max_norm,
                        float* total_norm_dev, void* ws, size_t ws_bytes, void* stream) {
  dod_optim_options o = {};
  o.beta1 = beta1; o.beta2 = beta2; o.weight_decay = weight_decay; o.eps = eps; o.max_norm = max_norm; o.total_norm_dev = total_norm_dev;
  return run_step("dod_optim_adam_step", t, nullptr, nullptr, n_tensors, o, ws, ws_bytes, (hipStream_t)stream);
}

int dod_optim_step(const dod_optim_tensor* t, float* const* ema, const double* decay, int n_tensors, const dod_optim_options* o, void* ws,
                   size_t ws_bytes, void* stream) {
  static const char* who = "dod_optim_step";
  if (!o) return dod_fail(DOD_ERR_INVALID, "%s: null options", who);
  if (ema && n_tensors > 0)
    for (int i = 0; i < n_tensors; ++i)
      if (ema[i] && t && t[i].n > 0 && (ema[i] == t[i].p || ema[i] == t[i].m || ema[i] == t[i].v))
        return dod_fail(DOD_ERR_INVALID, "%s: the average of tensor %d aliases its parameter or state", who, i);
  return run_step(who, t, ema, decay, n_tensors, *o, ws, ws_bytes, (hipStream_t)stream);
}

int dod_optim_ema_update(const dod_optim_ema_tensor* t, int n_tensors, double w, void* stream) {
  static const char* who = "dod_optim_ema_update";
  if (n_tensors < 0) return dod_fail(DOD_ERR_INVALID, "%s: n_tensors = %d is negative", who, n_tensors);
  if (n_tensors > 0 && !t) return dod_fail(DOD_ERR_INVALID, "%s: null tensor list", who);
  if (!(w >= 0.0 && w <= 1.0)) return dod_fail(DOD_ERR_INVALID, "%s: w = %g outside [0, 1]", who, w);
  for (int i = 0; i < n_tensors; ++i) {
    if (t[i].n < 0) return dod_fail(DOD_ERR_INVALID, "%s: tensor %d has n = %lld", who, i, (long long)t[i].n);
    if (t[i].n > (i64)kChunk * kMaxGrid) return dod_fail(DOD_ERR_INVALID, "%s: tensor %d has more than 2^42 elements", who, i);
    if (t[i].n > 0 && (!t[i].e || !t[i].p)) return dod_fail(DOD_ERR_INVALID, "%s: tensor %d has a null pointer", who, i);
  }
  hipStream_t s = (hipStream_t)stream;
  int i = 0;
  while (i < n_tensors) {
    EmaArgs a;
    a.nt = 0; a.first[0] = 0;
    for (; i < n_tensors && a.nt < kEmaT; ++i) {
      if (t[i].n == 0) continue;
      const i64 c = chunks_of(t[i].n, kChunk);
      if (a.first[a.nt] + c > kMaxGrid) break;
      a.e[a.nt] = t[i].e; a.p[a.nt] = t[i].p; a.n[a.nt] = t[i].n; a.first[a.nt + 1] = a.first[a.nt] + (int)c;
      ++a.nt;
    }
    if (!a.nt) continue;
    hipLaunchKernelGGL(optim_ema_kernel, dim3(a.first[a.nt]), dim3(kThreads), 0, s, a, w);
    if (int rc = launched(who)) return rc;
  }
  return DOD_OK;
}

}  // extern "C"
