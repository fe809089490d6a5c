// fp32-in, bf16-split GEMM with the whole GemmF32X contract of gemm_f32.hip's launch_gemm_f32x: the training step's products on the bf16 cores
// (DOD_PREC_BF16X3 in a training config; train_ops.hip lin_fwd / lin_bwd_x / gemm_tn_acc).
//   C (+)= alpha (Ah Wh^T + Ah Wl^T + Al Wh^T),   x = h + l,  h = bf16_rne(x),  l = bf16_rne(x - h)      (dod_op_split_pair's definition)
// accumulated in fp32 on v_mfma_f32_32x32x16_bf16.  The operands stay what the training step has -- fp32 tape buffers read in three layouts
// (a_kmajor / w_kmajor) -- and are split on the staging path: global fp32 quads (branch-free clamped loads in a register ring, as gemm_f32.hip's
// TileLoad) -> v_cvt_pk_bf16_f32 twice -> LDS as bf16 hi and lo tiles, k contiguous per row, so a lane's 8-element MFMA fragment is one
// ds_read_b128.  Nothing is written twice to memory, and there is no scratch beyond the workgroup's LDS.
//
// Tile (64 T) x (64 T) x 32, T = 1 or 2, 256 threads = 2x2 waves; a wave owns the 32x32 accumulator (wm, wn) of every 64x64 quadrant, computed
// transposed (D = W_tile A_tile^T) like the fp32 kernel: the two epilogues are that kernel's own (gemm_f32x_epi.h), once per quadrant.
// LDS: rows of 32 bf16 + 8 pad = 20 dwords.  Checked bank behaviour (MI355X_MICROARCH.md, LDS):
//   fragment read  ds_read_b128, 16-lane groups {0-3,12-15,20-27} ...: 16 rows distinct mod 16, start bank 20 r mod 64 = 4 (5 r mod 16): the 16
//                  four-bank spans are disjoint -- conflict-free; 4 T reads per 3 T^2 MFMAs (<= 2 per MFMA gap);
//   row-major operand: a thread's 4 k of one row are one ds_write_b64 (hi) + one (lo); 16 lanes = 2 rows x 16 dwords, 20 dwords apart: 4 banks 2-way;
//   k-major operand: a thread holds (k, k + 1) of 4 consecutive rows and writes 4 + 4 ds_write_b32 of a k pair each; lanes 0-31 = 16 k pairs x 2
//                  row quads: bank 16 (quad & 1) + pair (+ 20 i): conflict-free.  (16 k pairs per wave instruction instead of 16 row quads is what
//                  makes it so: a wave's global load covers 64 contiguous bytes of each of 32 k rows.)
// T = 1: two LDS stages, one barrier per k-tile.  T = 2: one stage, two barriers per k-tile -- twice the FLOP per staged byte, for products with
// at least one 128x128 tile per CU.  Both forms take 40 KB of LDS and 156-176 registers per lane (the compiler's resource report), which allows
// two workgroups per CU; that a second resident workgroup covers the one-stage form's barriers is the intent, its occupancy was not measured.
// Measured per product and per step: DESIGN.md section 6b.
#include "dod_common.h"
#include "operand_rows.h"
#include "gemm_f32x_epi.h"
#include <atomic>

#define XBK 32
#define XLD 40      // bf16 per LDS row

namespace {

// One operand's 64-row x 32-k unit (row offset 64 u inside the tile): two quads per thread.
//   KM = false: stored [rows, K]: thread -> (row = tid / 8 + 32 q, k = 4 (tid % 8))
//   KM = true : stored [K, rows]: thread -> (k = 2 (tid % 16) + q, row = 4 (tid / 16))
// VEC as in gemm_f32.hip: aligned float4 loads, else four scalar loads; both branch-free (clamped address, value zeroed at the LDS store).
template <bool KM, bool VEC>
struct SplitLoad {
  const float* base; int ld, rows, kend, r0; int a, b;
  __device__ __forceinline__ void init(const float* base_, int ld_, int rows_, int kend_, int r0_, int tid) {
    base = base_; ld = ld_; rows = rows_; kend = kend_; r0 = r0_;
    if (KM) { a = 2 * (tid & 15); b = 4 * (tid >> 4); } else { a = tid >> 3; b = 4 * (tid & 7); }
  }
  // (o, c): the strided and the contiguous coordinate of quad q of unit u at k-tile origin k0
  __device__ __forceinline__ int oc(int k0, int u, int q, int& c) const {
    c = KM ? r0 + 64 * u + b : k0 + b;
    return KM ? k0 + a + q : r0 + 64 * u + a + 32 * q;
  }
  __device__ __forceinline__ float4 load(int k0, int u, int q) const {
    int c; const int o = oc(k0, u, q, c);
    const int on = KM ? kend : rows, cn = KM ? rows : kend;
    const float* row = base + (size_t)(o < on ? o : 0) * ld;
    float4 v;
    if (VEC) {
      v = *reinterpret_cast<const float4*>(row + (c < cn ? c : 0));
    } else {
      v.x = row[c < cn ? c : 0]; v.y = row[c + 1 < cn ? c + 1 : 0]; v.z = row[c + 2 < cn ? c + 2 : 0]; v.w = row[c + 3 < cn ? c + 3 : 0];
    }
    return v;
  }
  __device__ __forceinline__ float4 mask(float4 v, int k0, int u, int q) const {
    int c; const int o = oc(k0, u, q, c);
    const int on = KM ? kend : rows, cn = KM ? rows : kend;
    const bool oin = o < on;
    v.x = oin && c < cn ? v.x : 0.f; v.y = oin && c + 1 < cn ? v.y : 0.f; v.z = oin && c + 2 < cn ? v.z : 0.f; v.w = oin && c + 3 < cn ? v.w : 0.f;
    return v;
  }
  // sh / sl: the hi / lo tile's row 0 of unit u
  __device__ __forceinline__ void store(bf16_t* sh, bf16_t* sl, float4 v0, float4 v1, int k0, int u) const {
    v0 = mask(v0, k0, u, 0); v1 = mask(v1, k0, u, 1);
    if (KM) {
      const float x0[4] = {v0.x, v0.y, v0.z, v0.w}, x1[4] = {v1.x, v1.y, v1.z, v1.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        uint32_t h, l; bf16_split2(x0[i], x1[i], h, l);
        *reinterpret_cast<uint32_t*>(sh + (b + i) * XLD + a) = h;      // a even: 4-byte aligned
        *reinterpret_cast<uint32_t*>(sl + (b + i) * XLD + a) = l;
      }
    } else {
      uint2 h, l;
      bf16_split2(v0.x, v0.y, h.x, l.x); bf16_split2(v0.z, v0.w, h.y, l.y);
      *reinterpret_cast<uint2*>(sh + a * XLD + b) = h;                 // 80-byte rows, b % 4 == 0: 8-byte aligned
      *reinterpret_cast<uint2*>(sl + a * XLD + b) = l;
      bf16_split2(v1.x, v1.y, h.x, l.x); bf16_split2(v1.z, v1.w, h.y, l.y);
      *reinterpret_cast<uint2*>(sh + (a + 32) * XLD + b) = h;
      *reinterpret_cast<uint2*>(sl + (a + 32) * XLD + b) = l;
    }
  }
};

// acc over the k-tiles [kt0, kt1) (kt0 < kt1); smem: NS stages of [A hi | A lo | W hi | W lo], each 64 T rows of XLD bf16.
// PD k-tiles of global loads are in flight per thread; tiles past the end load a clamped address and are zeroed at the LDS store, so the
// ring's loop body has no branch around a load.
template <int T, int PD, class LA, class LW>
__device__ __forceinline__ void x3_mainloop(const LA& la, const LW& lw, int kt0, int kt1, bf16_t* smem, f32x16 (&acc)[T][T]) {
  constexpr int NS = T == 1 ? 2 : 1;
  constexpr int OPER = T * 64 * XLD, STAGE = 4 * OPER;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int lr = lane & 31, lh = lane >> 5;
  const int nk = kt1 - kt0;
  float4 ra[PD][2 * T], rw[PD][2 * T];
  auto gload = [&](int p, int kt) {
#pragma unroll
    for (int u = 0; u < T; ++u)
#pragma unroll
      for (int q = 0; q < 2; ++q) { ra[p][2 * u + q] = la.load(kt * XBK, u, q); rw[p][2 * u + q] = lw.load(kt * XBK, u, q); }
  };
  auto sstore = [&](int st, int p, int kt) {
    bf16_t* s = smem + st * STAGE;
#pragma unroll
    for (int u = 0; u < T; ++u) {
      la.store(s + u * 64 * XLD, s + OPER + u * 64 * XLD, ra[p][2 * u], ra[p][2 * u + 1], kt * XBK, u);
      lw.store(s + 2 * OPER + u * 64 * XLD, s + 3 * OPER + u * 64 * XLD, rw[p][2 * u], rw[p][2 * u + 1], kt * XBK, u);
    }
  };
  auto mma = [&](int st) {
    const bf16_t* s = smem + st * STAGE;
#pragma unroll
    for (int ks = 0; ks < XBK / 16; ++ks) {
      bf16x8 ah[T], al[T], wh[T], wl[T];
#pragma unroll
      for (int i = 0; i < T; ++i) {
        const int oa = (i * 64 + wm * 32 + lr) * XLD + ks * 16 + 8 * lh, ow = (i * 64 + wn * 32 + lr) * XLD + ks * 16 + 8 * lh;
        ah[i] = *reinterpret_cast<const bf16x8*>(s + oa); al[i] = *reinterpret_cast<const bf16x8*>(s + OPER + oa);
        wh[i] = *reinterpret_cast<const bf16x8*>(s + 2 * OPER + ow); wl[i] = *reinterpret_cast<const bf16x8*>(s + 3 * OPER + ow);
      }
#pragma unroll
      for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl[j], ah[i], acc[i][j], 0, 0, 0);      // small terms first
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[j], al[i], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[j], ah[i], acc[i][j], 0, 0, 0);
        }
    }
  };
#pragma unroll
  for (int p = 0; p < PD; ++p) gload(p, kt0 + p);
  sstore(0, 0, kt0);
  __syncthreads();
  int kt = 0;
  for (; kt + PD <= nk; kt += PD) {               // full groups: tile kt + j sits in LDS stage j % NS and leaves ring slot j free
#pragma unroll
    for (int j = 0; j < PD; ++j) {
      gload(j, kt0 + kt + j + PD);
      mma(j % NS);
      if (NS == 1) __syncthreads();               // one stage: every wave has read it before the next tile overwrites it
      sstore((j + 1) % NS, (j + 1) % PD, kt0 + kt + j + 1);
      __syncthreads();
    }
  }
#pragma unroll
  for (int j = 0; j < PD - 1; ++j) {              // the last nk % PD tiles are already in the ring
    if (kt + j < nk) {                            // uniform
      mma(j % NS);
      if (kt + j + 1 < nk) {
        if (NS == 1) __syncthreads();
        sstore((j + 1) % NS, j + 1, kt0 + kt + j + 1);
      }
      __syncthreads();
    }
  }
}

template <int T, bool AKM, bool WKM, bool VEC>
__global__ __launch_bounds__(256) void gemm_f32x3_kernel(GemmF32X g) {
  constexpr int BT = 64 * T;
  constexpr int PD = T == 1 ? 4 : 2;                                   // ring depth: 64 VGPRs of loads in flight either way
  __shared__ __attribute__((aligned(16))) bf16_t x3_smem[(T == 1 ? 2 : 1) * 4 * T * 64 * XLD];      // 40 KB; the K-slice epilogue's [64][65] floats
  static_assert(sizeof(x3_smem) >= 64 * 65 * 4, "the staged epilogue reuses the tile buffer");
  const int tid = threadIdx.x;
  const int tiles_m = (g.M + BT - 1) / BT;
  const int tn = blockIdx.x / tiles_m, tm = blockIdx.x - tn * tiles_m;
  const int m0 = tm * BT, n0 = tn * BT;
  const int zb = blockIdx.y / g.hb, zh = blockIdx.y - zb * g.hb;
  const int nkt = (g.K + XBK - 1) / XBK;
  int kt0 = 0, kt1 = nkt;
  if (g.ksplit > 1) {
    const int per = (nkt + g.ksplit - 1) / g.ksplit;
    kt0 = blockIdx.z * per; kt1 = kt0 + per < nkt ? kt0 + per : nkt;
    if (kt0 >= kt1) return;                                   // uniform: before any barrier
  }
  const int kend = kt1 * XBK < g.K ? kt1 * XBK : g.K;
  SplitLoad<AKM, VEC> la;
  SplitLoad<WKM, VEC> lw;
  la.init(g.A + zb * g.a_sb + zh * g.a_sh, g.lda, g.M, kend, m0, tid);
  lw.init(g.W + zb * g.w_sb + zh * g.w_sh, g.ldw, g.N, kend, n0, tid);
  f32x16 acc[T][T];
#pragma unroll
  for (int i = 0; i < T; ++i)
#pragma unroll
    for (int j = 0; j < T; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  x3_mainloop<T, PD>(la, lw, kt0, kt1, x3_smem, acc);

  float* cz = g.C + zb * g.c_sb + zh * g.c_sh;
#pragma unroll
  for (int i = 0; i < T; ++i)
#pragma unroll
    for (int j = 0; j < T; ++j) {      // quadrants past the edge: the epilogues' own m / n guards skip every element
      if (g.ksplit > 1) f32x_epi_atomic(g, cz, m0 + 64 * i, n0 + 64 * j, acc[i][j], reinterpret_cast<float*>(x3_smem), blockIdx.z == 0);
      else f32x_epi_direct(g, cz, m0 + 64 * i, n0 + 64 * j, acc[i][j]);
    }
}

std::atomic<long> g_x3_count{0}, g_x3_wide{0};

template <int T>
void x3_launch(const GemmF32X& g, bool vec, hipStream_t s) {
  const int tiles = ((g.M + 64 * T - 1) / (64 * T)) * ((g.N + 64 * T - 1) / (64 * T));
  const dim3 grid(tiles, g.batch, g.ksplit);
#define X3_LAUNCH(AK, WK) do { if (vec) hipLaunchKernelGGL((gemm_f32x3_kernel<T, AK, WK, true>), grid, dim3(256), 0, s, g); \
                               else hipLaunchKernelGGL((gemm_f32x3_kernel<T, AK, WK, false>), grid, dim3(256), 0, s, g); } while (0)
  if (g.a_kmajor && g.w_kmajor) X3_LAUNCH(true, true);
  else if (g.a_kmajor) X3_LAUNCH(true, false);
  else if (g.w_kmajor) X3_LAUNCH(false, true);
  else X3_LAUNCH(false, false);
#undef X3_LAUNCH
}

}  // namespace

long gemm_f32x3_count(int wide) { return wide ? g_x3_wide.load() : g_x3_count.load(); }

int launch_gemm_f32x3(const GemmF32X& g_, hipStream_t s) {
  GemmF32X g = g_;
  if (const int rc = f32x_normalize(g, XBK)) return rc;
  // 128x128 from one such tile per CU up (256 CUs): below that the wide tile leaves CUs idle where the 64x64 grid fills them
  const long wide_tiles = (long)((g.M + 127) / 128) * ((g.N + 127) / 128) * g.batch;
  const int opt = dod_option(DOD_OPT_F32X3_TILE);      // test hook: 64 / 128 force a form
  const bool wide = opt == 128 || (opt != 64 && wide_tiles >= 256);
  const bool vec = vec_ok(g.A, g.lda, g.a_sb, g.a_sh) && vec_ok(g.W, g.ldw, g.w_sb, g.w_sh);
  if (wide) x3_launch<2>(g, vec, s); else x3_launch<1>(g, vec, s);
  ++g_x3_count;
  if (wide) ++g_x3_wide;
  return hipGetLastError() == hipSuccess ? 0 : 3;
}
