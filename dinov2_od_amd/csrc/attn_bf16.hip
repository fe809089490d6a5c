// Backbone self-attention (K5), flash-style, bf16 MFMA, head_dim 64 (every DINOv2 variant).
// Replaces Dinov2SelfAttention.forward's softmax(Q K^T * dh^-0.5) V
// (site-packages/transformers/models/dinov2/modeling_dinov2.py:153-178, 215-229): no mask, non-causal.
//
// Layout: qkv is the fused-QKV GEMM output [B*N, 3*D] bf16 (q | k | v column blocks, head h at
// columns h*64..h*64+63 of each block); ctx is [B*N, D] bf16.
// One workgroup = 4 waves = 256 query rows of one (batch, head); each wave owns 64 query rows (two 32-row MFMA blocks).
// K/V tiles of 64 keys stream by LDS-DMA into a 3-slot ring (48 KiB, 3 workgroups/CU), two tiles in flight behind
// a counted s_waitcnt vmcnt(4) and one raw s_barrier per tile.
// "Swapped" products keep the query on the MFMA lane so the softmax row state (m, l) is per-lane:
//   S^T = K Q^T   (A = K tile rows from LDS via ds_read_b128, B = Q fragments held in registers)
//   O^T += V^T P^T (A = V^T via ds_read_b64_tr_b16 from the row-major V tile, B = the S^T accumulator
//                  registers themselves, converted to bf16 - no LDS round trip for P)
// N = 1370 is not a multiple of 64: the last tile's keys >= N get -inf before the row max; rows >= N
// lie past the staging descriptor's bound and arrive as zeros (p = 0 times 0).  The last tile runs behind
// the loop of full tiles, at half width when it holds at most 32 keys.
#include "dod_common.h"
#include <atomic>
#include <cstdlib>
#include <type_traits>

#define AT_WAVES 4
// AT_NQ (32-row query blocks per wave) is a template parameter of the kernel: 2 for large launches, 1 for small ones
#define AT_KV 64

__device__ __forceinline__ int kswz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }
// V tile: rows r and r+2 of a 4-row tr-read block are 256 B apart (same banks): flip the 64-B half on row bit 1
__device__ __forceinline__ int vswz(int row, int chunk) { return chunk ^ (((row >> 1) & 1) << 2); }

typedef bf16x4 __attribute__((address_space(3))) * lds_bf16x4_ptr;

// One K/V tile (64 keys) for one wave and NQ blocks of 32 query rows (query on the lane).  TAIL != 0 masks keys >= N
// (last tile only, so the full tiles carry no compare/select).  TAIL == 2: the last tile holds at most 32 keys (N = 1370: 26), so its
// second 32-key block is all masked -- scores of -inf, p = +0, +0 into l and O -- and is not computed at all: KB = 1 key block, half the
// S MFMAs, exps and packs, no V^T read past row 31, two P V k-steps instead of four.  The bits equal the full-width tile's.
// Softmax in the exp2 domain with the scale folded into one FMA: p = exp2(s*c - m*c), m = running max of the raw scores (c > 0).
// NQ = 2 gives the scheduler two independent MFMA -> VALU -> MFMA chains to interleave (PMC on NQ = 1: 42 % of wave
// cycles stalled on instruction dependencies, MFMA pipe 34 % busy) and halves the K/V fragment reads per MFMA.
// REF: the reference form, for the tiles behind the first of the fixed-reference pass (attn_bf16_body).  m_run is then the row's FROZEN reference,
// the scaled maximum of key tile 0: p = exp2(s*c - m_run) and l += sum p, with no row maximum (its 46 v_max3 / v_max, the lane swap -- the
// head of the chain S -> max -> exp -> pack -> P V --), no alpha and no rescale of O and l: about 128 plain instructions and 2 exponentials
// less per tile at NQ = 2.  A masked key is still -inf -> p = +0.  p may exceed 1 here; what happens when it grows too far is the caller's.
template <int TAIL, int NQ, bool REF>
__device__ __forceinline__ void attn_tile(const char* sK, const char* sV, const bf16x8 (&qf)[NQ][4], f32x16 (&o)[NQ][2],
                                          float (&m_run)[NQ], float (&l_run)[NQ], float c, int kbase, int N,
                                          int lr, int lh, int g16, int tq, int tp) {
  constexpr int KB = TAIL == 2 ? 1 : 2;      // 32-key blocks computed
  f32x16 s[NQ][KB];
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    const int row = kb * 32 + lr;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sK + row * 128 + kswz(row, 2 * t + lh) * 16);
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        s[q][kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[q][t], t == 0 ? zero : s[q][kb], 0, 0, 0);
    }
  }
  bf16x8 pf[NQ][4];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    if (TAIL) {
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kbase + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          if (key >= N) s[q][kb][r] = -INFINITY;
        }
    }
    float alpha = 1.f;
    if (!REF) {
      float mx = s[q][0][0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[q][0][r]);
      if (KB == 2) {
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[q][KB - 1][r]);
      }
      {   // other half's max by v_permlane32_swap (VALU; __shfl_xor goes through the LDS crossbar and an lgkmcnt wait)
        const unsigned mb = __float_as_uint(mx);
        const auto sw = __builtin_amdgcn_permlane32_swap(mb, mb, false, false);
        mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
      }
      const float m_new = fmaxf(m_run[q], mx * c);            // scaled (exp2-domain) running max
      alpha = __builtin_amdgcn_exp2f(m_run[q] - m_new);
      m_run[q] = m_new;
    }
    const float nm = -m_run[q];
    float lsum;
    {      // Plain fp32 VALU only (one value per lane), and the file is built with -fno-slp-vectorize (_build.py) so that hipcc does not re-pack it:
           // `tools/probes/mfma_valu_overlap.hip` (profiles/r04_mfma_valu_overlap_probe.txt) shows that v_pk_*_f32 does NOT overlap an executing MFMA
           // on this part -- a wave of v_pk_fma_f32 beside a wave of MFMAs on the same SIMD takes the SUM of their times, and with two waves per
           // SIMD the packed form has no throughput advantage either (4 cycles per instruction against 2 for the plain one) -- while plain VALU,
           // v_exp_f32, v_max3_f32 and v_cvt_pk_bf16_f32 do overlap it.  Rounds 2-3 had forced v_pk_fma / v_pk_add / v_pk_mul here (fewer
           // instructions: 376 against 420 per tile); this form is 4 % faster (6.06 -> 5.83 ms of attention per batch-64 step).
      float l0 = 0.f, l1 = 0.f, l2 = 0.f, l3 = 0.f;
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; r += 4) {
          const float e0 = __builtin_amdgcn_exp2f(fmaf(s[q][kb][r], c, nm)), e1 = __builtin_amdgcn_exp2f(fmaf(s[q][kb][r + 1], c, nm));
          const float e2 = __builtin_amdgcn_exp2f(fmaf(s[q][kb][r + 2], c, nm)), e3 = __builtin_amdgcn_exp2f(fmaf(s[q][kb][r + 3], c, nm));
          l0 += e0; l1 += e1; l2 += e2; l3 += e3;
          s[q][kb][r] = e0; s[q][kb][r + 1] = e1; s[q][kb][r + 2] = e2; s[q][kb][r + 3] = e3;
        }
      lsum = (l0 + l1) + (l2 + l3);
    }
    // Two ideas to keep apart.  (a) A thresholded "lazy" rescale -- the per-tile maximum stays, all of its max instructions and the swap, and a
    //  wave-uniform branch INSIDE the tile moves the reference only when a row's maximum exceeds it by 2^8 -- was measured twice and lost: 4 % slower
    //  on the packed form of round 3, 5 % slower on this one (attention 6.05 -> 6.38 ms, tools/experiments/r4_exp30.sh; 8 spilled registers): the
    //  branch splits the scheduling region.  (b) REF removes the maximum itself from the tile and adds no branch to it; the one decision -- did a
    //  row outgrow its reference -- is taken once, behind the last tile (attn_bf16_body).
    if (REF) {
      l_run[q] += lsum;                       // per-half partial; the halves are combined once at the end
    } else {
      l_run[q] = fmaf(l_run[q], alpha, lsum);
#pragma unroll
      for (int r = 0; r < 16; ++r) { o[q][0][r] *= alpha; o[q][1][r] *= alpha; }
    }
    // P^T fragments: accumulator registers 8u..8u+7 of key block kb are the B operand of k-step 2kb+u
#pragma unroll
    for (int s4 = 0; s4 < 2 * KB; ++s4) {
      const f32x16& pp = s[q][s4 >> 1];
      const int u = (s4 & 1) * 8;
      uint4 pk;
      pk.x = pack2bf(pp[u + 0], pp[u + 1]);
      pk.y = pack2bf(pp[u + 2], pp[u + 3]);
      pk.z = pack2bf(pp[u + 4], pp[u + 5]);
      pk.w = pack2bf(pp[u + 6], pp[u + 7]);
      pf[q][s4] = __builtin_bit_cast(bf16x8, pk);
    }
  }
  // V^T fragments by ds_read_b64_tr_b16 in inline asm: the builtin form makes hipcc wait vmcnt(0) (it treats the
  // read as aliasing the pending LDS-DMA writes), which would drain the K/V ring every tile.  Eight reads + their
  // lgkmcnt wait form ONE statement (cdna guide 5.7 item 1, form i).  Rows 16*s4 (+8) of a lane's address differ
  // only by immediates because the V swizzle depends on row bit 1 alone.
  {
    const int rowb = 4 * lh + tq;
    const int col0 = 16 * (g16 & 1) + 4 * tp;
    const int chunk0 = col0 >> 3, inb = (col0 & 7) * 2;
    const unsigned vaddr = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const char*)sV;
    const unsigned a0 = vaddr + rowb * 128 + vswz(rowb, chunk0) * 16 + inb;        // d-block 0
    const unsigned a1 = vaddr + rowb * 128 + vswz(rowb, chunk0 + 4) * 16 + inb;    // d-block 1
#pragma unroll
    for (int db = 0; db < 2; ++db) {
      bf16x4 v0, v1, v2, v3, v4, v5, v6, v7;
      if (KB == 1) {      // keys 0..31 only
        asm volatile(
            "ds_read_b64_tr_b16 %0, %4\n\t"
            "ds_read_b64_tr_b16 %1, %4 offset:1024\n\t"
            "ds_read_b64_tr_b16 %2, %4 offset:2048\n\t"
            "ds_read_b64_tr_b16 %3, %4 offset:3072\n\t"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3)
            : "v"(db ? a1 : a0)
            : "memory");
        const bf16x8 vf0 = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
        const bf16x8 vf1 = __builtin_shufflevector(v2, v3, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          o[q][db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf0, pf[q][0], o[q][db], 0, 0, 0);
          o[q][db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf1, pf[q][1], o[q][db], 0, 0, 0);
        }
        continue;
      }
      asm volatile(
          "ds_read_b64_tr_b16 %0, %8\n\t"
          "ds_read_b64_tr_b16 %1, %8 offset:1024\n\t"
          "ds_read_b64_tr_b16 %2, %8 offset:2048\n\t"
          "ds_read_b64_tr_b16 %3, %8 offset:3072\n\t"
          "ds_read_b64_tr_b16 %4, %8 offset:4096\n\t"
          "ds_read_b64_tr_b16 %5, %8 offset:5120\n\t"
          "ds_read_b64_tr_b16 %6, %8 offset:6144\n\t"
          "ds_read_b64_tr_b16 %7, %8 offset:7168\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3), "=&v"(v4), "=&v"(v5), "=&v"(v6), "=&v"(v7)
          : "v"(db ? a1 : a0)
          : "memory");
      const bf16x8 vf0 = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
      const bf16x8 vf1 = __builtin_shufflevector(v2, v3, 0, 1, 2, 3, 4, 5, 6, 7);
      const bf16x8 vf2 = __builtin_shufflevector(v4, v5, 0, 1, 2, 3, 4, 5, 6, 7);
      const bf16x8 vf3 = __builtin_shufflevector(v6, v7, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        o[q][db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf0, pf[q][0], o[q][db], 0, 0, 0);
        o[q][db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf1, pf[q][1], o[q][db], 0, 0, 0);
        o[q][db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf2, pf[q][2], o[q][db], 0, 0, 0);
        o[q][db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf3, pf[q][3], o[q][db], 0, 0, 0);
      }
    }
  }
}

// tuning only (tools/attn_timeline.py): per workgroup {tile-loop cycles, cycles waiting for DMA + barrier, tiles, active,
// s_memrealtime (100 MHz) at kernel entry, at the end of the tile loop}; the exit time is the next workgroup's entry
#ifdef DINODET_TUNING
__device__ unsigned long long* g_attn_stamps = nullptr;
#define ATTN_STAMPS g_attn_stamps
#else
#define ATTN_STAMPS (static_cast<unsigned long long*>(nullptr))      // release build: the stamp code folds away
#endif

// K/V ring, [slot][K|V][64 rows][128 B] = 48 KiB: ONE file-scope array, so that both bodies of the fused kernel address the same
// compile-time-constant LDS locations (a pointer parameter cost the 64-rows-per-wave body three registers and a spill)
// Behind the ring: one vote word per wave (attn_bf16_body).  They live in THIS array on purpose: with a second __shared__ variable in the
// kernel hipcc tags every LDS access with the variable it belongs to, then sees the LDS-DMA writes and the K fragment reads hit the same one,
// and waits vmcnt(0) -- the two tiles in flight -- before the first ds_read of EVERY tile (measured: the kernel no faster than its parent).
#define AT_RING_BYTES (3 * 2 * AT_KV * 128)
__shared__ __attribute__((aligned(16))) char g_attn_smem[AT_RING_BYTES + 4 * AT_WAVES];
__device__ unsigned int g_attn_reruns;                                  // workgroups that reran (dod_test_counter("attn_rerun"))
// The fixed-reference pass holds for a row while its normaliser l_tot = sum_k exp2(s_k c - m0), m0 the scaled maximum of key tile 0, stays below
// 2^60.  Every p is at most l_tot, so below the threshold the exp2 argument stays <= 60: the fp32 rounding of s c - m0 then moves p by at most
// 60 * 2^-24 * ln 2 = 2.5e-6 relative (inside attention_cases.ACC_REL), bf16 keeps P's relative precision at any exponent, and an accumulator
// |sum p v| <= l_tot max|v| cannot overflow fp32 for any |v| < 2^67.  Whatever lies beyond that shows as an accumulator that is not finite.
constexpr float AT_REF_LMAX = 0x1p60f;
// the kernel body for workgroup index `blk_` of a launch over query rows [q_lo, q_hi)
// MX (fp8 mode, round 4): the context leaves as block-scaled e4m3 -- ctx is then a BYTE buffer [B*N, D], bs its e8m0 bytes [B*N][2][D / 64] --
// the out-proj GEMM's operand, written here instead of by a quantisation pass over bf16 rows (a head's 64 columns are two blocks of 32)
// DIET = false (test option "attn_diet" = 0): the full-width tail tile and the per-lane global pointers of the staging, as before
template <int AT_NQ, bool MX, bool DIET>
__device__ __forceinline__ void attn_bf16_body(const int blk_, const bf16_t* __restrict__ qkv, bf16_t* __restrict__ ctx,
                                               int N, int heads, int npairs, float scale_log2e, int q_lo, int q_hi, unsigned char* __restrict__ bs, int fixed_ref) {
  char* const smem = g_attn_smem;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lr = lane & 31, lh = lane >> 5;
  const int D = heads * 64, ld = 3 * D;
  const unsigned long long rt_entry = ATTN_STAMPS ? __builtin_amdgcn_s_memrealtime() : 0;
  // XCD-aware block order: workgroups are dealt round-robin over the 8 XCDs, so the q-blocks of one (image, head)
  // -- which all stream the same 350 KB of K/V -- are placed on ONE XCD (pair p -> XCD p % 8) and run back to back
  // there; with the plain (q-block, head, image) grid each XCD saw ~70 different pairs at once (24 MB of K/V
  // against a 4 MB L2: FETCH_SIZE showed K/V fetched 5.5x).  Speed only; any placement is correct.
  constexpr int AT_QW = 32 * AT_NQ;
  const int nqb = (q_hi - q_lo + AT_WAVES * AT_QW - 1) / (AT_WAVES * AT_QW);      // query rows [q_lo, q_hi) of every (image, head); keys 0..N-1
  int b, h, qb;
  {
    const int L = blk_, xcd = L & 7, s = L >> 3;
    const int pair = (s / nqb) * 8 + xcd;
    qb = s - (s / nqb) * nqb;
    if (pair >= npairs) return;            // grid is padded to a multiple of 8 pairs
    b = pair / heads;
    h = pair - b * heads;
  }
  const int q0 = q_lo + qb * (AT_WAVES * AT_QW) + wid * AT_QW;
  const bf16_t* base = qkv + (size_t)b * N * ld;

  // Q fragments: B operand of S^T = K Q^T: lane holds Q[q = lr][d = 16 t + 8 lh + 0..7]
  bf16x8 qf[AT_NQ][4];
#pragma unroll
  for (int q = 0; q < AT_NQ; ++q) {
    int qr = q0 + q * 32 + lr; qr = qr < N ? qr : N - 1;
    const bf16_t* qp = base + (size_t)qr * ld + h * 64 + lh * 8;
#pragma unroll
    for (int t = 0; t < 4; ++t) qf[q][t] = *reinterpret_cast<const bf16x8*>(qp + 16 * t);
  }
  // Retire the Q loads HERE, before any LDS-DMA is in flight: beside a pending global_load_lds hipcc waits
  // vmcnt(0) at the first use of an ordinary load's result, which would land inside the tile loop and drain
  // the DMA ring every iteration.  The empty asm makes the fragments "produced" at this point.
#pragma unroll
  for (int q = 0; q < AT_NQ; ++q)
#pragma unroll
    for (int t = 0; t < 4; ++t) asm volatile("" : "+v"(qf[q][t]));

  // staging: LDS-DMA (global_load_lds_dwordx4) into a 3-slot ring of K/V tiles, two tiles in flight.
  // One piece = 8 key rows x 128 B; per tile a wave issues 2 pieces of K and 2 of V.  lane -> (row = lane>>3,
  // LDS chunk slot = lane&7); the swizzle goes on the SOURCE chunk (K: ^(row>>1)&7, V: ^((row>>1)&1)<<2).
  typedef __attribute__((address_space(1))) const void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  const int wu = __builtin_amdgcn_readfirstlane(wid);
  const int prow0 = wu * 16 + (lane >> 3), prow1 = prow0 + 8;          // tile rows of this lane's two pieces
  const int kc0 = ((lane & 7) ^ ((prow0 >> 1) & 7)) * 8, kc1 = ((lane & 7) ^ ((prow1 >> 1) & 7)) * 8;
  const int vc0 = ((lane & 7) ^ (((prow0 >> 1) & 1) << 2)) * 8, vc1 = ((lane & 7) ^ (((prow1 >> 1) & 1) << 2)) * 8;
  const bf16_t* kbase = base + D + h * 64;
  // DIET: staging through a buffer descriptor (as gemm_pp.hip): the base is the (image, head) K column block advanced to the tile's first
  // key row -- wave-uniform, in SGPRs --, a lane keeps one 32-bit byte offset per piece, computed here once, and V lies 2 D bytes behind K
  // in the scalar offset.  num_records ends with the V columns of the tile's last key < N, so a key row >= N starts past it and reads
  // as zeros instead of being clamped to row N - 1: a zero K row is masked like any other, a zero V row meets p = 0.  (The bound is
  // met by the lane offset alone, however the hardware counts the scalar one: a valid K chunk ends 2 D bytes before it, the next row
  // starts 4 D - 128 past it.)  Four live offsets cost registers -- hipcc recomputed the pointers of AT_STAGE_PTR from the lane id every
  // tile: 227 -> 235 in the 64-row body, 126 -> 152 in the 32-row one --; what this form removes is per-tile VALU work.
  const unsigned ldb = (unsigned)ld * 2;
  const unsigned ok0 = prow0 * ldb + kc0 * 2, ok1 = prow1 * ldb + kc1 * 2, ov0 = prow0 * ldb + vc0 * 2, ov1 = prow1 * ldb + vc1 * 2;
  const unsigned row_end = 2 * D + 128;                               // from a key row's K columns to the end of its V columns
#define AT_STAGE_BUF(slot_, kt_)                                                                               \
  {                                                                                                            \
    const int left_ = N - (kt_) * AT_KV;                               /* key rows from this tile on */        \
    const __amdgpu_buffer_rsrc_t r_ = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)kbase + (size_t)(kt_) * AT_KV * ldb), 0, \
                                                                        (int)((unsigned)((left_ < AT_KV ? left_ : AT_KV) - 1) * ldb + row_end), 0x00020000); \
    char* sK_ = smem + (slot_) * (2 * AT_KV * 128) + wu * 2048;                                                \
    char* sV_ = sK_ + AT_KV * 128;                                                                             \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r_, (lptr_t)(sK_), 16, ok0, 0, 0, 0);                             \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r_, (lptr_t)(sK_ + 1024), 16, ok1, 0, 0, 0);                      \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r_, (lptr_t)(sV_), 16, ov0, 2 * D, 0, 0);                         \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r_, (lptr_t)(sV_ + 1024), 16, ov1, 2 * D, 0, 0);                  \
  }
#define AT_STAGE(slot_, kt_) { if (DIET) AT_STAGE_BUF(slot_, kt_) else AT_STAGE_PTR(slot_, kt_) }
#define AT_STAGE_PTR(slot_, kt_)                                                                               \
  {                                                                                                            \
    int key0 = (kt_) * AT_KV + prow0, key1 = (kt_) * AT_KV + prow1;                                            \
    key0 = key0 < N ? key0 : N - 1; key1 = key1 < N ? key1 : N - 1;                                            \
    const bf16_t* r0 = kbase + (size_t)key0 * ld;                                                              \
    const bf16_t* r1 = kbase + (size_t)key1 * ld;                                                              \
    char* sK_ = smem + (slot_) * (2 * AT_KV * 128) + wu * 2048;                                                \
    char* sV_ = sK_ + AT_KV * 128;                                                                             \
    __builtin_amdgcn_global_load_lds((gptr_t)(r0 + kc0), (lptr_t)(sK_), 16, 0, 0);                             \
    __builtin_amdgcn_global_load_lds((gptr_t)(r1 + kc1), (lptr_t)(sK_ + 1024), 16, 0, 0);                      \
    __builtin_amdgcn_global_load_lds((gptr_t)(r0 + D + vc0), (lptr_t)(sV_), 16, 0, 0);                         \
    __builtin_amdgcn_global_load_lds((gptr_t)(r1 + D + vc1), (lptr_t)(sV_ + 1024), 16, 0, 0);                  \
  }

  f32x16 o[AT_NQ][2];
  float m_run[AT_NQ], l_run[AT_NQ];
  const bool active = __builtin_amdgcn_readfirstlane(q0) < q_hi;     // waves past the last row only stage and sync

  // tr-read lane geometry (ds_read_b64_tr_b16: 16-lane groups, lane 4q+p supplies row q, cols 4p..4p+3)
  const int g16 = lane >> 4, i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;

  const int nkt = (N + AT_KV - 1) / AT_KV;
  const int nfull = N / AT_KV;                 // tiles without a masked key
  int slot = 0;
  unsigned long long* stamps = ATTN_STAMPS;
  unsigned long long t_begin = 0, t_wait = 0;
  // tile kt has landed (tile kt+1 may fly) and every wave is behind tile kt-1, whose slot takes tile kt+2
  auto tile_ready = [&](int kt) __attribute__((always_inline)) {
    unsigned long long tw0 = 0;
    if (stamps) tw0 = __builtin_amdgcn_s_memtime();
    if (kt + 1 < nkt) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (stamps) t_wait += __builtin_amdgcn_s_memtime() - tw0;
    if (kt + 2 < nkt) {
      const int ns = slot >= 1 ? slot - 1 : 2;      // (slot + 2) % 3: the slot tile kt-1 just vacated
      AT_STAGE(ns, kt + 2)
    }
  };
  // One pass over the keys: (m, l, O) of this wave's rows from nothing.
  // FIX = false: every tile tracks the running row maximum and rescales O and l by alpha.
  // FIX = true: tile 0 does, and stands in front of the loop; every tile behind it -- the loop of full tiles and the masked last one -- is the
  // reference form (attn_tile REF), which subtracts tile 0's maximum.  Softmax does not care which reference is subtracted; the rows whose
  // maximum lies in tile 0 get the very bits of FIX = false (alpha is exactly 1 there).
  // Either way the loop body holds ONE form of the tile -- with the tail forms as branches of the body the register allocation of all of them
  // met in one region (64-row body: 256 registers and spills; here 235).
  auto pass = [&](auto fix_) __attribute__((always_inline)) {
    constexpr bool FIX = decltype(fix_)::value;
#pragma unroll
    for (int q = 0; q < AT_NQ; ++q) {
#pragma unroll
      for (int r = 0; r < 16; ++r) { o[q][0][r] = 0.f; o[q][1][r] = 0.f; }
      m_run[q] = -INFINITY; l_run[q] = 0.f;
    }
    AT_STAGE(0, 0)
    if (nkt > 1) AT_STAGE(1, 1)
    slot = 0;
    int kt = 0;
    if (FIX) {      // only with nkt > 1: tile 0 is a full tile
      tile_ready(0);
      if (active) attn_tile<0, AT_NQ, false>(smem, smem + AT_KV * 128, qf, o, m_run, l_run, scale_log2e, 0, N, lr, lh, g16, tq, tp);
      slot = 1;
      kt = 1;
    }
    for (; kt < nfull; ++kt) {
      tile_ready(kt);
      const char* sK = smem + slot * (2 * AT_KV * 128);
      if (active) attn_tile<0, AT_NQ, FIX>(sK, sK + AT_KV * 128, qf, o, m_run, l_run, scale_log2e, kt * AT_KV, N, lr, lh, g16, tq, tp);
      slot = slot == 2 ? 0 : slot + 1;
    }
    if (nfull < nkt) {      // the last tile, 1..63 keys: nothing left to stage
      tile_ready(nfull);
      const char* sK = smem + slot * (2 * AT_KV * 128);
      if (active) {
        if (DIET && N - nfull * AT_KV <= 32) attn_tile<2, AT_NQ, FIX>(sK, sK + AT_KV * 128, qf, o, m_run, l_run, scale_log2e, nfull * AT_KV, N, lr, lh, g16, tq, tp);
        else attn_tile<1, AT_NQ, FIX>(sK, sK + AT_KV * 128, qf, o, m_run, l_run, scale_log2e, nfull * AT_KV, N, lr, lh, g16, tq, tp);
      }
    }
  };
  // the rows `sel` of this lane leave as O / l_tot
  auto store_rows = [&](const float (&l_tot)[AT_NQ], const bool (&sel)[AT_NQ]) __attribute__((always_inline)) {
#pragma unroll
    for (int qi = 0; qi < AT_NQ; ++qi) {
      const float inv = 1.0f / l_tot[qi];
      const int q = q0 + qi * 32 + lr;
      const bool okq = active && q < q_hi && sel[qi];
      if (MX) {
        // block db of this head = columns db*32 .. +31 of query q: 16 of them in this lane, 16 in lane ^ 32 (every lane takes part in the shuffle;
        // only the stores are predicated)
        unsigned char* op8 = reinterpret_cast<unsigned char*>(ctx) + ((size_t)b * N + q) * D + h * 64;
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          float amax = 0.f;
#pragma unroll
          for (int r = 0; r < 16; ++r) amax = fmaxf(amax, fabsf(o[qi][db][r] * inv));
          amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
          const unsigned eb = mx_ebyte(amax);
          const float sc = inv * mx_inv_scale(eb);
          if (okq) {
#pragma unroll
            for (int g = 0; g < 4; ++g)
              *reinterpret_cast<unsigned*>(op8 + db * 32 + 8 * g + 4 * lh) = pack4_fp8(o[qi][db][4 * g] * sc, o[qi][db][4 * g + 1] * sc, o[qi][db][4 * g + 2] * sc, o[qi][db][4 * g + 3] * sc);
            if (lh == 0) bs[((size_t)b * N + q) * (D >> 5) + mx_scale_off(D, h * 2 + db)] = (unsigned char)eb;
          }
        }
      } else if (okq) {
        bf16_t* op = ctx + ((size_t)b * N + q) * D + h * 64;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            uint2 pk;
            pk.x = pack2bf(o[qi][db][4 * g] * inv, o[qi][db][4 * g + 1] * inv);
            pk.y = pack2bf(o[qi][db][4 * g + 2] * inv, o[qi][db][4 * g + 3] * inv);
            *reinterpret_cast<uint2*>(op + db * 32 + 8 * g + 4 * lh) = pk;
          }
      }
    }
  };
  auto write_stamps = [&]() __attribute__((always_inline)) {
    if (stamps && tid == 0) {
      unsigned long long* o_ = stamps + (size_t)blockIdx.x * 6;
      o_[0] = __builtin_amdgcn_s_memtime() - t_begin; o_[1] = t_wait; o_[2] = nkt; o_[3] = active ? 1 : 0;
      o_[4] = rt_entry; o_[5] = __builtin_amdgcn_s_memrealtime();
    }
    stamps = nullptr;      // the first pass only
  };

  float l_tot[AT_NQ];
  bool redo[AT_NQ];      // rows the running-maximum pass (re)computes and stores
  if (stamps) t_begin = __builtin_amdgcn_s_memtime();
  // fixed_ref = 0 (test option "attn_fixed_ref"): every row goes through the running-maximum pass and nothing runs in front of it -- the
  // arithmetic before the reference form existed, from this same instantiation.  A sequence of one key tile has no tile behind the first.
  if (fixed_ref && nkt > 1) {
    pass(std::true_type{});
    write_stamps();
    // Did a row outgrow its reference?  Taken ONCE, here, not per tile.  A row is bad when its normaliser (both halves) is not below
    // AT_REF_LMAX or one of its 64 accumulators is not finite: chk = sum of o * 0 is (+-)0 when every o is finite and NaN otherwise, and goes
    // through the same combine as l (l + 0 = l: a good row's l_tot keeps today's bits).
    int any_bad = 0;
#pragma unroll
    for (int qi = 0; qi < AT_NQ; ++qi) {
      float c0 = 0.f, c1 = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) { c0 = fmaf(o[qi][0][r], 0.f, c0); c1 = fmaf(o[qi][1][r], 0.f, c1); }
      const float lc = l_run[qi] + (c0 + c1);
      l_tot[qi] = lc + __shfl_xor(lc, 32, 64);
      redo[qi] = !(l_tot[qi] < AT_REF_LMAX);      // a row's two half-lanes agree: l_tot is the same sum in both
      any_bad |= redo[qi] ? 1 : 0;
    }
    // the workgroup's vote: one LDS word per wave, one barrier.  The barrier also puts every wave behind its last tile: the ring is free.
    const int wave_bad = __builtin_amdgcn_readfirstlane(__any(any_bad) ? 1 : 0);
    int* const vote = reinterpret_cast<int*>(smem + AT_RING_BYTES);
    if (lane == 0) vote[wid] = wave_bad;
    bool good[AT_NQ];
#pragma unroll
    for (int qi = 0; qi < AT_NQ; ++qi) good[qi] = !redo[qi];
    store_rows(l_tot, good);
    __syncthreads();
    const int wg_bad = __builtin_amdgcn_readfirstlane(vote[0] | vote[1] | vote[2] | vote[3]);
    if (!wg_bad) return;      // every workgroup of ordinary activations ends here: the path costs the vote
    if (tid == 0) atomicAdd(&g_attn_reruns, 1u);
  } else {
#pragma unroll
    for (int qi = 0; qi < AT_NQ; ++qi) redo[qi] = true;
  }
  // The workgroup restages from tile 0 and runs the running-maximum pass for all of its rows, but stores ONLY the bad ones (per lane): a row's
  // bits depend on its own q and its image's K/V alone -- not on its workgroup mates, not on the body (32 or 64 rows per wave), not on the batch.
  pass(std::false_type{});
  write_stamps();
#pragma unroll
  for (int qi = 0; qi < AT_NQ; ++qi) l_tot[qi] = l_run[qi] + __shfl_xor(l_run[qi], 32, 64);
  store_rows(l_tot, redo);
}

template <int AT_NQ, bool MX, bool DIET>
__global__ __launch_bounds__(256, 2) void attn_bf16_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ ctx,
                                                        int N, int heads, int npairs, float scale_log2e, int q_lo, int q_hi, unsigned char* __restrict__ bs, int fixed_ref) {
  attn_bf16_body<AT_NQ, MX, DIET>(blockIdx.x, qkv, ctx, N, heads, npairs, scale_log2e, q_lo, q_hi, bs, fixed_ref);
}
// ONE launch for a sequence whose last 256-row block is short (N = 1370: 5 blocks + 90 rows): workgroups [0, main_blocks) run the
// 64-rows-per-wave body over rows [0, q_main), the workgroups behind them the 32-rows-per-wave body over the remainder -- dispatched
// last, they fill the main part's end-of-kernel bubble instead of costing a launch of their own (round 3: the separate tail launch
// took 62.6 us per layer for 6.6 % of the rows, profiles/r03_bench_bf16_kernel_stats.csv).  main_blocks % 8 == 0 keeps both XCD maps.
template <bool MX, bool DIET>
__global__ __launch_bounds__(256, 2) void attn_bf16_fused_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ ctx,
                                                              int N, int heads, int npairs, float scale_log2e, int main_blocks, int q_main, unsigned char* __restrict__ bs, int fixed_ref) {
  if ((int)blockIdx.x < main_blocks) attn_bf16_body<2, MX, DIET>(blockIdx.x, qkv, ctx, N, heads, npairs, scale_log2e, 0, q_main, bs, fixed_ref);
  else attn_bf16_body<1, MX, DIET>((int)blockIdx.x - main_blocks, qkv, ctx, N, heads, npairs, scale_log2e, q_main, N, bs, fixed_ref);
}

// (Round 4 built a 512-thread PING-PONG form of this kernel -- both waves of every SIMD in one workgroup, phased against each other with the
// workgroup barrier so that one group's MFMA phase (P V of the previous tile, K Q^T of the next) meets the other group's softmax; the groups split
// the keys and merge (m, l, O) through LDS at the end.  The probe says such phases overlap (tools/probes/mfma_valu_overlap.hip mode 16: 1 088 /
// 1 974 cycles side by side); the kernel was parity-green and 26 % SLOWER (attention 6.52 -> 8.25 ms per batch-64 step, tools/experiments/r4_exp19.sh):
// one workgroup per CU (2 x 48 KiB of rings) exposes every workgroup's prologue and merge, the MFMA phase carries six LDS round trips that two
// free-running workgroups hide from each other, and every phase lasts as long as its slower half.  Not kept.)
#ifdef DINODET_TUNING
extern "C" int dod_debug_attn_stamps(void* dev_buf) {
  unsigned long long* p = (unsigned long long*)dev_buf;
  return hipMemcpyToSymbol(HIP_SYMBOL(g_attn_stamps), &p, sizeof(p)) == hipSuccess ? 0 : 4;
}
#endif

// the kernel of a launch: NQ = 1 / 2 query blocks per wave, 0 = the fused kernel; every form has the same parameters
typedef void (*attn_kern_t)(const bf16_t*, bf16_t*, int, int, int, float, int, int, unsigned char*, int);
template <int NQ>
static attn_kern_t attn_pick(bool mx, bool diet) {
  if constexpr (NQ == 0) return mx ? (diet ? attn_bf16_fused_kernel<true, true> : attn_bf16_fused_kernel<true, false>)
                                   : (diet ? attn_bf16_fused_kernel<false, true> : attn_bf16_fused_kernel<false, false>);
  else return mx ? (diet ? attn_bf16_kernel<NQ, true, true> : attn_bf16_kernel<NQ, true, false>)
                 : (diet ? attn_bf16_kernel<NQ, false, true> : attn_bf16_kernel<NQ, false, false>);
}
static std::atomic<long> g_attn_half_tiles{0};
long attn_half_tile_count() { return g_attn_half_tiles.load(); }
long attn_rerun_count() {      // a synchronising copy: a test facility, not on the forward path
  unsigned int v = 0;
  return hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_attn_reruns), sizeof(v)) == hipSuccess ? (long)v : -1;
}

int launch_attn_bf16(const bf16_t* qkv, bf16_t* ctx, int B, int N, int heads, float scale, hipStream_t s, unsigned char* ctx_bs) {
  if (B <= 0 || N <= 0 || heads <= 0) return 1;
  if (ctx_bs && (heads * 64) % 64 != 0) return 2;
  const bool mx = ctx_bs != nullptr;
  const int npairs = B * heads, pairs8 = (npairs + 7) / 8 * 8;
  const float c = scale * 1.44269504088896340736f;
  const bool diet = dod_option(DOD_OPT_ATTN_DIET) != 0;                  // 0: the full-width tail tile and pointer staging (bit-identical)
  const int fixed_ref = dod_option(DOD_OPT_ATTN_FIXED_REF) != 0;         // 0: the running row maximum for every row
  if (diet && (N - 1) % AT_KV < 32) ++g_attn_half_tiles;                 // the last key tile holds 1..32 keys
  // 64 query rows per wave once the grid still fills the chip several times over (measured: +5 % at B*heads = 768,
  // -12 % at 96), else 32
  static const char* nqe = DOD_TUNE_ENV("DINODET_ATTN_NQ");   // tuning override
  if (nqe ? nqe[0] == '2' : (long)npairs * ((N + 255) / 256) >= 4 * 256) {
    // A workgroup lasts as long as its busiest wave: the last 256-row block of N = 1370 (90 rows) keeps one wave fully busy and costs a
    // whole block time for a third of the rows.  When the remainder fits 128 rows it goes to a second launch of the 32-rows-per-wave
    // kernel (three waves with one q-block each: about half a block time): 5 + 0.55 instead of 6 block times per (image, head).
    const int rem = N % (AT_WAVES * 64);
    static const char* tse = DOD_TUNE_ENV("DINODET_ATTN_TAILSPLIT");
    const bool split = (tse ? tse[0] != '0' : true) && rem > 0 && rem <= AT_WAVES * 32 && N > AT_WAVES * 64;
    const int q_main = split ? N - rem : N;
    const int nqb = (q_main + AT_WAVES * 64 - 1) / (AT_WAVES * 64);
    static const char* fse = DOD_TUNE_ENV("DINODET_ATTN_FUSED_TAIL");      // "0": the two-launch form (A/B)
    if (split && !(fse && fse[0] == '0')) {
#ifdef DINODET_TUNING
      // tuning builds: DINODET_ATTN_LDS_PAD = bytes of unused dynamic LDS per workgroup (64 KiB leaves ONE workgroup per CU: one wave per SIMD)
      static const int pad = [] { const char* v = getenv("DINODET_ATTN_LDS_PAD"); return v ? atoi(v) : 0; }();
      if (pad > 0 && !mx) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_bf16_fused_kernel<false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, pad);
        hipLaunchKernelGGL((attn_bf16_fused_kernel<false, true>), dim3(pairs8 * nqb + pairs8), dim3(256), pad, s, qkv, ctx, N, heads, npairs, c, pairs8 * nqb, q_main, ctx_bs, fixed_ref);
        return hipGetLastError() == hipSuccess ? 0 : 3;
      }
#endif
      hipLaunchKernelGGL(attn_pick<0>(mx, diet), dim3(pairs8 * nqb + pairs8), dim3(256), 0, s, qkv, ctx, N, heads, npairs, c, pairs8 * nqb, q_main, ctx_bs, fixed_ref);
    } else {
      hipLaunchKernelGGL(attn_pick<2>(mx, diet), dim3(pairs8 * nqb), dim3(256), 0, s, qkv, ctx, N, heads, npairs, c, 0, q_main, ctx_bs, fixed_ref);
      if (split) hipLaunchKernelGGL(attn_pick<1>(mx, diet), dim3(pairs8), dim3(256), 0, s, qkv, ctx, N, heads, npairs, c, q_main, N, ctx_bs, fixed_ref);
    }
  } else {
    const int nqb = (N + AT_WAVES * 32 - 1) / (AT_WAVES * 32);
    hipLaunchKernelGGL(attn_pick<1>(mx, diet), dim3(pairs8 * nqb), dim3(256), 0, s, qkv, ctx, N, heads, npairs, c, 0, N, ctx_bs, fixed_ref);
  }
  return hipGetLastError() == hipSuccess ? 0 : 3;
}
