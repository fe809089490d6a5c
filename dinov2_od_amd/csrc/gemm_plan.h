// Inference GEMM dispatch, stated once: which kernel form runs an inference linear, on which rows, with how many K slices.
// gemm_plan() is a pure function of (family, shape, what the policy reads of the epilogue, GemmPolicy): it calls no HIP runtime function and
// reads no global or environment state, so dod_test_gemm_plan (include/dinodet.h) answers for any shape and any CU count without a device.
// gemm_dispatch.hip gathers the GemmPolicy and executes the steps; the files that own the kernels only launch the form they are handed.
// The measurements quoted beside a rule are the reason for it (tools/bench_pp.py, bench_small_m.py, bench_h2.py, bench.py); MI355X, 256 CUs.
#pragma once
#include "dod_common.h"

enum { FORM_KSPLIT_REDUCE = FORM_COUNT };                          // step only: the tail split's reduce + epilogue launch (counted under no form)

// What the policy reads of a GemmEpi (gemm_plan_epi_flags, gemm_dispatch.hip).  Nothing else of the epilogue may influence the plan.
enum { PE_GELU = 1 << 0, PE_SIGMOID = 1 << 1,       // act == ACT_GELU / ACT_SIGMOID
       PE_ROWMAP = 1 << 2,                          // rows_per_img != 0
       PE_A_SCALE = 1 << 3,                         // a_scale (fp8 per-row scales)
       PE_OUT_SPLIT3 = 1 << 4,                      // out_split > 0
       PE_KSPLIT = 1 << 5,                          // ksplit > 1
       PE_ROWS_OK = 1 << 6,                         // gemm_epi_rows_ok(e): the epilogue of a row range can run as a launch of its own
       PE_REGMATH_OK = 1 << 7,                      // epi_regmath_ok(e, N): plain bf16 rows the register epilogue can write (never with glu)
       PE_A_BS = 1 << 8, PE_W_BS = 1 << 9, PE_OUT_BS = 1 << 10,      // fp8 block scales of A / W / the gated output
       PE_ALLOW_KSPLIT = 1 << 11 };                 // fp32: the caller allows the K split across workgroups

// Tuning-build overrides (gemm_tune(), gemm_dispatch.hip); these defaults = "unset" = the release build
struct GemmTune {
  char tile = 0;             // DINODET_GEMM_TILE: plain bf16 "q" ping-pong, "x" 16-wave k64, "8" 256x128, "1" 128x128
  char x3_tile = 0;          // DINODET_X3_TILE: split product "p" ping-pong / "w" 16-wave
  int rem_div = 6;           // DINODET_GEMM_REMCUT: the remainder cut takes a last round of at most CUs / rem_div tiles (0: off)
  double m16_bias = 1.02;    // DINODET_GEMM_M16_BIAS: > 1 favours the 256x256 tiles in the round rule
  int ring = 1;              // DINODET_GEMM_RING: 0 = never the 3-slot ring
  int k0frac = 0;            // DINODET_GEMM_KSPLIT0 = n: plain bf16 takes the underfilled-grid K split up to CUs * n / 12 tiles
  int tailsplit = 1;         // DINODET_GEMM_TAILSPLIT: 0 off, 1 the shipped heuristic, 2 every qualifying shape (the test option wins)
  int fp8_big = 1;           // DINODET_FP8_TILE: 0 = 256x128 everywhere, 2 = not for the gated weights_in
  int f32_ksplit = 1;        // DINODET_F32_KSPLIT: 0 = off, > 1 = the workgroups aimed at for 16 m-tiles
};

struct GemmPolicy {
  int cus = 256;             // CU count of the current device
  size_t tail_bytes = 0;     // tail-split scratch reserved, bytes per slab (gemm_tail_reserve)
  bool f32_slab = false;     // the fp32 K split's slab exists (gemm_f32_ksplit_reserve)
  int opt_tailsplit = -1, opt_f32_ksplit = -1, opt_epi_regmath = -1;      // DOD_OPT_* test options, -1 = unset
  GemmTune tune;
};

struct GemmStep {
  int form;                  // FORM_*, or FORM_KSPLIT_REDUCE
  int row0, rows;            // rows [row0, row0 + rows) of the call
  int kslices;               // K slices (grid.y) of a K-split launch and of its reduce; 1 otherwise
  int regmath;               // FORM_K64: the register epilogue
  int gm;                    // grouped-order depth of the forms that compute one (FORM_BF16_M16, the fp8 forms); 0 otherwise
};
struct GemmPlan {            // in launch order: at most main rows cut in two by the remainder cut, the K-split launch, the reduce launch
  int n = 0;
  GemmStep step[4];
  void add(int form, int row0, int rows, int kslices = 1, int regmath = 0, int gm = 0) { if (n < 4) step[n] = GemmStep{form, row0, rows, kslices, regmath, gm}; ++n; }
};

// scratch of the fp32 K split (gemm_f32.hip): a slab holds counters of F32K_TILES tiles and partials of F32K_PARTS (tile, slice) pairs
#define F32K_TILES 4096
#define F32K_PARTS 1536

namespace gemm_plan_detail {
inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline int wide_gm(int N) { return N >= 3072 ? 8 : (N >= 2048 ? 4 : 2); }      // measured on the 256x128 kernel: 8 for N = 3072, 4 for 2304, 2 for 768

// ---- plain bf16, the small-M rules: 256x128x32 on v_mfma_f32_16x16x32_bf16 (two workgroups per CU) from 1 024 rows up, 128x128 for small M (decoder
// memory at small batch, tests) -- and for a grid of a few dozen 256x128 tiles (the decoder's query-side linears: B*Q = 3 200 rows at batch 32 -> 78
// workgroups walking K' = 3K = 2 304), which leaves most CUs idle while one workgroup per CU pulls its operands at the per-CU staging rate whatever its
// tile: the 128x128 kernel puts the same bytes on twice as many CUs (tools/bench_small_m.py, M = 3200: N = 768 41.5 -> 30.9 us, N = 1024
// 42.7 -> 31.9, K = 3072 53.9 -> 38.7; N = 2304 (234 tiles) 47.8 vs 48.4: stays).  Also what the cut rows of a remainder cut run as.
inline void bf16_small(int row0, int M, int N, int K, const GemmPolicy& p, GemmPlan& out) {
  const char force = p.tune.tile;
  const bool few = (long)cdiv(M, 256) * cdiv(N, 128) * 2 <= 256 + 64;
  if (force ? force == '8' : (M >= 1024 && N >= 128 && !few)) { out.add(FORM_BF16_M16, row0, M, 1, 0, wide_gm(N)); return; }
  // a grid of at most one workgroup per CU has nothing beside it to hide its DMA latency: the 3-slot ring (two K-tiles in flight)
  const int tiles = cdiv(M, 128) * cdiv(N, 128);
  out.add(p.tune.ring && tiles <= p.cus && K >= 3 * 64 ? FORM_BF16_128_R3 : FORM_BF16_128_R2, row0, M);
}

// ---- plain bf16 without the tail split (also: the main rows of one)
inline void bf16_rows(int M, int N, int K, unsigned epi, const GemmPolicy& p, GemmPlan& out) {
  const char force = p.tune.tile;
  const int cu = p.cus;
  const int regmath = p.opt_epi_regmath != 0 && (epi & PE_REGMATH_OK);      // plain bf16 rows (QKV, fc1 of the bf16 mode): the register epilogue
  if (force == 'q' && K % 64 == 0) { out.add(FORM_PPM, 0, M); return; }
  if (force == 'x') { out.add(FORM_K64, 0, M, 1, regmath); return; }
  if (!force && M >= 4096 && N >= 512 && K % 64 == 0 && !(epi & (PE_SIGMOID | PE_ROWMAP))) {
    // Round-aware choice between the 256x256 tiles (one workgroup per CU: the 16-wave `k64` kernel of gemm_x3.hip -- 256x256x64, two 64-KiB
    // slots: QKV 760 / out-proj 460 / fc2 765 TFLOP/s at M = 87 680 -- or the 8-wave ping-pong kernel of gemm_pp.hip, 3-7 % faster on
    // N >= 1536 at every M measured) and the 256x128 tile (`m16`, two co-resident workgroups per CU that run at about half speed each, so
    // one of its tiles costs ~0.55 of a 256x256 tile only while a CU holds a single one).  Cost in units of a 256x256 tile time = rounds
    // of CUs x tile cost; a GELU epilogue costs the one-workgroup-per-CU kernels ~8 % (nothing overlaps it).
    // tools/bench_pp.py --rows {4112, 8224, 16448, 21920, 43840, 87680}: the rule reproduces the faster kernel in 27 of 28 cases
    // (M = 8224, batch 32 at 224x224: QKV 46 vs 53 us, out-proj 27 vs 32, fc1 66 vs 78, fc2 59 vs 75).
    const long tm = cdiv(M, 256), t_big = tm * cdiv(N, 256), t_small = tm * cdiv(N, 128);
    const double c_big = (double)((t_big + cu - 1) / cu) * ((epi & PE_GELU) ? 1.08 : 1.0);
    const double c_small = (double)((t_small + cu - 1) / cu) * (K >= 2048 ? 0.62 : 0.55);      // long K: the smaller tile's lower FLOP per staged byte shows
    // Round 4: with its epilogue passes written out the 16-wave kernel holds its accumulators in registers (it had spilled 34 of them since
    // round 1) and is the fastest choice for EVERY wide GEMM (N >= 1536: QKV, fc1 incl. its GELU epilogue) at every M measured
    // (tools/bench_pp.py, rows 8 224 / 10 960 / 43 840 / 87 680: QKV 46.9 / 53.2 / 173.0 / 338.2 us against 51.8 / 56.8 / 186.6 / 345.5 for the
    // round-3 choice, fc1 59.9 / 87.7 / 264.2 / 518.9 against 63.8 / 104.7 / 297.9 / 548.4); the narrow ones (N = 768) keep the round rule
    // below, and the long-K narrow one (fc2) the ping-pong kernel behind its tail split.
    if (N >= 1536 && K < 2048) {
      // The remainder cut.  A last round of a few tiles costs these short-K GEMMs a whole tile time when the grid is only one or two rounds deep
      // (32 images of 224^2: QKV = 33 x 9 = 297 = one round + 41).  The m-tiles of that round are cut off and run as a launch of their own, which
      // the small-M rules spread over the chip as 128-row tiles.
      // Window CUs / 16 <= rem <= CUs / rem_div (rem >= CUs / 16: a handful of lone tiles finish at well under a tile time -- and a second stream's
      // kernels fill the idle CUs -- so cutting them costs more than it saves: 2 x 4 images of 518^2, fc1 = 264 tiles = one round + 8, 1 737 against
      // 1 794 images/s with the cut; 8 images of 518^2, fc1 = 43 x 12 = 516 tiles = two rounds + 4, is below the window too and is NOT cut -- the
      // comment that stood here before the planner listed it as an example of the cut, which the rule never made)
      const long rounds = t_big / cu, rem = t_big % cu;
      const int rem_div = p.tune.rem_div;
      if (rounds >= 1 && rounds <= 2 && rem * 16 >= cu && rem_div > 0 && rem * rem_div <= cu && (epi & PE_ROWS_OK)) {
        const int Mmain = (int)((rounds * cu) / cdiv(N, 256)) * 256, R = M - Mmain;
        if (Mmain >= 2048 && R > 0 && R < 2048) {
          out.add(FORM_K64, 0, Mmain, 1, regmath);
          bf16_small(Mmain, R, N, K, p, out);
          return;
        }
      }
      out.add(FORM_K64, 0, M, 1, regmath);
      return;
    }
    if (c_big <= c_small * p.tune.m16_bias) {
      if (K >= 2048) out.add(FORM_PPM, 0, M);
      else out.add(FORM_K64, 0, M, 1, regmath);
      return;
    }
    out.add(FORM_BF16_M16, 0, M, 1, 0, wide_gm(N));
    return;
  }
  bf16_small(0, M, N, K, p, out);
}

// ---- split product without the tail split: the 8-wave ping-pong kernel (gemm_pp.hip) wherever a workgroup's K loop or column count is long enough
// to pay for its 512-thread epilogue: measured at M = 87680 against the 16-wave kernel -- QKV 400 vs 378, fc1 376 vs 363, fc2 406 vs 371 TFLOP/s
// algorithmic; out-proj (N = K = 768) 276 vs 293.  Round 4, after both kernels' epilogues were rewritten: the ping-pong kernel wins out-proj too
// -- 337.6 vs 345.1 us at M = 87 680, 183.0 vs 185.8 at 43 840, 58.0 vs 59.6 at 10 960 -- so every large-M split product takes it.
inline void x3_rows(int M, const GemmPolicy& p, GemmPlan& out) {
  out.add((p.tune.x3_tile ? p.tune.x3_tile == 'p' : M >= 4096) ? FORM_X3_PP : FORM_X3_16W, 0, M);
}

// ---- the wave-quantisation tail split of the 256x256-tile GEMMs; kind = family (GEMM_BF16 / GEMM_X3 / GEMM_H2).  One 256x256 tile per CU and
// round: 343 x 3 = 1029 tiles of an N = 768 GEMM at M = 87680 take FIVE rounds on 256 CUs for 4.02 rounds of work (tools/pp_timeline.py: kernel span
// = 5 tile times).  The rows of the short last round are cut off the main launch, their tiles K-split S ways in ONE launch of the family's
// ping-pong kernel (grid.y = slice: S CUs per tile, fp32 partial slabs of R x N floats each in the reserved scratch), and a reduce + epilogue
// launch sums the slabs in slice order.  false: the shape does not qualify and the family's own rules take all rows.
inline bool tail_split(int kind, int M, int N, int K, unsigned epi, const GemmPolicy& p, GemmPlan& out) {
  if (epi & (PE_KSPLIT | PE_ROWMAP | PE_A_SCALE | PE_OUT_SPLIT3)) return false;
  const int mode = p.opt_tailsplit >= 0 ? p.opt_tailsplit : p.tune.tailsplit;      // 0 off, 1 the shipped heuristic, 2 every qualifying shape
  if (mode == 0) return false;
  const int ktile = kind == GEMM_BF16 ? 64 : 32;
  if (N % 4 != 0 || K % ktile != 0) return false;
  const int CU = p.cus;
  const int tiles_n = cdiv(N, 256), tiles = cdiv(M, 256) * tiles_n;
  const int nk = K / ktile;
  const bool force = mode == 2;
  int Mmain, R, S = 0;
  auto slices = [&](int tiles_r) {        // the kernel's precondition: K divisible by S * ktile, at least three K-tiles per slice; tiles x S fills at most the chip
    for (int c : {8, 6, 4, 3, 2})
      if (nk % c == 0 && nk / c >= 3 && tiles_r * c <= CU) return c;
    return 0;
  };
  // plain bf16 has a 256x128 tile for underfilled grids and does NOT take case (a) by default.  Round 3 tried it on the decoder's query-side
  // linears (M = B*Q = 3 200 rows at batch 32: 39 tiles of 256x256 walking K' = 3K = 2 304, 48.5 us on 78 CUs as 256x128 tiles): six slices per
  // tile (234 workgroups) + the reduce launch write and re-read 59 MB of fp32 partials, and the forward gains nothing (`bench.py --workload
  // vitb224`: 7 539 vs 7 571 images/s, vitb518 2 241.7 both ways).  Tuning builds: k0frac = n enables it for grids of at most CUs * n / 12 tiles.
  if (M >= 2048 && (kind != GEMM_BF16 ? tiles * 2 <= CU + CU / 8 : tiles * 12 <= CU * p.tune.k0frac)) {
    // (a) an UNDERFILLED single round (the compensated kernels have no smaller tile): 99 tiles of an N = 768 GEMM at M = 8224 leave 157
    // CUs idle -- every tile is K-split so that tiles x S fills the chip (no main launch)
    Mmain = 0; R = M;
    S = slices(tiles);
  } else {
    // (b) a short LAST round.  Measured at M = 87680 (343 x 3 tiles, 4.02 rounds; tools/bench_h2.py, tools/bench_pp.py with
    // DINODET_GEMM_TAILSPLIT=0 / 2): the unsplit kernels last ~4.3 tile times, not 5 -- the five tiles of the last round run alone on
    // the chip -- so the split pays where a tile is long: fc2 (K = 3072) 976 vs 1047 us (split product), 866 vs 944 (H2), 474 vs 491
    // (plain bf16); out-proj (K = 768) 367 vs 373, 346 vs 350, 218 vs 217: not worth a second and third launch.  Enabled at K >= 2048
    // (mode 2 forces every qualifying shape).
    // (with the engine's two concurrent micro-batches the other stream's kernels fill the last-round bubble anyway: fp16x2 at 2 x 32
    // images 1 198 images/s with the split, 1 208 without; so case (b) is kept for the launches that only a single-stream forward of a
    // large batch makes, M >= 65536 rows)
    const int rounds = tiles / CU, rem = tiles % CU;
    // (round 4) a grid one or two rounds deep whose last round is 6-16 % full -- the compensated QKV at 32 images of 224^2: 33 x 9 = 297 tiles --
    // loses most of a tile time to it at any K (bench.py --workload vitb224: bf16x3 4 953 -> 5 015 images/s, fp16x2 5 258 -> 5 318; a fuller or
    // emptier last round, e.g. 2 x 4 images of 518^2, gains nothing).  The plain bf16 kernels cut those rows off instead (bf16_rows).
    const bool shallow = kind != GEMM_BF16 && M >= 4096 && rounds >= 1 && rounds <= 2 && rem * 16 >= CU && rem * 6 <= CU;
    if (M < 8192 && !shallow) return false;
    if (!force && !shallow && (K < 2048 || M < 65536)) return false;
    if (rounds < 1 || rounds > 6 || rem == 0) return false;
    Mmain = (rounds * CU) / tiles_n * 256; R = M - Mmain;
    if (R <= 0) return false;
    S = slices(cdiv(R, 256) * tiles_n);
    // worth it when the last round shrinks from one tile time to 1/S of one (+ ~1/4 for the slab round trip and the two extra
    // launches) and that is >= 4 % of the kernel: 1029 tiles (4 rounds + 5: S = 8) and 344 tiles (1 round + 88: S = 2) both qualify
    if (S >= 2 && (1.0 - 1.0 / S - 0.25) < 0.04 * (rounds + 1)) S = 0;
  }
  if (S < 2) return false;
  if (p.tail_bytes < (size_t)R * N * S * 4) return false;           // reserved outside stream capture (gemm_tail_reserve)
  if (Mmain > 0) {                                                  // main rows: the family's own rules, without this split
    if (kind == GEMM_BF16) bf16_rows(Mmain, N, K, epi, p, out);
    else if (kind == GEMM_X3) x3_rows(Mmain, p, out);
    else out.add(FORM_H2, 0, Mmain);
  }
  out.add(kind == GEMM_H2 ? FORM_H2 : (kind == GEMM_X3 ? FORM_X3_PP : FORM_PPM), Mmain, R, S);
  out.add(FORM_KSPLIT_REDUCE, Mmain, R, S);
  return true;
}
}  // namespace gemm_plan_detail

inline GemmPlan gemm_plan(int family, int M, int N, int K, unsigned epi, const GemmPolicy& p) {
  using namespace gemm_plan_detail;
  GemmPlan out;
  switch (family) {
    case GEMM_BF16:
      // the 256x256-tile shapes: a short last round (M >= 8192), or a grid of a few dozen tiles (M >= 2048)
      if (!p.tune.tile && M >= 2048 && N >= 512 && !(epi & (PE_GELU | PE_SIGMOID | PE_ROWMAP)) && K % 64 == 0 && tail_split(GEMM_BF16, M, N, K, epi, p, out)) break;
      bf16_rows(M, N, K, epi, p, out);
      break;
    case GEMM_X3:
      if (!tail_split(GEMM_X3, M, N, K, epi, p, out)) x3_rows(M, p, out);
      break;
    case GEMM_H2:
      if (!tail_split(GEMM_H2, M, N, K, epi, p, out)) out.add(FORM_H2, 0, M);
      break;
    case GEMM_FP8: {
      // both operands block-scaled, a grid of several rounds of 256x256 tiles: the one-workgroup-per-CU tile (fewer staged bytes per MAC)
      const int big = p.tune.fp8_big;
      int form = FORM_FP8_ROWS;
      if (epi & PE_A_BS)
        form = !(epi & PE_W_BS) ? FORM_FP8MX_256X128
             : (big && !(big == 2 && (epi & PE_OUT_BS)) && M >= 4096 && N >= 512) ? FORM_FP8MX2_256X256 : FORM_FP8MX2_256X128;
      out.add(form, 0, M, 1, 0, wide_gm(N));
      break;
    }
    case GEMM_F32: {
      // K split across workgroups (gemm_f32.hip).  The slice count S is chosen from (N, K) alone, so that the row count does not change a row's
      // bits while the split runs (micro-batches, single-image launches); the split is DROPPED -- S = 1, another summation order -- when tiles x S
      // exceeds the slab (F32K_PARTS), which does depend on M.  The callers that allow the split send at most ~16 m-tiles of N >= 128 here (larger
      // row counts take the bf16 split-3 form, dod_forward.hip qlinear); the narrow heads (N < 128) cross the limit above 8 192 rows.  Aim: two
      // workgroups per CU for 16 m-tiles, at least 8 k-tiles per slice, at most 8 slices.
      bool allow = (epi & PE_ALLOW_KSPLIT) != 0;
      if (p.opt_f32_ksplit == 0) allow = false; else if (p.opt_f32_ksplit == 1) allow = true;      // test hook
      int S = 1;
      const int mode = p.tune.f32_ksplit;
      if (allow && mode && !(epi & PE_ROWMAP)) {
        const int tiles_n = cdiv(N, 64), tiles = cdiv(M, 64) * tiles_n, nk = cdiv(K, 16);
        const int target = mode > 1 ? mode : 512;      // workgroups aimed at for 16 m-tiles
        int want = (target + 8 * tiles_n) / (16 * tiles_n);      // rounded: N = 768 (12 n-tiles) -> 3
        want = want > 8 ? 8 : want;
        want = want > nk / 8 ? nk / 8 : want;
        if (want >= 2 && tiles <= F32K_TILES && (long)tiles * want <= F32K_PARTS && p.f32_slab) S = want;
      }
      out.add(FORM_F32, 0, M, S);
      break;
    }
  }
  return out;
}

// The steps tile [0, M) exactly and in order; a reduce step sums the slabs of the K-split step just before it, over the same rows, and every such
// K-split step has one.  The executor rejects any other plan before its first launch: a wrong plan is a rejected call, never a kernel on rows
// that are not there.
inline bool gemm_plan_tiles(const GemmPlan& pl, int M) {
  if (pl.n < 1 || pl.n > 4) return false;
  int next = 0;
  for (int i = 0; i < pl.n; ++i) {
    const GemmStep& st = pl.step[i];
    if (st.rows <= 0 || st.kslices < 1) return false;
    if (st.form == FORM_KSPLIT_REDUCE) {
      if (i == 0) return false;
      const GemmStep& ks = pl.step[i - 1];
      if (ks.form == FORM_KSPLIT_REDUCE || ks.kslices < 2 || ks.kslices != st.kslices || ks.row0 != st.row0 || ks.rows != st.rows) return false;
      continue;
    }
    if (st.row0 != next) return false;
    next += st.rows;
    if (st.kslices > 1 && st.form != FORM_F32 && (i + 1 >= pl.n || pl.step[i + 1].form != FORM_KSPLIT_REDUCE)) return false;
  }
  return next == M;
}

// gemm_dispatch.hip: a GemmPolicy of the given device facts + the process-wide test options and tuning overrides, as the launchers gather it
GemmPolicy gemm_policy(int cus, size_t tail_bytes, bool f32_slab);
