// Boxes drawn into the image batch on device: up to two layers (ground truth below, predictions above) of outlined, optionally
// alpha-filled and captioned rectangles rendered into a fresh uint8 [B, H, W, 3] batch (include/dinodet.h dod_draw_detections states
// the contract; tests/draw_cases.py restates it in numpy).  One launch, no host synchronisation, no atomics: a gather, not a scatter,
// so every output byte is a function of the input bits alone.
//
// One workgroup of 256 threads owns a tile of 64 x 16 pixels of one image:
//   1. cull: the layers' rows in painter's order (layer 0 rows count-1 .. 0, then layer 1 likewise), 256 per round.  A thread turns
//      its row into the pixel rectangle and, with captions on, the caption rectangle, and keeps it when either touches the tile.  The
//      kept rows are compacted IN ORDER (ballot + population count per wave, wave totals through LDS) into a list of records in LDS:
//      rectangle (4 x int16), colour + caption length, and a word naming the row and its text.  2 x 1024 records fit.
//   2. the tile's input rows are staged in LDS by aligned dword loads (uint8 form; 3 W is no multiple of 4 in general, so a row's first
//      and last bytes move alone), or converted from the fp32 planes.
//   3. a thread owns 4 consecutive pixels of one row in registers and walks the list front to back: the loop bounds are the same for
//      the whole workgroup, every record is an LDS broadcast read.  Caption pixels are the slow path: they read the label, the name
//      table and the font from global memory.
//   4. the painted rows go back through LDS and leave in aligned dword stores, first and last bytes of a row alone.
// A tile no row touches has an empty list: steps 2 and 4 are then a straight copy or convert.
// The box conversion (dod_detect's) and `x * 255 + 0.5` of the fp32 -> byte rule must round once per operation: no multiply-add is
// contracted anywhere in this file.
#pragma clang fp contract(off)
#include "dod_common.h"
#include "../../include/dinodet.h"

#define DRW_THREADS 256
#define DRW_WAVES (DRW_THREADS / DOD_WAVE)
#define DRW_TW 64                 // tile width in pixels: 16 threads x 4 pixels
#define DRW_TH 16                 // tile height: one row per 16 threads
#define DRW_MAX_K 1024
#define DRW_LIST (2 * DRW_MAX_K)
#define DRW_PITCH 200             // bytes of a staged row: 3 * 64 + up to 3 bytes in front, rounded up to dwords
#define DRW_MAX_DIM 16384         // rectangles are kept as int16
#define DRW_MAX_B 65535           // grid.z
#define DRW_MAX_NAME 64

struct DrwLayer {
  const float* boxes; const int* counts; const int* labels; const float* scores;
  int K, format, use_palette;
  float threshold;
  unsigned color;                 // r | g << 8 | b << 16
};
struct DrwArgs {
  const void* img; unsigned char* out;
  int fp32, B, H, W;
  DrwLayer layer[2];
  int t, alpha, scale;
  const unsigned char* palette; int P;
  const unsigned char* names; int n_names, name_len;
  const unsigned char* font;
};

__device__ __forceinline__ int drw_min(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int drw_max(int a, int b) { return a > b ? a : b; }
// saturate, then convert: every float -- +-inf included -- lands in the int16 range (NaN never gets here)
__device__ __forceinline__ int drw_f2i(float v) { return (int)(v < -32768.0f ? -32768.0f : (v > 32767.0f ? 32767.0f : v)); }
__device__ __forceinline__ int drw_digits(unsigned m) {
  int n = 1;
  while (m >= 10u) { m /= 10u; ++n; }
  return n;
}
__device__ __forceinline__ unsigned drw_digit(unsigned m, int from_right) {
  for (; from_right > 0; --from_right) m /= 10u;
  return m % 10u;
}
__device__ __forceinline__ unsigned drw_div255(unsigned u) { u += 128u; return (u + (u >> 8)) >> 8; }
__device__ __forceinline__ unsigned drw_to_byte(float x) {
  float v = x * 255.0f;
  v = v + 0.5f;
  if (!(v == v)) return 0u;
  v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
  return (unsigned)(int)v;
}
// the caption rectangle of a box whose pixel rectangle starts at (xa, ya) and whose text has n characters
__device__ __forceinline__ void drw_caption(int xa, int ya, int n, int s, int W, int H, int& cx0, int& cy0, int& cw, int& ch) {
  cw = drw_min(6 * s * n + s, W);
  ch = drw_min(9 * s, H);
  cy0 = ya - ch >= 0 ? ya - ch : ya;
  cy0 = drw_min(drw_max(cy0, 0), H - ch);
  cx0 = drw_min(drw_max(xa, 0), W - cw);
}
// a layer's field by a run-time layer index, without indexing the argument block (which would move it to scratch)
#define DRW_SEL(l, f) ((l) ? a.layer[1].f : a.layer[0].f)
// record words.  slot: row (10 bits) | layer << 10 | name length << 11 (7 bits) | name from the table << 18 | has a score << 19 | percent << 20
__device__ __forceinline__ unsigned drw_text_char(const DrwArgs& a, int b, unsigned slot, int ci) {
  const int row = slot & 1023, l = (slot >> 10) & 1, nlen = (slot >> 11) & 127;
  if (ci < nlen) {
    const int label = DRW_SEL(l, labels)[(size_t)b * DRW_SEL(l, K) + row];
    if ((slot >> 18) & 1u) return a.names[(size_t)label * a.name_len + ci];
    if (label < 0 && ci == 0) return '-';
    const unsigned m = label < 0 ? 0u - (unsigned)label : (unsigned)label;
    return '0' + drw_digit(m, nlen - 1 - ci);
  }
  const unsigned pct = (slot >> 20) & 1023u;
  const int j = ci - nlen, pd = drw_digits(pct);       // ' ' digits '%'
  if (j == 0) return ' ';
  if (j == pd + 1) return '%';
  return '0' + drw_digit(pct, pd - j);
}

__global__ __launch_bounds__(DRW_THREADS) void drw_kernel(const DrwArgs a) {
  __shared__ uint2 s_rect[DRW_LIST];
  __shared__ unsigned s_meta[DRW_LIST];
  __shared__ unsigned s_slot[DRW_LIST];
  __shared__ __attribute__((aligned(16))) unsigned char s_in[DRW_TH * DRW_PITCH];
  __shared__ __attribute__((aligned(16))) unsigned char s_out[DRW_TH * DRW_PITCH];
  __shared__ int s_wcnt[DRW_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, W = a.W, H = a.H;
  const int x0 = blockIdx.x * DRW_TW, y0 = blockIdx.y * DRW_TH;
  const int tw = drw_min(DRW_TW, W - x0), th = drw_min(DRW_TH, H - y0);
  const int s = a.scale;

  // ---- 1: cull into the ordered list
  int cnt[2];
#pragma unroll
  for (int l = 0; l < 2; ++l) {
    const DrwLayer& ly = a.layer[l];
    int n = 0;
    if (ly.boxes && ly.K > 0) {
      n = ly.counts ? ly.counts[b] : ly.K;
      n = drw_min(drw_max(n, 0), ly.K);
    }
    cnt[l] = n;
  }
  const int total = cnt[0] + cnt[1];
  int n_list = 0;
  for (int c0 = 0; c0 < total; c0 += DRW_THREADS) {
    const int sl = c0 + tid;
    bool hit = false;
    uint2 rect = make_uint2(0u, 0u);
    unsigned meta = 0u, slot = 0u;
    if (sl < total) {
      const int l = sl < cnt[0] ? 0 : 1;
      const int row = l == 0 ? cnt[0] - 1 - sl : cnt[1] - 1 - (sl - cnt[0]);
      DrwLayer ly;
      ly.boxes = DRW_SEL(l, boxes); ly.counts = nullptr; ly.labels = DRW_SEL(l, labels); ly.scores = DRW_SEL(l, scores);
      ly.K = DRW_SEL(l, K); ly.format = DRW_SEL(l, format); ly.use_palette = DRW_SEL(l, use_palette);
      ly.threshold = DRW_SEL(l, threshold); ly.color = DRW_SEL(l, color);
      const size_t ri = (size_t)b * ly.K + row;
      const float4 bx = reinterpret_cast<const float4*>(ly.boxes)[ri];
      float x1 = bx.x, y1 = bx.y, x2 = bx.z, y2 = bx.w;
      if (ly.format == 1) {                                   // normalised cxcywh -> pixels, as dod_detect
        const float cx = bx.x, cy = bx.y, w = bx.z, h = bx.w, fw = (float)W, fh = (float)H;
        x1 = cx - 0.5f * w; y1 = cy - 0.5f * h; x2 = cx + 0.5f * w; y2 = cy + 0.5f * h;
        x1 *= fw; y1 *= fh; x2 *= fw; y2 *= fh;
      }
      const int label = ly.labels[ri];                        // beside the box: a later load would wait for it
      const float sc = ly.scores ? ly.scores[ri] : 0.0f;
      bool ok = x1 == x1 && y1 == y1 && x2 == x2 && y2 == y2;
      if (ly.scores && !(ly.threshold < 0.0f) && sc <= ly.threshold) ok = false;
      if (ok) {
        const int xa = drw_f2i(floorf(x1)), ya = drw_f2i(floorf(y1));
        const int xb = drw_f2i(ceilf(x2)) - 1, yb = drw_f2i(ceilf(y2)) - 1;
        ok = xb >= xa && yb >= ya && xb >= 0 && yb >= 0 && xa < W && ya < H;
        if (ok) {
          const bool box_y = yb >= y0 && ya < y0 + th, box_x = xb >= x0 && xa < x0 + tw;
          hit = box_y && box_x;
          int n = 0, nlen = 0, use_name = 0;
          unsigned pct = 0u;
          if (s > 0) {
            int cx0, cy0, cw, ch;
            drw_caption(xa, ya, 1, s, W, H, cx0, cy0, cw, ch);            // the rows of a caption do not depend on its text
            if (cy0 < y0 + th && cy0 + ch > y0) {
              if (a.names && label >= 0 && label < a.n_names) {
                const unsigned char* nm = a.names + (size_t)label * a.name_len;
                while (nlen < a.name_len && nm[nlen]) ++nlen;
                use_name = nlen > 0;
              }
              if (!use_name) nlen = drw_digits(label < 0 ? 0u - (unsigned)label : (unsigned)label) + (label < 0 ? 1 : 0);
              n = nlen;
              if (ly.scores) {
                float p = floorf(sc * 100.0f + 0.5f);
                p = p == p ? p : 0.0f;
                p = p < 0.0f ? 0.0f : (p > 999.0f ? 999.0f : p);
                pct = (unsigned)(int)p;
                n += 2 + drw_digits(pct);
              }
              drw_caption(xa, ya, n, s, W, H, cx0, cy0, cw, ch);
              if (cx0 < x0 + tw && cx0 + cw > x0) hit = true;
            }
          }
          if (hit) {
            unsigned col = ly.color;
            if (ly.use_palette) {
              int pi = label % a.P;
              pi = pi < 0 ? pi + a.P : pi;
              const unsigned char* pc = a.palette + 3 * pi;
              col = pc[0] | (pc[1] << 8) | (pc[2] << 16);
            }
            rect.x = ((unsigned)xa & 0xffffu) | ((unsigned)ya << 16);
            rect.y = ((unsigned)xb & 0xffffu) | ((unsigned)yb << 16);
            meta = (col & 0xffffffu) | ((unsigned)n << 24);
            slot = (unsigned)row | ((unsigned)l << 10) | ((unsigned)nlen << 11) | ((unsigned)use_name << 18) | ((ly.scores ? 1u : 0u) << 19) | (pct << 20);
          }
        }
      }
    }
    const unsigned long long m = __ballot(hit);
    if (lane == 0) s_wcnt[wave] = __popcll(m);
    __syncthreads();
    int off = n_list, tot = 0;
#pragma unroll
    for (int w = 0; w < DRW_WAVES; ++w) {
      const int c = s_wcnt[w];
      if (w < wave) off += c;
      tot += c;
    }
    if (hit) {
      const int pos = off + __popcll(m & ((1ull << lane) - 1ull));       // pos < total <= DRW_LIST
      s_rect[pos] = rect; s_meta[pos] = meta; s_slot[pos] = slot;
    }
    n_list += tot;
    __syncthreads();
  }

  // ---- 2: this thread's 4 pixels
  const int r = tid >> 4, g = tid & 15;
  const int y = y0 + r, xg = x0 + 4 * g;
  const int nb = 3 * tw;                                                  // bytes of a tile row
  unsigned pr[4], pg[4], pb[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) pr[p] = pg[p] = pb[p] = 0u;
  if (a.fp32) {
    if (r < th) {
      const float* im = (const float*)a.img;
      const bool vec = (W & 3) == 0 && ((uintptr_t)im & 15) == 0 && 4 * g + 3 < tw;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float* pl = im + ((size_t)(b * 3 + c) * H + y) * W + xg;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (vec) {
          const float4 q = *reinterpret_cast<const float4*>(pl);
          v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
          for (int p = 0; p < 4; ++p)
            if (4 * g + p < tw) v[p] = pl[p];
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const unsigned q = drw_to_byte(v[p]);
          if (c == 0) pr[p] = q; else if (c == 1) pg[p] = q; else pb[p] = q;
        }
      }
    }
  } else {
    if (r < th) {                                                         // byte i of the row's span sits at s_in[lead + i]: aligned dwords coincide
      const unsigned char* gp = (const unsigned char*)a.img + ((size_t)(b * H + y) * W + x0) * 3;
      const int lead = (int)((uintptr_t)gp & 3);
      gp -= lead;
      unsigned char* lp = s_in + r * DRW_PITCH;
      for (int k = 4 * g; k < lead + nb; k += 64) {
        if (k >= lead && k + 4 <= lead + nb) *reinterpret_cast<unsigned*>(lp + k) = *reinterpret_cast<const unsigned*>(gp + k);
        else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (k + j >= lead && k + j < lead + nb) lp[k + j] = gp[k + j];
        }
      }
    }
    __syncthreads();
    if (r < th) {
      const unsigned char* gp = (const unsigned char*)a.img + ((size_t)(b * H + y) * W + x0) * 3;
      const unsigned char* lp = s_in + r * DRW_PITCH + (int)((uintptr_t)gp & 3) + 12 * g;
#pragma unroll
      for (int p = 0; p < 4; ++p)
        if (4 * g + p < tw) { pr[p] = lp[3 * p]; pg[p] = lp[3 * p + 1]; pb[p] = lp[3 * p + 2]; }
    }
  }

  // ---- 3: painter's walk
  const int t = a.t;
  const unsigned al = (unsigned)a.alpha, ial = 255u - al;
  for (int i = 0; i < n_list; ++i) {
    const uint2 rc = s_rect[i];
    const unsigned meta = s_meta[i];
    const int xa = (short)(rc.x & 0xffffu), ya = (int)rc.x >> 16, xb = (short)(rc.y & 0xffffu), yb = (int)rc.y >> 16;
    const unsigned cr = meta & 255u, cg = (meta >> 8) & 255u, cb = (meta >> 16) & 255u;
    if (y >= ya && y <= yb && xg + 3 >= xa && xg <= xb) {
      const int dy = drw_min(y - ya, yb - y);
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int x = xg + p;
        if (x >= xa && x <= xb) {
          const int d = drw_min(dy, drw_min(x - xa, xb - x));
          if (d < t) { pr[p] = cr; pg[p] = cg; pb[p] = cb; }
          else if (al) {
            pr[p] = drw_div255(pr[p] * ial + cr * al);
            pg[p] = drw_div255(pg[p] * ial + cg * al);
            pb[p] = drw_div255(pb[p] * ial + cb * al);
          }
        }
      }
    }
    if (s > 0) {
      const int n = (int)(meta >> 24);
      int cx0, cy0, cw, ch;
      drw_caption(xa, ya, n, s, W, H, cx0, cy0, cw, ch);
      if (y >= cy0 && y < cy0 + ch && xg + 3 >= cx0 && xg < cx0 + cw) {
        const unsigned slot = s_slot[i];
        const unsigned tc = 299u * cr + 587u * cg + 114u * cb >= 128000u ? 0u : 255u;
        const int v = y - cy0 - s, cell = 6 * s;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int x = xg + p;
          if (x >= cx0 && x < cx0 + cw) {
            const int u = x - cx0 - s;
            bool on = false;
            if (u >= 0 && v >= 0) {
              const int ci = u / cell, gx = (u - ci * cell) / s, gy = v / s;
              if (ci < n && gx < 5 && gy < 7) {
                const unsigned chr = drw_text_char(a, b, slot, ci);
                const unsigned gl = (chr < 0x20u || chr > 0x7fu) ? 95u : chr - 0x20u;
                on = (a.font[gl * 7u + gy] >> (4 - gx)) & 1u;
              }
            }
            pr[p] = on ? tc : cr; pg[p] = on ? tc : cg; pb[p] = on ? tc : cb;
          }
        }
      }
    }
  }

  // ---- 4: back through LDS, out in aligned dwords
  unsigned char* orow = a.out + ((size_t)(b * H + y) * W + x0) * 3;      // only formed into an address when r < th
  const int olead = r < th ? (int)((uintptr_t)orow & 3) : 0;
  if (r < th) {
    unsigned char* lp = s_out + r * DRW_PITCH + olead + 12 * g;
#pragma unroll
    for (int p = 0; p < 4; ++p)
      if (4 * g + p < tw) { lp[3 * p] = (unsigned char)pr[p]; lp[3 * p + 1] = (unsigned char)pg[p]; lp[3 * p + 2] = (unsigned char)pb[p]; }
  }
  __syncthreads();
  if (r < th) {
    unsigned char* gp = orow - olead;
    const unsigned char* lp = s_out + r * DRW_PITCH;
    for (int k = 4 * g; k < olead + nb; k += 64) {
      if (k >= olead && k + 4 <= olead + nb) *reinterpret_cast<unsigned*>(gp + k) = *reinterpret_cast<const unsigned*>(lp + k);
      else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (k + j >= olead && k + j < olead + nb) gp[k + j] = lp[k + j];
      }
    }
  }
}

static bool drw_layer_present(const dod_draw_layer* l) { return l && l->boxes && l->K > 0; }

static bool drw_layer_ok(const dod_draw_layer* l, const dod_draw_style* st) {
  if (!l) return true;
  if (l->K < 0 || l->K > DRW_MAX_K) return false;
  if (l->format != 0 && l->format != 1) return false;
  if (!drw_layer_present(l)) return true;
  if (!l->labels) return false;
  if (((uintptr_t)l->boxes & 15) != 0) return false;                     // rows are loaded as float4
  if (l->use_palette && (!st->palette || st->palette_size < 1)) return false;
  return true;
}

static DrwLayer drw_layer(const dod_draw_layer* l) {
  DrwLayer d = {};
  if (!drw_layer_present(l)) return d;
  d.boxes = l->boxes; d.counts = l->counts; d.labels = l->labels; d.scores = l->scores;
  d.K = l->K; d.format = l->format; d.use_palette = l->use_palette ? 1 : 0;
  d.threshold = l->score_threshold;
  d.color = (unsigned)l->color[0] | ((unsigned)l->color[1] << 8) | ((unsigned)l->color[2] << 16);
  return d;
}

extern "C" int dod_draw_detections(const void* images, int images_fp32, int B, int H, int W, const dod_draw_layer* below,
                                   const dod_draw_layer* above, const dod_draw_style* style, uint8_t* out, void* stream) {
  if (!images || !out || !style || (const void*)out == images) return dod_fail(DOD_ERR_INVALID, "dod_draw_detections: null images / out / style, or out aliases images");
  if (images_fp32 != 0 && images_fp32 != 1) return dod_fail(DOD_ERR_INVALID, "dod_draw_detections: images_fp32 = %d is neither 0 nor 1", images_fp32);
  if (B < 1 || H < 1 || W < 1 || B > DRW_MAX_B || H > DRW_MAX_DIM || W > DRW_MAX_DIM) return dod_fail(DOD_ERR_INVALID, "dod_draw_detections: B=%d H=%d W=%d outside the limits", B, H, W);
  if (images_fp32 && ((uintptr_t)images & 3) != 0) return dod_fail(DOD_ERR_INVALID, "dod_draw_detections: fp32 images not 4-byte aligned");
  if (style->thickness < 1 || style->thickness > 8 || style->fill_alpha < 0 || style->fill_alpha > 255) return dod_fail(DOD_ERR_INVALID, "dod_draw_detections: thickness outside 1..8 or fill_alpha outside 0..255");
  if (style->font_scale < 0 || style->font_scale > 4 || (style->font_scale > 0 && !style->font)) return dod_fail(DOD_ERR_INVALID, "dod_draw_detections: font_scale outside 0..4, or a font_scale without a font");
  if (style->names && (style->n_names < 1 || style->name_len < 1 || style->name_len > DRW_MAX_NAME)) return dod_fail(DOD_ERR_INVALID, "dod_draw_detections: names with n_names < 1 or name_len outside the limits");
  if (!drw_layer_ok(below, style) || !drw_layer_ok(above, style)) return dod_fail(DOD_ERR_INVALID, "dod_draw_detections: a layer with K or format outside the limits, null labels, boxes not 16-byte aligned, or use_palette without a palette");
  DrwArgs a = {};
  a.img = images; a.out = out; a.fp32 = images_fp32; a.B = B; a.H = H; a.W = W;
  a.layer[0] = drw_layer(below); a.layer[1] = drw_layer(above);
  a.t = style->thickness; a.alpha = style->fill_alpha; a.scale = style->font_scale;
  a.palette = style->palette; a.P = style->palette ? style->palette_size : 1;
  a.names = style->names; a.n_names = style->names ? style->n_names : 0; a.name_len = style->name_len;
  a.font = style->font;
  const dim3 grid((W + DRW_TW - 1) / DRW_TW, (H + DRW_TH - 1) / DRW_TH, B);
  hipLaunchKernelGGL(drw_kernel, grid, dim3(DRW_THREADS), 0, (hipStream_t)stream, a);
  return dod_launched("dod_draw_detections");
}
