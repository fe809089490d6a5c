// Entropy stage of the JPEG decoder (dod_jpeg_*, include/dinodet.h): ONE function that decodes one restart interval of a baseline /
// extended-sequential Huffman scan into int16 coefficients in natural (de-zigzagged) order.  Plain C++ with no include of its own
// beyond <stdint.h>: the device kernel (jpeg.hip, one thread per restart interval), the host entry dod_jpeg_entropy_host and the
// stand-alone sanitizer program of the tests (tests/jpeg_entropy_main.cpp, host compiler only) all include this file, so the code
// that the sanitizers exercise on hostile bytes is the code the device runs.
//
// Memory safety on ANY bytes and ANY table contents:
//   * the bit reader never reads outside [begin, end) of its interval: past the end, or behind a marker (FF followed by anything but
//     00), it supplies zero bits, and consuming one of them raises DOD_JPEG_F_OVERRUN and ends the interval;
//   * every table index is masked or range-checked, every table pointer is picked by a checked index;
//   * the coefficient position k is checked against 63 before the store (DOD_JPEG_F_COEF), the block index against the image's own
//     block count and the buffer's (the MCU loop ends there);
//   * a code no table entry defines ends the interval with DOD_JPEG_F_CODE;
//   * whole bytes left unread when the interval's MCUs are done raise DOD_JPEG_F_EXTRA (the pixels are still what the library gives).
// What was decoded before a flag stays in the buffer, the rest of the interval keeps its zeros: the result is a function of the bytes.
#pragma once
#include <stdint.h>

#ifndef DOD_JPEG_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define DOD_JPEG_HD __host__ __device__
#else
#define DOD_JPEG_HD
#endif
#endif

// ---- per-image descriptor: DOD_JI_STRIDE int64 per image (the header parse of dinov2_od_amd/jpeg.py writes it)
enum {
  DOD_JI_WIDTH = 0, DOD_JI_HEIGHT, DOD_JI_NCOMP,      // pixels; 1 (grey) or 3 (YCbCr) components
  DOD_JI_HS, DOD_JI_VS,                                // luma sampling factors (1 | 2, 1 | 2); chroma is 1 x 1.  1, 1 for grey
  DOD_JI_MCUS_X, DOD_JI_MCUS_Y,                        // MCUs per row / column of the one interleaved scan
  DOD_JI_RESTART,                                      // restart interval in MCUs, 0 = none
  DOD_JI_SCAN_BEGIN, DOD_JI_SCAN_END,                  // the scan's entropy-coded bytes [begin, end) inside the batch's byte buffer
  DOD_JI_BLOCK0,                                       // +c: first 8 x 8 block of component c in the coefficient buffer (64 int16 each)
  DOD_JI_BLOCKS_W = DOD_JI_BLOCK0 + 3,                 // +c: blocks per row of component c (its plane is 8 * blocks_w bytes wide)
  DOD_JI_PLANE = DOD_JI_BLOCKS_W + 3,                  // +c: byte offset of component c's plane in the plane buffer
  DOD_JI_OUT = DOD_JI_PLANE + 3,                       // byte offset of the image's RGB bytes in the output
  DOD_JI_QT,                                           // +c: quantisation table (row of the batch's table array)
  DOD_JI_DC = DOD_JI_QT + 3,                           // +c: DC Huffman table (row of the batch's table array)
  DOD_JI_AC = DOD_JI_DC + 3,                           // +c: AC Huffman table
  DOD_JI_ITEM0 = DOD_JI_AC + 3,                        // first work item of the upsample + colour kernel (4 pixels of a row each)
  DOD_JI_STRIDE = 32
};
// ---- per-interval row: DOD_JV_STRIDE int64
enum { DOD_JV_IMAGE = 0, DOD_JV_BEGIN, DOD_JV_END, DOD_JV_MCU0, DOD_JV_NMCU, DOD_JV_STRIDE = 5 };
// ---- Huffman table: DOD_JH_STRIDE int32 per table
//   [0, 512)            look-up by the next 9 bits: (length << 8) | symbol for a code of <= 9 bits, 0 = longer or undefined
//   [512 + l], l 1..16  largest code of length l, -1 = none      (index 512 unused)
//   [529 + l]           (index of the length's first symbol) - (its first code)
//   [546, 802)          the symbols in code order
enum { DOD_JH_LOOK = 0, DOD_JH_MAXCODE = 512, DOD_JH_VALOFF = 529, DOD_JH_VAL = 546, DOD_JH_STRIDE = 802 };
// ---- flags of the per-image status word
enum { DOD_JPEG_F_OVERRUN = 1,      // the interval's bytes ran out (or a marker stood in them) before its MCUs were decoded
       DOD_JPEG_F_CODE = 2,         // a bit pattern no Huffman code of the table matches, or a DC size above 15
       DOD_JPEG_F_COEF = 4,         // a run that leaves the block (coefficient index above 63)
       DOD_JPEG_F_RESTART = 8,      // host entry: no restart marker where one was due
       DOD_JPEG_F_TABLE = 16,       // a table or block index outside its array (a descriptor the parser would not write)
       DOD_JPEG_F_EXTRA = 32 };     // whole bytes left over behind the interval's last MCU (an encoder pads with fewer than 8 bits)

// zigzag position -> natural position
DOD_JPEG_HD inline int dod_jpeg_natural(int k) {
  const unsigned char order[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return order[k & 63];
}

struct dod_jpeg_bits {
  const uint8_t* p;       // next byte to fetch
  const uint8_t* end;     // one past the interval's last byte
  uint32_t buf;           // the low `nbits` bits are unread, most significant first
  int nbits;
  int padded;             // how many of the unread bits, at the low end, are zeros supplied past the data
  int stopped;            // a marker was met: p stays on its FF
};

// one more byte into the buffer: FF 00 is the data byte FF; FF before anything else is a marker, which ends the data
DOD_JPEG_HD inline void dod_jpeg_fetch(dod_jpeg_bits& r) {
  uint32_t b = 0;
  if (!r.stopped && r.p < r.end) {
    b = *r.p;
    if (b == 0xFF) {
      if (r.p + 1 < r.end && r.p[1] == 0) r.p += 2;
      else { r.stopped = 1; b = 0; r.padded += 8; }
    } else {
      ++r.p;
    }
  } else {
    r.padded += 8;
  }
  r.buf = (r.buf << 8) | b;
  r.nbits += 8;
}
// n <= 16
DOD_JPEG_HD inline void dod_jpeg_ensure(dod_jpeg_bits& r, int n) {
  while (r.nbits < n) dod_jpeg_fetch(r);
}
DOD_JPEG_HD inline uint32_t dod_jpeg_peek(const dod_jpeg_bits& r, int n) { return (r.buf >> (r.nbits - n)) & ((1u << n) - 1u); }
// the next n bits (0 <= n <= 16)
DOD_JPEG_HD inline uint32_t dod_jpeg_get(dod_jpeg_bits& r, int n) {
  if (n == 0) return 0;
  dod_jpeg_ensure(r, n);
  const uint32_t v = dod_jpeg_peek(r, n);
  r.nbits -= n;
  return v;
}
// one Huffman symbol, -1 when no code matches
DOD_JPEG_HD inline int dod_jpeg_symbol(dod_jpeg_bits& r, const int32_t* ht) {
  dod_jpeg_ensure(r, 16);
  const uint32_t look = dod_jpeg_peek(r, 16);
  const int32_t e = ht[DOD_JH_LOOK + (look >> 7)];
  if (e) {
    r.nbits -= (e >> 8) & 15;      // 1..9
    return e & 255;
  }
  for (int l = 10; l <= 16; ++l) {
    const int32_t code = (int32_t)(look >> (16 - l));
    if (code <= ht[DOD_JH_MAXCODE + l]) {
      r.nbits -= l;
      return ht[DOD_JH_VAL + ((ht[DOD_JH_VALOFF + l] + code) & 255)] & 255;
    }
  }
  return -1;
}
// the value of `s` extra bits (jdhuff.c HUFF_EXTEND); 1 <= s <= 15
DOD_JPEG_HD inline int32_t dod_jpeg_extend(uint32_t v, int s) {
  return (int32_t)v < (1 << (s - 1)) ? (int32_t)v - (1 << s) + 1 : (int32_t)v;
}

// Decodes MCUs [mcu0, mcu0 + nmcu) of image `ji` (its DOD_JI_* row) from bytes[begin, end) with every DC prediction starting at 0.
// htabs: n_htabs tables of DOD_JH_STRIDE int32.  coef: the batch's coefficient buffer of coef_blocks blocks, zero-filled where this
// interval writes.  *stop (if given) receives the position the reader stopped at: on the marker that ended the data, or behind the
// last byte it took.  Returns the DOD_JPEG_F_* flags it raised.
DOD_JPEG_HD inline int dod_jpeg_decode_interval(const uint8_t* bytes, int64_t begin, int64_t end, const int64_t* ji, const int32_t* htabs,
                                                int n_htabs, int64_t mcu0, int64_t nmcu, int16_t* coef, int64_t coef_blocks, int64_t* stop) {
  if (stop) *stop = begin;
  if (end < begin) end = begin;
  const int ncomp = (int)ji[DOD_JI_NCOMP];
  const int64_t mcus_x = ji[DOD_JI_MCUS_X], mcus_y = ji[DOD_JI_MCUS_Y];
  if ((ncomp != 1 && ncomp != 3) || mcus_x < 1 || mcus_y < 1 || mcus_x > 65536 || mcus_y > 65536 || mcu0 < 0 || nmcu < 0) return DOD_JPEG_F_TABLE;
  const int32_t* dc_t[3];
  const int32_t* ac_t[3];
  int hs[3], vs[3];
  int64_t block0[3], blocks_w[3], blocks_n[3];
  for (int c = 0; c < ncomp; ++c) {
    const int64_t d = ji[DOD_JI_DC + c], a = ji[DOD_JI_AC + c];
    if (d < 0 || d >= n_htabs || a < 0 || a >= n_htabs) return DOD_JPEG_F_TABLE;
    dc_t[c] = htabs + d * DOD_JH_STRIDE;
    ac_t[c] = htabs + a * DOD_JH_STRIDE;
    hs[c] = c == 0 ? (int)ji[DOD_JI_HS] : 1;
    vs[c] = c == 0 ? (int)ji[DOD_JI_VS] : 1;
    if (hs[c] < 1 || hs[c] > 2 || vs[c] < 1 || vs[c] > 2) return DOD_JPEG_F_TABLE;
    block0[c] = ji[DOD_JI_BLOCK0 + c];
    blocks_w[c] = ji[DOD_JI_BLOCKS_W + c];
    blocks_n[c] = blocks_w[c] * (mcus_y * vs[c]);
    if (block0[c] < 0 || blocks_w[c] != mcus_x * hs[c] || block0[c] + blocks_n[c] > coef_blocks) return DOD_JPEG_F_TABLE;
  }
  dod_jpeg_bits r;
  r.p = bytes + begin; r.end = bytes + end; r.buf = 0; r.nbits = 0; r.padded = 0; r.stopped = 0;
  int32_t pred[3] = {0, 0, 0};
  int flags = 0;
  int64_t last = mcu0 + nmcu;
  if (last > mcus_x * mcus_y) last = mcus_x * mcus_y;
  for (int64_t m = mcu0; m < last && !flags; ++m) {
    const int64_t my = m / mcus_x, mx = m - my * mcus_x;
    for (int c = 0; c < ncomp && !flags; ++c) {
      for (int j = 0; j < vs[c] && !flags; ++j) {
        for (int i = 0; i < hs[c] && !flags; ++i) {
          int16_t* blk = coef + (block0[c] + (my * vs[c] + j) * blocks_w[c] + (mx * hs[c] + i)) * 64;
          // DC: size, then the difference to the component's previous DC
          int s = dod_jpeg_symbol(r, dc_t[c]);
          if (s < 0 || s > 15) { flags |= DOD_JPEG_F_CODE; break; }
          if (s) pred[c] = (int32_t)((uint32_t)pred[c] + (uint32_t)dod_jpeg_extend(dod_jpeg_get(r, s), s));
          blk[0] = (int16_t)pred[c];
          // AC: (run, size) pairs; 0x00 ends the block, 0xF0 skips 16 zeros
          for (int k = 1; k < 64; ++k) {
            const int rs = dod_jpeg_symbol(r, ac_t[c]);
            if (rs < 0) { flags |= DOD_JPEG_F_CODE; break; }
            s = rs & 15;
            const int run = rs >> 4;
            if (s) {
              k += run;
              if (k > 63) { flags |= DOD_JPEG_F_COEF; break; }
              blk[dod_jpeg_natural(k)] = (int16_t)dod_jpeg_extend(dod_jpeg_get(r, s), s);
            } else {
              if (run != 15) break;
              k += 15;
            }
          }
          if (r.nbits < r.padded) flags |= DOD_JPEG_F_OVERRUN;      // some bit this block consumed was not in the data
        }
      }
    }
  }
  if (!flags && last == mcu0 + nmcu) {
    // all MCUs decoded: what is left must be the padding bits of the last byte, then a marker or the end
    bool extra = r.nbits - r.padded >= 8;
    if (!extra && !r.stopped && r.p < r.end) extra = !(r.p[0] == 0xFF && (r.p + 1 >= r.end || r.p[1] != 0));
    if (extra) flags |= DOD_JPEG_F_EXTRA;
  }
  if (stop) *stop = r.p - bytes;
  return flags;
}

// The whole scan of one image on the host: its restart intervals one after the other (the whole scan as one when the file has none),
// each followed by the marker FF D0..D7 (behind any number of fill bytes FF).  Where that marker is missing the image is flagged and decoding goes on behind the next
// one found (none: the remaining blocks keep their zeros).  Returns the flags.
DOD_JPEG_HD inline int dod_jpeg_decode_scan(const uint8_t* bytes, int64_t nbytes, const int64_t* ji, const int32_t* htabs, int n_htabs,
                                            int16_t* coef, int64_t coef_blocks) {
  int64_t pos = ji[DOD_JI_SCAN_BEGIN], end = ji[DOD_JI_SCAN_END];
  if (pos < 0 || end > nbytes || end < pos) return DOD_JPEG_F_TABLE;
  const int64_t mcus = ji[DOD_JI_MCUS_X] * ji[DOD_JI_MCUS_Y];
  const int64_t ri = ji[DOD_JI_RESTART];
  if (ji[DOD_JI_MCUS_X] < 1 || ji[DOD_JI_MCUS_Y] < 1 || ji[DOD_JI_MCUS_X] > 65536 || ji[DOD_JI_MCUS_Y] > 65536 || ri < 0) return DOD_JPEG_F_TABLE;
  if (ri == 0) return dod_jpeg_decode_interval(bytes, pos, end, ji, htabs, n_htabs, 0, mcus, coef, coef_blocks, nullptr);
  int flags = 0;
  for (int64_t m = 0; m < mcus; m += ri) {
    int64_t stop = pos;
    flags |= dod_jpeg_decode_interval(bytes, pos, end, ji, htabs, n_htabs, m, ri, coef, coef_blocks, &stop);
    if (flags & DOD_JPEG_F_TABLE) break;
    if (m + ri >= mcus) break;
    pos = stop;
    while (pos + 1 < end && bytes[pos] == 0xFF && bytes[pos + 1] == 0xFF) ++pos;      // fill bytes in front of a marker are legal
    if (pos + 1 < end && bytes[pos] == 0xFF && bytes[pos + 1] >= 0xD0 && bytes[pos + 1] <= 0xD7) {
      pos += 2;
      continue;
    }
    flags |= DOD_JPEG_F_RESTART;
    while (pos + 1 < end && !(bytes[pos] == 0xFF && bytes[pos + 1] >= 0xD0 && bytes[pos + 1] <= 0xD7)) ++pos;
    if (pos + 1 >= end) break;
    pos += 2;
  }
  return flags;
}
