// Stand-alone driver of dinov2_od_amd/csrc/jpeg_entropy.h for the host compiler's sanitizers (tests/test_jpeg_cpu.py builds it with
// -fsanitize=address,undefined and runs it; nothing is preloaded, no GPU code is involved).  It includes ONLY that header.
//
//   jpeg_entropy_main CORPUS
// CORPUS (written by the test): int64 count, then per case
//   int64 nbytes, n_htabs, n_blocks;  int64 image[DOD_JI_STRIDE];  int32 htabs[n_htabs][DOD_JH_STRIDE];  uint8 bytes[nbytes]
// Every buffer is a heap block of exactly its size, so that one byte outside is a sanitizer report.  Each case is decoded twice into
// fresh zeroed coefficient buffers; the program prints "case flags fnv1a64(coefficients)" per case and fails when the two runs differ.
#include "../dinov2_od_amd/csrc/jpeg_entropy.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static uint64_t fnv1a(const void* p, size_t n) {
  const unsigned char* b = (const unsigned char*)p;
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s CORPUS\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int64_t count = 0;
  if (!read_exact(f, &count, 8) || count < 0) return 2;
  for (int64_t i = 0; i < count; ++i) {
    int64_t head[3];
    int64_t image[DOD_JI_STRIDE];
    if (!read_exact(f, head, sizeof head) || !read_exact(f, image, sizeof image)) return 2;
    const int64_t nbytes = head[0], n_htabs = head[1], n_blocks = head[2];
    if (nbytes < 0 || n_htabs < 1 || n_blocks < 0 || nbytes > (1ll << 30) || n_htabs > 64 || n_blocks > (1ll << 24)) return 2;
    int32_t* htabs = (int32_t*)malloc((size_t)n_htabs * DOD_JH_STRIDE * sizeof(int32_t));
    uint8_t* bytes = (uint8_t*)malloc(nbytes ? (size_t)nbytes : 1);
    if (!htabs || !bytes || !read_exact(f, htabs, (size_t)n_htabs * DOD_JH_STRIDE * sizeof(int32_t)) || !read_exact(f, bytes, (size_t)nbytes)) return 2;
    uint64_t sums[2];
    int flags[2];
    for (int run = 0; run < 2; ++run) {
      const size_t n = (size_t)n_blocks * 64;
      int16_t* coef = (int16_t*)calloc(n ? n : 1, sizeof(int16_t));
      if (!coef) return 2;
      flags[run] = dod_jpeg_decode_scan(bytes, nbytes, image, htabs, (int)n_htabs, coef, n_blocks);
      sums[run] = fnv1a(coef, n * sizeof(int16_t));
      free(coef);
    }
    free(htabs);
    free(bytes);
    if (flags[0] != flags[1] || sums[0] != sums[1]) {
      fprintf(stderr, "case %lld: two runs differ\n", (long long)i);
      return 1;
    }
    printf("%lld %d %016llx\n", (long long)i, flags[0], (unsigned long long)sums[0]);
  }
  fclose(f);
  return 0;
}
