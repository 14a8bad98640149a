// Stand-alone host check of avt_resize_u8_ksize / avt_resize_u8_tables (csrc/resize_u8.hip) for a sanitizer build: every
// (in, out) pair of tests/test_pil_resize_host.py, both filters, into heap buffers of exactly the size the ABI asks for, so
// that a write past a row or past the table is a report.  No device call is made.  From the repository root:
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -g -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=all tools/resize_u8_tables_check.cpp \
//       audio-video-textures_amd/csrc/resize_u8.hip audio-video-textures_amd/csrc/abi.hip -o build/resize_u8_tables_check
//   ./build/resize_u8_tables_check
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../include/avt.h"

int main() {
  const int pairs[][2] = {{45, 32}, {70, 64}, {95, 64}, {33, 32}, {32, 45}, {64, 70}, {360, 352}, {37, 32}, {1, 1}, {1, 7}, {7, 1}, {640, 360}};
  int bad = 0;
  for (const auto& p : pairs)
    for (int filter = AVT_RESIZE_BILINEAR; filter <= AVT_RESIZE_LANCZOS; ++filter) {
      const int in = p[0], out = p[1], ksize = avt_resize_u8_ksize(in, out, filter);
      if (ksize <= 0) {
        printf("%d -> %d filter %d: %s\n", in, out, filter, avt_last_error());
        return 1;
      }
      int32_t* k = static_cast<int32_t*>(malloc(sizeof(int32_t) * out * ksize));
      int32_t* bounds = static_cast<int32_t*>(malloc(sizeof(int32_t) * out * 2));
      if (avt_resize_u8_tables(in, out, filter, ksize, k, bounds) != AVT_OK) {
        printf("%d -> %d filter %d: %s\n", in, out, filter, avt_last_error());
        return 1;
      }
      for (int i = 0; i < out; ++i) {
        const int first = bounds[2 * i], n = bounds[2 * i + 1];
        int64_t sum = 0;
        for (int x = 0; x < ksize; ++x) sum += k[i * ksize + x];
        const int64_t off = sum - (1 << 22);
        if (first < 0 || n < 1 || n > ksize || first + n > in || off > ksize || off < -ksize) {
          printf("%d -> %d filter %d, output %d: first %d, taps %d of %d, sum %lld\n", in, out, filter, i, first, n, ksize, (long long)sum);
          ++bad;
        }
      }
      free(k);
      free(bounds);
      printf("%d -> %d filter %d: ksize %d ok\n", in, out, filter, ksize);
    }
  // refused, with nothing written: a ksize that is not the axis's
  int32_t one[2] = {0, 0};
  if (avt_resize_u8_tables(45, 32, AVT_RESIZE_LANCZOS, 1, one, one) != AVT_ERR_ARG) ++bad;
  printf(bad ? "FAILED\n" : "all tables in bounds\n");
  return bad != 0;
}
