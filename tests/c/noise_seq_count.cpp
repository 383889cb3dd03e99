// noise_seq_count.cpp — how many triggers the noisefilter's sequential part
// gets for a page (tests/test_filter_cases.py): the seq and clear sets of
// csrc/noise_planes.h, as k_noise_cand / k_noise_verdict build them (and
// tests/c/noise_planes_check.cpp checks them against the definitions), counted
// on the host.
//   noise_seq_count FILE   FILE: "W H white N\n", then W * H gray bytes
// prints "seq clear".
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "noise_planes.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  int W, H, white, N;
  if (!f || fscanf(f, "%d %d %d %d", &W, &H, &white, &N) != 4 || fgetc(f) != '\n') return 2;
  const int nwr = (W + 31) >> 5;
  std::vector<uint8_t> row((size_t)W);
  std::vector<uint32_t> plane((size_t)nwr * H, 0u);
  for (int y = 0; y < H; y++) {
    if (fread(row.data(), 1, (size_t)W, f) != (size_t)W) return 2;
    for (int x = 0; x < W; x++)
      if (row[x] < white) plane[(size_t)y * nwr + (x >> 5)] |= 1u << (x & 31);
  }
  fclose(f);
  const bool all_seq = N > 4;
  constexpr int R = 16;
  const NpPlane P{plane.data(), nwr, H};
  std::vector<uint32_t> small(plane.size(), 0u);
  long long seq = 0, clear = 0;
  for (int y0 = 0; y0 < H; y0 += R)
    for (int wi = 0; wi < nwr; wi++) {
      uint32_t l3w[R], cw[R], zw[R];
      np_strip<R>(P, wi, y0, all_seq ? 1 : 0, l3w, cw, zw);
      for (int r = 0; r < R && y0 + r < H; r++) {
        seq += __builtin_popcount(zw[r]);
        uint32_t sw = 0;
        for (uint32_t m = all_seq ? 0u : cw[r]; m; m &= m - 1) {
          const int b = __builtin_ctz(m);
          uint32_t comp[9], D[9];
          if (np_flood9(P, 32 * wi + b, y0 + r, comp, D) <= kNpSmallMax) sw |= 1u << b;
        }
        small[(size_t)(y0 + r) * nwr + wi] = sw;
      }
    }
  const NpPlane S{small.data(), nwr, H};
  if (!all_seq)
    for (int y = kNpZone; y < H; y++)
      for (int wi = 0; wi < nwr; wi++)
        for (uint32_t m = small[(size_t)y * nwr + wi]; m; m &= m - 1) {
          const int x = 32 * wi + __builtin_ctz(m);
          if (x < kNpZone) continue;
          const int v = np_verdict(P, S, x, y, N);
          seq += v == NP_SEQ;
          clear += v == NP_CLEAR;
        }
  printf("%lld %lld\n", seq, clear);
  return 0;
}
