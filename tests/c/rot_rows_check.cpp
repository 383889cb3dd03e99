// How the GRAY8 bicubic rotation deals a tile's rows to its waves
// (csrc/rot_tiles.h rot_wave_row): (wave, k) -> tile row must be a bijection
// onto 0 .. kRFH - 1 and strictly increasing in k for every wave (the kernel
// stops a wave's column sums at its first row below the image), and a band of
// n consecutive rows must give every wave at most ceil(n / kRFWaves) rows.
// Host program, no HIP (tests/test_rot_rows_cpu.py).
#include <stdio.h>

#include "rot_tiles.h"

int main() {
  static_assert(kRFH % kRFWaves == 0, "every wave takes the same number of rows");
  const int rows = kRFH / kRFWaves;
  int owner[kRFH], fails = 0;
  for (int r = 0; r < kRFH; r++) owner[r] = -1;
  for (int wu = 0; wu < kRFWaves; wu++)
    for (int k = 0; k < rows; k++) {
      const int r = rot_wave_row(wu, k);
      if (r < 0 || r >= kRFH) {
        printf("wave %d row %d -> %d outside the tile\n", wu, k, r);
        fails++;
        continue;
      }
      if (owner[r] >= 0) {
        printf("tile row %d dealt twice: waves %d and %d\n", r, owner[r], wu);
        fails++;
      }
      owner[r] = wu;
      if (k && r <= rot_wave_row(wu, k - 1)) {
        printf("wave %d: row %d -> %d not above row %d -> %d\n", wu, k, r, k - 1,
               rot_wave_row(wu, k - 1));
        fails++;
      }
    }
  for (int r = 0; r < kRFH; r++)
    if (owner[r] < 0) {
      printf("tile row %d dealt to no wave\n", r);
      fails++;
    }
  // every band [r0, r0 + n) of the tile: no wave holds more than ceil(n / waves)
  for (int r0 = 0; r0 < kRFH && !fails; r0++)
    for (int n = 1; r0 + n <= kRFH; n++) {
      int cnt[kRFWaves] = {0};
      for (int r = r0; r < r0 + n; r++) cnt[owner[r]]++;
      for (int wu = 0; wu < kRFWaves; wu++)
        if (cnt[wu] > (n + kRFWaves - 1) / kRFWaves) {
          printf("band %d..%d: wave %d holds %d rows\n", r0, r0 + n - 1, wu, cnt[wu]);
          fails++;
        }
    }
  if (fails) return 1;
  printf("ok: %d rows, %d waves, %d rows a wave\n", (int)kRFH, (int)kRFWaves, rows);
  return 0;
}
