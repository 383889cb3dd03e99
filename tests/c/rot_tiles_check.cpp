// The tile geometry of the GRAY8 bicubic rotation (csrc/rot_tiles.h) against
// a brute force over pixels: for every tile of every case, each in-mask
// pixel's source coordinate -- the rotation kernel's row loop expressions,
// restated below -- must keep its 4 x 4 taps inside the tile's window, and
// every flag must equal its definition.  Plain g++, contraction off like the
// device build.  Exits non-zero on the first violation.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "rot_tiles.h"

struct Mask {
  int32_t x0, y0, x1, y1;
  const char* name;
};

static int64_t floordiv4(int64_t v) { return v >= 0 ? v / 4 : -((-v + 3) / 4); }

#define FAIL(...)                                                                          \
  do {                                                                                     \
    printf("FAIL %dx%d mask %s (%d,%d,%d,%d) angle %g tile (%d,%d) window (%d,%d)+%ux%u "  \
           "flags %#x: ",                                                                  \
           W, H, m.name, m.x0, m.y0, m.x1, m.y1, deg, txi, tyi, t.bx0, t.by0, t.bw, t.bh, \
           t.flags);                                                                       \
    printf(__VA_ARGS__);                                                                   \
    printf("\n");                                                                          \
    exit(1);                                                                               \
  } while (0)

int main() {
  const int sizes[4][2] = {{128, 48}, {127, 47}, {129, 49}, {400, 560}};
  const double degs[10] = {0.3, -0.3, 2.0, -2.0, 2.6, -2.6, 2.8, -2.8, 4.9, -4.9};
  // the launcher's two classes at a 5 degree scan range: 58 window rows at
  // four tiles a CU, else the range's own
  const int rows_small = 58;
  const int rows_large = kRFH + (int)ceilf((kRFW - 1) * sinf(5.0f * 3.14159265f / 180.0f)) + 5;
  long tiles = 0, pixels = 0, n_flag[6] = {0, 0, 0, 0, 0, 0};
  for (const auto& sz : sizes) {
    const int32_t W = sz[0], H = sz[1];
    const Mask masks[] = {
        {W / 8, H / 8, W * 7 / 8, H * 7 / 8, "inside"},
        {0, 0, W - 1, H - 1, "whole image"},
        {0, H / 4, W / 2, H * 3 / 4, "left edge"},
        {W / 2, H / 4, W - 1, H * 3 / 4, "right edge"},
        {W / 4, 0, W * 3 / 4, H / 2, "top edge"},
        {W / 4, H / 2, W * 3 / 4, H - 1, "bottom edge"},
        {-20, -10, W / 2, H / 2, "past top left"},
        {W / 2, H / 2, W + 30, H + 17, "past bottom right"},
        {-15, H / 3, W + 15, H * 2 / 3, "past left and right"},
        {W * 3 / 4, H * 3 / 4, W / 4, H / 4, "inverted"},
    };
    for (const Mask& m : masks)
      for (double deg : degs) {
        const float radians = (float)(deg * 3.14159265358979323846 / 180.0);
        const float sinval = sinf(-radians), cosval = cosf(-radians);  // deskew.c:260-261
        RotSheet g;
        rot_sheet_geom(m.x0, m.y0, m.x1, m.y1, sinval, cosval, &g);
        const int max_rows = rot_need_rows(sinval) > rows_small ? rows_large : rows_small;
        for (int tyi = 0; tyi * kRFH < H; tyi++)
          for (int txi = 0; txi * kRFW < W; txi++) {
            const RotTile t = rot_tile(&g, W, H, txi, tyi, max_rows);
            tiles++;
            long n_img = 0, n_in = 0;
            bool all_ge1 = true;
            for (int32_t y = tyi * kRFH; y < (tyi + 1) * kRFH && y < H; y++)
              for (int32_t x = txi * kRFW; x < (txi + 1) * kRFW && x < W; x++) {
                n_img++;
                // the row loop: pixel (x, y) is mask pixel (u, v)
                const int32_t u = x - g.mx0, v = y - g.my0;
                if (!(u >= 0 && u < g.sw && v >= 0 && v < g.sh)) continue;
                n_in++;
                const float cu = u - g.tcx, cv = v - g.tcy;
                const float ax = g.scx + cu * g.cosval, bs = cu * g.sinval;
                const float VS = cv * g.sinval, VC = g.scy + cv * g.cosval;
                const float sx = ax + VS, sy = VC - bs;
                const int ix = (int)sx, iy = (int)sy;  // truncation
                all_ge1 = all_ge1 && sx >= 1.0f && sy >= 1.0f;
                if (t.flags & ROT_T_OUTSIDE) FAIL("in-mask pixel (%d,%d) in an outside tile", x, y);
                if (ix - 1 < t.bx0 || ix + 2 >= t.bx0 + (int32_t)t.bw || iy - 1 < t.by0 ||
                    iy + 2 >= t.by0 + (int32_t)t.bh)
                  FAIL("pixel (%d,%d) -> (%.9g,%.9g): taps leave the window", x, y, sx, sy);
              }
            pixels += n_in;
            const bool outside = n_in == 0;
            if (outside != !!(t.flags & ROT_T_OUTSIDE)) FAIL("outside: %ld in-mask pixels", n_in);
            if (outside) {
              if (t.flags != ROT_T_OUTSIDE) FAIL("an outside tile carries other flags");
              n_flag[0]++;
              continue;
            }
            const bool partial = n_in != n_img;
            // the staged rows: 8-byte loads from the window's start rounded
            // down to a dword, nq a row
            const int64_t xa = 4 * floordiv4(t.bx0);
            const int64_t nd = (t.bx0 - xa + t.bw + 3) / 4, nq = (nd + 1) / 2;
            const bool staged = t.bw > 0 && t.bh > 0 && 4 * nd <= kRFS && t.bh <= max_rows;
            const bool interior =
                xa >= 0 && xa + 8 * nq <= W && t.by0 >= 0 && t.by0 + (int32_t)t.bh <= H;
            const bool posc = t.bx0 >= 0 && t.by0 >= 0;
            const bool full = !partial && staged && posc && n_img == (long)kRFW * kRFH;
            if (xa != rot_window_xa(t.bx0) || nd != rot_window_nd(t.bx0, t.bw))
              FAIL("window start %ld / dwords %ld", (long)xa, (long)nd);
            if (partial != !!(t.flags & ROT_T_PARTIAL)) FAIL("partial: %ld of %ld", n_in, n_img);
            if (staged != !!(t.flags & ROT_T_STAGED)) FAIL("staged at %d rows", max_rows);
            if (interior != !!(t.flags & ROT_T_INTERIOR)) FAIL("interior");
            if (posc != !!(t.flags & ROT_T_POSC)) FAIL("posc");
            if (posc && !all_ge1) FAIL("posc with a source coordinate below 1");
            if (full != !!(t.flags & ROT_T_FULL)) FAIL("full");
            if (t.flags & ~63u) FAIL("unknown flag bits");
            for (int k = 1; k < 6; k++) n_flag[k] += (t.flags >> k) & 1;
          }
      }
  }
  printf("ok: %ld tiles, %ld in-mask pixels; outside %ld partial %ld staged %ld interior %ld "
         "posc %ld full %ld\n",
         tiles, pixels, n_flag[0], n_flag[1], n_flag[2], n_flag[3], n_flag[4], n_flag[5]);
  // every class must have occurred, or the cases above test less than they say
  for (int k = 0; k < 6; k++)
    if (!n_flag[k]) return 2;
  return 0;
}
