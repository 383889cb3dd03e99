/* rot_tiles.h — tile geometry of the GRAY8 bicubic rotation (kernels_rotate.hip
 * k_rotate_cubic_g8f), in one place.
 *
 * Everything here is a function of (sheet, tile) alone, never of pixels: the
 * per-sheet constants of deskew.c:248-286 / primitives.c:137-145 and, per
 * 128 x 48 output tile, the source window of the tile's in-mask pixels and
 * the class of the tile.  k_rot_tiles evaluates it once per launch into two
 * records (RotSheet, RotTile); the rotation kernel only reads them.  Plain
 * C++ with no HIP dependency, so a host program can check the geometry
 * against a brute force over pixels (tests/test_rot_tiles_cpu.py).  The
 * float expressions round like the row loop's (FP contraction off in every
 * build that includes this file).
 */
#ifndef UNPAPER_HIP_ROT_TILES_H
#define UNPAPER_HIP_ROT_TILES_H

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define ROT_FN __host__ __device__ static inline
#else
#define ROT_FN static inline
#endif

enum {
  kRFW = 128, /* output columns per tile (2 per lane) */
  kRFH = 48,  /* output rows per tile, every 8th to one wave: 6 per wave (rot_wave_row;
                 96-row tiles measured slower: DESIGN §5) */
  kRFS = 144, /* staged row stride in floats (>= 141-float window rows at 5 deg) */
  kRFWaves = 8 /* waves per tile */
};

/* Tile row (0 .. kRFH - 1) of the k-th row (k < kRFH / kRFWaves) of wave wu:
 * the rows are dealt round-robin, wave wu takes wu, wu + 8, ..., wu + 40.
 * Ink comes in horizontal bands, and the kernel skips the arithmetic of rows
 * whose taps are all white: a band of n consecutive rows gives every wave at
 * most ceil(n / 8) of them, where consecutive rows per wave gave some waves
 * six and others none while the tile waits for its slowest wave.
 * A bijection onto the tile's rows, strictly increasing in k: the kernel's
 * "rows from here on are below the image" tests rely on that
 * (tests/test_rot_rows_cpu.py). */
ROT_FN int rot_wave_row(int wu, int k) {
#if defined(UPHIP_DIAG) && defined(UPH_ROT_ROWS_CONSECUTIVE)
  return wu * (kRFH / kRFWaves) + k; /* tuning build only: the assignment before, for the A/B */
#else
  return wu + kRFWaves * k;
#endif
}

/* RotTile.flags */
enum {
  ROT_T_OUTSIDE = 1,   /* no pixel of the tile inside the mask: copied unchanged */
  ROT_T_PARTIAL = 2,   /* some pixel of the tile (inside the image) outside the mask */
  ROT_T_STAGED = 4,    /* the window fits the launch's LDS rows */
  ROT_T_INTERIOR = 8,  /* the staged (8-byte aligned) window lies inside the image */
  ROT_T_POSC = 16,     /* the window starts inside the image: coordinates >= 1 */
  ROT_T_FULL = 32      /* every pixel in mask and image, staged, posc: no per-pixel tests */
};

/* Per sheet, 64 bytes.  src / dst are the sheet's resolved planes (the
 * ctl[s].cur selection done once); mx0 / my0 the mask's first vertex as given
 * (output pixel (x, y) is mask pixel (x - mx0, y - my0)); the rest as named in
 * primitives.c:137-145 with the normalised mask's origin folded into scx, scy. */
typedef struct RotSheet {
  const uint8_t* src;
  uint8_t* dst;
  int32_t mx0, my0;
  int32_t sw, sh;
  float scx, scy, tcx, tcy;
  float sinval, cosval;
  int32_t active; /* 0: the sheet is not rotated (no tile record is valid) */
  int32_t large;  /* window-row class: 1 = taken by the large-window launch */
} RotSheet;

/* Per (sheet, tile), 16 bytes: the source window [bx0, bx0 + bw) x [by0, by0 + bh)
 * that holds the 4 x 4 taps of every in-mask pixel of the tile. */
typedef struct RotTile {
  int32_t bx0, by0;
  uint16_t bw, bh;
  uint32_t flags;
} RotTile;

ROT_FN int32_t rot_imin(int32_t a, int32_t b) { return a < b ? a : b; }
ROT_FN int32_t rot_imax(int32_t a, int32_t b) { return a > b ? a : b; }

/* Window rows a tile needs at this sine (the class test of the two launches). */
ROT_FN int rot_need_rows(float sinval) { return kRFH + (int)ceilf((kRFW - 1) * fabsf(sinval)) + 5; }

/* The per-sheet constants from the mask as given (x0, y0, x1, y1 may be
 * inverted); src, dst, active and large are the caller's. */
ROT_FN void rot_sheet_geom(int32_t x0, int32_t y0, int32_t x1, int32_t y1, float sinval,
                           float cosval, RotSheet* g) {
  const int32_t nx0 = rot_imin(x0, x1), ny0 = rot_imin(y0, y1);
  const int32_t nx1 = rot_imax(x0, x1), ny1 = rot_imax(y0, y1);
  const int32_t sw = nx1 - nx0 + 1, sh = ny1 - ny0 + 1;
  g->mx0 = x0;
  g->my0 = y0;
  g->sw = sw;
  g->sh = sh;
  g->scx = nx0 + sw / 2.0f; /* primitives.c:137-145 */
  g->scy = ny0 + sh / 2.0f;
  g->tcx = 0 + sw / 2.0f;
  g->tcy = 0 + sh / 2.0f;
  g->sinval = sinval;
  g->cosval = cosval;
}

/* Window start rounded down to a dword, and the source dwords per window row. */
ROT_FN int32_t rot_window_xa(int32_t bx0) { return bx0 >= 0 ? (bx0 & ~3) : -((-bx0 + 3) & ~3); }
ROT_FN int rot_window_nd(int32_t bx0, int32_t bw) { return (bx0 - rot_window_xa(bx0) + bw + 3) >> 2; }

/* Tile (txi, tyi) of a W x H plane; max_rows: the window rows the sheet's
 * launch stages.
 *
 * Source window of the tile's in-mask pixels (their 4x4 taps included): every
 * pixel's coordinate lies between the corners' (the same float expression,
 * monotone in u and v); its taps span (int)c - 1 .. (int)c + 2, and
 * (int)c <= floor(c) + 1 (truncation of negatives). */
ROT_FN RotTile rot_tile(const RotSheet* g, int32_t W, int32_t H, int txi, int tyi, int max_rows) {
  RotTile t;
  const int32_t tx0 = txi * kRFW, ty0 = tyi * kRFH;
  const int32_t u0 = rot_imax(tx0, 0) - g->mx0, u1 = rot_imin(tx0 + kRFW, W) - 1 - g->mx0;
  const int32_t v0 = rot_imax(ty0, 0) - g->my0, v1 = rot_imin(ty0 + kRFH, H) - 1 - g->my0;
  const int32_t cu0 = rot_imax(u0, 0), cu1 = rot_imin(u1, g->sw - 1);
  const int32_t cv0 = rot_imax(v0, 0), cv1 = rot_imin(v1, g->sh - 1);
  if (!(cu0 <= cu1 && cv0 <= cv1)) {
    t.bx0 = t.by0 = 0;
    t.bw = t.bh = 0;
    t.flags = ROT_T_OUTSIDE;
    return t;
  }
  float mnx = 0, mny = 0, mxx = 0, mxy = 0;
  for (int c = 0; c < 4; c++) {
    const int32_t u = c & 1 ? cu1 : cu0, v = c & 2 ? cv1 : cv0;
    const float X = g->scx + (u - g->tcx) * g->cosval + (v - g->tcy) * g->sinval;
    const float Y = g->scy + (v - g->tcy) * g->cosval - (u - g->tcx) * g->sinval;
    mnx = c ? fminf(mnx, X) : X;
    mxx = c ? fmaxf(mxx, X) : X;
    mny = c ? fminf(mny, Y) : Y;
    mxy = c ? fmaxf(mxy, Y) : Y;
  }
  const int32_t bx0 = (int32_t)floorf(mnx) - 1, by0 = (int32_t)floorf(mny) - 1;
  const int32_t bw = (int32_t)floorf(mxx) + 3 - bx0 + 1, bh = (int32_t)floorf(mxy) + 3 - by0 + 1;
  const int32_t xa = rot_window_xa(bx0);
  const int nd = rot_window_nd(bx0, bw);
  const int nq = (nd + 1) >> 1; /* 8-byte loads per window row */
  const int staged = bw > 0 && bh > 0 && 4 * nd <= kRFS && bh <= max_rows;
  const int interior = xa >= 0 && xa + 8 * nq <= W && by0 >= 0 && by0 + bh <= H;
  const int partial = !(cu0 == u0 && cu1 == u1 && cv0 == v0 && cv1 == v1);
  /* Every source coordinate of the tile's in-mask pixels is >= 1 when the
   * window starts inside the image: then (int)c == floor(c) and
   * c - (int)c == fract(c) exactly. */
  const int posc = bx0 >= 0 && by0 >= 0;
  const int full = !partial && staged && posc && tx0 + kRFW <= W && ty0 + kRFH <= H;
  t.bx0 = bx0;
  t.by0 = by0;
  /* an unstaged window's size is never read; 0xFFFF keeps "too large" too large */
  t.bw = (uint16_t)rot_imin(rot_imax(bw, 0), 0xFFFF);
  t.bh = (uint16_t)rot_imin(rot_imax(bh, 0), 0xFFFF);
  t.flags = (partial ? ROT_T_PARTIAL : 0) | (staged ? ROT_T_STAGED : 0) |
            (interior ? ROT_T_INTERIOR : 0) | (posc ? ROT_T_POSC : 0) | (full ? ROT_T_FULL : 0);
  return t;
}

#endif
