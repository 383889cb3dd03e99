// kernels_rotate.hip — the deskew rotation (imageprocess/deskew.c rotate) for
// gfx950: the LDS-tiled kernel for every format and interpolation, the gray
// bicubic kernels and the GRAY8 float-window kernel of the default pipeline.
// (The bilinear rotation is in kernels_rotlin.hip.)
#include <type_traits>

#include "blit_common.h"
#include "interp.h"
#include "kernels.h"
#include "rot_tiles.h"

namespace uph {

// ---------------------------------------------------------------------------
// deskew_cpu + rotate (deskew.c:248-286) fused out of place: inside the mask
// rectangle (placed at mask.vertex[0], clipped to the image) the rotated
// pixel, elsewhere the source pixel.
//
// One workgroup per 64x16 output tile.  The source footprint of the tile's
// in-mask part (a rotated rectangle, plus the interpolation taps) is staged
// in LDS once -- white outside the image, which is what get_pixel returns --
// and every tap is then an LDS read.  The float expressions are untouched,
// so the result is identical to the direct gather, which remains the path
// for tiles whose footprint does not fit (rotations far beyond the default
// 5 degree range).
// ---------------------------------------------------------------------------
constexpr int kRotTW = 64, kRotTH = 16;
constexpr int kRotCap = 4096;  // staged pixels per tile

// LDS-staged window [x0, x0+w) x [y0, y0+h) of the source (channels: 1 for
// GRAY8/Y400A gray, 3 for RGB24); W/H are the image's, for the interpolators.
template <int FMT>
struct LdsSrc {
  const uint8_t* lds;
  int32_t x0, y0, w, h;
  int32_t W, H;
  Src<FMT> g;
  __device__ __forceinline__ Px at(int32_t x, int32_t y) const {
    const int32_t u = x - x0, v = y - y0;
    if (u < 0 || v < 0 || u >= w || v >= h) return g.at(x, y);  // never for in-bound tiles
    if (FMT == F_RGB24) {
      const uint8_t* q = lds + 3 * (v * w + u);
      return Px{q[0], q[1], q[2]};
    }
    const uint8_t q = lds[v * w + u];
    return Px{q, q, q};
  }
};

template <int FMT>
__global__ void __launch_bounds__(kThreads) k_rotate_mask(PlaneRef src, PlaneRef dst,
                                                          const RotateArgs* args, int interp) {
  constexpr int CH = FMT == F_RGB24 ? 3 : 1;
  __shared__ uint8_t stage[kRotCap * CH];
  const int s = blockIdx.z;
  const RotateArgs a = args[s];
  if (!a.active) return;
  const Planes& P = src.P;
  const uint8_t* sbase = plane_ptr(src, s);
  uint8_t* dbase = plane_ptr(dst, s);
  const Rect nm = normalize(a.mask);
  const int32_t sw = nm.x1 - nm.x0 + 1, sh = nm.y1 - nm.y0 + 1;
  // center_of_rectangle (primitives.c:137-145)
  const float scx = nm.x0 + sw / 2.0f, scy = nm.y0 + sh / 2.0f;
  const float tcx = 0 + sw / 2.0f, tcy = 0 + sh / 2.0f;
  const Src<FMT> S{sbase, P.pitch, P.W, P.H};
  const int32_t tx0 = blockIdx.x * kRotTW, ty0 = blockIdx.y * kRotTH;
  // in-mask part of the tile, in mask coordinates (u, v)
  const int32_t u0 = imax(tx0, 0) - a.mask.x0, u1 = imin(tx0 + kRotTW, P.W) - 1 - a.mask.x0;
  const int32_t v0 = imax(ty0, 0) - a.mask.y0, v1 = imin(ty0 + kRotTH, P.H) - 1 - a.mask.y0;
  const int32_t cu0 = imax(u0, 0), cu1 = imin(u1, sw - 1);
  const int32_t cv0 = imax(v0, 0), cv1 = imin(v1, sh - 1);
  const bool any_in = cu0 <= cu1 && cv0 <= cv1;
  // source bounding box of the in-mask part (linear map: extremes at corners)
  int32_t bx0 = 0, by0 = 0, bw = 0, bh = 0;
  bool staged = false;
  if (any_in) {
    float mnx = 3.0e38f, mxx = -3.0e38f, mny = 3.0e38f, mxy = -3.0e38f;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const int32_t u = c & 1 ? cu1 : cu0, v = c & 2 ? cv1 : cv0;
      const float X = scx + (u - tcx) * a.cosval + (v - tcy) * a.sinval;
      const float Y = scy + (v - tcy) * a.cosval - (u - tcx) * a.sinval;
      mnx = fminf(mnx, X);
      mxx = fmaxf(mxx, X);
      mny = fminf(mny, Y);
      mxy = fmaxf(mxy, Y);
    }
    // taps: cubic (int)c-1 .. (int)c+2 (trunc, so up to floor+3 for negative
    // c), bilinear floor..ceil, NN round; one more pixel each side absorbs
    // the rounding of per-pixel coordinates against the corner values
    bx0 = (int32_t)floorf(mnx) - 3;
    by0 = (int32_t)floorf(mny) - 3;
    bw = (int32_t)floorf(mxx) + 4 - bx0 + 1;
    bh = (int32_t)floorf(mxy) + 4 - by0 + 1;
    staged = bw > 0 && bh > 0 && (int64_t)bw * bh <= kRotCap;
  }
  if (staged) {
    // all loads of a round are issued before the LDS stores
    const int n = bw * bh;
    for (int base = 0; base < n; base += 8 * kThreads) {
      uint8_t v[8][CH];
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int i = base + k * kThreads + threadIdx.x;
        const int32_t x = bx0 + i % bw, y = by0 + i / bw;
#pragma unroll
        for (int c = 0; c < CH; c++) v[k][c] = 255;
        if (i < n && x >= 0 && y >= 0 && x < P.W && y < P.H) {
          const Px p = load_px_row<FMT>(sbase + (int64_t)y * P.pitch, x);
          v[k][0] = p.r;
          if (CH == 3) {
            v[k][1] = p.g;
            v[k][2] = p.b;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int i = base + k * kThreads + threadIdx.x;
        if (i < n) {
#pragma unroll
          for (int c = 0; c < CH; c++) stage[i * CH + c] = v[k][c];
        }
      }
    }
  }
  __syncthreads();
  const LdsSrc<FMT> L{stage, bx0, by0, bw, bh, P.W, P.H, S};
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int32_t x = tx0 + lane;
  if (x >= P.W) return;
  const int32_t u = x - a.mask.x0;
#pragma unroll
  for (int k = 0; k < kRotTH / 4; k++) {
    const int32_t y = ty0 + w + 4 * k;
    if (y >= P.H) break;
    uint8_t* drow = dbase + (int64_t)y * P.pitch;
    const int32_t v = y - a.mask.y0;
    if (u >= 0 && u < sw && v >= 0 && v < sh) {
      const float srcX = scx + (u - tcx) * a.cosval + (v - tcy) * a.sinval;
      const float srcY = scy + (v - tcy) * a.cosval - (u - tcx) * a.sinval;
      if (FMT != F_RGB24 && staged && interp == UPHIP_INTERP_CUBIC) {
        // gray bicubic straight from the window: the 4x4 taps of (int)srcX,
        // (int)srcY lie inside it by construction of the bounding box
        const int ix = (int)srcX, iy = (int)srcY;
        const uint8_t* t = stage + (iy - 1 - by0) * bw + (ix - 1 - bx0);
        const float fx = srcX - ix;
        uint8_t col[4];
#pragma unroll
        for (int r = 0; r < 4; r++, t += bw) col[r] = cubic_scale(fx, t[0], t[1], t[2], t[3]);
        const uint8_t o = cubic_scale(srcY - iy, col[0], col[1], col[2], col[3]);
        store_px_row<FMT>(drow, x, Px{o, o, o});
        continue;
      }
      const Px o = staged ? interpolate<FMT>(L, srcX, srcY, interp)
                          : interpolate<FMT>(S, srcX, srcY, interp);
      store_px_row<FMT>(drow, x, o);
    } else {
      copy_px_raw<FMT>(drow, x, sbase + (int64_t)y * P.pitch, x);
    }
  }
}

// cubic_scale (interpolate.c:24-31) on integer taps.  Its integer-valued
// subexpressions -- 2a-5b+4c-d, 3(b-c)+d-a and c-a -- are exact in float
// (|x| < 2^24), so they are formed in int and converted; the six rounding
// operations remain, in the reference's order:
//   b + (0.5f*f) * ((c-a) + f * ((2a-5b+4c-d) + f * (3(b-c)+d-a)))
__device__ __forceinline__ uint8_t cubic_int(float f, float h, int a, int b, int c, int d) {
  const float s2 = (float)(3 * (b - c) + d - a);
  const float s1 = (float)(2 * a - 5 * b + 4 * c - d);
  const float u = s1 + f * s2;
  const float v = (float)(c - a) + f * u;
  const int r = (int)((float)b + h * v);
  return (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));  // av_clip_uint8
}

// deskew rotate for a gray plane with bicubic interpolation (Y400A):
// k_rotate_mask's tiling and staging, with the taps read straight from the
// window and no other interpolation code in the kernel.
constexpr int kRotGH = 32;     // output rows per tile of the gray bicubic kernel
constexpr int kRotGCap = 6144; // its staged pixels per tile

template <int FMT>
__global__ void __launch_bounds__(kThreads) k_rotate_cubic_gray(PlaneRef src, PlaneRef dst,
                                                                const RotateArgs* args) {
  __shared__ uint32_t stage32[kRotGCap / 4];
  uint8_t* stage = reinterpret_cast<uint8_t*>(stage32);
  // XCD-aware tile order: neighbouring windows share rows, fetched into one L2
  int txi, tyi, s;
  xcd_block(&txi, &tyi, &s);
  const RotateArgs a = args[s];
  if (!a.active) return;
  const Planes& P = src.P;
  const uint8_t* sbase = plane_ptr(src, s);
  uint8_t* dbase = plane_ptr(dst, s);
  const Rect nm = normalize(a.mask);
  const int32_t sw = nm.x1 - nm.x0 + 1, sh = nm.y1 - nm.y0 + 1;
  const float scx = nm.x0 + sw / 2.0f, scy = nm.y0 + sh / 2.0f;  // primitives.c:137-145
  const float tcx = 0 + sw / 2.0f, tcy = 0 + sh / 2.0f;
  const int32_t tx0 = txi * kRotTW, ty0 = tyi * kRotGH;
  const int32_t u0 = imax(tx0, 0) - a.mask.x0, u1 = imin(tx0 + kRotTW, P.W) - 1 - a.mask.x0;
  const int32_t v0 = imax(ty0, 0) - a.mask.y0, v1 = imin(ty0 + kRotGH, P.H) - 1 - a.mask.y0;
  const int32_t cu0 = imax(u0, 0), cu1 = imin(u1, sw - 1);
  const int32_t cv0 = imax(v0, 0), cv1 = imin(v1, sh - 1);
  int32_t bx0 = 0, by0 = 0, bw = 0, bh = 0;
  bool staged = false;
  if (cu0 <= cu1 && cv0 <= cv1) {
    float mnx = 3.0e38f, mxx = -3.0e38f, mny = 3.0e38f, mxy = -3.0e38f;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const int32_t u = c & 1 ? cu1 : cu0, v = c & 2 ? cv1 : cv0;
      const float X = scx + (u - tcx) * a.cosval + (v - tcy) * a.sinval;
      const float Y = scy + (v - tcy) * a.cosval - (u - tcx) * a.sinval;
      mnx = fminf(mnx, X);
      mxx = fmaxf(mxx, X);
      mny = fminf(mny, Y);
      mxy = fmaxf(mxy, Y);
    }
    bx0 = (int32_t)floorf(mnx) - 3;
    by0 = (int32_t)floorf(mny) - 3;
    bw = (int32_t)floorf(mxx) + 4 - bx0 + 1;
    bh = (int32_t)floorf(mxy) + 4 - by0 + 1;
    staged = bw > 0 && bh > 0;
  }
  // gray planes stage whole aligned dwords: row r of the window starts at
  // byte `lead` of a `sstride`-byte LDS row
  const int32_t xa = bx0 >= 0 ? (bx0 & ~3) : -((-bx0 + 3) & ~3);
  const int lead = FMT == F_GRAY8 ? bx0 - xa : 0;
  const int nd = (lead + bw + 3) >> 2;
  const int sstride = FMT == F_GRAY8 ? 4 * nd : bw;
  staged = staged && (int64_t)sstride * bh <= kRotGCap;
  if (staged && FMT == F_GRAY8) {
    const int n = nd * bh;
    for (int b0 = 0; b0 < n; b0 += 8 * kThreads) {
      uint32_t v[8];
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int i = b0 + k * kThreads + threadIdx.x;
        const int r = i / nd;
        const int32_t xd = xa + 4 * (i - r * nd), y = by0 + r;
        const bool row_ok = (y >= 0) & (y < P.H);
        const uint8_t* row = sbase + (int64_t)imin(imax(y, 0), P.H - 1) * P.pitch;
        // interior dwords: one aligned load (xd is a multiple of 4)
        v[k] = *reinterpret_cast<const uint32_t*>(row + imin(imax(xd, 0), (int32_t)P.pitch - 4));
        if (!row_ok) v[k] = 0xFFFFFFFFu;
      }
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int i = b0 + k * kThreads + threadIdx.x;
        if (i >= n) continue;
        const int r = i / nd;
        const int32_t xd = xa + 4 * (i - r * nd), y = by0 + r;
        uint32_t w4 = v[k];
        if ((y >= 0) & (y < P.H) & ((xd < 0) | (xd + 3 >= P.W))) {
          // a dword across the image edge: white outside, bytes inside
          const uint8_t* row = sbase + (int64_t)y * P.pitch;
          w4 = 0;
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const int32_t x = xd + j;
            const uint32_t b = (x >= 0 && x < P.W) ? row[x] : 255u;
            w4 |= b << (8 * j);
          }
        }
        stage32[i] = w4;
      }
    }
  } else if (staged) {
    // unconditional clamped loads (white off the image), all of a round in flight
    const int n = bw * bh;
    for (int b0 = 0; b0 < n; b0 += 8 * kThreads) {
      uint8_t v[8];
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int i = b0 + k * kThreads + threadIdx.x;
        const int r = i / bw;
        const int32_t x = bx0 + (i - r * bw), y = by0 + r;
        const bool ok = (x >= 0) & (y >= 0) & (x < P.W) & (y < P.H);
        const uint8_t q = load_px_row<FMT>(sbase + (int64_t)imin(imax(y, 0), P.H - 1) * P.pitch,
                                           imin(imax(x, 0), P.W - 1)).r;
        v[k] = ok ? q : (uint8_t)255;
      }
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int i = b0 + k * kThreads + threadIdx.x;
        if (i < n) stage[i] = v[k];
      }
    }
  }
  __syncthreads();
  const Src<FMT> S{sbase, P.pitch, P.W, P.H};
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int32_t x = tx0 + lane;
  if (x >= P.W) return;
  const int32_t u = x - a.mask.x0;
#pragma unroll
  for (int k = 0; k < kRotGH / 4; k++) {
    const int32_t y = ty0 + w + 4 * k;
    if (y >= P.H) break;
    uint8_t* drow = dbase + (int64_t)y * P.pitch;
    const int32_t v = y - a.mask.y0;
    if (u >= 0 && u < sw && v >= 0 && v < sh) {
      const float srcX = scx + (u - tcx) * a.cosval + (v - tcy) * a.sinval;
      const float srcY = scy + (v - tcy) * a.cosval - (u - tcx) * a.sinval;
      uint8_t o;
      if (staged) {
        const int ix = (int)srcX, iy = (int)srcY;  // interp_bicubic truncates
        const float fx = srcX - ix, fy = srcY - iy;
        const float hx = 0.5f * fx, hy = 0.5f * fy;
        const uint8_t* t = stage + (iy - 1 - by0) * sstride + lead + (ix - 1 - bx0);
        int col[4];
#pragma unroll
        for (int r = 0; r < 4; r++, t += sstride)
          col[r] = cubic_int(fx, hx, t[0], t[1], t[2], t[3]);
        o = cubic_int(fy, hy, col[0], col[1], col[2], col[3]);
      } else {
        o = interp_bicubic(S, srcX, srcY).r;
      }
      store_px_row<FMT>(drow, x, Px{o, o, o});
    } else {
      copy_px_raw<FMT>(drow, x, sbase + (int64_t)y * P.pitch, x);
    }
  }
}

// ---------------------------------------------------------------------------
// deskew rotate, GRAY8 + bicubic (the default pipeline): 256 x 32 output tiles,
// four horizontally adjacent pixels per lane and row, so one dword store per
// lane and the float work in pairs of pixels on packed FP32 (v_pk_mul/add/fma).
//   * the window is staged with a fixed 288-byte row stride, so the four tap
//     rows of a pixel are one ds_read2_b32 each at immediate offsets, and
//     v_alignbyte extracts its four taps;
//   * the integer-valued terms of cubic_scale (2a-5b+4c-d, 3(b-c)+d-a, c-a)
//     are formed by exact packed FMAs on float-valued bytes (every
//     intermediate is an integer below 2^24); the six rounding operations stay
//     separate multiplies and adds in the reference's order
//     (interpolate.c:24-31), so results are bit-identical.
// ---------------------------------------------------------------------------
typedef float f2 __attribute__((ext_vector_type(2)));
constexpr int kRQW = 256;              // output columns per tile (4 per lane)
constexpr int kRQH = 32;               // output rows per tile
constexpr int kRQStride = 72;          // staged row stride in dwords (>= window 269 B)
constexpr int kRQRows = 84;            // staged rows
constexpr int kRQWords = kRQStride * kRQRows + 2;

__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 splat2(float v) { return f2{v, v}; }

// cubic_scale on float-valued taps, truncated and clipped like av_clip_uint8
// (the result is an integer-valued float).  The integer-valued terms are
// formed from the differences ba = b-a, ca = c-a, da = d-a:
//   2a-5b+4c-d = -5ba + 4ca - da,   3(b-c)+d-a = 3(ba-ca) + da
// The integer coefficients of cubic_scale (interpolate.c:24-31) for taps
// a..d, exact in fp32 (|values| <= 1530), in six packed operations:
//   ca = c - a,  s2 = 3(b - c) + (d - a),  s1 = 2a - 5b + 4c - d
//                                         = -5(b - c) - ((d - a) + (c - a))
__device__ __forceinline__ void cubic_terms(f2 a, f2 b, f2 c, f2 d, f2& ca, f2& s1, f2& s2) {
  const f2 e = d - a, g = b - c;
  ca = c - a;
  s2 = fma2(splat2(3.0f), g, e);
  s1 = fma2(splat2(-5.0f), g, -(e + ca));
}

__device__ __forceinline__ f2 cubic2(f2 f, f2 h, f2 a, f2 b, f2 c, f2 d) {
  f2 ca, s1, s2;
  cubic_terms(a, b, c, d, ca, s1, s2);  // exact
  const f2 u = s1 + f * s2;
  const f2 v = ca + f * u;
  const f2 r = b + h * v;
  return f2{__builtin_amdgcn_fmed3f(__builtin_truncf(r.x), 0.0f, 255.0f),
            __builtin_amdgcn_fmed3f(__builtin_truncf(r.y), 0.0f, 255.0f)};
}

// byte K of w as a float.  Inline asm keeps the value opaque: otherwise the
// compiler turns differences of converted bytes back into integer subtracts
// plus conversions, which defeats the packed arithmetic.
template <int K>
__device__ __forceinline__ float ubyte_f(uint32_t w) {
  float r;
  if constexpr (K == 0) asm("v_cvt_f32_ubyte0 %0, %1" : "=v"(r) : "v"(w));
  else if constexpr (K == 1) asm("v_cvt_f32_ubyte1 %0, %1" : "=v"(r) : "v"(w));
  else if constexpr (K == 2) asm("v_cvt_f32_ubyte2 %0, %1" : "=v"(r) : "v"(w));
  else asm("v_cvt_f32_ubyte3 %0, %1" : "=v"(r) : "v"(w));
  return r;
}
template <int K>
__device__ __forceinline__ f2 tap2(uint32_t p, uint32_t q) {
  return f2{ubyte_f<K>(p), ubyte_f<K>(q)};
}

__global__ void __launch_bounds__(kThreads) k_rotate_cubic_g8(PlaneRef src, PlaneRef dst,
                                                              const RotateArgs* args) {
  __shared__ uint32_t win[kRQWords];
  int txi, tyi, s;
  xcd_block(&txi, &tyi, &s);  // neighbouring windows share rows, fetched into one L2
  const RotateArgs a = args[s];
  if (!a.active) return;
  const Planes& P = src.P;
  const uint8_t* sbase = plane_ptr(src, s);
  uint8_t* dbase = plane_ptr(dst, s);
  const Rect nm = normalize(a.mask);
  const int32_t sw = nm.x1 - nm.x0 + 1, sh = nm.y1 - nm.y0 + 1;
  const float scx = nm.x0 + sw / 2.0f, scy = nm.y0 + sh / 2.0f;  // primitives.c:137-145
  const float tcx = 0 + sw / 2.0f, tcy = 0 + sh / 2.0f;
  const int32_t tx0 = txi * kRQW, ty0 = tyi * kRQH;
  const int32_t u0 = imax(tx0, 0) - a.mask.x0, u1 = imin(tx0 + kRQW, P.W) - 1 - a.mask.x0;
  const int32_t v0 = imax(ty0, 0) - a.mask.y0, v1 = imin(ty0 + kRQH, P.H) - 1 - a.mask.y0;
  const int32_t cu0 = imax(u0, 0), cu1 = imin(u1, sw - 1);
  const int32_t cv0 = imax(v0, 0), cv1 = imin(v1, sh - 1);
  // source window of the tile's in-mask pixels (their 4x4 taps included)
  int32_t bx0 = 0, by0 = 0, bw = 0, bh = 0;
  if (cu0 <= cu1 && cv0 <= cv1) {
    float mnx = 3.0e38f, mxx = -3.0e38f, mny = 3.0e38f, mxy = -3.0e38f;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const int32_t u = c & 1 ? cu1 : cu0, v = c & 2 ? cv1 : cv0;
      const float X = scx + (u - tcx) * a.cosval + (v - tcy) * a.sinval;
      const float Y = scy + (v - tcy) * a.cosval - (u - tcx) * a.sinval;
      mnx = fminf(mnx, X);
      mxx = fmaxf(mxx, X);
      mny = fminf(mny, Y);
      mxy = fmaxf(mxy, Y);
    }
    bx0 = (int32_t)floorf(mnx) - 3;
    by0 = (int32_t)floorf(mny) - 3;
    bw = (int32_t)floorf(mxx) + 4 - bx0 + 1;
    bh = (int32_t)floorf(mxy) + 4 - by0 + 1;
  }
  const int32_t xa = bx0 >= 0 ? (bx0 & ~3) : -((-bx0 + 3) & ~3);  // window start, dword aligned
  const int lead = bx0 - xa;
  const int nd = (lead + bw + 3) >> 2;                               // dwords per window row
  const bool staged = bw > 0 && bh > 0 && nd < kRQStride && bh <= kRQRows;
  if (staged) {
    // row of flat dword index i: i / nd as a multiply-high (exact for
    // i * (m*nd - 2^32) < 2^32, far beyond these sizes)
    const uint32_t m = nd > 1 ? (uint32_t)((0xFFFFFFFFull / (uint32_t)nd) + 1) : 0u;
    const int n = nd * bh;
    for (int b0 = 0; b0 < n; b0 += 8 * kThreads) {
      uint32_t v[8];
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int i = b0 + k * kThreads + threadIdx.x;
        const int r = nd > 1 ? (int)__umulhi((uint32_t)i, m) : i;
        const int32_t xd = xa + 4 * (i - r * nd), y = by0 + r;
        const uint8_t* row = sbase + (int64_t)imin(imax(y, 0), P.H - 1) * P.pitch;
        v[k] = *reinterpret_cast<const uint32_t*>(row + imin(imax(xd, 0), (int32_t)P.pitch - 4));
        if ((y < 0) | (y >= P.H)) v[k] = 0xFFFFFFFFu;
      }
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int i = b0 + k * kThreads + threadIdx.x;
        if (i >= n) continue;
        const int r = nd > 1 ? (int)__umulhi((uint32_t)i, m) : i;
        const int j = i - r * nd;
        const int32_t xd = xa + 4 * j, y = by0 + r;
        uint32_t w4 = v[k];
        if ((y >= 0) & (y < P.H) & ((xd < 0) | (xd + 3 >= P.W))) {
          // a dword across the image edge: white outside, bytes inside
          const uint8_t* row = sbase + (int64_t)y * P.pitch;
          w4 = 0;
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const int32_t x = xd + q;
            const uint32_t b = (x >= 0 && x < P.W) ? row[x] : 255u;
            w4 |= b << (8 * q);
          }
        }
        win[r * kRQStride + j] = w4;
      }
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int32_t xl = tx0 + 4 * lane;
  if (xl >= P.W) return;
  // per-lane terms of the source coordinates (constant down the column):
  //   srcX = (scx + (u - tcx) cos) + (v - tcy) sin
  //   srcY = (scy + (v - tcy) cos) - (u - tcx) sin
  float ax[4], bs[4];
  bool colin[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int32_t u = xl + j - a.mask.x0;
    const float cu = u - tcx;
    ax[j] = scx + cu * a.cosval;
    bs[j] = cu * a.sinval;
    colin[j] = (u >= 0) & (u < sw) & (xl + j < P.W);
  }
  const f2 AX0{ax[0], ax[1]}, AX1{ax[2], ax[3]}, BS0{bs[0], bs[1]}, BS1{bs[2], bs[3]};
  const int base_off = (-1 - by0) * (4 * kRQStride) + lead - 1 - bx0;  // tap (ix-1, iy-1)
  const Src<F_GRAY8> S{sbase, P.pitch, P.W, P.H};
#pragma unroll 2
  for (int k = 0; k < kRQH / 4; k++) {
    const int32_t y = ty0 + w + 4 * k;
    if (y >= P.H) break;
    const int32_t v = y - a.mask.y0;
    const bool rowin = (v >= 0) & (v < sh);
    const float cv = v - tcy;
    const f2 VS = splat2(cv * a.sinval), VC = splat2(scy + cv * a.cosval);
    const f2 SX[2] = {AX0 + VS, AX1 + VS};
    const f2 SY[2] = {VC - BS0, VC - BS1};
    const uint8_t* srow = sbase + (int64_t)y * P.pitch;
    uint32_t out = 0;
    if (staged) {
#pragma unroll
      for (int pr = 0; pr < 2; pr++) {
        const int ix0 = (int)SX[pr].x, ix1 = (int)SX[pr].y;  // interp_bicubic truncates
        const int iy0 = (int)SY[pr].x, iy1 = (int)SY[pr].y;
        const f2 fx = SX[pr] - f2{(float)ix0, (float)ix1};
        const f2 fy = SY[pr] - f2{(float)iy0, (float)iy1};
        const f2 hx = 0.5f * fx, hy = 0.5f * fy;
        const bool in0 = rowin & colin[2 * pr], in1 = rowin & colin[2 * pr + 1];
        const int o0 = in0 ? base_off + iy0 * (4 * kRQStride) + ix0 : 0;
        const int o1 = in1 ? base_off + iy1 * (4 * kRQStride) + ix1 : 0;
        const uint32_t* w0 = win + (o0 >> 2);
        const uint32_t* w1 = win + (o1 >> 2);
        f2 col[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const uint32_t p = __builtin_amdgcn_alignbyte(w0[r * kRQStride + 1], w0[r * kRQStride], o0);
          const uint32_t q = __builtin_amdgcn_alignbyte(w1[r * kRQStride + 1], w1[r * kRQStride], o1);
          col[r] = cubic2(fx, hx, tap2<0>(p, q), tap2<1>(p, q), tap2<2>(p, q), tap2<3>(p, q));
        }
        const f2 o = cubic2(fy, hy, col[0], col[1], col[2], col[3]);
        // integer-valued in [0, 255]: the conversion is exact whatever its rounding
        out = __builtin_amdgcn_cvt_pk_u8_f32(o.x, 2 * pr, out);
        out = __builtin_amdgcn_cvt_pk_u8_f32(o.y, 2 * pr + 1, out);
      }
    } else {
      // window too tall for LDS (large angles): taps from the frame
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const f2 sx = SX[j >> 1], sy = SY[j >> 1];
        const float fx = (j & 1) ? sx.y : sx.x, fy = (j & 1) ? sy.y : sy.x;
        if (rowin & colin[j]) out |= (uint32_t)interp_bicubic(S, fx, fy).r << (8 * j);
      }
    }
    // outside the mask the pixel is copied unchanged (deskew.c:268-286)
    uint32_t inmask = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) inmask |= (rowin & colin[j]) ? 0xFFu << (8 * j) : 0u;
    uint8_t* drow = dbase + (int64_t)y * P.pitch;
    if (xl + 3 < P.W) {
      if (inmask != 0xFFFFFFFFu)
        out = (out & inmask) | (*reinterpret_cast<const uint32_t*>(srow + xl) & ~inmask);
      *reinterpret_cast<uint32_t*>(drow + xl) = out;
    } else {
      for (int j = 0; xl + j < P.W; j++)
        drow[xl + j] = (inmask >> (8 * j)) & 1 ? (uint8_t)(out >> (8 * j)) : srow[xl + j];
    }
  }
}

// ---------------------------------------------------------------------------
// deskew rotate, GRAY8 + bicubic, float window (the default pipeline's
// dominant kernel).  128 x 48 output tiles; the tile's source window is
// staged once as fp32 (one conversion per staged byte instead of one per
// tap), so the taps of a pixel come straight out of LDS in the pairs the
// packed FP32 ops consume:
//   * a lane owns output columns tx0+lane and tx0+64+lane (A, B); the row
//     cubics of one pixel run two tap rows at a time, each tap pair (row r,
//     row r+1) one ds_read2_b32 at offsets (k, kRFS+k);
//   * the vertical cubic runs A and B as one packed pair;
//   * lanes read consecutive columns (a wave whose pixels straddle a row
//     boundary meets at most two-way bank conflicts);
//   * all-white stretches of a tile row (the page background) are detected
//     from per-row non-white masks built while staging and skip the math;
//   * a tile's rows are dealt to its eight waves round-robin (wave w: tile
//     rows w, w + 8, ..., w + 40; rot_wave_row, rot_tiles.h), so that a band of
//     text, a run of non-white rows, costs every wave about the same and no
//     wave idles at the tile's last barrier for the others;
//   * each wave buffers its six output rows in LDS and stores them 8 bytes
//     per lane at the end (no global load after a store).
// Every rounding operation of cubic_scale (interpolate.c:24-31) stays a
// separate multiply or add in the reference's order, as in cubic2.
// ---------------------------------------------------------------------------
// kRFW x kRFH output tiles, kRFS floats a staged row: rot_tiles.h
constexpr int kRFT = 512;   // threads per tile: 8 waves, kRFH / 8 rows each (rot_wave_row)
static_assert(kRFWaves == kRFT / 64 && kRFH % kRFWaves == 0, "rot_wave_row deals kRFH rows to kRFT / 64 waves");

// The 16 taps of pixels A and B as row pairs: t[p][j] = {tap row 2q, tap row
// 2q+1} of column j for p = 2*pixel + q.  a[p] is the LDS byte address of
// (column 0, row 2q).  One ds_read2_b32 per pair (offsets k and kRFS + k,
// which the compiler would instead merge as k, k+1 and then shuffle), all 16
// in flight before the one wait.
#define UPH_TAP_PAIR(o, b, k) \
  "ds_read2_b32 %" #o ", %" #b " offset0:" #k " offset1:" UPH_STR(UPH_ROWOFF_##k) "\n\t"
#define UPH_STR2(x) #x
#define UPH_STR(x) UPH_STR2(x)
#define UPH_ROWOFF_0 144
#define UPH_ROWOFF_1 145
#define UPH_ROWOFF_2 146
#define UPH_ROWOFF_3 147
static_assert(kRFS == 144, "tap pair offsets are spelled out for a 144-float row stride");
// Issued in pair order t[0], t[1] (pixel A), t[2], t[3] (pixel B) with no
// wait: the caller waits for A's eight (lds_wait_a) and computes A's row
// cubics while B's are still in flight (LDS returns in order).
__device__ __forceinline__ void lds_taps16(const uint32_t (&a)[4], f2 (&t)[4][4]) {
  asm volatile(UPH_TAP_PAIR(0, 16, 0) UPH_TAP_PAIR(1, 16, 1) UPH_TAP_PAIR(2, 16, 2)
               UPH_TAP_PAIR(3, 16, 3) UPH_TAP_PAIR(4, 17, 0) UPH_TAP_PAIR(5, 17, 1)
               UPH_TAP_PAIR(6, 17, 2) UPH_TAP_PAIR(7, 17, 3) UPH_TAP_PAIR(8, 18, 0)
               UPH_TAP_PAIR(9, 18, 1) UPH_TAP_PAIR(10, 18, 2) UPH_TAP_PAIR(11, 18, 3)
               UPH_TAP_PAIR(12, 19, 0) UPH_TAP_PAIR(13, 19, 1) UPH_TAP_PAIR(14, 19, 2)
               UPH_TAP_PAIR(15, 19, 3)
               : "=&v"(t[0][0]), "=&v"(t[0][1]), "=&v"(t[0][2]), "=&v"(t[0][3]),
                 "=&v"(t[1][0]), "=&v"(t[1][1]), "=&v"(t[1][2]), "=&v"(t[1][3]),
                 "=&v"(t[2][0]), "=&v"(t[2][1]), "=&v"(t[2][2]), "=&v"(t[2][3]),
                 "=&v"(t[3][0]), "=&v"(t[3][1]), "=&v"(t[3][2]), "=&v"(t[3][3])
               : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3])
               : "memory");
}
// Wait until <= N LDS operations are outstanding: tap pair t becomes
// defined here; `prev` (the previous pair's result) must be computed above
// the wait, so each pair's arithmetic overlaps the later pairs' reads.
template <int N>
__device__ __forceinline__ void lds_wait_pair(f2 (&t)[4]) {
  asm volatile("s_waitcnt lgkmcnt(%4)"
               : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3])
               : "n"(N)
               : "memory");
}
template <int N>
__device__ __forceinline__ void lds_wait_pair_after(f2 (&t)[4], f2& prev) {
  asm volatile("s_waitcnt lgkmcnt(%5)"
               : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(prev)
               : "n"(N)
               : "memory");
}

// one packed row cubic (rows 2q, 2q+1 of one pixel), clamped like cubic_scale
__device__ __forceinline__ f2 cubic2_row_u(f2 f, f2 h, const f2 (&t)[4]) {
  f2 ca, s1, s2;
  cubic_terms(t[0], t[1], t[2], t[3], ca, s1, s2);  // exact
  f2 u = f * s2;
  u = s1 + u;
  u = f * u;
  u = ca + u;
  u = h * u;
  return t[1] + u;
}
// cubic_scale's truncation and clamp of one result
__device__ __forceinline__ float clamp_t255(float u) {
  return __builtin_amdgcn_fmed3f(__builtin_truncf(u), 0.0f, 255.0f);
}

// v from the lane given by the quad permutation CTRL (DPP quad_perm)
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, false));
}

// Byte offset of row y (0 <= y < H) as a 32-bit product: the launcher only
// picks k_rotate_cubic_g8f when pitch * H < 2^31 (one scalar multiply per row
// instead of a 64-bit product).
__device__ __forceinline__ uint32_t row_off(int32_t y, int64_t pitch) {
  return (uint32_t)y * (uint32_t)pitch;
}

#ifndef UPH_ROT_MINB
#define UPH_ROT_MINB 8
#endif
#ifdef UPHIP_DIAG
// tuning build: per-phase shader clocks of wave 0 of every in-mask tile
// (UPHIP_DIAG_DOUBLE bit 65536), summed; [7] counts the tiles
// (spread over 1024 slots by block so the counters do not contend)
__device__ unsigned long long g_rot_phase[1024 * 8];
#define UPH_ROT_T(k)                                                         \
  if (UPH_DIAG_BITS(diag, 65536) && threadIdx.x == 0) {                     \
    const unsigned long long tn = wall_clock64();                            \
    atomicAdd(&g_rot_phase[8 * (blockIdx.x & 1023) + (k)], tn - tprev);      \
    tprev = tn;                                                              \
  }
// (UPHIP_DIAG_DOUBLE bit 524288) the row loop's clocks of every wave of an
// in-mask tile, by tile record: the sum over the tile's waves and the slowest
// wave (how evenly rot_wave_row deals the non-white rows)
constexpr int kRotWaveSlots = 1 << 18;
__device__ unsigned int g_rot_wsum[kRotWaveSlots], g_rot_wmax[kRotWaveSlots];
#else
#define UPH_ROT_T(k)
#endif
// The sheet's planes come out of its record, so the compiler cannot see that
// they are global memory: without these, every access through them becomes a
// flat instruction (which also counts as an LDS operation in the waits).
template <class T>
__device__ __forceinline__ T gload(const uint8_t* p) {
  return *(const __attribute__((address_space(1))) T*)p;
}
template <class T>
__device__ __forceinline__ void gstore(uint8_t* p, T v) {
  *(__attribute__((address_space(1))) T*)p = v;
}

// The plane's geometry: what the kernel needs of Planes (pitch * H < 2^31).
struct RotPlane {
  int32_t W, H;
  uint32_t pitch;
};

// The per-sheet constants, the window and the class of every tile of every
// active sheet (rot_tiles.h), written once per launch so that the rotation's
// tiles read them instead of deriving them.  One thread per tile, one block
// row per sheet; block (0, 0) also counts the launch's large-window sheets.
//   cls_rows: 0 = one launch takes every sheet with rows_small window rows;
//   else sheets that need more than cls_rows rows are `large` (rows_large).
__global__ void __launch_bounds__(256) k_rot_tiles(PlaneRef src, PlaneRef dst, const RotateArgs* args,
                                                   int count, int tgx, int tgy, int rows_small,
                                                   int rows_large, int cls_rows, RotSheet* sheets,
                                                   RotTile* tiles, uint32_t* nlarge) {
  const int s = blockIdx.y;
  if (blockIdx.x == 0 && s == 0) {
    __shared__ uint32_t n_s;
    if (threadIdx.x == 0) n_s = 0;
    __syncthreads();
    uint32_t c = 0;
    if (cls_rows)
      for (int q = threadIdx.x; q < count; q += blockDim.x)
        c += args[q].active && rot_need_rows(args[q].sinval) > cls_rows;
    if (c) atomicAdd(&n_s, c);
    __syncthreads();
    if (threadIdx.x == 0) *nlarge = n_s;
  }
  const RotateArgs a = args[s];
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  if (!a.active) {  // the rotation reads no other field of an inactive sheet
    if (first) sheets[s].active = 0, sheets[s].large = 0;
    return;
  }
  RotSheet g;
  rot_sheet_geom(a.mask.x0, a.mask.y0, a.mask.x1, a.mask.y1, a.sinval, a.cosval, &g);
  g.src = plane_ptr(src, s);
  g.dst = plane_ptr(dst, s);
  g.active = 1;
  g.large = cls_rows && rot_need_rows(a.sinval) > cls_rows;
  if (first) sheets[s] = g;
  const int ti = blockIdx.x * blockDim.x + threadIdx.x;
  if (ti >= tgx * tgy) return;
  const int tyi = ti / tgx;
  tiles[(int64_t)s * (tgx * tgy) + ti] =
      rot_tile(&g, src.P.W, src.P.H, ti - tyi * tgx, tyi, g.large ? rows_large : rows_small);
}

// sheets / tiles: k_rot_tiles' records of this launch; tiles[s * tiles-per-
// sheet + tyi * (tiles per row) + txi].  LOOP: the large-window launch.
template <bool LOOP>
__global__ void __launch_bounds__(kRFT, UPH_ROT_MINB) k_rotate_cubic_g8f(
    const RotSheet* __restrict__ sheets, const RotTile* __restrict__ tiles,
    const uint32_t* __restrict__ nlarge, RotPlane P, int max_rows, int diag, uint32_t m_gxy,
    uint32_t m_gx, int loop_count, int tgx, int tgy, uint32_t* colsum, int64_t cs_stride) {
  // dynamic LDS: window [max_rows][kRFS] floats, nw[max_rows] u64, then one
  // (kRFH / 8) x kRFW byte output buffer per wave (its row k: the wave's k-th row)
  extern __shared__ __attribute__((aligned(16))) float winf[];
  // colsum (optional): the output's column sums over all rows, added into
  // colsum[s * cs_stride + x] (the next mask scan's, masks.c:54-209), so that
  // scan need not read the rotated plane again; per tile summed in LDS, then
  // one atomic per column
  __shared__ uint32_t csum_s[kRFW];
  // tile (txi, tyi) of sheet s, record ti; every return is block-uniform
  auto tile = [&](int txi, int tyi, int s, int ti) {
#ifdef UPHIP_DIAG
  unsigned long long tprev = wall_clock64();
#endif
  // Both records sit at addresses made of the block index and the kernel's
  // arguments alone: two independent scalar loads, one wait.  Nothing of the
  // tile's geometry is derived here (rot_tiles.h, k_rot_tiles).
  const RotTile T = tiles[ti];
  const RotSheet a = sheets[s];
  UPH_ROT_T(0)
  // (both records wanted whole right here, before the first branch on one of
  // their fields, and with them the arguments not fetched yet: otherwise the
  // compiler fetches them piece by piece, each piece behind the branch that
  // first needs it, one wait per piece)
  asm volatile("" ::"s"(T.bx0), "s"((uint32_t)T.bw), "s"(T.flags), "s"(a.src), "s"(a.dst),
               "s"(a.mx0), "s"(a.sw), "s"(a.scx), "s"(a.tcx), "s"(a.sinval), "s"(a.active),
               "s"(P.W), "s"(P.H), "s"(P.pitch), "s"(colsum), "s"(cs_stride));
  if (!a.active || (a.large != 0) != LOOP) return;  // each sheet: one of the two launches
  const uint8_t* sbase = a.src;
  uint8_t* dbase = a.dst;
  const int32_t sw = a.sw, sh = a.sh;
  const float scx = a.scx, scy = a.scy, tcx = a.tcx, tcy = a.tcy;
  const int32_t tx0 = txi * kRFW, ty0 = tyi * kRFH;
  // the tile's column sums (colsum): zeroed here, added per row below
  auto csum_flush = [&]() {
    __syncthreads();
    if (threadIdx.x < kRFW && tx0 + (int)threadIdx.x < P.W)
      atomicAdd(colsum + s * cs_stride + tx0 + threadIdx.x, csum_s[threadIdx.x]);
  };
  // the tile's column sums zeroed; in-mask tiles need no barrier of their
  // own here: the staging barrier below (taken by every in-mask tile, staged
  // or not) orders these writes before any wave's adds, so every wave starts
  // on its window loads as it arrives
  const bool outside_tile = T.flags & ROT_T_OUTSIDE;
  if (colsum) {
    if (threadIdx.x < kRFW) csum_s[threadIdx.x] = 0;
    if (outside_tile) __syncthreads();
  }
  if (outside_tile) {
    // no pixel of the tile inside the mask: copied unchanged (deskew.c:268-286)
    const int cb = 8 * (threadIdx.x & 15);
    const int32_t x = tx0 + cb;
    uint32_t cs8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int r = threadIdx.x >> 4; r < kRFH; r += kRFT / 16) {
      const int32_t y = ty0 + r;
      if (y >= P.H || x >= P.W) continue;
      const uint8_t* sp = sbase + row_off(y, P.pitch) + x;
      uint8_t* dp = dbase + row_off(y, P.pitch) + x;
      if (x + 8 <= P.W) {
        const uint64_t q = gload<uint64_t>(sp);
        gstore<uint64_t>(dp, q);
#pragma unroll
        for (int j = 0; j < 8; j++) cs8[j] += (uint32_t)(q >> (8 * j)) & 0xFFu;
      } else {
        for (int j = 0; x + j < P.W; j++) {
          const uint8_t q = gload<uint8_t>(sp + j);
          gstore<uint8_t>(dp + j, q);
          cs8[j & 7] += q;
        }
      }
    }
    if (colsum) {
#pragma unroll
      for (int j = 0; j < 8; j++) atomicAdd(&csum_s[cb + j], cs8[j]);
      csum_flush();
    }
    return;
  }
  UPH_ROT_T(1)
  const int lane = threadIdx.x & 63;
  const int wu = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // Source window of the tile's in-mask pixels (their 4x4 taps included) and
  // the tile's class, from the record (rot_tile, rot_tiles.h)
  const int32_t bx0 = T.bx0, by0 = T.by0, bw = T.bw, bh = T.bh;
  const int32_t xa = rot_window_xa(bx0);    // window start, dword aligned
  const int nd = rot_window_nd(bx0, bw);    // source dwords per row
  // (bh <= max_rows restated: the LDS window is this launch's)
  const bool staged = (T.flags & ROT_T_STAGED) && bh <= max_rows;
  uint64_t* nw = reinterpret_cast<uint64_t*>(winf + kRFS * max_rows);
  uint8_t* obuf = reinterpret_cast<uint8_t*>(nw + max_rows) + wu * (kRFH / kRFWaves * kRFW);
  if (staged && !UPH_DIAG_BITS(diag, 1024)) {
    // A wave-instruction stages three window rows, 8 bytes per lane: lanes
    // 18 q .. 18 q + 17 load row r + q (q < 3), lanes 54..63 idle.  nw[r] bit j:
    // window bytes 8 j .. 8 j + 7 of row r hold a non-white pixel.
    const int rq = (lane * 57) >> 10;  // lane / 18 for lane < 64
    const int jq = lane - 18 * rq;
    const int nq = (nd + 1) >> 1;
    const bool qv = rq < 3 && jq < nq;
    const int32_t xd = xa + 8 * jq;
    // one wave-instruction's rows: ballot, non-white flags, fp32 window row
    auto stage = [&](int rb, uint32_t w0, uint32_t w1) {
      const int r = rb + rq;
      const bool valid = qv && r < bh;
      const unsigned long long m = __ballot(valid && (w0 & w1) != 0xFFFFFFFFu);
      if (lane < 3 && rb + lane < bh) nw[rb + lane] = (m >> (18 * lane)) & 0x3FFFFull;
      if (valid) {
        float4* d = reinterpret_cast<float4*>(winf + r * kRFS + 8 * jq);
        d[0] = make_float4(ubyte_f<0>(w0), ubyte_f<1>(w0), ubyte_f<2>(w0), ubyte_f<3>(w0));
        d[1] = make_float4(ubyte_f<0>(w1), ubyte_f<1>(w1), ubyte_f<2>(w1), ubyte_f<3>(w1));
      }
    };
    const bool interior = T.flags & ROT_T_INTERIOR;
    if (interior) {
      // the whole window inside the image: straight loads.  A lane's byte
      // offset is its row-rq offset plus a scalar row product per group;
      // lanes past the window's rows (and idle lanes) read their row rq.
      const uint32_t off0 = row_off(by0 + rq, P.pitch) + (uint32_t)(qv ? xd : xa);
      for (int rg = 3 * wu; rg < bh; rg += 3 * 3 * kRFWaves) {
        uint2 v[3];
#pragma unroll
        for (int g = 0; g < 3; g++) {  // all loads of the group in flight
          const int rb = rg + 3 * kRFWaves * g;
          const uint32_t o = rb + rq < bh ? off0 + (uint32_t)rb * (uint32_t)P.pitch : off0;
          const uint64_t q = gload<uint64_t>(sbase + o);
          v[g] = make_uint2((uint32_t)q, (uint32_t)(q >> 32));
        }
#pragma unroll
        for (int g = 0; g < 3; g++) {
          const int rb = rg + 3 * kRFWaves * g;  // the wave's first row of this instruction
          if (rb >= bh) break;                   // uniform
          stage(rb, v[g].x, v[g].y);
        }
      }
    } else {
      // edge tiles load every dword clamped into the row, realign it by one
      // 64-bit shift and make the bytes outside [0, W) x [0, H) white
      const int32_t xc0 = imin(imax(xd, 0), (int32_t)P.pitch - 4);
      const int32_t xc1 = imin(imax(xd + 4, 0), (int32_t)P.pitch - 4);
      const int fs0 = imin(imax(24 + 8 * (xd - xc0), 0), 56);
      const int fs1 = imin(imax(24 + 8 * (xd + 4 - xc1), 0), 56);
      uint32_t out0 = qv ? 0u : 0xFFFFFFFFu, out1 = out0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (xd + k < 0 || xd + k >= P.W) out0 |= 0xFFu << (8 * k);
        if (xd + 4 + k < 0 || xd + 4 + k >= P.W) out1 |= 0xFFu << (8 * k);
      }
      for (int rg = 3 * wu; rg < bh; rg += 3 * 3 * kRFWaves) {
        uint2 v[3];
#pragma unroll
        for (int g = 0; g < 3; g++) {
          const int r = rg + 3 * kRFWaves * g + rq;
          const int32_t y = imin(imax(by0 + r, 0), P.H - 1);
          const uint8_t* row = sbase + row_off(y, P.pitch);
          v[g].x = gload<uint32_t>(row + xc0);
          v[g].y = gload<uint32_t>(row + xc1);
        }
#pragma unroll
        for (int g = 0; g < 3; g++) {
          const int rb = rg + 3 * kRFWaves * g;
          if (rb >= bh) break;
          const int32_t y = by0 + rb + rq;
          uint32_t w0 = (uint32_t)(((uint64_t)v[g].x << 24) >> fs0) | out0;
          uint32_t w1 = (uint32_t)(((uint64_t)v[g].y << 24) >> fs1) | out1;
          if ((y < 0) | (y >= P.H)) w0 = w1 = 0xFFFFFFFFu;
          stage(rb, w0, w1);
        }
      }
    }
  }
  __syncthreads();
  UPH_ROT_T(2)
  const int32_t xA = tx0 + lane, xB = xA + 64;
  const bool hasA = xA < P.W, hasB = xB < P.W;
  // per-lane terms of the source coordinates (constant down the column):
  //   srcX = (scx + (u - tcx) cos) + (v - tcy) sin
  //   srcY = (scy + (v - tcy) cos) - (u - tcx) sin
  const int32_t uA = xA - a.mx0, uB = xB - a.mx0;
  const float cuA = uA - tcx, cuB = uB - tcx;
  const float axA = scx + cuA * a.cosval, bsA = cuA * a.sinval;
  const float axB = scx + cuB * a.cosval, bsB = cuB * a.sinval;
  const bool colA = hasA & (uA >= 0) & (uA < sw), colB = hasB & (uB >= 0) & (uB < sw);
  typedef __attribute__((address_space(3))) float lds_f32;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_f32*)winf;  // LDS byte address of winf
  const Src<F_GRAY8> S{sbase, P.pitch, P.W, P.H};
  // Source coordinates are monotone along a row, so the tap rows of all 128
  // columns of a tile row lie between those of its end columns (computed
  // with the same expressions, wave-uniform).  When every tap there is white
  // (255) the bicubic result is exactly 255: all differences are zero, so
  // each cubic_scale returns b + (+-0) = b.
  const float cuL = (tx0 - a.mx0) - tcx, cuR = (tx0 + kRFW - 1 - a.mx0) - tcx;
  const float bsL = cuL * a.sinval, bsR = cuR * a.sinval;
  constexpr int kRows = kRFH / kRFWaves;            // rows per wave
  // image row of the wave's k-th row (k < kRows), increasing in k; obuf row k
  auto wrow = [&](int k) -> int32_t { return ty0 + rot_wave_row(wu, k); };
  // Outside the mask a pixel is copied unchanged (deskew.c:268-286).  Those
  // source bytes are read into the wave's output buffer first: on gfx9 a
  // wait for a load also waits for every earlier store, so no global load
  // may follow the first store.  Tiles wholly inside the mask skip this.
  // The wave's output rows move through obuf with one mapping for loads and
  // stores: lane -> the wave's row k0 + lane/16 (image row wrow of it), bytes
  // 8*(lane%16), k0 = 0, 4: four 128-byte row segments an instruction.
  const int cb = 8 * (lane & 15);
  const int32_t xo = tx0 + cb;
  const bool partial = T.flags & ROT_T_PARTIAL;
  if (partial) {
    constexpr int kQ = (kRows + 3) / 4;
    uint64_t q[kQ];
#pragma unroll
    for (int h = 0; h < kQ; h++) {
      q[h] = 0;
      const int rr = 4 * h + (lane >> 4);
      const int32_t y = imin(wrow(rr), P.H - 1);
      const int32_t x = imin(xo, (int32_t)P.pitch - 8);  // rows are 256-byte pitched
      if (rr < kRows) q[h] = gload<uint64_t>(sbase + row_off(y, P.pitch) + x);
    }
#pragma unroll
    for (int h = 0; h < kQ; h++) {
      const int rr = 4 * h + (lane >> 4);
      if (rr < kRows) *reinterpret_cast<uint64_t*>(obuf + rr * kRFW + cb) = q[h];
    }
  }
  // White flags of the wave's rows, computed lane-parallel up front: lane
  // 16 q + j tests window row r0 + j (+16, ...) of output row 4 h + q against
  // the row's dword columns; one ballot per four rows (instead of scalar
  // bounds and a ballot per row).
  uint32_t white_rows = 0;  // bit k: every tap of output row k is white
  if (staged) {
    // one pass: lane 8 k + j tests output row k against window rows
    // r0 + j, r0 + j + 8, ... of the row's tap band, over the whole window
    // width (a row's taps span all but the ~(kRFH sin) columns of the
    // window's slant, so a column restriction would rarely change a flag)
#pragma unroll
    for (int g = 0; g < kRows; g += 8) {
      const int k = g + (lane >> 3), j = lane & 7;
      bool hit = false;
      if (k < kRows) {
        const float cv = (wrow(k) - a.my0) - tcy;
        const float VC = scy + cv * a.cosval;
        const int32_t yl = (int)(VC - bsL), yr = (int)(VC - bsR);
        const int32_t r0 = imax(imin(yl, yr) - 1 - by0, 0);
        const int32_t r1 = imin(imax(yl, yr) + 2 - by0, bh - 1);
        for (int r = r0 + j; r <= r1; r += 8) hit |= nw[r] != 0;
      }
      const uint64_t m = __ballot(hit);
#pragma unroll
      for (int q = 0; q < 8 && g + q < kRows; q++)
        if (((m >> (8 * q)) & 0xFFull) == 0) white_rows |= 1u << (g + q);
    }
    if (UPH_DIAG_BITS(diag, 2048)) white_rows = 0;
    if (UPH_DIAG_BITS(diag, 512)) white_rows = ~0u;
  }
  // Every source coordinate of the tile's in-mask pixels is >= 1 when the
  // window starts inside the image: then (int)c == floor(c) and
  // c - (int)c == fract(c) exactly (one instruction instead of three).
  const bool posc = T.flags & ROT_T_POSC;
  // LDS byte address of window (row 0, column 0) minus the 4x4 tap offset,
  // so a pixel's first tap sits at wbase + 4 (iy kRFS + ix)
  const uint32_t wbase = lds0 - 4u * (uint32_t)((1 + by0) * kRFS + 1 + xa);
  UPH_ROT_T(3)
#ifdef UPHIP_DIAG
  const unsigned long long twave = wall_clock64();
#endif
  // Full tiles (every pixel inside the mask and the image, the window staged
  // and starting inside the image) take a copy of the row loop without the
  // per-pixel mask tests and their exec-mask branches.
  uint32_t fsA = 0, fsB = 0;  // full tiles: this wave's column sums
  auto row_loop = [&](auto full_tag) {
  constexpr bool FULL = decltype(full_tag)::value;
#pragma unroll
  for (int k = 0; k < kRows; k++) {
    const int32_t y = wrow(k);
    const int32_t v = y - a.my0;
    const bool rowin = FULL || ((v >= 0) & (v < sh) & (y < P.H));
    const float cv = v - tcy;
    const float VS = cv * a.sinval, VC = scy + cv * a.cosval;
    const bool inA = FULL || (rowin & colA), inB = FULL || (rowin & colB);
    uint32_t oA = 255, oB = 255;
    const bool white = (FULL || staged) && ((white_rows >> k) & 1u);
    if (!white && (FULL || staged)) {
      const float sxA = axA + VS, syA = VC - bsA, sxB = axB + VS, syB = VC - bsB;
      const int ixA = (int)sxA, iyA = (int)syA, ixB = (int)sxB, iyB = (int)syB;  // truncation
      float fxA, fyA, fxB, fyB;
      if (FULL || posc) {
        fxA = __builtin_amdgcn_fractf(sxA);
        fyA = __builtin_amdgcn_fractf(syA);
        fxB = __builtin_amdgcn_fractf(sxB);
        fyB = __builtin_amdgcn_fractf(syB);
      } else {
        fxA = sxA - ixA, fyA = syA - iyA, fxB = sxB - ixB, fyB = syB - iyB;
      }
      // window address as one full-rate 24-bit multiply-add; pixels outside
      // the mask read (and discard) the window origin
      const uint32_t pA = inA ? wbase + 4u * (uint32_t)(__mul24(iyA, kRFS) + ixA) : lds0;
      const uint32_t pB = inB ? wbase + 4u * (uint32_t)(__mul24(iyB, kRFS) + ixB) : lds0;
      const uint32_t ta[4] = {pA, pA + 8 * kRFS, pB, pB + 8 * kRFS};
      f2 t[4][4];
      lds_taps16(ta, t);
      // rows (0,1) and (2,3) of A once its eight tap pairs are in, then of B,
      // each pair's arithmetic under the later pairs' reads.  (A pixel's two
      // row pairs interleaved after one wait: 0.99 vs 0.975 ms a launch; a
      // shortcut for wave rows of uniform 4x4 windows was slower too: DESIGN §5.)
      const f2 FA = splat2(fxA), HA = splat2(0.5f * fxA);
      const f2 FB = splat2(fxB), HB = splat2(0.5f * fxB);
      f2 c[4];  // unclamped row results; clamped straight into the column pairs
      lds_wait_pair<12>(t[0]);
      c[0] = cubic2_row_u(FA, HA, t[0]);
      lds_wait_pair_after<8>(t[1], c[0]);
      c[1] = cubic2_row_u(FA, HA, t[1]);
      lds_wait_pair_after<4>(t[2], c[1]);
      c[2] = cubic2_row_u(FB, HB, t[2]);
      lds_wait_pair_after<0>(t[3], c[2]);
      c[3] = cubic2_row_u(FB, HB, t[3]);
      // the column cubic of A and B as one pair
      const f2 o = cubic2(f2{fyA, fyB}, f2{0.5f * fyA, 0.5f * fyB},
                          f2{clamp_t255(c[0].x), clamp_t255(c[2].x)},
                          f2{clamp_t255(c[0].y), clamp_t255(c[2].y)},
                          f2{clamp_t255(c[1].x), clamp_t255(c[3].x)},
                          f2{clamp_t255(c[1].y), clamp_t255(c[3].y)});
      oA = (uint32_t)o.x;  // integer-valued in [0, 255]
      oB = (uint32_t)o.y;
    }
#ifdef UPHIP_DIAG
    if (UPH_DIAG_BITS(diag, 131072)) {  // tuning: +32 SALU a row (is the scalar unit a limit?)
      int32_t z = k;
      asm volatile(
          "s_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 1\n\t"
          "s_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 1\n\t"
          "s_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 1\n\t"
          "s_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 1\n\t"
          "s_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 1\n\t"
          "s_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 1\n\t"
          "s_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 1\n\t"
          "s_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 1\n\ts_add_u32 %0, %0, 1"
          : "+s"(z));
      if (z == -1) oA = 0;
    }
#endif
    if (!FULL && !staged) break;  // uniform: the rows go through the loop below
    if (FULL) {  // every pixel in the mask: no per-lane branches
      obuf[k * kRFW + lane] = (uint8_t)oA;
      obuf[k * kRFW + 64 + lane] = (uint8_t)oB;
      fsA += oA;  // the column sums from registers (no re-read of obuf)
      fsB += oB;
    } else {
      if (inA) obuf[k * kRFW + lane] = (uint8_t)oA;
      if (inB) obuf[k * kRFW + 64 + lane] = (uint8_t)oB;
    }
  }
  };
  const bool full = (T.flags & ROT_T_FULL) && staged;
  if (full)
    row_loop(std::true_type{});
  else
    row_loop(std::false_type{});
  if (!staged) {
    // window too large for LDS (large angles): taps from the frame (kept out
    // of the unrolled loop above)
#pragma unroll 1
    for (int k = 0; k < kRows; k++) {
      const int32_t y = wrow(k);
      const int32_t v = y - a.my0;
      const bool rowin = (v >= 0) & (v < sh) & (y < P.H);
      const float cv = v - tcy;
      const float VS = cv * a.sinval, VC = scy + cv * a.cosval;
      if (rowin & colA) obuf[k * kRFW + lane] = interp_bicubic(S, axA + VS, VC - bsA).r;
      if (rowin & colB) obuf[k * kRFW + 64 + lane] = interp_bicubic(S, axB + VS, VC - bsB).r;
    }
  }
#ifdef UPHIP_DIAG
  if (UPH_DIAG_BITS(diag, 524288) && lane == 0 && ti < kRotWaveSlots) {
    const unsigned int dt = (unsigned int)(wall_clock64() - twave);
    atomicAdd(&g_rot_wsum[ti], dt);
    atomicMax(&g_rot_wmax[ti], dt);
  }
#endif
  UPH_ROT_T(4)
  // the wave's rows as 8-byte stores: lane -> row k0 + lane/16, bytes
  // 8*(lane%16).  One wave's LDS operations complete in order, so its reads
  // see its writes without a fence.
  __builtin_amdgcn_wave_barrier();
  if (full && !UPH_DIAG_BITS(diag, 8192)) {
    // inside the image: no bounds tests
#pragma unroll
    for (int k0 = 0; k0 < kRows; k0 += 4) {
      const int rr = k0 + (lane >> 4);
      if (rr < kRows) {
        const uint64_t q = *reinterpret_cast<const uint64_t*>(obuf + rr * kRFW + cb);
        gstore<uint64_t>(dbase + row_off(wrow(rr), P.pitch) + xo, q);
      }
    }
  } else
  for (int k0 = 0; k0 < kRows && !UPH_DIAG_BITS(diag, 8192); k0 += 4) {
    const int rr = k0 + (lane >> 4);
    const int32_t y = wrow(rr), x = xo;
    if (rr < kRows && y < P.H && x < P.W) {
      const uint64_t q = *reinterpret_cast<const uint64_t*>(obuf + rr * kRFW + cb);
      uint8_t* d = dbase + row_off(y, P.pitch) + x;
      if (x + 8 <= P.W) {
        gstore<uint64_t>(d, q);
      } else {
        for (int j = 0; x + j < P.W; j++) gstore<uint8_t>(d + j, (uint8_t)(q >> (8 * j)));
      }
    }
  }
  UPH_ROT_T(5)
  if (colsum) {
    // this wave's rows of columns lane and 64 + lane, then the tile's
    uint32_t sA = fsA, sB = fsB;
    if (!full) {
#pragma unroll
      for (int k = 0; k < kRows; k++) {
        if (wrow(k) >= P.H) break;  // and so is every later row: wrow increases with k
        sA += obuf[k * kRFW + lane];
        sB += obuf[k * kRFW + 64 + lane];
      }
    }
    atomicAdd(&csum_s[lane], sA);
    atomicAdd(&csum_s[64 + lane], sB);
    csum_flush();
  }
  UPH_ROT_T(6)
#ifdef UPHIP_DIAG
  if (UPH_DIAG_BITS(diag, 65536) && threadIdx.x == 0)
    atomicAdd(&g_rot_phase[8 * (blockIdx.x & 1023) + 7], 1ull);
#endif
  };
  if constexpr (!LOOP) {  // one tile per block, XCD-aware order
    int txi, tyi, s, ti;
    xcd_block_m(m_gxy, m_gx, &txi, &tyi, &s, &ti);
    tile(txi, tyi, s, ti);
  } else {
  // Persistent form for the large-window class, usually empty: then the
  // launch's count of large-window sheets is 0 and every block ends after
  // that one load.  Otherwise the lanes of every wave test 64 sheets at once
  // (the same ballot in every wave), and the block walks the tiles of the
  // sheets that belong here.
  if (*nlarge == 0) return;
  for (int s0 = 0; s0 < loop_count; s0 += 64) {
    const int l = threadIdx.x & 63;
    bool want = false;
    if (s0 + l < loop_count) want = sheets[s0 + l].active && sheets[s0 + l].large;
    uint64_t m = __ballot(want);
    m = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(m >> 32)) << 32) |
        __builtin_amdgcn_readfirstlane((uint32_t)m);
    while (m) {
      const int s = s0 + __ffsll((long long)m) - 1;
      m &= m - 1;
      for (int t = blockIdx.x; t < tgx * tgy; t += gridDim.x) {
        tile(t % tgx, t / tgx, s, s * (tgx * tgy) + t);
        __syncthreads();  // the next tile restages the LDS window
      }
    }
  }
  }
}

// Rows of source window a kRFW x kRFH tile needs at rotations up to |angle|.
static int rotate_window_rows(float max_abs_angle) {
  const float a = fminf(fabsf(max_abs_angle), 1.5707964f);
  // (kRFH-1) cos + (kRFW-1) sin rows of pixel centres, + 3 tap rows, + 2 for
  // the floor/truncation slack of the window bounds
  return kRFH + (int)ceilf((kRFW - 1) * sinf(a)) + 5;
}

// k_rot_tiles' records of one launch: the count of large-window sheets (its
// own 64 bytes), the RotSheet of every sheet, then every sheet's RotTile.
static size_t rot_tiles_per_sheet(int32_t W, int32_t H) {
  return (size_t)((W + kRFW - 1) / kRFW) * (size_t)((H + kRFH - 1) / kRFH);
}
size_t rotate_scratch_bytes(int32_t W, int32_t H, int count) {
  return 64 + (sizeof(RotSheet) + sizeof(RotTile) * rot_tiles_per_sheet(W, H)) * (size_t)count;
}
static_assert(sizeof(RotSheet) == 64 && sizeof(RotTile) == 16, "records are read as whole dwords");

bool launch_rotate_mask(const PlaneRef& src, const PlaneRef& dst, const RotateArgs* args,
                        int interp, int count, hipStream_t st, float max_abs_angle,
                        void* scratch, uint32_t* colsum, int64_t cs_stride) {
  const dim3 grid((src.P.W + kRotTW - 1) / kRotTW, (src.P.H + kRotTH - 1) / kRotTH, count);
  const dim3 ggrid((src.P.W + kRotTW - 1) / kRotTW, (src.P.H + kRotGH - 1) / kRotGH, count);
  if (interp == UPHIP_INTERP_CUBIC && src.P.fmt == F_GRAY8) {
    if (diag_double() & 4096) colsum = nullptr;  // tuning build: time without the column sums
    const int rows = rotate_window_rows(max_abs_angle);
    auto lds_of = [](int r) {
      return (sizeof(float) * kRFS + sizeof(uint64_t)) * (size_t)r + kRFH * kRFW;
    };
    // the most window rows that still let four tiles (32 waves) share a CU's
    // 160 KB of LDS (512 B of static LDS per tile; the 16 B more that the
    // bound still allows were the window bounds'); windows of up to ~2.25 deg
    const int rows4 = (int)((40 * 1024 - 16 - 4 * kRFW - kRFH * kRFW) /
                            (sizeof(float) * kRFS + sizeof(uint64_t)));
    if (lds_of(rows) <= 56 * 1024 &&
        src.P.pitch * (int64_t)src.P.H < (1ll << 31) && !(diag_double() & 256)) {
      const dim3 fgrid((src.P.W + kRFW - 1) / kRFW, (src.P.H + kRFH - 1) / kRFH, count);
      const uint32_t mgxy = div_magic(fgrid.x * fgrid.y), mgx = div_magic(fgrid.x);
      const int dd = diag_double() & (512 | 1024 | 2048 | 8192 | 65536 | 131072 | 524288);
#ifdef UPHIP_DIAG
      struct PhasePrint {  // after the launches below: the per-tile phase clocks
        hipStream_t st;
        ~PhasePrint() {
          if (diag_double() & 524288) {  // every wave's row loop: the tile's mean wave and its slowest
            static unsigned int ws[kRotWaveSlots], wm[kRotWaveSlots], wz[kRotWaveSlots];
            hipStreamSynchronize(st);
            hipMemcpyFromSymbol(ws, HIP_SYMBOL(g_rot_wsum), sizeof(ws));
            hipMemcpyFromSymbol(wm, HIP_SYMBOL(g_rot_wmax), sizeof(wm));
            hipMemcpyToSymbol(HIP_SYMBOL(g_rot_wsum), wz, sizeof(wz));
            hipMemcpyToSymbol(HIP_SYMBOL(g_rot_wmax), wz, sizeof(wz));
            unsigned long long n = 0, sum = 0, mx = 0;
            for (int i = 0; i < kRotWaveSlots; i++)
              if (wm[i]) n++, sum += ws[i], mx += wm[i];
            if (n)
              fprintf(stderr, "rotate row loop (10 ns ticks/tile, %llu tiles, %d waves a tile): mean wave %.1f "
                      "slowest wave %.1f\n", n, kRFWaves, (double)sum / kRFWaves / n, (double)mx / n);
          }
          if (!(diag_double() & 65536)) return;
          static unsigned long long hh[1024 * 8], z[1024 * 8];
          unsigned long long h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
          hipStreamSynchronize(st);
          hipMemcpyFromSymbol(hh, HIP_SYMBOL(g_rot_phase), sizeof(hh));
          hipMemcpyToSymbol(HIP_SYMBOL(g_rot_phase), z, sizeof(z));
          for (int i = 0; i < 1024 * 8; i++) h[i & 7] += hh[i];
          if (!h[7]) return;
          fprintf(stderr, "rotate phases (10 ns ticks/tile, %llu tiles): index %.0f records %.0f staging %.0f "
                  "flags %.0f compute %.0f stores %.0f colsum %.0f\n", h[7], (double)h[0] / h[7],
                  (double)h[1] / h[7], (double)h[2] / h[7], (double)h[3] / h[7],
                  (double)h[4] / h[7], (double)h[5] / h[7], (double)h[6] / h[7]);
        }
      } phase_print{st};
#endif
      // the records of this launch (k_rot_tiles), then the tiles that read them
      uint32_t* nlarge = static_cast<uint32_t*>(scratch);
      RotSheet* sheets = reinterpret_cast<RotSheet*>(static_cast<uint8_t*>(scratch) + 64);
      RotTile* tiles = reinterpret_cast<RotTile*>(sheets + count);
      const RotPlane rp{src.P.W, src.P.H, (uint32_t)src.P.pitch};
      const int tgx = (int)fgrid.x, tgy = (int)fgrid.y;
      const bool split = rows > rows4;
      hipLaunchKernelGGL(k_rot_tiles, dim3((tgx * tgy + 255) / 256, count), dim3(256), 0, st, src,
                         dst, args, count, tgx, tgy, split ? rows4 : rows, rows, split ? rows4 : 0,
                         sheets, tiles, nlarge);
      if (split) {
        // sheets whose angle fits the small window at four tiles per CU, then
        // the others at the scan range's window (three per CU); every sheet
        // is taken by exactly one of the two launches
        // (the second as a persistent grid: when no sheet needs the large
        // window its blocks only read the launch's count of such sheets)
        UPH_LAUNCH_DIAG(2, k_rotate_cubic_g8f<false>, fgrid, dim3(kRFT), lds_of(rows4), st, sheets,
                        tiles, nlarge, rp, rows4, dd, mgxy, mgx, 0, 0, 0, colsum, cs_stride);
        UPH_LAUNCH_DIAG(2, k_rotate_cubic_g8f<true>, dim3(3 * 256), dim3(kRFT), lds_of(rows), st,
                        sheets, tiles, nlarge, rp, rows, dd, 0u, 0u, count, tgx, tgy, colsum,
                        cs_stride);
      } else {
        UPH_LAUNCH_DIAG(2, k_rotate_cubic_g8f<false>, fgrid, dim3(kRFT), lds_of(rows), st, sheets,
                        tiles, nlarge, rp, rows, dd, mgxy, mgx, 0, 0, 0, colsum, cs_stride);
      }
      return colsum != nullptr;
    }
    const dim3 qgrid((src.P.W + kRQW - 1) / kRQW, (src.P.H + kRQH - 1) / kRQH, count);
    UPH_LAUNCH_DIAG(2, k_rotate_cubic_g8, qgrid, dim3(kThreads), 0, st, src, dst, args);
    return false;
  }
  if (interp == UPHIP_INTERP_CUBIC && src.P.fmt == F_Y400A) {
    hipLaunchKernelGGL(k_rotate_cubic_gray<F_Y400A>, ggrid, dim3(kThreads), 0, st, src, dst, args);
    return false;
  }
  if (src.P.fmt == F_GRAY8)
    hipLaunchKernelGGL(k_rotate_mask<F_GRAY8>, grid, dim3(kThreads), 0, st, src, dst, args,
                       interp);
  else if (src.P.fmt == F_Y400A)
    hipLaunchKernelGGL(k_rotate_mask<F_Y400A>, grid, dim3(kThreads), 0, st, src, dst, args,
                       interp);
  else
    hipLaunchKernelGGL(k_rotate_mask<F_RGB24>, grid, dim3(kThreads), 0, st, src, dst, args,
                       interp);
  return false;
}

}  // namespace uph
