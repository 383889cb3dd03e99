// kernels_move.hip — center_mask / align_mask (imageprocess/masks.c) as
// out-of-place gathers for gfx950: the generic move, the gray move with its
// folded mask and row counts, and the chained centring + align move.
// Destination-driven like kernels_blit.hip: every output byte is produced by
// exactly one thread.
#include <climits>

#include "blit_common.h"
#include "kernels.h"

namespace uph {

// ---------------------------------------------------------------------------
// center_mask / align_mask as a single out-of-place gather (masks.c:222-300):
//   newimage = bg-filled |area|; copy clip(area) -> newimage at (0,0);
//   wipe clip(area) with bg; copy newimage -> image at (tx,ty).
// ---------------------------------------------------------------------------
template <int FMT>
__global__ void __launch_bounds__(kThreads) k_move_rect(PlaneRef src, PlaneRef dst,
                                                        const MoveArgs* args) {
  const int s = blockIdx.z;
  const MoveArgs a = args[s];
  if (!a.active) return;
  const Planes& P = src.P;
  const uint8_t* sbase = plane_ptr(src, s);
  uint8_t* dbase = plane_ptr(dst, s);
  const Rect A = clip(a.area, P.W, P.H);
  const int32_t aw = A.x1 - A.x0 + 1, ah = A.y1 - A.y0 + 1;  // copied extent (may be <= 0)
  const int32_t sw = iabs(a.area.x0 - a.area.x1) + 1, sh = iabs(a.area.y0 - a.area.y1) + 1;
  const Px bg{a.bg[0], a.bg[1], a.bg[2]};
  // the paste back (copy_rectangle newimage -> image) is a raw memcpy only when
  // the whole target rectangle is inside the image (blit.c:38-69); otherwise
  // set_pixel per pixel, which rewrites Y400A alpha as 0xFF
  const bool raw_paste = a.tx >= 0 && a.ty >= 0 && a.tx + sw <= P.W && a.ty + sh <= P.H;
  for (int32_t y = blockIdx.x; y < P.H; y += gridDim.x) {
    const uint8_t* srow = sbase + (int64_t)y * P.pitch;
    uint8_t* drow = dbase + (int64_t)y * P.pitch;
    const int32_t v = y - a.ty;
    for (int32_t x = threadIdx.x; x < P.W; x += blockDim.x) {
      const int32_t u = x - a.tx;
      Px o;
      if (u >= 0 && u < sw && v >= 0 && v < sh) {
        if (u < aw && v < ah) {
          const uint8_t* srow_m = sbase + (int64_t)(A.y0 + v) * P.pitch;
          if (raw_paste) {
            copy_px_raw<FMT>(drow, x, srow_m, A.x0 + u);
            continue;
          }
          o = load_px_row<FMT>(srow_m, A.x0 + u);
        } else {
          o = bg;
        }
      } else if (x >= A.x0 && x <= A.x1 && y >= A.y0 && y <= A.y1) {
        o = bg;
      } else {
        copy_px_raw<FMT>(drow, x, srow, x);
        continue;
      }
      store_px_row<FMT>(drow, x, o);
    }
  }
}

// k_move_rect for RGB24 planes, a destination dword per lane.  A moved
// pixel's bytes come from the same row offset 3 (A.x0 - tx) away, so a dword
// whose bytes all share one class (unchanged / background / moved) is one
// aligned load, a constant pattern, or two aligned loads realigned by that
// offset; dwords across a class change, and the row's tail, go byte by byte.
// RGB24 has no alpha: set_pixel and the raw paste write the same bytes.
__global__ void __launch_bounds__(kThreads) k_move_rect_rgb(PlaneRef src, PlaneRef dst,
                                                            const MoveArgs* args) {
  const int s = blockIdx.z;
  const MoveArgs a = args[s];
  if (!a.active) return;
  const Planes& P = src.P;
  const uint8_t* sbase = plane_ptr(src, s);
  uint8_t* dbase = plane_ptr(dst, s);
  const Rect A = clip(a.area, P.W, P.H);
  const int32_t aw = A.x1 - A.x0 + 1, ah = A.y1 - A.y0 + 1;
  const int32_t sw = iabs(a.area.x0 - a.area.x1) + 1, sh = iabs(a.area.y0 - a.area.y1) + 1;
  const int32_t rowb = 3 * P.W, ndw = (rowb + 3) >> 2;
  const int32_t shift = 3 * (A.x0 - a.tx);  // source byte - destination byte, moved pixels
  // the background as bytes of a dword starting at a byte of phase 0, 1, 2
  uint32_t bgw[3];
#pragma unroll
  for (int ph = 0; ph < 3; ph++) {
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) w |= (uint32_t)a.bg[(ph + k) % 3] << (8 * k);
    bgw[ph] = w;
  }
  for (int32_t y = blockIdx.x; y < P.H; y += gridDim.x) {
    const uint8_t* srow = sbase + (int64_t)y * P.pitch;
    uint8_t* drow = dbase + (int64_t)y * P.pitch;
    const int32_t v = y - a.ty;
    const bool vin = v >= 0 && v < sh, vsrc = vin && v < ah;
    const bool wrow = y >= A.y0 && y <= A.y1;
    const uint8_t* srow_m = sbase + (int64_t)(A.y0 + (vsrc ? v : 0)) * P.pitch;
    // 0 unchanged, 1 background, 2 moved
    auto cls = [&](int32_t x) {
      const int32_t u = x - a.tx;
      if (vin && u >= 0 && u < sw) return vsrc && u < aw ? 2 : 1;
      return wrow && x >= A.x0 && x <= A.x1 ? 1 : 0;
    };
    for (int32_t d = threadIdx.x; d < ndw; d += blockDim.x) {
      const int32_t xb = 4 * d;
      const int c0 = cls(xb / 3), c1 = cls(imin(xb + 3, rowb - 1) / 3);
      if (c0 == c1 && xb + 4 <= rowb) {
        uint32_t out;
        if (c0 == 0) {
          out = *reinterpret_cast<const uint32_t*>(srow + xb);
        } else if (c0 == 1) {
          out = bgw[xb % 3];
        } else {
          const int32_t sb = xb + shift, sa = sb & ~3, r = sb & 3;
          const uint32_t w0 = *reinterpret_cast<const uint32_t*>(srow_m + sa);
          out = r ? __builtin_amdgcn_alignbyte(*reinterpret_cast<const uint32_t*>(srow_m + sa + 4), w0, r)
                  : w0;
        }
        *reinterpret_cast<uint32_t*>(drow + xb) = out;
      } else {
        for (int k = 0; k < 4 && xb + k < rowb; k++) {
          const int32_t b = xb + k, x = b / 3, c = cls(x);
          drow[b] = c == 0 ? srow[b] : c == 1 ? a.bg[b % 3] : srow_m[b + shift];
        }
      }
    }
  }
}

// k_move_rect for gray planes, 16 bytes of the destination per lane.  The
// class of a column (unchanged / background / moved) only changes at five
// breakpoints, so a vector not straddling one is one aligned 16-byte load, a
// constant, or two aligned loads realigned by the source shift, which is the
// same for every vector of the sheet ((A.x0 - tx) mod 16).  Vectors across a
// breakpoint or the right image edge go byte by byte.
template <int Q>
__device__ __forceinline__ uint4 shift_bytes16(const uint32_t* w, int r) {
  return make_uint4(__builtin_amdgcn_alignbyte(w[Q + 1], w[Q], r),
                    __builtin_amdgcn_alignbyte(w[Q + 2], w[Q + 1], r),
                    __builtin_amdgcn_alignbyte(w[Q + 3], w[Q + 2], r),
                    __builtin_amdgcn_alignbyte(w[Q + 4], w[Q + 3], r));
}

constexpr int kMoveRows = 8;  // rows per wave of k_move_rect_g16
constexpr int kMoveBp = 7;    // column breakpoints: five of the move, two of a folded mask
constexpr int kMoveBlockRows = kMoveRows * (kThreads / 64);
static_assert((kMoveBp + 1) * kMoveBlockRows <= kThreads, "one lane per deferred (row, vector)");

// bytes <= thr among four (kadd = (256 - (thr + 1)) * 0x00010001), keeping
// the bytes whose bit is set in `keep4` (bits 0..3 = bytes 0..3)
__device__ __forceinline__ uint32_t dark4(uint32_t x, uint32_t kadd, uint32_t keep4) {
  const uint32_t lo = ((x & 0x00FF00FFu) + kadd) & 0x01000100u;  // bytes 0, 2 > thr: bits 8, 24
  const uint32_t hi = (((x >> 8) & 0x00FF00FFu) + kadd) & 0x01000100u;  // bytes 1, 3
  const uint32_t kb = ((keep4 & 1u) << 8) | ((keep4 & 2u) << 8) | ((keep4 & 4u) << 22) |
                      ((keep4 & 8u) << 22);  // keep bits at 8, 9, 24, 25
  return __popc(kb) - __popc((lo | (hi << 1)) & kb);
}
// dark bytes of a 16-byte vector, bytes selected by a 16-bit mask
__device__ __forceinline__ uint32_t dark16(const uint4& v, uint32_t m16, uint32_t kadd) {
  return dark4(v.x, kadd, m16 & 15u) + dark4(v.y, kadd, (m16 >> 4) & 15u) +
         dark4(v.z, kadd, (m16 >> 8) & 15u) + dark4(v.w, kadd, m16 >> 12);
}
// 16-bit mask of the columns x0 .. x0+15 inside [c0, c1]
__device__ __forceinline__ uint32_t cols16(int32_t x0, int32_t c0, int32_t c1) {
  const int32_t lo = imax(c0 - x0, 0), hi = imin(c1 - x0, 15);
  return lo > hi ? 0u : ((2u << hi) - 1u) & ~((1u << lo) - 1u);
}
// byte mask of the four bits b (bit j -> byte j)
__device__ __forceinline__ uint32_t bytes_of4(uint32_t b) {
  return ((b * 0x00204081u) & 0x01010101u) * 0xFFu;
}

template <int MODE>
__global__ void __launch_bounds__(kThreads) k_move_rect_g16(PlaneRef src, PlaneRef dst,
                                                            const MoveArgs* args, MoveExtra X) {
  constexpr bool kMask = (MODE & 1) != 0, kRows = (MODE & 2) != 0;
  constexpr bool kDry = (MODE & 4) != 0;  // count only: nothing is written
  static_assert(!(kDry && kMask), "a dry pass counts; it does not mask");
  const int s = blockIdx.z;
  if (X.only && !X.only[s]) return;
  const MoveArgs a = args[s];
  if (!kMask && !kRows && !a.active) return;
  const Planes& P = src.P;
  const uint8_t* sbase = plane_ptr(src, s);
  uint8_t* dbase = plane_ptr(dst, s);
  const int lane = threadIdx.x & 63;
  const int32_t nv = (P.W + 15) >> 4;                  // vectors per row (inside the pitch)
  // the block's rows: blocks cover the row ranges [ya0, ya1) then [yb0, yb1)
  // (all rows by default), kMoveBlockRows each
  const bool ranged = X.ya1 > X.ya0 || X.yb1 > X.yb0;
  const int32_t ra0 = ranged ? X.ya0 : 0, ra1 = ranged ? X.ya1 : P.H;
  const int32_t nba = ra1 > ra0 ? (ra1 - ra0 + kMoveBlockRows - 1) / kMoveBlockRows : 0;
  const bool second = (int32_t)blockIdx.x >= nba;
  const int32_t yb = second ? X.yb0 + ((int32_t)blockIdx.x - nba) * kMoveBlockRows
                            : ra0 + (int32_t)blockIdx.x * kMoveBlockRows;  // the block's first row
  const int32_t yend = imin(second ? X.yb1 : ra1, P.H);  // first row past the block's range
  const int32_t y0 = yb + (threadIdx.x >> 6) * kMoveRows;
  const int32_t y1 = imin(y0 + kMoveRows, yend);
  // folded apply_masks (one mask, masks.c:306-322 semantics: normalized,
  // pixels outside it <- colour)
  Rect mk{INT_MIN / 2, INT_MIN / 2, INT_MAX / 2, INT_MAX / 2};
  uint8_t mcol = 0;
  if (kMask) {
    const MaskArgs* ma = X.masks + s;
    if (ma->n > 0) mk = normalize(ma->m[0]);
    mcol = gray_of(Px{ma->color[0], ma->color[1], ma->color[2]});
  }
  const uint32_t mcol4 = mcol * 0x01010101u;
  const uint32_t kadd = (256u - ((uint32_t)X.thr + 1u)) * 0x00010001u;
  __shared__ uint32_t rowcnt[kMoveBlockRows];
  if (kRows) {
    if (threadIdx.x < kMoveBlockRows) rowcnt[threadIdx.x] = 0;
    __syncthreads();
  }
  uint32_t acc[kMoveRows];
#pragma unroll
  for (int k = 0; k < kMoveRows; k++) acc[k] = 0;
  auto finish_rows = [&]() {
    if (!kRows) return;
#pragma unroll
    for (int k = 0; k < kMoveRows; k++) {
      uint32_t v = acc[k];
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (lane == 0 && v) atomicAdd(&rowcnt[y0 - yb + k], v);
    }
    __syncthreads();
    const int32_t y = yb + (int32_t)threadIdx.x;
    if (threadIdx.x < kMoveBlockRows && y < yend) X.rows[(int64_t)s * X.rows_stride + y] = rowcnt[threadIdx.x];
  };
  if (!a.active) {
    // the identity move: mask the current plane in place and/or count it
    for (int32_t vi = lane; vi < nv; vi += 64) {
      const int32_t x0 = 16 * vi;
      const uint32_t valid = cols16(x0, 0, P.W - 1);
      const uint32_t incol = cols16(x0, mk.x0, mk.x1) & valid;
      const uint32_t reg = kRows ? cols16(x0, X.rx0, X.rx1) : 0u;
#pragma unroll
      for (int k = 0; k < kMoveRows; k++) {
        const int32_t y = y0 + k;
        if (y >= y1) break;
        uint8_t* row = const_cast<uint8_t*>(sbase) + (int64_t)y * P.pitch;
        const uint32_t out16 = kMask ? valid & ~((y >= mk.y0 && y <= mk.y1) ? incol : 0u) : 0u;
        uint4 v = make_uint4(mcol4, mcol4, mcol4, mcol4);
        if ((kRows && reg) || out16 != valid || valid != 0xFFFFu)
          v = *reinterpret_cast<const uint4*>(row + x0);
        if (out16) {
          v.x = (v.x & ~bytes_of4(out16 & 15u)) | (mcol4 & bytes_of4(out16 & 15u));
          v.y = (v.y & ~bytes_of4((out16 >> 4) & 15u)) | (mcol4 & bytes_of4((out16 >> 4) & 15u));
          v.z = (v.z & ~bytes_of4((out16 >> 8) & 15u)) | (mcol4 & bytes_of4((out16 >> 8) & 15u));
          v.w = (v.w & ~bytes_of4(out16 >> 12)) | (mcol4 & bytes_of4(out16 >> 12));
          *reinterpret_cast<uint4*>(row + x0) = v;
        }
        if (kRows && reg) acc[k] += dark16(v, reg, kadd);
      }
    }
    finish_rows();
    return;
  }
  const Rect A = clip(a.area, P.W, P.H);
  const int32_t aw = A.x1 - A.x0 + 1, ah = A.y1 - A.y0 + 1;
  const int32_t sw = iabs(a.area.x0 - a.area.x1) + 1, sh = iabs(a.area.y0 - a.area.y1) + 1;
  const uint8_t bg = gray_of(Px{a.bg[0], a.bg[1], a.bg[2]});
  const uint32_t bg4 = bg * 0x01010101u;
  const int32_t delta = A.x0 - a.tx;                   // source column - destination column
  const int r16 = delta & 15, q = r16 >> 2, r = r16 & 3;
  // The class of a column changes only at the breakpoints (uniform per
  // sheet): five of the move, and the mask's two when one is folded in.
  // Vectors holding a breakpoint strictly inside, and the row's last
  // partial vector, are assembled byte by byte after the row's uniform
  // vectors -- one lane each, so the wave runs that path once per row.
  const int32_t bp[kMoveBp] = {a.tx, a.tx + aw, a.tx + sw, A.x0, A.x1 + 1,
                               kMask ? mk.x0 : 0, kMask ? mk.x1 + 1 : 0};
  // Deferred vectors (uniform): those holding a breakpoint strictly inside,
  // and the row's last partial vector, deduplicated.
  int32_t dvs[kMoveBp + 1];
  int nd = 0;
#pragma unroll
  for (int k = 0; k < kMoveBp + 1; k++) {
    const int32_t b = k < kMoveBp ? bp[k] : P.W;
    const bool has = k < kMoveBp ? (b > 0 && b < P.W && (b & 15)) : (P.W & 15) != 0;
    bool dup = false;
#pragma unroll
    for (int m = 0; m < kMoveBp + 1; m++)
      if (m < nd && dvs[m] == (b >> 4)) dup = true;
    if (has && !dup) dvs[nd++] = b >> 4;
  }
  // A column's class on a row is a function of four column facts (inside
  // the pasted columns, inside its copied part, inside the wiped area, inside
  // the mask) and four row facts; per row the sixteen column codes map to
  // classes (0 source, 1 background, 2 moved, 3 mask colour) through one
  // 32-bit table, so the column work is done once.
  auto col_code = [&](int32_t x) -> uint32_t {
    const int32_t u = x - a.tx;
    return (uint32_t)(u >= 0 && u < sw) | (uint32_t)(u < aw) << 1 |
           (uint32_t)(x >= A.x0 && x <= A.x1) << 2 | (uint32_t)(x >= mk.x0 && x <= mk.x1) << 3;
  };
  auto row_table = [&](int32_t y) -> uint32_t {
    const int32_t v = y - a.ty;
    const bool trow = v >= 0 && v < sh, mrow = trow && v < ah;
    const bool arow = y >= A.y0 && y <= A.y1;
    const bool krow = y >= mk.y0 && y <= mk.y1;
    uint32_t t = 0;
#pragma unroll
    for (int c = 0; c < 16; c++) {
      int cls = (trow && (c & 1)) ? ((mrow && (c & 2)) ? 2 : 1) : ((arow && (c & 4)) ? 1 : 0);
      if (kMask && cls == 0 && !(krow && (c & 8))) cls = 3;
      t |= (uint32_t)cls << (2 * c);
    }
    return t;
  };
  auto moved_row = [&](int32_t y) -> const uint8_t* {
    const int32_t v = y - a.ty;
    return sbase + (int64_t)(A.y0 + ((v >= 0 && v < ah) ? v : 0)) * P.pitch;
  };
  // kMoveVec vectors per lane per chunk of the row (192 slots: 155 used at A4 width)
  constexpr int kMoveVec = 3;
  for (int32_t vb = 0; vb < nv; vb += 64 * kMoveVec) {
    uint32_t cc[kMoveVec];   // column code, bit 4: no uniform vector here
    uint32_t reg[kMoveVec];  // counted columns (kRows)
#pragma unroll
    for (int k = 0; k < kMoveVec; k++) {
      const int32_t vi = vb + k * 64 + lane;
      const int32_t x0 = 16 * vi;
      bool deferred = vi >= nv || x0 + 16 > P.W;
#pragma unroll
      for (int j = 0; j < kMoveBp; j++) deferred |= bp[j] > x0 && bp[j] < x0 + 16;
      cc[k] = col_code(x0) | (deferred ? 16u : 0u);
      reg[k] = kRows ? cols16(x0, X.rx0, X.rx1) : 0u;
    }
#pragma unroll
    for (int ky = 0; ky < kMoveRows; ky++) {
      const int32_t y = y0 + ky;
      if (y >= y1) break;
      const uint8_t* srow = sbase + (int64_t)y * P.pitch;
      uint8_t* drow = dbase + (int64_t)y * P.pitch;
      const uint8_t* mrow_p = moved_row(y);
      const uint32_t tab = row_table(y);
      int cls[kMoveVec];
      uint4 lo[kMoveVec], hi[kMoveVec];
#pragma unroll
      for (int k = 0; k < kMoveVec; k++) {
        const int32_t x0 = 16 * (vb + k * 64 + lane);
        cls[k] = (cc[k] & 16u) ? -1 : (int)((tab >> (2 * (cc[k] & 15u))) & 3u);
        lo[k] = cls[k] == 3 ? make_uint4(mcol4, mcol4, mcol4, mcol4) : make_uint4(bg4, bg4, bg4, bg4);
        hi[k] = make_uint4(0, 0, 0, 0);
        if (cls[k] == 0) {
          lo[k] = *reinterpret_cast<const uint4*>(srow + x0);
        } else if (cls[k] == 2) {
          // a whole class-2 vector reads source columns inside [0, W), so
          // both aligned halves lie inside the (16-multiple) pitch
          const uint4* qp = reinterpret_cast<const uint4*>(mrow_p + ((x0 + delta) & ~15));
          lo[k] = qp[0];
          if (r16) hi[k] = qp[1];
        }
      }
#pragma unroll
      for (int k = 0; k < kMoveVec; k++) {
        const int32_t x0 = 16 * (vb + k * 64 + lane);
        if (cls[k] < 0) continue;
        uint4 out = lo[k];
        if (cls[k] == 2 && r16) {
          const uint32_t w[8] = {lo[k].x, lo[k].y, lo[k].z, lo[k].w,
                                 hi[k].x, hi[k].y, hi[k].z, hi[k].w};
          switch (q) {  // uniform over the sheet
            case 0: out = shift_bytes16<0>(w, r); break;
            case 1: out = shift_bytes16<1>(w, r); break;
            case 2: out = shift_bytes16<2>(w, r); break;
            default: out = shift_bytes16<3>(w, r); break;
          }
        }
        if (!kDry) *reinterpret_cast<uint4*>(drow + x0) = out;
        if (kRows && reg[k]) acc[ky] += dark16(out, reg[k], kadd);
      }
    }
  }
  // Deferred vectors: per byte, the class picks a byte of the source vector,
  // of the moved (realigned) vector, the background or the mask colour;
  // columns >= W stay 0.  The block's (row, deferred vector) pairs are
  // spread over all its lanes, one pair each (<= 8 x kMoveBlockRows <=
  // kThreads), so the byte work runs once per block rather than once per row
  // and wave.
  const int tid = threadIdx.x;
  const int32_t yr = yb + (nd ? tid / nd : 0);
  if (tid < nd * kMoveBlockRows && yr < yend) {
    const int di = tid - (tid / nd) * nd;
    int32_t vi = dvs[0];
#pragma unroll
    for (int m = 1; m < kMoveBp + 1; m++)
      if (m == di) vi = dvs[m];
    const int32_t x0 = 16 * vi;
    const int32_t y = yr;
    const uint8_t* srow = sbase + (int64_t)y * P.pitch;
    const uint8_t* mrow_p = moved_row(y);
    const uint32_t tab = row_table(y);
    // the aligned source halves of the moved bytes, each clamped into the row
    // (a clamped half only feeds bytes whose class is not 2)
    const int32_t al = (x0 + delta) & ~15;
    const int32_t alo = imin(imax(al, 0), (int32_t)P.pitch - 16);
    const int32_t ahi = imin(imax(al + 16, 0), (int32_t)P.pitch - 16);
    const uint4 sv = *reinterpret_cast<const uint4*>(srow + x0);
    const uint4 l = *reinterpret_cast<const uint4*>(mrow_p + alo);
    const uint4 h = *reinterpret_cast<const uint4*>(mrow_p + ahi);
    const uint32_t w[8] = {l.x, l.y, l.z, l.w, h.x, h.y, h.z, h.w};
    uint4 mv;
    switch (q) {
      case 0: mv = shift_bytes16<0>(w, r); break;
      case 1: mv = shift_bytes16<1>(w, r); break;
      case 2: mv = shift_bytes16<2>(w, r); break;
      default: mv = shift_bytes16<3>(w, r); break;
    }
    const uint32_t sw4[4] = {sv.x, sv.y, sv.z, sv.w};
    const uint32_t mw4[4] = {mv.x, mv.y, mv.z, mv.w};
    uint32_t o[4];
#pragma unroll
    for (int d = 0; d < 4; d++) {
      uint32_t m0 = 0, m2 = 0, mb = 0, mc = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int32_t x = x0 + 4 * d + j;
        const uint32_t code = x < P.W ? col_code(x) : 16u;
        const uint32_t cls = (code & 16u) ? 4u : (tab >> (2 * code)) & 3u;
        const uint32_t byte = 0xFFu << (8 * j);
        m0 |= cls == 0 ? byte : 0u;
        m2 |= cls == 2 ? byte : 0u;
        mb |= cls == 1 ? byte : 0u;
        mc |= cls == 3 ? byte : 0u;
      }
      o[d] = (sw4[d] & m0) | (mw4[d] & m2) | (bg4 & mb) | (mcol4 & mc);
    }
    const uint4 ov = make_uint4(o[0], o[1], o[2], o[3]);
    if (!kDry) *reinterpret_cast<uint4*>(dbase + (int64_t)y * P.pitch + x0) = ov;
    if (kRows) {
      const uint32_t rg = cols16(x0, X.rx0, X.rx1);
      if (rg) atomicAdd(&rowcnt[y - yb], dark16(ov, rg, kadd));
    }
  }
  finish_rows();
}

void launch_move_rect(const PlaneRef& src, const PlaneRef& dst, const MoveArgs* args, int count,
                      hipStream_t st) {
  int gx = src.P.H < 1 ? 1 : (src.P.H > 1024 ? 1024 : src.P.H);
  if (src.P.fmt == F_GRAY8) {
    // kMoveRows consecutive rows per wave
    const int64_t blocks = (src.P.H + kMoveBlockRows - 1) / kMoveBlockRows;
    UPH_LAUNCH_DIAG(4, k_move_rect_g16<0>, dim3((unsigned)(blocks < 1 ? 1 : blocks), 1, count),
                    dim3(kThreads), 0, st, src, dst, args, MoveExtra{});
  } else if (src.P.fmt == F_Y400A) {
    hipLaunchKernelGGL(k_move_rect<F_Y400A>, dim3(gx, 1, count), dim3(kThreads), 0, st, src, dst,
                       args);
  } else {
    hipLaunchKernelGGL(k_move_rect_rgb, dim3(gx, 1, count), dim3(kThreads), 0, st, src, dst,
                       args);
  }
}

bool launch_move_rect_fused(const PlaneRef& src, const PlaneRef& dst, const MoveArgs* args,
                            const MoveExtra& x, int count, hipStream_t st) {
  if (src.P.fmt != F_GRAY8) return false;
  int64_t blocks = (src.P.H + kMoveBlockRows - 1) / kMoveBlockRows;
  if (x.ya1 > x.ya0 || x.yb1 > x.yb0) {  // row ranges (see k_move_rect_g16)
    if (!x.dry) return false;             // only a counting pass may skip rows
    blocks = (x.ya1 > x.ya0 ? (x.ya1 - x.ya0 + kMoveBlockRows - 1) / kMoveBlockRows : 0) +
             (x.yb1 > x.yb0 ? (x.yb1 - x.yb0 + kMoveBlockRows - 1) / kMoveBlockRows : 0);
    if (blocks == 0) return true;
  }
  const dim3 grid((unsigned)(blocks < 1 ? 1 : blocks), 1, count);
  const int mode = (x.masks ? 1 : 0) | (x.rows ? 2 : 0) | (x.dry ? 4 : 0);
  if (x.dry && x.masks) return false;
  switch (mode) {
    case 6: UPH_LAUNCH_DIAG(4, k_move_rect_g16<6>, grid, dim3(kThreads), 0, st, src, dst, args, x); break;
    case 1: UPH_LAUNCH_DIAG(4, k_move_rect_g16<1>, grid, dim3(kThreads), 0, st, src, dst, args, x); break;
    case 2: UPH_LAUNCH_DIAG(4, k_move_rect_g16<2>, grid, dim3(kThreads), 0, st, src, dst, args, x); break;
    case 3: UPH_LAUNCH_DIAG(4, k_move_rect_g16<3>, grid, dim3(kThreads), 0, st, src, dst, args, x); break;
    default: UPH_LAUNCH_DIAG(4, k_move_rect_g16<0>, grid, dim3(kThreads), 0, st, src, dst, args, x); break;
  }
  return true;
}

// ---------------------------------------------------------------------------
// center_mask, then apply_masks + align_mask (sheet_stages.c:415-499,
// masks.c:222-322) as ONE gather from the uncentred plane R, so that the
// centred plane C is never written: O(x, y) follows the align move's class
// rule back to C, C's centring rule back to R, and ends at a pixel of R or a
// constant (a background or the mask colour).  The classes are
// k_move_rect_g16's, stage by stage (move_class), so O is byte for byte what
// the two passes produce.  The border scan between the two moves reads only
// C's dark counts per row, which a dry centring pass (k_move_rect_g16 with
// kDry) counts from R without writing C.
//
// Columns: every stage's class changes only at a few columns (the move's
// five, the mask's two, and the first move's five seen through both possible
// outcomes of the second), so a row is a few intervals with one source
// offset or constant each.  A block (kMoveBlockRows rows of one sheet)
// finds the breakpoints, evaluates each (row, interval) once into LDS, and
// its lanes then write 16-byte vectors: one constant, or two aligned loads of
// R realigned by the interval's offset; vectors holding a breakpoint go byte
// by byte.
// ---------------------------------------------------------------------------
// k_move_rect_g16's class of (x, y) under move `a` (0 keep, 1 background,
// 2 moved: (x, y) become its source, 3 mask colour)
__device__ __forceinline__ int move_class(const MoveArgs& a, int32_t W, int32_t H, bool kmask,
                                          const Rect& mk, int32_t& x, int32_t& y) {
  const bool inmk = y >= mk.y0 && y <= mk.y1 && x >= mk.x0 && x <= mk.x1;
  if (!a.active) return kmask && !inmk ? 3 : 0;  // the identity: masked in place
  const Rect A = clip(a.area, W, H);
  const int32_t aw = A.x1 - A.x0 + 1, ah = A.y1 - A.y0 + 1;
  const int32_t sw = iabs(a.area.x0 - a.area.x1) + 1, sh = iabs(a.area.y0 - a.area.y1) + 1;
  const int32_t u = x - a.tx, v = y - a.ty;
  const bool trow = v >= 0 && v < sh, mrow = trow && v < ah;
  const bool arow = y >= A.y0 && y <= A.y1;
  const bool c1 = u >= 0 && u < sw, c2 = u < aw, c4 = x >= A.x0 && x <= A.x1;
  int cls = (trow && c1) ? ((mrow && c2) ? 2 : 1) : ((arow && c4) ? 1 : 0);
  if (kmask && cls == 0 && !inmk) cls = 3;
  if (cls == 2) {
    x = A.x0 + u;
    y = A.y0 + v;
  }
  return cls;
}

constexpr int kChainBp = 17;  // 7 of the align move and mask + 2 x 5 of the centring
#ifndef UPH_CHAIN_WAVES
#define UPH_CHAIN_WAVES 4
#endif
#ifndef UPH_CHAIN_OCC
#define UPH_CHAIN_OCC 1  // waves per SIMD the register budget must allow
#endif
constexpr int kChainThreads = 64 * UPH_CHAIN_WAVES;
constexpr int kChainRows = kMoveRows * UPH_CHAIN_WAVES;  // rows per block (kMoveRows a wave)
static_assert(kChainThreads >= kChainBp, "a thread per breakpoint");
struct ChainSheet {
  MoveArgs m1, m2;
  Rect mk;
  bool kmask;
  uint8_t mcol, bg1, bg2;
};
// The source of O(x, y): {-1, byte offset of the R pixel from (x, y)} or
// {constant, 0}
__device__ __forceinline__ int2 chain_cell(const ChainSheet& c, int32_t W, int32_t H,
                                           int64_t pitch, int32_t x, int32_t y) {
  int32_t sx = x, sy = y;
  const int c2 = move_class(c.m2, W, H, c.kmask, c.mk, sx, sy);
  if (c2 == 1) return make_int2(c.bg2, 0);
  if (c2 == 3) return make_int2(c.mcol, 0);
  const int c1 = move_class(c.m1, W, H, false, c.mk, sx, sy);
  if (c1 == 1) return make_int2(c.bg1, 0);
  return make_int2(-1, (int32_t)((int64_t)(sy - y) * pitch + (sx - x)));
}

__global__ void __launch_bounds__(kChainThreads, UPH_CHAIN_OCC) k_move_chain_g16(PlaneRef src, PlaneRef dst,
                                                             const MoveArgs* center,
                                                             const MaskArgs* masks,
                                                             const MoveArgs* align) {
  const int s = blockIdx.z;
  const Planes& P = src.P;
  const int32_t W = P.W, H = P.H;
  const int64_t pitch = P.pitch;
  const uint8_t* sbase = plane_ptr(src, s);
  uint8_t* dbase = plane_ptr(dst, s);
  const int32_t yb = blockIdx.x * kChainRows;
  const int nrows = imin(kChainRows, H - yb);
  ChainSheet c;
  c.m1 = center[s];
  c.m2 = align[s];
  const MaskArgs& ma = masks[s];
  c.kmask = ma.n > 0;
  c.mk = c.kmask ? normalize(ma.m[0]) : Rect{INT_MIN / 2, INT_MIN / 2, INT_MAX / 2, INT_MAX / 2};
  c.mcol = gray_of(Px{ma.color[0], ma.color[1], ma.color[2]});
  c.bg1 = gray_of(Px{c.m1.bg[0], c.m1.bg[1], c.m1.bg[2]});
  c.bg2 = gray_of(Px{c.m2.bg[0], c.m2.bg[1], c.m2.bg[2]});
  __shared__ int32_t bp[kChainBp];
  __shared__ int32_t nbp_s, nd_s;
  __shared__ int32_t dv[kChainBp + 1];  // vectors holding a breakpoint (+ the row's partial one)
  __shared__ uint8_t live[kChainBp], imap[kChainBp + 1];
  __shared__ int2 cell[kChainRows][kChainBp + 1];
  __shared__ int32_t b[kChainBp];  // thread 0's candidate list (LDS, not scratch)
  if (threadIdx.x == 0) {
    // the columns where some stage's class can change (first column of the
    // new interval), sorted, unique, inside (0, W)
    int n = 0;
    auto add = [&](int32_t v) {
      if (v > 0 && v < W) b[n++] = v;
    };
    const MoveArgs& m2 = c.m2;
    int32_t d2 = 0;
    if (m2.active) {
      const Rect A = clip(m2.area, W, H);
      const int32_t sw = iabs(m2.area.x0 - m2.area.x1) + 1;
      add(m2.tx);
      add(m2.tx + (A.x1 - A.x0 + 1));
      add(m2.tx + sw);
      add(A.x0);
      add(A.x1 + 1);
      d2 = A.x0 - m2.tx;
    }
    if (c.kmask) {
      add(c.mk.x0);
      add(c.mk.x1 + 1);
    }
    if (c.m1.active) {
      const MoveArgs& m1 = c.m1;
      const Rect A = clip(m1.area, W, H);
      const int32_t sw = iabs(m1.area.x0 - m1.area.x1) + 1;
      const int32_t q[5] = {m1.tx, m1.tx + (A.x1 - A.x0 + 1), m1.tx + sw, A.x0, A.x1 + 1};
      for (int k = 0; k < 5; k++) {
        add(q[k]);                  // seen through a kept column of the align move
        if (m2.active) add(q[k] - d2);  // through a moved one
      }
    }
    for (int i = 1; i < n; i++)  // insertion sort
      for (int k = i; k > 0 && b[k - 1] > b[k]; k--) {
        const int32_t t = b[k];
        b[k] = b[k - 1];
        b[k - 1] = t;
      }
    int m = 0;
    for (int i = 0; i < n; i++)
      if (m == 0 || b[i] != bp[m - 1]) bp[m++] = b[i];
    nbp_s = m;
  }
  __syncthreads();
  int nbp = nbp_s;
  // every (row, interval) of the block: interval i starts at column 0 or bp[i-1]
  for (int t = threadIdx.x; t < nrows * (nbp + 1); t += blockDim.x) {
    const int r = t / (nbp + 1), i = t - r * (nbp + 1);
    cell[r][i] = chain_cell(c, W, H, pitch, i == 0 ? 0 : bp[i - 1], yb + r);
  }
  __syncthreads();
  // a breakpoint whose two intervals have the same source in every row of
  // the block changes nothing here: dropped (fewer byte-path vectors)
  if ((int)threadIdx.x < nbp) {
    const int k = threadIdx.x;
    bool same = true;
    for (int r = 0; r < nrows; r++) {
      const int2 a = cell[r][k], b = cell[r][k + 1];
      same = same && a.x == b.x && a.y == b.y;
    }
    live[k] = !same;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int m = 0;
    imap[0] = 0;
    for (int k = 0; k < nbp; k++)
      if (live[k]) {
        bp[m++] = bp[k];  // in place: m <= k
        imap[m] = (uint8_t)(k + 1);
      }
    nbp_s = m;
    int nd = 0;
    for (int k = 0; k < m; k++) {
      const int32_t v = bp[k] >> 4;
      if ((bp[k] & 15) && (nd == 0 || dv[nd - 1] != v)) dv[nd++] = v;
    }
    if ((W & 15) && (nd == 0 || dv[nd - 1] != (W >> 4))) dv[nd++] = W >> 4;
    nd_s = nd;
    for (int k = m; k < kChainBp; k++) bp[k] = INT_MAX;  // the register copy's padding
  }
  __syncthreads();
  nbp = nbp_s;
  int32_t bpr[kChainBp];  // the breakpoints in registers (INT_MAX past nbp)
#pragma unroll
  for (int k = 0; k < kChainBp; k++) bpr[k] = __builtin_amdgcn_readfirstlane(bp[k]);  // uniform: SGPRs
  auto interval = [&](int32_t x) {
    int i = 0;
#pragma unroll
    for (int k = 0; k < kChainBp; k++) i += bpr[k] <= x;
    return i;
  };
  const int lane = threadIdx.x & 63;
  const int32_t nv = (W + 15) >> 4;
  const int r0 = (threadIdx.x >> 6) * kMoveRows;  // the wave's rows of the block
  // uniform vectors: lanes along the row, the wave's kMoveRows rows
#ifndef UPH_CHAIN_KG
#define UPH_CHAIN_KG 4
#endif
  constexpr int kG = UPH_CHAIN_KG;  // rows whose loads are in flight together
  for (int32_t vi = lane; vi < nv; vi += 64) {
    const int32_t x0 = 16 * vi;
    const int il = interval(x0);
    if (x0 + 16 > W || il != interval(x0 + 15)) continue;  // byte path below
#pragma unroll
    for (int k0 = 0; k0 < kMoveRows; k0 += kG) {
      int2 ce[kG];
      int r16[kG];
      uint4 lo[kG], hi[kG];
#pragma unroll
      for (int j = 0; j < kG; j++) {
        // R bytes x0 + off .. + 15 of the row's cell: two aligned vectors
        // realigned by (off mod 16), the same for every vector of the interval
        const int r = r0 + k0 + j;
        ce[j] = r < nrows ? cell[r][imap[il]] : make_int2(0, 0);
        r16[j] = 0;
        lo[j] = hi[j] = make_uint4(0u, 0u, 0u, 0u);
        if (r < nrows && ce[j].x < 0) {
          const uint8_t* p = sbase + (int64_t)(yb + r) * pitch + x0 + ce[j].y;
          r16[j] = (int)((uintptr_t)p & 15u);
          const uint4* q = reinterpret_cast<const uint4*>(p - r16[j]);
          lo[j] = q[0];
          if (r16[j]) hi[j] = q[1];
        }
      }
#pragma unroll
      for (int j = 0; j < kG; j++) {
        const int r = r0 + k0 + j;
        if (r >= nrows) break;
        uint4 out;
        if (ce[j].x >= 0) {
          const uint32_t v4 = (uint32_t)ce[j].x * 0x01010101u;
          out = make_uint4(v4, v4, v4, v4);
        } else {
          const uint32_t w[8] = {lo[j].x, lo[j].y, lo[j].z, lo[j].w,
                                 hi[j].x, hi[j].y, hi[j].z, hi[j].w};
          const int ru = __builtin_amdgcn_readfirstlane(r16[j]);
          if (__builtin_amdgcn_ballot_w64(r16[j] != ru) == 0) {
            // the wave's vectors share one realignment (one cell, usually):
            // a uniform dword select, as k_move_rect_g16 does
            const int rb = ru & 3;
            switch (ru >> 2) {
              case 0: out = shift_bytes16<0>(w, rb); break;
              case 1: out = shift_bytes16<1>(w, rb); break;
              case 2: out = shift_bytes16<2>(w, rb); break;
              default: out = shift_bytes16<3>(w, rb); break;
            }
          } else {
            const int qd = r16[j] >> 2, rb = r16[j] & 3;
            uint32_t d[5];
#pragma unroll
            for (int m = 0; m < 5; m++)
              d[m] = qd == 0 ? w[m] : qd == 1 ? w[m + 1] : qd == 2 ? w[m + 2] : w[m + 3];
            out = make_uint4(__builtin_amdgcn_alignbyte(d[1], d[0], rb),
                             __builtin_amdgcn_alignbyte(d[2], d[1], rb),
                             __builtin_amdgcn_alignbyte(d[3], d[2], rb),
                             __builtin_amdgcn_alignbyte(d[4], d[3], rb));
          }
        }
        *reinterpret_cast<uint4*>(dbase + (int64_t)(yb + r) * pitch + x0) = out;
      }
    }
  }
  // vectors holding a breakpoint, and the row's partial last vector: a lane
  // per (row, vector), interval by interval, byte by byte; columns >= W are
  // written as 0
  const int nd = nd_s;
  for (int t = threadIdx.x; t < nrows * nd; t += blockDim.x) {
    const int r = t / nd, x0 = 16 * dv[t - r * nd];
    const int32_t y = yb + r;
    const uint8_t* srow = sbase + (int64_t)y * pitch;
    uint64_t o0 = 0, o1 = 0;
    const int il = interval(x0), ih = interval(imin(x0 + 15, W - 1));
    if (ih - il <= 3) {
      // the (at most three) breakpoints inside the vector; every byte's
      // source is independent of the others, so all 16 loads are in flight
      int32_t bk[3];
#pragma unroll
      for (int m = 0; m < 3; m++) bk[m] = il + m < ih ? bp[il + m] : INT_MAX;
      uint32_t v[16];
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const int32_t x = x0 + j;
        const int i = il + (bk[0] <= x) + (bk[1] <= x) + (bk[2] <= x);
        const int2 ce = cell[r][imap[i]];
        v[j] = x >= W ? 0u : ce.x >= 0 ? (uint32_t)ce.x : (uint32_t)srow[x + ce.y];
      }
#pragma unroll
      for (int j = 0; j < 8; j++) {
        o0 |= (uint64_t)v[j] << (8 * j);
        o1 |= (uint64_t)v[8 + j] << (8 * j);
      }
    } else {
      for (int i = il; i <= ih; i++) {
        const int32_t s0 = imax(i == 0 ? 0 : bp[i - 1], x0);
        const int32_t s1 = imin(imin(i < nbp ? bp[i] : W, W), x0 + 16);
        const int2 ce = cell[r][imap[i]];
        for (int32_t x = s0; x < s1; x++) {
          const uint64_t v = ce.x >= 0 ? (uint64_t)ce.x : (uint64_t)srow[x + ce.y];
          const int j = x - x0;
          if (j < 8) o0 |= v << (8 * j);
          else o1 |= v << (8 * (j - 8));
        }
      }
    }
    *reinterpret_cast<uint4*>(dbase + (int64_t)y * pitch + x0) =
        make_uint4((uint32_t)o0, (uint32_t)(o0 >> 32), (uint32_t)o1, (uint32_t)(o1 >> 32));
  }
}

bool launch_move_chain(const PlaneRef& src, const PlaneRef& dst, const MoveArgs* center,
                       const MaskArgs* masks, const MoveArgs* align, int count, hipStream_t st) {
  if (src.P.fmt != F_GRAY8 || src.P.pitch * (int64_t)src.P.H >= (1ll << 31) || src.P.H < 1)
    return false;
  const int64_t blocks = (src.P.H + kChainRows - 1) / kChainRows;
  UPH_LAUNCH_DIAG(4, k_move_chain_g16, dim3((unsigned)blocks, 1, count), dim3(kChainThreads), 0, st,
                  src, dst, center, masks, align);
  return true;
}

}  // namespace uph
