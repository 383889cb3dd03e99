// kernels_decode.hip — the GRAY8 page decode for gfx950: a pipeline stage of
// its own that, on the way, writes planes the noisefilter, the blurfilter and
// the blackfilter (kernels_black.hip) would otherwise compute themselves.
#include "filters_common.h"

namespace uph {

// The decode of a GRAY8 page into its sheet (sheet_stages.c:151-165 with the
// page covering the sheet: a plain copy) fused with the first pass that reads
// the result: the noisefilter's dark bit-plane (k_noise_bits).  A lane per
// 32-pixel word of the whole sheet (rows are ceil(W/32) words, not a multiple
// of 64: a wave per row would leave most lanes of its second pass idle): two
// 16-byte loads, two 16-byte stores (the row's last word in pieces up to W),
// one bit-plane word.
__global__ void __launch_bounds__(256) k_decode_gray(const uint8_t* src, int64_t spitch,
                                                     int64_t sstride, PlaneRef dst, uint8_t white,
                                                     uint32_t* bits, int64_t bstride, int32_t nwr,
                                                     float rnwr, uint32_t* bbits, uint32_t* rm,
                                                     int64_t rm_stride, uint32_t rm_max) {
  const int s = blockIdx.y;
  const Planes& P = dst.P;
  const int32_t t = blockIdx.x * 256 + threadIdx.x;
  // t / nwr from the float reciprocal, corrected by one either way
  int32_t y = (int32_t)((float)t * rnwr);
  if (y * nwr > t) y--;
  else if ((y + 1) * nwr <= t) y++;
  if (y >= P.H) return;
  const int32_t wi = t - y * nwr, x0 = 32 * wi;
  const uint8_t* srow = src + s * sstride + (int64_t)y * spitch;
  uint8_t* d = plane_ptr(dst, s) + (int64_t)y * P.pitch + x0;
  // a 16-byte chunk starting before W lies inside the 16-aligned pitch
  const uint4 a = *reinterpret_cast<const uint4*>(srow + x0);
  const uint4 b = x0 + 16 < P.W ? *reinterpret_cast<const uint4*>(srow + x0 + 16)
                                : make_uint4(~0u, ~0u, ~0u, ~0u);
  uint32_t m = dark_bits32({a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}, white);
  // the blurfilter's bits: pixel <= white (byte < white + 1)
  uint32_t mb = bbits ? dark_bits32({a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}, (uint32_t)white + 1u) : 0u;
  // the blackfilter's match plane: pixel <= mask_max
  uint32_t mr = rm ? dark_bits32({a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}, rm_max + 1u) : 0u;
  if (x0 + 32 <= P.W) {
    *reinterpret_cast<uint4*>(d) = a;
    *reinterpret_cast<uint4*>(d + 16) = b;
  } else {
    // the row's last word: n = W - x0 in [1, 31] bytes, as a 16-byte chunk,
    // dwords and the last dword's bytes
    const int32_t n = P.W - x0;
    m &= (1u << n) - 1u;
    mb &= (1u << n) - 1u;
    mr &= (1u << n) - 1u;
    uint4 q = a;
    int32_t j = 0;
    if (n >= 16) {
      *reinterpret_cast<uint4*>(d) = a;
      q = b;
      j = 16;
    }
    const int32_t r = n - j;  // 0..15
    if (r >= 4) *reinterpret_cast<uint32_t*>(d + j) = q.x;
    if (r >= 8) *reinterpret_cast<uint32_t*>(d + j + 4) = q.y;
    if (r >= 12) *reinterpret_cast<uint32_t*>(d + j + 8) = q.z;
    uint32_t last = r < 4 ? q.x : r < 8 ? q.y : r < 12 ? q.z : q.w;
    for (int32_t i = j + (r & ~3); i < n; i++, last >>= 8) d[i] = (uint8_t)last;
  }
  if (bits) bits[s * bstride + t] = m;
  if (bbits) bbits[s * bstride + t] = mb;
  if (rm) {  // rows of (nwr + 1) & ~1 words: an odd row's pad word is 0
    const int32_t rw = (nwr + 1) & ~1;
    uint32_t* r = rm + s * rm_stride + (int64_t)y * rw + wi;
    if (wi + 1 == nwr && (nwr & 1)) *reinterpret_cast<uint2*>(r) = make_uint2(mr, 0u);
    else *r = mr;
  }
}

// What k_decode_gray does with its word once it holds the sheet's 32 bytes at
// (x0, y) as a and b, for the fit decode below (k_decode_gray keeps its own
// text: its code is the measured one): the three bit-plane words from them,
// the bytes stored (the row's last word in pieces up to W).
__device__ __forceinline__ void decode_word_out(const uint4 a, const uint4 b, const PlaneRef& dst, int s,
                                                int32_t t, int32_t y, int32_t wi, int32_t nwr,
                                                uint8_t white, uint32_t* bits, int64_t bstride,
                                                uint32_t* bbits, uint32_t* rm, int64_t rm_stride,
                                                uint32_t rm_max) {
  const Planes& P = dst.P;
  const int32_t x0 = 32 * wi;
  uint8_t* d = plane_ptr(dst, s) + (int64_t)y * P.pitch + x0;
  uint32_t m = dark_bits32({a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}, white);
  // the blurfilter's bits: pixel <= white (byte < white + 1)
  uint32_t mb = bbits ? dark_bits32({a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}, (uint32_t)white + 1u) : 0u;
  // the blackfilter's match plane: pixel <= mask_max
  uint32_t mr = rm ? dark_bits32({a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}, rm_max + 1u) : 0u;
  if (x0 + 32 <= P.W) {
    *reinterpret_cast<uint4*>(d) = a;
    *reinterpret_cast<uint4*>(d + 16) = b;
  } else {
    // the row's last word: n = W - x0 in [1, 31] bytes, as a 16-byte chunk,
    // dwords and the last dword's bytes
    const int32_t n = P.W - x0;
    m &= (1u << n) - 1u;
    mb &= (1u << n) - 1u;
    mr &= (1u << n) - 1u;
    uint4 q = a;
    int32_t j = 0;
    if (n >= 16) {
      *reinterpret_cast<uint4*>(d) = a;
      q = b;
      j = 16;
    }
    const int32_t r = n - j;  // 0..15
    if (r >= 4) *reinterpret_cast<uint32_t*>(d + j) = q.x;
    if (r >= 8) *reinterpret_cast<uint32_t*>(d + j + 4) = q.y;
    if (r >= 12) *reinterpret_cast<uint32_t*>(d + j + 8) = q.z;
    uint32_t last = r < 4 ? q.x : r < 8 ? q.y : r < 12 ? q.z : q.w;
    for (int32_t i = j + (r & ~3); i < n; i++, last >>= 8) d[i] = (uint8_t)last;
  }
  if (bits) bits[s * bstride + t] = m;
  if (bbits) bbits[s * bstride + t] = mb;
  if (rm) {  // rows of (nwr + 1) & ~1 words: an odd row's pad word is 0
    const int32_t rw = (nwr + 1) & ~1;
    uint32_t* r = rm + s * rm_stride + (int64_t)y * rw + wi;
    if (wi + 1 == nwr && (nwr & 1)) *reinterpret_cast<uint2*>(r) = make_uint2(mr, 0u);
    else *r = mr;
  }
}

// The same decode with the page placed in the sheet (center_image, blit.c:
// 175-202): sheet pixel (x, y) is page pixel (x - tx + a.x0, y - ty + a.y0)
// inside the placed rectangle place[s] (a: the clipped page area, as k_copy
// takes it) and the background byte elsewhere; the planes come from the
// merged bytes.  It replaces the sheet's fill and the copy.
//
// The page bytes of a word start at any byte offset, so a lane reads the
// three 16-byte chunks [c0, c0 + 48) that cover them, c0 the word's first
// page column rounded down to 16, and shifts them into place.  A chunk is
// read only when it holds a column the word takes, [lo, hi) within
// [a.x0, a.x1 + 1): such a chunk starts at or after column 0 and ends at or
// before the page's width rounded up to 16, inside the 16-aligned pitch.
// Rows outside the rectangle load nothing.
__global__ void __launch_bounds__(256) k_decode_gray_fit(const uint8_t* src, int64_t spitch,
                                                         int64_t sstride, const CopyArgs* place,
                                                         uint32_t bg4, PlaneRef dst, uint8_t white,
                                                         uint32_t* bits, int64_t bstride, int32_t nwr,
                                                         float rnwr, uint32_t* bbits, uint32_t* rm,
                                                         int64_t rm_stride, uint32_t rm_max) {
  const int s = blockIdx.y;
  const Planes& P = dst.P;
  const int32_t t = blockIdx.x * 256 + threadIdx.x;
  int32_t y = (int32_t)((float)t * rnwr);
  if (y * nwr > t) y--;
  else if ((y + 1) * nwr <= t) y++;
  if (y >= P.H) return;
  const int32_t wi = t - y * nwr, x0 = 32 * wi;
  const CopyArgs p = place[s];
  const int32_t w = p.a.x1 - p.a.x0 + 1, h = p.a.y1 - p.a.y0 + 1;
  // the sheet columns of this word that the page covers: [xa, xb)
  const int32_t xa = imax(x0, p.tx), xb = imin(x0 + 32, p.tx + w);
  uint32_t v[8];
#pragma unroll
  for (int i = 0; i < 8; i++) v[i] = bg4;
  if (p.active && y >= p.ty && y < p.ty + h && xa < xb) {
    const uint8_t* srow = src + s * sstride + (int64_t)(y - p.ty + p.a.y0) * spitch;
    const int32_t p0 = x0 - p.tx + p.a.x0;  // the page column under the word's first byte, may be < 0
    const int32_t lo = xa - p.tx + p.a.x0, hi = xb - p.tx + p.a.x0;
    const int32_t c0 = p0 & ~15;
    uint32_t c[12];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const int32_t cb = c0 + 16 * k;
      uint4 q = make_uint4(0u, 0u, 0u, 0u);
      if (cb + 16 > lo && cb < hi) q = *reinterpret_cast<const uint4*>(srow + cb);
      c[4 * k] = q.x;
      c[4 * k + 1] = q.y;
      c[4 * k + 2] = q.z;
      c[4 * k + 3] = q.w;
    }
    // bytes [p0, p0 + 32) of the 48: whole dwords first, then the odd bytes
    const int32_t sh = p0 - c0, qd = sh >> 2;
    uint32_t e[9];
#pragma unroll
    for (int i = 0; i < 9; i++)
      e[i] = qd == 0 ? c[i] : qd == 1 ? c[i + 1] : qd == 2 ? c[i + 2] : c[i + 3];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint32_t px = __builtin_amdgcn_alignbyte(e[i + 1], e[i], (uint32_t)(sh & 3));
      // the dword's bytes below xa and from xb on stay background
      const int32_t xs = x0 + 4 * i;
      const int32_t nl = imin(imax(xa - xs, 0), 4), nh = imin(imax(xs + 4 - xb, 0), 4);
      const uint32_t keep = nl + nh >= 4 ? 0u : (0xFFFFFFFFu << (8 * nl)) & (0xFFFFFFFFu >> (8 * nh));
      v[i] = (px & keep) | (bg4 & ~keep);
    }
  }
  decode_word_out(make_uint4(v[0], v[1], v[2], v[3]), make_uint4(v[4], v[5], v[6], v[7]), dst, s, t, y,
                  wi, nwr, white, bits, bstride, bbits, rm, rm_stride, rm_max);
}

// The blackfilter's v-stripe row sums (darkness_rect's sums over the stripe's
// columns [vx0, vx1], filters.c:49-104) straight from the GRAY8 pages the
// decode copies unchanged.  A half-wave per row (32 lanes x 16 bytes cover a
// 500-column stripe in one load each), eight rows per wave with all their
// loads in flight, SAD byte sums, then a 32-lane sum per row.
constexpr int kStripeRowsPerWave = 8;
__global__ void __launch_bounds__(256) k_stripe_sums(const uint8_t* src, int64_t spitch,
                                                     int64_t sstride, int32_t H, uint32_t* vsum,
                                                     int64_t vstride, int32_t vx0, int32_t vx1) {
  const int s = blockIdx.y;
  const int lane = threadIdx.x & 63, half = lane >> 5, hl = lane & 31;
  const int32_t yw = (blockIdx.x * 4 + (threadIdx.x >> 6)) * kStripeRowsPerWave;
  if (yw >= H) return;
  const uint8_t* page = src + s * sstride;
  const int32_t xa = vx0 & ~15;
  constexpr int kR = kStripeRowsPerWave / 2;  // rows per half-wave
  uint32_t acc[kR] = {};
  for (int32_t x = xa + 16 * hl; x <= vx1; x += 16 * 32) {  // one pass for stripes <= 512 columns
    uint32_t keep[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int32_t xq = x + 4 * q;
      keep[q] = 0;
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (xq + j >= vx0 && xq + j <= vx1) keep[q] |= 0xFFu << (8 * j);
    }
    uint4 v[kR];
#pragma unroll
    for (int r = 0; r < kR; r++) {
      const int32_t y = imin(yw + 2 * r + half, H - 1);
      v[r] = *reinterpret_cast<const uint4*>(page + (int64_t)y * spitch + x);
    }
#pragma unroll
    for (int r = 0; r < kR; r++) {
      acc[r] = __builtin_amdgcn_sad_u8(v[r].x & keep[0], 0u, acc[r]);
      acc[r] = __builtin_amdgcn_sad_u8(v[r].y & keep[1], 0u, acc[r]);
      acc[r] = __builtin_amdgcn_sad_u8(v[r].z & keep[2], 0u, acc[r]);
      acc[r] = __builtin_amdgcn_sad_u8(v[r].w & keep[3], 0u, acc[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < kR; r++) {
    uint32_t a = acc[r];
    for (int o = 16; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);  // within the half-wave
    const int32_t y = yw + 2 * r + half;
    if (hl == 0 && y < H) vsum[s * vstride + y] = a;
  }
}

void launch_decode_gray(const uint8_t* src, int64_t spitch, int64_t sstride, const PlaneRef& dst,
                        uint8_t white, const SheetBits& bits, const BlackGeom& bg,
                        void* black_scratch, int64_t scratch_stride, int count, hipStream_t st) {
  const int32_t nwr = (dst.P.W + 31) >> 5;
  const int64_t words = (int64_t)nwr * dst.P.H;
  UPH_LAUNCH_DIAG(262144, k_decode_gray, dim3((unsigned)((words + 255) / 256), count), dim3(256), 0, st,
                     src, spitch, sstride, dst, white, bits.nbits, bits.stride, nwr, 1.0f / (float)nwr,
                     bits.bbits, bits.rm ? black_rm_plane(bg, black_scratch) : nullptr,
                     scratch_stride / 4, (uint32_t)bg.mask_max);
  if (bits.vsum && bg.vregion.x0 <= bg.vregion.x1)
    hipLaunchKernelGGL(k_stripe_sums,
                       dim3((unsigned)((dst.P.H + 4 * kStripeRowsPerWave - 1) / (4 * kStripeRowsPerWave)),
                            count),
                       dim3(256), 0, st, src, spitch, sstride, dst.P.H,
                       (uint32_t*)black_scratch + bg.W,  // the row sums follow the W column sums
                       scratch_stride / 4, bg.vregion.x0, bg.vregion.x1);
}

void launch_decode_gray_fit(const uint8_t* src, int64_t spitch, int64_t sstride, const CopyArgs* place,
                            uint8_t background, const PlaneRef& dst, uint8_t white, const SheetBits& bits,
                            const BlackGeom& bg, void* black_scratch, int64_t scratch_stride, int count,
                            hipStream_t st) {
  const int32_t nwr = (dst.P.W + 31) >> 5;
  const int64_t words = (int64_t)nwr * dst.P.H;
  hipLaunchKernelGGL(k_decode_gray_fit, dim3((unsigned)((words + 255) / 256), count), dim3(256), 0, st, src,
                     spitch, sstride, place, background * 0x01010101u, dst, white, bits.nbits, bits.stride,
                     nwr, 1.0f / (float)nwr, bits.bbits,
                     bits.rm ? black_rm_plane(bg, black_scratch) : nullptr, scratch_stride / 4,
                     (uint32_t)bg.mask_max);
}

}  // namespace uph
