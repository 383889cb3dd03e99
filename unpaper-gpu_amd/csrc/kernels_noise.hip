// kernels_noise.hip — the noisefilter for gfx950 (the split into a parallel
// pass and an exact resolution: see kernels_gray.hip).
#include "filters_common.h"
#include "noise_planes.h"

namespace uph {

// =========================================================================
// NOISEFILTER (filters.c:238-338)
//   Raster scan; a pixel p with max(rgb) < white ("trigger") counts the
//   pixels with min(rgb) < white ("dark") in square rings of level 1..N
//   (N = intensity) until a ring is empty; if 1 + rings <= N the centre and
//   the counted rings are cleared.  Away from the left/top edge (where the
//   ring loops' unsigned comparisons drop whole rows, see oracle.c) an empty
//   ring separates its inside from everything else, so a clear removes whole
//   8-connected dark components of <= N pixels ("small").  Hence:
//     * triggers of large components outside the edge zone never clear;
//     * a small component C farther than 2N-1 from any other small pixel and
//       from the edge zone is cleared iff one of its triggers passes the test
//       on the ORIGINAL image (nothing that test reads ever changes);
//     * everything else (edge zone, clustered small components) is replayed
//       literally, in raster order, by one wave per sheet.
//   The parallel path is used for N <= 4 (radius constants below).
//   Y400A and RGB24 classify in tiles staged from the bytes
//   (k_noise_classify); GRAY8 classifies its dark bit-plane in two streaming
//   passes (k_noise_cand, k_noise_verdict: noise_planes.h).
// =========================================================================
constexpr int kNT = 64;                    // tile height and width
constexpr int kHalo = 14;                  // 4 (ring) + 7 (cluster) + 3 (component)
constexpr int kRW = kNT + 2 * kHalo;       // 92 region rows and columns
constexpr int kZone = kNpZone;             // sequential edge zone (x or y < 32)
constexpr int kEligible = kNpEligible;     // parallel only for components at >= 40

bool noise_geometry(int32_t W, int32_t H, uint64_t intensity, uint8_t white, NoiseGeom* g) {
  g->W = W;
  g->H = H;
  g->intensity = intensity > 64 ? 64 : (int32_t)intensity;
  g->white = white;
  // the parallel path only queues edge-zone and clustered triggers; the
  // all-sequential path (intensity > 4) may queue every pixel
  g->all_seq = intensity > 4 ? 1 : 0;
  int64_t cap = g->all_seq ? (int64_t)W * H + 64 : ((int64_t)W * H) / 4 + 1024;
  if (cap > (1 << 27)) cap = 1 << 27;
  g->capacity = (int32_t)cap;
  return true;
}

static size_t noise_list_bytes(const NoiseGeom& g) {
  // counters (2 x u32 padded to 256 B) + clear list + seq list
  size_t b = 256 + (size_t)g.capacity * 4 * 2;
  return (b + 255) & ~(size_t)255;
}

static size_t pow2_at_least(size_t n) {
  size_t p = 1;
  while (p < n) p <<= 1;
  return p;
}

// 32-pixel words per row of the GRAY8 dark bit-plane
static int32_t noise_bit_words(const NoiseGeom& g) { return noise_bit_words(g.W); }

// k_noise_group keeps up to 16 triggers a thread in LDS (more: in HBM)
constexpr int kCapPerThread = 16;
size_t noise_scratch_bytes(const NoiseGeom& g) {
  // lists + a global sort buffer for the rare > 8192-trigger sequential case;
  // the GRAY8 dark bit-plane and, behind it, the small bit-plane share the
  // sort buffer's space (they are read by k_noise_cand / k_noise_verdict
  // only, before k_noise_group may sort; narrow tall images need more for
  // the two planes than for the sort)
  // (and k_noise_group's keys / roots / last, 3 x its LDS cap words)
  size_t sort = 4 * pow2_at_least((size_t)g.capacity);
  const size_t cap3 = 12 * (size_t)kCapPerThread * (size_t)noise_group_threads(g.W, g.H);
  if (sort < cap3) sort = cap3;
  const size_t bits = 2 * 4 * (size_t)noise_bit_words(g) * (size_t)g.H;
  return noise_list_bytes(g) + (sort > bits ? sort : bits);
}

struct NoisePtrs {
  uint32_t* nclear;
  uint32_t* nseq;
  uint32_t* clear;
  uint32_t* seq;
};
__device__ __forceinline__ NoisePtrs noise_ptrs(const NoiseGeom& g, uint8_t* base) {
  NoisePtrs p;
  p.nclear = (uint32_t*)base;
  p.nseq = p.nclear + 1;
  p.clear = (uint32_t*)(base + 256);
  p.seq = p.clear + g.capacity;
  return p;
}

// 9 bits of a region row bitmask starting at column c (bit i = column c+i)
__device__ __forceinline__ uint32_t row9(const uint32_t* w, int c) {
  const int word = c >> 5, off = c & 31;
  uint64_t v = ((uint64_t)w[word + 1] << 32) | w[word];
  return (uint32_t)(v >> off) & 0x1FFu;
}

// Dark component of (cx,cy) restricted to its 9x9 box; returns popcount
// (capped growth after 4 dilations) and the mask rows.  Every dilation step
// only adds pixels connected to the centre, so the search stops as soon as
// more than 4 are reached (the component is large; text strokes exit after
// the first step, whose 3x3 neighbourhood is all 8-adjacent to the centre).
__device__ __forceinline__ int flood9(const uint32_t (*drow)[4], int cx, int cy, uint32_t* comp) {
  uint32_t D[9], cur[9];
#pragma unroll
  for (int r = 0; r < 9; r++) {
    D[r] = row9(drow[cy - 4 + r], cx - 4);
    cur[r] = 0;
  }
  cur[4] = 1u << 4;
  for (int it = 0; it < 4; it++) {
    uint32_t nx[9];
    bool same = true;
    int n = 0;
#pragma unroll
    for (int r = 0; r < 9; r++) {
      uint32_t u = cur[r] | (r > 0 ? cur[r - 1] : 0) | (r < 8 ? cur[r + 1] : 0);
      u = (u | (u << 1) | (u >> 1)) & D[r] & 0x1FFu;
      nx[r] = u;
      same &= (u == cur[r]);
      n += __popc(u);
    }
#pragma unroll
    for (int r = 0; r < 9; r++) cur[r] = nx[r];
    if (n > 4) {
#pragma unroll
      for (int r = 0; r < 9; r++) comp[r] = cur[r];
      return n;
    }
    if (same) break;
  }
  int n = 0;
#pragma unroll
  for (int r = 0; r < 9; r++) {
    comp[r] = cur[r];
    n += __popc(cur[r]);
  }
  return n;
}

// bits [c, c+n) of a 128-bit region row (n <= 32, c + n <= 128)
__device__ __forceinline__ uint32_t row_bits(const uint32_t* w, int c, int n) {
  const int word = c >> 5, off = c & 31;
  const uint64_t v = ((uint64_t)(word < 3 ? w[word + 1] : 0u) << 32) | w[word];
  return (uint32_t)(v >> off) & (n >= 32 ? 0xFFFFFFFFu : ((1u << n) - 1u));
}

// Append the (gx, gy) keys of the lanes with `want` to a list: one atomic per
// wave, ballot-compacted.
__device__ __forceinline__ void wave_append(bool want, int32_t gx, int32_t gy, uint32_t* counter,
                                            uint32_t* list, int32_t capacity) {
  const unsigned long long M = __ballot(want);
  if (!M) return;
  const int lane = threadIdx.x & 63;
  uint32_t base = 0;
  const int leader = __ffsll((long long)M) - 1;
  if (lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(M));
  base = __shfl(base, leader, 64);
  if (want) {
    const uint32_t k = base + (uint32_t)__popcll(M & ((1ull << lane) - 1ull));
    if (k < (uint32_t)capacity) list[k] = ((uint32_t)gy << 16) | (uint32_t)gx;
  }
}

// The same for two lists (a lane wants at most one): both counters' atomics
// are under way before either answer is waited for.
__device__ __forceinline__ void wave_append2(bool want1, bool want2, int32_t gx, int32_t gy,
                                             uint32_t* counter1, uint32_t* list1,
                                             uint32_t* counter2, uint32_t* list2,
                                             int32_t capacity) {
  const unsigned long long M1 = __ballot(want1), M2 = __ballot(want2);
  if (!(M1 | M2)) return;
  const int lane = threadIdx.x & 63;
  uint32_t b1 = 0, b2 = 0;
  if (lane == 0) {
    if (M1) b1 = atomicAdd(counter1, (uint32_t)__popcll(M1));
    if (M2) b2 = atomicAdd(counter2, (uint32_t)__popcll(M2));
  }
  b1 = __shfl(b1, 0, 64);
  b2 = __shfl(b2, 0, 64);
  const unsigned long long below = (1ull << lane) - 1ull;
  const uint32_t k = want1 ? b1 + (uint32_t)__popcll(M1 & below) : b2 + (uint32_t)__popcll(M2 & below);
  if ((want1 | want2) && k < (uint32_t)capacity)
    (want1 ? list1 : list2)[k] = ((uint32_t)gy << 16) | (uint32_t)gx;
}

// GRAY8 dark bit-plane: bit b of word w of row y is (pixel 32 w + b < white);
// columns >= W are 0.  One lane per word, two 16-byte loads (rows are
// 256-byte pitched, so a row's last word reads inside the pitch).  For a
// plane filtered on its own; in the pipeline the decode hands the plane on
// (SheetBits::nbits).
__global__ void __launch_bounds__(256) k_noise_bits(PlaneRef img, NoiseGeom g, uint32_t* bits,
                                                    int64_t bstride, int32_t nwr, float rnwr) {
  const int s = blockIdx.y;
  const int32_t t = blockIdx.x * 256 + threadIdx.x;
  // t / nwr from the float reciprocal, corrected by one either way
  int32_t y = (int32_t)((float)t * rnwr);
  if (y * nwr > t) y--;
  else if ((y + 1) * nwr <= t) y++;
  if (y >= g.H) return;
  const int32_t wi = t - y * nwr, x0 = 32 * wi;
  const uint4* p = reinterpret_cast<const uint4*>(plane_ptr(img, s) + (int64_t)y * img.P.pitch + x0);
  const uint4 a = p[0], b = p[1];
  uint32_t m = dark_bits32({a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}, g.white);
  if (x0 + 32 > g.W) m &= (1u << (g.W - x0)) - 1u;  // g.W - x0 in [1, 31]
  bits[s * bstride + t] = m;
}

// Whether the classification of a small dark pixel (tile coordinates rx, ry)
// must go to the sequential replay, or clears it in parallel (see above).
struct SmallVerdict {
  bool seq, clear;
};
// A small component (<= 4 pixels) as offsets from one of its pixels, packed
// one byte a pixel (dx + 4 | (dy + 4) << 4, 0xFF = none): the restricted
// flood's result, kept from the candidate pass for the verdict pass.
constexpr uint32_t kNotSmall = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t pack_comp(const uint32_t (&comp)[9]) {
  uint32_t rec = kNotSmall;
  int nc = 0;
#pragma unroll
  for (int r = 0; r < 9; r++) {
    uint32_t mm = comp[r];
    while (mm) {
      const int b = __ffs(mm) - 1;
      mm &= mm - 1;
      if (nc < 4) rec = (rec & ~(0xFFu << (8 * nc))) | ((uint32_t)(b | (r << 4)) << (8 * nc));
      nc++;
    }
  }
  return nc <= 4 ? rec : kNotSmall;
}
// The verdict from the component's pixels (offsets cxs, cys from (rx, ry)).
__device__ __forceinline__ SmallVerdict small_verdict_pixels(const uint32_t (*drow)[4],
                                                             const uint32_t (*trow)[4],
                                                             const uint32_t (*srow)[4], int rx,
                                                             int ry, int32_t gx, int32_t gy,
                                                             bool trig, int N, int nc,
                                                             const int (&cxs)[4],
                                                             const int (&cys)[4]) {
  SmallVerdict v{false, false};
  int bx0 = 4, bx1 = -4, by0 = 4, by1 = -4;  // bounding box, offsets from (rx, ry)
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (k < nc) {
      bx0 = imin(bx0, cxs[k]);
      bx1 = imax(bx1, cxs[k]);
      by0 = imin(by0, cys[k]);
      by1 = imax(by1, cys[k]);
    }
  bool eligible = nc <= 4 && gx + bx0 >= kEligible && gy + by0 >= kEligible;
  // no foreign small pixel within Chebyshev 7 of the component: checked on
  // the bounding box dilated by 7 (a superset, so a component rejected here
  // merely takes the exact sequential path).  At most 4 + 14 rows: a fixed,
  // unrolled count, so the row reads are in flight together.
  if (eligible) {
    const int X0 = rx + bx0 - 7, n = bx1 - bx0 + 15;
    const int r0 = ry + by0 - 7, r1 = ry + by1 + 7;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < 18; j++)
      if (r0 + j <= r1) cnt += __popc(row_bits(srow[r0 + j], X0, n));
    eligible = cnt == nc;
  }
  if (!eligible) {
    v.seq = trig;
    return v;
  }
  // cleared iff some trigger of the component passes the ring test on the
  // original image (eligible pixels are >= 40 from the edges, so the
  // reference's unsigned ring-loop skips never apply).  Rings up to N <= 4
  // (larger intensities take the sequential path): the pixel's 9x9 dark
  // window read once, every ring's count from it in registers.
  for (int k = 0; k < nc && k < 4 && !v.clear; k++) {
    const int cx = rx + (k == 0 ? cxs[0] : k == 1 ? cxs[1] : k == 2 ? cxs[2] : cxs[3]);
    const int cy = ry + (k == 0 ? cys[0] : k == 1 ? cys[1] : k == 2 ? cys[2] : cys[3]);
    if (!((trow[cy][cx >> 5] >> (cx & 31)) & 1)) continue;
    uint32_t D[9];  // bit i of D[r]: pixel (cx - 4 + i, cy - 4 + r)
#pragma unroll
    for (int r = 0; r < 9; r++) D[r] = row_bits(drow[cy - 4 + r], cx - 4, 9);
    // noisefilter_count_pixel_neighbors (filters.c:256-300): count 1, then each level's ring until
    // an empty one or past N
    int count = 1;
    bool go = true;
#pragma unroll
    for (int L = 1; L <= 4; L++) {
      if (!go || L > N) break;
      const uint32_t span = ((1u << (2 * L + 1)) - 1u) << (4 - L);
      const uint32_t ends = (1u << (4 - L)) | (1u << (4 + L));
      int lc = __popc(D[4 - L] & span) + __popc(D[4 + L] & span);
#pragma unroll
      for (int r = 4 - L + 1; r <= 4 + L - 1; r++) lc += __popc(D[r] & ends);
      count += lc;
      go = lc != 0;
    }
    v.clear = count <= N;
  }
  return v;
}
__device__ __forceinline__ SmallVerdict small_verdict_rec(const uint32_t (*drow)[4],
                                                          const uint32_t (*trow)[4],
                                                          const uint32_t (*srow)[4], int rx, int ry,
                                                          int32_t gx, int32_t gy, bool trig, int N,
                                                          uint32_t rec) {
  int cxs[4], cys[4], nc = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t b = (rec >> (8 * k)) & 0xFFu;
    cxs[k] = (int)(b & 15u) - 4;
    cys[k] = (int)(b >> 4) - 4;
    nc += b != 0xFFu;
  }
  return small_verdict_pixels(drow, trow, srow, rx, ry, gx, gy, trig, N, nc, cxs, cys);
}
__device__ __forceinline__ SmallVerdict small_verdict(const uint32_t (*drow)[4],
                                                      const uint32_t (*trow)[4],
                                                      const uint32_t (*srow)[4], int rx, int ry,
                                                      int32_t gx, int32_t gy, bool trig, int N) {
  uint32_t comp[9];
  flood9(drow, rx, ry, comp);
  const uint32_t rec = pack_comp(comp);
  if (rec == kNotSmall) return SmallVerdict{trig, false};  // more than 4: not eligible
  return small_verdict_rec(drow, trow, srow, rx, ry, gx, gy, trig, N, rec);
}

constexpr int kListCap = 1024;  // LDS work list of one tile (else: row loops)

#ifndef UPH_CLASSIFY_OCC
#define UPH_CLASSIFY_OCC 8
#endif
template <int FMT>
__global__ void __launch_bounds__(256, UPH_CLASSIFY_OCC) k_noise_classify(PlaneRef img, NoiseGeom g, uint8_t* scratch,
                                                        int64_t sstride, SheetCtl* ctl) {
  static_assert(FMT != F_GRAY8, "GRAY8 classifies its bit-plane: k_noise_cand, k_noise_verdict");
  // XCD-aware tile order: neighbouring tiles' halos are fetched into one L2
  int bxi, byi, s;
  xcd_block(&bxi, &byi, &s);
  constexpr int NTX = kNT;                   // tile width
  constexpr int RWX = NTX + 2 * kHalo;       // region columns (<= 128)
  static_assert(RWX > 64 && RWX <= 128, "region rows are two 64-bit halves");
  const int32_t tx0 = bxi * NTX, ty0 = byi * kNT;
  const int32_t ox = tx0 - kHalo, oy = ty0 - kHalo;  // region origin
  const uint8_t* base = plane_ptr(img, s);
  NoisePtrs NP = noise_ptrs(g, scratch + s * sstride);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  // Everything is kept as 128-bit region rows (bit = region column):
  //   drow dark (lightness < white), trow trigger (max < white; the same
  //   bits for Y400A), srow small (component <= 4 pixels)
  constexpr bool kSplit = FMT == F_RGB24;
  // interior columns [kHalo, kHalo + NTX) of a region row's halves
  constexpr uint64_t kIn0 = ~0ull << kHalo;
  constexpr uint64_t kIn1 = (1ull << (kHalo + NTX - 64)) - 1ull;
  __shared__ uint32_t drow[kRW][4];
  __shared__ uint32_t trow_s[kSplit ? kRW : 1][4];
  __shared__ uint32_t srow[kRW][4];
  __shared__ uint64_t l3[kRW][2], cand[kRW][2];
  __shared__ uint16_t wl[kListCap];
  __shared__ uint32_t crec[kListCap];  // the candidates' components (pack_comp)
  __shared__ int32_t any_dark, nwl;
  uint32_t (*trow)[4] = kSplit ? trow_s : drow;
  constexpr int B = FMT == F_Y400A ? 2 : 3;
  const int64_t pitch = img.P.pitch;
  if (threadIdx.x == 0) {
    any_dark = 0;
    nwl = 0;
  }
  for (int i = threadIdx.x; i < kRW * 4; i += 256) (&srow[0][0])[i] = 0;
  {
    // Stage the region rows into LDS with 16-byte loads, all issued before
    // any is consumed.  Rows start 256-byte aligned, so every vector lies
    // inside its row's pitch; out-of-image pixels are masked below.
    constexpr int NV = (RWX * B + 30) / 16;             // vectors per region row
    constexpr int NLOAD = (kRW * NV + 255) / 256;       // loads per thread
    __shared__ uint4 stage[kRW][NV];
    const int64_t sb = (int64_t)ox * B;
    const int64_t a0 = sb >= 0 ? (sb & ~(int64_t)15) : -((-sb + 15) & ~(int64_t)15);
    uint4 v[NLOAD];
#pragma unroll
    for (int k = 0; k < NLOAD; k++) {
      const int i = threadIdx.x + k * 256;
      const int ry = i / NV, vi = i % NV;
      const int32_t gy = oy + ry;
      const int64_t off = a0 + 16 * vi;
      v[k] = make_uint4(0, 0, 0, 0);
      if (i < kRW * NV && gy >= 0 && gy < g.H && off >= 0 && off < pitch)
        v[k] = *reinterpret_cast<const uint4*>(base + (int64_t)gy * pitch + off);
    }
#pragma unroll
    for (int k = 0; k < NLOAD; k++) {
      const int i = threadIdx.x + k * 256;
      if (i < kRW * NV) stage[i / NV][i % NV] = v[k];
    }
    __syncthreads();
    // dark / trigger bit rows: wave w takes rows w, w+4, ...; lanes own
    // columns lane and 64+lane, each row mask is two ballots
    const int lead = (int)(sb - a0);
    bool colok[2];
    int rxc[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int rx = h * 64 + lane;
      colok[h] = (rx < RWX) & (ox + rx >= 0) & (ox + rx < g.W);
      rxc[h] = rx < RWX ? rx : 0;
    }
    bool tile_dark = false;
    for (int ry = w; ry < kRW; ry += 4) {
      const int32_t gy = oy + ry;
      const bool rowok = (gy >= 0) & (gy < g.H);
      const uint8_t* srow_b = reinterpret_cast<const uint8_t*>(stage[ry]) + lead;
      unsigned long long md[2], mt[2];
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const bool in = colok[h] & rowok;
        if constexpr (kSplit) {
          const Px p = load_px_row<FMT>(srow_b, rxc[h]);
          md[h] = __ballot(in & (light_of(p) < g.white));
          mt[h] = __ballot(in & (dark_of(p) < g.white));
        } else {  // one channel: lightness = darkness = the gray byte
          const uint32_t v = srow_b[rxc[h] * B];
          md[h] = mt[h] = __ballot(in & (v < (uint32_t)g.white));
        }
      }
      if (lane < 4) {
        const unsigned long long q = md[lane >> 1];
        drow[ry][lane] = (uint32_t)(lane & 1 ? q >> 32 : q);
        if (kSplit) {
          const unsigned long long t = mt[lane >> 1];
          trow[ry][lane] = (uint32_t)(lane & 1 ? t >> 32 : t);
        }
      }
      if (ry >= kHalo && ry < kHalo + kNT && ((md[0] & kIn0) | (md[1] & kIn1))) tile_dark = true;
    }
    if (lane == 0 && tile_dark) any_dark = 1;
  }
  __syncthreads();
  if (!any_dark) return;
  if (UPH_DIAG_BITS(g.diag, 3) == 1) return;
  // Pixels provably in a component of >= 5 pixels: L3 = dark pixels with >= 5
  // dark pixels in their 3x3 block (all 8-adjacent to the centre, so one
  // component); large = dark & (L3 | 8-dilation of L3) (8-adjacent to an L3
  // pixel = same component).  Only the remaining dark pixels ("candidates")
  // need the restricted 9x9 flood.  Rows outside the region read as empty,
  // which can only leave pixels undecided, never mislabel them.  One thread
  // per (row, 64-bit half).
  const int hr = threadIdx.x >> 1, hh = threadIdx.x & 1;
  auto dark64 = [&](int r, int h) -> uint64_t {
    return ((uint64_t)drow[r][2 * h + 1] << 32) | drow[r][2 * h];
  };
  if (threadIdx.x < 2 * kRW) {
    uint64_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
    for (int d = -1; d <= 1; d++) {
      const int r = hr + d;
      uint64_t v0 = 0, v1 = 0;
      if (r >= 0 && r < kRW) {
        v0 = dark64(r, 0);
        v1 = dark64(r, 1);
      }
      // left neighbour of column x is bit x-1 (shift up), right is x+1 (down)
      const uint64_t v = hh ? v1 : v0;
      const uint64_t Lw = hh ? (v1 << 1) | (v0 >> 63) : v0 << 1;
      const uint64_t Rw = hh ? v1 >> 1 : (v0 >> 1) | (v1 << 63);
      const uint64_t s0 = v ^ Lw ^ Rw;                          // bit 0
      const uint64_t s1 = (v & Lw) | (v & Rw) | (Lw & Rw);      // bit 1
      // c += s (c: 4 bits, <= 9; s: 2 bits)
      const uint64_t k0 = c0 & s0;
      c0 ^= s0;
      const uint64_t t1 = c1 ^ s1;
      const uint64_t k1 = (c1 & s1) | (t1 & k0);
      c1 = t1 ^ k0;
      const uint64_t k2 = c2 & k1;
      c2 ^= k1;
      c3 |= k2;
    }
    l3[hr][hh] = dark64(hr, hh) & (c3 | (c2 & (c1 | c0)));  // count >= 5: 8 | (4 & (2 | 1))
  }
  __syncthreads();
  // candidates within radius 10 of the tile (region rows [4, kRW - 4),
  // columns [4, RWX - 4)), appended to the tile's work list as
  // (row << 8 | column)
  if (threadIdx.x < 2 * kRW) {
    uint64_t c = 0;
    if (hr >= 4 && hr < kRW - 4) {
      uint64_t dil = 0;
#pragma unroll
      for (int d = -1; d <= 1; d++) {
        const uint64_t a0 = l3[hr + d][0], a1 = l3[hr + d][1];
        dil |= hh ? a1 | (a1 << 1) | (a0 >> 63) | (a1 >> 1) : a0 | (a0 << 1) | (a0 >> 1) | (a1 << 63);
      }
      // bits 4..63 of half 0, 64..RWX-5 of half 1
      c = dark64(hr, hh) & ~dil & (hh ? (1ull << (RWX - 4 - 64)) - 1ull : ~0xFull);
    }
    cand[hr][hh] = c;
    if (c) {
      int k = atomicAdd(&nwl, __popcll(c));
      while (c) {
        const int b = __ffsll((long long)c) - 1;
        c &= c - 1;
        if (k < kListCap) wl[k] = (uint16_t)((hr << 8) | (hh * 64 + b));
        k++;
      }
    }
  }
  __syncthreads();
  if (UPH_DIAG_BITS(g.diag, 3) == 2) return;
  // small bit rows: the restricted flood of every candidate
  const int ncand = nwl;
  if (ncand <= kListCap) {
    for (int i = threadIdx.x; i < ncand; i += 256) {
      const int e = wl[i], ry = e >> 8, rx = e & 0xFF;
      uint32_t comp[9];
      const bool small = flood9(drow, rx, ry, comp) <= 4;
      crec[i] = small ? pack_comp(comp) : kNotSmall;
      if (small) atomicOr(&srow[ry][rx >> 5], 1u << (rx & 31));
    }
  } else {
    for (int ry = w; ry < kRW; ry += 4) {
      unsigned long long m[2] = {0, 0};
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const uint64_t c = cand[ry][h];
        if (!c) continue;  // uniform
        bool small = false;
        if ((c >> lane) & 1) {
          uint32_t comp[9];
          small = flood9(drow, h * 64 + lane, ry, comp) <= 4;
        }
        m[h] = __ballot(small);
      }
      if (lane < 4) {
        const unsigned long long q = m[lane >> 1];
        srow[ry][lane] = (uint32_t)(lane & 1 ? q >> 32 : q);
      }
    }
  }
  __syncthreads();
  if (UPH_DIAG_BITS(g.diag, 3) == 3) return;
  const int N = g.intensity;
  const bool zone_tile = g.all_seq || tx0 < kZone || ty0 < kZone;  // uniform
  if (zone_tile) {
    // edge zone (and intensity > 4): every trigger there is replayed in
    // order; the tile's rows, one wave per row, lanes on the tile's columns
    for (int t = w; t < kNT; t += 4) {
#pragma unroll 1
      for (int h = 0; h < (NTX + 63) / 64; h++) {
        const int ry = kHalo + t, cx = h * 64 + lane, rx = kHalo + (cx < NTX ? cx : 0);
        const int32_t gy = oy + ry, gx = ox + rx;
        const bool trig = (trow[ry][rx >> 5] >> (rx & 31)) & 1;
        const bool zone = g.all_seq || gx < kZone || gy < kZone;
        const bool dark = (drow[ry][rx >> 5] >> (rx & 31)) & 1;
        // A trigger with >= 5 dark pixels in its 3x3 block, all outside the
        // strip the quirk triggers can bite (x < 2N-1 or y < 2N-2, N <= 4),
        // never clears: that block is connected and larger than N, so no
        // clear ever removes a pixel of it (away from the strip a clear
        // removes whole components of <= N pixels, see above), and its >= 4
        // dark ring-1 pixels keep the trigger's count above N.  Such triggers
        // are left out of the sequence (a dark border's interior).
        const bool noop = !g.all_seq && gx >= 8 && gy >= 7 && ((l3[ry][rx >> 6] >> (rx & 63)) & 1);
        wave_append(cx < NTX && dark & zone & trig & !noop, gx, gy, NP.nseq, NP.seq, g.capacity);
      }
    }
  }
  // small pixels of the tile outside the zone: one lane each, their
  // components kept from the candidate pass (the candidates hold every small
  // pixel: a pixel of a component of <= 4 has < 5 dark pixels in its 3x3 and
  // no large neighbour)
  if (ncand <= kListCap) {
    for (int b0 = 0; b0 < ncand; b0 += 256) {  // uniform trip count
      const int i = b0 + threadIdx.x;
      SmallVerdict v{false, false};
      int32_t gx = 0, gy = 0;
      if (i < ncand) {
        const uint32_t rec = crec[i];
        const int e = wl[i], ry = e >> 8, rx = e & 0xFF;
        gx = ox + rx;
        gy = oy + ry;
        const bool inside = ry >= kHalo && ry < kHalo + kNT && rx >= kHalo && rx < kHalo + NTX;
        if (rec != kNotSmall && inside && !g.all_seq && gx >= kZone && gy >= kZone) {
          const bool trig = (trow[ry][rx >> 5] >> (rx & 31)) & 1;
          v = small_verdict_rec(drow, trow, srow, rx, ry, gx, gy, trig, N, rec);
        }
      }
      wave_append(v.seq, gx, gy, NP.nseq, NP.seq, g.capacity);
      wave_append(v.clear, gx, gy, NP.nclear, NP.clear, g.capacity);
    }
    return;
  }
  // small pixels of the tile outside the zone: one lane each
  if (threadIdx.x == 0) nwl = 0;
  __syncthreads();
  // (row, 32-column chunk) per thread: 2 or 4 chunks a row
  constexpr int kChunks = (NTX + 31) / 32;
  static_assert(kChunks * kNT <= 256, "one thread per chunk");
  if (threadIdx.x < kChunks * kNT) {
    const int ry = kHalo + (threadIdx.x / kChunks), h = threadIdx.x % kChunks;
    uint32_t m = row_bits(srow[ry], kHalo + 32 * h, imin(32, NTX - 32 * h));
    if (m && !g.all_seq && oy + ry >= kZone) {
      const int32_t gx0 = ox + kHalo + 32 * h;  // column of bit 0
      if (gx0 < kZone) m &= kZone - gx0 >= 32 ? 0u : ~((1u << (kZone - gx0)) - 1u);
      if (m) {
        int k = atomicAdd(&nwl, __popc(m));
        while (m) {
          const int b = __ffs(m) - 1;
          m &= m - 1;
          if (k < kListCap) wl[k] = (uint16_t)((ry << 8) | (kHalo + 32 * h + b));
          k++;
        }
      }
    }
  }
  __syncthreads();
  const int nsmall = nwl;
  if (nsmall <= kListCap) {
    for (int b0 = 0; b0 < nsmall; b0 += 256) {  // uniform trip count
      const int i = b0 + threadIdx.x;
      SmallVerdict v{false, false};
      int32_t gx = 0, gy = 0;
      if (i < nsmall) {
        const int e = wl[i], ry = e >> 8, rx = e & 0xFF;
        gx = ox + rx;
        gy = oy + ry;
        const bool trig = (trow[ry][rx >> 5] >> (rx & 31)) & 1;
        v = small_verdict(drow, trow, srow, rx, ry, gx, gy, trig, N);
      }
      wave_append(v.seq, gx, gy, NP.nseq, NP.seq, g.capacity);
      wave_append(v.clear, gx, gy, NP.nclear, NP.clear, g.capacity);
    }
  } else {
    for (int t = w; t < kNT; t += 4) {
      const int ry = kHalo + t;
      uint32_t any = 0;
#pragma unroll
      for (int h = 0; h < kChunks; h++) any |= row_bits(srow[ry], kHalo + 32 * h, imin(32, NTX - 32 * h));
      if (!any) continue;  // uniform
#pragma unroll 1
      for (int h = 0; h < (NTX + 63) / 64; h++) {
        const int cx = h * 64 + lane, rx = kHalo + (cx < NTX ? cx : 0);
        const int32_t gy = oy + ry, gx = ox + rx;
        const bool zone = g.all_seq || gx < kZone || gy < kZone;
        const bool small = cx < NTX && !zone && ((srow[ry][rx >> 5] >> (rx & 31)) & 1);
        SmallVerdict v{false, false};
        if (small) {
          const bool trig = (trow[ry][rx >> 5] >> (rx & 31)) & 1;
          v = small_verdict(drow, trow, srow, rx, ry, gx, gy, trig, N);
        }
        wave_append(v.seq, gx, gy, NP.nseq, NP.seq, g.capacity);
        wave_append(v.clear, gx, gy, NP.nclear, NP.clear, g.capacity);
      }
    }
  }
}

// =========================================================================
// GRAY8 (intensity <= 4 and all_seq alike): the classification as two passes
// over bit-planes instead of tiles.  Every operator of noise_planes.h is
// local on the dark bit-plane and reads the true plane (np_word: 0 outside
// the image, and 0 for a word index outside [0, nwr), never the next row's
// word), so there is no region whose edge could leave a pixel undecided and
// the lists hold exactly the tile kernel's sets: the zone pixels, and for
// every small pixel outside the zone small_verdict_pixels's verdict.
//   k_noise_cand     a thread takes kPRA rows of one word column (np_strip):
//                    l3, candidates and zone pixels at full waves with no
//                    halo; the block's candidate and zone bits are compacted
//                    into an LDS list (drained in rounds of kPList, so any
//                    density works with no capacity of its own), one flood
//                    or one seq entry a lane; every word of the small plane
//                    is then written once by its owner
//   k_noise_verdict  the same mapping over the complete small plane: the
//                    small pixels at x, y >= 32 compacted likewise, one
//                    np_verdict a lane
// The lists only fail where they did: past g.capacity (k_noise_apply,
// k_noise_group).
// =========================================================================
// rows a thread (4, 8, 16, 32 measured: within 10 % of each other, both
// kernels are bound by the scattered box reads, not by their blocks)
constexpr int kPRA = 16;            // k_noise_cand
constexpr int kPRB = 16;            // k_noise_verdict
constexpr int kPList = 1024;        // LDS list entries a round
// entry: bit | thread << 5 | row << 13 | kind << 18
constexpr uint32_t kPZone = 1u << 18;

struct PlaneThread {
  int32_t wi, y0;  // word column, first row; y0 >= H: no words
};
// thread t of the sheet's flattened (strip, word) grid; t / nwr from the
// float reciprocal, corrected by one either way
template <int R>
__device__ __forceinline__ PlaneThread plane_thread(int32_t t, int32_t nwr, float rnwr) {
  int32_t q = (int32_t)((float)t * rnwr);
  if (q * nwr > t) q--;
  else if ((q + 1) * nwr <= t) q++;
  return PlaneThread{t - q * nwr, q * R};
}

// Appends the set bits of m (row r of this thread) to the block's list while
// it has room; returns the bits left for the next round.
__device__ __forceinline__ uint32_t list_append(uint32_t m, int r, uint32_t kind, int32_t* nwl,
                                                uint32_t* wl) {
  if (!m) return 0u;
  int k = atomicAdd(nwl, __popc(m));
  while (m && k < kPList) {
    const int b = __ffs(m) - 1;
    m &= m - 1;
    wl[k++] = (uint32_t)b | (threadIdx.x << 5) | ((uint32_t)r << 13) | kind;
  }
  return m;
}

__global__ void __launch_bounds__(256) k_noise_cand(NoiseGeom g, uint8_t* scratch, int64_t sstride,
                                                    const uint32_t* bits, int64_t bstride,
                                                    uint32_t* small, int64_t small_stride,
                                                    int32_t nwr, float rnwr) {
  const int s = blockIdx.y;
  const NpPlane P{bits + s * bstride, nwr, g.H};
  NoisePtrs NP = noise_ptrs(g, scratch + s * sstride);
  const int32_t t0 = blockIdx.x * 256;
  const PlaneThread me = plane_thread<kPRA>(t0 + threadIdx.x, nwr, rnwr);
  __shared__ uint32_t smallw[kPRA][256];
  __shared__ uint32_t wl[kPList];
  __shared__ int32_t nwl;
  uint32_t cand[kPRA], zone[kPRA];
  {
    uint32_t l3[kPRA];
    if (me.y0 < g.H) {
      np_strip<kPRA>(P, me.wi, me.y0, g.all_seq, l3, cand, zone);
    } else {
#pragma unroll
      for (int r = 0; r < kPRA; r++) cand[r] = zone[r] = 0u;
    }
  }
#pragma unroll
  for (int r = 0; r < kPRA; r++) {
    smallw[r][threadIdx.x] = 0u;
    if (g.all_seq) cand[r] = 0u;  // nothing is judged
  }
  for (;;) {
    if (threadIdx.x == 0) nwl = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kPRA; r++) {
      cand[r] = list_append(cand[r], r, 0u, &nwl, wl);
      zone[r] = list_append(zone[r], r, kPZone, &nwl, wl);
    }
    __syncthreads();
    const int tot = nwl, n = imin(tot, kPList);
    for (int b0 = 0; b0 < n; b0 += 256) {  // uniform trip count
      const int i = b0 + threadIdx.x;
      bool seq = false;
      int32_t gx = 0, gy = 0;
      if (i < n) {
        const uint32_t e = wl[i];
        const int et = (e >> 5) & 255, r = (e >> 13) & 31;
        const PlaneThread o = plane_thread<kPRA>(t0 + et, nwr, rnwr);
        gx = 32 * o.wi + (int32_t)(e & 31u);
        gy = o.y0 + r;
        seq = e & kPZone;
        if (!seq) {
          uint32_t comp[9], D[9];
          if (np_flood9(P, gx, gy, comp, D) <= kNpSmallMax) atomicOr(&smallw[r][et], 1u << (e & 31u));
        }
      }
      wave_append(seq, gx, gy, NP.nseq, NP.seq, g.capacity);
    }
    __syncthreads();  // the floods' bits landed; nwl may be reset
    if (tot <= kPList) break;
  }
  if (g.all_seq || me.y0 >= g.H) return;
  uint32_t* out = small + s * small_stride + (int64_t)me.y0 * nwr + me.wi;
#pragma unroll
  for (int r = 0; r < kPRA; r++)
    if (me.y0 + r < g.H) out[(int64_t)r * nwr] = smallw[r][threadIdx.x];
}

__global__ void __launch_bounds__(256) k_noise_verdict(NoiseGeom g, uint8_t* scratch,
                                                       int64_t sstride, const uint32_t* bits,
                                                       int64_t bstride, const uint32_t* small,
                                                       int64_t small_stride, int32_t nwr,
                                                       float rnwr) {
  const int s = blockIdx.y;
  const NpPlane P{bits + s * bstride, nwr, g.H};
  const NpPlane S{small + s * small_stride, nwr, g.H};
  NoisePtrs NP = noise_ptrs(g, scratch + s * sstride);
  const int32_t t0 = blockIdx.x * 256;
  const PlaneThread me = plane_thread<kPRB>(t0 + threadIdx.x, nwr, rnwr);
  __shared__ uint32_t wl[kPList];
  __shared__ int32_t nwl;
  uint32_t todo[kPRB];  // the thread's small pixels outside the zone
#pragma unroll
  for (int r = 0; r < kPRB; r++) {
    const int32_t y = me.y0 + r;
    todo[r] = me.wi > 0 && y >= kNpZone && y < g.H ? S.w[(int64_t)y * nwr + me.wi] : 0u;
  }
  for (;;) {
    if (threadIdx.x == 0) nwl = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kPRB; r++) todo[r] = list_append(todo[r], r, 0u, &nwl, wl);
    __syncthreads();
    const int tot = nwl, n = imin(tot, kPList);
    for (int b0 = 0; b0 < n; b0 += 256) {  // uniform trip count
      const int i = b0 + threadIdx.x;
      int v = NP_NONE;
      int32_t gx = 0, gy = 0;
      if (i < n) {
        const uint32_t e = wl[i];
        const PlaneThread o = plane_thread<kPRB>(t0 + (int)((e >> 5) & 255), nwr, rnwr);
        gx = 32 * o.wi + (int32_t)(e & 31u);
        gy = o.y0 + (int)((e >> 13) & 31);
        v = np_verdict(P, S, gx, gy, g.intensity);
      }
      wave_append2(v == NP_SEQ, v == NP_CLEAR, gx, gy, NP.nseq, NP.seq, NP.nclear, NP.clear,
                   g.capacity);
    }
    __syncthreads();  // nwl may be reset
    if (tot <= kPList) break;
  }
}

template <int FMT>
__device__ __forceinline__ uint32_t* sheet_bb(const NoiseGeom& g, int s) {
  return FMT == F_GRAY8 && g.bbits ? g.bbits + s * g.bb_stride : nullptr;
}
__device__ __forceinline__ void bb_clear(uint32_t* bb, int32_t W, int32_t x, int32_t y) {
  if (bb) atomicAnd(bb + (int64_t)y * ((W + 31) >> 5) + (x >> 5), ~(1u << (x & 31)));
}

template <int FMT>
__global__ void __launch_bounds__(256) k_noise_apply(PlaneRef img, NoiseGeom g, uint8_t* scratch,
                                                     int64_t sstride, SheetCtl* ctl) {
  const int s = blockIdx.y;
  NoisePtrs NP = noise_ptrs(g, scratch + s * sstride);
  const uint32_t n = *NP.nclear;
  if (n > (uint32_t)g.capacity) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && ctl) atomicOr(&ctl[s].status, STATUS_NOISE_OVERFLOW);
    return;
  }
  uint8_t* base = plane_ptr(img, s);
  uint32_t* bb = sheet_bb<FMT>(g, s);
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const uint32_t k = NP.clear[i];
    white_px<FMT>(base + (int64_t)(k >> 16) * img.P.pitch, (int32_t)(k & 0xFFFF));
    bb_clear(bb, g.W, (int32_t)(k & 0xFFFF), (int32_t)(k >> 16));
  }
}

// In-LDS / in-global bitonic sort of n uint32 keys by one 256-thread block.
// Bitonic sort of a[0 .. n_pow2) in LDS by the whole block (blockDim.x a
// multiple of 64).  Steps whose partners lie 64 or more apart go through LDS
// with a block barrier each; the steps below 64 of a merge run in registers
// (partners in the same wave: element i belongs to lane i % 64 of one wave),
// with one barrier per merge instead of one per step.
__device__ void block_sort(uint32_t* a, int n_pow2) {
  for (int k = 2; k <= n_pow2; k <<= 1) {
    int j = k >> 1;
    for (; j >= 64; j >>= 1) {
      for (int i = threadIdx.x; i < n_pow2; i += blockDim.x) {
        const int l = i ^ j;
        if (l > i) {
          const uint32_t x = a[i], y = a[l];
          const bool up = (i & k) == 0;
          if ((x > y) == up) {
            a[i] = y;
            a[l] = x;
          }
        }
      }
      __threadfence_block();
      __syncthreads();
    }
    for (int i = threadIdx.x; i < n_pow2; i += blockDim.x) {
      uint32_t x = a[i];
      const bool up = (i & k) == 0;
      for (int jj = j; jj > 0; jj >>= 1) {
        const uint32_t y = (uint32_t)__shfl_xor((int)x, jj, 64);
        const bool lower = (i & jj) == 0;  // keeps the smaller one when sorting up
        x = lower == up ? (x < y ? x : y) : (x < y ? y : x);
      }
      a[i] = x;
    }
    __threadfence_block();
    __syncthreads();
  }
}

// Pixel k of the Chebyshev ring L (8L pixels): the two rows dy = -L, +L
// (2L+1 each), then the two columns dx = -L, +L without the corners.
__device__ __forceinline__ bool ring_pos(int L, int k, int* dx, int* dy) {
  const int row = 2 * L + 1, col = 2 * L - 1;
  if (k < row) {
    *dx = k - L;
    *dy = -L;
  } else if (k < 2 * row) {
    *dx = k - row - L;
    *dy = L;
  } else if (k < 2 * row + col) {
    *dx = -L;
    *dy = k - 2 * row - (L - 1);
  } else if (k < 2 * row + 2 * col) {
    *dx = L;
    *dy = k - 2 * row - col - (L - 1);
  } else {
    return false;
  }
  return true;
}

// Whether the reference ring loops visit (x+dx, y+dy) at level L.
__device__ __forceinline__ bool ring_member(int L, int dx, int dy, int32_t x, int32_t y) {
  return iabs(dy) == L ? x >= L : y >= L - 1;
}

// 81-bit position masks of the 9x9 window (bit p = (dy+4)*9 + dx+4): for
// ring L, its two rows (|dy| = L) and its two columns without the corners.
struct Mask81 {
  uint64_t lo;
  uint32_t hi;
};
__device__ __forceinline__ Mask81 ring_part(int L, bool rows) {
  Mask81 m{0, 0};
#pragma unroll
  for (int p = 0; p < 81; p++) {
    const int dx = p % 9 - 4, dy = p / 9 - 4;
    const int adx = iabs(dx), ady = iabs(dy);
    const bool on = rows ? (ady == L && adx <= L) : (adx == L && ady < L);
    if (on) {
      if (p < 64) m.lo |= 1ull << p;
      else m.hi |= 1u << (p - 64);
    }
  }
  return m;
}

// The blurfilter's GRAY8 bit-plane (pixel <= white, NoiseGeom::bbits) follows
// a clear: the sheet's plane `bb` (null: none), bit x of row y.
// One trigger of the raster replay for intensity N <= 4 (filters.c:309-338):
// the 9x9 window read from the frame (dark = lightness < white), rings with
// the reference loops' unsigned comparisons -- rows of ring L counted iff
// x >= L, its columns iff y >= L-1 -- and the clears written straight back.
template <int FMT>
__device__ __forceinline__ void replay_trigger4(int32_t x, int32_t y, int N, const NoiseGeom& g,
                                                uint8_t* base, int64_t pitch,
                                                const Mask81 (&rowp)[5], const Mask81 (&colp)[5],
                                                uint32_t* bb) {
  uint64_t dlo = 0;
  uint32_t dhi = 0;
  bool ctr = false;
  if constexpr (FMT == F_GRAY8) {
    // a box row as three aligned dwords (rows are pitched in whole dwords,
    // so clamped addresses stay inside the row): 27 loads instead of 81
    const int32_t c0 = x - 4;
    const int32_t d0 = c0 >= 0 ? (c0 & ~3) : -(((-c0) + 3) & ~3);  // floor to a multiple of 4
    const int32_t dmax = (int32_t)pitch - 4;
    uint32_t w[9][3];
#pragma unroll
    for (int r = 0; r < 9; r++) {
      const uint8_t* row = base + (int64_t)imin(imax(y + r - 4, 0), g.H - 1) * pitch;
#pragma unroll
      for (int j = 0; j < 3; j++)
        w[r][j] = *reinterpret_cast<const uint32_t*>(row + imin(imax(d0 + 4 * j, 0), dmax));
    }
    const int o = c0 - d0;  // 0 .. 3
#pragma unroll
    for (int p = 0; p < 81; p++) {
      const int r = p / 9, c = p % 9;
      const int32_t qx = c0 + c, qy = y + r - 4;
      const bool in = (qx >= 0) & (qy >= 0) & (qx < g.W) & (qy < g.H);
      const int b = o + c;  // byte of the row's 12
      const uint32_t wd = b < 4 ? w[r][0] : b < 8 ? w[r][1] : w[r][2];
      const uint32_t v = (wd >> (8 * (b & 3))) & 0xFFu;
      const bool dk = in & (v < g.white);
      if (p < 64) dlo |= (uint64_t)dk << p;
      else dhi |= (uint32_t)dk << (p - 64);
      if (p == 40) ctr = v < g.white;
    }
  } else if constexpr (FMT == F_RGB24) {
    // a box row (27 bytes) as eight aligned dwords, realigned to its first
    // byte: 72 loads instead of 243
    const int32_t b0 = 3 * (x - 4);
    const int32_t d0 = b0 >= 0 ? (b0 & ~3) : -(((-b0) + 3) & ~3);
    const int32_t dmax = (int32_t)pitch - 4;
    const int o = b0 - d0;  // 0 .. 3
#pragma unroll
    for (int r = 0; r < 9; r++) {
      const uint8_t* row = base + (int64_t)imin(imax(y + r - 4, 0), g.H - 1) * pitch;
      uint32_t w[8], a[7];
#pragma unroll
      for (int j = 0; j < 8; j++)
        w[j] = *reinterpret_cast<const uint32_t*>(row + imin(imax(d0 + 4 * j, 0), dmax));
#pragma unroll
      for (int j = 0; j < 7; j++) a[j] = __builtin_amdgcn_alignbyte(w[j + 1], w[j], o);
#pragma unroll
      for (int c = 0; c < 9; c++) {
        const int p = 9 * r + c;
        const int32_t qx = x + c - 4, qy = y + r - 4;
        const bool in = (qx >= 0) & (qy >= 0) & (qx < g.W) & (qy < g.H);
        const int k = 3 * c;  // the pixel's first byte in the realigned row
        const Px q{(uint8_t)(a[k >> 2] >> (8 * (k & 3))), (uint8_t)(a[(k + 1) >> 2] >> (8 * ((k + 1) & 3))),
                   (uint8_t)(a[(k + 2) >> 2] >> (8 * ((k + 2) & 3)))};
        const bool dk = in & (light_of(q) < g.white);
        if (p < 64) dlo |= (uint64_t)dk << p;
        else dhi |= (uint32_t)dk << (p - 64);
        if (p == 40) ctr = dark_of(q) < g.white;
      }
    }
  } else {
#pragma unroll
    for (int p = 0; p < 81; p++) {  // unconditional clamped loads: one round trip
      const int32_t qx = x + p % 9 - 4, qy = y + p / 9 - 4;
      const bool in = (qx >= 0) & (qy >= 0) & (qx < g.W) & (qy < g.H);
      const Px q = load_px_row<FMT>(base + (int64_t)imin(imax(qy, 0), g.H - 1) * pitch,
                                    imin(imax(qx, 0), g.W - 1));
      const bool dk = in & (light_of(q) < g.white);
      if (p < 64) dlo |= (uint64_t)dk << p;
      else dhi |= (uint32_t)dk << (p - 64);
      if (p == 40) ctr = dark_of(q) < g.white;
    }
  }
  if (!ctr) return;  // cleared meanwhile
  Mask81 mem[5];
  int lc[5];
#pragma unroll
  for (int L = 1; L <= 4; L++) {
    mem[L].lo = (x >= L ? rowp[L].lo : 0ull) | (y >= L - 1 ? colp[L].lo : 0ull);
    mem[L].hi = (x >= L ? rowp[L].hi : 0u) | (y >= L - 1 ? colp[L].hi : 0u);
    lc[L] = __popcll(dlo & mem[L].lo) + __popc(dhi & mem[L].hi);
  }
  // do { lc = ring(level); count += lc; level++ } while (lc && level <= N)
  int count = 1, k = N + 1;  // k: first empty ring (N+1: none within N)
  bool open = true;
#pragma unroll
  for (int L = 1; L <= 4; L++) {
    if (open && L <= N) {
      count += lc[L];
      if (lc[L] == 0) {
        k = L;
        open = false;
      }
    }
  }
  if (count > N) return;
  // the centre and rings 1..k-1 are cleared
  white_px<FMT>(base + (int64_t)y * pitch, x);
  bb_clear(bb, g.W, x, y);
#pragma unroll
  for (int Lc = 1; Lc <= 3; Lc++) {
    if (Lc >= k) continue;
    uint64_t clo = dlo & mem[Lc].lo;
    uint32_t chi = dhi & mem[Lc].hi;
    while (clo) {
      const int p = __ffsll((long long)clo) - 1;
      clo &= clo - 1;
      white_px<FMT>(base + (int64_t)(y + p / 9 - 4) * pitch, x + p % 9 - 4);
      bb_clear(bb, g.W, x + p % 9 - 4, y + p / 9 - 4);
    }
    while (chi) {
      const int p = 64 + __ffs(chi) - 1;
      chi &= chi - 1;
      white_px<FMT>(base + (int64_t)(y + p / 9 - 4) * pitch, x + p % 9 - 4);
      bb_clear(bb, g.W, x + p % 9 - 4, y + p / 9 - 4);
    }
  }
}

// Parallel union-find over the trigger indices (parents always point to a
// smaller index, so the CAS links never form a cycle).  GLOBAL: the parents
// live in HBM and are read past the vector L1 (agent-scope atomic loads), so
// a link another wave's CAS made in L2 is seen on the next read.
template <bool GLOBAL = false>
__device__ __forceinline__ uint32_t uf_load(const uint32_t* parent, uint32_t i) {
  if constexpr (GLOBAL)
    return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else
    return parent[i];
}
template <bool GLOBAL = false>
__device__ __forceinline__ uint32_t uf_find(const uint32_t* parent, uint32_t i) {
  uint32_t p = uf_load<GLOBAL>(parent, i);
  while (p != i) {
    i = p;
    p = uf_load<GLOBAL>(parent, i);
  }
  return i;
}
template <bool GLOBAL = false>
__device__ __forceinline__ void uf_union(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = uf_find<GLOBAL>(parent, a);
    b = uf_find<GLOBAL>(parent, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    if (atomicCAS(&parent[a], a, b) == a) return;
  }
}

// k_noise_group is one 256-thread block a sheet with ~49 KiB of LDS: a block
// that needs a whole CU's wave slots and LDS (1024 threads, 147 KiB, round
// 5) waits for a CU to drain while other streams' kernels keep them busy
// (84 ms a launch in the JPEG 2000 runner, behind the code-block decode).
// k_noise_replay blocks per sheet: enough that a lone sheet's components
// spread over the chip (C2/C4 latency: up to 16384 threads a sheet), few
// enough that a 64-sheet batch is not mostly blocks that exit (C3): about one
// block a CU over the launch, clamped to [4, 64].
static int replay_blocks(int count) {
  const int per = (256 + count - 1) / (count > 0 ? count : 1);
  return per < 4 ? 4 : per > 64 ? 64 : per;
}

// The sequential part of the noisefilter (the triggers k_noise_classify could
// not decide in parallel) for intensity N <= 4, in two kernels:
// k_noise_group (a block per sheet) orders the triggers in raster order by a
// counting sort over row buckets (then insertion sort within a bucket; a
// bucket longer than kGroupBucketMax is bitonic-sorted by the whole block in
// LDS), links those within 2N-1 by union-find and writes, per trigger in
// raster order, its key, its component's root (the component's first
// trigger) and, for a root, its component's last trigger; k_noise_replay
// (many blocks per sheet) gives each component to one thread, which replays
// its triggers in raster order.  The replay's scattered box reads then spread
// over the chip instead of one CU's address path.  Where the arrays live is
// the sheet's layout word (word 2 of its list header):
//   kNoiseNothing  nothing left to replay (no trigger, or done in k_noise_group)
//   kNoiseLds      n <= kCompCap: keys / roots / last at [0, C), [C, 2C),
//                  [2C, 3C) of the sort buffer (C = kCompCap); the sort and
//                  the links ran in LDS
//   kNoiseBig      n > kCompCap: keys in the sort buffer, roots in the seq
//                  list (free once its keys are scattered), last in the clear
//                  list (free once k_noise_apply ran); the sort and the links
//                  ran on those global arrays
// Intensity > 4 (every trigger replayed: up to W*H of them) and a bucket of
// more than kCompCap triggers take the literal raster scan by one wave inside
// k_noise_group.  No separate resolver launch: a kernel asking for 128 KiB
// of LDS waits for a nearly idle CU even when all its blocks would exit.
constexpr uint32_t kNoiseNothing = 0, kNoiseLds = 1, kNoiseBig = 2;
constexpr int kGroupBucketMax = 256;  // longer buckets: block-wide bitonic sort
constexpr int kLongList = 64;         // long buckets remembered by id (else: all scanned)
// keys, parents, bucket starts, the scan's wave sums + 3 words, the long
// bucket list (all dynamic: allow_dynamic_lds raises the limit to 160 KiB)
constexpr size_t group_lds(int threads) {
  return sizeof(uint32_t) * (2 * (size_t)(kCapPerThread * threads) + kNoiseBuckets + 1 + 16 + 3 + kLongList);
}

// The literal raster scan of the sorted triggers by one wave (filters.c:
// 243-348): for intensity > 4 (every trigger queued) and for a sheet whose
// triggers crowd one bucket beyond what the block can sort in LDS.  keys: n
// triggers, pow2 p2 >= n slots (LDS when p2 <= kCompCap, else the sheet's
// global sort buffer).
template <int FMT>
__device__ void noise_raster_replay(uint32_t* keys, int n, int p2, const NoiseGeom& g, const NoisePtrs& NP,
                                    uint8_t* base, int64_t pitch, uint32_t* bb) {
  for (int i = threadIdx.x; i < p2; i += blockDim.x) keys[i] = i < n ? NP.seq[i] : 0xFFFFFFFFu;
  __threadfence_block();
  __syncthreads();
  block_sort(keys, p2);
  if (threadIdx.x >= 64) return;
  const int N = g.intensity;
  const int lane = threadIdx.x;
  if (N <= 4) {
    // small intensity: the whole (2N+1)^2 box of a trigger is read in one
    // round trip (two pixels per lane) and the rings are counted from
    // registers; clears are written straight back
    const int side = 2 * N + 1, area = side * side;
    for (int idx = 0; idx < n; idx++) {
      const uint32_t key = keys[idx];
      const int32_t x = (int32_t)(key & 0xFFFF), y = (int32_t)(key >> 16);
      __threadfence_block();
      int Lv[2];
      bool dk[2], ctr = false;
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int pos = h * 64 + lane;
        Lv[h] = -1;
        dk[h] = false;
        if (pos < area) {
          const int dx = pos % side - N, dy = pos / side - N;
          const int L = imax(iabs(dx), iabs(dy));
          const int32_t qx = x + dx, qy = y + dy;
          Lv[h] = L;
          const bool member = L == 0 || ring_member(L, dx, dy, x, y);
          if (member && qx >= 0 && qy >= 0 && qx < g.W && qy < g.H) {
            const Px p = load_px_row<FMT>(base + (int64_t)qy * pitch, qx);
            dk[h] = L > 0 && light_of(p) < g.white;
            if (L == 0) ctr = dark_of(p) < g.white;
          }
        }
      }
      if (!__ballot(ctr)) continue;  // cleared meanwhile
      int count = 1, level = 1, lc;
      do {
        lc = __popcll(__ballot(dk[0] && Lv[0] == level)) +
             __popcll(__ballot(dk[1] && Lv[1] == level));
        count += lc;
        level++;
      } while (lc != 0 && level <= N);
      if (count > N) continue;
      const int k = level - 1;
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int pos = h * 64 + lane;
        if (pos >= area || Lv[h] >= k || (Lv[h] > 0 && !dk[h])) continue;
        const int32_t qx = x + pos % side - N, qy = y + pos / side - N;
        white_px<FMT>(base + (int64_t)qy * pitch, qx);
        bb_clear(bb, g.W, qx, qy);
      }
    }
    return;
  }
  for (int idx = 0; idx < n; idx++) {
    const uint32_t key = keys[idx];
    const int32_t x = (int32_t)(key & 0xFFFF), y = (int32_t)(key >> 16);
    __threadfence_block();
    const Px cp = load_px_row<FMT>(base + (int64_t)y * pitch, x);
    if (!(dark_of(cp) < g.white)) continue;  // cleared meanwhile
    // ring counts with the reference loops' unsigned-comparison semantics:
    // rows +-L counted iff x >= L, columns +-L (|dy| < L) counted iff y >= L-1
    // (filters.c:243-302); ring L is walked as its 8L pixels, one per lane
    int count = 1, level = 1, lc;
    do {
      lc = 0;
      for (int b = 0; b < 8 * level; b += 64) {
        int dx, dy;
        const bool in = ring_pos(level, b + lane, &dx, &dy);
        bool dark = false;
        if (in && ring_member(level, dx, dy, x, y)) {
          const int32_t qx = x + dx, qy = y + dy;
          if (qx >= 0 && qy >= 0 && qx < g.W && qy < g.H)
            dark = light_of(load_px_row<FMT>(base + (int64_t)qy * pitch, qx)) < g.white;
        }
        lc += __popcll(__ballot(dark));
      }
      count += lc;
      level++;
    } while (lc != 0 && level <= N);
    if (count > N) continue;
    // centre + rings 1..k-1 (the loop stopped at the first empty ring k)
    const int k = level - 1;
    if (lane == 0) {
      white_px<FMT>(base + (int64_t)y * pitch, x);
      bb_clear(bb, g.W, x, y);
    }
    for (int L = 1; L < k; L++) {
      for (int b = 0; b < 8 * L; b += 64) {
        int dx, dy;
        if (!ring_pos(L, b + lane, &dx, &dy) || !ring_member(L, dx, dy, x, y)) continue;
        const int32_t qx = x + dx, qy = y + dy;
        if (qx < 0 || qy < 0 || qx >= g.W || qy >= g.H) continue;
        uint8_t* row = base + (int64_t)qy * pitch;
        if (light_of(load_px_row<FMT>(row, qx)) < g.white) {
          white_px<FMT>(row, qx);
          bb_clear(bb, g.W, qx, qy);
        }
      }
    }
    __threadfence_block();
  }
}

// k_noise_group's ordering and linking for one sheet of n (> 0) triggers;
// BIG (n > kCompCap): keys and parents in HBM, else in LDS.  A template
// parameter, so that every pointer below has one address space (LDS through
// ds_*, HBM through global_*): no flat accesses to LDS.
template <int FMT, int T, bool BIG>
__device__ __forceinline__ void noise_group_sheet(const NoiseGeom& g, const NoisePtrs& NP, uint32_t* gk,
                                                  uint32_t* glds, uint8_t* base, int64_t pitch,
                                                  uint32_t* flag, uint32_t n, uint32_t* bb) {
  const int N = g.intensity;
  const int tid = threadIdx.x;
  const bool big = BIG;
  constexpr int kCompCap = kCapPerThread * T;
  constexpr int kGroupThreads = T;
  uint32_t* keys = big ? gk : glds;         // the sorted keys
  uint32_t* cur = glds + kCompCap;          // scatter cursors, then the long-bucket stage
  uint32_t* bc = glds + 2 * kCompCap;       // bucket starts (nb + 1)
  uint32_t* wsum = bc + kNoiseBuckets + 1;
  uint32_t& nlong = wsum[16];
  uint32_t& huge = wsum[17];
  uint32_t* longs = wsum + 19;
  const int b = noise_bucket_shift(g.H);
  const int nb = ((g.H - 1) >> b) + 1;
  const int R = 2 * N - 1;
  if (tid == 0) {
    nlong = 0u;
    huge = 0u;
  }
  for (int i = tid; i <= nb; i += kGroupThreads) bc[i] = 0;
  __syncthreads();
  for (int i = tid; i < (int)n; i += kGroupThreads) {
    atomicAdd(&bc[(NP.seq[i] >> 16) >> b], 1u);
  }
  __syncthreads();
  // exclusive scan of the nb counts: KB consecutive buckets a thread
  {
    constexpr int KB = kNoiseBuckets / kGroupThreads;
    const int b0 = KB * tid;
    uint32_t c[KB], sum = 0;
#pragma unroll
    for (int k = 0; k < KB; k++) {
      c[k] = b0 + k < nb ? bc[b0 + k] : 0u;
      sum += c[k];
      if (c[k] > (uint32_t)kGroupBucketMax) {
        const uint32_t q = atomicAdd(&nlong, 1u);
        if (q < (uint32_t)kLongList) longs[q] = (uint32_t)(b0 + k);
        // staged in LDS, or (BIG) in the clear list: a bucket past that
        // (pow2 slots) takes the literal scan
        int p2 = 1;
        while (p2 < (int)c[k]) p2 <<= 1;
        if (p2 > (BIG ? g.capacity : kCompCap)) huge = 1u;
      }
    }
    // block exclusive scan of `sum`
    uint32_t incl = sum;
    const int lane = tid & 63, wv = tid >> 6;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t u = (uint32_t)__shfl_up((int)incl, o, 64);
      if (lane >= o) incl += u;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    uint32_t before = 0;
    for (int k = 0; k < wv; k++) before += wsum[k];
    uint32_t run = before + incl - sum;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KB; k++) {
      if (b0 + k < nb) {
        bc[b0 + k] = run;
        cur[b0 + k] = run;
      }
      run += c[k];
    }
    if (tid == 0) bc[nb] = n;
  }
  __syncthreads();
  if (huge) {  // one bucket beyond the LDS sort: the literal scan (never on real pages)
    int p2 = 1;
    while (p2 < (int)n) p2 <<= 1;
    if (tid == 0) *flag = kNoiseNothing;
    noise_raster_replay<FMT>(gk, (int)n, p2, g, NP, base, pitch, bb);
    return;
  }
  for (int i = tid; i < (int)n; i += kGroupThreads) {
    const uint32_t key = NP.seq[i];
    const uint32_t dst = atomicAdd(&cur[(key >> 16) >> b], 1u);
    keys[dst] = key;
  }
  __threadfence_block();
  __syncthreads();
  // raster order inside each bucket: short ones by one thread each
  for (int k = tid; k < nb; k += kGroupThreads) {
    const int lo = (int)bc[k], hi = (int)bc[k + 1];
    if (hi - lo > kGroupBucketMax) continue;
    for (int i = lo + 1; i < hi; i++) {
      const uint32_t v = keys[i];
      int j = i - 1;
      while (j >= lo && keys[j] > v) {
        keys[j + 1] = keys[j];
        j--;
      }
      keys[j + 1] = v;
    }
  }
  // long ones by the whole block, one after another, staged in LDS (BIG: in
  // the clear list when longer than the LDS stage)
  const int nl = (int)nlong;
  for (int q = 0, k = 0; nl > 0 && (nl <= kLongList ? q < nl : k < nb);) {
    const int kb = nl <= kLongList ? (int)longs[q++] : k++;  // uniform
    const int lo = (int)bc[kb], len = (int)bc[kb + 1] - lo;
    if (len <= kGroupBucketMax) continue;
    int p2 = 1;
    while (p2 < len) p2 <<= 1;
    __threadfence_block();
    __syncthreads();
    if (!BIG || p2 <= kCompCap) {
      for (int i = tid; i < p2; i += kGroupThreads) cur[i] = i < len ? keys[lo + i] : 0xFFFFFFFFu;
      __threadfence_block();
      __syncthreads();
      block_sort(cur, p2);
      for (int i = tid; i < len; i += kGroupThreads) keys[lo + i] = cur[i];
    } else {
      uint32_t* stage = NP.clear;
      for (int i = tid; i < p2; i += kGroupThreads) stage[i] = i < len ? keys[lo + i] : 0xFFFFFFFFu;
      __threadfence_block();
      __syncthreads();
      block_sort(stage, p2);
      for (int i = tid; i < len; i += kGroupThreads) keys[lo + i] = stage[i];
    }
  }
  __threadfence_block();
  __syncthreads();
  // parents: LDS, or (big) the seq list, whose keys are all scattered now
  uint32_t* par = big ? NP.seq : cur;
  for (int i = tid; i < (int)n; i += kGroupThreads) par[i] = (uint32_t)i;
  __threadfence_block();
  __syncthreads();
  // link every trigger to the earlier ones within R (rows y-R .. y)
  for (int i = tid; i < (int)n; i += kGroupThreads) {
    const uint32_t key = keys[i];
    const int32_t x = (int32_t)(key & 0xFFFF), y = (int32_t)(key >> 16);
    for (int j = (int)bc[imax(y - R, 0) >> b]; j < i; j++) {
      const uint32_t kj = keys[j];
      const int32_t xj = (int32_t)(kj & 0xFFFF), yj = (int32_t)(kj >> 16);
      if (yj >= y - R && xj >= x - R && xj <= x + R) {
        if (big) uf_union<true>(par, (uint32_t)i, (uint32_t)j);
        else uf_union(par, (uint32_t)i, (uint32_t)j);
      }
    }
  }
  __threadfence_block();
  __syncthreads();
  if (!big) {
    for (int i = tid; i < (int)n; i += kGroupThreads) {
      gk[i] = keys[i];
      gk[kCompCap + i] = uf_find(par, (uint32_t)i);
    }
    __syncthreads();
    for (int i = tid; i < (int)n; i += kGroupThreads) keys[i] = 0u;
    __syncthreads();
    for (int i = tid; i < (int)n; i += kGroupThreads) atomicMax(&keys[gk[kCompCap + i]], (uint32_t)i);
    __syncthreads();
    for (int i = tid; i < (int)n; i += kGroupThreads) gk[2 * kCompCap + i] = keys[i];
    if (tid == 0) *flag = kNoiseLds;
    return;
  }
  // big: roots flattened in place (a concurrent reader sees an old parent or
  // the root, both ancestors), last trigger per root in the clear list
  uint32_t* last = NP.clear;
  for (int i = tid; i < (int)n; i += kGroupThreads) last[i] = 0u;
  for (int i = tid; i < (int)n; i += kGroupThreads) par[i] = uf_find<true>(par, (uint32_t)i);
  __threadfence_block();
  __syncthreads();
  for (int i = tid; i < (int)n; i += kGroupThreads) atomicMax(&last[par[i]], (uint32_t)i);
  __threadfence();
  __syncthreads();
  if (tid == 0) *flag = kNoiseBig;
}

template <int FMT, int T>
__global__ void __launch_bounds__(T) k_noise_group(PlaneRef img, NoiseGeom g, uint8_t* scratch,
                                                   int64_t sstride, SheetCtl* ctl,
                                                   uint32_t* sortbuf, int64_t sort_stride) {
  constexpr int kCompCap = kCapPerThread * T;
  const int s = blockIdx.x;
  NoisePtrs NP = noise_ptrs(g, scratch + s * sstride);
  uint32_t* flag = NP.nclear + 2;
  const uint32_t n = *NP.nseq;
  const int N = g.intensity;
  const int tid = threadIdx.x;
#ifdef UPHIP_DIAG
  if ((g.diag & 8) && tid == 0) printf("uphip noise: sheet %d seq %u clear %u\n", s, n, *NP.nclear);
#endif
  if (n == 0 || n > (uint32_t)g.capacity) {
    if (tid == 0) {
      *flag = kNoiseNothing;
      if (n != 0 && ctl) atomicOr(&ctl[s].status, STATUS_NOISE_OVERFLOW);
    }
    return;
  }
  uint32_t* gk = sortbuf + s * sort_stride;
  extern __shared__ uint32_t glds[];
  uint8_t* base = plane_ptr(img, s);
  const int64_t pitch = img.P.pitch;
  uint32_t* bb = sheet_bb<FMT>(g, s);
  if (N > 4) {  // intensity > 4: every trigger, one wave in raster order
    int p2 = 1;
    while (p2 < (int)n) p2 <<= 1;
    if (tid == 0) *flag = kNoiseNothing;
    if (p2 <= kCompCap) noise_raster_replay<FMT>(glds, (int)n, p2, g, NP, base, pitch, bb);
    else noise_raster_replay<FMT>(gk, (int)n, p2, g, NP, base, pitch, bb);
    return;
  }
  if (n > (uint32_t)kCompCap)
    noise_group_sheet<FMT, T, true>(g, NP, gk, glds, base, pitch, flag, n, bb);
  else
    noise_group_sheet<FMT, T, false>(g, NP, gk, glds, base, pitch, flag, n, bb);
}

// No waves-per-SIMD hint (A/B: a budget of 6 waves 131 -> 144 us a C3 launch,
// C4 noisefilter 0.82 -> 0.88 ms; 8 waves worse).
template <int FMT>
__global__ void __launch_bounds__(256) k_noise_replay(PlaneRef img, NoiseGeom g, uint8_t* scratch,
                                                      int64_t sstride, const uint32_t* sortbuf,
                                                      int64_t sort_stride, int kCompCap) {
  const int s = blockIdx.y;
  NoisePtrs NP = noise_ptrs(g, scratch + s * sstride);
  const uint32_t n = *NP.nseq;
  const uint32_t layout = NP.nclear[2];
  if (layout == kNoiseNothing || blockIdx.x * blockDim.x >= n) return;
  const uint32_t* keys = sortbuf + s * sort_stride;
  const uint32_t* root = layout == kNoiseLds ? keys + kCompCap : NP.seq;
  const uint32_t* last = layout == kNoiseLds ? keys + 2 * kCompCap : NP.clear;
  Mask81 rowp[5], colp[5];
#pragma unroll
  for (int L = 1; L <= 4; L++) {
    rowp[L] = ring_part(L, true);
    colp[L] = ring_part(L, false);
  }
  uint8_t* base = plane_ptr(img, s);
  uint32_t* bb = sheet_bb<FMT>(g, s);
  // a few blocks per sheet walk its triggers (sheets hold far fewer triggers
  // than kCompCap: a grid sized for the cap was mostly blocks that exit)
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < (int)n; i += gridDim.x * blockDim.x) {
    if (root[i] != (uint32_t)i) continue;  // not a component's first trigger
    const int end = (int)last[i];
    for (int j = i; j <= end; j++) {
      if (root[j] != (uint32_t)i) continue;
      const uint32_t key = keys[j];
      __threadfence_block();  // this thread's earlier clears are visible to its loads
      replay_trigger4<FMT>((int32_t)(key & 0xFFFF), (int32_t)(key >> 16), g.intensity, g, base,
                           img.P.pitch, rowp, colp, bb);
    }
  }
}

__global__ void k_noise_zero(uint8_t* scr, int64_t stride, int count) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < count) {
    uint32_t* c = (uint32_t*)(scr + s * stride);
    c[0] = 0;
    c[1] = 0;
  }
}

template <int FMT>
static void launch_noise_t(const PlaneRef& img, const NoiseGeom& g, uint8_t* scr, int64_t ss,
                           SheetCtl* ctl, int count, hipStream_t st, uint32_t* sortbuf,
                           int64_t sort_stride, const SheetBits& ready) {
  NoiseGeom gd = g;  // the kernels' copy
  gd.diag = diag_noise();
  gd.bbits = ready.bbits;
  gd.bb_stride = ready.stride;
  if constexpr (FMT == F_GRAY8) {
    // the dark bit-plane from the decode, or made here at the start of the
    // sort buffer's space; the small bit-plane in that space too, behind it
    // (noise_scratch_bytes)
    const int32_t nwr = noise_bit_words(g);
    const int64_t words = (int64_t)nwr * g.H;
    const uint32_t* bits = ready.nbits;
    int64_t bstride = ready.stride;
    uint32_t* small = sortbuf;
    if (!bits) {
      hipLaunchKernelGGL(k_noise_bits, dim3((unsigned)((words + 255) / 256), count), dim3(256), 0, st,
                         img, g, sortbuf, sort_stride, nwr, 1.0f / (float)nwr);
      bits = sortbuf;
      bstride = sort_stride;
      small = sortbuf + words;
    }
    const int64_t ta = (int64_t)nwr * ((g.H + kPRA - 1) / kPRA);
    const int64_t tb = (int64_t)nwr * ((g.H + kPRB - 1) / kPRB);
    const dim3 grid((unsigned)((ta + 255) / 256), count), gridb((unsigned)((tb + 255) / 256), count);
    UPH_LAUNCH_DIAG(131072, k_noise_cand, grid, dim3(256), 0, st, gd, scr, ss, bits, bstride, small,
                    sort_stride, nwr, 1.0f / (float)nwr);
    if (!g.all_seq)
      UPH_LAUNCH_DIAG(131072, k_noise_verdict, gridb, dim3(256), 0, st, gd, scr, ss, bits, bstride,
                      small, sort_stride, nwr, 1.0f / (float)nwr);
  } else {
    dim3 grid((g.W + kNT - 1) / kNT, (g.H + kNT - 1) / kNT, count);
    UPH_LAUNCH_DIAG(131072, k_noise_classify<FMT>, grid, dim3(256), 0, st, img, gd, scr, ss, ctl);
  }
  hipLaunchKernelGGL(k_noise_apply<FMT>, dim3(64, count), dim3(256), 0, st, img, gd, scr, ss, ctl);
  const int gt = noise_group_threads(g.W, g.H);
  if (!(diag_skip() & 2)) {
    if (gt == 1024) {
      allow_dynamic_lds((const void*)k_noise_group<FMT, 1024>, group_lds(1024));
      hipLaunchKernelGGL((k_noise_group<FMT, 1024>), dim3(count), dim3(1024), group_lds(1024), st, img, gd,
                         scr, ss, ctl, sortbuf, sort_stride);
    } else {
      allow_dynamic_lds((const void*)k_noise_group<FMT, 256>, group_lds(256));
      hipLaunchKernelGGL((k_noise_group<FMT, 256>), dim3(count), dim3(256), group_lds(256), st, img, gd,
                         scr, ss, ctl, sortbuf, sort_stride);
    }
    hipLaunchKernelGGL(k_noise_replay<FMT>, dim3(replay_blocks(count), count), dim3(256), 0, st, img,
                       gd, scr, ss, sortbuf, sort_stride, kCapPerThread * gt);
  }
}

void launch_noisefilter(const PlaneRef& img, const NoiseGeom& g, void* scratch,
                        int64_t scratch_stride, SheetCtl* ctl, int count, hipStream_t st,
                        const SheetBits& bits) {
  // layout of `scratch` per sheet: [noise lists][sort buffer (capacity pow2)]
  uint8_t* scr = (uint8_t*)scratch;
  const size_t lists = noise_list_bytes(g);
  uint32_t* sortbuf = (uint32_t*)(scr + lists);
  const int64_t sort_stride = scratch_stride / 4;
  hipLaunchKernelGGL(k_noise_zero, dim3((count + 255) / 256), dim3(256), 0, st, scr,
                     scratch_stride, count);
  switch (img.P.fmt) {
    case F_GRAY8:
      launch_noise_t<F_GRAY8>(img, g, scr, scratch_stride, ctl, count, st, sortbuf, sort_stride,
                              bits);
      break;
    case F_Y400A:
      launch_noise_t<F_Y400A>(img, g, scr, scratch_stride, ctl, count, st, sortbuf, sort_stride,
                              {});
      break;
    default:
      launch_noise_t<F_RGB24>(img, g, scr, scratch_stride, ctl, count, st, sortbuf, sort_stride,
                              {});
      break;
  }
}

}  // namespace uph
