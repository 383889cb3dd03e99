// kernels_gray.hip — the grayfilter for gfx950.
//
// The grayfilter, blurfilter (kernels_blur.hip) and noisefilter
// (kernels_noise.hip) are raster-order scans in the reference whose later
// decisions can depend on earlier writes.  Each is split into (1) one
// streaming pass that computes every decision input in parallel on the
// unmodified image and (2) an exact resolution of the order dependence on
// small per-sheet data, proven equivalent to the sequential scan (DESIGN.md
// §Order-dependent scans).
#include "filters_common.h"

namespace uph {

__host__ __device__ static inline int32_t gcd_i(int32_t a, int32_t b) {
  a = a < 0 ? -a : a;
  b = b < 0 ? -b : b;
  while (b) {
    int32_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// =========================================================================
// GRAYFILTER (filters.c:370-402)
//   tile T at (i*sx, j*sy), visited x-fastest for x = 0.. first x >= W and
//   y = 0.. <= H.  T is wiped iff it holds no pixel with gray <= black_thr and
//   255 - lightness_sum/count(clip T) < abs_thr, evaluated on the image as
//   left by the wipes of EARLIER tiles.  A wipe never changes a dark count
//   (wiped tiles had none) and only raises lightness, so T's predicate is
//   monotone in the set of earlier wipes.  The exact result is the unique
//   fixed point of "wiped(T) = pred(T, {earlier wiped})", reached by Jacobi
//   iteration from the tiles that pass on the original image.
// =========================================================================
bool gray_geometry(int32_t W, int32_t H, const UphipGrayfilterParameters& p, uint8_t black_thr,
                   GrayGeom* g) {
  if (p.scan_size.width <= 0 || p.scan_size.height <= 0 || p.scan_step.horizontal <= 0 ||
      p.scan_step.vertical <= 0)
    return false;
  g->W = W;
  g->H = H;
  g->scan_w = p.scan_size.width;
  g->scan_h = p.scan_size.height;
  g->step_x = p.scan_step.horizontal;
  g->step_y = p.scan_step.vertical;
  g->cw = gcd_i(g->step_x, g->scan_w);
  g->ch = gcd_i(g->step_y, g->scan_h);
  g->ncx = (W + g->cw - 1) / g->cw;
  g->ncy = (H + g->ch - 1) / g->ch;
  g->tw = g->scan_w / g->cw;
  g->th = g->scan_h / g->ch;
  g->tsx = g->step_x / g->cw;
  g->tsy = g->step_y / g->ch;
  // x = 0, sx, ... up to and including the first value >= W (filters.c:392-399)
  g->ntx = (W + g->step_x - 1) / g->step_x + 1;
  g->nty = H / g->step_y + 1;  // y = 0.. <= H
  g->black_thr = black_thr;
  g->abs_thr = p.abs_threshold;
  return true;
}

size_t gray_scratch_bytes(const GrayGeom& g) {
  const size_t cells = (size_t)g.ncx * g.ncy;
  const size_t tiles = (size_t)g.ntx * g.nty;
  size_t b = cells * 8 + tiles;  // dark+light (2 x u32), tile state
  b = (b + 3) & ~(size_t)3;
  b += 4;                        // undecided-tile counter
  return (b + 255) & ~(size_t)255;
}

struct GrayPtrs {
  uint32_t* dark;
  uint32_t* light;
  uint8_t* tile;     // 0 = never, 1 = undecided, 2 = wiped (3 = newly wiped, transient)
  uint32_t* nund;    // undecided tiles
};
__device__ __forceinline__ GrayPtrs gray_ptrs(const GrayGeom& g, uint8_t* base) {
  const size_t cells = (size_t)g.ncx * g.ncy;
  const size_t tiles = (size_t)g.ntx * g.nty;
  GrayPtrs p;
  p.dark = (uint32_t*)base;
  p.light = p.dark + cells;
  p.tile = (uint8_t*)(p.light + cells);
  p.nund = (uint32_t*)(base + ((cells * 8 + tiles + 3) & ~(size_t)3));
  return p;
}

template <int FMT>
__global__ void __launch_bounds__(256) k_gray_cells(PlaneRef img, GrayGeom g, uint8_t* scratch,
                                                    int64_t sstride) {
  const int s = blockIdx.z;
  const int32_t cx = blockIdx.x * 256 + threadIdx.x, cy = blockIdx.y;
  GrayPtrs P = gray_ptrs(g, scratch + s * sstride);
  if (cx == 0 && cy == 0) *P.nund = 0;
  if (cx >= g.ncx) return;
  const uint8_t* base = plane_ptr(img, s);
  const int32_t x0 = cx * g.cw, x1 = imin(x0 + g.cw, g.W);
  const int32_t y0 = cy * g.ch, y1 = imin(y0 + g.ch, g.H);
  uint32_t dark = 0, light = 0;
  for (int32_t y = y0; y < y1; y++) {
    const uint8_t* row = base + (int64_t)y * img.P.pitch;
    for (int32_t x = x0; x < x1; x++) {
      Px p = load_px_row<FMT>(row, x);
      dark += gray_of(p) <= g.black_thr ? 1u : 0u;
      light += light_of(p);
    }
  }
  const size_t c = (size_t)cy * g.ncx + cx;
  P.dark[c] = dark;
  P.light[c] = light;
}

// k_gray_cells for a gray plane: one workgroup per kGrayStrips strips of cell
// rows, a lane per 8-byte column group (the block is as wide as a row's
// groups, so nearly every lane has one).  A lane adds its columns over the
// strip's rows as 16-bit lanes of four words (bytes 0/2 and 1/3 of each
// dword), counting bytes above the dark threshold as bit 8 of byte + 256 -
// (thr+1) (ch <= 255 keeps both in 16 bits), and posts the 16-bit column
// totals to LDS; then one lane per cell adds its cw columns.
// With `colsum`, the block's strips also add up per-column gray sums over all
// rows: the sums the next mask scan takes (detect_mask, masks.c:54-100, on
// the image the grayfilter leaves; k_gray_wipe adds what its wipes change), so
// that scan needs no pass of its own.  kGrayStrips strips per block keep the
// atomics at W per kGrayStrips * ch rows.
constexpr int kGrayStrips = 8;
__global__ void __launch_bounds__(1024) k_gray_cells_g(PlaneRef img, GrayGeom g, uint8_t* scratch,
                                                       int64_t sstride, uint32_t* colsum,
                                                       int64_t colsum_stride) {
  const int s = blockIdx.z;
  GrayPtrs P = gray_ptrs(g, scratch + s * sstride);
  if (blockIdx.x == 0 && threadIdx.x == 0) *P.nund = 0;
  const uint8_t* base = plane_ptr(img, s);
  const int64_t pitch = img.P.pitch;
  // [wq] dark counts, [wq] lightness sums (u16), then [W] u32 totals
  extern __shared__ __attribute__((aligned(16))) uint16_t cols16[];
  const int32_t wq = (g.W + 7) & ~7;
  uint16_t* cdark = cols16;
  uint16_t* clight = cols16 + wq;
  uint32_t* ctot = reinterpret_cast<uint32_t*>(cols16 + 2 * wq);
  if (colsum)
    for (int32_t x = threadIdx.x; x < g.W; x += blockDim.x) ctot[x] = 0;
  const int32_t n8 = (g.W + 7) >> 3;
  const uint32_t kadd = (256u - ((uint32_t)g.black_thr + 1u)) * 0x00010001u;
  const int32_t cy_end = imin((int32_t)(blockIdx.x + 1) * kGrayStrips, g.ncy);
  for (int32_t cy = blockIdx.x * kGrayStrips; cy < cy_end; cy++) {
    const int32_t y0 = cy * g.ch, y1 = imin(y0 + g.ch, g.H);
    for (int32_t d = threadIdx.x; d < n8; d += blockDim.x) {
      // words: bytes 0/2 and 1/3 of the group's dword 0, then of dword 1
      uint32_t l[4] = {0, 0, 0, 0}, ge[4] = {0, 0, 0, 0};
      auto add = [&](uint2 v) {
        const uint32_t w[4] = {v.x & 0x00FF00FFu, (v.x >> 8) & 0x00FF00FFu, v.y & 0x00FF00FFu,
                               (v.y >> 8) & 0x00FF00FFu};
#pragma unroll
        for (int j = 0; j < 4; j++) {
          l[j] += w[j];
          ge[j] += (w[j] + kadd) & 0x01000100u;
        }
      };
      const uint8_t* p = base + (int64_t)y0 * pitch + 8 * d;
      int32_t y = y0;
      for (; y + 4 <= y1; y += 4, p += 4 * pitch) {
        uint2 v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = *reinterpret_cast<const uint2*>(p + k * pitch);
#pragma unroll
        for (int k = 0; k < 4; k++) add(v[k]);
      }
      for (; y < y1; y++, p += pitch) add(*reinterpret_cast<const uint2*>(p));
      const uint32_t rows2 = (uint32_t)(y1 - y0) * 0x00010001u;
      uint32_t dk[4];
#pragma unroll
      for (int j = 0; j < 4; j++) dk[j] = rows2 - (ge[j] >> 8);
      // columns 8d + 4k + b sit in word 2k + (b & 1), half b >> 1
      const uint32_t sel_lo = 0x05040100u, sel_hi = 0x07060302u;  // (a.lo, b.lo), (a.hi, b.hi)
      const uint4 dv = make_uint4(__builtin_amdgcn_perm(dk[1], dk[0], sel_lo),
                                  __builtin_amdgcn_perm(dk[1], dk[0], sel_hi),
                                  __builtin_amdgcn_perm(dk[3], dk[2], sel_lo),
                                  __builtin_amdgcn_perm(dk[3], dk[2], sel_hi));
      const uint4 lv = make_uint4(__builtin_amdgcn_perm(l[1], l[0], sel_lo),
                                  __builtin_amdgcn_perm(l[1], l[0], sel_hi),
                                  __builtin_amdgcn_perm(l[3], l[2], sel_lo),
                                  __builtin_amdgcn_perm(l[3], l[2], sel_hi));
      *reinterpret_cast<uint4*>(cdark + 8 * d) = dv;
      *reinterpret_cast<uint4*>(clight + 8 * d) = lv;
    }
    __syncthreads();
    for (int32_t cx = threadIdx.x; cx < g.ncx; cx += blockDim.x) {
      const int32_t x0 = cx * g.cw, x1 = imin(x0 + g.cw, g.W);
      uint32_t dark = 0, light = 0;
      for (int32_t x = x0; x < x1; x++) {
        dark += cdark[x];
        light += clight[x];
      }
      const size_t c = (size_t)cy * g.ncx + cx;
      P.dark[c] = dark;
      P.light[c] = light;
    }
    if (colsum)
      for (int32_t x = threadIdx.x; x < g.W; x += blockDim.x) ctot[x] += clight[x];
    __syncthreads();  // the next strip rewrites the column tables
  }
  if (colsum) {
    uint32_t* out = colsum + (int64_t)s * colsum_stride;
    for (int32_t x = threadIdx.x; x < g.W; x += blockDim.x)
      if (ctot[x]) atomicAdd(out + x, ctot[x]);
  }
}

__device__ __forceinline__ uint32_t cell_pixels(const GrayGeom& g, int32_t cx, int32_t cy) {
  const int32_t w = imin((cx + 1) * g.cw, g.W) - cx * g.cw;
  const int32_t h = imin((cy + 1) * g.ch, g.H) - cy * g.ch;
  return (w > 0 && h > 0) ? (uint32_t)(w * h) : 0u;
}

// inverse_lightness_rect of tile (tx,ty) on the original image, the cells'
// lightness sums from light(cx, cy)
template <class Light>
__device__ __forceinline__ uint8_t gray_tile_inv0(const GrayGeom& g, int32_t tx, int32_t ty,
                                                  Light light) {
  const Rect r = clip(rect_from_size(tx * g.step_x, ty * g.step_y, g.scan_w, g.scan_h), g.W, g.H);
  const uint64_t count = count_pixels(r);
  uint64_t sum = 0;
  const int32_t cx0 = tx * g.tsx, cy0 = ty * g.tsy;
  for (int32_t j = 0; j < g.th; j++) {
    const int32_t cy = cy0 + j;
    if (cy >= g.ncy) break;
    for (int32_t i = 0; i < g.tw; i++) {
      const int32_t cx = cx0 + i;
      if (cx >= g.ncx) break;
      sum += light(cx, cy);
    }
  }
  if (r.x1 < r.x0 || r.y1 < r.y0) sum = 0;  // loop body never runs
  return (uint8_t)(0xFFull - sum / count);
}

// inverse_lightness_rect of tile (tx,ty) with wiped cells reading 255.
// mode 0: original image; mode 1: cells covered by an EARLIER wiped tile are white.
__device__ uint8_t gray_tile_inv(const GrayGeom& g, const GrayPtrs& P, int32_t tx, int32_t ty,
                                 int mode) {
  const Rect r = clip(rect_from_size(tx * g.step_x, ty * g.step_y, g.scan_w, g.scan_h), g.W, g.H);
  const uint64_t count = count_pixels(r);
  uint64_t sum = 0;
  const int32_t cx0 = tx * g.tsx, cy0 = ty * g.tsy;
  for (int32_t j = 0; j < g.th; j++) {
    const int32_t cy = cy0 + j;
    if (cy >= g.ncy) break;
    for (int32_t i = 0; i < g.tw; i++) {
      const int32_t cx = cx0 + i;
      if (cx >= g.ncx) break;
      const size_t c = (size_t)cy * g.ncx + cx;
      bool white = false;
      if (mode) {
        // tiles covering cell (cx,cy) that precede (tx,ty) and are wiped
        for (int32_t oy = cy - g.th + 1; oy <= cy && !white; oy++) {
          if (oy < 0 || oy % g.tsy) continue;
          const int32_t uy = oy / g.tsy;
          if (uy >= g.nty || uy > ty) continue;
          for (int32_t ox = cx - g.tw + 1; ox <= cx; ox++) {
            if (ox < 0 || ox % g.tsx) continue;
            const int32_t ux = ox / g.tsx;
            if (ux >= g.ntx) continue;
            if (uy == ty && ux >= tx) continue;
            if (P.tile[(size_t)uy * g.ntx + ux] == 2) {
              white = true;
              break;
            }
          }
        }
      }
      sum += white ? 255u * cell_pixels(g, cx, cy) : P.light[c];
    }
  }
  if (r.x1 < r.x0 || r.y1 < r.y0) sum = 0;  // loop body never runs
  return (uint8_t)(0xFFull - sum / count);
}

// Whether cell (cx, cy) lies in a wiped tile (2): the tiles covering it are
// ux in [ceil((cx - tw + 1) / tsx), cx / tsx], likewise uy.
__device__ __forceinline__ bool gray_cell_wiped(const GrayGeom& g, const uint8_t* tile, int32_t cx,
                                                int32_t cy) {
  const int32_t uy0 = imax(0, (cy - g.th + g.tsy) / g.tsy), uy1 = imin(cy / g.tsy, g.nty - 1);
  const int32_t ux0 = imax(0, (cx - g.tw + g.tsx) / g.tsx), ux1 = imin(cx / g.tsx, g.ntx - 1);
  for (int32_t uy = uy0; uy <= uy1; uy++)
    for (int32_t ux = ux0; ux <= ux1; ux++)
      if (tile[(size_t)uy * g.ntx + ux] == 2) return true;
  return false;
}

// Every tile decided on the original image, one thread per tile: tiles with
// a dark pixel never wipe; tiles light enough on the original always wipe
// (wipes only brighten); the rest are undecided and counted.
__global__ void __launch_bounds__(256) k_gray_tiles(GrayGeom g, uint8_t* scratch, int64_t sstride) {
  const int s = blockIdx.y;
  GrayPtrs P = gray_ptrs(g, scratch + s * sstride);
  const int32_t t = blockIdx.x * 256 + threadIdx.x;
  const int32_t ntiles = g.ntx * g.nty;
  bool und = false;
  if (t < ntiles) {
    const int32_t tx = t % g.ntx, ty = t / g.ntx;
    uint32_t dark = 0;
    for (int32_t j = 0; j < g.th; j++) {
      const int32_t cy = ty * g.tsy + j;
      if (cy >= g.ncy) break;
      for (int32_t i = 0; i < g.tw; i++) {
        const int32_t cx = tx * g.tsx + i;
        if (cx >= g.ncx) break;
        dark += P.dark[(size_t)cy * g.ncx + cx];
      }
    }
    uint8_t st = 0;
    if (dark == 0) {
      st = gray_tile_inv(g, P, tx, ty, 0) < g.abs_thr ? 2 : 1;
      und = st == 1;
    }
    P.tile[t] = st;
  }
  const unsigned long long M = __ballot(und);
  if (M && (threadIdx.x & 63) == __ffsll((long long)M) - 1) atomicAdd(P.nund, (uint32_t)__popcll(M));
}

// k_gray_tiles with a workgroup per tile row: the th cell rows it covers
// (dark counts and lightness sums) staged in LDS once instead of every tile
// reading its tw x th cells from the scratch (the host takes it when those
// rows fit kGrayRowLds).
__global__ void __launch_bounds__(256) k_gray_tiles_rows(GrayGeom g, uint8_t* scratch,
                                                         int64_t sstride) {
  const int s = blockIdx.y;
  GrayPtrs P = gray_ptrs(g, scratch + s * sstride);
  const int32_t ty = blockIdx.x, cy0 = ty * g.tsy;
  const int32_t nr = imax(0, imin(g.th, g.ncy - cy0));  // cell rows inside the image
  extern __shared__ uint32_t gcl[];
  uint32_t* sd = gcl;                 // [nr][ncx] dark
  uint32_t* sl = gcl + nr * g.ncx;    // [nr][ncx] light
  for (int32_t i = threadIdx.x; i < nr * g.ncx; i += 256) {
    const size_t c = (size_t)cy0 * g.ncx + i;  // rows cy0.. are consecutive
    sd[i] = P.dark[c];
    sl[i] = P.light[c];
  }
  __syncthreads();
  bool und_any = false;
  for (int32_t tx = threadIdx.x; tx - (int32_t)threadIdx.x < g.ntx; tx += 256) {
    bool und = false;
    if (tx < g.ntx) {
      const int32_t cx0 = tx * g.tsx;
      uint32_t dark = 0;
      for (int32_t j = 0; j < nr; j++)
        for (int32_t i = 0; i < g.tw && cx0 + i < g.ncx; i++) dark += sd[j * g.ncx + cx0 + i];
      uint8_t st = 0;
      if (dark == 0) {
        const uint8_t inv = gray_tile_inv0(g, tx, ty, [&](int32_t cx, int32_t cy) {
          return sl[(cy - cy0) * g.ncx + cx];
        });
        st = inv < g.abs_thr ? 2 : 1;
        und = st == 1;
      }
      P.tile[(size_t)ty * g.ntx + tx] = st;
    }
    const unsigned long long M = __ballot(und);
    if (M && (threadIdx.x & 63) == __ffsll((long long)M) - 1) atomicAdd(P.nund, (uint32_t)__popcll(M));
    und_any |= und;
  }
  (void)und_any;
}

// The wipe feedback: Jacobi sweeps over the undecided tiles until nothing
// changes (one block per sheet; returns at once when none is undecided).
__global__ void __launch_bounds__(1024) k_gray_decide(GrayGeom g, uint8_t* scratch,
                                                      int64_t sstride) {
  const int s = blockIdx.x;
  GrayPtrs P = gray_ptrs(g, scratch + s * sstride);
  if (*P.nund == 0) return;
  const int32_t ntiles = g.ntx * g.nty;
  __shared__ int32_t changed;
  for (int iter = 0; iter < ntiles + 1; iter++) {
    if (threadIdx.x == 0) changed = 0;
    __syncthreads();
    for (int32_t t = threadIdx.x; t < ntiles; t += blockDim.x) {
      if (P.tile[t] != 1) continue;
      const int32_t tx = t % g.ntx, ty = t / g.ntx;
      if (gray_tile_inv(g, P, tx, ty, 1) < g.abs_thr) {
        P.tile[t] = 3;
        changed = 1;
      }
    }
    __threadfence_block();
    __syncthreads();
    if (!changed) break;
    for (int32_t t = threadIdx.x; t < ntiles; t += blockDim.x)
      if (P.tile[t] == 3) P.tile[t] = 2;
    __threadfence_block();
    __syncthreads();
  }
}

template <int FMT>
__global__ void __launch_bounds__(256) k_gray_wipe(PlaneRef img, GrayGeom g, uint8_t* scratch,
                                                   int64_t sstride, uint32_t* colsum,
                                                   int64_t colsum_stride) {
  const int s = blockIdx.z;
  const int32_t cx = blockIdx.x * 256 + threadIdx.x, cy = blockIdx.y;
  if (cx >= g.ncx) return;
  GrayPtrs P = gray_ptrs(g, scratch + s * sstride);
  // a cell whose lightness sum is all white is white already (Y400A wipes
  // also set alpha, so its cells are always written): one load decides the
  // blank paper before the covering tiles' states are read
  if (FMT != F_Y400A && P.light[(size_t)cy * g.ncx + cx] == 255u * cell_pixels(g, cx, cy)) return;
  if (!gray_cell_wiped(g, P.tile, cx, cy)) return;
  uint8_t* base = plane_ptr(img, s);
  const int32_t x0 = cx * g.cw, x1 = imin(x0 + g.cw, g.W);
  const int32_t y0 = cy * g.ch, y1 = imin(y0 + g.ch, g.H);
  if (FMT == F_GRAY8 && colsum) {
    // the column gray sums (k_gray_cells_g) follow the wipe: + (255 - old)
    uint32_t* out = colsum + (int64_t)s * colsum_stride;
    for (int32_t x = x0; x < x1; x++) {
      uint32_t add = 0;
      for (int32_t y = y0; y < y1; y++) add += 255u - base[(int64_t)y * img.P.pitch + x];
      if (add) atomicAdd(out + x, add);
    }
  }
  for (int32_t y = y0; y < y1; y++) {
    uint8_t* row = base + (int64_t)y * img.P.pitch;
    for (int32_t x = x0; x < x1; x++) white_px<FMT>(row, x);
  }
}

template <int FMT>
static bool launch_gray_t(const PlaneRef& img, const GrayGeom& g, uint8_t* scr, int64_t ss,
                          int count, hipStream_t st, uint32_t* colsum, int64_t cs) {
  dim3 grid((g.ncx + 255) / 256, g.ncy, count);
  const bool strips = gray_cells_by_strips(g, FMT);
  if (!strips) colsum = nullptr;
  if (strips) {
    const size_t wq = (size_t)((g.W + 7) & ~7);
    // a lane per 8-byte column group, up to 1024
    const int n8 = (g.W + 7) >> 3;
    const int threads = imin(1024, (n8 + 63) & ~63);
    UPH_LAUNCH_DIAG(32, k_gray_cells_g, dim3((g.ncy + kGrayStrips - 1) / kGrayStrips, 1, count),
                    dim3(threads), 4 * wq + (colsum ? 4 * (size_t)g.W : 0), st, img, g, scr, ss,
                    colsum, cs);
  } else {
    hipLaunchKernelGGL(k_gray_cells<FMT>, grid, dim3(256), 0, st, img, g, scr, ss);
  }
  const int32_t ntiles = g.ntx * g.nty;
  if (gray_tiles_in_lds(g))
    hipLaunchKernelGGL(k_gray_tiles_rows, dim3(g.nty, count), dim3(256), gray_rows_lds(g), st, g, scr,
                       ss);
  else
    hipLaunchKernelGGL(k_gray_tiles, dim3((ntiles + 255) / 256, count), dim3(256), 0, st, g, scr,
                       ss);
  if (!(diag_skip() & 4))
    hipLaunchKernelGGL(k_gray_decide, dim3(count), dim3(1024), 0, st, g, scr, ss);
  hipLaunchKernelGGL(k_gray_wipe<FMT>, grid, dim3(256), 0, st, img, g, scr, ss, colsum, cs);
  return colsum != nullptr;
}

bool launch_grayfilter(const PlaneRef& img, const GrayGeom& g, void* scratch,
                       int64_t scratch_stride, int count, hipStream_t st, uint32_t* colsum,
                       int64_t colsum_stride) {
  uint8_t* scr = (uint8_t*)scratch;
  switch (img.P.fmt) {
    case F_GRAY8:
      return launch_gray_t<F_GRAY8>(img, g, scr, scratch_stride, count, st, colsum, colsum_stride);
    case F_Y400A:
      return launch_gray_t<F_Y400A>(img, g, scr, scratch_stride, count, st, nullptr, 0);
    default:
      return launch_gray_t<F_RGB24>(img, g, scr, scratch_stride, count, st, nullptr, 0);
  }
}

}  // namespace uph
