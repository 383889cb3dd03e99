// filters.h — geometry records and launchers of the filter kernels
// (imageprocess/filters.c) and rotation detection (imageprocess/deskew.c).
#pragma once

#include "scan.h"

namespace uph {

// ---- what the page decode hands on -----------------------------------------
// By-products of the fused GRAY8 decode (launch_decode_gray) that later
// filters take instead of computing them; all zero: nothing handed on.  The
// launchers pass them to F_GRAY8 planes only.
struct SheetBits {
  // the noisefilter's dark bit-plane (pixel < white) of the image as it
  // stands, one u32 per 32 pixels, noise_bit_words(W) words a row: the
  // blackfilter clears it where its fills paint, k_noise_bits is skipped
  uint32_t* nbits = nullptr;
  // the blurfilter's bit-plane (pixel <= white), same layout: the
  // blackfilter's paints and every clear of the noisefilter clear it too, the
  // block counts then read it instead of the plane (1/8 of the bytes).  Only
  // where blur_bits_usable.
  uint32_t* bbits = nullptr;
  int64_t stride = 0;  // words per sheet, of both planes
  // in the blackfilter's scratch: its v-stripe row sums (H entries per sheet
  // after the W column sums) ...
  bool vsum = false;
  // ... and its row-major match plane (black_rm_plane)
  bool rm = false;
};

// ---- grayfilter (filters.c:370-402) -------------------------------------
// Tiles of scan_w x scan_h at origins (i*step_x, j*step_y) decompose exactly
// into cells of gcd(step_x, scan_w) x gcd(step_y, scan_h) pixels.
struct GrayGeom {
  int32_t W, H;
  int32_t cw, ch;      // cell size (pixels)
  int32_t ncx, ncy;    // cells covering the image
  int32_t tw, th;      // tile size in cells
  int32_t tsx, tsy;    // tile step in cells
  int32_t ntx, nty;    // tiles per row, tile rows (raster order, x fastest)
  int32_t scan_w, scan_h, step_x, step_y;
  uint8_t black_thr, abs_thr;
};
bool gray_geometry(int32_t W, int32_t H, const UphipGrayfilterParameters& p, uint8_t black_thr,
                   GrayGeom* g);
size_t gray_scratch_bytes(const GrayGeom& g);  // per sheet
// colsum (optional, zeroed by the caller): per-column gray sums over all rows
// of the image the grayfilter leaves, added into colsum[s * colsum_stride + x]
// (gray planes only).  Returns whether colsum was produced.
bool launch_grayfilter(const PlaneRef& img, const GrayGeom& g, void* scratch,
                       int64_t scratch_stride, int count, hipStream_t st,
                       uint32_t* colsum = nullptr, int64_t colsum_stride = 0);
// The launcher's choices.  Cells: k_gray_cells_g (a gray plane by strips of
// cell rows: 16-bit column lanes, a block as wide as the row) or the generic
// k_gray_cells<FMT>.
constexpr int kGrayStripMaxW = 16384;
constexpr int kGrayMaxCh = 255;
inline bool gray_cells_by_strips(const GrayGeom& g, int fmt) {
  return fmt == F_GRAY8 && g.W <= kGrayStripMaxW && g.ch <= kGrayMaxCh;
}
// Tiles: k_gray_tiles_rows (a tile row's th cell rows staged in LDS) where
// those rows fit kGrayRowLds, else k_gray_tiles.
constexpr int kGrayRowLds = 32 * 1024;
inline size_t gray_rows_lds(const GrayGeom& g) {
  return 2 * sizeof(uint32_t) * (size_t)g.th * g.ncx;
}
inline bool gray_tiles_in_lds(const GrayGeom& g) { return gray_rows_lds(g) <= (size_t)kGrayRowLds; }

// ---- blurfilter (filters.c:149-232) -------------------------------------
struct BlurGeom {
  int32_t W, H;
  int32_t sw, sh, step_y;
  int32_t bpr;       // blocks per row
  int32_t T;         // iterations of the top loop
  int32_t nrect;     // counted rectangles: bpr (row 0) + T*(bpr+1)
  uint8_t white;
  float intensity;
};
bool blur_geometry(int32_t W, int32_t H, const UphipBlurfilterParameters& p, uint8_t white,
                   BlurGeom* g);
size_t blur_scratch_bytes(const BlurGeom& g);
// Whether the block counts of a plane of format fmt can come from
// SheetBits::bbits: the one condition for making the plane and for reading it
// (it stays exact only while every clear makes a pixel > white).
bool blur_bits_usable(const BlurGeom& g, int fmt);
// The launcher's choices.  Counts: from the bit-plane (have_bits: the caller
// holds SheetBits::bbits and blur_bits_usable), k_blur_counts_g on a gray
// plane (<true> with 16-byte aligned rows, `aligned16`), or the generic
// k_blur_counts<FMT>; none for an image below one block.
enum BlurCountsArm : int32_t {
  BLUR_COUNTS_NONE,
  BLUR_COUNTS_BITS,
  BLUR_COUNTS_GRAY_V16,
  BLUR_COUNTS_GRAY,
  BLUR_COUNTS_GENERIC,
};
inline BlurCountsArm blur_counts_arm(const BlurGeom& g, int fmt, bool have_bits, bool aligned16) {
  if (have_bits) return BLUR_COUNTS_BITS;
  if (g.nrect <= 0) return BLUR_COUNTS_NONE;
  if (fmt == F_GRAY8 && g.sh <= 65535 && g.W <= (1 << 16))
    return aligned16 ? BLUR_COUNTS_GRAY_V16 : BLUR_COUNTS_GRAY;
  return BLUR_COUNTS_GENERIC;
}
// Resolve: one wave holding a block row in lanes (k_blur_resolve_w; <true>
// works a row of 33 .. 112 blocks in chunks), else k_blur_resolve: one lane
// over the counts staged in LDS where they fit the 64 KiB every launch may
// ask for, else over the counts in HBM.
constexpr int kBlurLanesMax = 120;  // bpr + 8 entries of A in two VGPRs
constexpr size_t kBlurResolveLds = 64 * 1024;
enum BlurResolveArm : int32_t {
  BLUR_RESOLVE_WAVE,
  BLUR_RESOLVE_WAVE_CHUNKED,
  BLUR_RESOLVE_GENERIC,
  BLUR_RESOLVE_GENERIC_HBM,
};
inline size_t blur_resolve_lds(const BlurGeom& g) {
  return sizeof(uint64_t) * ((size_t)g.nrect + 3 * (size_t)(g.bpr + 2));
}
inline BlurResolveArm blur_resolve_arm(const BlurGeom& g) {
  const bool scalar = g.bpr >= 1 && g.bpr + 8 <= kBlurLanesMax && (int64_t)g.sw * g.sh < (1ll << 31);
  if (scalar && g.bpr > 32 && g.bpr <= 112) return BLUR_RESOLVE_WAVE_CHUNKED;
  if (scalar) return BLUR_RESOLVE_WAVE;
  return blur_resolve_lds(g) <= kBlurResolveLds ? BLUR_RESOLVE_GENERIC : BLUR_RESOLVE_GENERIC_HBM;
}
void launch_blurfilter(const PlaneRef& img, const BlurGeom& g, void* scratch,
                       int64_t scratch_stride, int count, hipStream_t st, const SheetBits& bits);

// ---- noisefilter (filters.c:238-338) ------------------------------------
struct NoiseGeom {
  int32_t W, H;
  int32_t intensity;   // clamped: > 4 => everything resolved sequentially
  uint8_t white;
  int32_t capacity;    // entries per list per sheet
  int32_t all_seq;
  int32_t diag;        // TEMP timing diagnostics
  // kernel side only: SheetBits::bbits and ::stride, set by launch_noisefilter
  uint32_t* bbits;
  int64_t bb_stride;
};
bool noise_geometry(int32_t W, int32_t H, uint64_t intensity, uint8_t white, NoiseGeom* g);
size_t noise_scratch_bytes(const NoiseGeom& g);
void launch_noisefilter(const PlaneRef& img, const NoiseGeom& g, void* scratch,
                        int64_t scratch_stride, SheetCtl* ctl, int count, hipStream_t st,
                        const SheetBits& bits);
// 32-pixel words per row of the GRAY8 bit-planes
inline int32_t noise_bit_words(int32_t W) { return (W + 31) >> 5; }
// The launcher's choices.  k_noise_group's block: large sheets (C4's 9920 x
// 7016 double pages: several thousand triggers a sheet, never next to the
// code-block decode) keep 1024 threads and 16384 triggers in LDS.
inline int noise_group_threads(int32_t W, int32_t H) {
  return (int64_t)W * H > (16 << 20) ? 1024 : 256;
}
// Its row buckets: kNoiseBuckets of 2^shift rows each.
constexpr int kNoiseBuckets = 4096;
__host__ __device__ inline int noise_bucket_shift(int32_t H) {
  int b = 0;
  while (((H - 1) >> b) >= kNoiseBuckets) b++;
  return b;
}

// ---- blackfilter (filters.c:49-127, fill.c) -----------------------------
struct BlackBar {
  Rect r;          // the bar as scanned (not clipped)
  int32_t dir;     // 0: horizontal-scan stripe, 1: vertical-scan stripe
  int32_t excluded;
};
struct BlackGeom {
  int32_t W, H;
  int32_t nbars;
  int32_t nbars_h;     // first nbars_h bars belong to the horizontal scan
  Rect hregion, vregion;  // clipped sum regions (rows of h-stripe, cols of v-stripe)
  uint8_t abs_threshold;
  uint8_t mask_max;       // image.abs_black_threshold
  uint64_t intensity;
  int32_t stack_capacity; // DFS frames per sheet
  int32_t diag;           // tuning build only: bit 16 prints replay counters
};
// Enumerates the bars exactly as blackfilter_scan's loops visit them.
bool black_geometry(int32_t W, int32_t H, const UphipBlackfilterParameters& p, uint8_t mask_max,
                    BlackGeom* g, BlackBar* bars, int max_bars);
size_t black_scratch_bytes(const BlackGeom& g);
void launch_blackfilter(const PlaneRef& img, const BlackGeom& g, const BlackBar* bars, void* scratch,
                        int64_t ss, SheetCtl* ctl, int count, hipStream_t st, const AxisArgs* hargs,
                        const AxisArgs* vargs, const SheetBits& bits);
// The launcher's choice of k_black_resolve<FMT, LONG>: the long-line machinery
// up to 16 Mpixel a sheet (kernels_black.hip, launch_black_t).
inline bool black_resolve_long(const BlackGeom& g) { return (int64_t)g.W * g.H <= (16 << 20); }
// The lowest frames of the resolve's DFS stack live in LDS, deeper ones in HBM.
constexpr int kStackLds = 1024;
// The blackfilter's row-major match plane (RM: bit x of row y = gray <=
// mask_max, 64-bit words, black_wpr words a row) of sheet 0 inside its
// scratch; sheet s at + s * scratch_stride bytes.
uint32_t* black_rm_plane(const BlackGeom& g, void* scratch);

// ---- rotation detection (deskew.c:48-241) -------------------------------
constexpr int kMaxAngles = 512;
struct RotTable {
  int32_t nangles;
  float angle[kMaxAngles];
  float slope[kMaxAngles];   // tanf(angle) computed on the host (deskew.c:161)
};
struct RotGeom {
  int32_t W, H;
  int32_t nedges;           // enabled edges (<= 4)
  int32_t edge_shift[4][2]; // shift per edge in enable order (left,top,right,bottom)
  int32_t scan_size;        // params.deskewScanSize
  float scan_depth;
  int32_t max_masks;
};
// peaks[(sheet*max_masks + mask)*4 + edge][angle]
void launch_rotation_peaks(const PlaneRef& img, const RotGeom& g, const RotTable* table,
                           const Rect* masks, const int32_t* mask_active, int mask_index,
                           int32_t* peaks, int count, hipStream_t st, int nangles, int max_scan,
                           int32_t* lines, float max_abs_angle);
// Scratch for the scan-line point lists of one launch_rotation_peaks call.
size_t rotation_lines_bytes(int count, int nedges, int nangles, int max_scan);
// Per-line fallback flags inside that scratch (diagnostics).
const int32_t* rotation_line_flags(const int32_t* lines, int nlines, int max_scan);
// Host: the angle sequence of detect_edge_rotation (deskew.c:153-174).
int rotation_angles(const UphipDeskewParameters& p, RotTable* t);
// Host: detect_rotation_cpu's combination of per-edge results (deskew.c:219-240)
float combine_edge_rotations(const float* rot, int count, float deviation_rad);

// ---- page decode (sheet_stages.c:151-165) ---------------------------------
// GRAY8 page -> sheet plane (same size), plus on the way what `bits` asks for:
// its planes, and into the blackfilter's scratch (bg, black_scratch, sheet s
// at + s * scratch_stride bytes) the v-stripe row sums and the RM plane.
// Pages 16-byte aligned with a 16-multiple pitch.
void launch_decode_gray(const uint8_t* src, int64_t spitch, int64_t sstride, const PlaneRef& dst,
                        uint8_t white, const SheetBits& bits, const BlackGeom& bg,
                        void* black_scratch, int64_t scratch_stride, int count, hipStream_t st);
// The same with sheet s's page placed by place[s] (the clipped page area and
// its target, as k_copy takes them) in a sheet of `background` bytes: the
// sheet's fill, the copy and the planes in one pass.  bits.vsum is not served
// (the blackfilter sums the sheet).  Same alignment conditions.
void launch_decode_gray_fit(const uint8_t* src, int64_t spitch, int64_t sstride, const CopyArgs* place,
                            uint8_t background, const PlaneRef& dst, uint8_t white, const SheetBits& bits,
                            const BlackGeom& bg, void* black_scratch, int64_t scratch_stride, int count,
                            hipStream_t st);

}  // namespace uph
