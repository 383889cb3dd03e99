// scan.h — argument records and launchers of the reduction / scan kernels.
#pragma once

#include "kernels.h"

namespace uph {

enum Measure : int32_t {
  M_GRAY_SUM = 0,     // (r+g+b)/3              inverse_brightness_rect
  M_DARK_COUNT = 1,   // gray <= thr            count_pixels_within_brightness(0, thr)
  M_DARKINV_SUM = 2,  // max(r,g,b)             darkness_rect
  M_LIGHT_SUM = 3,    // min(r,g,b)             inverse_lightness_rect
};

struct AxisArgs {
  Rect region;   // clipped to the image
  uint8_t thr;
  int32_t active;
};

// One detect_edge scan (masks.c:54-100) over precomputed axis sums.
struct EdgeArgs {
  int32_t active;
  int32_t sums_offset;    // entry offset into the sheet's sums row
  int32_t extent;         // image size along the scan axis (W or H)
  int32_t cross_extent;   // image size across (H or W)
  int32_t c0, c1;         // bar extent across the scan axis (unclipped)
  int32_t b0;             // first bar's low coordinate along the scan axis
  int32_t step;           // signed shift per step
  int32_t size;           // bar size along the scan axis
  float threshold;
};

// One detect_border_edge scan (masks.c:410-449) over per-row/column dark counts.
struct BorderEdgeArgs {
  int32_t active;
  int32_t sums_offset;
  int32_t extent;         // number of valid entries (image rows or columns)
  int32_t lo, hi;         // band 0 span (inclusive, as scanned; lo > hi = empty)
  int32_t step;           // signed shift per iteration
  int32_t max_step;       // result < max_step
  int32_t threshold;
};

void launch_axis_reduce(const PlaneRef& ref, const AxisArgs* args, int axis, int meas,
                        int32_t span_x, int32_t span_y, uint32_t* out, int64_t out_stride,
                        int count, hipStream_t st);
// One point's band along one axis (detect_masks with more than two points):
// the rows (axis 0) or columns (axis 1) its bars span, clipped to the image
// (lo > hi: none), and where its W (or H) sums go in the sheet's sums row.
struct PointBand {
  int32_t lo, hi;
  int32_t sums_offset;
};
// The M_GRAY_SUM column sums over band [2 i]'s rows and the row sums over band
// [2 i + 1]'s columns of every point i, in one launch: every entry stored
// (zeros for an empty band), no atomics, `out` need not be cleared.
// band_cols: the widest axis-1 band.
void launch_mask_sums_points(const PlaneRef& ref, const PointBand* bands, int npoints, int32_t W,
                             int32_t H, int32_t band_cols, uint32_t* out, int64_t out_stride,
                             int count, hipStream_t st);
// Which kernel launch_axis_reduce takes (uphip_filter_arms reports it).
enum AxisArm : int32_t {
  AXIS_COLSUM_GRAY,    // k_colsum_g
  AXIS_ROWSUM_GRAY,    // k_rowsum_g, 2^lg < 64 lanes a row
  AXIS_ROWSUM_GRAY_WAVE,  // k_rowsum_g at lg = 6: a wave a row
  AXIS_COLSUM,         // k_colsum<FMT>
  AXIS_ROWSUM,         // k_rowsum<FMT>, a block a row
  AXIS_ROWSUM_STRIDE,  // k_rowsum<FMT>, 2048 blocks striding over the rows
};
constexpr int32_t kRowsumMaxBlocks = 2048;
// k_rowsum_g's lanes per row, as a power of two: the one covering a
// full-width row's 16-byte vectors (the regions of one launch differ per sheet
// only in position)
inline int rowsum_gray_lg(int32_t span_x) {
  const int nv = (span_x + 30) / 16;
  int lg = 0;
  while ((1 << lg) < nv && lg < 6) lg++;
  return lg;
}
inline AxisArm axis_arm(int fmt, int axis, int32_t span_x, int32_t span_y) {
  if (fmt == F_GRAY8) {
    if (axis == 0) return AXIS_COLSUM_GRAY;
    return rowsum_gray_lg(span_x) == 6 ? AXIS_ROWSUM_GRAY_WAVE : AXIS_ROWSUM_GRAY;
  }
  if (axis == 0) return AXIS_COLSUM;
  return span_y > kRowsumMaxBlocks ? AXIS_ROWSUM_STRIDE : AXIS_ROWSUM;
}
// grid: jobs_per_sheet x count; results[s*jobs + j] = detect_edge count
// max_extent: the largest EdgeArgs/BorderEdgeArgs extent of the launch
void launch_edge_scan(const EdgeArgs* args, int jobs_per_sheet, const uint32_t* sums,
                      int64_t sums_stride, int32_t* results, int count, hipStream_t st,
                      int32_t max_extent);
// Rows [gap0, gap1) of the sums not counted (gap0 >= gap1: none): a sheet
// whose scan reaches them before a hit gets need[s] = 1 and result 0, to be
// scanned again once they are.  only (optional): the sheets to scan.
void launch_border_scan(const BorderEdgeArgs* args, int jobs_per_sheet, const uint32_t* sums,
                        int64_t sums_stride, int32_t* results, int count, hipStream_t st,
                        int32_t max_extent, int32_t gap0 = 0, int32_t gap1 = 0,
                        int32_t* need = nullptr, const int32_t* only = nullptr);

}  // namespace uph
