// pipeline_internal.h — what the batch's three files share: the batch object,
// its plan and the argument blocks prepared for it.
//   pipeline_plan.hip  plan, allocate, prepare: host only, once per batch
//   pipeline_run.hip   the control kernels, run_batch and its stage helpers
//   pipeline.hip       the uphip_batch_* exports and the three encode branches
#pragma once

#include <string>
#include <utility>
#include <vector>

#include "filters.h"
#include "g4_enc.h"
#include "jpeg_enc.h"
#include "png_enc.h"
#include "tiff_enc.h"
#include "runtime.h"
#include "sheet_sizes.h"

namespace uph {

// ---- arguments of the control kernels (pipeline_run.hip) -------------------
struct MaskAssembleArgs {
  UphipMaskDetectionParameters p;
  int32_t W, H, npoints, assign;
};

struct RotCombo {
  float result, sinv, cosv;
};

struct RotSelectArgs {
  int32_t nangles, nedges;
  int32_t negate[4];     // top/bottom edges are negated (deskew.c:197,211)
  int32_t max_masks, mask_index;
  float deviation_rad;
  UphipRectangle dummy;
};

struct BorderAssembleArgs {
  int32_t W, H, nout, cap;
  Rect outside[UPHIP_MAX_PAGES];
  int32_t horizontal, vertical, align;
  UphipMaskAlignmentParameters ap;
  uint8_t mask_color[3];
  uint8_t bg[3];
};

// The chained border scan first counts only the rows within
// kBorderEdgeRows of the top and bottom (the scan from each edge stops at the
// first dark band, normally within the margin); sheets whose scan reaches
// the middle rows get them counted and are scanned again.
constexpr int32_t kBorderEdgeRows = 320;  // a multiple of the move's block rows

// ---- prepared argument blocks ----------------------------------------------
// Device arrays of one record per sheet of the batch, the same for every
// sheet, built and uploaded once by batch_prepare.  A null block: no launch.
template <class T>
struct Block {
  const T* args = nullptr;
  int32_t rows = 0;  // the rows the launch covers
};
using Fill = Block<FillArgs>;
using Copy = Block<CopyArgs>;
struct Wipes {  // apply_wipes: one fill per rectangle that meets the sheet
  int n = 0;
  Fill fill[UPHIP_MAX_MASKS];
};
struct AxisSums {  // the axis sums one point's (outside rectangle's) scans read
  const AxisArgs* h = nullptr;
  const AxisArgs* v = nullptr;
};

// One step of a size chain: what stretch_and_replace, resize_and_replace and
// flip_rotate_90 (blit.c:231-310) do to the sheet, as sheet_stages.c calls
// them before and after the filters.
struct SizeStep {
  enum Kind : int32_t { Stretch, Place, Rotate90 } kind;
  int32_t w, h;  // the sheet's size after the step
  Placement at;  // Place: where the sheet goes in the w x h background
  Fill fill;     // Place: that background ...
  Copy copy;     // ... and the sheet's copy into it
};
struct SizeChain {
  int n = 0;
  SizeStep step[4];  // at most: rotate, stretch, stretch to fit, place
};

// What depends only on the options and the input geometry, decided once.
struct BatchPlan {
  SizeChain pre, post;
  bool covered = false;                  // the pages cover the sheet: no background fill
  bool mask_sums_from_gray = false;      // first mask scan's column sums from the grayfilter
  bool mask_sums_from_rotate = false;    // second mask scan's from the rotation
  bool border_rows_from_center = false;  // border scan's row sums from the last centring move
  bool chain_center_align = false;       // centring, border scan and align move chained
  bool border_edge_rows_only = false;    // ... counting the rows near the edges first
  bool linear = false;                   // the bilinear rotate kernel serves the deskew
};

struct BatchArgs {
  struct {
    Fill sheet;                    // the sheet's background, for the runs whose pages leave some
    Copy page[UPHIP_MAX_PAGES];    // the decode's placements (center_image of each page): k_copy's
                                   // blits, the fit decode's records
  } decode;
  struct {
    const MaskArgs* masks = nullptr;
    Wipes wipes;
    const MaskArgs* border = nullptr;
  } pre;
  struct {  // detect_masks: both scans (deskew, centring) read the same blocks
    AxisSums sums[UPHIP_MAX_POINTS];
    const EdgeArgs* edges = nullptr;
    MaskAssembleArgs assemble{};
    // more than two points: every point's bands, one copy (k_mask_sums_points)
    const PointBand* bands = nullptr;
    int32_t band_cols = 0;  // the widest vertical band
  } mask_scan;
  struct {
    RotGeom geom{};
    RotSelectArgs select{};
  } deskew;
  struct {
    Wipes wipes, post_wipes;
    const MaskArgs *border = nullptr, *post_border = nullptr;
  } post;
  struct {
    AxisSums sums[UPHIP_MAX_PAGES];
    const BorderEdgeArgs* edges = nullptr;
    BorderAssembleArgs assemble{};
  } border_scan;
  Copy output;  // the conversion into the saved format
};

}  // namespace uph

// The batch object
struct UphipBatch {
  UphipOptions o;
  UphipBatchGeometry geo;
  int device = 0;
  hipStream_t st = nullptr;
  int cap = 0, n_in = 1;
  size_t dev_bytes = 0;                // device memory this batch allocated
  // geometry (host-planned)
  int32_t rp_w = 0, rp_h = 0;          // page after pre_rotate
  int32_t sheet_w = 0, sheet_h = 0;    // after decode
  int32_t W = 0, H = 0;                // processing size (after pre ops)
  int32_t out_w = 0, out_h = 0;        // after post ops
  int32_t work_fmt = uph::F_GRAY8;
  int32_t out_fmt = uph::F_GRAY8;      // saved format
  int32_t max_w = 0, max_h = 0;
  int64_t in_pitch = 0, in_page_stride = 0;
  int64_t pitch = 0, plane_stride = 0;
  int64_t out_pitch = 0, out_stride = 0;
  uph::BatchPlan plan;
  uph::BatchArgs args;
  uint8_t* inputs = nullptr;
  uint8_t* planes[2] = {nullptr, nullptr};
  uint8_t* out = nullptr;   // only when out_fmt != work_fmt
  uph::SheetCtl* ctl = nullptr;
  // layout
  std::vector<UphipPoint> points;
  std::vector<uph::Rect> outside;
  UphipMaskDetectionParameters mask_params;
  UphipBlackfilterParameters black_params;
  // scratch
  uint8_t* scr = nullptr;
  int64_t scr_stride = 0;
  uint8_t* rot_page = nullptr;   // pre_rotate temp pages
  // device argument arrays (uniform per batch or written by control kernels)
  std::vector<void*> allocs;
  // stage boundary events of every run since the last kernel_times() query
  std::vector<std::vector<std::pair<const char*, hipEvent_t>>> runs;
  std::vector<std::string> time_names;
  bool timing = false;                 // uphip_batch_set_timing
  int32_t* sticky = nullptr;           // OR of every sheet status since the last wait
  // geometry records
  uph::BlackGeom bgeo{};
  uph::BlackBar* dbars = nullptr;
  uph::AxisArgs *black_h = nullptr, *black_v = nullptr;
  uph::NoiseGeom ngeo{};
  uph::BlurGeom blgeo{};
  uph::GrayGeom ggeo{};
  uph::RotTable table{};
  uph::RotTable* dtable = nullptr;
  uph::RotCombo* dcombo = nullptr;
  uint32_t* dpow2 = nullptr;           // > 2 edges: glibc powf(x, 2) exceptions (libm_glibc.h)
  int npow2 = 0;
  int max_scan = 0;
  float max_angle = 0.0f;  // largest |angle| of the scan table (rotation bound)
  int32_t* peaks = nullptr;
  int32_t* rot_lines = nullptr;  // scan-line point lists (k_rot_points)
  uph::Rect* pick_mask = nullptr;
  int32_t* pick_active = nullptr;
  uph::RotateArgs* rot_args = nullptr; // [max(points, UPHIP_MAX_PAGES)][cap]
  uint8_t* rot_scratch = nullptr;      // launch_rotate_mask's records (one launch at a time: stream-ordered)
  int32_t* rot_indep = nullptr;        // two-mask launch: mask 1 independent of deskew 0
  int32_t* rot_dep = nullptr;          // ... or redone after it
  uint32_t* nbits = nullptr;           // GRAY8 noisefilter dark bit-plane (k_decode_gray)
  int64_t nbits_stride = 0;            // words per sheet (also bbits')
  uint32_t* bbits = nullptr;           // GRAY8 blurfilter bit-plane, pixel <= white (k_decode_gray)
  uph::MoveArgs* move_args = nullptr;  // cap * MAX_PAGES
  int32_t* border_need = nullptr;      // cap: the chained border scan needs the middle rows
  uph::MaskArgs* border_mask_args = nullptr;
  int32_t* edge_res = nullptr;         // cap * npoints * 4
  // more than two points (null otherwise): the options' points, uploaded once
  // (k_ctl_points), and a rotation for every mask, cap * npoints
  // (SheetCtl.rotation holds UPHIP_MAX_PAGES)
  const UphipPoint* dpoints = nullptr;
  float* rot_all = nullptr;
  int32_t mask_scan_route = 0;         // more than two points: 0 one launch, 1 looped
  int32_t* border_res = nullptr;       // cap * nout * 4
  uint32_t* sums = nullptr;            // cap * sums_stride
  int64_t sums_stride = 0;
  int last_count = 0;
  // A page size per input slot (uphip_batch_set_page_size): empty until the
  // first call, then cap * n_in entries, 0 for the geometry's size.  `place`
  // is the host mirror of args.decode.page[j].args, rebuilt by batch_place and
  // uploaded by the next run when a size changed.
  std::vector<int32_t> slot_w, slot_h;
  std::vector<uph::CopyArgs> place[UPHIP_MAX_PAGES];
  bool place_dirty = false;
  int32_t identity_sheets = 0;  // sheets [0, n) whose page is the sheet unchanged
  int32_t covered_sheets = 0;   // sheets [0, n) whose page leaves no background
  int32_t route = -1;           // the last run's decode (uphip_batch_decode_route)
  // GPU JPEG output branch (uphip_batch_encode_jpeg_async)
  uph::JencContext* jenc = nullptr;
  int jenc_pages = 0;
  // bilevel output branch (uphip_batch_encode_g4_async)
  uph::G4Context* g4 = nullptr;
  int g4_pages = 0;
  // lossless output branch (uphip_batch_encode_png_async)
  uph::PngContext* png = nullptr;
  int png_pages = 0;
  // TIFF output branch (uphip_batch_encode_tiff_async)
  uph::TiffEncContext* tiffenc = nullptr;
  int tiff_pages = 0;
};

namespace uph {

// pipeline_plan.hip: sizes and flags; device memory; the argument blocks
bool batch_plan(UphipBatch* b);
bool batch_allocate(UphipBatch* b);
bool batch_prepare(UphipBatch* b);
// a fully set sheet_size and no pre_rotate: the pages of a run may differ in size
bool fixed_sheet(const UphipOptions& o);
// the placements of every slot's page from slot_w / slot_h into b->place
void batch_place(UphipBatch* b);
// pipeline_run.hip: queues one run of `count` sheets read from src on b->st
bool run_batch(UphipBatch* b, int count, const uint8_t* src, int64_t spitch, int64_t sstride);
// the sources of a batch's output pages for the JPEG encode
void launch_jenc_sources(UphipBatch* b, int oc, int64_t page_bytes, JencImage* out, int n);

}  // namespace uph
