// pipeline_plan.hip — what a batch decides once, on the host, from its options
// and input geometry alone: the sizes and flags (batch_plan), its device
// memory (batch_allocate) and every argument block that is the same for all
// sheets and all runs (batch_prepare).  run_batch only launches from these.
#include <cmath>
#include <cstring>

#include "libm_glibc.h"
#include "pipeline_internal.h"

namespace uph {
namespace {

template <class T>
T* dalloc(UphipBatch* b, size_t n) {
  void* p = nullptr;
  if (!UPH_HIP(hipMalloc(&p, sizeof(T) * (n ? n : 1)))) return nullptr;
  b->allocs.push_back(p);
  b->dev_bytes += sizeof(T) * (n ? n : 1);
  return (T*)p;
}

bool is_gray_px(UphipPixel p) { return p.r == p.g && p.g == p.b; }

SizeStep& push_step(SizeChain& c, SizeStep::Kind kind, int32_t& w, int32_t& h, int32_t nw, int32_t nh) {
  SizeStep& s = c.step[c.n++];
  s.kind = kind;
  s.w = w = nw;
  s.h = h = nh;
  return s;
}

// stretch_and_replace to `stretch` times `zoom`, then resize_and_replace to
// `page` (sheet_stages.c:283-300 and :512-530, blit.c:231-282) as steps of c;
// (w, h) follows the sheet's size.
void size_steps(SizeChain& c, int32_t& w, int32_t& h, UphipRectangleSize stretch, float zoom,
                UphipRectangleSize page) {
  int32_t sw = stretch.width == -1 ? w : stretch.width;
  int32_t sh = stretch.height == -1 ? h : stretch.height;
  sw *= zoom;
  sh *= zoom;
  if (compare_sizes(w, h, sw, sh) != 0) push_step(c, SizeStep::Stretch, w, h, sw, sh);
  if (page.width == -1 && page.height == -1) return;
  const int32_t pw = page.width == -1 ? w : page.width;
  const int32_t ph = page.height == -1 ? h : page.height;
  if (compare_sizes(w, h, pw, ph) == 0) return;
  aspect_fit(w, h, pw, ph, &sw, &sh);
  if (compare_sizes(w, h, sw, sh) != 0) push_step(c, SizeStep::Stretch, w, h, sw, sh);
  if (pw == sw && ph == sh) return;
  // resized = bg-filled (pw x ph); center_image(stretched, resized, origin, size)
  const Placement at = center_in(w, h, 0, 0, pw, ph);
  push_step(c, SizeStep::Place, w, h, pw, ph).at = at;
}

// One point, a horizontal-only scan over every row, a gray plane: the mask
// scan's sums are plain column sums of the whole image.
bool mask_scan_all_rows(const UphipBatch* b) {
  const UphipMaskDetectionParameters& p = b->mask_params;
  if (b->points.size() != 1 || !p.scan_direction.horizontal || p.scan_direction.vertical) return false;
  if (b->work_fmt != F_GRAY8) return false;
  const int32_t depth = p.scan_depth.horizontal == -1 ? b->H : p.scan_depth.horizontal;
  const int32_t c0 = b->points[0].y - depth / 2, c1 = c0 + depth - 1;
  return c0 <= 0 && c1 >= b->H - 1;
}

// The border scan's row sums can come out of the last mask-centering move
// (k_move_rect_g16 counts the dark pixels of every row it writes): one
// outside rectangle, a vertical scan only, a gray plane, and nothing between
// the centering and the border scan that writes the sheet (sheet_stages.c:
// 425-473: explicit wipes, the middle wipe, the explicit border).
bool border_rows_from_center(const UphipBatch* b) {
  const UphipOptions& o = b->o;
  const uint32_t dis = o.disable;
  const UphipBorderScanParameters& p = o.border_scan_parameters;
  if ((dis & UPHIP_NO_MASK_CENTER) || b->points.empty()) return false;
  if ((dis & UPHIP_NO_BORDER_SCAN) || b->outside.size() != 1) return false;
  if (p.scan_direction.horizontal || !p.scan_direction.vertical) return false;
  if (b->work_fmt != F_GRAY8) return false;
  if (b->outside[0].x0 > b->outside[0].x1) return false;
  if (!(dis & UPHIP_NO_WIPE)) {
    if (o.wipes.count > 0) return false;
    if (o.layout == UPHIP_LAYOUT_DOUBLE && (o.middle_wipe[0] > 0 || o.middle_wipe[1] > 0)) return false;
  }
  if (!(dis & UPHIP_NO_BORDER) &&
      (o.border.left || o.border.top || o.border.right || o.border.bottom))
    return false;
  return true;
}

// The flags of the plan: which stage hands its by-product to which.
void plan_flags(UphipBatch* b) {
  const UphipOptions& o = b->o;
  const uint32_t dis = o.disable;
  BatchPlan& p = b->plan;
  p.covered = b->n_in == 1 && b->rp_w == b->sheet_w && b->rp_h == b->sheet_h;
  // The first mask scan (sheet_stages.c:393-399) runs on the image the
  // grayfilter leaves: its column sums come out of the grayfilter's cell pass
  // (plus its wipes' changes) instead of a pass of their own.
  p.mask_sums_from_gray =
      !(dis & (UPHIP_NO_DESKEW | UPHIP_NO_MASK_SCAN | UPHIP_NO_GRAYFILTER)) && mask_scan_all_rows(b);
  // The second mask scan (sheet_stages.c:415-421) runs on the deskewed image:
  // its column sums are the rotate kernel's output sums for the rotated sheets
  // and, for the others (unchanged since), the first scan's, still in b->sums.
  p.mask_sums_from_rotate =
      !(dis & (UPHIP_NO_DESKEW | UPHIP_NO_MASK_SCAN | UPHIP_NO_MASK_CENTER)) && mask_scan_all_rows(b);
  p.border_rows_from_center = border_rows_from_center(b);
  // The centring move, the border scan and the masked align move chained
  // (launch_move_chain): the centring only counts (a dry pass, C is never
  // written) and the align move gathers straight from the uncentred plane.
  // Needs border_rows_from_center, one page (one centring move), the align move
  // on, and 32-bit plane offsets; otherwise the two moves run as separate passes.
  p.chain_center_align = p.border_rows_from_center && b->points.size() == 1 &&
                         !(dis & UPHIP_NO_BORDER_ALIGN) && b->pitch * (int64_t)b->H < (1ll << 31) &&
                         UPHIP_MAX_PAGES >= 2;
  p.border_edge_rows_only = b->H > 2 * kBorderEdgeRows + 64;
  p.linear = o.interpolate_type == UPHIP_INTERP_LINEAR && (b->work_fmt == F_GRAY8 || b->work_fmt == F_RGB24);
}

}  // namespace

// ---------------------------------------------------------------------------
// Planning
// ---------------------------------------------------------------------------
bool batch_plan(UphipBatch* b) {
  const UphipOptions& o = b->o;
  const int n = b->n_in;
  b->rp_w = b->geo.page_width;
  b->rp_h = b->geo.page_height;
  if (o.pre_rotate != 0) std::swap(b->rp_w, b->rp_h);
  // decode: input_size = coerce(sheet_size, (page_w * n, page_h))
  b->sheet_w = o.sheet_size.width == -1 ? b->rp_w * n : o.sheet_size.width;
  b->sheet_h = o.sheet_size.height == -1 ? b->rp_h : o.sheet_size.height;
  // working plane: GRAY8 is exact when every colour written is gray
  const bool gray_in = b->geo.page_format != UPHIP_FMT_RGB24;
  b->work_fmt = (gray_in && is_gray_px(o.sheet_background) && is_gray_px(o.mask_color)) ? F_GRAY8
                                                                                       : F_RGB24;
  // the size chains before and after the filters; the planes hold the largest
  int32_t w = b->sheet_w, h = b->sheet_h;
  size_steps(b->plan.pre, w, h, o.stretch_size, o.pre_zoom_factor, o.page_size);
  b->W = w;
  b->H = h;
  if (o.post_rotate != 0) push_step(b->plan.post, SizeStep::Rotate90, w, h, h, w);
  size_steps(b->plan.post, w, h, o.post_stretch_size, o.post_zoom_factor, o.post_page_size);
  b->out_w = w;
  b->out_h = h;
  b->max_w = b->sheet_w;
  b->max_h = b->sheet_h;
  for (const SizeChain* c : {&b->plan.pre, &b->plan.post})
    for (int i = 0; i < c->n; i++) {
      b->max_w = imax(b->max_w, c->step[i].w);
      b->max_h = imax(b->max_h, c->step[i].h);
    }
  if (b->W <= 0 || b->H <= 0 || b->out_w <= 0 || b->out_h <= 0) return fail("batch: empty sheet");
  b->pitch = round_pitch((int64_t)b->max_w * (b->work_fmt == F_GRAY8 ? 1 : 3));
  b->plane_stride = b->pitch * b->max_h;
  // output format (sheet_stages.c:536-552 + saveImage mapping, file.c:193-200)
  int32_t of = o.output_pixel_format == UPHIP_FMT_NONE ? b->geo.page_format : o.output_pixel_format;
  if (of == UPHIP_FMT_Y400A) of = UPHIP_FMT_GRAY8;
  if (of == UPHIP_FMT_MONOBLACK) of = UPHIP_FMT_MONOWHITE;
  b->out_fmt = of;
  // layout defaults (sheet_stages.c:232-279) on the processing size
  const int32_t W = b->W, H = b->H;
  if (o.point_count > UPHIP_MAX_POINTS)
    return fail("batch: point_count %zu exceeds UPHIP_MAX_POINTS (%d)", (size_t)o.point_count,
                UPHIP_MAX_POINTS);
  b->points.assign(o.points, o.points + o.point_count);
  int32_t mmw = o.mask_detection_parameters.maximum_width;
  int32_t mmh = o.mask_detection_parameters.maximum_height;
  if (o.layout == UPHIP_LAYOUT_SINGLE) {
    if (b->points.empty()) b->points.push_back(UphipPoint{W / 2, H / 2});
    if (mmw == -1) mmw = W;
    if (mmh == -1) mmh = H;
    b->outside.push_back(Rect{0, 0, W - 1, H - 1});
  } else if (o.layout == UPHIP_LAYOUT_DOUBLE) {
    if (b->points.empty()) {
      b->points.push_back(UphipPoint{W / 4, H / 2});
      b->points.push_back(UphipPoint{W - W / 4, H / 2});
    }
    if (mmw == -1) mmw = W / 2;
    if (mmh == -1) mmh = H;
    b->outside.push_back(Rect{0, 0, W / 2, H - 1});
    b->outside.push_back(Rect{W / 2, 0, W - 1, H - 1});
  }
  if (mmw == -1) mmw = W;
  if (mmh == -1) mmh = H;
  b->mask_params = o.mask_detection_parameters;
  b->mask_params.maximum_width = mmw;
  b->mask_params.maximum_height = mmh;
  b->black_params = o.blackfilter_parameters;
  if (b->black_params.exclusions_count == 0 && o.layout != UPHIP_LAYOUT_NONE) {
    UphipBlackfilterParameters& bp = b->black_params;
    if (o.layout == UPHIP_LAYOUT_SINGLE) {
      bp.exclusions[bp.exclusions_count++] = from_rect(rect_from_size(W / 4, H / 4, W / 2, H / 2));
    } else {
      const int32_t fw = W / 4, fh = H / 2;
      bp.exclusions[bp.exclusions_count++] = from_rect(rect_from_size(W / 8, H / 4, fw, fh));
      bp.exclusions[bp.exclusions_count++] =
          from_rect(rect_from_size(W / 8 + W / 2, H / 4, fw, fh));
    }
  }
  plan_flags(b);
  return true;
}

bool batch_allocate(UphipBatch* b) {
  const int cap = b->cap;
  const UphipOptions& o = b->o;
  b->in_pitch = round_pitch(row_bytes(b->geo.page_width, b->geo.page_format));
  b->in_page_stride = b->in_pitch * b->geo.page_height;
  b->inputs = dalloc<uint8_t>(b, (size_t)b->in_page_stride * cap * b->n_in);
  b->planes[0] = dalloc<uint8_t>(b, (size_t)b->plane_stride * cap);
  b->planes[1] = dalloc<uint8_t>(b, (size_t)b->plane_stride * cap);
  if (b->out_fmt != b->work_fmt) {
    b->out_pitch = round_pitch(row_bytes(b->out_w, b->out_fmt));
    b->out_stride = b->out_pitch * b->out_h;
    b->out = dalloc<uint8_t>(b, (size_t)b->out_stride * cap);
    if (b->out) UPH_HIP(hipMemset(b->out, 0, (size_t)b->out_stride * cap));
  }
  if (o.pre_rotate != 0) {
    const int64_t rp = round_pitch(row_bytes(b->rp_w, b->geo.page_format));
    b->rot_page = dalloc<uint8_t>(b, (size_t)rp * b->rp_h * cap);
  }
  b->ctl = dalloc<SheetCtl>(b, cap);
  b->sticky = dalloc<int32_t>(b, 1);
  if (!b->inputs || !b->planes[0] || !b->planes[1] || !b->ctl || !b->sticky) return false;
  if (!UPH_HIP(hipMemset(b->sticky, 0, sizeof(int32_t)))) return false;
  // filter geometry + scratch (one region per sheet, reused stage after stage)
  const int32_t W = b->W, H = b->H;
  size_t need = 0;
  std::vector<BlackBar> bars(2 * (size_t)(W + H) + 16);
  if (!(o.disable & UPHIP_NO_BLACKFILTER)) {
    if (b->work_fmt == F_GRAY8 && o.abs_black_threshold == 255)
      return fail("batch: abs_black_threshold 255 makes the reference flood fill recurse forever");
    if (!black_geometry(W, H, b->black_params, o.abs_black_threshold, &b->bgeo, bars.data(),
                        (int)bars.size()))
      return fail("batch: invalid blackfilter parameters");
    need = std::max(need, black_scratch_bytes(b->bgeo));
    if (b->bgeo.nbars) {
      b->dbars = dalloc<BlackBar>(b, b->bgeo.nbars);
      UPH_HIP(hipMemcpy(b->dbars, bars.data(), sizeof(BlackBar) * b->bgeo.nbars,
                        hipMemcpyHostToDevice));
    }
    std::vector<AxisArgs> hv((size_t)cap, AxisArgs{b->bgeo.hregion, 0, 1});
    b->black_h = dalloc<AxisArgs>(b, cap);
    UPH_HIP(hipMemcpy(b->black_h, hv.data(), sizeof(AxisArgs) * cap, hipMemcpyHostToDevice));
    hv.assign((size_t)cap, AxisArgs{b->bgeo.vregion, 0, 1});
    b->black_v = dalloc<AxisArgs>(b, cap);
    UPH_HIP(hipMemcpy(b->black_v, hv.data(), sizeof(AxisArgs) * cap, hipMemcpyHostToDevice));
  }
  if (!(o.disable & UPHIP_NO_NOISEFILTER)) {
    noise_geometry(W, H, o.noisefilter_intensity, o.abs_white_threshold, &b->ngeo);
    need = std::max(need, noise_scratch_bytes(b->ngeo));
    if (b->work_fmt == F_GRAY8) {
      b->nbits_stride = ((int64_t)noise_bit_words(W) * H + 63) & ~(int64_t)63;
      b->nbits = dalloc<uint32_t>(b, (size_t)b->nbits_stride * cap);
      if (!b->nbits) return false;
    }
  }
  if (!(o.disable & UPHIP_NO_BLURFILTER)) {
    if (!blur_geometry(W, H, o.blurfilter_parameters, o.abs_white_threshold, &b->blgeo))
      return fail("batch: invalid blurfilter parameters");
    need = std::max(need, blur_scratch_bytes(b->blgeo));
    if (blur_bits_usable(b->blgeo, b->work_fmt)) {
      b->nbits_stride = ((int64_t)noise_bit_words(W) * H + 63) & ~(int64_t)63;
      b->bbits = dalloc<uint32_t>(b, (size_t)b->nbits_stride * cap);
      if (!b->bbits) return false;
    }
  }
  if (!(o.disable & UPHIP_NO_GRAYFILTER)) {
    if (!gray_geometry(W, H, o.grayfilter_parameters, o.abs_black_threshold, &b->ggeo))
      return fail("batch: invalid grayfilter parameters");
    need = std::max(need, gray_scratch_bytes(b->ggeo));
  }
  need = (need + 255) & ~(size_t)255;
  b->scr_stride = (int64_t)need;
  if (need) {
    b->scr = dalloc<uint8_t>(b, need * cap);
    if (!b->scr) return false;
  }
  // detection buffers
  const int np = (int)b->points.size();
  const int nout = (int)b->outside.size();
  b->sums_stride = (int64_t)imax(b->max_w, b->max_h) * 2 * imax(np, nout) + 64;
  b->sums = dalloc<uint32_t>(b, (size_t)b->sums_stride * cap);
  b->edge_res = dalloc<int32_t>(b, (size_t)cap * imax(np, 1) * 4);
  b->border_res = dalloc<int32_t>(b, (size_t)cap * imax(nout, 1) * 4);
  b->move_args = dalloc<MoveArgs>(b, (size_t)cap * UPHIP_MAX_PAGES);
  b->border_need = dalloc<int32_t>(b, cap);
  b->border_mask_args = dalloc<MaskArgs>(b, cap);
  // a record per mask; more than two points: a rotation per mask as well
  b->rot_args = dalloc<RotateArgs>(b, (size_t)cap * (np > 2 ? np : UPHIP_MAX_PAGES));
  if (np > 2) {
    b->rot_all = dalloc<float>(b, (size_t)cap * np);
    if (!b->rot_all) return false;
  }
  b->rot_scratch = dalloc<uint8_t>(b, rotate_scratch_bytes(b->max_w, b->max_h, cap));
  if (!b->rot_scratch) return false;
  b->rot_indep = dalloc<int32_t>(b, cap);
  b->rot_dep = dalloc<int32_t>(b, cap);
  b->pick_mask = dalloc<Rect>(b, cap);
  b->pick_active = dalloc<int32_t>(b, cap);
  // rotation tables
  if (!(o.disable & UPHIP_NO_DESKEW)) {
    if (rotation_angles(o.deskew_parameters, &b->table) < 0)
      return fail("batch: too many deskew angles");
    const int na = b->table.nangles;
    for (int i = 0; i < na; i++) b->max_angle = fmaxf(b->max_angle, fabsf(b->table.angle[i]));
    b->dtable = dalloc<RotTable>(b, 1);
    UPH_HIP(hipMemcpy(b->dtable, &b->table, sizeof(RotTable), hipMemcpyHostToDevice));
    int nedges = 0;
    int kinds[4];
    const UphipEdges& E = o.deskew_parameters.scan_edges;
    const bool on[4] = {E.left, E.top, E.right, E.bottom};
    for (int k = 0; k < 4; k++)
      if (on[k]) kinds[nedges++] = k;
    // exact combination table for <= 2 edges (host libm, like deskew.c)
    size_t ncombo = nedges == 2 ? (size_t)na * na : (size_t)na;
    std::vector<RotCombo> combo(ncombo);
    for (size_t key = 0; key < ncombo; key++) {
      float rot[2];
      int idx[2] = {(int)(nedges == 2 ? key / na : key), (int)(key % na)};
      for (int e = 0; e < nedges && e < 2; e++) {
        const float v = b->table.angle[idx[e]];
        rot[e] = (kinds[e] == 1 || kinds[e] == 3) ? -v : v;
      }
      RotCombo c;
      c.result = combine_edge_rotations(rot, nedges > 2 ? 2 : nedges,
                                        o.deskew_parameters.deskewScanDeviationRad);
      c.sinv = sinf(-c.result);
      c.cosv = cosf(-c.result);
      combo[key] = c;
    }
    b->dcombo = dalloc<RotCombo>(b, ncombo);
    UPH_HIP(hipMemcpy(b->dcombo, combo.data(), sizeof(RotCombo) * ncombo, hipMemcpyHostToDevice));
    if (nedges > 2) {
      const uint32_t* t = glibc_pow2_table(&b->npow2);
      if (!t) return fail("batch: this libm's powf(x, 2) is not reproducible on the device");
      b->dpow2 = dalloc<uint32_t>(b, imax(b->npow2, 1));
      UPH_HIP(hipMemcpy(b->dpow2, t, sizeof(uint32_t) * b->npow2, hipMemcpyHostToDevice));
    }
    // k_rot_peaks and k_rot_select index it with RotGeom/RotSelectArgs.max_masks
    b->peaks = dalloc<int32_t>(b, (size_t)cap * (np > 2 ? np : UPHIP_MAX_PAGES) * 4 * (na > 0 ? na : 1));
    int ms = o.deskew_parameters.deskewScanSize;
    if (ms == -1 || ms > 10000) ms = 10000;
    b->max_scan = imin(ms, imax(W, H));
    b->rot_lines = (int32_t*)dalloc<uint8_t>(b, rotation_lines_bytes(cap, nedges, na, b->max_scan));
    if (!b->rot_lines) return false;
  }
  return true;
}

// ---------------------------------------------------------------------------
// The argument blocks
// ---------------------------------------------------------------------------
namespace {

// Builds the blocks of BatchArgs: every sheet's copy of a record, uploaded.
struct Uploader {
  UphipBatch* b;
  bool ok = true;

  template <class T>
  const T* all(const T* v, size_t n) {
    std::vector<T> h;
    for (int s = 0; s < b->cap; s++) h.insert(h.end(), v, v + n);
    T* d = dalloc<T>(b, h.size());
    ok = ok && d && (h.empty() || UPH_HIP(hipMemcpy(d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice)));
    return d;
  }
  template <class T>
  const T* all(const T& v) { return all(&v, 1); }
  // a table the sheets share: one copy
  template <class T>
  const T* once(const T* v, size_t n) {
    T* d = dalloc<T>(b, n);
    ok = ok && d && (n == 0 || UPH_HIP(hipMemcpy(d, v, sizeof(T) * n, hipMemcpyHostToDevice)));
    return d;
  }
  // wipe_rectangle of an already clipped rectangle; an empty one has no block
  Fill fill(Rect clipped, UphipPixel c) {
    if (clipped.x1 < clipped.x0 || clipped.y1 < clipped.y0) return Fill{};
    return Fill{all(FillArgs{clipped, {c.r, c.g, c.b}, 1}), clipped.y1 - clipped.y0 + 1};
  }
  // copy_rectangle of the placed part of a sw x sh source
  Copy copy(const Placement& p, int32_t sw, int32_t sh) {
    return Copy{all(CopyArgs{clip(rect_from_size(p.sx, p.sy, p.w, p.h), sw, sh), p.tx, p.ty, 1}), p.h};
  }
  const MaskArgs* masks(const Rect* m, int n, UphipPixel c) {
    if (n <= 0) return nullptr;
    MaskArgs ma{n, {c.r, c.g, c.b}, {}};
    for (int i = 0; i < n; i++) ma.m[i] = m[i];
    return all(ma);
  }
  // apply_wipes_cpu (masks.c:333-345): as-given rectangles, set_pixel clips
  void wipes(const UphipWipes& w, Wipes* out) {
    for (size_t i = 0; i < w.count && i < UPHIP_MAX_MASKS; i++) {
      const Rect r = to_rect(w.areas[i]);
      if (r.x0 > r.x1 || r.y0 > r.y1) continue;
      const Fill f = fill(clip(r, b->W, b->H), b->o.mask_color);
      if (f.args) out->fill[out->n++] = f;
    }
  }
  const MaskArgs* border(const UphipBorder& br) {
    if (br.left == 0 && br.top == 0 && br.right == 0 && br.bottom == 0) return nullptr;
    const Rect m{br.left, br.top, b->W - br.right - 1, b->H - br.bottom - 1};
    return masks(&m, 1, b->o.mask_color);
  }
  // center_image's fill and copy for the Place step of a chain that starts at w x h
  void place(SizeChain* c, int32_t w, int32_t h) {
    for (int i = 0; i < c->n; i++) {
      SizeStep& s = c->step[i];
      if (s.kind == SizeStep::Place) {
        s.fill = fill(Rect{0, 0, s.w - 1, s.h - 1}, b->o.sheet_background);
        s.copy = copy(s.at, w, h);
      }
      w = s.w;
      h = s.h;
    }
  }
};

// detect_masks' scans (masks.c:54-209): per point the axis sums' regions and
// the four edge scans over them
void prepare_mask_scan(UphipBatch* b, Uploader& up) {
  const UphipMaskDetectionParameters& p = b->mask_params;
  const int np = (int)b->points.size();
  const int32_t W = b->W, H = b->H;
  EdgeArgs ea[UPHIP_MAX_POINTS * 4];
  memset(ea, 0, sizeof(ea));
  // more than two points: the bands of k_mask_sums_points, the regions below
  std::vector<PointBand> bands;
  if (np > 2)
    for (int i = 0; i < 2 * np; i++) bands.push_back(PointBand{0, -1, i * imax(W, H)});
  for (int i = 0; i < np; i++) {
    const UphipPoint o = b->points[i];
    if (p.scan_direction.horizontal) {
      const int32_t depth = p.scan_depth.horizontal == -1 ? H : p.scan_depth.horizontal;
      const int32_t c0 = o.y - depth / 2, c1 = c0 + depth - 1;
      const Rect reg = clip(Rect{0, c0, W - 1, c1}, W, H);
      const int32_t off = (2 * i) * imax(W, H);
      if (np > 2) bands[2 * i].lo = reg.y0, bands[2 * i].hi = reg.y1;
      if (reg.y1 >= reg.y0) b->args.mask_scan.sums[i].h = up.all(AxisArgs{reg, 0, 1});
      for (int k = 0; k < 2; k++)
        ea[i * 4 + k] = EdgeArgs{1, off, W, H, c0, c1, o.x - p.scan_size.width / 2,
                                 (k == 0 ? -1 : 1) * p.scan_step.horizontal, p.scan_size.width,
                                 p.scan_threshold.horizontal};
    }
    if (p.scan_direction.vertical) {
      const int32_t depth = p.scan_depth.vertical == -1 ? W : p.scan_depth.vertical;
      const int32_t c0 = o.x - depth / 2, c1 = c0 + depth - 1;
      const Rect reg = clip(Rect{c0, 0, c1, H - 1}, W, H);
      const int32_t off = (2 * i + 1) * imax(W, H);
      if (np > 2) {
        bands[2 * i + 1].lo = reg.x0, bands[2 * i + 1].hi = reg.x1;
        b->args.mask_scan.band_cols = imax(b->args.mask_scan.band_cols, reg.x1 - reg.x0 + 1);
      }
      if (reg.x1 >= reg.x0) b->args.mask_scan.sums[i].v = up.all(AxisArgs{reg, 0, 1});
      for (int k = 2; k < 4; k++)
        ea[i * 4 + k] = EdgeArgs{1, off, H, W, c0, c1, o.y - p.scan_size.height / 2,
                                 (k == 2 ? -1 : 1) * p.scan_step.vertical, p.scan_size.height,
                                 p.scan_threshold.vertical};
    }
  }
  if (np > 2) b->args.mask_scan.bands = up.once(bands.data(), bands.size());
  b->args.mask_scan.edges = up.all(ea, (size_t)np * 4);
  b->args.mask_scan.assemble = MaskAssembleArgs{p, W, H, np, 1};
}

// detect_border's scans (masks.c:351-449) per outside rectangle, and what
// k_border_assemble makes of their results
void prepare_border_scan(UphipBatch* b, Uploader& up) {
  const UphipOptions& opt = b->o;
  const UphipBorderScanParameters& p = opt.border_scan_parameters;
  const int nout = (int)b->outside.size();
  const int32_t W = b->W, H = b->H;
  BorderEdgeArgs ea[UPHIP_MAX_PAGES * 4];
  memset(ea, 0, sizeof(ea));
  for (int i = 0; i < nout; i++) {
    const Rect o = b->outside[i];
    const int32_t mw = iabs(o.x0 - o.x1) + 1, mh = iabs(o.y0 - o.y1) + 1;
    if (p.scan_direction.horizontal) {
      const int32_t off = (2 * i) * imax(W, H);
      const AxisArgs a{clip(Rect{0, o.y0, W - 1, o.y1}, W, H), opt.abs_black_threshold, o.y0 <= o.y1 ? 1 : 0};
      if (a.active && a.region.y1 >= a.region.y0) b->args.border_scan.sums[i].h = up.all(a);
      const int32_t sz = p.scan_size.width, stp = p.scan_step.horizontal;
      ea[i * 4 + 0] = BorderEdgeArgs{1, off, W, o.x0, o.x0 + sz, stp, mw, p.scan_threshold.horizontal};
      ea[i * 4 + 1] = BorderEdgeArgs{1, off, W, o.x1 - sz, o.x1, -stp, mw, p.scan_threshold.horizontal};
    }
    if (p.scan_direction.vertical) {
      const int32_t off = (2 * i + 1) * imax(W, H);
      const AxisArgs a{clip(Rect{o.x0, 0, o.x1, H - 1}, W, H), opt.abs_black_threshold, o.x0 <= o.x1 ? 1 : 0};
      if (a.active && a.region.x1 >= a.region.x0) b->args.border_scan.sums[i].v = up.all(a);
      const int32_t sz = p.scan_size.height, stp = p.scan_step.vertical;
      ea[i * 4 + 2] = BorderEdgeArgs{1, off, H, o.y0, o.y0 + sz, stp, mh, p.scan_threshold.vertical};
      ea[i * 4 + 3] = BorderEdgeArgs{1, off, H, o.y1 - sz, o.y1, -stp, mh, p.scan_threshold.vertical};
    }
  }
  b->args.border_scan.edges = up.all(ea, (size_t)nout * 4);
  BorderAssembleArgs& ba = b->args.border_scan.assemble;
  ba = BorderAssembleArgs{W, H, nout, b->cap, {}, p.scan_direction.horizontal, p.scan_direction.vertical,
                          !(opt.disable & UPHIP_NO_BORDER_ALIGN), opt.mask_alignment_parameters,
                          {opt.mask_color.r, opt.mask_color.g, opt.mask_color.b},
                          {opt.sheet_background.r, opt.sheet_background.g, opt.sheet_background.b}};
  for (int i = 0; i < nout; i++) ba.outside[i] = b->outside[i];
}

// the rotation detection's geometry and k_rot_select's constants (deskew.c:127-240)
void prepare_deskew(UphipBatch* b) {
  const UphipDeskewParameters& dp = b->o.deskew_parameters;
  RotGeom& rg = b->args.deskew.geom;
  RotSelectArgs& ra = b->args.deskew.select;
  memset(&rg, 0, sizeof(rg));
  memset(&ra, 0, sizeof(ra));
  rg.W = b->W;
  rg.H = b->H;
  const int shifts[4][2] = {{1, 0}, {0, 1}, {-1, 0}, {0, -1}};
  const bool on[4] = {dp.scan_edges.left, dp.scan_edges.top, dp.scan_edges.right, dp.scan_edges.bottom};
  for (int k = 0; k < 4; k++)
    if (on[k]) {
      rg.edge_shift[rg.nedges][0] = shifts[k][0];
      rg.edge_shift[rg.nedges][1] = shifts[k][1];
      ra.negate[rg.nedges] = (k == 1 || k == 3);
      rg.nedges++;
    }
  rg.scan_size = dp.deskewScanSize;
  rg.scan_depth = dp.deskewScanDepth;
  const int np = (int)b->points.size();  // the stride of b->peaks
  rg.max_masks = np > 2 ? np : UPHIP_MAX_PAGES;
  ra.nangles = b->table.nangles;
  ra.nedges = rg.nedges;
  ra.max_masks = np > 2 ? np : UPHIP_MAX_PAGES;
  ra.deviation_rad = dp.deskewScanDeviationRad;
}

}  // namespace

bool fixed_sheet(const UphipOptions& o) {
  return o.sheet_size.width != -1 && o.sheet_size.height != -1 && o.pre_rotate == 0;
}

// Slot (s, j)'s page placed as batch_prepare places the geometry's: the same
// center_image, of the slot's own size.  Only the records change; the plan,
// the sheet and everything after the decode stay as planned.
void batch_place(UphipBatch* b) {
  const int n = b->n_in;
  const int32_t sw = b->sheet_w, sh = b->sheet_h;
  b->identity_sheets = b->covered_sheets = b->cap;
  for (int j = 0; j < n; j++) {
    b->place[j].resize((size_t)b->cap);
    int32_t rows = 1;
    for (int s = 0; s < b->cap; s++) {
      const size_t q = (size_t)s * n + j;
      const int32_t w = b->slot_w[q] ? b->slot_w[q] : b->geo.page_width;
      const int32_t h = b->slot_h[q] ? b->slot_h[q] : b->geo.page_height;
      const Placement p = center_in(w, h, sw * j / n, 0, sw / n, sh);
      b->place[j][(size_t)s] = CopyArgs{clip(rect_from_size(p.sx, p.sy, p.w, p.h), w, h), p.tx, p.ty, 1};
      rows = imax(rows, p.h);
      if (n != 1 || w != sw || h != sh) b->identity_sheets = imin(b->identity_sheets, s);
      if (n != 1 || w < sw || h < sh) b->covered_sheets = imin(b->covered_sheets, s);
    }
    b->args.decode.page[j].rows = rows;
  }
  b->place_dirty = true;
}

bool batch_prepare(UphipBatch* b) {
  const UphipOptions& o = b->o;
  const uint32_t dis = o.disable;
  BatchArgs& A = b->args;
  Uploader up{b};
  // decode: the unfused blits are built whether or not a run will be fused
  // (that depends on the alignment of the pages a run is given)
  const int32_t sw = b->sheet_w, sh = b->sheet_h;
  if (!b->plan.covered || fixed_sheet(o)) A.decode.sheet = up.fill(Rect{0, 0, sw - 1, sh - 1}, o.sheet_background);
  for (int j = 0; j < b->n_in; j++)  // center_image(page, sheet, (w*j/n, 0), (w/n, h))  (blit.c:175-202)
    A.decode.page[j] = up.copy(center_in(b->rp_w, b->rp_h, sw * j / b->n_in, 0, sw / b->n_in, sh), b->rp_w, b->rp_h);
  // pre and post (sheet_stages.c:187-325, :415-534)
  if (o.pre_mask_count > 0) {
    Rect pm[UPHIP_MAX_MASKS];
    const int n = (int)(o.pre_mask_count < UPHIP_MAX_MASKS ? o.pre_mask_count : UPHIP_MAX_MASKS);
    for (int i = 0; i < n; i++) pm[i] = to_rect(o.pre_masks[i]);
    A.pre.masks = up.masks(pm, n, o.mask_color);
  }
  up.place(&b->plan.pre, sw, sh);
  up.place(&b->plan.post, b->W, b->H);
  if (!(dis & UPHIP_NO_WIPE)) {
    UphipWipes wp = o.wipes;
    if (o.layout == UPHIP_LAYOUT_DOUBLE && (o.middle_wipe[0] > 0 || o.middle_wipe[1] > 0) &&
        wp.count < UPHIP_MAX_MASKS) {
      wp.areas[wp.count++] = from_rect(Rect{b->W / 2 - o.middle_wipe[0], 0,
                                            b->W / 2 + o.middle_wipe[1], b->H - 1});
    }
    up.wipes(o.pre_wipes, &A.pre.wipes);
    up.wipes(wp, &A.post.wipes);
    up.wipes(o.post_wipes, &A.post.post_wipes);
  }
  if (!(dis & UPHIP_NO_BORDER)) {
    A.pre.border = up.border(o.pre_border);
    A.post.border = up.border(o.border);
    A.post.post_border = up.border(o.post_border);
  }
  // k_ctl_init carries two points; more go up here once (k_ctl_points)
  if (b->points.size() > 2) b->dpoints = up.once(b->points.data(), b->points.size());
  if (!(dis & UPHIP_NO_MASK_SCAN)) prepare_mask_scan(b, up);
  if (!(dis & UPHIP_NO_DESKEW)) prepare_deskew(b);
  if (!(dis & UPHIP_NO_BORDER_SCAN) && !b->outside.empty()) prepare_border_scan(b, up);
  if (b->out) A.output = Copy{up.all(CopyArgs{Rect{0, 0, b->out_w - 1, b->out_h - 1}, 0, 0, 1}), b->out_h};
  return up.ok;
}

}  // namespace uph
