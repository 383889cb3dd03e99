// pipeline_run.hip — one run of a batch: the control kernels (one thread per
// sheet) and run_batch with its stage helpers.  Every size, flag and uniform
// argument block comes from the plan (pipeline_plan.hip); a run only launches,
// and its one branch on its own arguments is the decode's route.
#include <cstdio>
#include <cstdlib>

#include "libm_glibc.h"
#include "pipeline_internal.h"

namespace uph {

// ---------------------------------------------------------------------------
// control kernels (one thread per sheet)
// ---------------------------------------------------------------------------
__global__ void k_ctl_init(SheetCtl* ctl, int count, int32_t npoints, UphipPoint p0, UphipPoint p1) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= count) return;
  SheetCtl& c = ctl[s];
  c.cur = 0;
  c.status = 0;
  c.point_count = npoints;
  c.mask_count = 0;
  c.points[0] = p0;
  c.points[1] = p1;
  for (int i = 0; i < UPHIP_MAX_PAGES; i++) c.rotation[i] = 0.0f;
}

// More than two points, after k_ctl_init: every point from the plan's copy
// and a zero rotation for every mask (rot_all[s * npoints + i]).
__global__ void k_ctl_points(SheetCtl* ctl, int count, int32_t npoints, const UphipPoint* points,
                             float* rot_all) {
  const int s = blockIdx.x;
  if (s >= count) return;
  for (int i = threadIdx.x; i < npoints; i += blockDim.x) {
    ctl[s].points[i] = points[i];
    rot_all[(int64_t)s * npoints + i] = 0.0f;
  }
}

// Folds every sheet's status into the batch's sticky word at the end of a
// run: k_ctl_init clears the per-sheet words at the start of the next run,
// so without this a failure in an earlier of several runs enqueued before
// one uphip_batch_wait would be lost.
__global__ void k_status_fold(const SheetCtl* ctl, int count, int32_t* sticky) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < count && ctl[s].status) atomicOr(sticky, ctl[s].status);
}

__global__ void k_flip_all(SheetCtl* ctl, int count) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < count) ctl[s].cur ^= 1;
}

// detect_mask / detect_masks_cpu (masks.c:107-209) from the four edge counts
__global__ void k_mask_assemble(SheetCtl* ctl, const int32_t* edges, MaskAssembleArgs a,
                                int count) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= count) return;
  SheetCtl& c = ctl[s];
  const UphipMaskDetectionParameters& p = a.p;
  int32_t valid = 0;
  for (int i = 0; i < a.npoints; i++) {
    const int32_t* e = edges + ((int64_t)s * a.npoints + i) * 4;
    const UphipPoint o = c.points[i];
    Rect m;
    if (p.scan_direction.horizontal) {
      m.x0 = o.x - (p.scan_step.horizontal * e[0]) - p.scan_size.width / 2;
      m.x1 = o.x + (p.scan_step.horizontal * e[1]) + p.scan_size.width / 2;
    } else {
      m.x0 = 0;
      m.x1 = a.W - 1;
    }
    if (p.scan_direction.vertical) {
      m.y0 = o.y - (p.scan_step.vertical * e[2]) - p.scan_size.height / 2;
      m.y1 = o.y + (p.scan_step.vertical * e[3]) + p.scan_size.height / 2;
    } else {
      m.y0 = 0;
      m.y1 = a.H - 1;
    }
    const int32_t mw = iabs(m.x0 - m.x1) + 1, mh = iabs(m.y0 - m.y1) + 1;
    if ((p.minimum_width != -1 && mw < p.minimum_width) ||
        (p.maximum_width != -1 && mw > p.maximum_width)) {
      m.x0 = o.x - p.maximum_width / 2;
      m.x1 = o.x + p.maximum_width / 2;
    }
    if ((p.minimum_height != -1 && mh < p.minimum_height) ||
        (p.maximum_height != -1 && mh > p.maximum_height)) {
      m.y0 = o.y - p.maximum_height / 2;
      m.y1 = o.y + p.maximum_height / 2;
    }
    c.masks[i] = from_rect(m);
    if (!(m.x0 == -1 && m.y0 == -1 && m.x1 == -1 && m.y1 == -1)) valid++;
  }
  if (a.assign) c.mask_count = valid;
}

// masks[i] -> a Rect array + active flags for the rotation-peak kernel
// only (may be null): sheets outside it are marked inactive
__global__ void k_mask_pick(const SheetCtl* ctl, int i, Rect* out, int32_t* active, int count,
                            const int32_t* only) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= count) return;
  out[s] = to_rect(ctl[s].masks[i]);
  active[s] = i < ctl[s].mask_count && (!only || only[s]);
}

// Two masks rotated in one launch (the double layout): the reference detects
// and deskews mask 1 after deskewing mask 0 (sheet_stages.c:401-412).  Doing
// both detections first and both rotations from the same image is the same
// thing unless deskew 0 changes a pixel that mask 1's detection or rotation
// reads: detection reads only pixels inside its mask (deskew.c:127-131), and
// the rotation the source window of its mask (a rotated rectangle, bounded
// here by its corners with two taps of margin either side).  dep[s] = 1 for
// the sheets where that may happen: mask 1 is then detected and rotated again
// after mask 0 (second pass); indep[s] = 1 where mask 1 rotates in the first.
__global__ void k_rot_independent(const SheetCtl* ctl, const RotateArgs* args, int64_t mstride,
                                  int32_t* indep, int32_t* dep, int count) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= count) return;
  const SheetCtl& c = ctl[s];
  const RotateArgs a0 = args[s], a1 = args[mstride + s];
  bool d = false;
  if (c.mask_count >= 2 && a0.active) {
    const Rect m0 = normalize(to_rect(c.masks[0])), m1 = normalize(to_rect(c.masks[1]));
    auto meets = [](const Rect& p, const Rect& q) {
      return p.x0 <= q.x1 && q.x0 <= p.x1 && p.y0 <= q.y1 && q.y0 <= p.y1;
    };
    d = meets(m0, m1);
    if (!d && a1.active) {
      // mask 1's source footprint is a rotated rectangle: in source space
      // (deskew.c:264-268) the point of mask pixel (u, v) is C + (u - tcx) e_u
      // + (v - tcy) e_v with e_u = (cos, -sin), e_v = (sin, cos).  It meets
      // mask 0 unless an axis of either separates them (x, y, e_u, e_v);
      // 4 px of margin cover the interpolation taps and float rounding.
      const Rect nm = normalize(a1.mask);
      const int32_t sw = nm.x1 - nm.x0 + 1, sh = nm.y1 - nm.y0 + 1;
      const float scx = nm.x0 + sw / 2.0f, scy = nm.y0 + sh / 2.0f;
      const float tcx = 0 + sw / 2.0f, tcy = 0 + sh / 2.0f;
      const float cs = a1.cosval, sn = a1.sinval, mg = 4.0f;
      float mnx = 3.0e38f, mxx = -3.0e38f, mny = 3.0e38f, mxy = -3.0e38f;
      for (int k = 0; k < 4; k++) {
        const int32_t u = k & 1 ? sw - 1 : 0, v = k & 2 ? sh - 1 : 0;
        const float X = scx + (u - tcx) * cs + (v - tcy) * sn;
        const float Y = scy + (v - tcy) * cs - (u - tcx) * sn;
        mnx = fminf(mnx, X);
        mxx = fmaxf(mxx, X);
        mny = fminf(mny, Y);
        mxy = fmaxf(mxy, Y);
      }
      bool sep = mxx + mg < (float)m0.x0 || mnx - mg > (float)m0.x1 || mxy + mg < (float)m0.y0 ||
                 mny - mg > (float)m0.y1;
      if (!sep) {
        // mask 0's corners on the footprint's own axes
        float au = 3.0e38f, bu = -3.0e38f, av = 3.0e38f, bv = -3.0e38f;
        for (int k = 0; k < 4; k++) {
          const float dx = (float)(k & 1 ? m0.x1 : m0.x0) - scx;
          const float dy = (float)(k & 2 ? m0.y1 : m0.y0) - scy;
          const float pu = dx * cs - dy * sn, pv = dx * sn + dy * cs;
          au = fminf(au, pu);
          bu = fmaxf(bu, pu);
          av = fminf(av, pv);
          bv = fmaxf(bv, pv);
        }
        sep = bu + mg < -tcx || au - mg > (sw - 1) - tcx || bv + mg < -tcy || av - mg > (sh - 1) - tcy;
      }
      d = !sep;
    }
  }
  dep[s] = d;
  indep[s] = !d;
}

// flip every sheet the two-mask launch rotated
// Zero the first n column sums of the sheets whose rotation is active (the
// rotate kernel accumulates theirs; the others keep the previous scan's).
__global__ void k_zero_sums_if_active(const RotateArgs* args, uint32_t* sums, int64_t stride,
                                      int32_t n) {
  const int s = blockIdx.y;
  if (!args[s].active) return;
  for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    sums[s * stride + i] = 0;
}

__global__ void k_flip_rot2(SheetCtl* ctl, const RotateArgs* args, int64_t mstride,
                            const int32_t* indep, int count) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= count) return;
  if (args[s].active || (args[mstride + s].active && indep[s])) ctl[s].cur ^= 1;
}

// detect_edge_rotation's argmax + detect_rotation_cpu's combination -> RotateArgs
// for deskew.  <= 2 edges: the host-computed table (host libm); > 2 edges:
// deskew.c:219-240 and :260-261 on the device with glibc's sinf/cosf/powf
// restated bit for bit (libm_glibc.h).  `only`
// only (may be null): other sheets get an inactive RotateArgs and keep their ctl.
// One wave per sheet: the lanes scan the angles in strides, then a wave
// reduction keeps the largest peak and, among equal ones, the first angle --
// the reference loop's `if (peak > max_peak)` from max_peak = 0 (an edge with
// no positive peak keeps angle 0).
// rot_all (null in k_rot_select): a rotation for every mask, [s * a.max_masks + i]
// (k_rot_select_all, more than two points).
__device__ __forceinline__ void rot_select(SheetCtl* ctl, const int32_t* peaks,
                                           const RotTable* table, const RotCombo* combo,
                                           const RotSelectArgs& a, RotateArgs* out, int count,
                                           const int32_t* only, const uint32_t* pow2, int npow2,
                                           float* rot_all) {
  const int s = blockIdx.x, lane = threadIdx.x;
  if (s >= count) return;
  if (only && !only[s]) {
    if (lane == 0) out[s].active = 0;
    return;
  }
  SheetCtl& c = ctl[s];
  const int i = a.mask_index;
  const bool active = i < c.mask_count;
  int idx[4] = {0, 0, 0, 0};
  for (int e = 0; e < a.nedges; e++) {
    const int32_t* pk = peaks + (((int64_t)s * a.max_masks + i) * 4 + e) * a.nangles;
    int best = 0, bi = 0;
    for (int k = lane; k < a.nangles; k += 64) {
      const int v = pk[k];
      if (v > best) {
        best = v;
        bi = k;
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const int ob = __shfl_xor(best, o, 64), oi = __shfl_xor(bi, o, 64);
      if (ob > best || (ob == best && oi < bi)) {
        best = ob;
        bi = oi;
      }
    }
    idx[e] = best > 0 ? bi : 0;
  }
  if (lane != 0) return;
  RotCombo r;
  if (a.nedges <= 2) {
    int key = 0;
    if (a.nedges >= 1) key = idx[0];
    if (a.nedges == 2) key = idx[0] * a.nangles + idx[1];
    r = combo[key];
  } else {
    // > 2 edges: the reference's float expressions in its order, IEEE division
    // and square root, glibc's powf(d, 2) and sinf/cosf (libm_glibc.h)
    float rot[4], total = 0.0f;
    for (int e = 0; e < a.nedges; e++) {
      const float v = table->angle[idx[e]];
      rot[e] = a.negate[e] ? -v : v;
      total += rot[e];
    }
    const float avg = __fdiv_rn(total, (float)a.nedges);
    float t2 = 0.0f;
    for (int e = 0; e < a.nedges; e++) t2 += glibc::pow2(rot[e] - avg, pow2, npow2);
    r.result = __fsqrt_rn(t2) <= a.deviation_rad ? avg : 0.0f;
    r.sinv = glibc::sinf(-r.result);
    r.cosv = glibc::cosf(-r.result);
  }
  if (i < UPHIP_MAX_PAGES) c.rotation[i] = active ? r.result : 0.0f;
  if (rot_all) rot_all[(int64_t)s * a.max_masks + i] = active ? r.result : 0.0f;
  RotateArgs ra;
  ra.mask = to_rect(c.masks[i]);
  ra.sinval = r.sinv;
  ra.cosval = r.cosv;
  ra.active = active && r.result != 0.0f;
  out[s] = ra;
}

__global__ void __launch_bounds__(64) k_rot_select(SheetCtl* ctl, const int32_t* peaks,
                                                   const RotTable* table, const RotCombo* combo,
                                                   RotSelectArgs a, RotateArgs* out, int count,
                                                   const int32_t* only, const uint32_t* pow2,
                                                   int npow2) {
  rot_select(ctl, peaks, table, combo, a, out, count, only, pow2, npow2, nullptr);
}

__global__ void __launch_bounds__(64) k_rot_select_all(SheetCtl* ctl, const int32_t* peaks,
                                                       const RotTable* table, const RotCombo* combo,
                                                       RotSelectArgs a, RotateArgs* out, int count,
                                                       const int32_t* only, const uint32_t* pow2,
                                                       int npow2, float* rot_all) {
  rot_select(ctl, peaks, table, combo, a, out, count, only, pow2, npow2, rot_all);
}

// center_mask (masks.c:222-249) for mask i -> MoveArgs
__global__ void k_center_args(const SheetCtl* ctl, int i, int32_t W, int32_t H, UphipPixel bg,
                              MoveArgs* out, int count) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= count) return;
  const SheetCtl& c = ctl[s];
  MoveArgs m;
  m.area = to_rect(c.masks[i]);
  const int32_t sw = iabs(m.area.x0 - m.area.x1) + 1, sh = iabs(m.area.y0 - m.area.y1) + 1;
  m.tx = c.points[i].x - sw / 2;
  m.ty = c.points[i].y - sh / 2;
  m.bg[0] = bg.r;
  m.bg[1] = bg.g;
  m.bg[2] = bg.b;
  const Rect na = rect_from_size(m.tx, m.ty, sw, sh);
  const Rect img{0, 0, W - 1, H - 1};
  bool active = i < c.mask_count && point_in(na.x0, na.y0, img) && point_in(na.x1, na.y1, img);
  // identity move: area inside the image, normalised, and target == origin
  const Rect n = normalize(m.area);
  const Rect cl = clip(m.area, W, H);
  if (active && n.x0 == m.area.x0 && n.y0 == m.area.y0 && cl.x0 == n.x0 && cl.y0 == n.y0 &&
      cl.x1 == n.x1 && cl.y1 == n.y1 && m.tx == n.x0 && m.ty == n.y0)
    active = false;
  m.active = active;
  out[s] = m;
}

// detect_border + border_to_mask + apply_masks args + align_mask args
// (masks.c:351-488, sheet_stages.c:480-499)
__global__ void k_border_assemble(SheetCtl* ctl, const int32_t* res, BorderAssembleArgs a,
                                  MaskArgs* masks_out, MoveArgs* move_out, int count) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= count) return;
  SheetCtl& c = ctl[s];
  MaskArgs& ma = masks_out[s];
  ma.n = a.nout;
  ma.color[0] = a.mask_color[0];
  ma.color[1] = a.mask_color[1];
  ma.color[2] = a.mask_color[2];
  for (int i = 0; i < a.nout; i++) {
    const Rect o = a.outside[i];
    const int32_t* r = res + ((int64_t)s * a.nout + i) * 4;
    int32_t left = o.x0, top = o.y0, right = a.W - o.x1, bottom = a.H - o.y1;
    if (a.horizontal) {
      left += r[0];
      right += r[1];
    }
    if (a.vertical) {
      top += r[2];
      bottom += r[3];
    }
    const Rect m{left, top, a.W - right - 1, a.H - bottom - 1};
    c.border_masks[i] = from_rect(m);
    ma.m[i] = m;
    // align_mask_cpu target (masks.c:265-290)
    const int32_t iw = iabs(m.x0 - m.x1) + 1, ih = iabs(m.y0 - m.y1) + 1;
    int32_t tx, ty;
    if (a.ap.alignment.left) tx = o.x0 + a.ap.margin.horizontal;
    else if (a.ap.alignment.right) tx = o.x1 - iw - a.ap.margin.horizontal;
    else tx = (o.x0 + o.x1 - iw) / 2;
    if (a.ap.alignment.top) ty = o.y0 + a.ap.margin.vertical;
    else if (a.ap.alignment.bottom) ty = o.y1 - ih - a.ap.margin.vertical;
    else ty = (o.y0 + o.y1 - ih) / 2;
    MoveArgs mv;
    mv.area = m;
    mv.tx = tx;
    mv.ty = ty;
    mv.bg[0] = a.bg[0];
    mv.bg[1] = a.bg[1];
    mv.bg[2] = a.bg[2];
    const Rect n = normalize(m);
    const Rect cl = clip(m, a.W, a.H);
    const bool identity = n.x0 == m.x0 && n.y0 == m.y0 && cl.x0 == n.x0 && cl.y0 == n.y0 &&
                          cl.x1 == n.x1 && cl.y1 == n.y1 && tx == n.x0 && ty == n.y0;
    mv.active = a.align && !identity;
    move_out[(int64_t)i * a.cap + s] = mv;
  }
}

// ---------------------------------------------------------------------------
// Stage helpers
// ---------------------------------------------------------------------------
namespace {

Planes planes_of(UphipBatch* b, int32_t w, int32_t h) {
  return Planes{{b->planes[0], b->planes[1]}, b->pitch, b->plane_stride, w, h, b->work_fmt, b->cap};
}

void mark(UphipBatch* b, const char* name) {
  if (!b->timing || b->runs.empty()) return;
  hipEvent_t e;
  hipEventCreate(&e);
  hipEventRecord(e, b->st);
  b->runs.back().push_back({name, e});
}

void flip_all(UphipBatch* b, int count) {
  hipLaunchKernelGGL(k_flip_all, dim3((count + 255) / 256), dim3(256), 0, b->st, b->ctl, count);
}

void fill(UphipBatch* b, const Planes& P, int which, const Fill& f, int count) {
  if (f.args)
    launch_fill_thr(PlaneRef{P, b->ctl, which}, f.args, count, f.rows, b->o.abs_black_threshold, b->st);
}

void wipe(UphipBatch* b, const Planes& P, const Wipes& w, int count) {
  for (int i = 0; i < w.n; i++) fill(b, P, 0, w.fill[i], count);
}

void apply_masks(UphipBatch* b, const Planes& P, const MaskArgs* m, int count) {
  if (m) launch_apply_masks_thr(cur_ref(P, b->ctl), m, count, b->o.abs_black_threshold, b->st);
}

// A size chain of the plan on every sheet, from w x h on: stretch_and_replace,
// resize_and_replace's centring in a background, flip_rotate_90 (blit.c:231-310)
void run_chain(UphipBatch* b, const SizeChain& c, int32_t w, int32_t h, int count) {
  const uint8_t thr = b->o.abs_black_threshold;
  for (int i = 0; i < c.n; i++) {
    const SizeStep& s = c.step[i];
    const PlaneRef S = cur_ref(planes_of(b, w, h), b->ctl);
    const Planes D = planes_of(b, s.w, s.h);
    if (s.kind == SizeStep::Stretch) {
      launch_stretch_thr(S, other_ref(D, b->ctl), b->o.interpolate_type, thr, count, b->st);
    } else if (s.kind == SizeStep::Rotate90) {  // only the post chain turns the sheet
      launch_rotate90_thr(S, other_ref(D, b->ctl), b->o.post_rotate / 90, thr, count, b->st);
    } else {
      fill(b, D, 1, s.fill, count);
      launch_copy_thr(S, other_ref(D, b->ctl), s.copy.args, count, s.copy.rows, thr, b->st);
    }
    flip_all(b, count);
    w = s.w;
    h = s.h;
  }
}

void mirror_shift(UphipBatch* b, const Planes& P, UphipDirection mirror, UphipDelta shift, int count) {
  const UphipOptions& o = b->o;
  if (mirror.horizontal || mirror.vertical) {
    launch_mirror_oop(cur_ref(P, b->ctl), other_ref(P, b->ctl), mirror.horizontal, mirror.vertical,
                      o.abs_black_threshold, count, b->st);
    flip_all(b, count);
  }
  if (shift.horizontal != 0 || shift.vertical != 0) {
    const uint8_t bg[3] = {o.sheet_background.r, o.sheet_background.g, o.sheet_background.b};
    launch_shift(cur_ref(P, b->ctl), other_ref(P, b->ctl), shift.horizontal, shift.vertical, bg,
                 o.abs_black_threshold, count, b->st);
    flip_all(b, count);
  }
}

// detect_masks on every sheet -> ctl.masks / ctl.mask_count (masks.c:54-209).
// sums_ready: point 0's horizontal column sums are already in b->sums
// (mask_sums_from_gray, mask_sums_from_rotate).
void detect_masks_all(UphipBatch* b, int count, bool sums_ready) {
  const UphipMaskDetectionParameters& p = b->mask_params;
  if (!p.scan_direction.horizontal && !p.scan_direction.vertical) return;
  const auto& A = b->args.mask_scan;
  const int np = (int)b->points.size();
  const int32_t W = b->W, H = b->H;
  const PlaneRef R = cur_ref(planes_of(b, W, H), b->ctl);
  const bool one_launch = np > 2 && b->mask_scan_route == 0;
  if (one_launch)  // every entry the scans read is stored: nothing to clear
    launch_mask_sums_points(R, A.bands, np, W, H, A.band_cols, b->sums, b->sums_stride, count, b->st);
  if (!sums_ready && !one_launch)
    UPH_HIP(hipMemsetAsync(b->sums, 0, sizeof(uint32_t) * b->sums_stride * count, b->st));
  for (int i = 0; i < np && !one_launch; i++) {
    uint32_t* sums = b->sums + (2 * i) * imax(W, H);
    if (A.sums[i].h && !(sums_ready && i == 0))
      launch_axis_reduce(R, A.sums[i].h, 0, M_GRAY_SUM, W, H, sums, b->sums_stride, count, b->st);
    if (A.sums[i].v)
      launch_axis_reduce(R, A.sums[i].v, 1, M_GRAY_SUM, W, H, sums + imax(W, H), b->sums_stride, count,
                         b->st);
  }
  launch_edge_scan(A.edges, np * 4, b->sums, b->sums_stride, b->edge_res, count, b->st, imax(W, H));
  hipLaunchKernelGGL(k_mask_assemble, dim3((count + 255) / 256), dim3(256), 0, b->st, b->ctl,
                     b->edge_res, A.assemble, count);
}

// The centring move's counting pass (border_rows_from_center): C's dark
// pixels per row over outside rect 0's columns into border_all's row sums.
MoveExtra center_count_args(const UphipBatch* b) {
  const Rect oc = clip(b->outside[0], b->W, b->H);
  MoveExtra x{};
  x.rows = b->sums + imax(b->W, b->H);  // border_all's vertical offset, outside rect 0
  x.rows_stride = b->sums_stride;
  x.rx0 = oc.x0;
  x.rx1 = oc.x1;
  x.thr = b->o.abs_black_threshold;
  return x;
}

// detect_border, apply_masks and align_mask on every sheet (masks.c:351-488,
// sheet_stages.c:478-488).  rows_ready: the vertical scan's row sums are
// already in b->sums (border_rows_from_center).  center: the chained centring
// move's arguments (chain_center_align), whose plane was never written.
void border_all(UphipBatch* b, int count, bool rows_ready, const MoveArgs* center) {
  const auto& A = b->args.border_scan;
  const int nout = (int)b->outside.size();
  const int32_t W = b->W, H = b->H;
  const Planes P = planes_of(b, W, H);
  if (!rows_ready)
    UPH_HIP(hipMemsetAsync(b->sums, 0, sizeof(uint32_t) * b->sums_stride * count, b->st));
  for (int i = 0; i < nout; i++) {
    uint32_t* sums = b->sums + (2 * i) * imax(W, H);
    if (A.sums[i].h)
      launch_axis_reduce(cur_ref(P, b->ctl), A.sums[i].h, 0, M_DARK_COUNT, W, H, sums, b->sums_stride,
                         count, b->st);
    if (A.sums[i].v && !rows_ready)
      launch_axis_reduce(cur_ref(P, b->ctl), A.sums[i].v, 1, M_DARK_COUNT, W, H, sums + imax(W, H),
                         b->sums_stride, count, b->st);
  }
  UPH_HIP(hipMemsetAsync(b->border_res, 0, sizeof(int32_t) * count * nout * 4, b->st));
  if (center && b->plan.border_edge_rows_only) {
    // rows [kBorderEdgeRows, H - kBorderEdgeRows) not counted yet: scan, count
    // them for the sheets that reach them, scan those again
    UPH_HIP(hipMemsetAsync(b->border_need, 0, sizeof(int32_t) * count, b->st));
    launch_border_scan(A.edges, nout * 4, b->sums, b->sums_stride, b->border_res, count, b->st,
                       imax(W, H), kBorderEdgeRows, H - kBorderEdgeRows, b->border_need);
    MoveExtra x = center_count_args(b);
    x.dry = true;
    x.ya0 = kBorderEdgeRows;
    x.ya1 = H - kBorderEdgeRows;
    x.only = b->border_need;
    launch_move_rect_fused(cur_ref(P, b->ctl), other_ref(P, b->ctl), center, x, count, b->st);
    launch_border_scan(A.edges, nout * 4, b->sums, b->sums_stride, b->border_res, count, b->st,
                       imax(W, H), 0, 0, nullptr, b->border_need);
  } else {
    launch_border_scan(A.edges, nout * 4, b->sums, b->sums_stride, b->border_res, count, b->st,
                       imax(W, H));
  }
  hipLaunchKernelGGL(k_border_assemble, dim3((count + 255) / 256), dim3(256), 0, b->st, b->ctl,
                     b->border_res, A.assemble, b->border_mask_args, b->move_args, count);
  // apply_masks then align_mask (sheet_stages.c:478-488): with one outside
  // rectangle on a gray plane, one pass -- the move writes the mask colour
  // outside the border mask (and masks in place where the move is the
  // identity)
  const bool align = A.assemble.align;
  const bool fold = align && nout == 1 && P.fmt == F_GRAY8;
  if (center) {
    // every sheet's output written to the other plane: flip them all
    launch_move_chain(cur_ref(P, b->ctl), other_ref(P, b->ctl), center, b->border_mask_args,
                      b->move_args, count, b->st);
    flip_all(b, count);
    return;
  }
  if (!fold) apply_masks(b, P, b->border_mask_args, count);
  for (int i = 0; i < nout && align; i++) {
    MoveArgs* mv = b->move_args + (int64_t)i * b->cap;
    if (fold) {
      MoveExtra x{};
      x.masks = b->border_mask_args;
      launch_move_rect_fused(cur_ref(P, b->ctl), other_ref(P, b->ctl), mv, x, count, b->st);
    } else {
      launch_move_rect(cur_ref(P, b->ctl), other_ref(P, b->ctl), mv, count, b->st);
    }
    launch_flip_if_active(b->ctl, &mv->active, sizeof(MoveArgs), count, b->st);
  }
}

// The decode may also produce the noisefilter's dark bit-plane, the
// blurfilter's bit-plane and the blackfilter's match plane (k_decode_gray,
// k_decode_gray_fit) when a GRAY8 page is placed in the sheet and nothing
// writes the sheet between the decode and the filters (sheet_stages.c:187-325:
// pre-mirror, -shift, -masks, -stretch/size, -wipes, -border all off).  The
// alignment of the pages a run is given decides with the options, so this is
// asked per run.
bool decode_fusable(const UphipBatch* b, const uint8_t* src, int64_t spitch, int64_t sstride) {
  const UphipOptions& o = b->o;
  const uint32_t dis = o.disable;
  if (b->work_fmt != F_GRAY8 || b->geo.page_format != F_GRAY8 || b->n_in != 1) return false;
  if (o.pre_rotate != 0) return false;
  if (b->sheet_w != b->W || b->sheet_h != b->H) return false;  // stretch / page size
  // 16-byte vector loads at src + s*sstride + y*spitch (a row's last vector
  // may read up to 15 bytes past the row within its pitch)
  if (((uintptr_t)src & 15) || (spitch & 15) || (sstride & 15)) return false;
  if (o.pre_mirror.horizontal || o.pre_mirror.vertical) return false;
  if (o.pre_shift.horizontal != 0 || o.pre_shift.vertical != 0 || o.pre_mask_count > 0) return false;
  if (!(dis & UPHIP_NO_WIPE) && o.pre_wipes.count > 0) return false;
  if (!(dis & UPHIP_NO_BORDER) &&
      (o.pre_border.left || o.pre_border.top || o.pre_border.right || o.pre_border.bottom))
    return false;
  return true;
}

// The deskew of every sheet (sheet_stages.c:388-413); returns whether the
// rotation left the second mask scan's column sums in b->sums.
bool deskew_all(UphipBatch* b, const Planes& P, int count) {
  const UphipOptions& o = b->o;
  const RotGeom& rg = b->args.deskew.geom;
  bool center_sums_ready = false;
  // detection of mask i (mask_pick, peaks, select) into rot_args[i]
  auto detect = [&](int i, const int32_t* only) {
    hipLaunchKernelGGL(k_mask_pick, dim3((count + 255) / 256), dim3(256), 0, b->st, b->ctl, i,
                       b->pick_mask, b->pick_active, count, only);
    launch_rotation_peaks(cur_ref(P, b->ctl), rg, b->dtable, b->pick_mask, b->pick_active, i,
                          b->peaks, count, b->st, b->table.nangles, b->max_scan, b->rot_lines,
                          b->max_angle);
#ifdef UPHIP_DIAG
    if (getenv("UPHIP_DIAG_ROTATION")) {  // tuning build only: lines left to the direct walk
      const int nl = count * rg.nedges * b->table.nangles;
      std::vector<int32_t> fl((size_t)nl);
      UPH_HIP(hipMemcpyAsync(fl.data(), rotation_line_flags(b->rot_lines, nl, b->max_scan),
                             sizeof(int32_t) * nl, hipMemcpyDeviceToHost, b->st));
      UPH_HIP(hipStreamSynchronize(b->st));
      int nf = 0;
      for (int t = 0; t < nl; t++) nf += fl[t] != 0;
      fprintf(stderr, "uphip: batch rotation %d of %d lines walked directly\n", nf, nl);
    }
#endif
    RotSelectArgs ra = b->args.deskew.select;
    ra.mask_index = i;
    if (b->points.size() > 2)  // a rotation kept for every mask
      hipLaunchKernelGGL(k_rot_select_all, dim3(count), dim3(64), 0, b->st, b->ctl,
                         b->peaks, b->dtable, b->dcombo, ra, b->rot_args + (int64_t)i * b->cap,
                         count, only, b->dpow2, b->npow2, b->rot_all);
    else
      hipLaunchKernelGGL(k_rot_select, dim3(count), dim3(64), 0, b->st, b->ctl,
                         b->peaks, b->dtable, b->dcombo, ra, b->rot_args + (int64_t)i * b->cap,
                         count, only, b->dpow2, b->npow2);
  };
  // rotations are angles of the scan table, |angle| <= scan range
  auto rotate = [&](const RotateArgs* args, int nmask, const int32_t* indep,
                    uint32_t* colsum = nullptr) {
    if (b->plan.linear && launch_rotate_linear(cur_ref(P, b->ctl), other_ref(P, b->ctl), args, nmask,
                                               b->cap, indep, count, b->st, b->max_angle))
      return false;
    return launch_rotate_mask(cur_ref(P, b->ctl), other_ref(P, b->ctl), args,
                              o.interpolate_type, count, b->st, b->max_angle, b->rot_scratch,
                              colsum, b->sums_stride);
  };
  if (b->plan.linear && b->points.size() == 2) {
    // both masks detected on the same image, rotated in one launch where
    // independent (k_rot_independent); mask 1 again after mask 0 elsewhere
    detect(0, nullptr);
    detect(1, nullptr);
    hipLaunchKernelGGL(k_rot_independent, dim3((count + 255) / 256), dim3(256), 0, b->st,
                       b->ctl, b->rot_args, (int64_t)b->cap, b->rot_indep, b->rot_dep, count);
    mark(b, "deskew_detect");
    rotate(b->rot_args, 2, b->rot_indep);
    mark(b, "deskew_rotate");  // brackets exactly the rotation kernel
    hipLaunchKernelGGL(k_flip_rot2, dim3((count + 255) / 256), dim3(256), 0, b->st, b->ctl,
                       b->rot_args, (int64_t)b->cap, b->rot_indep, count);
    RotateArgs* a1 = b->rot_args + b->cap;
    detect(1, b->rot_dep);
    mark(b, "deskew_detect");
    rotate(a1, 1, nullptr);
    mark(b, "deskew_rotate");
    launch_flip_if_active(b->ctl, &a1->active, sizeof(RotateArgs), count, b->st);
    return false;
  }
  for (size_t i = 0; i < b->points.size(); i++) {
    detect((int)i, nullptr);
    RotateArgs* ai = b->rot_args + (int64_t)i * b->cap;
    const bool fuse = b->plan.mask_sums_from_rotate;
    if (fuse)
      hipLaunchKernelGGL(k_zero_sums_if_active, dim3(4, count), dim3(256), 0, b->st, ai,
                         b->sums, b->sums_stride, b->W);
    mark(b, "deskew_detect");
    center_sums_ready = rotate(ai, 1, nullptr, fuse ? b->sums : nullptr);
    mark(b, "deskew_rotate");  // brackets exactly the rotation kernel
    launch_flip_if_active(b->ctl, &ai->active, sizeof(RotateArgs), count, b->st);
  }
  return center_sums_ready;
}

}  // namespace

// ---------------------------------------------------------------------------
// run
// ---------------------------------------------------------------------------
bool run_batch(UphipBatch* b, int count, const uint8_t* src, int64_t spitch, int64_t sstride) {
  const UphipOptions& o = b->o;
  const uint32_t dis = o.disable;
  const BatchPlan& plan = b->plan;
  const BatchArgs& A = b->args;
  if (b->timing) b->runs.emplace_back();
  mark(b, "start");
  const UphipPoint p0 = b->points.size() > 0 ? b->points[0] : UphipPoint{0, 0};
  const UphipPoint p1 = b->points.size() > 1 ? b->points[1] : UphipPoint{0, 0};
  hipLaunchKernelGGL(k_ctl_init, dim3((count + 255) / 256), dim3(256), 0, b->st, b->ctl, count,
                     (int32_t)b->points.size(), p0, p1);
  if (b->points.size() > 2)
    hipLaunchKernelGGL(k_ctl_points, dim3(count), dim3(64), 0, b->st, b->ctl, count,
                       (int32_t)b->points.size(), b->dpoints, b->rot_all);
  // ---- decode: pages -> working sheet (sheet_stages.c:44-185) ----------
  const int n = b->n_in;  // pages a sheet
  const Planes S0 = planes_of(b, b->sheet_w, b->sheet_h);
  // the slots' page sizes, when a run was given some: their placements go up
  // once per change, and decide with the plan which decode this run takes
  const bool sized = !b->slot_w.empty();
  if (sized && b->place_dirty) {
    for (int j = 0; j < n; j++)
      UPH_HIP(hipMemcpyAsync(const_cast<CopyArgs*>(A.decode.page[j].args), b->place[j].data(),
                             sizeof(CopyArgs) * b->cap, hipMemcpyHostToDevice, b->st));
    b->place_dirty = false;
  }
  const bool identity = sized ? count <= b->identity_sheets : plan.covered;
  const bool covered = sized ? count <= b->covered_sheets : plan.covered;
  const bool fused = decode_fusable(b, src, spitch, sstride);
  b->route = !fused ? 0 : identity ? 1 : 2;
  SheetBits bits;  // what the fused decode hands on
  if (fused) {
    const bool black_on = !(dis & UPHIP_NO_BLACKFILTER) && b->bgeo.nbars > 0;
    bits.nbits = !(dis & UPHIP_NO_NOISEFILTER) ? b->nbits : nullptr;
    bits.bbits = !(dis & UPHIP_NO_BLURFILTER) ? b->bbits : nullptr;
    bits.stride = b->nbits_stride;
    // the v-stripe sums are read from the pages, which are the sheet only
    // under the identity: a placed sheet is summed by the blackfilter itself
    bits.vsum = identity && black_on && b->bgeo.vregion.x1 >= b->bgeo.vregion.x0;
    bits.rm = black_on;
    if (identity)
      launch_decode_gray(src, spitch, sstride, cur_ref(S0, b->ctl), o.abs_white_threshold, bits,
                         b->bgeo, b->scr, b->scr_stride, count, b->st);
    else
      launch_decode_gray_fit(src, spitch, sstride, A.decode.page[0].args,
                             gray_of(Px{o.sheet_background.r, o.sheet_background.g, o.sheet_background.b}),
                             cur_ref(S0, b->ctl), o.abs_white_threshold, bits, b->bgeo, b->scr,
                             b->scr_stride, count, b->st);
  }
  if (!fused && !covered) fill(b, S0, 0, A.decode.sheet, count);
  for (int j = 0; j < n && !fused; j++) {
    uint8_t* const page = const_cast<uint8_t*>(src) + j * sstride;
    Planes pg{{page, page}, spitch, sstride * n, b->geo.page_width, b->geo.page_height, b->geo.page_format, count};
    if (o.pre_rotate != 0) {
      const int64_t rpitch = round_pitch(row_bytes(b->rp_w, pg.fmt));
      const Planes rp{{b->rot_page, b->rot_page}, rpitch, rpitch * b->rp_h, b->rp_w, b->rp_h, pg.fmt, count};
      launch_rotate90_thr(fixed_ref(pg, 0), fixed_ref(rp, 0), o.pre_rotate / 90,
                          o.abs_black_threshold, count, b->st);
      pg = rp;
    }
    launch_copy_thr(fixed_ref(pg, 0), cur_ref(S0, b->ctl), A.decode.page[j].args, count,
                    A.decode.page[j].rows, o.abs_black_threshold, b->st);
  }
  mark(b, "decode");
  // ---- pre (sheet_stages.c:187-325) -----------------------------------
  mirror_shift(b, S0, o.pre_mirror, o.pre_shift, count);
  apply_masks(b, S0, A.pre.masks, count);
  run_chain(b, plan.pre, b->sheet_w, b->sheet_h, count);
  const Planes P = planes_of(b, b->W, b->H);
  wipe(b, P, A.pre.wipes, count);
  apply_masks(b, P, A.pre.border, count);
  mark(b, "pre");
  // ---- filters (sheet_stages.c:327-357) ---------------------------------
  if (!(dis & UPHIP_NO_BLACKFILTER) && b->bgeo.nbars > 0) {
    launch_blackfilter(cur_ref(P, b->ctl), b->bgeo, b->dbars, b->scr, b->scr_stride, b->ctl, count,
                       b->st, b->black_h, b->black_v, bits);
    mark(b, "blackfilter");
  }
  if (!(dis & UPHIP_NO_NOISEFILTER)) {
    launch_noisefilter(cur_ref(P, b->ctl), b->ngeo, b->scr, b->scr_stride, b->ctl, count, b->st,
                       bits);
    mark(b, "noisefilter");
  }
  if (!(dis & UPHIP_NO_BLURFILTER)) {
    launch_blurfilter(cur_ref(P, b->ctl), b->blgeo, b->scr, b->scr_stride, count, b->st, bits);
    mark(b, "blurfilter");
  }
  bool mask_sums_ready = false;
  bool center_sums_ready = false;  // the second scan's sums came with the rotation
  // ---- masks (sheet_stages.c:359-386): the first detection is dead for a
  // fresh job (its count is discarded and its masks are overwritten before
  // any read), so it is skipped; mask_count is 0 -> no apply_masks.
  if (!(dis & UPHIP_NO_GRAYFILTER)) {
    uint32_t* cs = nullptr;
    if (plan.mask_sums_from_gray) {
      UPH_HIP(hipMemsetAsync(b->sums, 0, sizeof(uint32_t) * b->sums_stride * count, b->st));
      cs = b->sums;  // point 0, horizontal: offset 0
    }
    mask_sums_ready = launch_grayfilter(cur_ref(P, b->ctl), b->ggeo, b->scr, b->scr_stride, count,
                                        b->st, cs, b->sums_stride);
    mark(b, "grayfilter");
  }
  // ---- deskew (sheet_stages.c:388-413) ---------------------------------
  if (!(dis & UPHIP_NO_DESKEW)) {
    if (!(dis & UPHIP_NO_MASK_SCAN)) {
      detect_masks_all(b, count, mask_sums_ready);
      mark(b, "masks_deskew");
    }
    center_sums_ready = deskew_all(b, P, count);
  }
  // ---- post (sheet_stages.c:415-534) -------------------------------------
  const bool chain = plan.chain_center_align;
  MoveArgs* const center_mv = chain ? b->move_args + b->cap : nullptr;  // align uses [0, cap)
  if (!(dis & UPHIP_NO_MASK_CENTER)) {
    if (!(dis & UPHIP_NO_MASK_SCAN)) {
      detect_masks_all(b, count, center_sums_ready);
      mark(b, "masks_center");
    }
    for (size_t i = 0; i < b->points.size(); i++) {
      MoveArgs* mv = chain ? center_mv : b->move_args;  // reuse the first cap entries
      hipLaunchKernelGGL(k_center_args, dim3((count + 255) / 256), dim3(256), 0, b->st, b->ctl,
                         (int)i, b->W, b->H, o.sheet_background, mv, count);
      if (plan.border_rows_from_center && i + 1 == b->points.size()) {
        // the last move also counts the border scan's dark pixels per row
        MoveExtra x = center_count_args(b);
        x.dry = chain;  // chained: count C's rows from R, write nothing
        if (chain && plan.border_edge_rows_only) {  // the rows near the edges first
          x.ya0 = 0;
          x.ya1 = kBorderEdgeRows;
          x.yb0 = b->H - kBorderEdgeRows;
          x.yb1 = b->H;
        }
        launch_move_rect_fused(cur_ref(P, b->ctl), other_ref(P, b->ctl), mv, x, count, b->st);
      } else {
        launch_move_rect(cur_ref(P, b->ctl), other_ref(P, b->ctl), mv, count, b->st);
      }
      if (!chain) launch_flip_if_active(b->ctl, &mv->active, sizeof(MoveArgs), count, b->st);
    }
    mark(b, "center");
  }
  wipe(b, P, A.post.wipes, count);
  apply_masks(b, P, A.post.border, count);
  if (!(dis & UPHIP_NO_BORDER_SCAN) && !b->outside.empty()) {
    border_all(b, count, plan.border_rows_from_center, center_mv);
    mark(b, "border");
  }
  wipe(b, P, A.post.post_wipes, count);
  apply_masks(b, P, A.post.post_border, count);
  mirror_shift(b, P, o.post_mirror, o.post_shift, count);
  run_chain(b, plan.post, b->W, b->H, count);
  // ---- output (sheet_stages.c:536-631, saveImage file.c:187-259) --------
  if (b->out) {
    const Planes O{{b->out, b->out}, b->out_pitch, b->out_stride, b->out_w, b->out_h, b->out_fmt, count};
    launch_copy_thr(cur_ref(planes_of(b, b->out_w, b->out_h), b->ctl), fixed_ref(O, 0), A.output.args,
                    count, A.output.rows, o.abs_black_threshold, b->st);
  }
  mark(b, "output");
  hipLaunchKernelGGL(k_status_fold, dim3((count + 255) / 256), dim3(256), 0, b->st, b->ctl, count,
                     b->sticky);
  b->last_count = count;
  return uphip_last_error() == nullptr;
}

}  // namespace uph
