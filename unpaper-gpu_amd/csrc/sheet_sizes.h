// sheet_sizes.h — the size arithmetic of the sheet chain, in one place: the
// batch plan (pipeline_plan.hip) and the per-image operations (ops.hip) both
// take it from here.  Plain C++, no HIP.  The float expressions and their
// (int32_t) truncations are the reference's and must stay bit for bit.
#pragma once

#include <stdint.h>

namespace uph {

// compare_sizes, primitives.c:70-80
inline int compare_sizes(int32_t aw, int32_t ah, int32_t bw, int32_t bh) {
  if (ah == bh && aw == bw) return 0;
  return (ah < aw ? ah : aw) < (bh < bw ? bh : bw) ? -1 : 1;
}

// The size resize_and_replace stretches a w x h image to before it centres it
// in pw x ph (blit.c:246-266): the largest of its aspect that fits.
inline void aspect_fit(int32_t w, int32_t h, int32_t pw, int32_t ph, int32_t* sw, int32_t* sh) {
  const float hr = (float)pw / (float)w, vr = (float)ph / (float)h;
  *sw = pw;
  *sh = ph;
  if (hr < vr) *sh = (int32_t)(h * hr);
  else if (vr < hr) *sw = (int32_t)(w * vr);
}

// center_image's placement (blit.c:175-202) of a sw x sh source in the target
// rectangle tw x th at (tx, ty): a smaller source is centred, a larger one
// cropped about its centre.  (sx, sy) source origin, (tx, ty) target origin,
// w x h the copied size (the source area is still to be clipped).
struct Placement {
  int32_t sx, sy, tx, ty, w, h;
};
inline Placement center_in(int32_t sw, int32_t sh, int32_t tx, int32_t ty, int32_t tw, int32_t th) {
  Placement p{0, 0, tx, ty, sw, sh};
  if (sw <= tw) p.tx += (tw - sw) / 2;
  else {
    p.sx += (sw - tw) / 2;
    p.w = tw;
  }
  if (sh <= th) p.ty += (th - sh) / 2;
  else {
    p.sy += (sh - th) / 2;
    p.h = th;
  }
  return p;
}

}  // namespace uph
