// Device functions the face localizer (localizer.hip) shares with the closed-loop tracker (track.hip): the letterbox geometry, the
// map of the localizer's box to frame pixels, the face probability and the tracker's box rule.
#pragma once
#include <math.h>

#include "ttk_common.h"

namespace ttk {

constexpr int kLocH = 224, kLocW = 288;  // the localizer's input, H x W

// The tracker's box rule (include/ttk.h, ttk_track_update): candidate c = the box clamped to the image as the reference clamps it;
// valid iff the four values are finite (tested before the clamp: fmaxf(0, NaN) is 0), the clamped box has a positive width and
// height, and max(w, h) * factor >= 2.  (ttk_track_update additionally tests the order of the network's own box.)
__device__ __forceinline__ bool track_candidate(float x0, float y0, float x1, float y1, int Ws, int Hs, float factor, float c[4]) {
  const bool finite = isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1);
  c[0] = fmaxf(0.f, x0), c[1] = fmaxf(0.f, y0), c[2] = fminf(x1, (float)Ws), c[3] = fminf(y1, (float)Hs);
  const float w = c[2] - c[0], h = c[3] - c[1];
  return finite && w > 0.f && h > 0.f && fmaxf(w, h) * factor >= 2.f;
}

// The localizer's box in the input's [-1, 1] coordinates -> frame pixels under the letterbox lb = (s, ox, oy):
// input pixels X = (x + 1) * 144, Y = (y + 1) * 112; frame pixels ((X - ox) / s, (Y - oy) / s).  This project's convention.
__device__ __forceinline__ void localizer_box_to_frame(const float* box, const float* lb, float r[4]) {
  // (no contraction: every sum, product and quotient is rounded on its own, so that the host can restate the map bit for bit)
#pragma clang fp contract(off)
  const float s = lb[0], ox = lb[1], oy = lb[2];
  r[0] = ((box[0] + 1.f) * (0.5f * kLocW) - ox) / s;
  r[1] = ((box[1] + 1.f) * (0.5f * kLocH) - oy) / s;
  r[2] = ((box[2] + 1.f) * (0.5f * kLocW) - ox) / s;
  r[3] = ((box[3] + 1.f) * (0.5f * kLocH) - oy) / s;
}

__device__ __forceinline__ float face_probability(float logit) { return 1.f / (1.f + expf(-logit)); }

}  // namespace ttk
