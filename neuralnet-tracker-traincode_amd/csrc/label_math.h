// Labels of one sample under a 2-D affine map (tensors/affinetrafo.py:37-148), shared by the label kernel of the crop (warp.hip) and the
// ensemble reduction (ensemble.hip): one statement of the formulas and of the 68-point flip map.
#pragma once
#include "head_math.h"

namespace ttk {

// 68-landmark left/right partner under a horizontal mirror (facemodel/keypoints68.py:7-77)
static __constant__ unsigned char kFlipMap[68] = {16, 15, 14, 13, 12, 11, 10, 9,  8,  7,  6,  5,  4,  3,  2,  1,  0,  26, 25, 24, 23, 22, 21,
                                           20, 19, 18, 17, 27, 28, 29, 30, 35, 34, 33, 32, 31, 45, 44, 43, 42, 47, 46, 39, 38, 37, 36,
                                           41, 40, 54, 53, 52, 51, 50, 49, 48, 59, 58, 57, 56, 55, 64, 63, 62, 61, 60, 67, 66, 65};

struct Aff {
  float a, b, tx, c, d, ty;
  __device__ __forceinline__ float det() const { return a * d - b * c; }
  __device__ __forceinline__ float scale() const { return sqrtf(a * a + b * b + c * c + d * d) * 0.70710678118654752440f; }
};

// labels of one sample under `m` (tensors/affinetrafo.py: transform_coord :107-114, transform_rot :117-148,
// transform_roi :91-104, transform_points/keypoints :37-88).  pts_in/pts_out may alias only if det >= 0; likewise p2_in/p2_out, the
// 2-D landmark field [68][2] (transform_points :51-52, transform_keypoints :70-71: the same map and flip map without a depth).
__device__ void labels_under(const Aff m, float* coord, float* pose, float* roi, const float* pts_in, float* pts_out,
                             const float* p2_in, float* p2_out, int lane) {
  const float det = m.det();
  if (lane == 0) {
    if (coord) {
      const float x = coord[0], y = coord[1];
      coord[0] = m.a * x + m.b * y + m.tx;
      coord[1] = m.c * x + m.d * y + m.ty;
      coord[2] = m.scale() * coord[2];
    }
    if (pose) {
      const float sg = det > 0.f ? 1.f : (det < 0.f ? -1.f : 0.f);
      const float alpha = atan2f(-m.b, m.d);
      const hm::Q z{0.f, 0.f, sinf(0.5f * alpha) * sg, cosf(0.5f * alpha)};
      hm::Q o = hm::qmul(z, hm::Q{pose[0], pose[1], pose[2], pose[3]});
      pose[0] = o.i; pose[1] = sg * o.j; pose[2] = sg * o.k; pose[3] = o.w;
    }
    if (roi) {
      const float xs[2] = {roi[0], roi[2]}, ys[2] = {roi[1], roi[3]};
      float lo0 = 3.4e38f, lo1 = 3.4e38f, hi0 = -3.4e38f, hi1 = -3.4e38f;
      for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) {
          const float px = m.a * xs[i] + m.b * ys[j] + m.tx, py = m.c * xs[i] + m.d * ys[j] + m.ty;
          lo0 = fminf(lo0, px); hi0 = fmaxf(hi0, px); lo1 = fminf(lo1, py); hi1 = fmaxf(hi1, py);
        }
      roi[0] = lo0; roi[1] = lo1; roi[2] = hi0; roi[3] = hi1;
    }
  }
  if (pts_in) {
    const float zs = sqrtf(fabsf(det));
    for (int p = lane; p < 68; p += 64) {
      const int q = det < 0.f ? kFlipMap[p] : p;  // out[p] = transformed in[flip_map[p]]
      const float x = pts_in[3 * q], y = pts_in[3 * q + 1], z = pts_in[3 * q + 2];
      pts_out[3 * p] = m.a * x + m.b * y + m.tx;
      pts_out[3 * p + 1] = m.c * x + m.d * y + m.ty;
      pts_out[3 * p + 2] = zs * z;
    }
  }
  if (p2_in) {
    for (int p = lane; p < 68; p += 64) {
      const int q = det < 0.f ? kFlipMap[p] : p;
      const float x = p2_in[2 * q], y = p2_in[2 * q + 1];  // x / y as the 3-D field writes them: bitwise its x / y for equal inputs
      p2_out[2 * p] = m.a * x + m.b * y + m.tx;
      p2_out[2 * p + 1] = m.c * x + m.d * y + m.ty;
    }
  }
}

}  // namespace ttk
