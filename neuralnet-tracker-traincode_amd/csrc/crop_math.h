// The crop of one sample, shared by the batched crop kernels (warp.hip) and the closed-loop tracker's fused crop (track.hip): ONE statement of
// the view-ROI rule, of the ROI -> crop transform and of the bilinear sample.  The two files produce bitwise equal results because they
// run these functions, with their operands in memory in between exactly as the three separate launches leave them.
//
//   view_roi_row       : GeneralFocusRoi._compute_view_roi (:108-157) + torch.round(...).to(int32) (:205)
//                        INTEGER result, bit-exact: every float op is an explicitly rounded __f*_rn (no fma
//                        contraction) in the reference's order; rintf = round-half-to-even like torch.round.
//   roi_transform_row  : tr = unnorm(N) @ rot(angle) @ norm(N) @ remap(view_roi -> [0,N]^2), row-major 2x3   (:159-177)
//   warp_pixel         : bilinear(src, tr^-1 (j+.5, i+.5) - .5) * mul + add, zero padding
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ttk {

// roi[4] = (x0, y0, x1, y1), enlargement f, relative shift (rx, ry) -> out[4]
__device__ __forceinline__ void view_roi_row(const float* __restrict__ roi, float f, float rx, float ry, float bbs, int* __restrict__ out) {
  const float x0 = roi[0], y0 = roi[1], x1 = roi[2], y1 = roi[3];
  const float bw = __fsub_rn(x1, x0), bh = __fsub_rn(y1, y0);
  const float cx = __fmul_rn(0.5f, __fadd_rn(x1, x0)), cy = __fmul_rn(0.5f, __fadd_rn(y1, y0));
  const float size = __fmul_rn(fmaxf(bw, bh), f);
  const float wx = __fadd_rn(__fmul_rn(0.5f, fabsf(__fsub_rn(size, bw))), __fmul_rn(bbs, fminf(size, bw)));
  const float wy = __fadd_rn(__fmul_rn(0.5f, fabsf(__fsub_rn(size, bh))), __fmul_rn(bbs, fminf(size, bh)));
  const float tx = __fmul_rn(wx, rx), ty = __fmul_rn(wy, ry);
  const float hs = __fmul_rn(size, 0.5f);
  out[0] = (int)rintf(__fadd_rn(__fsub_rn(cx, hs), tx));
  out[1] = (int)rintf(__fadd_rn(__fsub_rn(cy, hs), ty));
  out[2] = (int)rintf(__fadd_rn(__fadd_rn(cx, hs), tx));
  out[3] = (int)rintf(__fadd_rn(__fadd_rn(cy, hs), ty));
}

// vr[4] -> m[6]; angles == nullptr: no rotation (angle 0)
__device__ __forceinline__ void roi_transform_row(const int* __restrict__ vr, const float* __restrict__ angles, int b, int N,
                                                  float* __restrict__ m) {
  const float x0 = (float)vr[0], y0 = (float)vr[1], x1 = (float)vr[2], y1 = (float)vr[3];
  const float sx = (float)N / (x1 - x0), sy = (float)N / (y1 - y0);
  const float ox = -x0 * sx, oy = -y0 * sy;  // remap
  const float a = angles ? angles[b] : 0.f, c = cosf(a), s = sinf(a), h = 0.5f * (float)N;
  // p -> (p - h)/h -> R -> *h + h   ==  R p + (h - R h)
  const float r00 = c, r01 = -s, r10 = s, r11 = c;
  const float t0 = h - (r00 * h + r01 * h), t1 = h - (r10 * h + r11 * h);
  m[0] = r00 * sx; m[1] = r01 * sy; m[2] = r00 * ox + r01 * oy + t0;
  m[3] = r10 * sx; m[4] = r11 * sy; m[5] = r10 * ox + r11 * oy + t1;
}

template <typename T>
__device__ __forceinline__ float fetch(const T* img, int H, int W, int y, int x) {
  return (x >= 0 && x < W && y >= 0 && y < H) ? (float)img[(size_t)y * W + x] : 0.f;
}

// output pixel (row i, column j) of the crop of `img` [Hs][Ws] under m[6] (image pixels -> crop pixels)
template <typename T>
__device__ __forceinline__ float warp_pixel(const T* __restrict__ img, int Hs, int Ws, const float* __restrict__ m, int i, int j, float mul,
                                            float add) {
  // No contraction by the compiler in here: every fused multiply-add is written as fmaf, every other product and sum is rounded on its
  // own.  Which products the compiler would contract otherwise depends on the code around these lines - it differs between their
  // vectorised and their scalar form - and two kernels that share this function must agree bit for bit.  The pattern is the one the
  // batched warp kernel has always been compiled to:
  //   det = (m0 m4) - (m1 m3);  u = fma((m4 px) - (m1 py), 1 / det, -.5);  v = fma(fma(m0, py, -(m3 px)), 1 / det, -.5)
  //   row = fma(v_0, 1 - ax, (v_1 ax));  val = (top (1 - ay)) + (bottom ay)
#pragma clang fp contract(off)
  const float det = m[0] * m[4] - m[1] * m[3];
  const float inv = 1.f / det;
  const float px = (float)j + 0.5f - m[2], py = (float)i + 0.5f - m[5];
  const float u = fmaf(m[4] * px - m[1] * py, inv, -0.5f);
  const float v = fmaf(fmaf(m[0], py, -(m[3] * px)), inv, -0.5f);
  const float fu = floorf(u), fv = floorf(v);
  const int x0 = (int)fu, y0 = (int)fv;
  const float ax = u - fu, ay = v - fv;
  const float v00 = fetch(img, Hs, Ws, y0, x0), v01 = fetch(img, Hs, Ws, y0, x0 + 1);
  const float v10 = fetch(img, Hs, Ws, y0 + 1, x0), v11 = fetch(img, Hs, Ws, y0 + 1, x0 + 1);
  const float top = fmaf(v00, 1.f - ax, v01 * ax), bottom = fmaf(v10, 1.f - ax, v11 * ax);
  const float val = top * (1.f - ay) + bottom * ay;
  return fmaf(val, mul, add);
}

}  // namespace ttk
