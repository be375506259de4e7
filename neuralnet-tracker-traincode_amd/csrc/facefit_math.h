// Per-point and per-term arithmetic of the face-model fit (csrc/facefit.hip), forward and hand-derived backward, all in double.
// Host + device header like head_math.h: hipcc compiles it into facefit.hip, a host compiler can compile it alone.
//
// Reference: scripts/DsWflwFitFaceModel.ipynb, the cell that defines DeformableHeadFitting (`lossfunc`): per sample, with
// x = (q[4] in i,j,k,w order, c[3] = x, y, size, s[50]) and qh = q / |q|,
//   f(x) = (1/136) sum_p sum_{d in x,y} w_p huber_0.1(P_pd - Y_pd)          smooth_l1_loss(beta = 0.1) of the posed landmarks
//        + 1e-6 (1 - |q|)^2                                                   norm_constraint
//        + 0.01 * (-(1/150) log p_GMM(s))                                     shape_plausibility
//        + 10 exp(-c[2] / 0.05)                                               size_constraint
//   P = rigid_transformation_25d(qh, c[:2], c[2], keypts + sum_i s_i keyeigvecs_i)   (neuralnets/modelcomponents.py:38-56)
#pragma once
#include <math.h>

#include "head_math.h"  // TTK_HD

namespace ttk {
namespace ff {

constexpr int kN = 57, kPose = 7, kShape = 50, kPts = 68, kEl = 204, kMaxK = 16;
constexpr double kBeta = 0.1, kNormWeight = 1.0e-6, kGmmWeight = 0.01, kGmmFudge = 1.0 / 150.0, kSizeWeight = 10.0, kSizeScale = 0.05;
constexpr double kPointNorm = 1.0 / 136.0;  // the mean over 68 points x 2 coordinates

// smooth_l1_loss(beta): r^2 / (2 beta) inside |r| < beta, |r| - beta / 2 outside; and its derivative (0 at r = 0)
TTK_HD double huber(double r, double beta) {
  const double a = fabs(r);
  return a < beta ? 0.5 * r * r / beta : a - 0.5 * beta;
}
TTK_HD double huber_d(double r, double beta) {
  const double a = fabs(r);
  return a < beta ? r / beta : (r > 0.0 ? 1.0 : (r < 0.0 ? -1.0 : r));  // (a NaN residual stays NaN)
}

// the pose of one sample: the normalised quaternion and the coordinates
struct Pose {
  double qi, qj, qk, qw;  // qh = q / |q|
  double cx, cy, size;
};
// the gradient with respect to qh and c that the points accumulate (plus the data term's value)
struct PoseGrad {
  double f, qi, qj, qk, qw, cx, cy, size;
};

// q (t, 0) q* for a unit q: (w^2 - |v|^2) t + 2 (v.t) v + 2 w (v x t)   (neuralnets/torchquaternion.py:51-67)
TTK_HD void rotate(const Pose& p, double t0, double t1, double t2, double& r0, double& r1, double& r2) {
  const double vv = p.qi * p.qi + p.qj * p.qj + p.qk * p.qk, vt = p.qi * t0 + p.qj * t1 + p.qk * t2;
  const double a = p.qw * p.qw - vv;
  r0 = a * t0 + 2.0 * vt * p.qi + 2.0 * p.qw * (p.qj * t2 - p.qk * t1);
  r1 = a * t1 + 2.0 * vt * p.qj + 2.0 * p.qw * (p.qk * t0 - p.qi * t2);
  r2 = a * t2 + 2.0 * vt * p.qk + 2.0 * p.qw * (p.qi * t1 - p.qj * t0);
}

// One landmark: P = rotate(local) * size + (cx, cy, 0).
TTK_HD void point_fwd(const Pose& p, double t0, double t1, double t2, double& P0, double& P1, double& P2) {
  double r0, r1, r2;
  rotate(p, t0, t1, t2, r0, r1, r2);
  P0 = r0 * p.size + p.cx;
  P1 = r1 * p.size + p.cy;
  P2 = r2 * p.size;
}

// One landmark of the data term: adds w huber(P_xy - Y) / 136 to g.f, its gradient to g, and writes the gradient with respect to the
// local point (gl0..2).  The derivative of rotate with respect to (v, w) is taken for the quadratic form above, i.e. without the unit
// constraint; the caller projects it through the normalisation (quat_norm_bwd).
TTK_HD void point_term(const Pose& p, double t0, double t1, double t2, double y0, double y1, double w, PoseGrad& g, double& gl0,
                       double& gl1, double& gl2) {
  double r0, r1, r2;
  rotate(p, t0, t1, t2, r0, r1, r2);
  const double e0 = r0 * p.size + p.cx - y0, e1 = r1 * p.size + p.cy - y1;
  g.f += w * (huber(e0, kBeta) + huber(e1, kBeta)) * kPointNorm;
  const double gP0 = w * huber_d(e0, kBeta) * kPointNorm, gP1 = w * huber_d(e1, kBeta) * kPointNorm;
  g.cx += gP0;
  g.cy += gP1;
  g.size += gP0 * r0 + gP1 * r1;
  const double h0 = gP0 * p.size, h1 = gP1 * p.size;  // gradient with respect to the rotated point; its z component is 0
  const double vt = p.qi * t0 + p.qj * t1 + p.qk * t2, th = t0 * h0 + t1 * h1, vh = p.qi * h0 + p.qj * h1;
  // d/dw: h . (2 w t + 2 v x t)
  g.qw += 2.0 * (p.qw * th + h0 * (p.qj * t2 - p.qk * t1) + h1 * (p.qk * t0 - p.qi * t2));
  // d/dv: -2 (t.h) v + 2 (v.h) t + 2 (v.t) h + 2 w (t x h),  t x h = (-t2 h1, t2 h0, t0 h1 - t1 h0)
  g.qi += 2.0 * (-th * p.qi + vh * t0 + vt * h0 + p.qw * (-t2 * h1));
  g.qj += 2.0 * (-th * p.qj + vh * t1 + vt * h1 + p.qw * (t2 * h0));
  g.qk += 2.0 * (-th * p.qk + vh * t2 + p.qw * (t0 * h1 - t1 * h0));
  // d/dt = R^T h: (w^2 - |v|^2) h + 2 (v.h) v - 2 w (v x h),  v x h = (-qk h1, qk h0, qi h1 - qj h0)
  const double a = p.qw * p.qw - (p.qi * p.qi + p.qj * p.qj + p.qk * p.qk);
  gl0 = a * h0 + 2.0 * vh * p.qi - 2.0 * p.qw * (-p.qk * h1);
  gl1 = a * h1 + 2.0 * vh * p.qj - 2.0 * p.qw * (p.qk * h0);
  gl2 = 2.0 * vh * p.qk - 2.0 * p.qw * (p.qi * h1 - p.qj * h0);
}

// qh = q / |q| and 1e-6 (1 - |q|)^2.  Returns the term's value.
TTK_HD double quat_norm_fwd(double q0, double q1, double q2, double q3, Pose& p, double& n) {
  n = sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
  p.qi = q0 / n; p.qj = q1 / n; p.qk = q2 / n; p.qw = q3 / n;
  return kNormWeight * (1.0 - n) * (1.0 - n);
}
// gradient with respect to q of (terms of qh with gradient g) + 1e-6 (1 - n)^2:  (g - qh (qh.g)) / n - 2e-6 (1 - n) qh
TTK_HD void quat_norm_bwd(const Pose& p, double n, const PoseGrad& g, double& g0, double& g1, double& g2, double& g3) {
  const double d = p.qi * g.qi + p.qj * g.qj + p.qk * g.qk + p.qw * g.qw, c = -2.0 * kNormWeight * (1.0 - n);
  g0 = (g.qi - p.qi * d) / n + c * p.qi;
  g1 = (g.qj - p.qj * d) / n + c * p.qj;
  g2 = (g.qk - p.qk * d) / n + c * p.qk;
  g3 = (g.qw - p.qw * d) / n + c * p.qw;
}

// 10 exp(-size / 0.05) and its derivative
TTK_HD double size_term(double size, double& gsize) {
  const double e = kSizeWeight * exp(-size / kSizeScale);
  gsize = -e / kSizeScale;
  return e;
}

}  // namespace ff
}  // namespace ttk
