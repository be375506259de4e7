// Fit of the deformable face model to 68 landmarks (reference: scripts/DsWflwFitFaceModel.ipynb / DsLapaMegafaceFitFaceModel.ipynb, class
// DeformableHeadFitting; the objective is restated in facefit_math.h).  The reference minimises it per sample on the CPU with two BFGS
// runs of the third-party torchmin; this is the project's own two-stage BFGS, one workgroup of ONE wave per sample,
// everything - state, reductions, point math - in float64:
//
//   stage 1 frees x[0:7] (pose) with the shape fixed, stage 2 all 57.  Per stage the inverse Hessian starts at I; one iteration is
//   d = -H g (H = I, d = -g when g.d >= 0), t = 1 (first iteration of a stage: min(1, 1 / |g|_1)), t halved at most 30 times until
//   f(x + t d) is finite and <= f + 1e-4 t g.d (none accepted: status 2, x unchanged), and the BFGS inverse update with s = t d,
//   y = g_new - g only when s.y > 1e-10 |s| |y|.  Status: 0 converged (|g|_inf <= gtol), 1 iteration limit, 2 line search, 3 non-finite
//   input or f(x0) (outputs = inputs, no iteration).
//
// Lanes.  An evaluation: the 204 local coordinates keypts + sum_i s_i keyeigvecs_i are formed by lane e mod 64 (coalesced reads of the
// float32 basis in global memory, which every workgroup shares in cache) into LDS; lane p owns landmark p and lanes 0..3 also 64 + p;
// the data term's value and its 7 pose gradients are folded with a fixed butterfly (every lane ends with the same bits); lane k < K sums
// the mixture energy of component k; lane i < 50 owns shape gradient i (its row of the basis against the 204 local gradients in LDS).
// H (57 x 57 doubles, 26 KB) and the vectors sit in LDS; lane r owns row r of H in the products and in the update.  Every short sum
// (g.d, s.y, ...) is serial in index order, computed redundantly by all lanes from LDS.  No atomics: two runs are bitwise equal.
// Every loop has an integer bound; no loop ends on a floating-point condition alone, so no input can hang a workgroup.
// Compiled without the SLP vectoriser like heads.hip (Makefile).
#include "facefit_math.h"
#include "ttk_common.h"

namespace ttk {

using namespace ff;

struct FfModel {
  const float* kp;     // [68][3]
  const float* eig;    // [50][68][3]
  const double* ck;    // [K]
  const double* mu;    // [K][50]
  const double* sinv;  // [K][50]
  int K;
};
// this lane's landmarks: p = lane and (lanes 0..3) p = 64 + lane, whose weight is 0 on the other lanes
struct FfData {
  double y0x, y0y, w0, y1x, y1y, w1;
};
struct FfScratch {
  double loc[kEl];   // local coordinates of the current evaluation
  double gl[kEl];    // gradient with respect to them
  double a[kMaxK];   // mixture energies ck - 0.5 |z_k|^2
};

__device__ __forceinline__ double ff_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// loc = keypts + sum_i xs[7 + i] keyeigvecs_i.  Barriers: before (xs complete, earlier readers of loc done) and after.
__device__ __forceinline__ void ff_local(const FfModel& m, const double* xs, FfScratch& sh, int lane) {
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int e = lane + kWave * k;
    if (e < kEl) {
      double acc = (double)m.kp[e];
      for (int i = 0; i < kShape; ++i) acc += xs[kPose + i] * (double)m.eig[i * kEl + e];
      sh.loc[e] = acc;
    }
  }
  if (lane < m.K) {
    double e = 0.0;
    for (int d = 0; d < kShape; ++d) {
      const double z = (xs[kPose + d] - m.mu[lane * kShape + d]) * m.sinv[lane * kShape + d];
      e += z * z;
    }
    sh.a[lane] = m.ck[lane] - 0.5 * e;
  }
  __syncthreads();
}

// f(xs) -> return value (the same bits in every lane); gs[0 .. 57) = gradient, entries beyond n_free written as 0.  xs, gs: LDS.
__device__ double ff_eval(const FfModel& m, const FfData& dt, const double* xs, int n_free, double* gs, FfScratch& sh, int lane) {
  ff_local(m, xs, sh, lane);
  Pose p;
  double n;
  double f = quat_norm_fwd(xs[0], xs[1], xs[2], xs[3], p, n);
  p.cx = xs[4]; p.cy = xs[5]; p.size = xs[6];
  PoseGrad g{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  {
    double a, b, c;
    point_term(p, sh.loc[3 * lane], sh.loc[3 * lane + 1], sh.loc[3 * lane + 2], dt.y0x, dt.y0y, dt.w0, g, a, b, c);
    sh.gl[3 * lane] = a; sh.gl[3 * lane + 1] = b; sh.gl[3 * lane + 2] = c;
    if (lane < kPts - kWave) {
      const int q = kWave + lane;
      point_term(p, sh.loc[3 * q], sh.loc[3 * q + 1], sh.loc[3 * q + 2], dt.y1x, dt.y1y, dt.w1, g, a, b, c);
      sh.gl[3 * q] = a; sh.gl[3 * q + 1] = b; sh.gl[3 * q + 2] = c;
    }
  }
  g.f = ff_wave_sum(g.f);
  g.qi = ff_wave_sum(g.qi); g.qj = ff_wave_sum(g.qj); g.qk = ff_wave_sum(g.qk); g.qw = ff_wave_sum(g.qw);
  g.cx = ff_wave_sum(g.cx); g.cy = ff_wave_sum(g.cy); g.size = ff_wave_sum(g.size);
  f += g.f;
  // -(1/150) log p_GMM(s): logsumexp over the K energies, as gmm_nll of loss_math.h
  double mx = -1.0e300;
  for (int k = 0; k < m.K; ++k) mx = sh.a[k] > mx ? sh.a[k] : mx;
  double se = 0.0;
  for (int k = 0; k < m.K; ++k) se += exp(sh.a[k] - mx);
  f += kGmmWeight * (-(mx + log(se)) * kGmmFudge);
  double gsize;
  f += size_term(p.size, gsize);
  __syncthreads();  // gl complete
  if (lane < kShape) {
    double acc = 0.0;
    if (n_free > kPose) {
      const float* row = m.eig + lane * kEl;
      for (int e = 0; e < kEl; ++e) acc += sh.gl[e] * (double)row[e];
      double gg = 0.0;
      for (int k = 0; k < m.K; ++k) {
        const double si = m.sinv[k * kShape + lane];
        gg += exp(sh.a[k] - mx) / se * (xs[kPose + lane] - m.mu[k * kShape + lane]) * si * si;
      }
      acc += kGmmWeight * kGmmFudge * gg;
    }
    gs[kPose + lane] = acc;
  }
  if (lane == 0) {
    double g0, g1, g2, g3;
    quat_norm_bwd(p, n, g, g0, g1, g2, g3);
    gs[0] = g0; gs[1] = g1; gs[2] = g2; gs[3] = g3;
    gs[4] = g.cx; gs[5] = g.cy; gs[6] = g.size + gsize;
  }
  __syncthreads();
  return f;
}

__device__ __forceinline__ bool ff_converged(const double* g, int n, double gtol) {
  bool ok = true;
  for (int c = 0; c < n; ++c) ok = ok && (fabs(g[c]) <= gtol);  // (a NaN component is not converged)
  return ok;
}

struct FfState {
  double H[kN * kN];
  double x[kN], g[kN], d[kN], xn[kN], gn[kN], y[kN], hy[kN];
  FfScratch sh;
};

// One stage on the first n unknowns.  On entry st.x and f = f(st.x) are valid; st.g is valid for n when `fresh`.  Returns the status.
__device__ int ff_stage(const FfModel& m, const FfData& dt, int n, int max_it, double gtol, bool fresh, double& f, int& its, FfState& st,
                        int lane) {
  if (!fresh) f = ff_eval(m, dt, st.x, n, st.g, st.sh, lane);
  for (int idx = lane; idx < n * n; idx += kWave) st.H[(idx / n) * kN + idx % n] = (idx / n == idx % n) ? 1.0 : 0.0;
  __syncthreads();
  int it = 0;
  bool failed = false;
  for (; it < max_it; ++it) {
    if (ff_converged(st.g, n, gtol)) break;
    if (lane < n) {
      double a = 0.0;
      for (int c = 0; c < n; ++c) a += st.H[lane * kN + c] * st.g[c];
      st.d[lane] = -a;
    }
    __syncthreads();
    double gd = 0.0;
    for (int c = 0; c < n; ++c) gd += st.g[c] * st.d[c];
    if (!(gd < 0.0)) {  // not a descent direction (or NaN): steepest descent from a fresh H
      __syncthreads();
      for (int idx = lane; idx < n * n; idx += kWave) st.H[(idx / n) * kN + idx % n] = (idx / n == idx % n) ? 1.0 : 0.0;
      if (lane < n) st.d[lane] = -st.g[lane];
      __syncthreads();
      gd = 0.0;
      for (int c = 0; c < n; ++c) gd += st.g[c] * st.d[c];
    }
    double t = 1.0;
    if (it == 0) {
      double g1 = 0.0;
      for (int c = 0; c < n; ++c) g1 += fabs(st.g[c]);
      const double r = 1.0 / g1;
      t = r < 1.0 ? r : 1.0;
    }
    bool accepted = false;
    double fn = f;
    for (int h = 0; h <= 30; ++h) {
      if (lane < kN) st.xn[lane] = lane < n ? st.x[lane] + t * st.d[lane] : st.x[lane];
      fn = ff_eval(m, dt, st.xn, n, st.gn, st.sh, lane);  // (its first barrier orders the writes of xn)
      if (isfinite(fn) && fn <= f + 1.0e-4 * t * gd) {
        accepted = true;
        break;
      }
      t *= 0.5;
    }
    if (!accepted) {
      failed = true;
      break;
    }
    if (lane < n) {
      st.d[lane] = t * st.d[lane];  // s
      st.y[lane] = st.gn[lane] - st.g[lane];
    }
    __syncthreads();
    double sy = 0.0, ss = 0.0, yy = 0.0;
    for (int c = 0; c < n; ++c) {
      sy += st.d[c] * st.y[c];
      ss += st.d[c] * st.d[c];
      yy += st.y[c] * st.y[c];
    }
    if (sy > 1.0e-10 * sqrt(ss) * sqrt(yy)) {
      const double rho = 1.0 / sy;
      double hyr = 0.0;
      if (lane < n) {
        for (int c = 0; c < n; ++c) hyr += st.H[lane * kN + c] * st.y[c];
        st.hy[lane] = hyr;
      }
      __syncthreads();
      double yhy = 0.0;
      for (int c = 0; c < n; ++c) yhy += st.y[c] * st.hy[c];
      const double a = (1.0 + rho * yhy) * rho;
      if (lane < n) {
        const double sr = st.d[lane];
        for (int c = 0; c < n; ++c) st.H[lane * kN + c] += a * sr * st.d[c] - rho * (hyr * st.d[c] + sr * st.hy[c]);
      }
    }
    __syncthreads();
    if (lane < kN) {
      st.x[lane] = st.xn[lane];
      st.g[lane] = st.gn[lane];
    }
    f = fn;
    __syncthreads();
  }
  its = it;
  if (failed) return 2;
  return ff_converged(st.g, n, gtol) ? 0 : 1;
}

__device__ __forceinline__ FfData ff_load(const float* __restrict__ target, const float* __restrict__ weight, int b, int lane, bool& bad) {
  const float* y = target + (size_t)b * (kPts * 2);
  const float* w = weight + (size_t)b * kPts;
  FfData dt;
  dt.y0x = (double)y[2 * lane]; dt.y0y = (double)y[2 * lane + 1]; dt.w0 = (double)w[lane];
  dt.y1x = dt.y1y = dt.w1 = 0.0;
  if (lane < kPts - kWave) {
    const int q = kWave + lane;
    dt.y1x = (double)y[2 * q]; dt.y1y = (double)y[2 * q + 1]; dt.w1 = (double)w[q];
  }
  bad = !(isfinite(dt.y0x) && isfinite(dt.y0y) && isfinite(dt.w0) && isfinite(dt.y1x) && isfinite(dt.y1y) && isfinite(dt.w1));
  return dt;
}

__global__ void __launch_bounds__(kWave) facefit_objective_k(const float* __restrict__ x, const float* __restrict__ target,
                                                              const float* __restrict__ weight, FfModel m, int B, int n_free,
                                                              double* __restrict__ f, double* __restrict__ g) {
  __shared__ double sx[kN], sg[kN];
  __shared__ FfScratch sh;
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  bool bad;
  const FfData dt = ff_load(target, weight, b, lane, bad);
  if (lane < kN) sx[lane] = (double)x[(size_t)b * kN + lane];
  const double v = ff_eval(m, dt, sx, n_free, sg, sh, lane);
  if (lane == 0) f[b] = v;
  if (lane < kN) g[(size_t)b * kN + lane] = sg[lane];
}

__global__ void __launch_bounds__(kWave) facefit_k(const float* __restrict__ x0, const float* __restrict__ target,
                                                    const float* __restrict__ weight, FfModel m, int B, int iters1, double gtol1, int iters2,
                                                    double gtol2, float* __restrict__ x_out, float* __restrict__ pts_out,
                                                    double* __restrict__ f_out, int* __restrict__ status, int* __restrict__ iters) {
  __shared__ FfState st;
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  bool bad;
  const FfData dt = ff_load(target, weight, b, lane, bad);
  if (lane < kN) {
    const float v = x0[(size_t)b * kN + lane];
    st.x[lane] = (double)v;
    bad = bad || !isfinite(v);
  }
  double f = ff_eval(m, dt, st.x, kPose, st.g, st.sh, lane);
  const double f_start = f;
  int code = 3, it1 = 0, it2 = 0;
  if (!__any(bad) && isfinite(f)) {
    ff_stage(m, dt, kPose, iters1, gtol1, true, f, it1, st, lane);
    code = ff_stage(m, dt, kN, iters2, gtol2, false, f, it2, st, lane);
  }
  // the landmarks of the final x, and the outputs
  ff_local(m, st.x, st.sh, lane);
  Pose p;
  double n;
  quat_norm_fwd(st.x[0], st.x[1], st.x[2], st.x[3], p, n);
  p.cx = st.x[4]; p.cy = st.x[5]; p.size = st.x[6];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int q = lane + kWave * k;
    if (q < kPts) {
      double P0, P1, P2;
      point_fwd(p, st.sh.loc[3 * q], st.sh.loc[3 * q + 1], st.sh.loc[3 * q + 2], P0, P1, P2);
      float* o = pts_out + ((size_t)b * kPts + q) * 3;
      o[0] = (float)P0; o[1] = (float)P1; o[2] = (float)P2;
    }
  }
  if (lane < kN) {
    float v;
    if (code == 3) v = x0[(size_t)b * kN + lane];  // outputs equal the inputs
    else v = (float)(lane == 0 ? p.qi : (lane == 1 ? p.qj : (lane == 2 ? p.qk : (lane == 3 ? p.qw : st.x[lane]))));
    x_out[(size_t)b * kN + lane] = v;
  }
  if (lane == 0) {
    f_out[2 * (size_t)b] = f_start;
    f_out[2 * (size_t)b + 1] = f;
    status[b] = code;
    iters[2 * (size_t)b] = it1;
    iters[2 * (size_t)b + 1] = it2;
  }
}

}  // namespace ttk

using namespace ttk;

#define TTK_FACEFIT_MODEL_CHECK(name)                                                                                              \
  TTK_REQUIRE(K >= 1 && K <= kMaxK, name ": 1 <= K <= %d mixture components, got %d", kMaxK, K);                                    \
  TTK_REQUIRE(target && weight && keypts && keyeigvecs && ck && mu && sinv, name ": a required pointer is null");                  \
  TTK_REQUIRE(B >= 0, name ": B = %d", B)

extern "C" {

int ttk_facefit_objective(const float* x, const float* target, const float* weight, const float* keypts, const float* keyeigvecs,
                          const double* ck, const double* mu, const double* sinv, int K, int B, int n_free, double* f, double* g,
                          ttk_stream_t stream) {
  TTK_FACEFIT_MODEL_CHECK("facefit_objective");
  TTK_REQUIRE(x && f && g, "facefit_objective: a required pointer is null");
  TTK_REQUIRE(n_free == kPose || n_free == kN, "facefit_objective: n_free is 7 (pose) or 57 (pose and shape), got %d", n_free);
  if (B == 0) return 0;
  hipLaunchKernelGGL(facefit_objective_k, dim3(B), dim3(kWave), 0, (hipStream_t)stream, x, target, weight,
                     FfModel{keypts, keyeigvecs, ck, mu, sinv, K}, B, n_free, f, g);
  TTK_LAUNCH_CHECK("facefit_objective");
}

int ttk_facefit(const float* x0, const float* target, const float* weight, const float* keypts, const float* keyeigvecs, const double* ck,
                const double* mu, const double* sinv, int K, int B, int iters1, double gtol1, int iters2, double gtol2, float* x_out,
                float* pts_out, double* f_out, int* status, int* iters, ttk_stream_t stream) {
  TTK_FACEFIT_MODEL_CHECK("facefit");
  TTK_REQUIRE(x0 && x_out && pts_out && f_out && status && iters, "facefit: a required pointer is null");
  TTK_REQUIRE(iters1 >= 0 && iters2 >= 0, "facefit: iteration limits must not be negative, got %d and %d", iters1, iters2);
  TTK_REQUIRE(gtol1 > 0.0 && gtol2 > 0.0, "facefit: gradient tolerances must be positive, got %g and %g", gtol1, gtol2);
  if (B == 0) return 0;
  hipLaunchKernelGGL(facefit_k, dim3(B), dim3(kWave), 0, (hipStream_t)stream, x0, target, weight, FfModel{keypts, keyeigvecs, ck, mu, sinv, K},
                     B, iters1, gtol1, iters2, gtol2, x_out, pts_out, f_out, status, iters);
  TTK_LAUNCH_CHECK("facefit");
}

}  // extern "C"
