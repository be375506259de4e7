// Ensemble reduction for pseudo-labelling (reference: scripts/add_pose_pseudolabels.py:84-156, neuralnets/torchquaternion.py:239-256).
// E networks have predicted the same B crops; this maps every member's prediction from the crop's [-1, 1] coordinates to image pixels
// (labels_under of label_math.h: the formulas and the flip map of the crop's label kernel, tensors/affinetrafo.py:37-148) and averages the
// transformed members per row:
//
//   pose   : quat_average - pivot = first argmax over components of sum_e |q_e|, members with a negative pivot component negated,
//            mean, divided by max(|mean|, FLT_MIN)
//   coord, pt3d_68, shapeparam : arithmetic mean (shapeparam has no geometry: it is averaged as it is)
//   stats  : [0] mean_e of the geodesic angle between member e and the averaged rotation (radians)
//            [1] |mean| before the normalisation (the reference warns where it is <= 0.5)
//            [2..4] population standard deviation over the members of coord x, y, size (pixels)
//
// Mapping: one wave per row.  Member by member, lane 0 transforms pose and coord and the lanes stride over the 68 landmarks into LDS; then
// every lane adds the member's value to the accumulators of ITS output elements (element i = lane + 64 k of the 204 landmark coordinates
// followed by the S shape parameters).  The sum of an element is serial in member order in one lane, so the result is bitwise repeatable: no
// atomics, no cross-lane reduction.  The quaternion / coord / statistics part reads the E transformed members back from LDS and is computed
// redundantly by every lane (wave-uniform); lanes 0..11 store it.  Compiled without the SLP vectoriser like heads.hip (Makefile).
#include <float.h>

#include "head_math.h"
#include "label_math.h"
#include "ttk_common.h"

namespace ttk {

constexpr int kEnsMaxMembers = 16, kEnsMaxShape = 64;
constexpr int kEnsAcc = (204 + kEnsMaxShape + kWave - 1) / kWave;  // output elements per lane

__device__ __forceinline__ float pick4(const float v[4], int p) { return p == 0 ? v[0] : (p == 1 ? v[1] : (p == 2 ? v[2] : v[3])); }

__global__ void __launch_bounds__(kWave) ensemble_reduce_k(const float* __restrict__ pose, const float* __restrict__ coord,
                                                            const float* __restrict__ pts, const float* __restrict__ shape,
                                                            const float* __restrict__ back, int E, int B, int S,
                                                            float* __restrict__ pose_out, float* __restrict__ coord_out,
                                                            float* __restrict__ pts_out, float* __restrict__ shape_out,
                                                            float* __restrict__ stats) {
  __shared__ float s_pts[204];               // the current member's landmarks in image pixels
  __shared__ float s_qc[kEnsMaxMembers][8];  // every member's pose [0..3] and coord [4..6] in image pixels
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  const float* t = back + 6 * (size_t)b;
  const Aff m{t[0], t[1], t[2], t[3], t[4], t[5]};
  const int npts = pts ? 204 : 0, nel = npts + (shape ? S : 0);
  const float fE = (float)E;

  float acc[kEnsAcc];
#pragma unroll
  for (int k = 0; k < kEnsAcc; ++k) acc[k] = 0.f;
  for (int e = 0; e < E; ++e) {
    const size_t row = (size_t)e * B + b;
    if (lane < 4) s_qc[e][lane] = pose[row * 4 + lane];
    else if (lane < 7) s_qc[e][lane] = coord[row * 3 + (lane - 4)];
    __syncthreads();
    labels_under(m, &s_qc[e][4], &s_qc[e][0], nullptr, pts ? pts + row * 204 : nullptr, s_pts, nullptr, nullptr, lane);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kEnsAcc; ++k) {
      const int i = lane + kWave * k;
      if (i < nel) acc[k] += i < npts ? s_pts[i] : shape[row * S + (i - npts)];
    }
    __syncthreads();  // s_pts is rewritten by the next member
  }
#pragma unroll
  for (int k = 0; k < kEnsAcc; ++k) {
    const int i = lane + kWave * k;
    if (i < npts) pts_out[(size_t)b * 204 + i] = acc[k] / fE;
    else if (i < nel) shape_out[(size_t)b * S + (i - npts)] = acc[k] / fE;
  }

  // ---- wave-uniform: quat_average, the coord mean and the five statistics
  float sa[4] = {0.f, 0.f, 0.f, 0.f};
  for (int e = 0; e < E; ++e)
    for (int c = 0; c < 4; ++c) sa[c] += fabsf(s_qc[e][c]);
  int p = 0;
  for (int c = 1; c < 4; ++c)
    if (sa[c] > pick4(sa, p)) p = c;  // strictly greater: the first index wins a tie (np.argmax)
  float sm[4] = {0.f, 0.f, 0.f, 0.f}, sc[3] = {0.f, 0.f, 0.f};
  for (int e = 0; e < E; ++e) {
    const float sg = s_qc[e][p] < 0.f ? -1.f : 1.f;
    for (int c = 0; c < 4; ++c) sm[c] += sg * s_qc[e][c];
    for (int c = 0; c < 3; ++c) sc[c] += s_qc[e][4 + c];
  }
  float q[4], cm[3];
  for (int c = 0; c < 4; ++c) sm[c] = sm[c] / fE;
  const float norm = sqrtf(sm[0] * sm[0] + sm[1] * sm[1] + sm[2] * sm[2] + sm[3] * sm[3]);
  const float den = fmaxf(norm, FLT_MIN);
  for (int c = 0; c < 4; ++c) q[c] = sm[c] / den;
  for (int c = 0; c < 3; ++c) cm[c] = sc[c] / fE;
  // geodesic angle of conj(q) * q_e: 2 atan2(|ijk|, |w|) (torchquaternion.geodesicdistance: positivereal, then to_rotvec)
  float ang = 0.f, var[3] = {0.f, 0.f, 0.f};
  const hm::Q qc = hm::qconj(hm::Q{q[0], q[1], q[2], q[3]});
  for (int e = 0; e < E; ++e) {
    const hm::Q d = hm::qmul(qc, hm::Q{s_qc[e][0], s_qc[e][1], s_qc[e][2], s_qc[e][3]});
    ang += 2.f * atan2f(sqrtf(d.i * d.i + d.j * d.j + d.k * d.k), fabsf(d.w));
    for (int c = 0; c < 3; ++c) {
      const float r = s_qc[e][4 + c] - cm[c];
      var[c] += r * r;
    }
  }
  if (lane < 4) pose_out[(size_t)b * 4 + lane] = pick4(q, lane);
  else if (lane < 7) coord_out[(size_t)b * 3 + (lane - 4)] = lane == 4 ? cm[0] : (lane == 5 ? cm[1] : cm[2]);
  else if (lane < 12) {
    const int s = lane - 7;
    const float v = s == 0 ? ang / fE : (s == 1 ? norm : sqrtf((s == 2 ? var[0] : (s == 3 ? var[1] : var[2])) / fE));
    stats[(size_t)b * 5 + s] = v;
  }
}

}  // namespace ttk

using namespace ttk;

extern "C" {

int ttk_ensemble_reduce(const float* pose, const float* coord, const float* pts, const float* shape, const float* back, int E, int B, int S,
                        float* pose_out, float* coord_out, float* pts_out, float* shape_out, float* stats, ttk_stream_t stream) {
  TTK_REQUIRE(E >= 1 && E <= kEnsMaxMembers, "ensemble_reduce: 1 <= E <= %d members, got %d", kEnsMaxMembers, E);
  TTK_REQUIRE(pose && coord && back && pose_out && coord_out && stats && B > 0, "ensemble_reduce: bad arguments");
  TTK_REQUIRE((pts == nullptr) == (pts_out == nullptr), "ensemble_reduce: pts and pts_out are given together or not at all");
  TTK_REQUIRE((shape == nullptr) == (shape_out == nullptr), "ensemble_reduce: shape and shape_out are given together or not at all");
  TTK_REQUIRE(!shape || (S >= 1 && S <= kEnsMaxShape), "ensemble_reduce: 1 <= S <= %d shape parameters, got %d", kEnsMaxShape, S);
  hipLaunchKernelGGL(ensemble_reduce_k, dim3(B), dim3(kWave), 0, (hipStream_t)stream, pose, coord, pts, shape, back, E, B, S, pose_out,
                     coord_out, pts_out, shape_out, stats);
  TTK_LAUNCH_CHECK("ensemble_reduce");
}

}  // extern "C"
