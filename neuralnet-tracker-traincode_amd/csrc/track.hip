// Closed-loop tracking on the device (reference: scripts/evaluate_stability.py:248-264 closed_loop_tracking).  The reference crops every frame
// around the box the network predicted on the previous one and reads that box back to the host once per frame; here the loop-carried state
// stays on the device: roi_state[L][4] (the current box of each of L lanes - independent trackers that share one network and advance in
// lockstep) and the frame counter *t_dev.  A frame is three enqueues - track_crop, the network's eval forward, track_update - none of which
// returns to the host, so a whole video is enqueued (or one captured graph is replayed T times) before the single synchronisation.
//
//   track_crop   : ONE launch for ttk_view_roi + ttk_roi_transform + ttk_affine_warp of every lane on frame (lane_seq[l], *t_dev).  Thread 0
//                  of every workgroup runs the two per-sample functions of crop_math.h into LDS (workgroup 0 of a lane also stores them),
//                  then every thread samples one output pixel with warp_pixel from the transform in LDS: the operands pass through memory
//                  between the three steps exactly as between the three launches, and the results are bitwise theirs.
//   track_update : ONE workgroup, one wave per lane.  back = (norm(N) o tr[l])^-1 in closed form, the lane's predictions through
//                  labels_under (label_math.h: the function of the label kernel and of the ensemble reduction) into row *t_dev of the
//                  trajectory buffers, the reference's clamp, the validity rule, and - after a workgroup barrier - *t_dev + 1.
//                  Every value is computed serially in one lane: no atomics, bitwise repeatable.
//   track_reacquire : with a face localizer (localizer.hip) in the loop, after the update: counts every lane's run of lost frames and,
//                  once it reaches reacquire_after, restarts the lane from the localizer's box if that is a valid box with a face
//                  probability above the threshold; records the localizer's per-sequence outputs of the frame.
// Compiled without the SLP vectoriser like heads.hip / ensemble.hip (Makefile): per-sample head math of the same kind.
#include <math.h>

#include "crop_math.h"
#include "head_math.h"
#include "label_math.h"
#include "localizer_math.h"
#include "ttk_common.h"

namespace ttk {

constexpr int kTrackMaxLanes = 16;

// grid (ceil(N * N / kBlock), L).  `angles` is always null (the tracker never rotates): a run-time null, so that roi_transform_row is
// compiled as in roi_transform_k.
template <typename T>
__global__ void __launch_bounds__(kBlock) track_crop_k(const T* __restrict__ frames, int S, int Tn, int Hs, int Ws,
                                                        const int* __restrict__ lane_seq, const float* __restrict__ lane_factor,
                                                        const float* __restrict__ roi_state, const int* __restrict__ t_dev,
                                                        const float* __restrict__ angles, int N, float mul, float add,
                                                        int* __restrict__ view_roi, float* __restrict__ tr, float* __restrict__ out) {
  __shared__ int s_vr[4];
  __shared__ float s_m[6];
  const int l = blockIdx.y;
  const int t = *t_dev, seq = lane_seq[l];
  if (t < 0 || t >= Tn || seq < 0 || seq >= S) return;  // uniform over the workgroup: nothing is written
  if (threadIdx.x == 0) {
    // translation (0, 0): the shift term is 0 whatever beyond_border_shift is
    view_roi_row(roi_state + 4 * l, lane_factor[l], 0.f, 0.f, 0.f, s_vr);
    roi_transform_row(s_vr, angles, l, N, s_m);
    if (blockIdx.x == 0) {
      for (int k = 0; k < 4; ++k) view_roi[4 * l + k] = s_vr[k];
      for (int k = 0; k < 6; ++k) tr[6 * l + k] = s_m[k];
    }
  }
  __syncthreads();
  const int idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx >= N * N) return;
  const T* img = frames + ((size_t)seq * Tn + t) * ((size_t)Hs * Ws);
  out[(size_t)l * N * N + idx] = warp_pixel(img, Hs, Ws, s_m, idx / N, idx % N, mul, add);
}

__device__ __forceinline__ float pick4f(float v0, float v1, float v2, float v3, int p) { return p == 0 ? v0 : (p == 1 ? v1 : (p == 2 ? v2 : v3)); }

// one workgroup of L waves; wave l = lane l of the tracker
__global__ void __launch_bounds__(kWave* kTrackMaxLanes) track_update_k(const float* __restrict__ roi, const float* __restrict__ coord,
                                                                        const float* __restrict__ pose, const float* __restrict__ pts,
                                                                        const float* __restrict__ tr, int* t_dev, int L, int N, int Tn, int Hs,
                                                                        int Ws, const float* __restrict__ lane_factor, float* roi_state,
                                                                        float* __restrict__ traj_roi_in, float* __restrict__ traj_roi,
                                                                        float* __restrict__ traj_coord, float* __restrict__ traj_pose,
                                                                        float* __restrict__ traj_pts, unsigned char* __restrict__ lost) {
  __shared__ float s_lab[kTrackMaxLanes][12];  // roi [0..3], coord [4..6], pose [7..10] of every lane
  const int l = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
  const int t = *t_dev;  // read by every thread before the first barrier; written by one thread after the last
  if (t < 0 || t >= Tn) return;
  if (lane < 4) s_lab[l][lane] = roi[4 * l + lane];
  else if (lane < 7) s_lab[l][lane] = coord[3 * l + (lane - 4)];
  else if (lane < 11) s_lab[l][lane] = pose[4 * l + (lane - 7)];
  __syncthreads();
  // back = (norm(N) o tr)^-1, norm(N): x -> x 2/N - 1.  A = norm o tr = (s a, s b, s tx - 1; s c, s d, s ty - 1); A^-1 = (R^-1, -R^-1 T)
  const float* m = tr + 6 * l;
  const float s = 2.f / (float)N;
  const float a = s * m[0], b = s * m[1], tx = s * m[2] - 1.f, c = s * m[3], d = s * m[4], ty = s * m[5] - 1.f;
  const float det = a * d - b * c;
  const float ia = d / det, ib = -b / det, ic = -c / det, id = a / det;
  const Aff back{ia, ib, -(ia * tx + ib * ty), ic, id, -(ic * tx + id * ty)};
  const size_t row = (size_t)t * L + l;
  labels_under(back, &s_lab[l][4], &s_lab[l][7], &s_lab[l][0], pts ? pts + (size_t)l * 204 : nullptr,
               traj_pts ? traj_pts + row * 204 : nullptr, nullptr, nullptr, lane);
  __syncthreads();
  if (lane < 4) {
    // the reference's clamp (:257-259) and the validity rule, evaluated alike by the four lanes that store the box
    const float x0 = s_lab[l][0], y0 = s_lab[l][1], x1 = s_lab[l][2], y1 = s_lab[l][3];
    float c[4];
    const bool inside = track_candidate(x0, y0, x1, y1, Ws, Hs, lane_factor[l], c);  // localizer_math.h: shared with track_reacquire_k
    const float c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
    // (the back-transformed box is the bounding box of four corners, which re-sorts an inverted prediction: its order is tested on the
    // network's own box)
    const bool ordered = roi[4 * l + 2] > roi[4 * l] && roi[4 * l + 3] > roi[4 * l + 1];
    const bool valid = inside && ordered;
    traj_roi_in[row * 4 + lane] = roi_state[4 * l + lane];
    traj_roi[row * 4 + lane] = s_lab[l][lane];
    if (valid) roi_state[4 * l + lane] = pick4f(c0, c1, c2, c3, lane);
    if (lane == 0) lost[row] = valid ? 0 : 1;
  } else if (lane < 7) {
    traj_coord[row * 3 + (lane - 4)] = s_lab[l][lane];
  } else if (lane < 11) {
    traj_pose[row * 4 + (lane - 7)] = s_lab[l][lane];
  }
  __syncthreads();
  if (threadIdx.x == 0) *t_dev = t + 1;
}

// one workgroup; runs after track_update_k of frame t, so it reads t = *t_dev - 1.  Threads l < L handle the lanes, all threads the rows
// of the per-sequence outputs.  Every value is computed by one thread: no atomics, bitwise repeatable.
__global__ void __launch_bounds__(kBlock) track_reacquire_k(const float* __restrict__ loc_out, const float* __restrict__ lb,
                                                             const int* __restrict__ t_dev, int L, int S, int Tn, int Hs, int Ws,
                                                             const int* __restrict__ lane_seq, const float* __restrict__ lane_factor,
                                                             const unsigned char* __restrict__ lost, int reacquire_after, float face_threshold,
                                                             float* __restrict__ roi_state, int* __restrict__ lost_run,
                                                             unsigned char* __restrict__ reacquired, float* __restrict__ hasface,
                                                             float* __restrict__ loc_roi) {
  const int t = *t_dev - 1;
  if (t < 0 || t >= Tn) return;
  for (int q = threadIdx.x; q < S; q += kBlock) {
    float r[4];
    localizer_box_to_frame(loc_out + 5 * q + 1, lb + 3 * q, r);
    hasface[(size_t)t * S + q] = face_probability(loc_out[5 * q]);
    for (int k = 0; k < 4; ++k) loc_roi[((size_t)t * S + q) * 4 + k] = r[k];
  }
  const int l = threadIdx.x;
  if (l >= L) return;
  const int q = lane_seq[l];
  const int run = lost[(size_t)t * L + l] ? lost_run[l] + 1 : 0;
  bool take = false;
  float c[4];
  if (q >= 0 && q < S && run >= reacquire_after) {
    float r[4];
    localizer_box_to_frame(loc_out + 5 * q + 1, lb + 3 * q, r);
    const bool valid = track_candidate(r[0], r[1], r[2], r[3], Ws, Hs, lane_factor[l], c);
    take = valid && face_probability(loc_out[5 * q]) > face_threshold;  // a NaN logit fails the comparison
  }
  if (take)
    for (int k = 0; k < 4; ++k) roi_state[4 * l + k] = c[k];
  lost_run[l] = take ? 0 : run;
  reacquired[(size_t)t * L + l] = take ? 1 : 0;
}

}  // namespace ttk

using namespace ttk;

extern "C" {

int ttk_track_crop(const void* frames, int src_is_u8, int S, int T, int Hs, int Ws, const int* lane_seq, const float* lane_factor,
                   const float* roi_state, const int* t_dev, int L, int N, float mul, float add, int* view_roi, float* tr, float* out,
                   ttk_stream_t stream) {
  TTK_REQUIRE(L >= 1 && L <= kTrackMaxLanes, "track_crop: 1 <= L <= %d lanes, got %d", kTrackMaxLanes, L);
  TTK_REQUIRE(frames && lane_seq && lane_factor && roi_state && t_dev && view_roi && tr && out, "track_crop: a required pointer is null");
  TTK_REQUIRE(S > 0 && T > 0 && Hs > 0 && Ws > 0 && N > 0 && N <= 4096, "track_crop: bad sizes (S %d, T %d, frames %d x %d, N %d)", S, T, Hs, Ws, N);
  const dim3 grid((unsigned)ceil_div((int64_t)N * N, kBlock), (unsigned)L);
  const float* angles = nullptr;
  if (src_is_u8)
    hipLaunchKernelGGL(track_crop_k<unsigned char>, grid, dim3(kBlock), 0, (hipStream_t)stream, (const unsigned char*)frames, S, T, Hs, Ws,
                       lane_seq, lane_factor, roi_state, t_dev, angles, N, mul, add, view_roi, tr, out);
  else
    hipLaunchKernelGGL(track_crop_k<float>, grid, dim3(kBlock), 0, (hipStream_t)stream, (const float*)frames, S, T, Hs, Ws, lane_seq,
                       lane_factor, roi_state, t_dev, angles, N, mul, add, view_roi, tr, out);
  TTK_LAUNCH_CHECK("track_crop");
}

int ttk_track_update(const float* roi, const float* coord, const float* pose, const float* pts, const float* tr, int* t_dev, int L, int N,
                     int T, int Hs, int Ws, const float* lane_factor, float* roi_state, float* traj_roi_in, float* traj_roi,
                     float* traj_coord, float* traj_pose, float* traj_pts, unsigned char* lost, ttk_stream_t stream) {
  TTK_REQUIRE(L >= 1 && L <= kTrackMaxLanes, "track_update: 1 <= L <= %d lanes, got %d", kTrackMaxLanes, L);
  TTK_REQUIRE(roi && coord && pose && tr && t_dev && lane_factor && roi_state && traj_roi_in && traj_roi && traj_coord && traj_pose && lost,
              "track_update: a required pointer is null");
  TTK_REQUIRE((pts == nullptr) == (traj_pts == nullptr), "track_update: pts and traj_pts are given together or not at all");
  TTK_REQUIRE(N > 0 && T > 0 && Hs > 0 && Ws > 0, "track_update: bad sizes (N %d, T %d, frames %d x %d)", N, T, Hs, Ws);
  hipLaunchKernelGGL(track_update_k, dim3(1), dim3(kWave * L), 0, (hipStream_t)stream, roi, coord, pose, pts, tr, t_dev, L, N, T, Hs, Ws,
                     lane_factor, roi_state, traj_roi_in, traj_roi, traj_coord, traj_pose, traj_pts, lost);
  TTK_LAUNCH_CHECK("track_update");
}

int ttk_track_reacquire(const float* loc_out, const float* lb, const int* t_dev, int L, int S, int T, int Hs, int Ws, const int* lane_seq,
                        const float* lane_factor, const unsigned char* lost, int reacquire_after, float face_threshold, float* roi_state,
                        int* lost_run, unsigned char* reacquired, float* hasface, float* loc_roi, ttk_stream_t stream) {
  TTK_REQUIRE(L >= 1 && L <= kTrackMaxLanes, "track_reacquire: 1 <= L <= %d lanes, got %d", kTrackMaxLanes, L);
  TTK_REQUIRE(loc_out && lb && t_dev && lane_seq && lane_factor && lost && roi_state && lost_run && reacquired && hasface && loc_roi,
              "track_reacquire: a required pointer is null");
  TTK_REQUIRE(S > 0 && T > 0 && Hs > 0 && Ws > 0 && reacquire_after >= 1, "track_reacquire: bad sizes (S %d, T %d, frames %d x %d, reacquire_after %d)",
              S, T, Hs, Ws, reacquire_after);
  hipLaunchKernelGGL(track_reacquire_k, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, loc_out, lb, t_dev, L, S, T, Hs, Ws, lane_seq, lane_factor,
                     lost, reacquire_after, face_threshold, roi_state, lost_run, reacquired, hasface, loc_roi);
  TTK_LAUNCH_CHECK("track_reacquire");
}

}  // extern "C"
