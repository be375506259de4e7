// On-GPU affine-warp augmentation.  In the reference this runs per sample on
// the CPU inside DataLoader workers with OpenCV (datatransformation/batch/geometric.py:193-231); its pure
// torch formulation (tensors/image_geometric_torch.py:60-98: affine_grid + grid_sample, bilinear, zero
// padding, align_corners=False) is the semantic oracle for the image, and tensors/affinetrafo.py:37-148 for
// the labels.
//
//   view_roi   : GeneralFocusRoi._compute_view_roi (:108-157) + torch.round(...).to(int32) (:205)
//                INTEGER result, bit-exact: every float op is an explicitly rounded __f*_rn (no fma
//                contraction) in the reference's order; rintf = round-half-to-even like torch.round.
//   roi -> tr  : center_rotation(angle) @ range_remap(view_roi -> [0,N]^2)            (:159-177)
//   warp       : out[b,0,i,j] = bilinear(src_b, tr^-1 (j+.5, i+.5) - .5) * mul + add   (gather-bound)
//   labels     : coord / pose / roi / pt3d_68 / pt2d_68 under tr, then under the [0,N] -> [-1,1] normalisation
// The per-sample arithmetic of the first three is in crop_math.h, shared with the fused crop of the closed-loop tracker (track.hip).
#include "crop_math.h"
#include "head_math.h"
#include "label_math.h"
#include "ttk_common.h"

namespace ttk {

__global__ void view_roi_k(const float* __restrict__ roi, const float* __restrict__ f, const float* __restrict__ t, float bbs,
                           int B, int* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  view_roi_row(roi + 4 * b, f[b], t[2 * b], t[2 * b + 1], bbs, out + 4 * b);
}

// tr = unnorm(N) @ rot(angle) @ norm(N) @ remap(view_roi -> [0,N]^2), row-major 2x3
__global__ void roi_transform_k(const int* __restrict__ vr, const float* __restrict__ angles, int B, int N,
                                float* __restrict__ tr) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  roi_transform_row(vr + 4 * b, angles, b, N, tr + 6 * b);
}

// one thread per output pixel; consecutive lanes = consecutive output columns (coalesced store, gather load)
template <typename T>
__global__ void __launch_bounds__(kBlock) affine_warp_k(const T* __restrict__ src, int B, int Hs, int Ws,
                                                         const float* __restrict__ tr, float* __restrict__ out, int N, float mul,
                                                         float add) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= (int64_t)B * N * N) return;
  const int j = (int)(idx % N), i = (int)((idx / N) % N), b = (int)(idx / ((int64_t)N * N));
  out[idx] = warp_pixel(src + (size_t)b * Hs * Ws, Hs, Ws, tr + 6 * b, i, j, mul, add);
}

// one wave per sample: labels under tr[b], then (N > 0) under the pixel -> [-1,1] normalisation
__global__ void __launch_bounds__(kWave) affine_labels_k(const float* __restrict__ tr, int B, int N, float* coord, float* pose,
                                                          float* roi, const float* pts_in, float* pts_out,
                                                          const float* p2_in, float* p2_out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  const float* t = tr + 6 * b;
  float* c = coord ? coord + 3 * b : nullptr;
  float* q = pose ? pose + 4 * b : nullptr;
  float* r = roi ? roi + 4 * b : nullptr;
  const float* pi = pts_in ? pts_in + (size_t)b * 204 : nullptr;
  float* po = pts_out ? pts_out + (size_t)b * 204 : nullptr;
  const float* p2i = p2_in ? p2_in + (size_t)b * 136 : nullptr;
  float* p2o = p2_out ? p2_out + (size_t)b * 136 : nullptr;
  labels_under(Aff{t[0], t[1], t[2], t[3], t[4], t[5]}, c, q, r, pi, po, p2i, p2o, lane);
  if (N > 0) {
    __syncthreads();
    const float s = 2.f / (float)N;
    labels_under(Aff{s, 0.f, -1.f, 0.f, s, -1.f}, c, q, r, po, po, p2o, p2o, lane);
  }
}

}  // namespace ttk

using namespace ttk;

extern "C" {

int ttk_view_roi(const float* face_roi, const float* scales, const float* translations, float beyond_border_shift, int B,
                 int* view_roi, ttk_stream_t stream) {
  TTK_REQUIRE(face_roi && scales && translations && view_roi && B > 0, "view_roi: bad arguments");
  hipLaunchKernelGGL(view_roi_k, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, face_roi, scales, translations,
                     beyond_border_shift, B, view_roi);
  TTK_LAUNCH_CHECK("view_roi");
}

int ttk_roi_transform(const int* view_roi, const float* angles, int B, int N, float* tr, ttk_stream_t stream) {
  TTK_REQUIRE(view_roi && tr && B > 0 && N > 0, "roi_transform: bad arguments");
  hipLaunchKernelGGL(roi_transform_k, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, view_roi, angles, B, N, tr);
  TTK_LAUNCH_CHECK("roi_transform");
}

int ttk_affine_warp(const void* src, int src_is_u8, int B, int Hs, int Ws, const float* tr, float* out, int N, float mul,
                    float add, ttk_stream_t stream) {
  TTK_REQUIRE(src && tr && out && B > 0 && Hs > 0 && Ws > 0 && N > 0, "affine_warp: bad arguments");
  const unsigned grid = (unsigned)ceil_div((int64_t)B * N * N, kBlock);
  if (src_is_u8)
    hipLaunchKernelGGL(affine_warp_k<unsigned char>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream,
                       (const unsigned char*)src, B, Hs, Ws, tr, out, N, mul, add);
  else
    hipLaunchKernelGGL(affine_warp_k<float>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, (const float*)src, B, Hs, Ws, tr,
                       out, N, mul, add);
  TTK_LAUNCH_CHECK("affine_warp");
}

int ttk_affine_labels(const float* tr, int B, int N, float* coord, float* pose, float* roi, const float* pts_in, float* pts_out,
                      ttk_stream_t stream) {
  TTK_REQUIRE(tr && B > 0, "affine_labels: bad arguments");
  TTK_REQUIRE((pts_in == nullptr) == (pts_out == nullptr) && pts_in != pts_out || !pts_in, "affine_labels: pts_in/pts_out must be two distinct buffers");
  hipLaunchKernelGGL(affine_labels_k, dim3(B), dim3(kWave), 0, (hipStream_t)stream, tr, B, N, coord, pose, roi, pts_in, pts_out,
                     (const float*)nullptr, (float*)nullptr);
  TTK_LAUNCH_CHECK("affine_labels");
}

int ttk_affine_labels2d(const float* tr, int B, int N, float* coord, float* pose, float* roi, const float* pts_in, float* pts_out,
                        const float* pts2d_in, float* pts2d_out, ttk_stream_t stream) {
  TTK_REQUIRE(tr && B > 0, "affine_labels2d: bad arguments");
  TTK_REQUIRE((pts_in == nullptr) == (pts_out == nullptr) && pts_in != pts_out || !pts_in, "affine_labels2d: pts_in/pts_out must be two distinct buffers");
  TTK_REQUIRE((pts2d_in == nullptr) == (pts2d_out == nullptr) && pts2d_in != pts2d_out || !pts2d_in,
              "affine_labels2d: pts2d_in/pts2d_out must be two distinct buffers");
  hipLaunchKernelGGL(affine_labels_k, dim3(B), dim3(kWave), 0, (hipStream_t)stream, tr, B, N, coord, pose, roi, pts_in, pts_out,
                     pts2d_in, pts2d_out);
  TTK_LAUNCH_CHECK("affine_labels2d");
}

}  // extern "C"
