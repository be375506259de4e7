// The any-channel-count kernel family (ttk_anyc_*, csrc/anyc_*.hip): the MobileNet path for channel counts that are multiples of 8 in
// 8..2048 (width-scaled backbones, MobileNet(widen_factor=w)).  Same contracts as the tuned kernels they stand in for (include/ttk.h): BatchNorm
// (+ ReLU, + residual) applied on load, raw outputs + per-workgroup partial sums on store, no float atomics anywhere - every reduction is
// workgroup rows + a fixed-order fold, so two runs give bitwise equal results in every mode.
//
// Layout (include/ttk.h, "Activation layout"): channel blocks of 32 with ONE narrower last block,
//   [M][32], ..., [M][32], [M][C mod 32];  element (m, c) of block b = c >> 5 at  b * M * 32 + m * width(b) + (c & 31).
// For C a multiple of 32 this is the tuned kernels' layout, so the two families are neighbours in one chain.
#pragma once
#include "ttk_common.h"

namespace ttk {
namespace anyc {

constexpr int kMaxC = 2048;
constexpr int kPixLanes = 32;  // pixel lanes of a pixel-wise workgroup: 256 threads = 32 pixels x 8 channel quads of one channel block
constexpr int kMaxRows = 1024;

inline bool c_ok(int C) { return C >= 8 && C <= kMaxC && (C & 7) == 0; }
__host__ __device__ __forceinline__ int blk_w(int C, int cb) { const int r = C - (cb << 5); return r < 32 ? r : 32; }
__host__ __device__ __forceinline__ int n_blk(int C) { return (C + 31) >> 5; }
__host__ __device__ __forceinline__ size_t blk_base(int64_t M, int cb) { return (size_t)cb * (size_t)M * 32; }
__host__ __device__ __forceinline__ size_t off(int64_t m, int c, int64_t M, int C) {
  const int cb = c >> 5;
  return blk_base(M, cb) + (size_t)m * blk_w(C, cb) + (c & 31);
}

// rows of partial sums a pixel-wise kernel of the family writes for M pixels (= its grid.x)
inline int pix_rows(int64_t M) {
  int64_t g = ceil_div(M, 4 * kPixLanes);
  return (int)(g > kMaxRows ? kMaxRows : (g < 1 ? 1 : g));
}

// Thread geometry of the pixel-wise kernels: blockIdx.y = channel block, q = channel quad inside it, pl = pixel lane.
struct PixThread {
  int cb, wb, q, pl, c;  // c = first of the thread's 4 channels
  bool active;           // the quad exists in this (possibly narrower) block
  __device__ __forceinline__ PixThread(int C) {
    cb = blockIdx.y;
    wb = blk_w(C, cb);
    q = threadIdx.x & 7;
    pl = threadIdx.x >> 3;
    c = (cb << 5) + 4 * q;
    active = 4 * q < wb;
  }
};

// One float4 per thread -> the sum over the workgroup's 32 pixel lanes, in lane order (fixed), valid in threads pl == 0.
// sm: [32][8] float4.
__device__ __forceinline__ float4 pix_reduce(float4 v, float4* sm) {
  const int q = threadIdx.x & 7, pl = threadIdx.x >> 3;
  __syncthreads();  // (the previous use of sm is over)
  sm[pl * 8 + q] = v;
  __syncthreads();
  float4 s = f4(0.f);
  if (pl == 0) {
#pragma unroll 8
    for (int i = 0; i < kPixLanes; ++i) s = add4(s, sm[i * 8 + q]);
  }
  return s;
}

// the workgroup's row of BatchNorm partial sums: part[row][0][c], part[row][1][c] for the channels of this block
__device__ __forceinline__ void pix_partials(const PixThread& t, float4 s1, float4 s2, float* part, int C, float4* sm) {
  s1 = pix_reduce(s1, sm);
  s2 = pix_reduce(s2, sm);
  if (t.pl == 0 && t.active) {
    float* row = part + (size_t)blockIdx.x * 2 * C;
    st4(row + t.c, s1);
    st4(row + C + t.c, s2);
  }
}

__device__ __forceinline__ float max_abs4(float m, float4 v) {
  return fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
}
// raises bn[TTK_BN_AUX][TTK_AUX_GMAX] (an integer maximum on the bit pattern of a non-negative float: order independent)
__device__ __forceinline__ void raise_gmax(float* bn, int C, float v) { wave_raise_max(bn + (size_t)TTK_BN_AUX * C + TTK_AUX_GMAX, v); }

}  // namespace anyc
}  // namespace ttk
