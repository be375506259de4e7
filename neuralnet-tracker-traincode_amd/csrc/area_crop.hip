// Area-filtered (anti-aliased) crop: the reference's resampler for every crop that shrinks its view ROI
// (datatransformation/tensors/image_geometric_cv2.py:65-155: cut the integer ROI out of a zero-padded canvas and
// cv2.resize(INTER_AREA); a rotated crop is warped bilinearly to a source-resolution intermediate first).  One definition
// for both branches, per sample, with tr = rows (a, b, tx), (c, d, ty) as ttk_affine_warp takes it:
//
//   Rx = max(N, rint(N / sqrt(a^2 + b^2))),  Ry = max(N, rint(N / sqrt(c^2 + d^2)))         intermediate size
//   I[p][q] = bilinear(src, tr^-1((q + .5) N / Rx, (p + .5) N / Ry) - .5),  zeros outside     (affine_warp_k's arithmetic)
//   out[i][j] = mul * sum_p sum_q wy[i][p] wx[j][q] I[p][q] + add
//   wx[j][q] = |[q, q + 1) n [j Rx / N, (j + 1) Rx / N)| * N / Rx                              (rows sum to 1)
//
// The overlaps are INTEGERS in units of 1 / N: |[q N, (q + 1) N) n [j Rx, (j + 1) Rx)|, so the weights are exact and the
// only roundings are those of the bilinear taps and of the fp32 sum.  Rx = Ry = N (a crop that magnifies): every weight
// is 1 for q = j and the result is ttk_affine_warp's.
//
// One workgroup per tile of at most 32 x 8 output pixels of one sample.  The tile's patch of I is formed ONCE in LDS
// (consecutive lanes = consecutive q = consecutive source bytes of an unrotated crop), then every thread sums its own
// output pixel's (Rx / N + 1) x (Ry / N + 1) window out of LDS and the rows leave coalesced.  At the ratios of the
// workload (1.6 - 5) the plain 2-D window costs the same LDS reads as a columns-then-rows pass with its second buffer.
// The ratio differs per sample and has no upper bound: a tile whose patch does not fit the 32 KiB takes the direct loop
// (every thread samples its own window from global memory) - a branch that is uniform over the workgroup.
// No atomics; the summation order is fixed: bitwise reproducible.
#include "ttk_common.h"

namespace ttk {
namespace {

constexpr int kAreaTileW = 32, kAreaTileH = 8;  // at most kBlock output pixels per workgroup: one pass
constexpr int kAreaPatch = 8192;                // floats of LDS (32 KiB; 5 workgroups per CU): ratios up to ~6 at N = 129
constexpr int kAreaMaxR = 1 << 20;              // a degenerate tr (zero row) must still terminate

struct AreaGeom {
  float m0, m1, m2, m3, m4, m5, inv, sx, sy;
  int Rx, Ry;
};

__device__ __forceinline__ int area_extent(float r0, float r1, int N) {
  const float f = rintf((float)N / sqrtf(r0 * r0 + r1 * r1));  // half to even, like the float64 restatement (np.rint)
  return f > (float)N ? (f < (float)kAreaMaxR ? (int)f : kAreaMaxR) : N;  // NaN -> N
}

__device__ __forceinline__ AreaGeom area_geom(const float* __restrict__ m, int N) {
#pragma clang fp contract(off)  // det: two rounded products and a subtraction, as affine_warp_k's compiled code has it (area_sample)
  AreaGeom g;
  g.m0 = m[0]; g.m1 = m[1]; g.m2 = m[2]; g.m3 = m[3]; g.m4 = m[4]; g.m5 = m[5];
  g.inv = 1.f / (g.m0 * g.m4 - g.m1 * g.m3);
  g.Rx = area_extent(g.m0, g.m1, N);
  g.Ry = area_extent(g.m3, g.m4, N);
  g.sx = (float)N / (float)g.Rx;  // exactly 1 when Rx = N
  g.sy = (float)N / (float)g.Ry;
  return g;
}

template <typename T>
__device__ __forceinline__ float area_fetch(const T* img, int H, int W, int y, int x) {
  return (x >= 0 && x < W && y >= 0 && y < H) ? (float)img[(size_t)y * W + x] : 0.f;
}

// I[p][q]: affine_warp_k's taps at the crop point ((q + .5) sx, (p + .5) sy).  Contraction is off and every fused multiply-add is
// written out: they are the ones affine_warp_k's compiled code performs (which of its products are fused is the compiler's choice
// there), so with sx = sy = 1 the sample is that kernel's value and a crop that magnifies is ttk_affine_warp's
// (tests/test_area_crop_gpu.py holds the two together).
template <typename T>
__device__ __forceinline__ float area_sample(const T* __restrict__ img, int Hs, int Ws, const AreaGeom& g, float q, float p) {
#pragma clang fp contract(off)
  const float px = fmaf(q + 0.5f, g.sx, -g.m2), py = fmaf(p + 0.5f, g.sy, -g.m5);
  const float u = fmaf(g.m4 * px - g.m1 * py, g.inv, -0.5f);
  const float v = fmaf(fmaf(g.m0, py, -(g.m3 * px)), g.inv, -0.5f);
  // far outside the source (also: beyond the int range) every tap is zero
  if (!(u > -2.f && u < (float)Ws + 1.f && v > -2.f && v < (float)Hs + 1.f)) return 0.f;
  const float fu = floorf(u), fv = floorf(v);
  const int x0 = (int)fu, y0 = (int)fv;
  const float ax = u - fu, ay = v - fv, bx = 1.f - ax, by = 1.f - ay;
  const float v00 = area_fetch(img, Hs, Ws, y0, x0), v01 = area_fetch(img, Hs, Ws, y0, x0 + 1);
  const float v10 = area_fetch(img, Hs, Ws, y0 + 1, x0), v11 = area_fetch(img, Hs, Ws, y0 + 1, x0 + 1);
  const float top = fmaf(bx, v00, ax * v01), bot = fmaf(bx, v10, ax * v11);
  return by * top + ay * bot;
}

// sum over the window of output pixel (i, j), rows outside, columns inside; I = int when R (N + 1) fits, else int64_t
template <typename I, typename At>
__device__ __forceinline__ float area_window(int i, int j, int N, int Rx, int Ry, At at) {
  const I n = (I)N, xa = (I)j * Rx, xb = xa + Rx, ya = (I)i * Ry, yb = ya + Ry;
  const I qa = xa / n, qb = (xb + n - 1) / n, pa = ya / n, pb = (yb + n - 1) / n;
  float acc = 0.f;
  for (I p = pa; p < pb; ++p) {
    const I lo = p * n, hi = lo + n;
    const float wy = (float)((yb < hi ? yb : hi) - (ya > lo ? ya : lo));
    float row = 0.f;
    for (I q = qa; q < qb; ++q) {
      const I l = q * n, h = l + n;
      row = fmaf((float)((xb < h ? xb : h) - (xa > l ? xa : l)), at(q, p), row);
    }
    acc = fmaf(wy, row, acc);
  }
  return acc * (1.f / ((float)Rx * (float)Ry));
}

template <typename T>
__global__ void __launch_bounds__(kBlock) area_crop_k(const T* __restrict__ src, int Hs, int Ws, const float* __restrict__ tr,
                                                       float* __restrict__ out, int N, int tw, int th, int ntx, int nty, float mul,
                                                       float add) {
  __shared__ float patch[kAreaPatch];
  const int tiles = ntx * nty, b = blockIdx.x / tiles, t = blockIdx.x % tiles;
  const int j0 = (t % ntx) * tw, i0 = (t / ntx) * th;
  const int j1 = min(N, j0 + tw), i1 = min(N, i0 + th);
  const AreaGeom g = area_geom(tr + 6 * (size_t)b, N);
  const T* img = src + (size_t)b * Hs * Ws;
  // the tile's patch of I: q in [q0, q0 + pw), p in [p0, p0 + ph)
  const int64_t q0 = (int64_t)j0 * g.Rx / N, pw = ceil_div((int64_t)j1 * g.Rx, N) - q0;
  const int64_t p0 = (int64_t)i0 * g.Ry / N, ph = ceil_div((int64_t)i1 * g.Ry, N) - p0;
  const int64_t lim = (int64_t)1 << 31;
  const bool staged = pw * ph <= kAreaPatch && (int64_t)g.Rx * (N + 1) < lim && (int64_t)g.Ry * (N + 1) < lim;  // workgroup-uniform
  if (staged) {
    const int w = (int)pw, n = w * (int)ph, qs = (int)q0, ps = (int)p0;
    // k = p * w + q walks in steps of kBlock: one division per thread, then carries
    const int dq = kBlock % w, dp = kBlock / w;
    int q = threadIdx.x % w, p = threadIdx.x / w;
    for (int k = threadIdx.x; k < n; k += kBlock) {
      patch[k] = area_sample(img, Hs, Ws, g, (float)(qs + q), (float)(ps + p));
      q += dq; p += dp;
      if (q >= w) { q -= w; ++p; }
    }
    __syncthreads();
  }
  const int ow = j1 - j0, k = threadIdx.x;
  if (k >= ow * (i1 - i0)) return;
  const int j = j0 + k % ow, i = i0 + k / ow;
  float val;
  if (staged) {
    const int w = (int)pw, qs = (int)q0, ps = (int)p0;
    val = area_window<int>(i, j, N, g.Rx, g.Ry, [&](int q, int p) { return patch[(p - ps) * w + (q - qs)]; });
  } else {
    val = area_window<int64_t>(i, j, N, g.Rx, g.Ry, [&](int64_t q, int64_t p) { return area_sample(img, Hs, Ws, g, (float)q, (float)p); });
  }
  out[((size_t)b * N + i) * N + j] = fmaf(val, mul, add);
}

}  // namespace
}  // namespace ttk

using namespace ttk;

extern "C" int ttk_area_crop(const void* src, int src_is_u8, int B, int Hs, int Ws, const float* tr, float* out, int N, float mul,
                             float add, ttk_stream_t stream) {
  TTK_REQUIRE(src && tr && out && B > 0 && Hs > 0 && Ws > 0 && N > 0, "area_crop: bad arguments");
  // equal tiles of at most 32 x 8 that cover N (N = 129: 5 x 17 tiles of 26 x 8)
  const int ntx = (int)ceil_div(N, kAreaTileW), nty = (int)ceil_div(N, kAreaTileH);
  const int tw = (int)ceil_div(N, ntx), th = (int)ceil_div(N, nty);
  const int64_t grid = (int64_t)B * ntx * nty;
  TTK_REQUIRE(grid < ((int64_t)1 << 31), "area_crop: B * tiles = %lld workgroups exceed the grid", (long long)grid);
  if (src_is_u8)
    hipLaunchKernelGGL(area_crop_k<unsigned char>, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream,
                       (const unsigned char*)src, Hs, Ws, tr, out, N, tw, th, ntx, nty, mul, add);
  else
    hipLaunchKernelGGL(area_crop_k<float>, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, (const float*)src, Hs, Ws, tr,
                       out, N, tw, th, ntx, nty, mul, add);
  TTK_LAUNCH_CHECK("area_crop");
}
