// The pixel-wise kernels of the any-channel-count family (anyc_common.h): stem 5x5 s2, depthwise 3x3 (forward, data gradient with the fused
// weight gradient), global average pool (forward, backward), ttk_bn_act's sibling.  A workgroup is 32 pixel lanes x 8 channel quads of ONE
// channel block (blockIdx.y); a thread keeps its quad for the whole launch, strides over pixels and accumulates its sums in registers; the
// workgroup folds them over its pixel lanes in lane order and stores one row - no atomics except the integer maximum of TTK_AUX_GMAX.
#include "anyc_common.h"

namespace ttk {
namespace anyc {

// ---- stem: y[B][Ho][Wo][C] = conv5x5/s2/p2(x[B][H][W]) -------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) stem_fwd_k(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y,
                                                      float* __restrict__ part, const float* __restrict__ pivot, int B, int H, int W, int Ho,
                                                      int Wo, int C) {
  __shared__ float4 sm[kPixLanes * 8];
  __shared__ __attribute__((aligned(16))) float sw[25][32];
  const PixThread t(C);
  for (int i = threadIdx.x; i < 25 * 32; i += kBlock) {
    const int k = i >> 5, cc = i & 31;
    sw[k][cc] = cc < t.wb ? w[(size_t)((t.cb << 5) + cc) * 25 + k] : 0.f;
  }
  __syncthreads();
  const int64_t M = (int64_t)B * Ho * Wo;
  const float4 pv = (pivot && t.active) ? ld4(pivot + t.c) : f4(0.f);
  float* yb = y + blk_base(M, t.cb);
  float4 s1 = f4(0.f), s2 = f4(0.f);
  for (int64_t m = (int64_t)blockIdx.x * kPixLanes + t.pl; m < M; m += (int64_t)gridDim.x * kPixLanes) {
    if (!t.active) continue;
    const int ow = (int)(m % Wo), oh = (int)((m / Wo) % Ho), n = (int)(m / ((int64_t)Wo * Ho));
    const float* xn = x + (size_t)n * H * W;
    float4 acc = f4(0.f);
#pragma unroll
    for (int kh = 0; kh < 5; ++kh) {
      const int ih = 2 * oh + kh - 2;
      if (ih < 0 || ih >= H) continue;
#pragma unroll
      for (int kw = 0; kw < 5; ++kw) {
        const int iw = 2 * ow + kw - 2;
        if (iw < 0 || iw >= W) continue;
        acc = fma4(f4(xn[(size_t)ih * W + iw]), ld4(&sw[kh * 5 + kw][4 * t.q]), acc);
      }
    }
    st4(yb + (size_t)m * t.wb + 4 * t.q, acc);
    const float4 d = sub4(acc, pv);
    s1 = add4(s1, d);
    s2 = fma4(d, d, s2);
  }
  if (part) pix_partials(t, s1, s2, part, C, sm);
}

// dW[C][25] rows: rowsbuf[blockIdx.x][C * 25] = sum over the workgroup's pixels of dy * x(tap)
__global__ void __launch_bounds__(kBlock) stem_wgrad_k(const float* __restrict__ g, const float* __restrict__ y, const float* __restrict__ bnp,
                                                        const float* __restrict__ x, float* __restrict__ rowsbuf, int B, int H, int W, int Ho,
                                                        int Wo, int C) {
  __shared__ float4 sm[kPixLanes * 8];
  const PixThread t(C);
  const int64_t M = (int64_t)B * Ho * Wo;
  const int cl = t.active ? t.c : 0;
  const BnGrad4 bn = BnGrad4::load(bnp, C, cl);
  const size_t base = blk_base(M, t.cb);
  float4 acc[25];
#pragma unroll
  for (int k = 0; k < 25; ++k) acc[k] = f4(0.f);
  for (int64_t m = (int64_t)blockIdx.x * kPixLanes + t.pl; m < M; m += (int64_t)gridDim.x * kPixLanes) {
    if (!t.active) continue;
    const int ow = (int)(m % Wo), oh = (int)((m / Wo) % Ho), n = (int)(m / ((int64_t)Wo * Ho));
    const float* xn = x + (size_t)n * H * W;
    const size_t o = base + (size_t)m * t.wb + 4 * t.q;
    const float4 dy = bn.dy(ld4(g + o), ld4(y + o));
#pragma unroll
    for (int kh = 0; kh < 5; ++kh) {
      const int ih = 2 * oh + kh - 2;
      const bool hok = ih >= 0 && ih < H;
#pragma unroll
      for (int kw = 0; kw < 5; ++kw) {
        const int iw = 2 * ow + kw - 2;
        const float xv = (hok && iw >= 0 && iw < W) ? xn[(size_t)ih * W + iw] : 0.f;
        acc[kh * 5 + kw] = fma4(dy, f4(xv), acc[kh * 5 + kw]);
      }
    }
  }
  float* row = rowsbuf + (size_t)blockIdx.x * C * 25;
#pragma unroll
  for (int k = 0; k < 25; ++k) {
    const float4 s = pix_reduce(acc[k], sm);
    if (t.pl == 0 && t.active) {
      row[(size_t)(t.c + 0) * 25 + k] = s.x;
      row[(size_t)(t.c + 1) * 25 + k] = s.y;
      row[(size_t)(t.c + 2) * 25 + k] = s.z;
      row[(size_t)(t.c + 3) * 25 + k] = s.w;
    }
  }
}

// ---- depthwise 3x3, pad 1, stride 1|2 ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void load_w9(const float* w, int c, float4 (&wk)[9]) {
#pragma unroll
  for (int k = 0; k < 9; ++k) wk[k] = make_float4(w[(size_t)c * 9 + k], w[(size_t)(c + 1) * 9 + k], w[(size_t)(c + 2) * 9 + k], w[(size_t)(c + 3) * 9 + k]);
}

__global__ void __launch_bounds__(kBlock) dw_fwd_k(const float* __restrict__ yprev, const float* __restrict__ bnp, const float* __restrict__ skip,
                                                    float* __restrict__ a_out, const float* __restrict__ w, float* __restrict__ y,
                                                    float* __restrict__ part, const float* __restrict__ pivot, int B, int H, int W, int Ho, int Wo,
                                                    int C, int stride) {
  __shared__ float4 sm[kPixLanes * 8];
  const PixThread t(C);
  const int64_t Mi = (int64_t)B * H * W, Mo = (int64_t)B * Ho * Wo;
  const int cl = t.active ? t.c : 0;
  const BnApply4 bn = BnApply4::load(bnp, C, cl);
  const float4 pv = (pivot && t.active) ? ld4(pivot + t.c) : f4(0.f);
  float4 wk[9];
  load_w9(w, cl, wk);
  const size_t ib = blk_base(Mi, t.cb) + 4 * t.q, ob = blk_base(Mo, t.cb) + 4 * t.q;
  float4 s1 = f4(0.f), s2 = f4(0.f);
  for (int64_t m = (int64_t)blockIdx.x * kPixLanes + t.pl; m < Mo; m += (int64_t)gridDim.x * kPixLanes) {
    if (!t.active) continue;
    const int ow = (int)(m % Wo), oh = (int)((m / Wo) % Ho), n = (int)(m / ((int64_t)Wo * Ho));
    float4 acc = f4(0.f);
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int ih = oh * stride + kh - 1;
      if (ih < 0 || ih >= H) continue;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int iw = ow * stride + kw - 1;
        if (iw < 0 || iw >= W) continue;
        const size_t o = ib + ((size_t)((int64_t)n * H + ih) * W + iw) * t.wb;
        const float4 a = skip ? bn.act(ld4(yprev + o), ld4(skip + o)) : bn.act(ld4(yprev + o));
        if (a_out && kh == 1 && kw == 1) st4(a_out + o, a);  // (stride 1: the centre tap IS this output pixel - every input pixel once)
        acc = fma4(a, wk[kh * 3 + kw], acc);
      }
    }
    st4(y + ob + (size_t)m * t.wb, acc);
    const float4 d = sub4(acc, pv);
    s1 = add4(s1, d);
    s2 = fma4(d, d, s2);
  }
  if (part) pix_partials(t, s1, s2, part, C, sm);
}

// thread = input pixel x quad: G = convT(dy) (+ skip_grad), g_prev = G * [a_in > 0]; every (dy, a_in) pair of the weight gradient passes through here
template <bool WGRAD>
__global__ void __launch_bounds__(kBlock) dw_bwd_k(const float* __restrict__ g_dw, const float* __restrict__ y_dw, const float* __restrict__ bn_dw,
                                                    const float* __restrict__ w, const float* __restrict__ skip_grad,
                                                    const float* __restrict__ yprev, float* __restrict__ bn_prev, const float* __restrict__ skip_prev,
                                                    const float* __restrict__ a_in, float* __restrict__ g_prev, float* __restrict__ part,
                                                    float* __restrict__ rowsbuf, int B, int H, int W, int Ho, int Wo, int C, int stride) {
  __shared__ float4 sm[kPixLanes * 8];
  const PixThread t(C);
  const int64_t Mi = (int64_t)B * H * W, Mo = (int64_t)B * Ho * Wo;
  const int cl = t.active ? t.c : 0;
  const BnApply4 bnp = BnApply4::load(bn_prev, C, cl);
  const BnGrad4 bng = BnGrad4::load(bn_dw, C, cl);
  float4 wk[9];
  load_w9(w, cl, wk);
  const size_t ib = blk_base(Mi, t.cb) + 4 * t.q, ob = blk_base(Mo, t.cb) + 4 * t.q;
  float4 s1 = f4(0.f), s2 = f4(0.f);
  float4 dwa[WGRAD ? 9 : 1];
#pragma unroll
  for (int k = 0; k < (WGRAD ? 9 : 1); ++k) dwa[k] = f4(0.f);
  float gmx = 0.f;
  for (int64_t m = (int64_t)blockIdx.x * kPixLanes + t.pl; m < Mi; m += (int64_t)gridDim.x * kPixLanes) {
    if (!t.active) continue;
    const int iw = (int)(m % W), ih = (int)((m / W) % H), n = (int)(m / ((int64_t)W * H));
    const size_t o = ib + (size_t)m * t.wb;
    const float4 yv = ld4(yprev + o);
    const float4 a = a_in ? ld4(a_in + o) : (skip_prev ? bnp.act(yv, ld4(skip_prev + o)) : bnp.act(yv));
    float4 G = f4(0.f);
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int th = ih + 1 - kh;
      if (th < 0 || (stride == 2 && (th & 1))) continue;
      const int oh = stride == 2 ? th >> 1 : th;
      if (oh >= Ho) continue;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int tw = iw + 1 - kw;
        if (tw < 0 || (stride == 2 && (tw & 1))) continue;
        const int ow = stride == 2 ? tw >> 1 : tw;
        if (ow >= Wo) continue;
        const size_t oo = ob + ((size_t)((int64_t)n * Ho + oh) * Wo + ow) * t.wb;
        const float4 dy = bng.dy(ld4(g_dw + oo), ld4(y_dw + oo));
        G = fma4(dy, wk[kh * 3 + kw], G);
        if (WGRAD) dwa[kh * 3 + kw] = fma4(dy, a, dwa[kh * 3 + kw]);
      }
    }
    if (skip_grad) G = add4(G, ld4(skip_grad + o));
    const float4 gp = mask4(G, a);
    st4(g_prev + o, gp);
    gmx = max_abs4(gmx, gp);
    s1 = add4(s1, gp);
    s2 = fma4(gp, sub4(yv, bnp.mean), s2);
  }
  raise_gmax(bn_prev, C, gmx);
  if (part) pix_partials(t, s1, s2, part, C, sm);
  if (WGRAD) {
    float* row = rowsbuf + (size_t)blockIdx.x * C * 9;
#pragma unroll
    for (int k = 0; k < (WGRAD ? 9 : 1); ++k) {
      const float4 s = pix_reduce(dwa[k], sm);
      if (t.pl == 0 && t.active) {
        row[(size_t)(t.c + 0) * 9 + k] = s.x;
        row[(size_t)(t.c + 1) * 9 + k] = s.y;
        row[(size_t)(t.c + 2) * 9 + k] = s.z;
        row[(size_t)(t.c + 3) * 9 + k] = s.w;
      }
    }
  }
}

// ---- global average pool -------------------------------------------------------------------------------------------------------------
// thread = (sample, channel quad)
__global__ void __launch_bounds__(kBlock) avgpool_fwd_k(const float* __restrict__ y, const float* __restrict__ bnp, const float* __restrict__ skip,
                                                         float* __restrict__ feat, int B, int HW, int C) {
  const int quads = C >> 2;
  const int64_t items = (int64_t)B * quads, M = (int64_t)B * HW;
  const float inv = 1.0f / (float)HW;
  for (int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x; idx < items; idx += (int64_t)gridDim.x * kBlock) {
    const int c = 4 * (int)(idx % quads), n = (int)(idx / quads);
    const BnApply4 bn = BnApply4::load(bnp, C, c);
    float4 s = f4(0.f);
    for (int p = 0; p < HW; ++p) {
      const size_t o = off((int64_t)n * HW + p, c, M, C);
      s = add4(s, skip ? bn.act(ld4(y + o), ld4(skip + o)) : bn.act(ld4(y + o)));
    }
    st4(feat + (size_t)n * C + c, make_float4(s.x * inv, s.y * inv, s.z * inv, s.w * inv));
  }
}

__global__ void __launch_bounds__(kBlock) avgpool_bwd_k(const float* __restrict__ gfeat, const float* __restrict__ y, float* __restrict__ bnp,
                                                         const float* __restrict__ skip, float* __restrict__ g, float* __restrict__ part, int B,
                                                         int HW, int C) {
  __shared__ float4 sm[kPixLanes * 8];
  const PixThread t(C);
  const int64_t M = (int64_t)B * HW;
  const BnApply4 bn = BnApply4::load(bnp, C, t.active ? t.c : 0);
  const float inv = 1.0f / (float)HW;
  const size_t base = blk_base(M, t.cb) + 4 * t.q;
  float4 s1 = f4(0.f), s2 = f4(0.f);
  float gmx = 0.f;
  for (int64_t m = (int64_t)blockIdx.x * kPixLanes + t.pl; m < M; m += (int64_t)gridDim.x * kPixLanes) {
    if (!t.active) continue;
    const int n = (int)(m / HW);
    const size_t o = base + (size_t)m * t.wb;
    const float4 yv = ld4(y + o);
    const float4 a = skip ? bn.act(yv, ld4(skip + o)) : bn.act(yv);
    float4 gv = ld4(gfeat + (size_t)n * C + t.c);
    gv = mask4(make_float4(gv.x * inv, gv.y * inv, gv.z * inv, gv.w * inv), a);
    st4(g + o, gv);
    gmx = max_abs4(gmx, gv);
    s1 = add4(s1, gv);
    s2 = fma4(gv, sub4(yv, bn.mean), s2);
  }
  raise_gmax(bnp, C, gmx);
  if (part) pix_partials(t, s1, s2, part, C, sm);
}

// a[rows][C] (plain channels-last) = max(bn(y) (+ skip), 0)
__global__ void __launch_bounds__(kBlock) bn_act_k(const float* __restrict__ y, const float* __restrict__ bnp, const float* __restrict__ skip,
                                                    float* __restrict__ a, int64_t M, int C) {
  const int quads = C >> 2;
  const int64_t items = M * quads;
  for (int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x; idx < items; idx += (int64_t)gridDim.x * kBlock) {
    const int c = 4 * (int)(idx % quads);
    const int64_t m = idx / quads;
    const BnApply4 bn = BnApply4::load(bnp, C, c);
    const size_t o = off(m, c, M, C);
    st4(a + (size_t)m * C + c, skip ? bn.act(ld4(y + o), ld4(skip + o)) : bn.act(ld4(y + o)));
  }
}

static int grid_1d(int64_t items) {
  int64_t g = ceil_div(items, kBlock);
  return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}

}  // namespace anyc
}  // namespace ttk

using namespace ttk;
using namespace ttk::anyc;

extern "C" {

int ttk_anyc_partial_rows(int64_t pixels) { return pix_rows(pixels); }

int ttk_anyc_stem_fwd(const float* x, const float* w, float* y, float* part, const float* pivot, int B, int H, int W, int Cout,
                      ttk_stream_t stream) {
  TTK_REQUIRE(x && w && y, "anyc_stem_fwd: null pointer");
  TTK_REQUIRE(B > 0 && H > 4 && W > 4 && c_ok(Cout), "anyc_stem_fwd: unsupported shape B=%d H=%d W=%d Cout=%d (Cout: a multiple of 8 in 8..2048)", B, H, W, Cout);
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  TTK_REQUIRE((int64_t)B * H * W < (int64_t)1 << 31, "anyc_stem_fwd: too many pixels for 32-bit indexing");
  hipLaunchKernelGGL(stem_fwd_k, dim3(pix_rows((int64_t)B * Ho * Wo), n_blk(Cout)), dim3(kBlock), 0, (hipStream_t)stream, x, w, y, part, pivot, B, H, W,
                     Ho, Wo, Cout);
  TTK_LAUNCH_CHECK("anyc_stem_fwd");
}

size_t ttk_anyc_stem_wgrad_scratch_bytes(int B, int H, int W, int Cout) {
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  return (size_t)pix_rows((int64_t)B * Ho * Wo) * 25 * Cout * sizeof(float);
}

int ttk_anyc_stem_bwd_weight(const float* g, const float* y, const float* bn, const float* x, float* dw, int accumulate, float* scratch, int B,
                             int H, int W, int Cout, ttk_stream_t stream) {
  TTK_REQUIRE(g && y && bn && x && dw && scratch, "anyc_stem_bwd_weight: null pointer");
  TTK_REQUIRE(B > 0 && H > 4 && W > 4 && c_ok(Cout), "anyc_stem_bwd_weight: unsupported shape B=%d H=%d W=%d Cout=%d", B, H, W, Cout);
  TTK_REQUIRE((int64_t)B * H * W < (int64_t)1 << 31, "anyc_stem_bwd_weight: too many pixels for 32-bit indexing");
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const int rows = pix_rows((int64_t)B * Ho * Wo);
  hipLaunchKernelGGL(stem_wgrad_k, dim3(rows, n_blk(Cout)), dim3(kBlock), 0, (hipStream_t)stream, g, y, bn, x, scratch, B, H, W, Ho, Wo, Cout);
  launch_fold_partials(scratch, rows, (int64_t)Cout * 25, dw, accumulate, (hipStream_t)stream);
  TTK_LAUNCH_CHECK("anyc_stem_bwd_weight");
}

int ttk_anyc_dw_fwd(const float* yprev, const float* bn_prev, const float* skip_prev, float* a_out, const float* w, float* y, float* part,
                    const float* pivot, int B, int H, int W, int C, int stride, ttk_stream_t stream) {
  TTK_REQUIRE(yprev && bn_prev && w && y, "anyc_dw_fwd: null pointer");
  TTK_REQUIRE(B > 0 && H > 0 && W > 0 && c_ok(C) && (stride == 1 || stride == 2), "anyc_dw_fwd: unsupported shape B=%d H=%d W=%d C=%d stride=%d", B, H, W,
              C, stride);
  TTK_REQUIRE(!a_out || stride == 1, "anyc_dw_fwd: a_out (the materialised block input of a residual block) needs stride 1");
  TTK_REQUIRE((int64_t)B * H * W < (int64_t)1 << 31, "anyc_dw_fwd: too many pixels for 32-bit indexing");
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  hipLaunchKernelGGL(dw_fwd_k, dim3(pix_rows((int64_t)B * Ho * Wo), n_blk(C)), dim3(kBlock), 0, (hipStream_t)stream, yprev, bn_prev, skip_prev, a_out, w,
                     y, part, pivot, B, H, W, Ho, Wo, C, stride);
  TTK_LAUNCH_CHECK("anyc_dw_fwd");
}

size_t ttk_anyc_dw_wgrad_scratch_bytes(int B, int H, int W, int C) { return (size_t)pix_rows((int64_t)B * H * W) * 9 * C * sizeof(float); }

int ttk_anyc_dw_bwd_data(const float* g_dw, const float* y_dw, const float* bn_dw, const float* w, const float* skip_grad, const float* yprev,
                         float* bn_prev, const float* skip_prev, const float* a_in, float* g_prev, float* part, float* dw, int dw_accumulate,
                         float* dw_scratch, int B, int H, int W, int C, int stride, ttk_stream_t stream) {
  TTK_REQUIRE(g_dw && y_dw && bn_dw && w && yprev && bn_prev && g_prev, "anyc_dw_bwd_data: null pointer");
  TTK_REQUIRE(B > 0 && H > 0 && W > 0 && c_ok(C) && (stride == 1 || stride == 2), "anyc_dw_bwd_data: unsupported shape B=%d H=%d W=%d C=%d stride=%d", B,
              H, W, C, stride);
  TTK_REQUIRE(!dw || dw_scratch, "anyc_dw_bwd_data: the fused weight gradient needs dw_scratch (ttk_anyc_dw_wgrad_scratch_bytes)");
  TTK_REQUIRE((int64_t)B * H * W < (int64_t)1 << 31, "anyc_dw_bwd_data: too many pixels for 32-bit indexing");
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const int rows = pix_rows((int64_t)B * H * W);
  const dim3 grid(rows, n_blk(C));
  if (dw) {
    hipLaunchKernelGGL(dw_bwd_k<true>, grid, dim3(kBlock), 0, (hipStream_t)stream, g_dw, y_dw, bn_dw, w, skip_grad, yprev, bn_prev, skip_prev, a_in,
                       g_prev, part, dw_scratch, B, H, W, Ho, Wo, C, stride);
    launch_fold_partials(dw_scratch, rows, (int64_t)C * 9, dw, dw_accumulate, (hipStream_t)stream);
  } else {
    hipLaunchKernelGGL(dw_bwd_k<false>, grid, dim3(kBlock), 0, (hipStream_t)stream, g_dw, y_dw, bn_dw, w, skip_grad, yprev, bn_prev, skip_prev, a_in,
                       g_prev, part, nullptr, B, H, W, Ho, Wo, C, stride);
  }
  TTK_LAUNCH_CHECK("anyc_dw_bwd_data");
}

int ttk_anyc_avgpool_fwd(const float* y, const float* bn, const float* skip, float* feat, int B, int HW, int C, ttk_stream_t stream) {
  TTK_REQUIRE(y && bn && feat, "anyc_avgpool_fwd: null pointer");
  TTK_REQUIRE(B > 0 && HW > 0 && c_ok(C), "anyc_avgpool_fwd: unsupported shape B=%d HW=%d C=%d", B, HW, C);
  hipLaunchKernelGGL(anyc::avgpool_fwd_k, dim3(grid_1d((int64_t)B * (C / 4))), dim3(kBlock), 0, (hipStream_t)stream, y, bn, skip, feat, B, HW, C);
  TTK_LAUNCH_CHECK("anyc_avgpool_fwd");
}

int ttk_anyc_avgpool_bwd(const float* gfeat, const float* y, float* bn, const float* skip, float* g, float* part, int B, int HW, int C,
                         ttk_stream_t stream) {
  TTK_REQUIRE(gfeat && y && bn && g, "anyc_avgpool_bwd: null pointer");
  TTK_REQUIRE(B > 0 && HW > 0 && c_ok(C), "anyc_avgpool_bwd: unsupported shape B=%d HW=%d C=%d", B, HW, C);
  TTK_REQUIRE((int64_t)B * HW < (int64_t)1 << 31, "anyc_avgpool_bwd: too many pixels for 32-bit indexing");
  hipLaunchKernelGGL(anyc::avgpool_bwd_k, dim3(pix_rows((int64_t)B * HW), n_blk(C)), dim3(kBlock), 0, (hipStream_t)stream, gfeat, y, bn, skip, g, part, B,
                     HW, C);
  TTK_LAUNCH_CHECK("anyc_avgpool_bwd");
}

int ttk_anyc_bn_act(const float* y, const float* bn, const float* skip, float* a, int64_t rows, int C, ttk_stream_t stream) {
  TTK_REQUIRE(y && bn && a, "anyc_bn_act: null pointer");
  TTK_REQUIRE(rows > 0 && c_ok(C), "anyc_bn_act: unsupported shape rows=%lld C=%d", (long long)rows, C);
  hipLaunchKernelGGL(anyc::bn_act_k, dim3(grid_1d(rows * (C / 4))), dim3(kBlock), 0, (hipStream_t)stream, y, bn, skip, a, rows, C);
  TTK_LAUNCH_CHECK("anyc_bn_act");
}

}  // extern "C"
