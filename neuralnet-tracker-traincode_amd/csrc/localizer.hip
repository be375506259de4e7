// The face localizer's inference path (reference: neuralnets/models.py:30-93 LocalizerNet): the tracker's first network, which finds the
// face box in the whole frame.  x [B][224][288] (whitened grey levels) -> out [B][5] = (face logit, x0, y0, x1, y1).  All tensors are
// planar fp32 [B][C][H][W]; the host has folded every BatchNorm into its convolution (include/ttk.h, "parameter block").
//
//   loc_input_k : letterbox of a frame into the 224 x 288 input: every input pixel is the exact area average of the frame over the
//                 pixel's pre-image (outside the frame counts as 0), in double, rows then columns in a fixed order.
//   loc_stem_k  : ONE launch for the 3x3 stride-2 stem (1 -> 8, ReLU) and the first depthwise-separable pair (depthwise 3x3, ReLU,
//                 1x1 8 -> 8).  A workgroup owns 16 x 16 outputs: the 37 x 37 input patch and the 18 x 18 x 8 stem tile live in LDS.
//   loc_block_k : ONE launch per inverted-residual block.  A workgroup owns a TH x TW output tile of one image: the input tile with its
//                 halo, the expanded tensor (Cmid channels, ReLU, zero outside the image as the depthwise convolution pads it) and the
//                 depthwise output live in LDS; the projection adds the residual and stores.  Neither the expanded tensor nor the
//                 depthwise output goes to global memory.  The host picks the largest tile whose three LDS arrays fit 60 KB.
//   loc_head_k  : the 1x1 56 -> 2 convolution with bias, the mean of map 0 (the logit), the softmax over the 63 cells of map 1 and its
//                 centre of mass / deviation (modelcomponents.py CenterOfMassAndStd, half_size 1.5), one workgroup per image.
// 14 launches per forward, all on one stream; every output value is summed serially by one thread: no atomics, bitwise repeatable.
// Plain fp32 FMA arithmetic: the channel counts (12, 20, 56, ...) are no matrix-instruction shapes and the network is ~27 MMAC per frame.
#include <math.h>

#include "localizer_math.h"
#include "ttk_common.h"

namespace ttk {

constexpr int kLocMaxC = 112;           // widest expanded tensor (56 x 2)
constexpr int kLocLdsFloats = 15360;    // 60 KB of a workgroup's 64 KB
constexpr int kLocH1 = kLocH / 2, kLocW1 = kLocW / 2;  // 112 x 144 after the stem
constexpr int kLocStemFloats = 8 * 9 + 8 + 8 * 9 + 8 + 8 * 8 + 8;
constexpr int kLocHeadC = 56, kLocCellsH = 7, kLocCellsW = 9, kLocCells = kLocCellsH * kLocCellsW;
constexpr int kLocHeadFloats = 2 * kLocHeadC + 2 + 2;  // weight, bias, half_size, eps

struct LocBlock { int cin, cout, k, stride, expand; };
// convnet[2:14] of the reference; trackertraincode/neuralnets/models.py LocalizerNet.BLOCKS is the same table
constexpr int kLocNumBlocks = 12;
constexpr LocBlock kLocBlocks[kLocNumBlocks] = {{8, 12, 3, 2, 2},  {12, 12, 3, 1, 2}, {12, 20, 3, 2, 4}, {20, 20, 3, 1, 4},
                                                {20, 20, 3, 1, 4}, {20, 32, 5, 2, 2}, {32, 32, 5, 1, 2}, {32, 32, 3, 1, 2},
                                                {32, 32, 3, 1, 2}, {32, 56, 3, 2, 2}, {56, 56, 3, 1, 2}, {56, 56, 3, 1, 2}};
// per image: buffer A takes the stem's output and every second block's, buffer B the others' (the largest is block 0's)
constexpr size_t kLocBufA = (size_t)8 * kLocH1 * kLocW1, kLocBufB = (size_t)12 * (kLocH1 / 2) * (kLocW1 / 2);

inline int loc_block_floats(int cin, int cmid, int cout, int k) { return cmid * cin + cmid + cmid * k * k + cmid + cout * cmid + cout; }

inline int round4(int v) { return (v + 3) & ~3; }

struct LocTile { int th, tw, lds_floats; };
// the largest tile (from 16 x 18 outputs down, halving the longer side) whose LDS arrays fit: input tile + inside mask + expanded tensor
// over (th - 1) stride + k rows and as many columns, depthwise output over th x tw; a 1 x 1 tile of the widest block takes 27 KB
inline LocTile loc_tile(int Ho, int Wo, int cin, int cmid, int k, int stride) {
  int th = Ho < 16 ? Ho : 16, tw = Wo < 18 ? Wo : 18;
  for (;;) {
    const int ihw = round4(((th - 1) * stride + k) * ((tw - 1) * stride + k));
    const int floats = (cin + cmid + 1) * ihw + cmid * round4(th * tw);
    if (floats <= kLocLdsFloats || (th == 1 && tw == 1)) return LocTile{th, tw, floats};
    if (th >= tw) th = (th + 1) / 2; else tw = (tw + 1) / 2;
  }
}

// grid (tiles, B); dynamic LDS: X [Cin][IHWp], M [IHWp], E [Cmid][IHWp], D [Cmid][THWp] (pixel counts padded to 4 for float4 rows)
__global__ void __launch_bounds__(kBlock) loc_block_k(const float* __restrict__ x, const float* __restrict__ p, int H, int W, int Ho, int Wo,
                                                       int Cin, int Cmid, int Cout, int k, int stride, int residual, int TH, int TW,
                                                       int tiles_x, float* __restrict__ y) {
  extern __shared__ __attribute__((aligned(16))) float loc_smem[];
  const int tid = threadIdx.x;
  const int IH = (TH - 1) * stride + k, IW = (TW - 1) * stride + k;
  const int IHW = IH * IW, IHWp = (IHW + 3) & ~3, THW = TH * TW, THWp = (THW + 3) & ~3, kk = k * k, pad = k / 2;
  float* X = loc_smem;
  float* M = X + Cin * IHWp;
  float* E = M + IHWp;
  float* D = E + Cmid * IHWp;
  const int b = blockIdx.y, oy0 = (blockIdx.x / tiles_x) * TH, ox0 = (blockIdx.x % tiles_x) * TW;
  const int iy0 = oy0 * stride - pad, ix0 = ox0 * stride - pad;
  const float* xb = x + (size_t)b * Cin * H * W;
  const float *w1 = p, *b1 = w1 + Cmid * Cin, *w2 = b1 + Cmid, *b2 = w2 + Cmid * kk, *w3 = b2 + Cmid, *b3 = w3 + Cout * Cmid;

  // the input tile (0 outside the image and in the padding slots) and the inside mask
  for (int idx = tid; idx < (Cin + 1) * IHWp; idx += kBlock) {
    const int ci = idx / IHWp, q = idx - ci * IHWp;
    const int iy = iy0 + q / IW, ix = ix0 + q % IW;
    const bool inside = q < IHW && iy >= 0 && iy < H && ix >= 0 && ix < W;
    if (ci < Cin) X[idx] = inside ? xb[((size_t)ci * H + iy) * W + ix] : 0.f;
    else M[q] = inside ? 1.f : 0.f;
  }
  __syncthreads();
  // expansion 1x1 + ReLU, four pixels per item; outside the image the expanded tensor is 0 (the depthwise convolution's padding)
  const int q4n = IHWp >> 2;
  for (int idx = tid; idx < Cmid * q4n; idx += kBlock) {
    const int m = idx / q4n, q = (idx - m * q4n) << 2;
    float4 a = f4(b1[m]);
    const float* w = w1 + m * Cin;
    for (int ci = 0; ci < Cin; ++ci) a = fma4(f4(w[ci]), ld4(X + ci * IHWp + q), a);
    st4(E + m * IHWp + q, mul4(relu4(a), ld4(M + q)));
  }
  __syncthreads();
  // depthwise k x k + ReLU out of LDS
  for (int idx = tid; idx < Cmid * THWp; idx += kBlock) {
    const int m = idx / THWp, o = idx - m * THWp;
    float a = 0.f;
    if (o < THW) {
      const float* e = E + m * IHWp + (o / TW) * stride * IW + (o % TW) * stride;
      const float* w = w2 + m * kk;
      a = b2[m];
      for (int ky = 0; ky < k; ++ky)
        for (int kx = 0; kx < k; ++kx) a = fmaf(w[ky * k + kx], e[ky * IW + kx], a);
      a = fmaxf(a, 0.f);
    }
    D[idx] = a;
  }
  __syncthreads();
  // projection 1x1 (no activation), the residual, the store
  const int o4n = THWp >> 2;
  for (int idx = tid; idx < Cout * o4n; idx += kBlock) {
    const int co = idx / o4n, o = (idx - co * o4n) << 2;
    float4 a = f4(b3[co]);
    const float* w = w3 + co * Cmid;
    for (int m = 0; m < Cmid; ++m) a = fma4(f4(w[m]), ld4(D + m * THWp + o), a);
    const float v[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int oo = o + e, ly = oo / TW, lx = oo - ly * TW;
      const int oy = oy0 + ly, ox = ox0 + lx;
      if (oo < THW && oy < Ho && ox < Wo) {
        float r = v[e];
        if (residual) r += X[co * IHWp + (ly + pad) * IW + lx + pad];  // stride 1, Cin == Cout: the tile's centre is the block input
        y[(((size_t)b * Cout + co) * Ho + oy) * Wo + ox] = r;
      }
    }
  }
}

// grid (W1 / 16, H1 / 16, B); p: stem w[8][9] b[8], depthwise w[8][9] b[8], pointwise w[8][8] b[8]
constexpr int kStemT = 16, kStemS = kStemT + 2, kStemI = 2 * kStemS + 1;
__global__ void __launch_bounds__(kBlock) loc_stem_k(const float* __restrict__ x, const float* __restrict__ p, float* __restrict__ y) {
  __shared__ float In[kStemI * kStemI];
  __shared__ float S[8][kStemS * kStemS];
  const int tid = threadIdx.x, b = blockIdx.z, oy0 = blockIdx.y * kStemT, ox0 = blockIdx.x * kStemT;
  const float* xb = x + (size_t)b * kLocH * kLocW;
  const float *w0 = p, *b0 = w0 + 72, *w2 = b0 + 8, *b2 = w2 + 72, *w3 = b2 + 8, *b3 = w3 + 64;
  // stem row sy reads input rows 2 sy - 1 .. 2 sy + 1; the stem tile starts at oy0 - 1: input rows from 2 oy0 - 3
  for (int idx = tid; idx < kStemI * kStemI; idx += kBlock) {
    const int iy = 2 * oy0 - 3 + idx / kStemI, ix = 2 * ox0 - 3 + idx % kStemI;
    In[idx] = (iy >= 0 && iy < kLocH && ix >= 0 && ix < kLocW) ? xb[(size_t)iy * kLocW + ix] : 0.f;
  }
  __syncthreads();
  for (int idx = tid; idx < 8 * kStemS * kStemS; idx += kBlock) {
    const int c = idx / (kStemS * kStemS), q = idx - c * (kStemS * kStemS), r = q / kStemS, s = q - r * kStemS;
    const int sy = oy0 - 1 + r, sx = ox0 - 1 + s;
    float a = 0.f;  // outside the stem's output: the depthwise convolution's zero padding
    if (sy >= 0 && sy < kLocH1 && sx >= 0 && sx < kLocW1) {
      a = b0[c];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) a = fmaf(w0[c * 9 + ky * 3 + kx], In[(2 * r + ky) * kStemI + 2 * s + kx], a);
      a = fmaxf(a, 0.f);
    }
    S[c][q] = a;
  }
  __syncthreads();
  const int ly = tid / kStemT, lx = tid % kStemT, oy = oy0 + ly, ox = ox0 + lx;
  if (oy >= kLocH1 || ox >= kLocW1) return;
  float d[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float a = b2[c];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) a = fmaf(w2[c * 9 + ky * 3 + kx], S[c][(ly + ky) * kStemS + lx + kx], a);
    d[c] = fmaxf(a, 0.f);
  }
#pragma unroll
  for (int co = 0; co < 8; ++co) {
    float a = b3[co];
#pragma unroll
    for (int c = 0; c < 8; ++c) a = fmaf(w3[co * 8 + c], d[c], a);
    y[(((size_t)b * 8 + co) * kLocH1 + oy) * kLocW1 + ox] = a;
  }
}

// torch.linspace(-1, 1, n)[i] in float32: from the start in the lower half, from the end in the upper
__device__ __forceinline__ float linspace_pm1(int i, int n) {
  const float step = 2.f / (float)(n - 1);
  return i < n / 2 ? -1.f + step * (float)i : 1.f - step * (float)(n - 1 - i);
}

// grid (B); x [B][56][63]; p: w[2][56], b[2], half_size, eps
__global__ void __launch_bounds__(128) loc_head_k(const float* __restrict__ x, const float* __restrict__ p, float* __restrict__ out,
                                                   float* __restrict__ attention) {
  __shared__ float z[2][kLocCells];
  const int tid = threadIdx.x, b = blockIdx.x;
  const float* xb = x + (size_t)b * kLocHeadC * kLocCells;
  if (tid < 2 * kLocCells) {
    const int mp = tid / kLocCells, cell = tid - mp * kLocCells;
    float a = p[2 * kLocHeadC + mp];
    for (int c = 0; c < kLocHeadC; ++c) a = fmaf(p[mp * kLocHeadC + c], xb[c * kLocCells + cell], a);
    z[mp][cell] = a;
  }
  __syncthreads();
  if (tid == 0) {
    const float half = p[2 * kLocHeadC + 2], eps = p[2 * kLocHeadC + 3];
    float sum = 0.f, mx = z[1][0];
    for (int i = 0; i < kLocCells; ++i) sum += z[0][i], mx = fmaxf(mx, z[1][i]);
    float den = 0.f;
    for (int i = 0; i < kLocCells; ++i) den += (z[1][i] = expf(z[1][i] - mx));
    float mean_x = 0.f, mean_y = 0.f;
    for (int i = 0; i < kLocCells; ++i) {
      const float a = (z[1][i] /= den);
      mean_x += a * linspace_pm1(i % kLocCellsW, kLocCellsW), mean_y += a * linspace_pm1(i / kLocCellsW, kLocCellsH);
    }
    mean_x *= half, mean_y *= half;
    // (the reference's deviation: the unscaled position code against the scaled mean)
    float var_x = 0.f, var_y = 0.f;
    for (int i = 0; i < kLocCells; ++i) {
      const float dx = linspace_pm1(i % kLocCellsW, kLocCellsW) - mean_x, dy = linspace_pm1(i / kLocCellsW, kLocCellsH) - mean_y;
      var_x += z[1][i] * (dx * dx), var_y += z[1][i] * (dy * dy);
    }
    const float sx = sqrtf(var_x + eps), sy = sqrtf(var_y + eps);
    float* o = out + 5 * (size_t)b;
    o[0] = sum / (float)kLocCells, o[1] = mean_x - sx, o[2] = mean_y - sy, o[3] = mean_x + sx, o[4] = mean_y + sy;
  }
  __syncthreads();
  if (attention && tid < kLocCells) attention[(size_t)b * kLocCells + tid] = z[1][tid];
}

// grid (ceil(224 * 288 / 256), S).  Input pixel (X, Y) covers [X, X + 1) x [Y, Y + 1); its pre-image in frame pixels is
// [(X - ox) / s, (X + 1 - ox) / s) x ...; the frame is piecewise constant on its pixels and 0 outside.
template <typename T>
__global__ void __launch_bounds__(kBlock) loc_input_k(const T* __restrict__ frames, int Tn, int Hs, int Ws, const int* __restrict__ t_dev,
                                                       double s, double ox, double oy, float mul, float add, float* __restrict__ x,
                                                       float* __restrict__ lb) {
  const int seq = blockIdx.y, t = t_dev ? *t_dev : 0;
  if (t < 0 || t >= Tn) return;  // uniform: nothing is written
  const int idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx == 0) lb[3 * seq] = (float)s, lb[3 * seq + 1] = (float)ox, lb[3 * seq + 2] = (float)oy;
  if (idx >= kLocH * kLocW) return;
  const int Y = idx / kLocW, X = idx - Y * kLocW;
  const T* img = frames + ((size_t)seq * Tn + t) * ((size_t)Hs * Ws);
  const double x_lo = ((double)X - ox) / s, x_hi = ((double)(X + 1) - ox) / s, y_lo = ((double)Y - oy) / s, y_hi = ((double)(Y + 1) - oy) / s;
  const int jx0 = max(0, (int)floor(x_lo)), jx1 = min(Ws, (int)ceil(x_hi)), jy0 = max(0, (int)floor(y_lo)), jy1 = min(Hs, (int)ceil(y_hi));
  double acc = 0.0;
  for (int jy = jy0; jy < jy1; ++jy) {
    const double wy = fmin(y_hi, (double)(jy + 1)) - fmax(y_lo, (double)jy);
    if (!(wy > 0.0)) continue;
    double row = 0.0;
    for (int jx = jx0; jx < jx1; ++jx) {
      const double wx = fmin(x_hi, (double)(jx + 1)) - fmax(x_lo, (double)jx);
      if (wx > 0.0) row += wx * (double)img[(size_t)jy * Ws + jx];
    }
    acc += wy * row;
  }
  x[(size_t)seq * (kLocH * kLocW) + idx] = fmaf((float)(acc * (s * s)), mul, add);
}

static bool loc_block_args_ok(int B, int H, int W, int Cin, int Cmid, int Cout, int k, int stride, int residual) {
  return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= 4096 && W <= 4096 && Cin >= 1 && Cin <= kLocMaxC && Cmid >= 1 && Cmid <= kLocMaxC &&
         Cout >= 1 && Cout <= kLocMaxC && (k == 3 || k == 5) && (stride == 1 || stride == 2) && (!residual || (Cin == Cout && stride == 1));
}

static void loc_launch_block(const float* x, const float* p, int B, int H, int W, int Cin, int Cmid, int Cout, int k, int stride, int residual,
                             float* y, hipStream_t st) {
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const LocTile t = loc_tile(Ho, Wo, Cin, Cmid, k, stride);
  const int tiles_x = (Wo + t.tw - 1) / t.tw, tiles_y = (Ho + t.th - 1) / t.th;
  hipLaunchKernelGGL(loc_block_k, dim3((unsigned)(tiles_x * tiles_y), (unsigned)B), dim3(kBlock), (size_t)t.lds_floats * sizeof(float), st, x, p,
                     H, W, Ho, Wo, Cin, Cmid, Cout, k, stride, residual ? 1 : 0, t.th, t.tw, tiles_x, y);
}

}  // namespace ttk

using namespace ttk;

extern "C" {

int ttk_localizer_param_floats(void) {
  int n = kLocStemFloats + kLocHeadFloats;
  for (const LocBlock& b : kLocBlocks) n += loc_block_floats(b.cin, b.cin * b.expand, b.cout, b.k);
  return n;
}

size_t ttk_localizer_workspace_bytes(int B) { return B < 1 ? 0 : (size_t)B * (kLocBufA + kLocBufB) * sizeof(float); }

int ttk_localizer_launches(void) { return 1 + kLocNumBlocks + 1; }

int ttk_localizer_forward(const float* x, const float* params, void* workspace, int B, float* out, float* attention, ttk_stream_t stream) {
  TTK_REQUIRE(x && params && workspace && out, "localizer_forward: a required pointer is null");
  TTK_REQUIRE(B >= 1 && B <= 65535, "localizer_forward: 1 <= B <= 65535, got %d", B);
  hipStream_t st = (hipStream_t)stream;
  float* cur = (float*)workspace;
  float* nxt = cur + (size_t)B * kLocBufA;
  hipLaunchKernelGGL(loc_stem_k, dim3(kLocW1 / kStemT, kLocH1 / kStemT, (unsigned)B), dim3(kBlock), 0, st, x, params, cur);
  const float* p = params + kLocStemFloats;
  int H = kLocH1, W = kLocW1;
  for (const LocBlock& b : kLocBlocks) {
    const int cmid = b.cin * b.expand;
    loc_launch_block(cur, p, B, H, W, b.cin, cmid, b.cout, b.k, b.stride, b.cin == b.cout && b.stride == 1, nxt, st);
    p += loc_block_floats(b.cin, cmid, b.cout, b.k);
    H = (H - 1) / b.stride + 1, W = (W - 1) / b.stride + 1;
    float* tmp = cur; cur = nxt; nxt = tmp;
  }
  hipLaunchKernelGGL(loc_head_k, dim3((unsigned)B), dim3(128), 0, st, cur, p, out, attention);
  TTK_LAUNCH_CHECK("localizer_forward");
}

int ttk_localizer_block(const float* x, const float* params, int B, int H, int W, int Cin, int Cmid, int Cout, int k, int stride, int residual,
                        float* y, ttk_stream_t stream) {
  TTK_REQUIRE(x && params && y, "localizer_block: a required pointer is null");
  TTK_REQUIRE(loc_block_args_ok(B, H, W, Cin, Cmid, Cout, k, stride, residual),
              "localizer_block: takes 1 <= B <= 65535, 1 <= H, W <= 4096, channels in [1, %d], k in {3, 5}, stride in {1, 2}, a residual only "
              "with Cin == Cout and stride 1; got B %d, %d x %d, %d -> %d -> %d, k %d, stride %d, residual %d",
              kLocMaxC, B, H, W, Cin, Cmid, Cout, k, stride, residual);
  loc_launch_block(x, params, B, H, W, Cin, Cmid, Cout, k, stride, residual, y, (hipStream_t)stream);
  TTK_LAUNCH_CHECK("localizer_block");
}

int ttk_localizer_input(const void* frames, int src_is_u8, int S, int T, int Hs, int Ws, const int* t_dev, float mul, float add, float* x,
                        float* lb, ttk_stream_t stream) {
  TTK_REQUIRE(frames && x && lb, "localizer_input: a required pointer is null");
  TTK_REQUIRE(S >= 1 && S <= 65535 && T >= 1 && Hs >= 1 && Ws >= 1 && Hs <= 32768 && Ws <= 32768,
              "localizer_input: bad sizes (S %d, T %d, frames %d x %d)", S, T, Hs, Ws);
  const double sx = (double)kLocW / Ws, sy = (double)kLocH / Hs, s = sx < sy ? sx : sy;
  const double ox = 0.5 * (kLocW - Ws * s), oy = 0.5 * (kLocH - Hs * s);
  const dim3 grid((unsigned)ceil_div(kLocH * kLocW, kBlock), (unsigned)S);
  if (src_is_u8)
    hipLaunchKernelGGL(loc_input_k<unsigned char>, grid, dim3(kBlock), 0, (hipStream_t)stream, (const unsigned char*)frames, T, Hs, Ws, t_dev, s,
                       ox, oy, mul, add, x, lb);
  else
    hipLaunchKernelGGL(loc_input_k<float>, grid, dim3(kBlock), 0, (hipStream_t)stream, (const float*)frames, T, Hs, Ws, t_dev, s, ox, oy, mul, add,
                       x, lb);
  TTK_LAUNCH_CHECK("localizer_input");
}

}  // extern "C"
