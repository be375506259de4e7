// Pointwise 1x1 convolutions of the any-channel-count family (anyc_common.h) on the exact-fp32 matrix instruction
// v_mfma_f32_32x32x2_f32: forward, data gradient, weight gradient for Cin, Cout multiples of 8 in 8..2048.
//
// Operand map of the instruction: lane l = (i = l & 31, h = l >> 5) supplies A[i][k = h] and B[k = h][j = i].  Which two k of the reduction a
// step multiplies is free as long as both operands agree, so a lane loads FOUR consecutive k (k0 + 4h .. k0 + 4h + 3: one 16-byte load where k is
// the contiguous axis) and four steps consume them - eight k per group, which is why the family's channel counts are multiples of 8: a group
// never straddles a channel block.  C/D map: column = l & 31, row = (r & 3) + 8 (r >> 2) + 4 h for accumulator register r.
// A tile narrower than 32 (the last channel block of 8, 16 or 24; the last rows of M) is padded with zeros in registers, never in memory.
#include "anyc_common.h"

namespace ttk {
namespace anyc {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ f32x16 mfma4(float4 a, float4 b, f32x16 c) {
  c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, c, 0, 0, 0);
  return c;
}
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// The workgroup's row of BatchNorm partial sums from per-lane column sums: s1[j], s2[j] of column (lane & 31) of tile j, already summed over the
// lane's 16 rows.  The two halves of a wave meet by shuffle, the four waves in LDS in wave order (fixed).
__device__ __forceinline__ void gemm_partials(float (&s1)[2], float (&s2)[2], float* part_row, int n0, int N, float (*sm)[2][64]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    s1[j] += __shfl_xor(s1[j], 32);
    s2[j] += __shfl_xor(s2[j], 32);
    if (lane < 32) {
      sm[wv][0][32 * j + lane] = s1[j];
      sm[wv][1][32 * j + lane] = s2[j];
    }
  }
  __syncthreads();
  if (threadIdx.x < 128) {
    const int which = threadIdx.x >> 6, col = threadIdx.x & 63;
    if (n0 + col < N) part_row[(size_t)which * N + n0 + col] = ((sm[0][which][col] + sm[1][which][col]) + sm[2][which][col]) + sm[3][which][col];
  }
}

// y[M][Cout] = relu(bn_dw(ydw))[M][Cin] . w[Cout][Cin]^T.  Workgroup: 128 rows (one 32-row tile per wave) x 64 columns (two tiles per wave).
__global__ void __launch_bounds__(kBlock) pw_fwd_k(const float* __restrict__ ydw, const float* __restrict__ bn_dw, const float* __restrict__ w,
                                                    float* __restrict__ y, float* __restrict__ part, const float* __restrict__ pivot, int64_t M, int Cin,
                                                    int Cout, int ntiles) {
  __shared__ float sm[4][2][64];
  const int nt = blockIdx.x % ntiles;
  const int64_t mt = blockIdx.x / ntiles;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, i = lane & 31, h = lane >> 5;
  const int n0 = nt * 64;
  const int64_t m0 = mt * 128 + wv * 32, row = m0 + i;
  const bool rok = row < M;
  f32x16 acc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  const int kblocks = n_blk(Cin);
  for (int kb = 0; kb < kblocks; ++kb) {
    const int wbk = blk_w(Cin, kb);
    const float* ap = ydw + blk_base(M, kb) + (size_t)(rok ? row : 0) * wbk + 4 * h;
    for (int kk = 0; kk < wbk; kk += 8) {
      const int k = (kb << 5) + kk + 4 * h;
      const BnApply4 bn = BnApply4::load(bn_dw, Cin, k);
      const float4 a = rok ? bn.act(ld4(ap + kk)) : f4(0.f);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = n0 + 32 * j + i;
        const float4 b = col < Cout ? ld4(w + (size_t)col * Cin + k) : f4(0.f);
        acc[j] = mfma4(a, b, acc[j]);
      }
    }
  }
  float s1[2] = {0.f, 0.f}, s2[2] = {0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c0 = n0 + 32 * j;
    if (c0 >= Cout) continue;
    const int wbo = blk_w(Cout, c0 >> 5);
    if (i >= wbo) continue;
    const float pv = pivot ? pivot[c0 + i] : 0.f;
    float* yb = y + blk_base(M, c0 >> 5) + i;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t m = m0 + acc_row(r, h);
      if (m < M) {
        const float v = acc[j][r];
        yb[(size_t)m * wbo] = v;
        const float d = v - pv;
        s1[j] += d;
        s2[j] = fmaf(d, d, s2[j]);
      }
    }
  }
  if (part) gemm_partials(s1, s2, part + (size_t)mt * 2 * Cout, n0, Cout, sm);
}

// g_dw[M][Cin] = (dy[M][Cout] . w[Cout][Cin]) * [bn_dw(ydw) > 0],  dy = ga*(g - gmean) + gb*(y - mean) of bn_pw on load
__global__ void __launch_bounds__(kBlock) pw_bwd_data_k(const float* __restrict__ g, const float* __restrict__ y, const float* __restrict__ bn_pw,
                                                         const float* __restrict__ w, const float* __restrict__ ydw, float* __restrict__ bn_dw,
                                                         float* __restrict__ g_dw, float* __restrict__ part, int64_t M, int Cin, int Cout, int ntiles) {
  __shared__ float sm[4][2][64];
  const int nt = blockIdx.x % ntiles;
  const int64_t mt = blockIdx.x / ntiles;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, i = lane & 31, h = lane >> 5;
  const int n0 = nt * 64;
  const int64_t m0 = mt * 128 + wv * 32, row = m0 + i;
  const bool rok = row < M;
  f32x16 acc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  const int kblocks = n_blk(Cout);
  for (int kb = 0; kb < kblocks; ++kb) {
    const int wbk = blk_w(Cout, kb);
    const size_t ao = blk_base(M, kb) + (size_t)(rok ? row : 0) * wbk + 4 * h;
    for (int kk = 0; kk < wbk; kk += 8) {
      const int k = (kb << 5) + kk + 4 * h;
      const BnGrad4 bn = BnGrad4::load(bn_pw, Cout, k);
      const float4 a = rok ? bn.dy(ld4(g + ao + kk), ld4(y + ao + kk)) : f4(0.f);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = n0 + 32 * j + i;
        float4 b = f4(0.f);
        if (col < Cin) {
          const float* wp = w + (size_t)k * Cin + col;
          b = make_float4(wp[0], wp[Cin], wp[2 * (size_t)Cin], wp[3 * (size_t)Cin]);
        }
        acc[j] = mfma4(a, b, acc[j]);
      }
    }
  }
  float s1[2] = {0.f, 0.f}, s2[2] = {0.f, 0.f};
  float gmx = 0.f;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c0 = n0 + 32 * j;
    if (c0 >= Cin) continue;
    const int wbo = blk_w(Cin, c0 >> 5);
    if (i >= wbo) continue;
    const int c = c0 + i;
    const float scale = bn_dw[TTK_BN_SCALE * Cin + c], mean = bn_dw[TTK_BN_MEAN * Cin + c], beta = bn_dw[TTK_BN_BETA * Cin + c];
    const size_t base = blk_base(M, c0 >> 5) + i;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t m = m0 + acc_row(r, h);
      if (m < M) {
        const size_t o = base + (size_t)m * wbo;
        const float yc = ydw[o] - mean;
        const float gv = fmaf(scale, yc, beta) > 0.f ? acc[j][r] : 0.f;
        g_dw[o] = gv;
        gmx = fmaxf(gmx, fabsf(gv));
        s1[j] += gv;
        s2[j] = fmaf(gv, yc, s2[j]);
      }
    }
  }
  raise_gmax(bn_dw, Cin, gmx);
  if (part) gemm_partials(s1, s2, part + (size_t)mt * 2 * Cin, n0, Cin, sm);
}

// slice[s][Cout][Cin] = sum over the slice's rows of dy[m][co] * a[m][ci].  Workgroup: one 64 x 64 tile of dW (a 32 x 32 tile per wave) over one slice of M.
__global__ void __launch_bounds__(kBlock) pw_wgrad_k(const float* __restrict__ g, const float* __restrict__ y, const float* __restrict__ bn_pw,
                                                      const float* __restrict__ ydw, const float* __restrict__ bn_dw, float* __restrict__ slices,
                                                      int64_t M, int Cin, int Cout, int ci_tiles, int64_t rows_per_slice) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, i = lane & 31, h = lane >> 5;
  const int co0 = (blockIdx.x / ci_tiles) * 64 + 32 * (wv >> 1), ci0 = (blockIdx.x % ci_tiles) * 64 + 32 * (wv & 1);
  if (co0 >= Cout || ci0 >= Cin) return;  // (no barrier below)
  const int wbo = blk_w(Cout, co0 >> 5), wbi = blk_w(Cin, ci0 >> 5);
  const bool ook = i < wbo, iok = i < wbi;
  const int co = ook ? co0 + i : co0, ci = iok ? ci0 + i : ci0;
  const float ga = bn_pw[TTK_BN_GA * Cout + co], gb = bn_pw[TTK_BN_GB * Cout + co], gmean = bn_pw[TTK_BN_GMEAN * Cout + co],
              pmean = bn_pw[TTK_BN_MEAN * Cout + co];
  const float scale = bn_dw[TTK_BN_SCALE * Cin + ci], dmean = bn_dw[TTK_BN_MEAN * Cin + ci], beta = bn_dw[TTK_BN_BETA * Cin + ci];
  const float* gp = g + blk_base(M, co0 >> 5) + (co - co0);
  const float* yp = y + blk_base(M, co0 >> 5) + (co - co0);
  const float* ap = ydw + blk_base(M, ci0 >> 5) + (ci - ci0);
  const int64_t mb = (int64_t)blockIdx.y * rows_per_slice;
  const int64_t me = mb + rows_per_slice < M ? mb + rows_per_slice : M;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int64_t m0 = mb; m0 < me; m0 += 8) {
    float av[4], bv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int64_t m = m0 + 4 * h + t;
      const bool ok = m < me;
      const size_t mm = ok ? (size_t)m : (size_t)mb;
      const float gv = gp[mm * wbo], yv = yp[mm * wbo], dv = ap[mm * wbi];
      av[t] = (ok && ook) ? fmaf(ga, gv - gmean, gb * (yv - pmean)) : 0.f;
      bv[t] = (ok && iok) ? fmaxf(fmaf(scale, dv - dmean, beta), 0.f) : 0.f;
    }
    acc = mfma4(make_float4(av[0], av[1], av[2], av[3]), make_float4(bv[0], bv[1], bv[2], bv[3]), acc);
  }
  float* out = slices + (size_t)blockIdx.y * Cout * Cin;
  if (iok) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rr = acc_row(r, h);
      if (rr < wbo) out[(size_t)(co0 + rr) * Cin + ci0 + i] = acc[r];
    }
  }
}

// slices of M of the weight gradient: enough (tile, slice) pairs to fill the GPU, at most 16 MiB of scratch
static int wgrad_slices(int64_t M, int Cin, int Cout) {
  const int64_t tiles = (int64_t)n_blk(Cin) * n_blk(Cout);
  int64_t s = 4096 / tiles;
  const int64_t most = ceil_div(M, 64);
  if (s > most) s = most;
  return (int)(s < 1 ? 1 : s);
}

}  // namespace anyc
}  // namespace ttk

using namespace ttk;
using namespace ttk::anyc;

extern "C" {

int ttk_anyc_pw_fwd(const float* ydw, const float* bn_dw, const float* w, float* y, float* part, const float* pivot, int64_t M, int Cin, int Cout,
                    ttk_stream_t stream) {
  TTK_REQUIRE(ydw && bn_dw && w && y, "anyc_pw_fwd: null pointer");
  TTK_REQUIRE(M > 0 && M < ((int64_t)1 << 31) && c_ok(Cin) && c_ok(Cout), "anyc_pw_fwd: unsupported shape M=%lld Cin=%d Cout=%d (multiples of 8 in 8..2048)",
              (long long)M, Cin, Cout);
  const int ntiles = (Cout + 63) / 64;
  const int64_t grid = ceil_div(M, 128) * ntiles;
  TTK_REQUIRE(grid < ((int64_t)1 << 31), "anyc_pw_fwd: grid too large");
  hipLaunchKernelGGL(pw_fwd_k, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, ydw, bn_dw, w, y, part, pivot, M, Cin, Cout, ntiles);
  TTK_LAUNCH_CHECK("anyc_pw_fwd");
}

int ttk_anyc_pw_bwd_data(const float* g, const float* y, const float* bn_pw, const float* w, const float* ydw, float* bn_dw, float* g_dw,
                         float* part, int64_t M, int Cin, int Cout, ttk_stream_t stream) {
  TTK_REQUIRE(g && y && bn_pw && w && ydw && bn_dw && g_dw, "anyc_pw_bwd_data: null pointer");
  TTK_REQUIRE(M > 0 && M < ((int64_t)1 << 31) && c_ok(Cin) && c_ok(Cout), "anyc_pw_bwd_data: unsupported shape M=%lld Cin=%d Cout=%d", (long long)M, Cin,
              Cout);
  const int ntiles = (Cin + 63) / 64;
  const int64_t grid = ceil_div(M, 128) * ntiles;
  TTK_REQUIRE(grid < ((int64_t)1 << 31), "anyc_pw_bwd_data: grid too large");
  hipLaunchKernelGGL(pw_bwd_data_k, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, g, y, bn_pw, w, ydw, bn_dw, g_dw, part, M, Cin, Cout,
                     ntiles);
  TTK_LAUNCH_CHECK("anyc_pw_bwd_data");
}

size_t ttk_anyc_pw_wgrad_scratch_bytes(int64_t M, int Cin, int Cout) {
  if (M <= 0 || !c_ok(Cin) || !c_ok(Cout)) return 0;
  return (size_t)wgrad_slices(M, Cin, Cout) * Cin * Cout * sizeof(float);
}

int ttk_anyc_pw_bwd_weight(const float* g, const float* y, const float* bn_pw, const float* ydw, const float* bn_dw, float* dw, int accumulate,
                           float* scratch, int64_t M, int Cin, int Cout, ttk_stream_t stream) {
  TTK_REQUIRE(g && y && bn_pw && ydw && bn_dw && dw && scratch, "anyc_pw_bwd_weight: null pointer");
  TTK_REQUIRE(M > 0 && M < ((int64_t)1 << 31) && c_ok(Cin) && c_ok(Cout), "anyc_pw_bwd_weight: unsupported shape M=%lld Cin=%d Cout=%d", (long long)M, Cin,
              Cout);
  const int slices = wgrad_slices(M, Cin, Cout);
  const int64_t rows_per = ceil_div(ceil_div(M, slices), 8) * 8;
  const int ci_tiles = (Cin + 63) / 64, co_tiles = (Cout + 63) / 64;
  hipLaunchKernelGGL(pw_wgrad_k, dim3(ci_tiles * co_tiles, slices), dim3(kBlock), 0, (hipStream_t)stream, g, y, bn_pw, ydw, bn_dw, scratch, M, Cin, Cout,
                     ci_tiles, rows_per);
  launch_fold_partials(scratch, slices, (int64_t)Cin * Cout, dw, accumulate, (hipStream_t)stream);
  TTK_LAUNCH_CHECK("anyc_pw_bwd_weight");
}

}  // extern "C"
