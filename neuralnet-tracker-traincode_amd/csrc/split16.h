// The two-piece fp16 operand split of the fp32 GEMMs on the fp16 matrix pipe - one definition for every file that forms, stores or
// reads such operands: pwconv.hip (prepared weights), pwconv_f16.hip, pwconv_r.hip, pw_bwd_fused.hip, conv.hip and resnet.hip.
// (bc_common.h - bf16 compute - and anyc_common.h have operand formats of their own.)
//
// Arithmetic.  Every fp32 operand value x of a tensor with a known magnitude bound is scaled by a power of two S (exact)
// so that |x S| < 2^15 and cut into two fp16 pieces,
//     h = fp16(x S)  (round to nearest, 11 significant bits),   l = fp16(x S - h)   (the next 11 bits; x S - h is exact),
// so x S = h + l up to 2^-23 |x S|.  A product a*b is accumulated in fp32 as  h_a l_b + l_a h_b + h_a h_b  (three
// v_mfma_f32_32x32x16_f16, each piece product exact in fp32; the dropped l_a l_b is below 2^-24 |a b|) and the tile is
// multiplied by 1/(S_a S_b) on its way out.  Measured against an fp64 product this is as close as a chain of fp32 fmas
// (tests/test_pwconv_gpu.py holds every shape to that criterion; tools/exp/split16.py is the numpy model) - the same
// accuracy class as round 1's 3-piece bf16 split (six products) at HALF the matrix work, two thirds of the LDS and L2
// bytes and a cheaper conversion (v_cvt_pk_f16_f32 instead of mask/subtract chains).
//
// Range.  fp16 has 5 exponent bits: pieces below 2^-14 lose bits and anything above 65504 overflows, so each operand
// tensor carries an upper bound of its magnitude (row TTK_BN_AUX of the BatchNorm block that forms it, include/ttk.h):
// S = 2^(14 - floor(log2 bound)).  Elements down to 2^-17 of the bound keep all 22 bits; smaller ones keep an ABSOLUTE
// error of 2^-40 of the bound, far below the fp32 rounding of the elements that dominate a sum.  Bounds come from the
// statistics the step has anyway (bn.hip: Cauchy-Schwarz on the batch variance forward, the producer's max|g| backward).
//
// The accuracy tests pin exactly the expressions below.  Two kernels form pieces in place instead, to the same values: pw16m_k
// (pwconv_r.hip) cuts h and l in separate phases of its schedule, l by v_fma_mix (rlow2), and the fused backward kernels
// (pw_bwd_fused.hip) cut the raw weights they keep in registers element by element.
#pragma once
#include "ttk_common.h"

namespace ttk {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// Power-of-two scale S of an operand: bound * S lies in [2^14, 2^15), so every scaled value is below the fp16 maximum;
// 1 when the bound is unknown (<= 0, inf, nan).  |log2 S| <= 60: products of two scales and their reciprocals stay
// inside the fp32 exponent range.
__host__ __device__ inline float pow2_scale(float bound) {
  if (!(bound > 0.f) || bound > 3.0e38f) return 1.f;
  union { float f; unsigned u; } b;
  b.f = bound;
  int s = 14 - ((int)((b.u >> 23) & 0xffu) - 127);
  s = s > 60 ? 60 : (s < -60 ? -60 : s);
  b.u = (unsigned)(s + 127) << 23;
  return b.f;
}

// The pieces of ONE (already scaled) value - the weight-plane kernels
__device__ __forceinline__ void split16(float xs, uint16_t& h, uint16_t& l) {
  const _Float16 hh = (_Float16)xs;
  const _Float16 ll = (_Float16)(xs - (float)hh);
  h = __builtin_bit_cast(uint16_t, hh);
  l = __builtin_bit_cast(uint16_t, ll);
}
// ... of two values, each pair packed in 4 bytes
__device__ __forceinline__ void split16x2(float a, float b, unsigned& h, unsigned& l) {
  const f16x2 hh = __builtin_convertvector(f32x2{a, b}, f16x2);
  const f32x2 back = __builtin_convertvector(hh, f32x2);
  const f16x2 ll = __builtin_convertvector(f32x2{a - back.x, b - back.y}, f16x2);
  h = __builtin_bit_cast(unsigned, hh);
  l = __builtin_bit_cast(unsigned, ll);
}
// ... of 4 consecutive-k values: 8 bytes per piece
__device__ __forceinline__ void split16x4(f32x4 v, uint2& h, uint2& l) {
  const f16x2 h01 = __builtin_convertvector(f32x2{v.x, v.y}, f16x2), h23 = __builtin_convertvector(f32x2{v.z, v.w}, f16x2);
  const f32x2 f01 = __builtin_convertvector(h01, f32x2), f23 = __builtin_convertvector(h23, f32x2);
  const f16x2 l01 = __builtin_convertvector(f32x2{v.x - f01.x, v.y - f01.y}, f16x2);
  const f16x2 l23 = __builtin_convertvector(f32x2{v.z - f23.x, v.w - f23.y}, f16x2);
  h = make_uint2(__builtin_bit_cast(unsigned, h01), __builtin_bit_cast(unsigned, h23));
  l = make_uint2(__builtin_bit_cast(unsigned, l01), __builtin_bit_cast(unsigned, l23));
}
// ... written at dst (h) and dst + plane (l)
__device__ __forceinline__ void split_store16(f32x4 v, unsigned char* dst, int plane) {
  uint2 h, l;
  split16x4(v, h, l);
  *reinterpret_cast<uint2*>(dst) = h;
  *reinterpret_cast<uint2*>(dst + plane) = l;
}

// *wmax = max |w| of a weight tensor of n elements: the bound its pieces are scaled by (pow2_scale).  Raised as ordered uint bits
// (non-negative floats order like their bit patterns) from zero.  One kernel for every per-call weight split: pwconv_f16.hip,
// pwconv_r.hip, ttk_conv_weight_repack.
template <int kDummy = 0>
__global__ void __launch_bounds__(256) w16_absmax_k(const float* __restrict__ w, int64_t n, unsigned* __restrict__ wmax) {
  float m = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) m = fmaxf(m, fabsf(w[i]));
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
  if ((threadIdx.x & 63) == 0 && __float_as_uint(m) > __hip_atomic_load(wmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMax(wmax, __float_as_uint(m));
}
template <int kDummy = 0>  // (a template so that only the files that launch it hold a copy of the kernel)
void launch_w16_absmax(const float* w, int64_t n, float* wmax, hipStream_t st) {
  (void)hipMemsetAsync(wmax, 0, sizeof(float), st);
  hipLaunchKernelGGL(w16_absmax_k<kDummy>, dim3((unsigned)(n / 1024 < 1 ? 1 : (n / 1024 > 256 ? 256 : n / 1024))), dim3(256), 0, st, w, n,
                     reinterpret_cast<unsigned*>(wmax));
}

// Byte offset of 16-byte chunk `chunk` (0 / 1) of row `row` inside the LDS image of one piece plane of a k16 stage (32 B per row): the two
// chunks are swapped where (row >> 3) & 1, which spreads a wave's ds_read_b128 fragment reads over all banks (r_plane_index, conv_geom.h,
// is the same order in elements)
__device__ __forceinline__ int swz16(int row, int chunk) { return row * 32 + ((chunk ^ ((row >> 3) & 1)) << 4); }

// 4 consecutive activation values as f32x4 (streamed: non-temporal)
__device__ __forceinline__ f32x4 ld_act4(const float* p) {
  const float4 v = ld4nt(p);
  return f32x4{v.x, v.y, v.z, v.w};
}

}  // namespace ttk
