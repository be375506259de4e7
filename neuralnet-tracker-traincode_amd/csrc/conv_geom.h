// Shared between the pointwise-GEMM files (pwconv*.hip, pw_bwd_fused.hip) and conv.hip: operand / epilogue forms, the implicit-GEMM geometry
// and the layout of the prepared weight blocks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ttk {

// A-operand forms (what the producers compute from the loaded rows) and epilogue forms
// AMODE_PLANES: the A operand arrives already split - A0 / A1 = the h / l fp16 planes [rows][Kc] of x * pow2_scale(bound)
// (ttk_bn_bwd_apply writes dy that way) - and the producers only move it (fp16 kernels)
enum { AMODE_BNRELU = 0, AMODE_BNGRAD = 1, AMODE_PLAIN = 2, AMODE_PLANES = 3 };
enum { EMODE_STATS = 0, EMODE_MASK = 1, EMODE_PLAIN = 2 };

// Implicit-GEMM convolution (ResNet 3x3 / strided 1x1, backbones/resnet.py): the GEMM rows enumerate the pixels of a
// grid (Hg x Wg per image) and the contraction runs over (tap, channel): for tap (kh, kw) row (n, gh, gw) reads the
// source pixel   forward:    (gh*stride - pad + kh, gw*stride - pad + kw)            [grid = output, source = input]
//                transposed: ((gh + pad - kh)/stride, (gw + pad - kw)/stride) if divisible  [grid = input, source = output]
// of a [n][Hs][Ws][Kc] tensor, or contributes zero outside it.  The B operand is [tap][Nout][Kc].
// Parity classes (par = 1; fp16 kernels, transposed stride-2 only): a grid pixel (gh, gw) of a stride-2 data gradient is
// reached by the taps with kh = gh + pad (mod 2) only - 1, 2, 2 or 4 of the 9 taps of a 3x3 kernel, one of the four
// classes of a strided 1x1 kernel - so the launch enumerates the pixels class by class ((gh & 1, gw & 1) = (1,1), (1,0),
// (0,1), (0,0): longest contraction first) and every tile contracts over its class's taps only.  ctile[c] = first tile
// of class c, nimg = images (the rows of class c are nimg x its pixels).
struct ConvGeom {
  int Hs, Ws, Hg, Wg, stride, pad, KW, Kc, transposed;
  int par, nimg, ctile[4];
};

// Layout of a prepared weight block of n = Cin * Cout elements (ttk_pwconv_prepare_weights): [forward operand][data-gradient operand]
// [header: |w| maximum ...].  Every reader of the block takes the offsets from here.
__host__ __device__ inline size_t prep_bwd_offset(size_t n) { return 4 * n; }
__host__ __device__ inline size_t prep_hdr_offset(size_t n) { return 8 * n; }

// ---- launchers and shape predicates of the pointwise GEMM files, declared once (MODE: 0 forward, 1 data gradient) ----
// A `bool` launcher returns false when the shape is not its own (nothing launched) - the caller falls through to the next form.

// pwconv_f16.hip: the compute-bound shapes on the fp16 pipe with 2-piece operand splits (three products) - the default
template <int MODE>
bool launch_f16_gemm(const float* A0, const float* A1, const float* bnA, const float* Bm, float* out, const float* E0, const float* bnE,
                     float* part, int64_t M, int K, int Nout, void* planes, float* wmax, hipStream_t st);
bool f16_gemm_shape(int K, int Nout);
bool launch_f16_wgrad(const float* g, const float* y, const float* bn_pw, const float* ydw, const float* bn_dw, float* dw, float* partial,
                      int64_t M, int Cin, int Cout, hipStream_t st);
size_t f16_wgrad_partial_bytes(int64_t M, int Cin, int Cout);

// the convolutions' forms (conv.hip): Bq = two fp16 planes scaled by pow2_scale(*wmax); a_bound = bound of a plain A operand
bool launch_conv_gemm16(int amode, int emode, const float* A0, const float* A1, const float* bnA, const float* a_bound, const uint16_t* Bq,
                        const float* wmax, float* out, const float* E0, float* bnE, float* part, int64_t M, int K, int Nout,
                        const ConvGeom& geo, hipStream_t st);
bool launch_conv_wgrad16(const float* g, const float* y, const float* bn, const float* a_in, const float* a_bound, float* dw, float* partial,
                         int64_t M, int Cout, int taps, const ConvGeom& geo, hipStream_t st);
size_t conv_wgrad16_partial_bytes(int64_t M, int Cout, int ncols, int taps);

// Row-block GEMMs (pwconv_r.hip): element (row, k) of a [rows][K] weight operand inside one piece plane [K/16][rows][16] whose two
// 16-byte chunks per row are swapped where (row >> 3) & 1 - the LDS image of a k16 stage, so that LDS-DMA copies it linearly
__host__ __device__ inline int64_t r_plane_index(int row, int k, int rows) {
  return ((int64_t)(k >> 4) * rows + row) * 16 + ((((k >> 3) & 1) ^ ((row >> 3) & 1)) << 3) + (k & 7);
}

// pwconv_r.hip: the wide layers (K >= 128, Nout a multiple of 256) in row-block form: 8 consumer waves, variable tile height,
// LDS-DMA weight planes in the [K/16][Nout][16] layout above
template <int MODE>
bool launch_f16r_gemm(const float* A0, const float* A1, const float* bnA, const float* Bm, float* out, const float* E0, const float* bnE,
                      float* part, int64_t M, int K, int Nout, void* planes, float* wmax, hipStream_t st);
bool f16r_gemm_shape(int K, int Nout, int dgrad);
int f16r_partial_rows(int64_t M, int K, int Nout, int dgrad);
int f16r_tile_rows(int64_t M, int K, int Nout, int dgrad);

// pwconv_r.hip: weight gradient of the layers with Cin a multiple of 256 and Cout of 128 (but not 256 -> 256) on 128 (Cout) x 256 (Cin) tiles with
// transposed LDS fragment reads; always reduces through `partial` (scratch of f16t_wgrad_scratch_bytes) and a fixed-order fold
bool launch_f16t_wgrad(const float* g, const float* y, const float* bn_pw, const float* ydw, const float* bn_dw, float* dw, float* partial,
                       int64_t M, int Cin, int Cout, hipStream_t st);
size_t f16t_wgrad_scratch_bytes(int64_t M, int Cin, int Cout);

}  // namespace ttk
