// Latency form of the 1x1-conv GEMM + folded BN (+ReLU) for FEW pixel rows -- the reference's own
// protocol is one image, M = 196 rows (kernel_512_one_128 & co at N = 1: Kernel128_one.cu:98,316,
// Kernel256_one.cu:100,318).
//
// At M = 196 the LDS-staged kernel (conv1x1_kernel.h: 112-row x 64/128-column tiles) has 4-8 tiles for
// 256 CUs; its split-K form spreads them over 32-64 workgroups and pays a serial gather of up to eight
// 28-56 KB slabs by whoever arrives last (1024->256: 19.4 us for 0.1 GFLOP).  Here the output is cut into
// BLOCKS of (16 RT) x (16 CT) -- RT x CT MFMA tiles held by ONE wave (RT = CT = 1 at M = 196: 13 x Kout/16
// blocks) -- a workgroup is 4 waves = 4 / KS blocks side by side whose K loop is split over KS waves (KS = 4:
// 1024->256 is 208 workgroups, every wave contracts 256 channels = 64 MFMAs); the KS partial blocks meet in
// LDS.  No cross-workgroup reduction, no scratch, no tickets.  Operands come straight from global memory in
// MFMA fragment layout:
//   pixel fragment  : lane (m = lane & 15, h = lane >> 4) loads A[m][16 s + 4 h .. + 3]   (one 16-byte load per
//                     row tile and 16-channel super-chunk s; MFMA k-step jj contracts channel 16 s + 4 h + jj)
//   filter fragment : lane (n = lane & 15, h) loads B[16 s + 4 h + jj][n0 + n], jj = 0..3  (four 4-byte loads per
//                     column tile: B stays in the reference's [Cin][Kout] layout, Kernel128_one.cu:40-42)
// As in the big kernel the filter fragment is the MFMA's A operand and the pixel fragment its B operand, so a
// lane ends up with four CONSECUTIVE out-channels of one pixel: BN with four scales, one 16-byte store per tile.
// The form is bound by the bytes every wave pulls through its CU's vector memory path: a 16 x 16 block costs
// 128 Cin bytes, a 32 x 32 block (RT = CT = 2: each fragment feeds two MFMA tiles) 256 Cin for four times the
// output -- half the bytes per FLOP, which is what carries the form from a handful of images to a dozen
// (conv1x1.hip: small1_plan).  The chained forms of the bottleneck block travel too (flags as in the tiled kernel:
// WINO_A_PADDED / WINO_C_PADDED = the operand is the padded [N][H+2][W+2][.] tensor of the 3x3 layer, the output's zero
// ring written by a flat pass over the grid; WINO_ADD_RESIDUAL = + residual before the ReLU), wave-uniform branches.
// CT = 4 is the WIDE form: a wave's 64 columns are cut into four tiles of STRIDED columns -- tile c = columns
// n0 + 4 j + c, j = 0..15 -- so that lane (j, h) reads B[k][n0 + 4 j .. + 3] with ONE 16-byte load per k-step and uses
// component c as tile c's operand: a quarter of the filter load instructions, each touching 8 whole cache lines (four
// k-rows x 256 B) where the four-byte loads of the other forms touch 4 half lines per 256 B.  After the MFMAs register
// r of tile c is column n0 + 16 h + 4 r + c: the four tiles' components r form 16-byte stores again.
#pragma once
#include "conv1x1_kernel.h"

namespace wino {
namespace gemm1x1 {

template <int KS, int RT = 1, int CT = 1>
__global__ void __launch_bounds__(256)
conv1x1_small_kernel(const float* __restrict__ A, const float* __restrict__ B,
                     const float* __restrict__ bnBias, const float* __restrict__ bnScale,
                     const float* __restrict__ Res, float* __restrict__ Cout, long M, int Cin, int Kout, int flags,
                     const PadGeo pg) {
  constexpr int AF = A_PLAIN;
  const ProjGeo xg{};
#include "conv1x1_small_kernel_body.inc"
}

// The projection block's forms (proj_block.hip, operand forms as in conv1x1_kernel.h).  A_STRIDED: A = x, Cin = x's
// channels.  A_TWO: A = t2 (padded, flags WINO_A_PADDED), Cin = cm + cx, B = the stacked tail matrix; each wave
// contracts its share of both sources (cm / KS channels of t2, then cx / KS of x), so the K split stays in k order.
template <int KS, int RT, int CT, int AF>
__global__ void __launch_bounds__(256)
conv1x1_small_proj_kernel(const float* __restrict__ A, const float* __restrict__ B,
                          const float* __restrict__ bnBias, const float* __restrict__ bnScale, float* __restrict__ Cout,
                          long M, int Cin, int Kout, int flags, const PadGeo pg, const ProjGeo xg) {
  static_assert(AF == A_STRIDED || AF == A_TWO, "operand form");
  const float* const Res = nullptr;
#include "conv1x1_small_kernel_body.inc"
}

}  // namespace gemm1x1
}  // namespace wino
