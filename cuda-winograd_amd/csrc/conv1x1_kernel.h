// The 1x1-conv GEMM kernel as a header, so that the library (conv1x1.hip) and the ablation tool
// (tools/ablate_1x1.hip) compile the same source.  ABLATE (0 = product): 1 skip the A LDS-DMA,
// 2 skip the B LDS-DMA, 4 skip the MFMAs, 8 skip the per-stage wait+barrier, 512 skip the stores.
//
// SK = true is the stream-K launch form.  A launch lasts as long as its busiest CU: a CU gives its
// workgroups a fixed throughput (one alone walks 32 k-steps of the 1024->256 layer in 57 us, two
// that share it take 115 us each), so the plain form costs ceil(tiles / CUs) tile-times (measured:
// 384, 448 and 512 workgroups 116-117 us, every further 256 add 57 us) and the reference's 448-tile
// layers pay for 512; with fewer tiles than CUs it leaves CUs idle while the busy ones walk whole K
// loops.  Stream-K cuts the (row tile, k-step) space into equal contiguous ranges instead; a range
// is a run of whole tiles with at most one cut tile at either end.  A segment that is not a
// whole tile stores its raw accumulators as a write-through slab and the workgroup draws one
// ticket on the tile; whoever learns that the tile's other segments are all there adds them in k
// order (bitwise reproducible) and runs the epilogue.
// Nobody waits for anybody.  Same slab / ticket rules as the fused 3x3 kernel (wino_f2_fused_kernel.h).
#pragma once
#include "wino_common.h"

#include <type_traits>

namespace wino {
namespace gemm1x1 {

#ifndef WINO_1X1_DMA0
#define WINO_1X1_DMA0 4   // first step of a stage (of 14) that issues an LDS-DMA piece of the next one;
                          // tools/ablate_1x1: 0 / 2 / 4 / 6 within 1 % on all four reference shapes, 8 up to +9 %
#endif
#ifndef WINO_1X1_SK_PRIO
#define WINO_1X1_SK_PRIO 0   // experiment, measured slower; tools may build with 1
#endif
#ifndef WINO_1X1_PROLOGUE_PRIO
#define WINO_1X1_PROLOGUE_PRIO 1
#endif
constexpr int BM = 112;
constexpr int WINO_INTERNAL_NO_BN = 1 << 16;   // not part of the public flag set
constexpr int RB = BM / 16;  // 7 row blocks

__device__ __forceinline__ void wait_lds1(int n) {
  switch (n) {
    case 0: __builtin_amdgcn_s_waitcnt(0xC07F); break;
    case 1: __builtin_amdgcn_s_waitcnt(0xC17F); break;
    case 2: __builtin_amdgcn_s_waitcnt(0xC27F); break;
    case 3: __builtin_amdgcn_s_waitcnt(0xC37F); break;
    case 4: __builtin_amdgcn_s_waitcnt(0xC47F); break;
    case 5: __builtin_amdgcn_s_waitcnt(0xC57F); break;
    case 6: __builtin_amdgcn_s_waitcnt(0xC67F); break;
    case 7: __builtin_amdgcn_s_waitcnt(0xC77F); break;
    case 8: __builtin_amdgcn_s_waitcnt(0xC87F); break;
    case 9: __builtin_amdgcn_s_waitcnt(0xC97F); break;
    case 10: __builtin_amdgcn_s_waitcnt(0xCA7F); break;
    case 11: __builtin_amdgcn_s_waitcnt(0xCB7F); break;
    case 12: __builtin_amdgcn_s_waitcnt(0xCC7F); break;
    default: __builtin_amdgcn_s_waitcnt(0xCF7F); break;
  }
}

// Geometry of the padded tensors a chained layer reads (WINO_A_PADDED) or writes (WINO_C_PADDED):
// H x W feature maps inside [N][H+2][W+2][.] -- the 3x3 layer's input / output layout.  The
// reference's stage is 14 x 14 in 16 x 16; any other size travels here.
struct PadGeo {
  unsigned hw, w;        // pixels per image, per row
  unsigned Hp, Wp;       // padded extents
  FastDiv d_hw, d_w;
};
__host__ inline PadGeo make_padgeo(int H, int W) {
  PadGeo g;
  g.hw = (unsigned)H * (unsigned)W;
  g.w = (unsigned)W;
  g.Hp = (unsigned)H + 2;
  g.Wp = (unsigned)W + 2;
  g.d_hw = make_fastdiv(g.hw);
  g.d_w = make_fastdiv(g.w);
  return g;
}
// logical pixel row m = n*H*W + y*W + x  ->  row of the padded [N][H+2][W+2][.] tensor
__device__ __forceinline__ long padded_row(long m, const PadGeo& g) {
  const unsigned mu = (unsigned)m;   // M < 2^31 (checked on the host)
  const unsigned n = fastdiv(mu, g.d_hw);
  const unsigned rem = mu - n * g.hw;
  const unsigned y = fastdiv(rem, g.d_w);
  const unsigned x = rem - y * g.w;
  return (long)n * (g.Hp * g.Wp) + (long)((y + 1) * g.Wp + x + 1);
}

// A operand forms of the projection block (proj_block.hip).  A_PLAIN is every launch of conv1x1.hip: the forms
// are template parameters, so that its kernels compile to exactly what they were before the others existed.
//   A_STRIDED  A is an unpadded [N][Hin][Win][Cin] tensor read at stride s: logical row m = n*H*W + y*W + x of
//              the H x W output grid (pg) is input row n*Hin*Win + s*y*Win + s*x (a 1x1 conv with stride s)
//   A_TWO      two A sources along K: k-steps [0, cm/BK) read A (the padded t2 tensor, row length cm), the rest
//              read the strided x (row length cx) -- the block's last 1x1 and its projection shortcut in one
//              set of accumulators; B is the stacked [cm + cx][Kout] matrix
enum { A_PLAIN = 0, A_STRIDED = 1, A_TWO = 2 };
struct ProjGeo {
  const float* X;         // A_TWO: the block input x
  unsigned img, row, s;   // x's pixels per image (Hin*Win), pixels per strided row step (s*Win), the stride
  int cx, cm;             // A_TWO: channels of x, of the first source (the phase boundary is k = cm)
};
// logical pixel row m of the H x W grid -> row of the strided input (same FastDiv work as padded_row)
__device__ __forceinline__ long strided_row(long m, const PadGeo& g, const ProjGeo& x) {
  const unsigned mu = (unsigned)m;   // M < 2^31 (checked on the host)
  const unsigned n = fastdiv(mu, g.d_hw);
  const unsigned rem = mu - n * g.hw;
  const unsigned y = fastdiv(rem, g.d_w);
  const unsigned xx = rem - y * g.w;
  return (long)n * x.img + (long)(y * x.row + xx * x.s);   // y*row + xx*s < Hin*Win < 2^31 (host)
}

template <int BK, int NW>
struct Cfg {
  static constexpr int NT = 64 * NW;                // threads per workgroup
  static constexpr int BN = 16 * NW;                // output columns per workgroup (one 16-col block per wave)
  static constexpr int S = BK / 16;                 // 16-wide k sub-chunks per stage
  static constexpr int T = S * RB;                  // pinned steps per stage (4 MFMAs each)
  static constexpr int UNITS = BK / 4;              // 16-byte units per A row
  static constexpr int A_BYTES = BM * BK * 4;
  static constexpr int B_BYTES = BK * BN * 4;
  static constexpr int STAGE = A_BYTES + B_BYTES;
  static constexpr int LDS_BYTES = 2 * STAGE;
  static constexpr int A_PIECES = A_BYTES / 1024;   // LDS-DMA wave-instructions per stage
  static constexpr int B_PIECES = B_BYTES / 1024;
  static constexpr int A_PER_WAVE = (A_PIECES + NW - 1) / NW;
  static constexpr int B_PER_WAVE = B_PIECES / NW;
  static constexpr int ROWS_PER_PIECE = 1024 / (BK * 4);
  static constexpr int B_UNITS = BN / 4;            // 16-byte units per B row
  static constexpr int B_ROWS_PER_PIECE = 1024 / (BN * 4);
  static __device__ __forceinline__ int fa(int row) { return BK == 64 ? (row & 15) : ((row >> 1) & 7); }
  // LDS requests at the top of step q: the A fragment of step q+2, then (on row block 2) the
  // four B values of the next sub-chunk
  static constexpr int nA(int q) { return q + 2 < T ? 1 : 0; }
  static constexpr int nB(int q) { return (q % RB == 2 && q / RB + 1 < S) ? 4 : 0; }
  // requests younger than the A fragment step t consumes
  static constexpr int wait_count(int t) {
    int after = 0;
    if (t < 2) {
      after = 1 - t;                                  // pre-loop block: B(0)x4, A(0), A(1)
      for (int q = 0; q <= t; q++) after += nA(q) + nB(q);
    } else {
      after = nB(t - 2);
      for (int q = t - 1; q <= t; q++) after += nA(q) + nB(q);
    }
    return after;
  }
};

// scratch of the stream-K form (library-owned, per stream): 2 slab slots of NW*RB KiB per
// workgroup, one ticket counter per tile (zero between launches)
struct SkArgs {
  float* slabs;
  unsigned* tickets;
  unsigned long long* dbg;   // timeline build only (ABLATE & 32768, tools/ablate_1x1 t): 8 uint64 per workgroup
  unsigned* err;             // host-visible word, set when a ticket is drawn on a counter that was not zero at launch
};

// In-kernel clock of the most recent launch (see wino_clk_slot_3x3 in wino_f2_fused_kernel.h): workgroup 0
// stores {s_memtime, s_memrealtime} at its entry and at its exit; wino_diag_last_clock(1, ...) copies them out.
__device__ unsigned long long wino_clk_slot_1x1[4];

// Resident waves per SIMD the LDS footprint allows -- two 8-wave workgroups (60 KB each) or three
// 4-wave ones (44 KB) per CU -- stated to the register allocator, which otherwise takes the
// freedom of 256 VGPRs and halves the residency (tests/test_build_budget.py).
// RES = the launch adds a residual (WINO_ADD_RESIDUAL): a compile-time property, because the two epilogues in one
// kernel cost the one without residual 2-5 % (256->1024 99.6 -> 101.3 us, 64->256 14.1 -> 14.9) through nothing but
// their presence -- register allocation and code layout of the rest.
template <int BK, int NW, int ABLATE = 0, bool SK = false, bool RES = false>
__global__ void __launch_bounds__(64 * NW, NW == 8 ? 4 : 3)
conv1x1_bn_kernel(const float* __restrict__ A, const float* __restrict__ B,
                  const float* __restrict__ bnBias, const float* __restrict__ bnScale,
                  const float* __restrict__ R, float* __restrict__ Cout, long M, int Cin, int Kout,
                  int flags, int nMB, long batchA, long batchB, long batchC, SkArgs sk, PadGeo pg) {
  constexpr int AF = A_PLAIN;
  const ProjGeo xg{};
#include "conv1x1_kernel_body.inc"
}

// The projection block's forms (proj_block.hip): BK = 32, no residual, no batch.  A_STRIDED: A = x, Cin = x's
// channels; A_TWO: A = t2 (padded, flags WINO_A_PADDED), Cin = cm + cx, B = the stacked tail matrix.
template <int NW, bool SK, int AF>
__global__ void __launch_bounds__(64 * NW, NW == 8 ? 4 : 3)
conv1x1_proj_kernel(const float* __restrict__ A, const float* __restrict__ B,
                    const float* __restrict__ bnBias, const float* __restrict__ bnScale,
                    float* __restrict__ Cout, long M, int Cin, int Kout, int flags, int nMB, SkArgs sk, PadGeo pg,
                    ProjGeo xg) {
  static_assert(AF == A_STRIDED || AF == A_TWO, "operand form");
  constexpr int BK = 32, ABLATE = 0;
  constexpr bool RES = false;
  const float* const R = nullptr;
  constexpr long batchA = 0, batchB = 0, batchC = 0;
#include "conv1x1_kernel_body.inc"
}


}  // namespace gemm1x1
}  // namespace wino
