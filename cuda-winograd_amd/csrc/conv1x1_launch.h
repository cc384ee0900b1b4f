// The 1x1 kernels' launch plan and launcher, shared by the translation units that launch them: conv1x1.hip (the plain
// operand form, A_PLAIN), proj_block.hip (the projection block's A_STRIDED / A_TWO forms), conv3x3_s2.hip (the
// stride-2 3x3's A_TAPS form), basic_block_s2.hip (A_TAPS_PROJ, the stride-2 3x3 with its 1x1 shortcut), fpn.hip
// (A_PLAIN with the upsampled residual), conv3x3_dilated.hip (A_DIL, tiled forms only: launch_tiled_1x1) and aspp.hip
// (A_CAT, tiled forms only); the forms: conv1x1_kernel.h.
// A template is instantiated where it is used, so each file compiles the kernels of its own forms and no others.
#pragma once
#include "conv1x1_kernel.h"
#include "conv1x1_small_kernel.h"

namespace wino {

// The latency form's choice (conv1x1_small_kernel.h): use it or not, its K split and MFMA tiles per wave.
struct Small1Plan {
  bool use;
  int ks, rt, ct;
  long long wgs;
  double t_us, t_big_us;   // the two launch models' times
};
// The plan of one launch, read by every consumer -- see plan_1x1 in conv1x1.hip.
struct Plan1x1 {
  bool four;            // 4-wave workgroups (64 columns), else 8 (128)
  int nblk, nk;         // column blocks, k-steps
  long long nMB;        // row tiles
  int sk;               // stream-K / split-K grid, 0: the plain form
  int grid;             // the tiled launch's grid (per batch)
  Small1Plan small;
};
Plan1x1 plan_1x1(long M, int Cin, int Kout, int batch, int cus, const Knobs& kn);
// the tiled kernel's stream-K scratch of stream `s` for this plan (sk_scratch)
int tiled_scratch(int dev, hipStream_t s, const Plan1x1& p, SkBufs* bufs);

// One launch's operands.  R: the residual (A_PLAIN, WINO_ADD_RESIDUAL) or the shortcut's output (A_TAPS_PROJ); xg: the strided / second source (A_STRIDED,
// A_TWO) or the padded input's tap geometry (A_TAPS); batch and the per-batch strides: the batched plain GEMM (gemm_batched; its plans have no stream-K form).
// A_CAT: batchA is the spacing of the sources in floats (batch stays 1), bnBias the per-image bias [N][Kout].
struct Operands1x1 {
  const float *A, *B, *bnBias, *bnScale, *R;
  float* C;
  long M;
  int Cin, Kout, flags;
  gemm1x1::PadGeo pg;
  gemm1x1::ProjGeo xg = {};
  int batch = 1;
  long batchA = 0, batchB = 0, batchC = 0;
};

// the latency kernel's instantiations by [KS / 2][RT - 1][CT / 2]
template <int AF, bool UP2 = false>
constexpr decltype(&gemm1x1::conv1x1_small_kernel<1, 1, 1, UP2, AF>) SMALL_1X1_KERNELS[3][2][3] = {
    {{gemm1x1::conv1x1_small_kernel<1, 1, 1, UP2, AF>, gemm1x1::conv1x1_small_kernel<1, 1, 2, UP2, AF>,
      gemm1x1::conv1x1_small_kernel<1, 1, 4, UP2, AF>},
     {gemm1x1::conv1x1_small_kernel<1, 2, 1, UP2, AF>, gemm1x1::conv1x1_small_kernel<1, 2, 2, UP2, AF>,
      gemm1x1::conv1x1_small_kernel<1, 2, 4, UP2, AF>}},
    {{gemm1x1::conv1x1_small_kernel<2, 1, 1, UP2, AF>, gemm1x1::conv1x1_small_kernel<2, 1, 2, UP2, AF>,
      gemm1x1::conv1x1_small_kernel<2, 1, 4, UP2, AF>},
     {gemm1x1::conv1x1_small_kernel<2, 2, 1, UP2, AF>, gemm1x1::conv1x1_small_kernel<2, 2, 2, UP2, AF>,
      gemm1x1::conv1x1_small_kernel<2, 2, 4, UP2, AF>}},
    {{gemm1x1::conv1x1_small_kernel<4, 1, 1, UP2, AF>, gemm1x1::conv1x1_small_kernel<4, 1, 2, UP2, AF>,
      gemm1x1::conv1x1_small_kernel<4, 1, 4, UP2, AF>},
     {gemm1x1::conv1x1_small_kernel<4, 2, 1, UP2, AF>, gemm1x1::conv1x1_small_kernel<4, 2, 2, UP2, AF>,
      gemm1x1::conv1x1_small_kernel<4, 2, 4, UP2, AF>}}};

template <int NW, bool SK, int AF, int RES>
int launch_tiled_1x1_kernel(dim3 grid, int nMB, const Operands1x1& o, gemm1x1::SkArgs sk, hipStream_t s) {
  using G = gemm1x1::Cfg<32, NW>;
  hipLaunchKernelGGL((gemm1x1::conv1x1_bn_kernel<32, NW, 0, SK, RES, AF>), grid, dim3(G::NT), G::LDS_BYTES, s, o.A,
                     o.B, o.bnBias, o.bnScale, o.R, o.C, o.M, o.Cin, o.Kout, o.flags, nMB, o.batchA, o.batchB, o.batchC, sk,
                     o.pg, o.xg);
  return launch_status(SK ? "conv1x1_bn_kernel (stream-K)" : "conv1x1_bn_kernel");
}

// BK = 32 keeps a workgroup at 60 KB of LDS, so two workgroups share a CU (4 waves per SIMD)
// and one's prologue / barrier bubbles / store tail hide under the other's MFMAs; measured
// 3-14 % faster than BK = 64 (120 KB, one workgroup per CU) on the four reference shapes.
template <int NW, int AF, int RES>
int launch_tiled_1x1(const Plan1x1& p, int dev, const Operands1x1& o, hipStream_t s) {
  constexpr int LDS_BYTES = gemm1x1::Cfg<32, NW>::LDS_BYTES;
  if (int rc = lds_cap_once<gemm1x1::conv1x1_bn_kernel<32, NW, 0, false, RES, AF>,
                            gemm1x1::conv1x1_bn_kernel<32, NW, 0, true, RES, AF>>(dev, LDS_BYTES))
    return rc;
  // A_TAPS_PROJ: the shortcut's whole tiles (a plain tiled grid) go behind the planned grid, whose size batchA carries
  unsigned extra = 0;
  Operands1x1 op = o;
  if constexpr (AF == gemm1x1::A_TAPS_PROJ) {
    extra = (unsigned)(8ll * p.nblk * ((p.nMB + 7) / 8));
    op.batchA = p.sk ? p.sk : p.grid;
  }
  if (!p.sk)
    return launch_tiled_1x1_kernel<NW, false, AF, RES>(dim3(p.grid + extra, o.batch), (int)p.nMB, op,
                                                       gemm1x1::SkArgs{nullptr, nullptr, nullptr, nullptr}, s);
  SkBufs bufs;
  if (int rc = tiled_scratch(dev, s, p, &bufs)) return rc;
  const int rc = launch_tiled_1x1_kernel<NW, true, AF, RES>(dim3(p.sk + extra), (int)p.nMB, op,
                                                            gemm1x1::SkArgs{bufs.slabs, bufs.tickets, nullptr, bufs.err}, s);
  if (rc) sk_mark_failed(dev, s);   // the launch held the stream's scratch
  return rc;
}

// One launch of the 1x1 GEMM in operand form AF as planned: the latency form, or the tiled kernel with 4 or 8 waves,
// plain or stream-K.  UP2: the launch adds the upsampled residual (WINO_RESIDUAL_UP2: o.R the padded coarser map, o.xg
// from make_up2geo) -- the same plan, the kernels of that epilogue and no others.
template <int AF, bool UP2 = false>
int launch_1x1(const Plan1x1& p, int dev, const Operands1x1& o, hipStream_t s) {
  if (p.small.use) {
    const Small1Plan& pl = p.small;
    const auto kernel = SMALL_1X1_KERNELS<AF, UP2>[pl.ks >> 1][pl.rt - 1][pl.ct >> 1];
    // x = column group, y = row block: see the kernel.  A_TAPS_PROJ: the shortcut's row blocks behind the 3x3's
    const long long rows = (o.M + 16 * pl.rt - 1) / (16 * pl.rt) * (AF == gemm1x1::A_TAPS_PROJ ? 2 : 1);
    if (rows > 65535) { set_error("latency form: %lld row blocks (gridDim.y)", rows); return WINO_E_SHAPE; }
    const dim3 grid((unsigned)(o.Kout / ((4 / pl.ks) * pl.ct * 16)), (unsigned)rows);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, o.A, o.B, o.bnBias, o.bnScale, o.R, o.C, o.M, o.Cin, o.Kout,
                       o.flags, o.pg, o.xg);
    return launch_status("conv1x1_small_kernel");
  }
  if constexpr (UP2) {
    return (p.four ? launch_tiled_1x1<4, AF, gemm1x1::RES_UP2> : launch_tiled_1x1<8, AF, gemm1x1::RES_UP2>)(p, dev, o, s);
  } else {
    auto* launch = p.four ? launch_tiled_1x1<4, AF, gemm1x1::RES_NONE> : launch_tiled_1x1<8, AF, gemm1x1::RES_NONE>;
    if constexpr (AF == gemm1x1::A_PLAIN)   // the residual epilogue is a compile-time property (conv1x1_kernel.h)
      if (o.flags & WINO_ADD_RESIDUAL)
        launch = p.four ? launch_tiled_1x1<4, AF, gemm1x1::RES_SAME> : launch_tiled_1x1<8, AF, gemm1x1::RES_SAME>;
    return launch(p, dev, o, s);
  }
}
// The plain operand form with the upsampled residual, defined in fpn.hip: that file instantiates the WINO_RESIDUAL_UP2
// kernels, so that conv1x1.hip keeps exactly the kernels it had.
int launch_1x1_up2(const Plan1x1& p, int dev, const Operands1x1& o, hipStream_t s);
// The shape limits of one 1x1 layer on an H x W feature map with padded operands (conv1x1.hip), for the blocks that
// check every layer before their first launch.
int check_1x1_hw(int N, int H, int W, int Cin, int Kout);

}  // namespace wino
