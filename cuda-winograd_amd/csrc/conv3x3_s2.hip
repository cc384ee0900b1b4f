// Stride-2, pad-1 3x3 convolution + folded BN (+ReLU), gfx950: the 3x3 of the ResNet v1.5 downsampling block
// (the placement torchvision uses: the stride sits on the 3x3, not on the first 1x1).  F(2x2,3x3) has no stride-2
// form; over the padded input a stride-2 3x3 is the GEMM
//   out[m][k] = act( bnScale[k] * sum_{tap, c} in[window(m) + tap][c] * w_taps[tap][c][k] + bnBias[k] )
// of M = N*H*W output pixels, K = 9 C and Kout = K, with the window of output pixel (n, y, x) at padded input pixel
// (n, 2y, 2x) and tap (dy, dx) a constant pixel offset dy*(Win+2) + dx from it.  The 1x1 kernel templates run it in
// operand form A_TAPS (conv1x1_kernel.h): the same LDS-DMA pipeline and MFMA loop with one scalar A offset per k-step,
// the same latency / tiled / stream-K forms, the same planner (plan_1x1 on the GEMM's shape, its latency-or-tiled
// choice re-priced for the tap form: plan_s2) and launcher (launch_1x1, conv1x1_launch.h).  This file instantiates that form and no other.
// check_s2 and plan_s2 are shared with basic_block_s2.hip, check_s2 also with bottleneck.hip (conv3x3_s2.h).
#include "conv3x3_s2.h"

namespace wino {

using namespace gemm1x1;

// The layer's geometry, checked once.  Every 32-bit quantity of the tap addressing is bounded here: the pixel row
// index (M < 2^31, one padded input image < 2^31 pixels), a 112-row tile's buffer-descriptor window over the padded
// input, B's descriptor and the ring pass's 16-byte units.
int check_s2(int N, int Hin, int Win, int C, int K, S2Geom* g) {
  if (N < 1 || Hin < 1 || Win < 1) { set_error("stride-2 3x3: bad N=%d Hin=%d Win=%d", N, Hin, Win); return WINO_E_SHAPE; }
  if (C <= 0 || K <= 0 || C % 32 || K % 64) {
    set_error("stride-2 3x3: unsupported channels C=%d K=%d (need C %% 32 == 0, K %% 64 == 0)", C, K);
    return WINO_E_SHAPE;
  }
  const int H = (Hin - 1) / 2 + 1, W = (Win - 1) / 2 + 1;
  if (H > 4094 || W > 4094) { set_error("stride-2 3x3: unsupported feature map %dx%d", H, W); return WINO_E_SHAPE; }
  const unsigned long long M = (unsigned long long)N * H * W, Wp = (unsigned long long)Win + 2;
  if (M >= (1ull << 31)) { set_error("stride-2 3x3: N*H*W = %llu pixel rows (need < 2^31)", M); return WINO_E_SHAPE; }
  if (((unsigned long long)Hin + 2) * Wp >= (1ull << 31)) { set_error("stride-2 3x3: input image too large"); return WINO_E_SHAPE; }
  // a tile's window: consecutive pixel rows are at most 4 (Win+2) padded pixels apart (the step to the next image;
  // 2 (Win+2) inside one), and the last row's taps reach 2 (Win+2) + 2 pixels past its window start
  const unsigned long long a_win = ((unsigned long long)(BM - 1) * 4 * Wp + 2 * Wp + 3) * C * sizeof(float);
  const unsigned long long b = 9ull * C * K * sizeof(float);
  const unsigned long long ring = (unsigned long long)N * (2ull * (W + 2) + 2ull * H) * (K / 4);
  if (a_win >= FOUR_GIB || b >= FOUR_GIB || ring >= FOUR_GIB) {
    set_error("stride-2 3x3: a tile's window, the filter matrix or the ring pass reaches 2^32 (Win=%d C=%d K=%d)", Win, C, K);
    return WINO_E_SHAPE;
  }
  if ((M + BM - 1) / BM > (1ull << 24)) { set_error("stride-2 3x3: M too large"); return WINO_E_SHAPE; }
  *g = S2Geom{N, Hin, Win, C, K, H, W, (long)M};
  return WINO_OK;
}
// The plan: plan_1x1 of the GEMM (N*H*W, 9C, K), with the choice between the latency and the tiled form re-priced for
// the tap form.  Measured at the conv3/4/5 shapes for N = 1..128 (tools/conv3x3_s2_bench.py policy,
// profiles/proj_block_v15/policy.json), both 1x1 launch models run short here:
//   * the stream-K model leaves out a split tile's serial gather: (G / tiles - 1) segments of 0.9 us (8 waves) /
//     0.47 us (4 waves) on the finisher's path (conv5 N = 8, 16 segments a tile: modelled 26.5 us, 40.0 with the
//     gather, measured 40.6);
//   * the latency model reads 1.2-1.36x short of the forms it picks from N = 8 on (K = 9C: 1152-4608 channels).
// Routed by the plain models, conv5 at N = 8 took stream-K at 40.2 us where the latency form takes 28.4-33.4.  The
// decision keeps the 1x1 planner's margins (0.93, several rounds deep 0.8) on the corrected times; the plain 1x1
// layers' plans do not change.  Forced forms (WINO_1X1_ALGO, WINO_1X1_SK, WINO_1X1_SK_GRID) are left as planned.
Plan1x1 plan_s2(const S2Geom& g, int cus, const Knobs& kn) {
  Plan1x1 p = plan_1x1(g.M, 9 * g.C, g.K, 1, cus, kn);
  const bool forced = kn.algo_1x1 != 0 || kn.sk_1x1 != -1 || kn.sk_1x1_grid != 0;
  if (forced || p.small.wgs <= 0) return p;   // (wgs == 0: no legal latency form)
  double t_tiled = p.small.t_big_us;
  const double seg = p.sk ? (double)p.sk / (double)(p.nMB * p.nblk) : 1.0;
  if (seg > 1.0) t_tiled += (seg - 1.0) * (p.four ? 0.47 : 0.9);
  p.small.use = 1.25 * p.small.t_us < (p.small.wgs > cus ? 0.8 : 0.93) * t_tiled;
  return p;
}

}  // namespace wino

using namespace wino;

extern "C" {

int wino_conv3x3_s2_bn_relu_hw(const float* in, const float* w_taps, const float* bnBias, const float* bnScale,
                               float* out, int N, int Hin, int Win, int C, int K, int relu, wino_stream_t s) {
  if (int rc = check_nonnull(in, w_taps, bnBias, bnScale, out)) return rc;
  if (int rc = check_aligned16(in, w_taps, out)) return rc;
  S2Geom g;
  if (int rc = check_s2(N, Hin, Win, C, K, &g)) return rc;
  int dev = 0, cus = 0;
  if (int rc = current_device(&dev, &cus)) return rc;
  const ProjGeo xg{nullptr, (unsigned)(Hin + 2) * (unsigned)(Win + 2), 2u * (unsigned)(Win + 2), 2u, C, Win + 2};
  const int flags = (relu ? WINO_RELU : 0) | WINO_C_PADDED;
  return launch_1x1<A_TAPS>(plan_s2(g, cus, knobs()), dev,
                            {in, w_taps, bnBias, bnScale, nullptr, out, g.M, 9 * C, K, flags, make_padgeo(g.H, g.W), xg},
                            (hipStream_t)s);
}

int wino_conv3x3_s2_prepare_hw(int N, int Hin, int Win, int C, int K, wino_stream_t s) {
  S2Geom g;
  if (int rc = check_s2(N, Hin, Win, C, K, &g)) return rc;
  int dev = 0, cus = 0;
  if (int rc = current_device(&dev, &cus)) return rc;
  const Plan1x1 p = plan_s2(g, cus, knobs());
  if (!p.sk) return WINO_OK;
  SkBufs bufs;
  return tiled_scratch(dev, (hipStream_t)s, p, &bufs);
}

int wino_conv3x3_s2_plan(int N, int Hin, int Win, int C, int K, int cus, int* form) {
  if (!form || cus < 1) { set_error("bad argument"); return WINO_E_ARG; }
  S2Geom g;
  if (int rc = check_s2(N, Hin, Win, C, K, &g)) return rc;
  const Plan1x1 p = plan_s2(g, cus, knobs());
  *form = p.small.use ? WINO_1X1_FORM_LATENCY : p.sk ? WINO_1X1_FORM_STREAM_K : WINO_1X1_FORM_TILED;
  return WINO_OK;
}

}  // extern "C"
