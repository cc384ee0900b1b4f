// The Feature Pyramid Network's level, and the 1x1 kernels of its top-down sum:
//
//   wino_fpn_level_hw   inner = conv1x1(c, wl) + bias [+ nearest_upsample(top)]; P = conv3x3(inner, U) + bias   (two launches)
//
// The top-down sum is the 1x1 GEMM's residual epilogue reading the coarser map at (y >> 1, x >> 1)
// (WINO_RESIDUAL_UP2; RES_UP2 in conv1x1_kernel.h): the lateral launch costs a quarter of a same-size residual's
// bytes more than the plain lateral, and the upsampled tensor never exists.  This file instantiates the 1x1 kernels of
// that epilogue -- tiled 4- and 8-wave, plain and stream-K, and the latency forms -- and no others; the launch plan is
// the plain layer's (conv1x1.hip), whose entry point wino_conv1x1_bn_ex_hw hands such launches to launch_1x1_up2.
#include "conv1x1_launch.h"

namespace wino {
int launch_1x1_up2(const Plan1x1& p, int dev, const Operands1x1& o, hipStream_t s) {
  return launch_1x1<gemm1x1::A_PLAIN, true>(p, dev, o, s);
}
}  // namespace wino

using namespace wino;

namespace {

// both layers' shape checks: the lateral Cin -> Cf writing the padded inner, the Winograd 3x3 Cf -> Cf
int check_level_shape(int N, int H, int W, int Cin, int Cf) {
  if (int rc = check_1x1_hw(N, H, W, Cin, Cf)) return rc;
  return check_conv3x3_dims(H, W, Cf, Cf);
}

}  // namespace

extern "C" {

int wino_fpn_level_hw(const float* c, const float* wl, const float* lBias, const float* lScale, const float* top,
                      float* inner, const float* U, const float* oBias, const float* oScale, float* P, int N, int H,
                      int W, int Cin, int Cf, int c_padded, wino_stream_t s) {
  if (int rc = check_nonnull(c, wl, lBias, lScale, inner, U, oBias, oScale, P)) return rc;
  if (int rc = check_aligned16(c, wl, top, inner, U, P)) return rc;
  if (int rc = check_level_shape(N, H, W, Cin, Cf)) return rc;
  const size_t c_b = c_padded ? padded_bytes(N, H, W, Cin) : (size_t)N * H * W * Cin * sizeof(float);
  const size_t lvl_b = padded_bytes(N, H, W, Cf), top_b = top ? padded_bytes(N, (H + 1) / 2, (W + 1) / 2, Cf) : 0;
  if (any_overlap({{c, c_b}, {inner, lvl_b}, {P, lvl_b}}) ||
      (top && (overlaps(top, top_b, inner, lvl_b) || overlaps(top, top_b, P, lvl_b)))) {
    set_error("c, top, inner and P must not overlap");
    return WINO_E_ARG;
  }
  const int flags = WINO_C_PADDED | (c_padded ? WINO_A_PADDED : 0) | (top ? WINO_ADD_RESIDUAL | WINO_RESIDUAL_UP2 : 0);
  if (int rc = wino_conv1x1_bn_ex_hw(c, wl, lBias, lScale, top, inner, N, H, W, Cin, Cf, flags, s)) return rc;
  return wino_conv3x3_bn_relu_hw(inner, U, oBias, oScale, P, N, H, W, Cf, Cf, 0, s);
}

int wino_fpn_level_prepare_hw(int N, int H, int W, int Cin, int Cf, wino_stream_t s) {
  if (int rc = check_level_shape(N, H, W, Cin, Cf)) return rc;
  // (the upsampled residual does not alter the GEMM: the lateral's plan, and so its scratch, is the plain layer's)
  if (int rc = wino_conv1x1_prepare((long)N * H * W, Cin, Cf, s)) return rc;
  return wino_conv3x3_prepare_hw(N, H, W, Cf, Cf, s);
}

}  // extern "C"
