// The pooled form of the F(2x2,3x3) layer (a VGG convolution that is followed by MaxPool2d(2, 2)):
//
//   wino_conv3x3_bn_relu_pool_hw   out = maxpool2x2_s2(act(bnScale*conv3x3(in, U) + bnBias))       (one launch)
//
// The kernels are the plain layer's with EPI = EPI_POOL (wino_f2_fused_kernel.h, wino_f2_small_kernel.h): an F(2x2) tile
// is one pooling window, its four outputs sit in one lane's registers in the finalize, and the max over them is taken
// there -- behind the stream-K gather, BN and the ReLU, in front of the LDS transpose and the stores.  out is
// [N][H/2+2][W/2+2][K] with its zero ring.  A pooled launch takes exactly the plan of the plain layer of the same
// shape (wino_f2_launch.h); this file instantiates the POOL kernels only.
#include "wino_f2_launch.h"

using namespace wino;

extern "C" {

int wino_conv3x3_bn_relu_pool_hw(const float* in, const float* U, const float* bnBias, const float* bnScale,
                                 float* out, int N, int H, int W, int C, int K, int relu, wino_stream_t s) {
  if (int rc = check_nonnull(in, U, bnBias, bnScale, out)) return rc;
  if (int rc = check_aligned16(in, U, out)) return rc;
  if (int rc = check_conv3x3_dims(H, W, C, K)) return rc;
  if (H < 2 || W < 2) {
    set_error("pooled 3x3: feature map %dx%d has no 2x2 window (need H, W >= 2)", H, W);
    return WINO_E_SHAPE;
  }
  if (N < 1) { set_error("bad batch N=%d", N); return WINO_E_SHAPE; }
  if (overlaps(in, padded_bytes(N, H, W, C), out, padded_bytes(N, H / 2, W / 2, K))) {
    set_error("the input overlaps the output");
    return WINO_E_ARG;
  }
  return conv3x3_launch<EPI_POOL>(in, U, bnBias, bnScale, nullptr, out, N, H, W, C, K, relu, (hipStream_t)s);
}

}  // extern "C"
