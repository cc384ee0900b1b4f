// The residual forms of the F(2x2,3x3) layer and the ResNet basic block built on them:
//
//   wino_conv3x3_bn_add_relu_hw   out = act(bnScale*conv3x3(in, U) + bnBias + residual)       (one launch)
//   wino_basic_block_hw           out = relu(bn2(conv3x3(relu(bn1(conv3x3(x, U1))), U2)) + x)  (two launches)
//
// The kernels are the plain layer's with RES = true (wino_f2_fused_kernel.h, wino_f2_small_kernel.h): the residual is
// padded like out, [N][H+2][W+2][K], and each output's residual is read by the lane that stores that output, at the
// same byte offset, just before the store -- so out may be the residual itself (in place).  A residual launch takes
// exactly the plan of the plain layer of the same shape (wino_f2_launch.h); this file instantiates the RES kernels only.
#include "wino_f2_launch.h"

using namespace wino;

namespace {

// the residual layer's checks, all before any device query: pointers, shape, overlap (out == residual is allowed)
int check_res(const float* in, const float* U, const float* bnBias, const float* bnScale, const float* residual,
              const float* out, int N, int H, int W, int C, int K) {
  if (int rc = check_nonnull(in, U, bnBias, bnScale, residual, out)) return rc;
  if (int rc = check_aligned16(in, U, residual, out)) return rc;
  if (int rc = check_conv3x3_dims(H, W, C, K)) return rc;
  if (N < 1) { set_error("bad batch N=%d", N); return WINO_E_SHAPE; }
  const size_t in_b = padded_bytes(N, H, W, C), out_b = padded_bytes(N, H, W, K);
  if (overlaps(in, in_b, out, out_b) || overlaps(in, in_b, residual, out_b)) {
    set_error("the input overlaps the residual or the output");
    return WINO_E_ARG;
  }
  if (residual != out && overlaps(residual, out_b, out, out_b)) {
    set_error("the residual and the output overlap without being the same tensor");
    return WINO_E_ARG;
  }
  return WINO_OK;
}

}  // namespace

extern "C" {

int wino_conv3x3_bn_add_relu_hw(const float* in, const float* U, const float* bnBias, const float* bnScale,
                                const float* residual, float* out, int N, int H, int W, int C, int K, int relu,
                                wino_stream_t s) {
  if (int rc = check_res(in, U, bnBias, bnScale, residual, out, N, H, W, C, K)) return rc;
  return conv3x3_launch<true>(in, U, bnBias, bnScale, residual, out, N, H, W, C, K, relu, (hipStream_t)s);
}

size_t wino_basic_block_workspace_bytes_hw(int N, int H, int W, int C) {
  if (N < 1 || H < 1 || W < 1 || C < 1) return 0;
  return padded_bytes(N, H, W, C);
}

int wino_basic_block_prepare_hw(int N, int H, int W, int C, wino_stream_t s) {
  // both launches have the shape (and so the plan) of the plain C -> C layer: its scratch serves them both
  return wino_conv3x3_prepare_hw(N, H, W, C, C, s);
}

int wino_basic_block_hw(const float* x, const float* U1, const float* bn1Bias, const float* bn1Scale,
                        const float* U2, const float* bn2Bias, const float* bn2Scale, float* out,
                        int N, int H, int W, int C, void* workspace, size_t workspace_bytes, wino_stream_t s) {
  if (int rc = check_nonnull(x, U1, bn1Bias, bn1Scale, U2, bn2Bias, bn2Scale, out, workspace)) return rc;
  if (int rc = check_aligned16(x, U1, U2, out, workspace)) return rc;
  if (int rc = check_conv3x3_dims(H, W, C, C)) return rc;
  if (N < 1) { set_error("bad batch N=%d", N); return WINO_E_SHAPE; }
  const size_t need = wino_basic_block_workspace_bytes_hw(N, H, W, C);
  if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
  if (overlaps(workspace, need, x, need) || overlaps(workspace, need, out, need)) {
    set_error("the workspace overlaps x or out");
    return WINO_E_ARG;
  }
  if (x != out && overlaps(x, need, out, need)) {
    set_error("x and out overlap without being the same tensor");
    return WINO_E_ARG;
  }
  float* t1 = (float*)workspace;
  // (the first conv through the plain entry point: this file compiles the RES kernels only)
  if (int rc = wino_conv3x3_bn_relu_hw(x, U1, bn1Bias, bn1Scale, t1, N, H, W, C, C, 1, s)) return rc;
  return conv3x3_launch<true>(t1, U2, bn2Bias, bn2Scale, x, out, N, H, W, C, C, 1, (hipStream_t)s);
}

}  // extern "C"
