// The two ResNeXt bottleneck blocks: the identity and the projection bottleneck with the grouped 3x3
// (conv3x3_grouped.hip) as their middle layer.  Both are host code over existing launches, every argument, shape and
// overlap checked before the first of them.
//
// Identity block (wino_residual_block_hw with the grouped layer in the middle), x and out [N][H][W][C4]:
//   t1  = relu(bn1(x . w1))                        padded [N][H+2][W+2][Cm]   (workspace; the plain 1x1 entry point)
//   t2  = relu(bn2(conv3x3_grouped(t1, wg)))       padded [N][H+2][W+2][Cm]   (workspace)
//   out = relu(bn3(t2 . w3) + x)                                              (the 1x1 with a residual)
// Projection block, torchvision's placement (the stride on the 3x3), H = (Hin-1)/stride + 1:
//   t1  = relu(bn1(x . w1))                        padded [N][Hin+2][Win+2][Cm]
//   t2  = relu(bn2(conv3x3_grouped(t1, wg, stride)))   padded [N][H+2][W+2][Cm]
//   out = relu(bn3(t2 . w3) + bnp(xs . wp)), xs = x[:, ::stride, ::stride, :]  (proj_block.hip's fused tail, A_TWO)
// The intermediates are exactly the dense blocks', so the workspaces are theirs: wino_residual_block_workspace_bytes_hw,
// wino_proj_block_workspace_bytes_hw (stride 1) and wino_proj_block_v15_workspace_bytes_hw (stride 2).  The grouped
// layer uses no stream scratch: the prepare entry points reserve the two 1x1 launches' only.
// This file instantiates no kernel.
#include "conv3x3_grouped.h"
#include "proj_block.h"

namespace wino {
namespace {

int check_grouped_residual(int N, int H, int W, int C4, int Cm, int groups) {
  if (int rc = check_bottleneck_1x1s(N, H, W, C4, Cm)) return rc;
  GroupedGeom gg;
  return check_grouped(N, H, W, Cm, groups, 1, &gg);
}

int check_grouped_proj(int N, int Hin, int Win, int Cin, int Cm, int C4, int groups, int stride, ProjGeom* g) {
  if (int rc = check_proj(N, Hin, Win, Cin, Cm, C4, stride, g)) return rc;
  if (int rc = check_first_1x1_full(N, Hin, Win, Cm)) return rc;
  GroupedGeom gg;
  return check_grouped(N, Hin, Win, Cm, groups, stride, &gg);
}

size_t grouped_proj_workspace(const ProjGeom& g) {
  return g.s == 1 ? wino_proj_block_workspace_bytes_hw(g.N, g.H, g.W, g.Cm)
                  : wino_proj_block_v15_workspace_bytes_hw(g.N, g.Hin, g.Win, g.Cm);
}

}  // namespace
}  // namespace wino

using namespace wino;

extern "C" {

int wino_grouped_residual_block_hw(const float* x, const float* w1, const float* bn1Bias, const float* bn1Scale,
                                   const float* wg, const float* bn2Bias, const float* bn2Scale, const float* w3,
                                   const float* bn3Bias, const float* bn3Scale, float* out, int N, int H, int W, int C4,
                                   int Cm, int groups, void* workspace, size_t workspace_bytes, wino_stream_t s) {
  if (int rc = check_nonnull(x, w1, bn1Bias, bn1Scale, wg, bn2Bias, bn2Scale, w3, bn3Bias, bn3Scale, out)) return rc;
  if (int rc = check_aligned16(x, w1, wg, w3, out, workspace)) return rc;
  if (int rc = check_grouped_residual(N, H, W, C4, Cm, groups)) return rc;
  const size_t need = wino_residual_block_workspace_bytes_hw(N, H, W, Cm);
  if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
  // x is read again as the residual by the third launch, after the first two have written the workspace
  const size_t act_b = (size_t)N * H * W * C4 * sizeof(float);
  if (overlaps(workspace, need, x, act_b) || overlaps(workspace, need, out, act_b)) {
    set_error("the workspace overlaps x or out");
    return WINO_E_ARG;
  }
  float* t1 = (float*)workspace;
  float* t2 = (float*)((char*)workspace + padded_bytes(N, H, W, Cm));
  int rc = wino_conv1x1_bn_ex_hw(x, w1, bn1Bias, bn1Scale, NULL, t1, N, H, W, C4, Cm, WINO_RELU | WINO_C_PADDED, s);
  if (rc) return rc;
  rc = wino_conv3x3_grouped_bn_relu_hw(t1, wg, bn2Bias, bn2Scale, t2, N, H, W, Cm, groups, 1, 1, s);
  if (rc) return rc;
  return wino_conv1x1_bn_ex_hw(t2, w3, bn3Bias, bn3Scale, x, out, N, H, W, Cm, C4,
                               WINO_RELU | WINO_A_PADDED | WINO_ADD_RESIDUAL, s);
}

int wino_grouped_residual_block_prepare_hw(int N, int H, int W, int C4, int Cm, int groups, wino_stream_t s) {
  if (int rc = check_grouped_residual(N, H, W, C4, Cm, groups)) return rc;
  const long M = (long)N * H * W;
  if (int rc = wino_conv1x1_prepare(M, C4, Cm, s)) return rc;
  return wino_conv1x1_prepare(M, Cm, C4, s);
}

int wino_grouped_proj_block_hw(const float* x, const float* w1, const float* bn1Bias, const float* bn1Scale,
                               const float* wg, const float* bn2Bias, const float* bn2Scale, const float* tail_packed,
                               float* out, int N, int Hin, int Win, int Cin, int Cm, int C4, int groups, int stride,
                               void* workspace, size_t workspace_bytes, wino_stream_t s) {
  if (int rc = check_nonnull(x, w1, bn1Bias, bn1Scale, wg, bn2Bias, bn2Scale, tail_packed, out)) return rc;
  if (int rc = check_aligned16(x, w1, wg, tail_packed, out, workspace)) return rc;
  ProjGeom g;
  if (int rc = check_grouped_proj(N, Hin, Win, Cin, Cm, C4, groups, stride, &g)) return rc;
  const size_t need = grouped_proj_workspace(g);
  if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
  if (int rc = check_ws_overlap(g, x, out, workspace, need)) return rc;
  int dev = 0, cus = 0;
  if (int rc = current_device(&dev, &cus)) return rc;
  float* t1 = (float*)workspace;
  float* t2 = (float*)((char*)workspace + padded_bytes(N, Hin, Win, Cm));
  int rc = wino_conv1x1_bn_ex_hw(x, w1, bn1Bias, bn1Scale, NULL, t1, N, Hin, Win, Cin, Cm, WINO_RELU | WINO_C_PADDED, s);
  if (rc) return rc;
  rc = wino_conv3x3_grouped_bn_relu_hw(t1, wg, bn2Bias, bn2Scale, t2, N, Hin, Win, Cm, groups, stride, 1, s);
  if (rc) return rc;
  return launch_proj_tail(g, t2, tail_packed, x, out, dev, cus, knobs(), (hipStream_t)s);
}

int wino_grouped_proj_block_prepare_hw(int N, int Hin, int Win, int Cin, int Cm, int C4, int groups, int stride,
                                       wino_stream_t s) {
  ProjGeom g;
  if (int rc = check_grouped_proj(N, Hin, Win, Cin, Cm, C4, groups, stride, &g)) return rc;
  int dev = 0, cus = 0;
  if (int rc = current_device(&dev, &cus)) return rc;
  if (int rc = wino_conv1x1_prepare((long)N * Hin * Win, Cin, Cm, s)) return rc;
  return prepare_proj_tail(g, dev, cus, (hipStream_t)s);
}

}  // extern "C"
