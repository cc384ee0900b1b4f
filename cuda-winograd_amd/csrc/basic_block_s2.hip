// The downsampling basic block of ResNet-18 / -34 (the first block of conv3, conv4 and conv5; torchvision's BasicBlock
// with `downsample`):
//   t1  = relu(bn1(conv3x3_s2(x, w1)))          C -> K, stride 2, pad 1        padded [N][H+2][W+2][K]  (workspace)
//   sc  = bnd(conv1x1_s2(x, wd))                C -> K, stride 2, no ReLU      interior of out
//   out = relu(bn2(conv3x3(t1, U2)) + sc)       K -> K, stride 1, in place on out
// In the stride-2, pad-1 3x3 the centre tap (1, 1) of output pixel (y, x) reads input pixel (2y, 2x) -- exactly the
// pixel the 1x1 stride-2 shortcut reads.  So the shortcut is the stride-2 3x3's implicit GEMM (A_TAPS, conv3x3_s2.hip)
// over GEMM columns [4C, 5C) with its own B, BN and no ReLU: operand form A_TAPS_PROJ (conv1x1_kernel.h) runs both in
// ONE launch, the shortcut as whole tiles (tiled / stream-K) or column groups (latency form) appended to the 3x3's
// grid.  The 3x3's own workgroups keep the plain layer's mapping, plan (plan_s2, unchanged), k order and epilogue:
// t1 is bitwise the plain layer's output.  The block's second launch is the residual Winograd 3x3 in place on out
// (conv3x3_res.hip).  This file instantiates the 1x1 kernel templates in form A_TAPS_PROJ and no other.
#include "conv3x3_s2.h"

namespace wino {
namespace {

using namespace gemm1x1;

// packed = [w_taps ; wd] ([10 C][K], row-major: the nine taps' 9 C rows, then the shortcut's C rows), then bn1Bias,
// bn1Scale, bndBias, bndScale (K each).  The scales stay unfolded: the epilogues apply them as the plain layer does.
__global__ void s2_proj_pack_kernel(const float* __restrict__ w_taps, const float* __restrict__ b1,
                                    const float* __restrict__ s1, const float* __restrict__ wd,
                                    const float* __restrict__ bd, const float* __restrict__ sd,
                                    float* __restrict__ packed, int C, int K) {
  const long total = (long)(10 * C + 4) * K;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long r = i / K;
  const int k = (int)(i - r * K);
  float v;
  if (r < 9l * C) v = w_taps[i];
  else if (r < 10l * C) v = wd[i - 9l * C * K];
  else if (r == 10l * C) v = b1[k];
  else if (r == 10l * C + 1) v = s1[k];
  else if (r == 10l * C + 2) v = bd[k];
  else v = sd[k];
  packed[i] = v;
}

size_t packed_bytes(int C, int K) { return (size_t)(10 * (size_t)C + 4) * K * sizeof(float); }

// The fused layer's launch: the plain stride-2 layer's plan and operands, plus the shortcut's output in R
int launch_s2_proj(const float* in, const float* packed, float* t1, float* sc, const S2Geom& g, hipStream_t s) {
  int dev = 0, cus = 0;
  if (int rc = current_device(&dev, &cus)) return rc;
  const ProjGeo xg{nullptr, (unsigned)(g.Hin + 2) * (unsigned)(g.Win + 2), 2u * (unsigned)(g.Win + 2), 2u, g.C, g.Win + 2};
  const float* bn = packed + (size_t)10 * g.C * g.K;
  return launch_1x1<A_TAPS_PROJ>(plan_s2(g, cus, knobs()), dev,
                                 {in, packed, bn, bn + g.K, sc, t1, g.M, 9 * g.C, g.K, WINO_RELU | WINO_C_PADDED,
                                  make_padgeo(g.H, g.W), xg},
                                 s);
}

}  // namespace
}  // namespace wino

using namespace wino;

extern "C" {

size_t wino_s2_proj_elems(int C, int K) {
  if (C <= 0 || K <= 0) return 0;
  return (size_t)(10 * (size_t)C + 4) * (size_t)K;
}

int wino_s2_proj_pack(const float* w_taps, const float* bn1Bias, const float* bn1Scale, const float* wd,
                      const float* bndBias, const float* bndScale, float* packed, int C, int K, wino_stream_t s) {
  if (int rc = check_nonnull(w_taps, bn1Bias, bn1Scale, wd, bndBias, bndScale, packed)) return rc;
  if (int rc = check_aligned16(packed)) return rc;
  if (C <= 0 || K <= 0 || C % 32 || K % 64) {
    set_error("stride-2 projection pack: unsupported channels C=%d K=%d (need C %% 32 == 0, K %% 64 == 0)", C, K);
    return WINO_E_SHAPE;
  }
  const long total = (long)(10 * C + 4) * K;
  hipLaunchKernelGGL(s2_proj_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)s, w_taps,
                     bn1Bias, bn1Scale, wd, bndBias, bndScale, packed, C, K);
  return launch_status("s2_proj_pack_kernel");
}

int wino_conv3x3_s2_proj_bn_relu_hw(const float* in, const float* packed, float* t1, float* sc, int N, int Hin, int Win,
                                    int C, int K, wino_stream_t s) {
  if (int rc = check_nonnull(in, packed, t1, sc)) return rc;
  if (int rc = check_aligned16(in, packed, t1, sc)) return rc;
  S2Geom g;
  if (int rc = check_s2(N, Hin, Win, C, K, &g)) return rc;
  const size_t in_b = padded_bytes(N, Hin, Win, C), out_b = padded_bytes(N, g.H, g.W, K);
  if (any_overlap({{in, in_b}, {packed, packed_bytes(C, K)}, {t1, out_b}, {sc, out_b}})) {
    set_error("the input, the packed filters, t1 and sc must not overlap");
    return WINO_E_ARG;
  }
  return launch_s2_proj(in, packed, t1, sc, g, (hipStream_t)s);
}

size_t wino_basic_block_s2_workspace_bytes_hw(int N, int Hin, int Win, int K) {
  if (N < 1 || Hin < 1 || Win < 1 || K < 1) return 0;
  return padded_bytes(N, (Hin - 1) / 2 + 1, (Win - 1) / 2 + 1, K);
}

int wino_basic_block_s2_prepare_hw(int N, int Hin, int Win, int C, int K, wino_stream_t s) {
  S2Geom g;
  if (int rc = check_s2(N, Hin, Win, C, K, &g)) return rc;
  if (int rc = check_conv3x3_dims(g.H, g.W, K, K)) return rc;   // the second conv, K -> K on the H x W grid
  // the fused layer's scratch is the plain stride-2 layer's (same plan), the second launch's the plain K -> K 3x3's
  if (int rc = wino_conv3x3_s2_prepare_hw(N, Hin, Win, C, K, s)) return rc;
  return wino_conv3x3_prepare_hw(N, g.H, g.W, K, K, s);
}

int wino_basic_block_s2_hw(const float* x, const float* packed, const float* U2, const float* bn2Bias,
                           const float* bn2Scale, float* out, int N, int Hin, int Win, int C, int K, void* workspace,
                           size_t workspace_bytes, wino_stream_t s) {
  if (int rc = check_nonnull(x, packed, U2, bn2Bias, bn2Scale, out, workspace)) return rc;
  if (int rc = check_aligned16(x, packed, U2, out, workspace)) return rc;
  S2Geom g;
  if (int rc = check_s2(N, Hin, Win, C, K, &g)) return rc;
  if (int rc = check_conv3x3_dims(g.H, g.W, K, K)) return rc;   // the second conv
  const size_t need = wino_basic_block_s2_workspace_bytes_hw(N, Hin, Win, K);
  if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
  if (any_overlap({{x, padded_bytes(N, Hin, Win, C)}, {packed, packed_bytes(C, K)}, {out, need}, {workspace, need}})) {
    set_error("x, packed, out and the workspace must not overlap");
    return WINO_E_ARG;
  }
  float* t1 = (float*)workspace;
  // sc goes into out's interior; the residual 3x3 then reads each element just before it stores over it, and writes
  // out's zero ring (conv3x3_res.hip)
  if (int rc = launch_s2_proj(x, packed, t1, out, g, (hipStream_t)s)) return rc;
  return wino_conv3x3_bn_add_relu_hw(t1, U2, bn2Bias, bn2Scale, out, out, N, g.H, g.W, K, K, 1, s);
}

}  // extern "C"
