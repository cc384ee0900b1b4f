// The bottleneck blocks: one composition behind seven block entry points (and the 14x14 form of the first).
//   first 1x1 (+BN+ReLU)           ->  t1, padded [N][H1+2][W1+2][Cm]   (workspace)
//   middle 3x3 (+BN+ReLU)          ->  t2, padded [N][H+2][W+2][Cm]     (workspace)
//   last 1x1 + shortcut (+ReLU)    ->  out [N][H][W][C4]
// with H = (Hin-1)/stride + 1 and H1 x W1 the grid the first 1x1 writes: H x W when it carries the stride, Hin x Win
// otherwise.  A block is one row of this table, a `Bottleneck` below:
//   entry point (wino_...)        stride        middle 3x3                             last layer
//   residual_block[_hw]           none          Winograd (wino_f2_fused.hip)           1x1 + residual x
//   proj_block_hw (v1)            first 1x1     Winograd at H x W                      fused tail (proj_block.hip, A_TWO)
//   proj_block_v15_hw             3x3, 2        stride-2 implicit GEMM (conv3x3_s2)    fused tail
//   grouped_residual_block_hw     none          grouped (conv3x3_grouped.hip)          1x1 + residual x
//   grouped_proj_block_hw         3x3, 1 or 2   grouped                                fused tail
//   dilated_residual_block_hw     none          dilated implicit GEMM (conv3x3_dilated) 1x1 + residual x
//   dilated_proj_block_hw         none (1)      dilated implicit GEMM                  fused tail
// From the row follow, once each: the shape check (the layers' own checks, so that a shape any of them refuses launches
// nothing), the workspace size and its t1 / t2 split, the overlap test, and ONE listing of the three layers
// (run_bottleneck) that the block's launch and its *_prepare both walk -- a prepare reserves the stream scratch of
// exactly the launches the block makes.  Every refusal comes in one order: NULL, alignment, shape, workspace size,
// overlap, then the launches' device queries.  Host code over the layers' launches: this file instantiates no kernel.
#include "conv3x3_dilated.h"
#include "conv3x3_grouped.h"
#include "proj_block.h"

namespace wino {
namespace {

enum StrideAt { STRIDE_NONE, STRIDE_FIRST, STRIDE_MIDDLE };   // which layer carries the stride (and the shortcut with it)
enum Middle { MID_WINOGRAD, MID_S2_GEMM, MID_GROUPED, MID_DILATED };
enum Last { LAST_RESIDUAL, LAST_TAIL };   // 1x1 + the identity shortcut (Cin = C4), or the fused projection tail
struct Bottleneck {
  int N, Hin, Win, Cin, Cm, C4;
  StrideAt at;
  int stride;
  Middle mid;
  int groups;   // MID_GROUPED
  Last last;
  int dilation = 1;   // MID_DILATED
};
// A launch's tensors; w3: the last 1x1's matrix, or the packed tail (then without b3 / s3)
struct Tensors {
  const float *x, *w1, *b1, *s1, *w2, *b2, *s2, *w3, *b3, *s3;
  float* out;
};

// the workspace: t1 on the first 1x1's grid, then t2 on the output grid
size_t workspace_need(int N, int H1, int W1, int H, int W, int Cm) {
  return padded_bytes(N, H1, W1, Cm) + padded_bytes(N, H, W, Cm);
}

// Every layer's shape check, in the block's layer order; *g: the geometry the launches use (an identity block is the
// projection geometry at stride 1 with Cin = C4)
int check_shape(const Bottleneck& b, ProjGeom* g) {
  if (b.last == LAST_TAIL) {
    if (int rc = check_proj(b.N, b.Hin, b.Win, b.Cin, b.Cm, b.C4, b.stride, g)) return rc;
    if (b.at != STRIDE_FIRST)
      if (int rc = check_first_1x1_full(b.N, b.Hin, b.Win, b.Cm)) return rc;
  } else {
    if (int rc = check_bottleneck_1x1s(b.N, b.Hin, b.Win, b.C4, b.Cm)) return rc;
    *g = ProjGeom{b.N, b.Hin, b.Win, b.C4, b.Cm, b.C4, 1, b.Hin, b.Win, (long)b.N * b.Hin * b.Win};
  }
  switch (b.mid) {
    case MID_WINOGRAD: return check_conv3x3_dims(g->H, g->W, b.Cm, b.Cm);
    case MID_S2_GEMM: {
      S2Geom g2;
      return check_s2(b.N, b.Hin, b.Win, b.Cm, b.Cm, &g2);
    }
    case MID_DILATED: {
      DilGeom gd;
      return check_dilated(b.N, b.Hin, b.Win, b.Cm, b.Cm, b.dilation, &gd);
    }
    default: {
      GroupedGeom gg;
      return check_grouped(b.N, b.Hin, b.Win, b.Cm, b.groups, g->s, &gg);
    }
  }
}

// The block: checked, then its three layers launched (t: the tensors, with the workspace) or, t == nullptr, the stream
// scratch of those launches reserved ahead of a graph capture.
int run_bottleneck(const Bottleneck& b, const Tensors* t, void* workspace, size_t workspace_bytes, wino_stream_t s) {
  if (t) {
    if (int rc = check_nonnull(t->x, t->w1, t->b1, t->s1, t->w2, t->b2, t->s2, t->w3, t->out)) return rc;
    if (b.last == LAST_RESIDUAL)
      if (int rc = check_nonnull(t->b3, t->s3)) return rc;
    if (int rc = check_aligned16(t->x, t->w1, t->w2, t->w3, t->out, workspace)) return rc;
  }
  ProjGeom g;
  if (int rc = check_shape(b, &g)) return rc;
  const bool strided_first = b.at == STRIDE_FIRST;
  const int N = g.N, Cm = g.Cm, H1 = strided_first ? g.H : g.Hin, W1 = strided_first ? g.W : g.Win;
  float *t1 = nullptr, *t2 = nullptr;
  if (t) {
    const size_t need = workspace_need(N, H1, W1, g.H, g.W, Cm);
    if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    // t1 and t2 are written before the last launch reads x again (its shortcut) and writes out
    const size_t x_b = (size_t)N * g.Hin * g.Win * g.Cin * sizeof(float), out_b = (size_t)g.M * g.C4 * sizeof(float);
    if (overlaps(workspace, need, t->x, x_b) || overlaps(workspace, need, t->out, out_b)) {
      set_error("the workspace overlaps x or out");
      return WINO_E_ARG;
    }
    t1 = (float*)workspace;
    t2 = (float*)((char*)workspace + padded_bytes(N, H1, W1, Cm));
  }
  const hipStream_t hs = (hipStream_t)s;
  int rc;
  // first 1x1, Cin -> Cm on H1 x W1 (the strided form launches the plain layer's plan at that grid: one reservation)
  if (!t) rc = wino_conv1x1_prepare((long)N * H1 * W1, g.Cin, Cm, s);
  else if (strided_first && g.s != 1) rc = launch_first_strided(g, t->x, t->w1, t->b1, t->s1, t1, hs);
  else rc = wino_conv1x1_bn_ex_hw(t->x, t->w1, t->b1, t->s1, NULL, t1, N, H1, W1, g.Cin, Cm, WINO_RELU | WINO_C_PADDED, s);
  if (rc) return rc;
  // middle 3x3, Cm -> Cm from H1 x W1 to H x W
  switch (b.mid) {
    case MID_WINOGRAD:
      rc = t ? wino_conv3x3_bn_relu_hw(t1, t->w2, t->b2, t->s2, t2, N, H1, W1, Cm, Cm, 1, s)
             : wino_conv3x3_prepare_hw(N, H1, W1, Cm, Cm, s);
      break;
    case MID_S2_GEMM:
      rc = t ? wino_conv3x3_s2_bn_relu_hw(t1, t->w2, t->b2, t->s2, t2, N, H1, W1, Cm, Cm, 1, s)
             : wino_conv3x3_s2_prepare_hw(N, H1, W1, Cm, Cm, s);
      break;
    case MID_DILATED:
      rc = t ? wino_conv3x3_dilated_bn_relu_hw(t1, t->w2, t->b2, t->s2, t2, N, H1, W1, Cm, Cm, b.dilation, 1, s)
             : wino_conv3x3_dilated_prepare_hw(N, H1, W1, Cm, Cm, b.dilation, s);
      break;
    default:   // (the grouped layer uses no stream scratch)
      rc = t ? wino_conv3x3_grouped_bn_relu_hw(t1, t->w2, t->b2, t->s2, t2, N, H1, W1, Cm, b.groups, g.s, 1, s) : WINO_OK;
  }
  if (rc) return rc;
  // last 1x1 with its shortcut, Cm -> C4 on H x W
  if (b.last == LAST_TAIL) return t ? launch_proj_tail(g, t2, t->w3, t->x, t->out, hs) : prepare_proj_tail(g, hs);
  if (!t) return wino_conv1x1_prepare(g.M, Cm, g.C4, s);
  return wino_conv1x1_bn_ex_hw(t2, t->w3, t->b3, t->s3, t->x, t->out, N, g.H, g.W, Cm, g.C4,
                               WINO_RELU | WINO_A_PADDED | WINO_ADD_RESIDUAL, s);
}

// the seven rows of the table
Bottleneck residual(int N, int H, int W, int C4, int Cm) {
  return {N, H, W, C4, Cm, C4, STRIDE_NONE, 1, MID_WINOGRAD, 1, LAST_RESIDUAL};
}
Bottleneck proj_v1(int N, int Hin, int Win, int Cin, int Cm, int C4, int stride) {
  return {N, Hin, Win, Cin, Cm, C4, STRIDE_FIRST, stride, MID_WINOGRAD, 1, LAST_TAIL};
}
Bottleneck proj_v15(int N, int Hin, int Win, int Cin, int Cm, int C4) {
  return {N, Hin, Win, Cin, Cm, C4, STRIDE_MIDDLE, 2, MID_S2_GEMM, 1, LAST_TAIL};
}
Bottleneck grouped_residual(int N, int H, int W, int C4, int Cm, int groups) {
  return {N, H, W, C4, Cm, C4, STRIDE_NONE, 1, MID_GROUPED, groups, LAST_RESIDUAL};
}
Bottleneck grouped_proj(int N, int Hin, int Win, int Cin, int Cm, int C4, int groups, int stride) {
  return {N, Hin, Win, Cin, Cm, C4, STRIDE_MIDDLE, stride, MID_GROUPED, groups, LAST_TAIL};
}
Bottleneck dilated_residual(int N, int H, int W, int C4, int Cm, int dilation) {
  return {N, H, W, C4, Cm, C4, STRIDE_NONE, 1, MID_DILATED, 1, LAST_RESIDUAL, dilation};
}
Bottleneck dilated_proj(int N, int H, int W, int Cin, int Cm, int C4, int dilation) {
  return {N, H, W, Cin, Cm, C4, STRIDE_MIDDLE, 1, MID_DILATED, 1, LAST_TAIL, dilation};
}

}  // namespace
}  // namespace wino

using namespace wino;

extern "C" {

// ---- the identity block: 1x1 (C4 -> Cm), Winograd 3x3, 1x1 (Cm -> C4) + x
int wino_residual_block_hw(const float* x, const float* w1, const float* bn1Bias, const float* bn1Scale,
                           const float* U2, const float* bn2Bias, const float* bn2Scale,
                           const float* w3, const float* bn3Bias, const float* bn3Scale, float* out,
                           int N, int H, int W, int C4, int Cm, void* workspace, size_t workspace_bytes,
                           wino_stream_t s) {
  const Tensors t{x, w1, bn1Bias, bn1Scale, U2, bn2Bias, bn2Scale, w3, bn3Bias, bn3Scale, out};
  return run_bottleneck(residual(N, H, W, C4, Cm), &t, workspace, workspace_bytes, s);
}

int wino_residual_block_prepare_hw(int N, int H, int W, int C4, int Cm, wino_stream_t s) {
  return run_bottleneck(residual(N, H, W, C4, Cm), nullptr, nullptr, 0, s);
}

size_t wino_residual_block_workspace_bytes_hw(int N, int H, int W, int Cm) { return workspace_need(N, H, W, H, W, Cm); }

int wino_residual_block(const float* x, const float* w1, const float* bn1Bias, const float* bn1Scale,
                        const float* U2, const float* bn2Bias, const float* bn2Scale,
                        const float* w3, const float* bn3Bias, const float* bn3Scale, float* out,
                        int N, int C4, int Cm, void* workspace, size_t workspace_bytes,
                        wino_stream_t s) {
  return wino_residual_block_hw(x, w1, bn1Bias, bn1Scale, U2, bn2Bias, bn2Scale, w3, bn3Bias, bn3Scale, out,
                                N, WINO_PQ, WINO_PQ, C4, Cm, workspace, workspace_bytes, s);
}

int wino_residual_block_prepare(int N, int C4, int Cm, wino_stream_t s) {
  return wino_residual_block_prepare_hw(N, WINO_PQ, WINO_PQ, C4, Cm, s);
}

size_t wino_residual_block_workspace_bytes(int N, int Cm) {
  return wino_residual_block_workspace_bytes_hw(N, WINO_PQ, WINO_PQ, Cm);
}

// ---- the projection block, v1 placement: strided 1x1, Winograd 3x3 on the output grid, fused tail
int wino_proj_block_hw(const float* x, const float* w1, const float* bn1Bias, const float* bn1Scale, const float* U2,
                       const float* bn2Bias, const float* bn2Scale, const float* tail_packed, float* out, int N, int Hin,
                       int Win, int Cin, int Cm, int C4, int stride, void* workspace, size_t workspace_bytes,
                       wino_stream_t s) {
  const Tensors t{x, w1, bn1Bias, bn1Scale, U2, bn2Bias, bn2Scale, tail_packed, nullptr, nullptr, out};
  return run_bottleneck(proj_v1(N, Hin, Win, Cin, Cm, C4, stride), &t, workspace, workspace_bytes, s);
}

int wino_proj_block_prepare_hw(int N, int Hin, int Win, int Cin, int Cm, int C4, int stride, wino_stream_t s) {
  return run_bottleneck(proj_v1(N, Hin, Win, Cin, Cm, C4, stride), nullptr, nullptr, 0, s);
}

size_t wino_proj_block_workspace_bytes_hw(int N, int H, int W, int Cm) {
  if (N < 1 || H < 1 || W < 1 || Cm < 1) return 0;
  return workspace_need(N, H, W, H, W, Cm);
}

// ---- the projection block, v1.5 placement: 1x1 at the full input, stride-2 3x3, fused tail
int wino_proj_block_v15_hw(const float* x, const float* w1, const float* bn1Bias, const float* bn1Scale,
                           const float* w2_taps, const float* bn2Bias, const float* bn2Scale, const float* tail_packed,
                           float* out, int N, int Hin, int Win, int Cin, int Cm, int C4, void* workspace,
                           size_t workspace_bytes, wino_stream_t s) {
  const Tensors t{x, w1, bn1Bias, bn1Scale, w2_taps, bn2Bias, bn2Scale, tail_packed, nullptr, nullptr, out};
  return run_bottleneck(proj_v15(N, Hin, Win, Cin, Cm, C4), &t, workspace, workspace_bytes, s);
}

int wino_proj_block_v15_prepare_hw(int N, int Hin, int Win, int Cin, int Cm, int C4, wino_stream_t s) {
  return run_bottleneck(proj_v15(N, Hin, Win, Cin, Cm, C4), nullptr, nullptr, 0, s);
}

size_t wino_proj_block_v15_workspace_bytes_hw(int N, int Hin, int Win, int Cm) {
  if (N < 1 || Hin < 1 || Win < 1 || Cm < 1) return 0;
  return workspace_need(N, Hin, Win, (Hin - 1) / 2 + 1, (Win - 1) / 2 + 1, Cm);
}

// ---- the ResNeXt blocks: the grouped 3x3 in the middle.  Their intermediates are the dense blocks', so their
// workspaces are sized by the dense blocks' queries above.
int wino_grouped_residual_block_hw(const float* x, const float* w1, const float* bn1Bias, const float* bn1Scale,
                                   const float* wg, const float* bn2Bias, const float* bn2Scale, const float* w3,
                                   const float* bn3Bias, const float* bn3Scale, float* out, int N, int H, int W, int C4,
                                   int Cm, int groups, void* workspace, size_t workspace_bytes, wino_stream_t s) {
  const Tensors t{x, w1, bn1Bias, bn1Scale, wg, bn2Bias, bn2Scale, w3, bn3Bias, bn3Scale, out};
  return run_bottleneck(grouped_residual(N, H, W, C4, Cm, groups), &t, workspace, workspace_bytes, s);
}

int wino_grouped_residual_block_prepare_hw(int N, int H, int W, int C4, int Cm, int groups, wino_stream_t s) {
  return run_bottleneck(grouped_residual(N, H, W, C4, Cm, groups), nullptr, nullptr, 0, s);
}

int wino_grouped_proj_block_hw(const float* x, const float* w1, const float* bn1Bias, const float* bn1Scale,
                               const float* wg, const float* bn2Bias, const float* bn2Scale, const float* tail_packed,
                               float* out, int N, int Hin, int Win, int Cin, int Cm, int C4, int groups, int stride,
                               void* workspace, size_t workspace_bytes, wino_stream_t s) {
  const Tensors t{x, w1, bn1Bias, bn1Scale, wg, bn2Bias, bn2Scale, tail_packed, nullptr, nullptr, out};
  return run_bottleneck(grouped_proj(N, Hin, Win, Cin, Cm, C4, groups, stride), &t, workspace, workspace_bytes, s);
}

int wino_grouped_proj_block_prepare_hw(int N, int Hin, int Win, int Cin, int Cm, int C4, int groups, int stride,
                                       wino_stream_t s) {
  return run_bottleneck(grouped_proj(N, Hin, Win, Cin, Cm, C4, groups, stride), nullptr, nullptr, 0, s);
}

// ---- the dilated blocks (the segmentation backbones' layer3 / layer4): the dilated 3x3 in the middle, stride 1.
// Their intermediates are the dense blocks', so their workspaces are sized by the dense blocks' queries above.
int wino_dilated_residual_block_hw(const float* x, const float* w1, const float* bn1Bias, const float* bn1Scale,
                                   const float* w2_taps, const float* bn2Bias, const float* bn2Scale, const float* w3,
                                   const float* bn3Bias, const float* bn3Scale, float* out, int N, int H, int W, int C4,
                                   int Cm, int dilation, void* workspace, size_t workspace_bytes, wino_stream_t s) {
  const Tensors t{x, w1, bn1Bias, bn1Scale, w2_taps, bn2Bias, bn2Scale, w3, bn3Bias, bn3Scale, out};
  return run_bottleneck(dilated_residual(N, H, W, C4, Cm, dilation), &t, workspace, workspace_bytes, s);
}

int wino_dilated_residual_block_prepare_hw(int N, int H, int W, int C4, int Cm, int dilation, wino_stream_t s) {
  return run_bottleneck(dilated_residual(N, H, W, C4, Cm, dilation), nullptr, nullptr, 0, s);
}

int wino_dilated_proj_block_hw(const float* x, const float* w1, const float* bn1Bias, const float* bn1Scale,
                               const float* w2_taps, const float* bn2Bias, const float* bn2Scale,
                               const float* tail_packed, float* out, int N, int H, int W, int Cin, int Cm, int C4,
                               int dilation, void* workspace, size_t workspace_bytes, wino_stream_t s) {
  const Tensors t{x, w1, bn1Bias, bn1Scale, w2_taps, bn2Bias, bn2Scale, tail_packed, nullptr, nullptr, out};
  return run_bottleneck(dilated_proj(N, H, W, Cin, Cm, C4, dilation), &t, workspace, workspace_bytes, s);
}

int wino_dilated_proj_block_prepare_hw(int N, int H, int W, int Cin, int Cm, int C4, int dilation, wino_stream_t s) {
  return run_bottleneck(dilated_proj(N, H, W, Cin, Cm, C4, dilation), nullptr, nullptr, 0, s);
}

}  // extern "C"
