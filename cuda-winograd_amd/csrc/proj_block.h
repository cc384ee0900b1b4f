// What bottleneck.hip composes the bottleneck blocks from, beside the layers' public entry points: the projection
// block's geometry check and its two launches in operand forms of their own (defined in proj_block.hip), and the
// identity block's 1x1 checks (conv1x1.hip).
#pragma once
#include "conv3x3_s2.h"

namespace wino {

struct ProjGeom {
  int N, Hin, Win, Cin, Cm, C4, s, H, W;
  long M;
};
// stride 1 or 2 (WINO_E_ARG otherwise) and every 32-bit quantity of the strided first 1x1 and of the tail bounded
int check_proj(int N, int Hin, int Win, int Cin, int Cm, int C4, int stride, ProjGeom* g);
// the limits of a first 1x1 (-> Cm, padded output) that runs at the full Hin x Win
int check_first_1x1_full(int N, int Hin, int Win, int Cm);
// the first 1x1 reading x at stride g.s (its plan, and so its stream scratch, is the plain layer's at M = N*H*W)
int launch_first_strided(const ProjGeom& g, const float* x, const float* w1, const float* bnBias, const float* bnScale,
                         float* t1, hipStream_t s);
// the tail launch (the last 1x1 and the projection shortcut as one GEMM), and its stream-K scratch ahead of a capture
int launch_proj_tail(const ProjGeom& g, const float* t2, const float* tail_packed, const float* x, float* out,
                     hipStream_t s);
int prepare_proj_tail(const ProjGeom& g, hipStream_t s);
// the identity bottleneck's batch, feature map and two 1x1 layers (C4 -> Cm writing padded t1, Cm -> C4 reading padded t2)
int check_bottleneck_1x1s(int N, int H, int W, int C4, int Cm);

}  // namespace wino
