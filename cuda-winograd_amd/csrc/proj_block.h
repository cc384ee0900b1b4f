// The projection block's geometry check and its fused tail (defined in proj_block.hip), and the bottleneck block's 1x1
// checks (conv1x1.hip), shared with grouped_block.hip: the grouped blocks are the same compositions around another
// middle layer, so they run the same checks, plans and launches for their 1x1 layers.
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
int check_ws_overlap(const ProjGeom& g, const void* x, const void* out, const void* workspace, size_t need);
// the tail launch (the last 1x1 and the projection shortcut as one GEMM), and its stream-K scratch ahead of a capture
int launch_proj_tail(const ProjGeom& g, const float* t2, const float* tail_packed, const float* x, float* out, int dev,
                     int cus, const Knobs& kn, hipStream_t s);
int prepare_proj_tail(const ProjGeom& g, int dev, int cus, hipStream_t s);
// the identity bottleneck's batch, feature map and two 1x1 layers (C4 -> Cm writing padded t1, Cm -> C4 reading padded t2)
int check_bottleneck_1x1s(int N, int H, int W, int C4, int Cm);

}  // namespace wino
