// The stride-2 3x3 layer's geometry check and launch plan (defined in conv3x3_s2.hip), shared by the translation units
// that launch the tap forms: conv3x3_s2.hip (A_TAPS) and basic_block_s2.hip (A_TAPS_PROJ, the layer with the
// downsampling basic block's shortcut), which takes exactly the plain layer's plan.  bottleneck.hip runs check_s2 for
// the v1.5 block's stride-2 3x3 before its first launch.
#pragma once
#include "conv1x1_launch.h"

namespace wino {

struct S2Geom {
  int N, Hin, Win, C, K, H, W;
  long M;
};
// every 32-bit quantity of the tap addressing bounded (WINO_E_SHAPE and the error text otherwise)
int check_s2(int N, int Hin, int Win, int C, int K, S2Geom* g);
// plan_1x1 of the GEMM (N*H*W, 9C, K) with its latency-or-tiled choice re-priced for the tap form
Plan1x1 plan_s2(const S2Geom& g, int cus, const Knobs& kn);

}  // namespace wino
