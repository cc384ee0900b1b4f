// The dilated 3x3 layer's geometry check (defined in conv3x3_dilated.hip), shared with bottleneck.hip, which runs it
// for the dilated blocks' 3x3 before its first launch.
#pragma once
#include "conv1x1_launch.h"

namespace wino {

struct DilGeom {
  int N, H, W, C, K, d;
  long M;
};
// every 32-bit quantity of the dilated tap addressing bounded (WINO_E_SHAPE and the error text otherwise)
int check_dilated(int N, int H, int W, int C, int K, int dilation, DilGeom* g);

}  // namespace wino
