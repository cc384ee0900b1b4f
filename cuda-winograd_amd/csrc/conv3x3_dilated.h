// The dilated 3x3 layer's geometry check (defined in conv3x3_dilated.hip), shared with bottleneck.hip, which runs it
// for the dilated blocks' 3x3 before its first launch, and the layer's launch for aspp.hip, whose dilated branches write
// unpadded slots of a workspace.
#pragma once
#include "conv1x1_launch.h"

namespace wino {

struct DilGeom {
  int N, H, W, C, K, d;
  long M;
};
// every 32-bit quantity of the dilated tap addressing bounded (WINO_E_SHAPE and the error text otherwise)
int check_dilated(int N, int H, int W, int C, int K, int dilation, DilGeom* g);
// The layer's launch (g from check_dilated; the pointers are the caller's to check): in padded, out padded with its ring
// pass (out_padded) or plain [N*H*W][K] with no ring pass at all.  The plan is the layer's own either way, so
// wino_conv3x3_dilated_prepare_hw reserves its scratch.
int launch_dilated(const DilGeom& g, const float* in, const float* w_taps, const float* bnBias, const float* bnScale,
                   float* out, bool relu, bool out_padded, hipStream_t s);

}  // namespace wino
