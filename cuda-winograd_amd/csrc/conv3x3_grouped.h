// The grouped 3x3 layer's geometry check (defined in conv3x3_grouped.hip), shared with bottleneck.hip, which runs
// it for both grouped blocks before their first launch.
#pragma once
#include "wino_common.h"

namespace wino {

struct GroupedGeom {
  int N, Hin, Win, C, groups, Cg, stride, H, W;
  int KC;                  // input channels a 16-column MFMA tile contracts over: max(Cg, 16)
  int TW;                  // output columns of a workgroup's tile, 8 or 16
  int tiles_y, tiles_x;    // tiles per image
};
// stride 1 or 2 (WINO_E_ARG otherwise); C % 64 == 0, Cg = C / groups in {4, 8, 16, 32, 64}; one padded image of `in`
// below 2^31 elements and the grid below 2^31 workgroups (WINO_E_SHAPE and the error text otherwise).  Host only.
int check_grouped(int N, int Hin, int Win, int C, int groups, int stride, GroupedGeom* g);

}  // namespace wino
