// The 1x1 layer's launch plan (conv1x1.hip), shared by the translation units that launch the 1x1 kernels:
// conv1x1.hip and the projection block's proj_block.hip.
#pragma once
#include "wino_common.h"

namespace wino {

// The latency form's choice (conv1x1_small_kernel.h): use it or not, its K split and MFMA tiles per wave.
struct Small1Plan {
  bool use;
  int ks, rt, ct;
  long long wgs;
  double t_us, t_big_us;   // the two launch models' times
};
// The plan of one launch, read by every consumer -- see plan_1x1 in conv1x1.hip.
struct Plan1x1 {
  bool four;            // 4-wave workgroups (64 columns), else 8 (128)
  int nblk, nk;         // column blocks, k-steps
  long long nMB;        // row tiles
  int sk;               // stream-K / split-K grid, 0: the plain form
  int grid;             // the tiled launch's grid (per batch)
  Small1Plan small;
};
Plan1x1 plan_1x1(long M, int Cin, int Kout, int batch, int cus, const Knobs& kn);
// the tiled kernel's stream-K scratch of stream `s` for this plan (sk_scratch)
int tiled_scratch(int dev, hipStream_t s, const Plan1x1& p, SkBufs* bufs);

}  // namespace wino
