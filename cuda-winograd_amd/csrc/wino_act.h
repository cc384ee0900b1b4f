// The WINO_ACT_* activations as the depthwise K x K layer and the squeeze-excite kernels apply them (depthwise_ex.hip,
// se.hip).  Every compare is one a NaN fails, so a NaN passes through all of them, as relu_nan does; all but the hard
// sigmoid map 0 to 0, which is what lets a zero ring and zero pad channels survive them.  Compile the including source
// under `#pragma clang fp contract(off)`: the products and sums below are the contract, not an fma.
#pragma once
#include "wino_common.h"

namespace wino {

__host__ __device__ __forceinline__ float min_nan(float v, float cap) { return v > cap ? cap : v; }
// min(max(y + 3, 0), 6) / 6
__host__ __device__ __forceinline__ float hardsigmoid_nan(float y) { return min_nan(relu_nan(y + 3.0f), 6.0f) * (1.0f / 6.0f); }

__host__ __device__ __forceinline__ float act_apply(float y, int act) {
  switch (act) {
    case WINO_ACT_RELU: return relu_nan(y);
    case WINO_ACT_RELU6: return min_nan(relu_nan(y), 6.0f);
    case WINO_ACT_HARDSWISH: return (y * min_nan(relu_nan(y + 3.0f), 6.0f)) * (1.0f / 6.0f);
    case WINO_ACT_HARDSIGMOID: return hardsigmoid_nan(y);
    default: return y;
  }
}
__host__ __device__ __forceinline__ f32x4 act_apply4(f32x4 v, int act) {
  if (act == WINO_ACT_NONE) return v;
  f32x4 r;
#pragma unroll
  for (int j = 0; j < 4; j++) r[j] = act_apply(v[j], act);
  return r;
}
inline bool act_known(int act) { return act >= WINO_ACT_NONE && act <= WINO_ACT_HARDSIGMOID; }
// the activations a depthwise layer takes in front of and behind it: all of them map 0 to 0
inline bool act_keeps_zero(int act) { return act_known(act) && act != WINO_ACT_HARDSIGMOID; }

}  // namespace wino
