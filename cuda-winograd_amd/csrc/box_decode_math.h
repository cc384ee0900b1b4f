// torchvision's BoxCoder.decode_single + clip_boxes_to_image for one box, operation by operation in fp32: the one place
// the arithmetic is written.  boxes.hip (box_decode_kernel: every anchor of a level or every class of a RoI) and
// retina.hip (retina_decode_kernel: only the selected anchors) both call it, so a box decoded by either is the same bits.
#pragma once
#include "wino_common.h"

#pragma clang fp contract(off)   // torch's arithmetic operation by operation: no product folded into a sum

namespace wino {

struct DecodeWeights {
  float wx, wy, ww, wh, clamp;
};

// torch.clamp's two halves: a NaN fails the compare and passes through
__device__ __forceinline__ float min_nan(float v, float hi) { return v > hi ? hi : v; }
__device__ __forceinline__ float clip_nan(float v, float hi) { return v < 0.f ? 0.f : (v > hi ? hi : v); }

// torchvision's AnchorGenerator: the base anchor shifted to pixel (x, y) of its level
__device__ __forceinline__ f32x4 grid_anchor(f32x4 base, unsigned x, unsigned y, float stride_x, float stride_y) {
  const float ox = (float)x * stride_x, oy = (float)y * stride_y;
  return base + f32x4{ox, oy, ox, oy};
}

__device__ __forceinline__ f32x4 decode_box(f32x4 anc, float d0, float d1, float d2, float d3, const DecodeWeights& k,
                                            float Himg, float Wimg) {
  const float w = anc.z - anc.x, h = anc.w - anc.y;
  const float cx = anc.x + 0.5f * w, cy = anc.y + 0.5f * h;
  const float dx = d0 / k.wx, dy = d1 / k.wy;
  const float dw = min_nan(d2 / k.ww, k.clamp), dh = min_nan(d3 / k.wh, k.clamp);
  const float pcx = dx * w + cx, pcy = dy * h + cy;
  const float pw = expf(dw) * w, ph = expf(dh) * h;
  const float hw_ = 0.5f * pw, hh_ = 0.5f * ph;
  return f32x4{clip_nan(pcx - hw_, Wimg), clip_nan(pcy - hh_, Himg), clip_nan(pcx + hw_, Wimg), clip_nan(pcy + hh_, Himg)};
}

}  // namespace wino
