// The bilinear align_corners=False coordinate rule and value formula that resize.hip and image_transform.hip share
// (mask_paste.hip states the same rule for its own window arithmetic).
#pragma once
#include "wino_common.h"

namespace wino {

struct Coord {
  int i0, i1;
  float lam;
};
// (2d+1) in < 2 out in < 2^31 (checked by the entry points)
__host__ __device__ __forceinline__ Coord coord(int d, int in, int out) {
  int num = (2 * d + 1) * in - out;
  if (num < 0) num = 0;
  const int two = 2 * out;
  Coord c;
  c.i0 = num / two;
  c.i1 = c.i0 + 1 < in ? c.i0 + 1 : in - 1;
  c.lam = (float)(num - c.i0 * two) / (float)two;
  return c;
}

__device__ __forceinline__ float lerp2(float a, float b, float c, float d, float lx, float ly) {
  const float top = (1.f - lx) * a + lx * b;
  const float bot = (1.f - lx) * c + lx * d;
  return (1.f - ly) * top + ly * bot;
}

}  // namespace wino
