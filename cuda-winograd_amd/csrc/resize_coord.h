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

// The bicubic align_corners=False coordinate of keypoints.hip: the same exact integers, NOT clamped at 0 (num > -2 out,
// so the floor division gives -1 below 0), and torch's cubic convolution coefficients at A = -0.75 for the taps
// i - 1 .. i + 2, which the caller clamps into [0, in) with clampi.  (2d+1) in < 2^31.
struct Cubic {
  int i;
  float c[4];
};
__host__ __device__ __forceinline__ Cubic cubic(int d, int in, int out) {
  const int num = (2 * d + 1) * in - out, two = 2 * out;
  Cubic q;
  q.i = num < 0 ? -1 : num / two;
  const float t = (float)(num - q.i * two) / (float)two, u = 1.f - t, A = -0.75f;
  const float xa = t + 1.f, xb = u + 1.f;
  q.c[0] = ((A * xa - 5.f * A) * xa + 8.f * A) * xa - 4.f * A;
  q.c[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
  q.c[2] = ((A + 2.f) * u - (A + 3.f)) * u * u + 1.f;
  q.c[3] = ((A * xb - 5.f * A) * xb + 8.f * A) * xb - 4.f * A;
  return q;
}
__host__ __device__ __forceinline__ int clampi(int i, int n) { return i < 0 ? 0 : (i < n ? i : n - 1); }

__device__ __forceinline__ float lerp2(float a, float b, float c, float d, float lx, float ly) {
  const float top = (1.f - lx) * a + lx * b;
  const float bot = (1.f - lx) * c + lx * d;
  return (1.f - ly) * top + ly * bot;
}

}  // namespace wino
