// Multi-scale RoIAlign: torchvision's roi_align(..., aligned=False) over 1 to 4 pyramid levels, with MultiScaleRoIAlign's
// level assignment in the kernel.  One launch serves all boxes of all images and levels; no workspace, no stream
// scratch, no prepare: it can be captured into a graph as it is.
//
// wino_roi_align_hw:  f_l [N][h_l(+2)][w_l(+2)][C] (NHWC, finest first), rois [R][5] = (batch index, x1, y1, x2, y2) in image
//   pixels -> out [R][P(+2)][P(+2)][C]; with out_padded the ring is written as exact 0 (the Winograd layer's input at N = R).
//
// Arithmetic, torchvision's CPU kernel operation by operation in fp32 (s = scale of the box's level, S = sampling):
//   sx = x1 s, sy = y1 s, ex = x2 s, ey = y2 s;  roi_w = max(ex - sx, 1), roi_h = max(ey - sy, 1);  bin = roi / P.
//   Output (ph, pw) is the sum over iy, ix < S (iy outer) of the sample at y = sy + ph bin_h + (iy + .5) bin_h / S,
//   x = sx + pw bin_w + (ix + .5) bin_w / S, divided by S^2.  A sample with y < -1 || y > h || x < -1 || x > w
//   contributes 0 and reads nothing that reaches the result.  Otherwise v = max(v, 0), low = (int)v; at low >= size - 1
//   both taps are size - 1 and the fraction is 0, else high = low + 1 and l = v - low; with h. = 1 - l. the sample is
//   hy hx a + hy lx b + ly hx c + ly lx d.  Every in-range sample multiplies all four taps, so a NaN or Inf under a
//   zero weight still reaches the output (0 * NaN), as in wino_resize_bilinear_hw.  (The sums contract into FMAs.)
//
// Level of a box (levels > 1): torchvision's clamp(floor(canonical_level + log2(sqrt(area) / canonical_scale) + 1e-6),
//   k_min, k_max) - k_min, area = (x2 - x1)(y2 - y1) in fp32, k_min = k0 = -log2(scale[0]), without a transcendental: the
//   host computes the levels - 1 area thresholds (canonical_scale 2^(k0 + j - canonical_level - 1e-6))^2, j = 1.., in
//   double and passes them as floats; a box's level is the number of thresholds its area reaches.  Two deviations:
//     * an area that is <= 0 or NaN takes level 0 (torch's log2 of it is -Inf / NaN and the cast to an integer undefined);
//     * the thresholds can place a box on the other side than torch's fp32 log2 does only when its area lies within about
//       1e-6 relative of a threshold.
//
// Memory safety: every tap address is clamped into [0, h-1] x [0, w-1] of the box's own image by construction (low and
// high are built from a value already forced into [0, size]; the level is clamped to levels - 1 after the count).  A box
// whose batch index is not an integer in [0, N) (NaN included) reads nothing and gets zeros; otherwise a box with a
// non-finite coordinate reads nothing and gets NaN in its P x P x C outputs (the ring stays 0).  A wave writes the one
// output position it owns and nothing else.
//
// The kernel: one wave per output position (ring positions included: they store zeros) of one box; a lane owns four
// channels of a 256-channel slab (16 bytes per load and per store) and walks the slabs of a wider C.  The box, its level,
// and per axis the S samples' tap offsets and weights are wave-uniform: computed from the box's five values and moved
// to scalar registers (v_readfirstlane), so a lane holds only its loads and its sum.  All 4 S^2 loads of a position are
// issued before the first use for S <= 2 (16 loads, 64 registers); for S = 3, 4 the loads of one sample row (4 S) are,
// which keeps the kernel at four waves per SIMD.  Four waves per workgroup, no LDS, no MFMA, no atomics.
#include <cmath>

#include "wino_common.h"

namespace wino {
namespace {

constexpr int ROI_WAVES = 4;
constexpr int ROI_MAX_LEVELS = 4;
constexpr int ROI_MAX_P = 64;
constexpr int ROI_MAX_SAMPLING = 4;

struct RoiArgs {
  const float* f0;
  const float* f1;
  const float* f2;
  const float* f3;
  int h[ROI_MAX_LEVELS], w[ROI_MAX_LEVELS];
  float scale[ROI_MAX_LEVELS];
  float thr[ROI_MAX_LEVELS - 1];   // area thresholds of levels 1.., +Inf beyond the last level
  int levels, N, C, pad;           // pad: 1 when the level maps carry a ring
  int P, Q, ring;                  // Q = P + 2 ring: the stored extent
  FastDiv divQQ, divQ;
  unsigned tasks;                  // boxes of this launch x Q x Q
  const float* rois;               // this launch's first box
  float* out;                      // ... and its output
};

__device__ __forceinline__ int sgpr(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float sgpr(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// One sample coordinate along an axis of `size` pixels whose pixel stride is `stride` elements: the two taps' element
// offsets, their weights, and whether the sample is in range.  low and high lie in [0, size - 1] whatever v is.
struct Tap {
  unsigned lo, hi;
  float l, h;
  bool ok;
};
__device__ __forceinline__ Tap tap(float v, int size, unsigned stride) {
  Tap t;
  t.ok = v >= -1.f && v <= (float)size;          // (a NaN is out of range)
  float c = t.ok ? (v <= 0.f ? 0.f : v) : 0.f;   // in [0, size]
  int low = (int)c, high;
  if (low >= size - 1) {
    low = high = size - 1;
    c = (float)low;
  } else {
    high = low + 1;
  }
  t.l = sgpr(c - (float)low);
  t.h = sgpr(1.f - (c - (float)low));
  t.lo = (unsigned)sgpr(low) * stride;
  t.hi = (unsigned)sgpr(high) * stride;
  return t;
}

__device__ __forceinline__ f32x4 sample(f32x4 a, f32x4 b, f32x4 c, f32x4 d, const Tap& ty, const Tap& tx) {
  const float w1 = ty.h * tx.h, w2 = ty.h * tx.l, w3 = ty.l * tx.h, w4 = ty.l * tx.l;
  const f32x4 v = w1 * a + w2 * b + w3 * c + w4 * d;
  return (ty.ok && tx.ok) ? v : f32x4{0.f, 0.f, 0.f, 0.f};
}

template <int S>
__global__ __launch_bounds__(64 * ROI_WAVES, 4) void roi_align_kernel(const RoiArgs a) {
  const int lane = threadIdx.x & 63;
  const unsigned t = blockIdx.x * ROI_WAVES + (unsigned)sgpr((int)(threadIdx.x >> 6));
  if (t >= a.tasks) return;
  const unsigned r = fastdiv(t, a.divQQ), q = t - r * (unsigned)(a.Q * a.Q);
  const unsigned qy = fastdiv(q, a.divQ), qx = q - qy * (unsigned)a.Q;
  float* o = a.out + (size_t)r * ((size_t)a.Q * a.Q * a.C) + (size_t)q * a.C;   // 64-bit box base; q C < 2^31
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const int ph = (int)qy - a.ring, pw = (int)qx - a.ring;
  if (ph < 0 || ph >= a.P || pw < 0 || pw >= a.P) {   // a ring position
    for (int c = lane * 4; c < a.C; c += 256) *(f32x4*)(o + c) = zero;
    return;
  }
  const float* box = a.rois + (size_t)r * 5;
  const float bi = sgpr(box[0]), x1 = sgpr(box[1]), y1 = sgpr(box[2]), x2 = sgpr(box[3]), y2 = sgpr(box[4]);
  const bool image_ok = bi >= 0.f && bi < 2147483648.f && (int)bi < a.N && (float)(int)bi == bi;
  const bool finite = fabsf(x1) < INFINITY && fabsf(y1) < INFINITY && fabsf(x2) < INFINITY && fabsf(y2) < INFINITY;
  if (!image_ok || !finite) {   // reads nothing
    const float fill = image_ok ? NAN : 0.f;
    for (int c = lane * 4; c < a.C; c += 256) *(f32x4*)(o + c) = f32x4{fill, fill, fill, fill};
    return;
  }
  const float area = (x2 - x1) * (y2 - y1);
  int lvl = (area >= a.thr[0] ? 1 : 0) + (area >= a.thr[1] ? 1 : 0) + (area >= a.thr[2] ? 1 : 0);
  lvl = sgpr(lvl < a.levels - 1 ? lvl : a.levels - 1);   // (an area of +Inf reaches the +Inf of an unused threshold)
  const float* f = lvl == 0 ? a.f0 : lvl == 1 ? a.f1 : lvl == 2 ? a.f2 : a.f3;
  const int h = lvl == 0 ? a.h[0] : lvl == 1 ? a.h[1] : lvl == 2 ? a.h[2] : a.h[3];
  const int w = lvl == 0 ? a.w[0] : lvl == 1 ? a.w[1] : lvl == 2 ? a.w[2] : a.w[3];
  const float s = lvl == 0 ? a.scale[0] : lvl == 1 ? a.scale[1] : lvl == 2 ? a.scale[2] : a.scale[3];

  const float sx = x1 * s, sy = y1 * s, ex = x2 * s, ey = y2 * s;
  const float roi_w = fmaxf(ex - sx, 1.f), roi_h = fmaxf(ey - sy, 1.f);
  const float bin_w = roi_w / (float)a.P, bin_h = roi_h / (float)a.P;
  const unsigned RW = (unsigned)(w + 2 * a.pad);
  // the image's interior origin: one image of a level map is below 2^31 elements (checked by the entry point)
  f += ((size_t)(int)bi * (unsigned)(h + 2 * a.pad) * RW + (size_t)a.pad * (RW + 1)) * (unsigned)a.C;
  Tap tx[S];
#pragma unroll
  for (int i = 0; i < S; i++) tx[i] = tap(sx + (float)pw * bin_w + ((float)i + .5f) * bin_w / (float)S, w, (unsigned)a.C);
  constexpr int RB = S <= 2 ? S : 1;   // sample rows whose 4 S loads each are in flight together
  for (int c = lane * 4; c < a.C; c += 256) {
    const float* fc = f + c;
    f32x4 acc = zero;
#pragma unroll 1
    for (int y0 = 0; y0 < S; y0 += RB) {   // (a real loop: unrolled, the scheduler hoists every row's loads and spills)
      Tap ty[RB];
      f32x4 v[RB][S][4];
#pragma unroll
      for (int iy = 0; iy < RB; iy++) {
        ty[iy] = tap(sy + (float)ph * bin_h + ((float)(y0 + iy) + .5f) * bin_h / (float)S, h, RW * (unsigned)a.C);
#pragma unroll
        for (int ix = 0; ix < S; ix++) {
          v[iy][ix][0] = *(const f32x4*)(fc + (size_t)(ty[iy].lo + tx[ix].lo));
          v[iy][ix][1] = *(const f32x4*)(fc + (size_t)(ty[iy].lo + tx[ix].hi));
          v[iy][ix][2] = *(const f32x4*)(fc + (size_t)(ty[iy].hi + tx[ix].lo));
          v[iy][ix][3] = *(const f32x4*)(fc + (size_t)(ty[iy].hi + tx[ix].hi));
        }
      }
#pragma unroll
      for (int iy = 0; iy < RB; iy++)
#pragma unroll
        for (int ix = 0; ix < S; ix++)
          acc += sample(v[iy][ix][0], v[iy][ix][1], v[iy][ix][2], v[iy][ix][3], ty[iy], tx[ix]);
    }
    *(f32x4*)(o + c) = acc / (float)(S * S);
  }
}

// Boxes per launch: a launch's tasks (boxes x Q x Q) stay within 2^31 -- at least 493 k boxes, 2^31 at Q = 1 -- or within
// the developer knob WINO_ROI_LAUNCH_TASKS when that is positive (tests run the split loop with it); one box at least.
long roi_boxes_per_launch(unsigned QQ) {
  const int cap = knobs().roi_launch_tasks;
  const unsigned long long tasks = cap > 0 ? (unsigned long long)cap : 1ull << 31;
  const long n = (long)(tasks / QQ);
  return n > 0 ? n : 1;
}

template <int S>
void launch_roi(const RoiArgs& a, hipStream_t s) {
  const unsigned blocks = (a.tasks + ROI_WAVES - 1) / ROI_WAVES;
  hipLaunchKernelGGL(roi_align_kernel<S>, dim3(blocks), dim3(64 * ROI_WAVES), 0, s, a);
}

}  // namespace
}  // namespace wino

using namespace wino;

extern "C" int wino_roi_align_hw(const float* f0, const float* f1, const float* f2, const float* f3, const int* hw_host,
                                 const float* scale_host, int levels, int N, int C, int in_padded, const float* rois,
                                 int R, int P, int sampling, float canonical_scale, int canonical_level, float* out,
                                 int out_padded, wino_stream_t s) {
  if (levels < 1 || levels > ROI_MAX_LEVELS || N < 1 || C < 1 || (C % 4) != 0 || P < 1 || P > ROI_MAX_P || R < 0 ||
      sampling < 1 || sampling > ROI_MAX_SAMPLING || (in_padded != 0 && in_padded != 1) ||
      (out_padded != 0 && out_padded != 1)) {
    set_error("roi_align: unsupported shape levels=%d N=%d C=%d in_padded=%d R=%d P=%d sampling=%d out_padded=%d (need "
              "1 <= levels <= 4, N >= 1, C >= 1, C %% 4 == 0, 1 <= P <= 64, R >= 0, 1 <= sampling <= 4, in_padded and "
              "out_padded 0 or 1)", levels, N, C, in_padded, R, P, sampling, out_padded);
    return WINO_E_SHAPE;
  }
  if (R == 0) return WINO_OK;
  const float* f[ROI_MAX_LEVELS] = {f0, f1, f2, f3};
  if (int rc = check_nonnull(hw_host, scale_host, rois, out)) return rc;
  for (int l = 0; l < levels; l++)
    if (int rc = check_nonnull(f[l])) return rc;
  if (int rc = check_aligned16(rois, out)) return rc;
  for (int l = 0; l < levels; l++)
    if (int rc = check_aligned16(f[l])) return rc;
  const unsigned long long lim = 1ull << 31;
  const int Q = P + 2 * out_padded;
  const unsigned long long box_elems = (unsigned long long)Q * Q * C;
  if (box_elems >= lim) {
    set_error("roi_align: one box's output %dx%dx%d (P=%d C=%d) exceeds 32-bit offsets", Q, Q, C, P, C);
    return WINO_E_SHAPE;
  }
  size_t map_bytes[ROI_MAX_LEVELS];
  for (int l = 0; l < levels; l++) {
    const int h = hw_host[2 * l], w = hw_host[2 * l + 1];
    if (h < 1 || w < 1) {
      set_error("roi_align: unsupported shape h=%d w=%d of level %d (need h, w >= 1)", h, w, l);
      return WINO_E_SHAPE;
    }
    const unsigned long long pix = (unsigned long long)(h + 2ll * in_padded) * (unsigned long long)(w + 2ll * in_padded);
    if (pix >= lim || pix * C >= lim) {
      set_error("roi_align: one image of level %d, h=%d w=%d C=%d, exceeds 32-bit offsets", l, h, w, C);
      return WINO_E_SHAPE;
    }
    map_bytes[l] = (size_t)N * pix * C * sizeof(float);
  }
  int k0 = 0;
  for (int l = 0; l < levels; l++) {
    const float sc = scale_host[l];
    bool ok = std::isfinite(sc) && sc > 0.f;
    if (ok && levels > 1) {   // torchvision's LevelMapper: scale[l] = 2^-(k0 + l) exactly
      int e;
      ok = std::frexp(sc, &e) == 0.5f;
      if (l == 0) k0 = 1 - e;
      ok = ok && 1 - e == k0 + l;
    }
    if (!ok) {
      set_error("roi_align: scale_host[%d]=%g: need a finite positive scale%s", l, (double)sc,
                levels > 1 ? ", and with several levels exactly 2^-(k0+l) for an integer k0" : "");
      return WINO_E_ARG;
    }
  }
  if (!(std::isfinite(canonical_scale) && canonical_scale > 0.f)) {
    set_error("roi_align: canonical_scale=%g must be finite and positive", (double)canonical_scale);
    return WINO_E_ARG;
  }
  const size_t out_b = (size_t)R * box_elems * sizeof(float), rois_b = (size_t)R * 5 * sizeof(float);
  bool clash = overlaps(out, out_b, rois, rois_b);
  for (int l = 0; l < levels; l++) clash = clash || overlaps(out, out_b, f[l], map_bytes[l]);
  if (clash) {
    set_error("roi_align: out must not overlap a level map or rois");
    return WINO_E_ARG;
  }

  RoiArgs a;
  a.f0 = f0;
  a.f1 = levels > 1 ? f1 : f0;
  a.f2 = levels > 2 ? f2 : f0;
  a.f3 = levels > 3 ? f3 : f0;
  for (int l = 0; l < ROI_MAX_LEVELS; l++) {
    const int m = l < levels ? l : 0;   // (never selected: the level is clamped to levels - 1)
    a.h[l] = hw_host[2 * m];
    a.w[l] = hw_host[2 * m + 1];
    a.scale[l] = scale_host[m];
  }
  for (int j = 1; j < ROI_MAX_LEVELS; j++) {
    if (j < levels) {
      const double edge = (double)canonical_scale * std::exp2((double)(k0 + j - canonical_level) - 1e-6);
      a.thr[j - 1] = (float)(edge * edge);
    } else {
      a.thr[j - 1] = INFINITY;
    }
  }
  a.levels = levels, a.N = N, a.C = C, a.pad = in_padded;
  a.P = P, a.Q = Q, a.ring = out_padded;
  a.divQQ = make_fastdiv((unsigned)(Q * Q));
  a.divQ = make_fastdiv((unsigned)Q);
  const unsigned QQ = (unsigned)(Q * Q);
  const long per_launch = roi_boxes_per_launch(QQ);
  for (long r0 = 0; r0 < R; r0 += per_launch) {
    const long n = R - r0 < per_launch ? R - r0 : per_launch;
    a.tasks = (unsigned)(n * QQ);
    a.rois = rois + (size_t)r0 * 5;
    a.out = out + (size_t)r0 * box_elems;
    switch (sampling) {
      case 1: launch_roi<1>(a, (hipStream_t)s); break;
      case 2: launch_roi<2>(a, (hipStream_t)s); break;
      case 3: launch_roi<3>(a, (hipStream_t)s); break;
      default: launch_roi<4>(a, (hipStream_t)s); break;
    }
    if (int rc = launch_status("roi_align_kernel")) return rc;
  }
  return WINO_OK;
}

extern "C" int wino_roi_align_launches(int R, int P, int out_padded, long* launches) {
  if (R < 0 || P < 1 || P > ROI_MAX_P || (out_padded != 0 && out_padded != 1)) {
    set_error("roi_align_launches: unsupported shape R=%d P=%d out_padded=%d", R, P, out_padded);
    return WINO_E_SHAPE;
  }
  if (int rc = check_nonnull(launches)) return rc;
  const int Q = P + 2 * out_padded;
  const long per_launch = roi_boxes_per_launch((unsigned)(Q * Q));
  *launches = (R + per_launch - 1) / per_launch;
  return WINO_OK;
}
