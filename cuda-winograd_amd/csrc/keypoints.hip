// Keypoint R-CNN's output stage: torchvision's heatmaps_to_keypoints (a Python loop over detections with a host read of
// each box size, a [K][h][w] bicubic resize per detection and an argmax over it) for all detections in one launch.
//
// wino_keypoints_hw: for every (r, k), resize heatmap plane (r, k) (M x M) to the box of detection r (hc x wc) with
//   torch's bicubic and write the argmax as a keypoint in image coordinates, with its value as the score.
//   maps     PLANES:      [R][K][M][M], torchvision's keypoint logits
//            DECONV_ROWS: [R P P][ld], M = 4 P: the partial products of ConvTranspose2d(C, K, 4, stride 2, padding 1), row
//                         (r, iy, ix), column (ky 4 + kx) K + k.  low[oy][ox] (2P x 2P) = the at most four elements with
//                         ky = (oy + 1) mod 2 (+ 2), iy = (oy + 1 - ky) / 2 in [0, P), likewise x, summed in ascending
//                         (ky, kx), + bias[k] last; plane = low upsampled x2 with coord(d, 2P, 4P) and lerp2
//                         (resize_coord.h): torch's interpolate(scale_factor=2, bilinear, align_corners=False)
//   rois     [R][5] = (n, x1, y1, x2, y2).  !(n >= 0), a padding row: the row's outputs are 0 and nothing else is read
//   box      w = max(x2 - x1, 1), wc = (int) ceil(w), cw = w / wc, likewise h, in fp32 and uncontracted.  A coordinate
//            that is not finite, or wc or hc above max_side: NaN in the row's outputs, no map read (named deviation)
//   resize   per axis (in = M, out = wc or hc), exact integers, NOT clamped at 0: num = (2 d + 1) M - out, i =
//            floor_div(num, 2 out), t = float(num - i 2 out) / float(2 out); taps i - 1 .. i + 2, each clamped into
//            [0, M), with torch's cubic convolution coefficients at A = -0.75; all 16 taps always multiplied
//   argmax   torch.argmax's rules over the hc x wc values: a NaN is the greatest value, among equal values the lowest
//            flat index pos = y wc + x wins
//   out      keypoints[r][k] = ((x_i + 0.5) cw + x1, (y_i + 0.5) ch + y1, 1), scores[r][k] = the value at pos
//
// One workgroup of four waves per (r, k).  The plane is staged in LDS once (16 KB static; DECONV_ROWS gathers the 2P x 2P
// map into 4 KB first and upsamples from there).  Wave v owns output rows v, v + 4, ...: it blends the row's four source
// rows into one M-wide row of its own in LDS (4 multiply-adds per source column, a lane per column), then its lanes
// walk x with the 4-tap horizontal sum, each keeping a running (value, flat index).  Lanes see their indices in
// ascending order, so a later value wins only when it is greater.  A wave reduction and one LDS step pick the winner.
// The hc x wc map is never stored: no workspace and no stream scratch.
#include <cmath>

#include "resize_coord.h"
#include "wino_common.h"

#pragma clang fp contract(off)   // torch's box arithmetic operation by operation

namespace wino {
namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_M = 64;
constexpr int MAX_P = 16;
constexpr int MAX_SIDE = 16384;
constexpr long long MAX_BLOCKS = 1ll << 22;   // workgroups per launch (HIP takes fewer than 2^32 threads along x)

struct KpArgs {
  const float* maps;
  const float* bias;
  const float* rois;
  float* keypoints;
  float* scores;
  long long first;   // the launch's first (r, k) pair
  int K, M, ld, layout, max_side;
};

// the best value so far under torch.argmax's order
struct Best {
  float v;
  int i;
};
__device__ __forceinline__ bool better(float v, int i, const Best& b) {
  const bool vn = v != v, bn = b.v != b.v;
  if (vn) return !bn || i < b.i;
  return !bn && (v > b.v || (v == b.v && i < b.i));
}

__global__ __launch_bounds__(THREADS) void keypoints_kernel(const KpArgs a) {
  __shared__ float plane[MAX_M * MAX_M];
  __shared__ float low[4 * MAX_P * MAX_P];
  __shared__ float rowbuf[WAVES][MAX_M];
  __shared__ float red_v[WAVES];
  __shared__ int red_i[WAVES];
  const int tid = threadIdx.x;
  const long long pair = a.first + blockIdx.x;
  const long long r = pair / a.K;
  const int k = (int)(pair - r * a.K);
  float* const kp = a.keypoints + (size_t)pair * 3;
  float* const sc = a.scores + (size_t)pair;
  const float* const roi = a.rois + (size_t)r * 5;

  // ---- the row's box: the same for every thread
  if (!(roi[0] >= 0.f)) {
    if (tid == 0) kp[0] = 0.f, kp[1] = 0.f, kp[2] = 0.f, sc[0] = 0.f;
    return;
  }
  const float x1 = roi[1], y1 = roi[2], x2 = roi[3], y2 = roi[4];
  const bool finite = fabsf(x1) < INFINITY && fabsf(y1) < INFINITY && fabsf(x2) < INFINITY && fabsf(y2) < INFINITY;
  float w = x2 - x1, h = y2 - y1;
  w = w > 1.f ? w : 1.f;
  h = h > 1.f ? h : 1.f;
  const float side = (float)a.max_side;
  if (!finite || !(w <= side) || !(h <= side)) {   // (ceil(w) > max_side exactly when w > max_side)
    const float nan = __builtin_nanf("");
    if (tid == 0) kp[0] = nan, kp[1] = nan, kp[2] = nan, sc[0] = nan;
    return;
  }
  const int wc = (int)ceilf(w), hc = (int)ceilf(h);
  const float cw = w / (float)wc, ch = h / (float)hc;

  // ---- the M x M plane into LDS
  const int M = a.M;
  if (a.layout == WINO_KP_LAYOUT_PLANES) {
    const float* const src = a.maps + (size_t)pair * M * M;
    for (int u = tid; u < M * M; u += THREADS) plane[u] = src[u];
  } else {
    const int P = M >> 2, L = 2 * P;
    const float b = a.bias[k];
    for (int u = tid; u < L * L; u += THREADS) {
      const int oy = u / L, ox = u - oy * L;
      float acc = 0.f;
#pragma unroll
      for (int jy = 0; jy < 2; jy++) {
        const int ky = ((oy + 1) & 1) + 2 * jy, iy2 = oy + 1 - ky;   // iy2 = 2 iy, even
#pragma unroll
        for (int jx = 0; jx < 2; jx++) {
          const int kx = ((ox + 1) & 1) + 2 * jx, ix2 = ox + 1 - kx;
          if (iy2 >= 0 && iy2 < 2 * P && ix2 >= 0 && ix2 < 2 * P) {
            const size_t row = ((size_t)r * P + (iy2 >> 1)) * P + (ix2 >> 1);
            acc += a.maps[row * (size_t)a.ld + (size_t)(ky * 4 + kx) * a.K + k];
          }
        }
      }
      low[u] = acc + b;
    }
    __syncthreads();
    for (int u = tid; u < M * M; u += THREADS) {
      const int Y = u / M, X = u - Y * M;
      const Coord cy = coord(Y, L, M), cx = coord(X, L, M);
      plane[u] = lerp2(low[cy.i0 * L + cx.i0], low[cy.i0 * L + cx.i1], low[cy.i1 * L + cx.i0], low[cy.i1 * L + cx.i1], cx.lam,
                       cy.lam);
    }
  }
  __syncthreads();

  // ---- the resize and the running argmax: wave v takes rows v, v + 4, ...; the trip count is the workgroup's
  const int lane = tid & 63, wave = tid >> 6;
  Best best;
  best.v = -INFINITY, best.i = 0x7fffffff;
  float* const mine = rowbuf[wave];
  for (int y0 = 0; y0 < hc; y0 += WAVES) {
    const int y = y0 + wave;
    const bool live = y < hc;
    if (live && lane < M) {
      const Cubic cy = cubic(y, M, hc);
      mine[lane] = cy.c[0] * plane[clampi(cy.i - 1, M) * M + lane] + cy.c[1] * plane[clampi(cy.i, M) * M + lane] +
                   cy.c[2] * plane[clampi(cy.i + 1, M) * M + lane] + cy.c[3] * plane[clampi(cy.i + 2, M) * M + lane];
    }
    __syncthreads();
    if (live) {
      const int base = y * wc;
      for (int x = lane; x < wc; x += 64) {
        const Cubic cx = cubic(x, M, wc);
        const float v = cx.c[0] * mine[clampi(cx.i - 1, M)] + cx.c[1] * mine[clampi(cx.i, M)] +
                        cx.c[2] * mine[clampi(cx.i + 1, M)] + cx.c[3] * mine[clampi(cx.i + 2, M)];
        if (better(v, base + x, best)) best.v = v, best.i = base + x;
      }
    }
    __syncthreads();   // (the next blend overwrites the row)
  }

  // ---- the winner: across the wave, then across the four waves
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best.v, off, 64);
    const int oi = __shfl_xor(best.i, off, 64);
    if (better(ov, oi, best)) best.v = ov, best.i = oi;
  }
  if (lane == 0) red_v[wave] = best.v, red_i[wave] = best.i;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int v = 1; v < WAVES; v++)
      if (better(red_v[v], red_i[v], best)) best.v = red_v[v], best.i = red_i[v];
    const int yi = best.i / wc, xi = best.i - yi * wc;
    kp[0] = ((float)xi + 0.5f) * cw + x1;
    kp[1] = ((float)yi + 0.5f) * ch + y1;
    kp[2] = 1.f;
    sc[0] = best.v;
  }
}

}  // namespace
}  // namespace wino

using namespace wino;

extern "C" int wino_keypoints_hw(const float* maps, int layout, const float* bias, const float* rois, int R, int K, int M,
                                 int ld, int max_side, float* keypoints, float* scores, wino_stream_t s) {
  if (layout != WINO_KP_LAYOUT_PLANES && layout != WINO_KP_LAYOUT_DECONV_ROWS) {
    set_error("keypoints: layout=%d is neither WINO_KP_LAYOUT_PLANES nor WINO_KP_LAYOUT_DECONV_ROWS", layout);
    return WINO_E_ARG;
  }
  const bool rows = layout == WINO_KP_LAYOUT_DECONV_ROWS;
  if (R < 0 || K < 1 || M < 1 || M > MAX_M || max_side < 1 || max_side > MAX_SIDE ||
      (rows && ((M & 3) || (long long)16 * K > ld))) {
    set_error("keypoints: unsupported shape R=%d K=%d M=%d ld=%d max_side=%d (need R >= 0, K >= 1, 1 <= M <= %d, "
              "1 <= max_side <= %d; DECONV_ROWS: M = 4 P with 1 <= P <= %d, 16 K <= ld)", R, K, M, ld, max_side, MAX_M,
              MAX_SIDE, MAX_P);
    return WINO_E_SHAPE;
  }
  if (R == 0) return WINO_OK;
  if (int rc = check_nonnull(maps, rois, keypoints, scores)) return rc;
  if (rows ? !bias : bias != nullptr) {
    set_error("keypoints: bias is required in the DECONV_ROWS layout and must be NULL in the PLANES layout");
    return WINO_E_ARG;
  }
  if (int rc = check_aligned16(maps, bias, rois, keypoints, scores)) return rc;
  const size_t P = (size_t)M >> 2;
  const size_t maps_b = (rows ? (size_t)R * P * P * (size_t)ld : (size_t)R * K * M * M) * sizeof(float);
  const size_t kp_b = (size_t)R * K * 3 * sizeof(float), sc_b = (size_t)R * K * sizeof(float);
  const std::pair<const void*, size_t> ins[3] = {
      {maps, maps_b}, {rois, (size_t)R * 5 * sizeof(float)}, {bias, bias ? (size_t)K * sizeof(float) : 0}};
  bool clash = overlaps(keypoints, kp_b, scores, sc_b);
  for (const auto& in : ins)
    clash = clash || (in.second && (overlaps(keypoints, kp_b, in.first, in.second) || overlaps(scores, sc_b, in.first, in.second)));
  if (clash) {
    set_error("keypoints: keypoints and scores must not overlap maps, bias, rois or each other");
    return WINO_E_ARG;
  }
  KpArgs a;
  a.maps = maps, a.bias = bias, a.rois = rois, a.keypoints = keypoints, a.scores = scores;
  a.K = K, a.M = M, a.ld = ld, a.layout = layout, a.max_side = max_side;
  const long long pairs = (long long)R * K;
  for (a.first = 0; a.first < pairs; a.first += MAX_BLOCKS) {
    const long long nb = pairs - a.first < MAX_BLOCKS ? pairs - a.first : MAX_BLOCKS;
    hipLaunchKernelGGL(keypoints_kernel, dim3((unsigned)nb), dim3(THREADS), 0, (hipStream_t)s, a);
    if (int rc = launch_status("keypoints_kernel")) return rc;
  }
  return WINO_OK;
}
