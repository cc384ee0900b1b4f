// The two memory-bound kernels a torchvision VGG needs around its 3x3 layers.
//
// wino_image_pack_hw:  x [N][Cin][H][W] (NCHW) -> out [N][H+2][W+2][Cpad], channels Cin .. Cpad-1 and the ring 0.
//   One lane per 16-byte unit of the output (4 channels of one padded pixel), units in memory order: the stores are
//   whole coalesced lines; the loads are 4-byte, consecutive lanes Cpad/4 apart on a row of x -- every line of x is
//   read once from memory and Cpad/4 - 1 times from cache.  Each workgroup row (blockIdx.y) is one image, re-based
//   in 64 bits; inside an image offsets are 32-bit.
//
// wino_avgpool7_flatten_hw:  feat [N][H(+2)][W(+2)][C] -> out [N][49*C] in (h, w, c) order, torch's
//   AdaptiveAvgPool2d((7, 7)) + flatten with the channel innermost: bin (i, j) is the mean over rows
//   floor(i*H/7) .. ceil((i+1)*H/7) - 1 and the same for columns.  One lane per (bin, 4 channels): 16-byte loads along
//   the channels, 16-byte stores.  The sum runs row by row in f32 and is divided by the bin's pixel count.
#include "wino_common.h"

namespace wino {
namespace {

__global__ __launch_bounds__(256) void image_pack_kernel(const float* __restrict__ x, float* __restrict__ out, int Cin,
                                                         int H, int W, int Cpad) {
  const int upp = Cpad >> 2;                               // 16-byte units per pixel
  const int Wp = W + 2;
  const unsigned units = (unsigned)(H + 2) * Wp * upp;    // per image
  const float* xn = x + (size_t)blockIdx.y * Cin * H * W;
  float* on = out + (size_t)blockIdx.y * units * 4;
  for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < units; u += gridDim.x * 256u) {
    const unsigned pix = u / upp, unit = u - pix * upp;
    const int py = (int)(pix / Wp), px = (int)(pix - py * Wp);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (py >= 1 && py <= H && px >= 1 && px <= W) {
      const unsigned sp = (unsigned)(py - 1) * W + (px - 1), hw = (unsigned)H * W;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int c = (int)unit * 4 + i;
        if (c < Cin) v[i] = xn[c * hw + sp];
      }
    }
    *(f32x4*)(on + (size_t)u * 4) = v;
  }
}

__global__ __launch_bounds__(256) void avgpool7_flatten_kernel(const float* __restrict__ feat, float* __restrict__ out,
                                                               int H, int W, int C, int pad) {
  const int upp = C >> 2;
  const unsigned units = 49u * upp;                       // per image
  const int RW = W + 2 * pad;
  const float* fn = feat + (size_t)blockIdx.y * (H + 2 * pad) * RW * C;
  float* on = out + (size_t)blockIdx.y * units * 4;
  for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < units; u += gridDim.x * 256u) {
    const unsigned bin = u / upp, unit = u - bin * upp;
    const int bi = (int)(bin / 7), bj = (int)(bin - bi * 7);
    const int y0 = (int)(((long)bi * H) / 7), y1 = (int)(((long)(bi + 1) * H + 6) / 7);
    const int x0 = (int)(((long)bj * W) / 7), x1 = (int)(((long)(bj + 1) * W + 6) / 7);
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
    for (int y = y0; y < y1; y++) {
      const float* row = fn + ((size_t)(y + pad) * RW + pad) * C + unit * 4;
      for (int xx = x0; xx < x1; xx++) sum += *(const f32x4*)(row + (size_t)xx * C);
    }
    const float cnt = (float)((y1 - y0) * (x1 - x0));
    *(f32x4*)(on + (size_t)u * 4) = sum / cnt;
  }
}

// blocks along x for `units` 16-byte units per image: enough to cover them once, at most 1024 (grid-stride beyond)
unsigned blocks_for(unsigned long long units) {
  const unsigned long long b = (units + 255) / 256;
  return (unsigned)(b < 1 ? 1 : b > 1024 ? 1024 : b);
}

}  // namespace
}  // namespace wino

using namespace wino;

extern "C" {

int wino_image_pack_hw(const float* x, float* out, int N, int Cin, int H, int W, int Cpad, wino_stream_t s) {
  if (int rc = check_nonnull(x, out)) return rc;
  if (int rc = check_aligned16(x, out)) return rc;
  if (N < 1 || H < 1 || W < 1 || Cin < 1 || Cpad < 8 || (Cpad % 8) != 0 || Cin > Cpad) {
    set_error("image pack: unsupported shape N=%d Cin=%d H=%d W=%d Cpad=%d (need N, H, W >= 1, 1 <= Cin <= Cpad, "
              "Cpad %% 8 == 0)", N, Cin, H, W, Cpad);
    return WINO_E_SHAPE;
  }
  const unsigned long long img_in = (unsigned long long)Cin * H * W;
  const unsigned long long img_out = (unsigned long long)(H + 2) * (W + 2) * Cpad;
  if (img_in >= (1ull << 31) || img_out >= (1ull << 31)) {
    set_error("image pack: one image of %dx%d (or its padded output) exceeds 32-bit offsets", H, W);
    return WINO_E_SHAPE;
  }
  if (overlaps(x, (size_t)N * img_in * sizeof(float), out, (size_t)N * img_out * sizeof(float))) {
    set_error("x and out must not overlap");
    return WINO_E_ARG;
  }
  for (int n0 = 0; n0 < N; n0 += 65535) {   // gridDim.y
    const int n = N - n0 < 65535 ? N - n0 : 65535;
    hipLaunchKernelGGL(image_pack_kernel, dim3(blocks_for(img_out / 4), (unsigned)n), dim3(256), 0, (hipStream_t)s,
                       x + (size_t)n0 * img_in, out + (size_t)n0 * img_out, Cin, H, W, Cpad);
    if (int rc = launch_status("image_pack_kernel")) return rc;
  }
  return WINO_OK;
}

int wino_avgpool7_flatten_hw(const float* feat, float* out, int N, int H, int W, int C, int in_padded,
                             wino_stream_t s) {
  if (int rc = check_nonnull(feat, out)) return rc;
  if (int rc = check_aligned16(feat, out)) return rc;
  if (N < 1 || H < 1 || W < 1 || C < 4 || (C % 4) != 0 || (in_padded != 0 && in_padded != 1)) {
    set_error("avgpool7: unsupported shape N=%d H=%d W=%d C=%d in_padded=%d (need N, H, W >= 1, C %% 4 == 0, "
              "in_padded 0 or 1)", N, H, W, C, in_padded);
    return WINO_E_SHAPE;
  }
  const unsigned long long img_in = (unsigned long long)(H + 2 * in_padded) * (W + 2 * in_padded) * C;
  const unsigned long long img_out = 49ull * C;
  if (img_in >= (1ull << 31) || img_out >= (1ull << 31) || (long)H * W >= (1l << 24)) {
    set_error("avgpool7: shape H=%d W=%d C=%d out of range", H, W, C);
    return WINO_E_SHAPE;
  }
  if (overlaps(feat, (size_t)N * img_in * sizeof(float), out, (size_t)N * img_out * sizeof(float))) {
    set_error("feat and out must not overlap");
    return WINO_E_ARG;
  }
  for (int n0 = 0; n0 < N; n0 += 65535) {
    const int n = N - n0 < 65535 ? N - n0 : 65535;
    hipLaunchKernelGGL(avgpool7_flatten_kernel, dim3(blocks_for(img_out / 4), (unsigned)n), dim3(256), 0,
                       (hipStream_t)s, feat + (size_t)n0 * img_in, out + (size_t)n0 * img_out, H, W, C, in_padded);
    if (int rc = launch_status("avgpool7_flatten_kernel")) return rc;
  }
  return WINO_OK;
}

}  // extern "C"
