// torchvision's GeneralizedRCNNTransform at test time -- normalise, resize, batch -- for N images of different sizes in
// one launch per 32 images, and the host-only size rule that goes with it.
//
// wino_image_transform_hw:  images i = [C][h_i][w_i] (fp32 or uint8, each at its own address) -> out [N][C][Hb][Wb] fp32:
//   plane (i, c) holds the normalised image i, channel c, resized to ho_i x wo_i, in its top-left corner and 0 elsewhere.
//   Every element of out is written by exactly one lane, so no memset precedes the launch.
//
// Arithmetic: a pixel is v (fp32) or float(byte) / 255.0f (uint8); the tap is t = (v - mean_c) * inv_c with inv_c =
// 1.0f / std_c computed on the host in fp32; the output is resize_coord.h's lerp2 of the four taps at its coord()s, all
// four always multiplied.  Normalise, then interpolate: torchvision's order.
//
// One form, a direct gather.  resize.hip stages because its layer is an NHWC -> NCHW transpose: without staging its
// loads would be 4 bytes out of every ld * 4.  Here source and output are both planes and neighbouring lanes read
// neighbouring (or, upscaling, equal) addresses of one source row.  The launch is not bound by its stores, though: a
// lane issues 16 gathers per 16-byte store, and measured it takes several times the fill of its output (DESIGN.md
// section 3.2q has the figures); staging the two source rows of an output row in LDS has not been tried.
//   A workgroup of four waves owns a tile of ROWS output rows x 256 output columns of one image, all C channels.
//   Wave v takes rows v, v + 4, ...: a row's y coordinate is wave-uniform.  A lane owns four consecutive x and computes
//   their coordinates once for all rows and channels.  Per row and channel it stores its four values with one 16-byte
//   store when the address allows it (a row of an odd Wb that starts off 16 bytes, or the last pixels of a row, go out
//   as 4-byte stores).  Outputs at x >= wo or y >= ho are 0 by a select, never by a multiplication; a tile wholly
//   outside ho x wo loads nothing.  uint8: the workgroup first fills a table t[c][byte] in LDS (C * 256 floats, one
//   division per entry), so a tap is a byte load and a table read and no tap is converted twice.
//   The image descriptors (pointer, h, w, ho, wo) and the C means and reciprocals travel by value in the kernel's
//   arguments: no workspace, no stream scratch, nothing to copy before the launch.
#include <cmath>

#include "resize_coord.h"
#include "wino_common.h"

namespace wino {
namespace {

constexpr int MAX_IMAGES = WINO_TRANSFORM_MAX_IMAGES;
constexpr int MAX_C = 4;
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int TILE_W = 4 * 64;   // four x per lane
constexpr int ROWS = 8;          // output rows of a tile: two per wave
constexpr unsigned long long MAX_TILES = (1ull << 32) / THREADS;   // tiles of one plane: the grid's x times THREADS < 2^32

struct ImageDesc {
  const void* p;
  int h, w, ho, wo;
};
struct TransformArgs {
  ImageDesc img[MAX_IMAGES];
  float mean[MAX_C], inv[MAX_C];
  float* out;   // plane (0, 0) of this launch's first image
  int C, Hb, Wb, xchunks;
};

__device__ __forceinline__ void store4(float* o, f32x4 v, int valid) {
  if (valid == 4 && (reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
    *(f32x4*)o = v;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (j < valid) o[j] = v[j];
  }
}

// grid.x = xchunks * row tiles, grid.y = the launch's images
template <bool U8>
__global__ __launch_bounds__(THREADS) void image_transform_kernel(const TransformArgs a) {
  __shared__ float table[U8 ? MAX_C * 256 : 1];
  const int tid = threadIdx.x;
  const int C = a.C, Hb = a.Hb, Wb = a.Wb;
  const ImageDesc im = a.img[blockIdx.y];
  const int xc = blockIdx.x % a.xchunks, rt = blockIdx.x / a.xchunks;
  const int x_first = xc * TILE_W, y_first = rt * ROWS;
  const int y_end = y_first + ROWS < Hb ? y_first + ROWS : Hb;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int x = x_first + 4 * lane;
  const int valid = x >= Wb ? 0 : (Wb - x < 4 ? Wb - x : 4);
  const size_t plane = (size_t)Hb * Wb;
  float* on = a.out + (size_t)blockIdx.y * C * plane;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  if (y_first >= im.ho || x_first >= im.wo) {   // the tile lies in the pad region
    if (valid == 0) return;
    for (int y = y_first + wave; y < y_end; y += WAVES)
      for (int c = 0; c < C; c++) store4(on + (size_t)c * plane + (size_t)y * Wb + x, zero, valid);
    return;
  }

  if constexpr (U8) {
    for (int c = 0; c < C; c++) table[c * 256 + tid] = ((float)tid / 255.0f - a.mean[c]) * a.inv[c];
    __syncthreads();
  }
  if (valid == 0) return;

  const int h = im.h, w = im.w, ho = im.ho, wo = im.wo;
  int c0[4], c1[4];
  float lx[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const Coord cx = coord(x + j < wo ? x + j : wo - 1, w, wo);   // (lanes past the image stay inside it)
    c0[j] = cx.i0;
    c1[j] = cx.i1;
    lx[j] = cx.lam;
  }
  const size_t src_plane = (size_t)h * w;
  for (int y = y_first + wave; y < y_end; y += WAVES) {
    float* orow = on + (size_t)y * Wb + x;
    if (y >= ho) {   // wave-uniform
      for (int c = 0; c < C; c++) store4(orow + (size_t)c * plane, zero, valid);
      continue;
    }
    const Coord cy = coord(y, h, ho);
    const size_t r0 = (size_t)cy.i0 * w, r1 = (size_t)cy.i1 * w;
#pragma unroll 1
    for (int c = 0; c < C; c++) {
      f32x4 v;
      if constexpr (U8) {
        const unsigned char* p0 = (const unsigned char*)im.p + (size_t)c * src_plane + r0;
        const unsigned char* p1 = (const unsigned char*)im.p + (size_t)c * src_plane + r1;
        const float* t = table + c * 256;
#pragma unroll
        for (int j = 0; j < 4; j++)
          v[j] = lerp2(t[p0[c0[j]]], t[p0[c1[j]]], t[p1[c0[j]]], t[p1[c1[j]]], lx[j], cy.lam);
      } else {
        const float* p0 = (const float*)im.p + (size_t)c * src_plane + r0;
        const float* p1 = (const float*)im.p + (size_t)c * src_plane + r1;
        const float m = a.mean[c], s = a.inv[c];
#pragma unroll
        for (int j = 0; j < 4; j++)
          v[j] = lerp2((p0[c0[j]] - m) * s, (p0[c1[j]] - m) * s, (p1[c0[j]] - m) * s, (p1[c1[j]] - m) * s, lx[j], cy.lam);
      }
#pragma unroll
      for (int j = 0; j < 4; j++) v[j] = x + j < wo ? v[j] : 0.f;
      store4(orow + (size_t)c * plane, v, valid);
    }
  }
}

}  // namespace
}  // namespace wino

using namespace wino;

extern "C" {

int wino_transform_size(int h, int w, int min_size, int max_size, int* ho, int* wo) {
  if (int rc = check_nonnull(ho, wo)) return rc;
  if (h < 1 || w < 1 || min_size < 1 || max_size < 1) {
    set_error("transform_size: unsupported shape h=%d w=%d min_size=%d max_size=%d (need all four >= 1)", h, w, min_size,
              max_size);
    return WINO_E_SHAPE;
  }
  // torch: `float / tensor` is reciprocal(tensor) * float, both in fp32
  const float r_min = 1.0f / (float)(h < w ? h : w), r_max = 1.0f / (float)(h < w ? w : h);
  const float s_min = r_min * (float)min_size, s_max = r_max * (float)max_size;
  const double s = (double)(s_min < s_max ? s_min : s_max);
  const double fh = std::floor((double)h * s), fw = std::floor((double)w * s);
  if (fh < 1.0 || fw < 1.0 || fh >= 2147483648.0 || fw >= 2147483648.0) {
    set_error("transform_size: %dx%d at scale %g resizes to %.0fx%.0f (need 1 <= both < 2^31)", h, w, s, fh, fw);
    return WINO_E_SHAPE;
  }
  *ho = (int)fh;
  *wo = (int)fw;
  return WINO_OK;
}

int wino_image_transform_hw(const void* const* images_host, const int* hw_host, const int* out_hw_host, int N, int C,
                            int dtype, const float* mean_host, const float* std_host, float* out, int Hb, int Wb,
                            wino_stream_t s) {
  if (N < 0 || C < 1 || C > MAX_C || Hb < 1 || Wb < 1) {
    set_error("image_transform: unsupported shape N=%d C=%d Hb=%d Wb=%d (need N >= 0, 1 <= C <= 4, Hb, Wb >= 1)", N, C, Hb,
              Wb);
    return WINO_E_SHAPE;
  }
  if (dtype != WINO_IMAGE_F32 && dtype != WINO_IMAGE_U8) {
    set_error("image_transform: dtype=%d is neither WINO_IMAGE_F32 nor WINO_IMAGE_U8", dtype);
    return WINO_E_ARG;
  }
  if (N == 0) return WINO_OK;
  if (int rc = check_nonnull(images_host, hw_host, out_hw_host, mean_host, std_host)) return rc;
  if (int rc = check_nonnull(out)) return rc;
  if (int rc = check_aligned16(out)) return rc;
  for (int c = 0; c < C; c++) {
    // (1 / std must be finite too: a denormal std's reciprocal is not)
    if (!std::isfinite(mean_host[c]) || !std::isfinite(std_host[c]) || std_host[c] == 0.f ||
        !std::isfinite(1.0f / std_host[c])) {
      set_error("image_transform: mean[%d]=%g std[%d]=%g: need a finite mean and a finite non-zero std with a finite "
                "reciprocal", c, (double)mean_host[c], c, (double)std_host[c]);
      return WINO_E_ARG;
    }
  }
  const unsigned long long lim = 1ull << 31;
  const unsigned long long out_image = (unsigned long long)Hb * Wb * C;
  if (out_image >= lim) {
    set_error("image_transform: one image of out %dx%dx%d exceeds 32-bit offsets", C, Hb, Wb);
    return WINO_E_SHAPE;
  }
  // the grid's x: tiles * 256 threads must stay below 2^32
  const unsigned long long tiles64 = (unsigned long long)((Wb + TILE_W - 1) / TILE_W) * (unsigned long long)((Hb + ROWS - 1) / ROWS);
  if (tiles64 >= MAX_TILES) {
    set_error("image_transform: a plane of %dx%d is %llu tiles of %d rows x %d columns, one launch takes fewer than %llu",
              Hb, Wb, tiles64, ROWS, TILE_W, MAX_TILES);
    return WINO_E_SHAPE;
  }
  const size_t px = dtype == WINO_IMAGE_U8 ? 1 : sizeof(float);
  const size_t out_b = (size_t)N * out_image * sizeof(float);
  for (int i = 0; i < N; i++) {
    const int h = hw_host[2 * i], w = hw_host[2 * i + 1], ho = out_hw_host[2 * i], wo = out_hw_host[2 * i + 1];
    if (h < 1 || w < 1 || ho < 1 || wo < 1) {
      set_error("image_transform: image %d: unsupported shape h=%d w=%d ho=%d wo=%d (need all four >= 1)", i, h, w, ho, wo);
      return WINO_E_SHAPE;
    }
    if (ho > Hb || wo > Wb) {
      set_error("image_transform: image %d resizes to %dx%d, the batch is %dx%d", i, ho, wo, Hb, Wb);
      return WINO_E_SHAPE;
    }
    if (2ull * ho * h >= lim || 2ull * wo * w >= lim) {
      set_error("image_transform: image %d: 2*ho*h = %llu or 2*wo*w = %llu is not below 2^31", i, 2ull * ho * h,
                2ull * wo * w);
      return WINO_E_SHAPE;
    }
    const unsigned long long in_image = (unsigned long long)h * w * C;
    if (in_image >= lim) {
      set_error("image_transform: image %d, %dx%dx%d, exceeds 32-bit offsets", i, C, h, w);
      return WINO_E_SHAPE;
    }
    const void* p = images_host[i];
    if (!p) {
      set_error("NULL pointer (image %d)", i);
      return WINO_E_ARG;
    }
    if (dtype == WINO_IMAGE_F32 && (reinterpret_cast<uintptr_t>(p) & 3u)) {
      set_error("image_transform: image %d: a float image must be 4-byte aligned", i);
      return WINO_E_ARG;
    }
    if (overlaps(p, (size_t)in_image * px, out, out_b)) {
      set_error("image_transform: out must not overlap image %d", i);
      return WINO_E_ARG;
    }
  }

  TransformArgs a;
  for (int c = 0; c < MAX_C; c++) {
    a.mean[c] = c < C ? mean_host[c] : 0.f;
    a.inv[c] = c < C ? 1.0f / std_host[c] : 1.f;
  }
  a.C = C, a.Hb = Hb, a.Wb = Wb;
  a.xchunks = (Wb + TILE_W - 1) / TILE_W;
  const unsigned tiles = (unsigned)tiles64;
  for (int n0 = 0; n0 < N; n0 += MAX_IMAGES) {
    const int n = N - n0 < MAX_IMAGES ? N - n0 : MAX_IMAGES;
    for (int i = 0; i < MAX_IMAGES; i++) {
      const int k = n0 + (i < n ? i : 0);   // (slots past n are never indexed: the grid's y stops at n)
      a.img[i] = {images_host[k], hw_host[2 * k], hw_host[2 * k + 1], out_hw_host[2 * k], out_hw_host[2 * k + 1]};
    }
    a.out = out + (size_t)n0 * out_image;
    if (dtype == WINO_IMAGE_U8) {
      hipLaunchKernelGGL(image_transform_kernel<true>, dim3(tiles, (unsigned)n), dim3(THREADS), 0, (hipStream_t)s, a);
    } else {
      hipLaunchKernelGGL(image_transform_kernel<false>, dim3(tiles, (unsigned)n), dim3(THREADS), 0, (hipStream_t)s, a);
    }
    if (int rc = launch_status("image_transform_kernel")) return rc;
  }
  return WINO_OK;
}

}  // extern "C"
