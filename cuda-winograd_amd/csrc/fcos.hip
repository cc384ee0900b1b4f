// FCOS's two kernels beside the select: the score map and the decode of the selected locations.  Plain HIP: no MFMA, no
// inline assembly, no LDS, no scratch, no hand-off between workgroups; both entry points own no state and can be
// captured into a graph as they are.
//
// wino_fcos_score_map_hw: in place on the class-logit map [N][h+2][w+2][ld_c]: interior columns < K become
//   sqrt(sigmoid(logit) * sigmoid(ctr)),  ctr = column ctr_col of the same pixel of the regression map [N][h+2][w+2][ld_r],
//   sigmoid(v) = 1 / (1 + exp(-v)) in fp32, as torch computes the score of a location.  One thread per (pixel, quad of
//   four columns): a 16-byte load and store for a quad below K, single columns for the K % 4 of the last, so that no pad
//   column and no ring pixel is read or written; the threads of a pixel read the same centerness word.  A NaN logit or
//   centerness gives NaN; a product that underflows gives 0 (torch's fp32 does the same).
//
// wino_fcos_decode_hw: decode_rows.h's rows with the anchor-free box of torchvision's
//   BoxLinearCoder(normalize_by_size=True).decode on max(columns, 0), operation by operation in fp32, clipped to the image.
#include "decode_rows.h"

#pragma clang fp contract(off)

namespace wino {
namespace {

struct ScoreArgs {
  float* cls;
  const float* reg;
  unsigned total;             // N h w qk threads
  unsigned K, qk, w, hw;      // qk = ceil(K / 4)
  unsigned ld_c, ld_r, pitch_c, pitch_r, ctr_col;
  long long image_c, image_r;
  FastDiv divqk, divhw, divw;
};

__device__ __forceinline__ float sigmoidf(float v) { return 1.0f / (1.0f + expf(-v)); }

__global__ __launch_bounds__(256) void fcos_score_kernel(const ScoreArgs a) {
  const unsigned t = blockIdx.x * 256u + threadIdx.x;
  if (t >= a.total) return;
  const unsigned pix = fastdiv(t, a.divqk), quad = t - pix * a.qk;
  const unsigned n = fastdiv(pix, a.divhw), rem = pix - n * a.hw;
  const unsigned y = fastdiv(rem, a.divw), x = rem - y * a.w;
  const float ctr = a.reg[(size_t)n * (size_t)a.image_r + (size_t)(y + 1u) * a.pitch_r + (size_t)(x + 1u) * a.ld_r + a.ctr_col];
  const float sc = sigmoidf(ctr);
  float* p = a.cls + (size_t)n * (size_t)a.image_c + (size_t)(y + 1u) * a.pitch_c + (size_t)(x + 1u) * a.ld_c + 4u * quad;
  if (4u * quad + 4u <= a.K) {
    const f32x4 v = *(const f32x4*)p;
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; j++) r[j] = sqrtf(sigmoidf(v[j]) * sc);
    *(f32x4*)p = r;
  } else {
    for (unsigned j = 0; 4u * quad + j < a.K; j++) p[j] = sqrtf(sigmoidf(p[j]) * sc);
  }
}

__device__ __forceinline__ f32x4 fcos_box(f32x4 anc, float d0, float d1, float d2, float d3, float Himg, float Wimg) {
  const float l = relu_nan(d0), t = relu_nan(d1), r = relu_nan(d2), b = relu_nan(d3);
  const float cx = 0.5f * (anc.x + anc.z), cy = 0.5f * (anc.y + anc.w);
  const float aw = anc.z - anc.x, ah = anc.w - anc.y;
  const float x1 = cx - l * aw, y1 = cy - t * ah, x2 = cx + r * aw, y2 = cy + b * ah;
  return f32x4{clip_nan(x1, Wimg), clip_nan(y1, Himg), clip_nan(x2, Wimg), clip_nan(y2, Himg)};
}

__global__ __launch_bounds__(256) void fcos_decode_kernel(const DecodeRowsArgs a) { decode_row(a, fcos_box); }

// pitch and image elements of a padded map; false: past the limits
bool map_extent(int h, int w, int ld, unsigned* pitch, long long* image) {
  const unsigned long long p = (unsigned long long)(w + 2ll) * (unsigned long long)ld;
  if (p >= (1ull << 32)) return false;
  const unsigned long long im = (unsigned long long)(h + 2ll) * p;
  if (im >= (1ull << 40)) return false;
  *pitch = (unsigned)p, *image = (long long)im;
  return true;
}

}  // namespace
}  // namespace wino

using namespace wino;

extern "C" int wino_fcos_score_map_hw(float* cls, const float* reg, int N, int h, int w, int K, int ld_c, int ld_r, int ctr_col,
                                      wino_stream_t s) {
  ScoreArgs a;
  bool ok = N >= 0 && h >= 1 && w >= 1 && K >= 1 && K <= ld_c && ld_c % 4 == 0 && ld_r >= 4 && ld_r % 4 == 0 && ctr_col >= 0 &&
            ctr_col < ld_r;
  ok = ok && map_extent(h, w, ld_c, &a.pitch_c, &a.image_c) && map_extent(h, w, ld_r, &a.pitch_r, &a.image_r);
  const long long qk = ok ? (K + 3ll) / 4 : 1;
  ok = ok && (long long)h * w < (1ll << 31) && (long long)N * h * w < (1ll << 31) && (long long)N * h * w * qk < (1ll << 31);
  if (!ok) {
    set_error("fcos_score_map: unsupported shape N=%d h=%d w=%d K=%d ld_c=%d ld_r=%d ctr_col=%d (need N >= 0, h, w >= 1, "
              "1 <= K <= ld_c, 0 <= ctr_col < ld_r, ld_c and ld_r multiples of 4, (w + 2) ld < 2^32, (h + 2)(w + 2) ld < 2^40, "
              "N h w ceil(K / 4) < 2^31)", N, h, w, K, ld_c, ld_r, ctr_col);
    return WINO_E_SHAPE;
  }
  if (N == 0) return WINO_OK;
  if (int rc = check_nonnull(cls, reg)) return rc;
  if (int rc = check_aligned16(cls, reg)) return rc;
  if (overlaps(cls, (size_t)N * (size_t)a.image_c * 4, reg, (size_t)N * (size_t)a.image_r * 4)) {
    set_error("fcos_score_map: cls and reg must not overlap");
    return WINO_E_ARG;
  }
  a.cls = cls, a.reg = reg;
  a.K = (unsigned)K, a.qk = (unsigned)qk, a.w = (unsigned)w, a.hw = (unsigned)((long long)h * w);
  a.total = (unsigned)((long long)N * h * w * qk);
  a.ld_c = (unsigned)ld_c, a.ld_r = (unsigned)ld_r, a.ctr_col = (unsigned)ctr_col;
  a.divqk = make_fastdiv(a.qk), a.divhw = make_fastdiv(a.hw), a.divw = make_fastdiv(a.w);
  hipLaunchKernelGGL(fcos_score_kernel, dim3((a.total + 255u) / 256u), dim3(256), 0, (hipStream_t)s, a);
  return launch_status("fcos_score_kernel");
}

extern "C" int wino_fcos_decode_hw(const int* idx, int N, int k, long stride, long offset, const float* reg, int h, int w,
                                   int ld_r, int A, int K, const float* base, int stride_y, int stride_x,
                                   const float* image_hw, float* boxes, int* labels, wino_stream_t s) {
  DecodeRowsArgs a;
  bool launch;
  if (int rc = decode_rows_args("fcos_decode", nullptr, idx, N, k, stride, offset, reg, h, w, ld_r, A, K, base, stride_y,
                                stride_x, image_hw, boxes, labels, &a, &launch))
    return rc;
  if (!launch) return WINO_OK;
  hipLaunchKernelGGL(fcos_decode_kernel, dim3((a.total + 255u) / 256u), dim3(256), 0, (hipStream_t)s, a);
  return launch_status("fcos_decode_kernel");
}
