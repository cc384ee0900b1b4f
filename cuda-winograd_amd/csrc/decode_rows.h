// The rows of a selected-anchor decode, shared by retina.hip (retina_decode_kernel) and fcos.hip (fcos_decode_kernel):
// the kernel arguments, the index arithmetic that turns row j of image i into its anchor, its label and the address of
// its four regression columns, and the entry points' shape, pointer and overlap checks.  The two kernels differ in the
// function that turns (shifted base anchor, four columns) into a box, and in nothing else.
//
//   row j < k of image i holds idx = a flat index into the level's (h w A) x K scores, as wino_select_topk_map_hw
//   writes it (cols = A K), or a negative number past the kept count.
//     anchor = idx / K, label = idx % K, pixel = anchor / A, a = anchor % A, (y, x) = (pixel / w, pixel % w)
//   The four columns of anchor a lie at 4a .. 4a + 3 of pixel (1 + y, 1 + x) of the padded regression map
//   [N][h+2][w+2][ld_r]; the anchor is base[a] shifted by (x stride_x, y stride_y).  A row with idx < 0, or with an index
//   past the level (which the select never writes), gets a zero box and label -1 and reads nothing of the map.  One
//   thread per row, one 16-byte store per box: a NaN column stays in its own row.
#pragma once
#include "box_decode_math.h"
#include "wino_common.h"

#pragma clang fp contract(off)

namespace wino {

struct DecodeRowsArgs {
  const int* idx;
  const float* reg;
  const float* base;
  const float* image_hw;
  float* boxes;
  int* labels;
  unsigned total, k;          // total = N k rows
  unsigned A, K, w, limit;    // limit = h w A K: the indices of the level
  unsigned ld, pitch;         // pitch = (w + 2) ld_r
  long long image_elems;      // (h + 2)(w + 2) ld_r
  long long stride, offset;   // of idx, boxes and labels, in rows
  float stride_x, stride_y;
  DecodeWeights wts;
  FastDiv divk, divK, divA, divW;
};

// One thread's row of a 256-thread block: box(anc, d0, d1, d2, d3, Himg, Wimg) -> f32x4 is the kernel's own decode.
template <class Box>
__device__ __forceinline__ void decode_row(const DecodeRowsArgs& a, Box box_of) {
  const unsigned t = blockIdx.x * 256u + threadIdx.x;
  if (t >= a.total) return;
  const unsigned i = fastdiv(t, a.divk), j = t - i * a.k;
  const size_t row = (size_t)((long long)i * a.stride + a.offset) + j;
  const int id = a.idx[row];
  f32x4 box = {0.f, 0.f, 0.f, 0.f};
  int label = -1;
  if (id >= 0 && (unsigned)id < a.limit) {
    const unsigned anchor = fastdiv((unsigned)id, a.divK);
    label = (int)((unsigned)id - anchor * a.K);
    const unsigned pixel = fastdiv(anchor, a.divA), an = anchor - pixel * a.A;
    const unsigned y = fastdiv(pixel, a.divW), x = pixel - y * a.w;
    const float* d = a.reg + (size_t)i * (size_t)a.image_elems + (size_t)(y + 1u) * a.pitch + (size_t)(x + 1u) * a.ld + 4u * an;
    const float d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3];
    const float Himg = a.image_hw[2 * (size_t)i], Wimg = a.image_hw[2 * (size_t)i + 1];
    const f32x4 anc = grid_anchor(((const f32x4*)a.base)[an], x, y, a.stride_x, a.stride_y);
    box = box_of(anc, d0, d1, d2, d3, Himg, Wimg);
  }
  ((f32x4*)a.boxes)[row] = box;
  a.labels[row] = label;
}

// Every check of the entry points, then the arguments (wts.clamp apart).  WINO_OK with *launch = false: nothing to do.
// clamp: NULL, or the caller's clamp, refused when NaN where wino_retina_decode_hw always refused it: after the pointer
// checks, before the overlap check.
inline int decode_rows_args(const char* name, const float* clamp, const int* idx, int N, int k, long stride, long offset,
                            const float* reg, int h, int w, int ld_r, int A, int K, const float* base, int stride_y,
                            int stride_x, const float* image_hw, float* boxes, int* labels, DecodeRowsArgs* a, bool* launch) {
  *launch = false;
  const long long limit = (h >= 1 && w >= 1 && A >= 1 && K >= 1) ? (long long)h * w : -1;
  const unsigned long long pitch = (unsigned long long)(w > 0 ? w + 2ll : 0) * (unsigned long long)(ld_r > 0 ? ld_r : 0);
  const unsigned long long image = (unsigned long long)(h > 0 ? h + 2ll : 0) * (pitch < (1ull << 32) ? pitch : 0);
  if (N < 0 || k < 0 || limit < 0 || limit > 0x7fffffffll / A || limit * A > 0x7fffffffll / K || ld_r < 1 ||
      4ll * A > ld_r || stride_y < 1 || stride_x < 1 || pitch >= (1ull << 32) || image >= (1ull << 40) ||
      (long long)N * k >= (1ll << 31) || offset < 0 || offset > stride || k > stride - offset) {
    set_error("%s: unsupported shape N=%d k=%d stride=%ld offset=%ld h=%d w=%d ld_r=%d A=%d K=%d stride_y=%d "
              "stride_x=%d (need N, k >= 0, N k < 2^31, h, w, A, K >= 1, h w A K <= 2^31 - 1, 4 A <= ld_r, (w + 2) ld_r < "
              "2^32, (h + 2)(w + 2) ld_r < 2^40, strides >= 1, 0 <= offset, offset + k <= stride)", name, N, k, stride, offset, h,
              w, ld_r, A, K, stride_y, stride_x);
    return WINO_E_SHAPE;
  }
  if (N == 0 || k == 0) return WINO_OK;
  if (int rc = check_nonnull(idx, reg, base, image_hw, boxes, labels)) return rc;
  if (int rc = check_aligned16(idx, reg, base, image_hw)) return rc;
  if (int rc = check_aligned16(boxes, labels)) return rc;
  if (clamp && *clamp != *clamp) {
    set_error("%s: clamp is NaN", name);
    return WINO_E_ARG;
  }
  const size_t rows = (size_t)(N - 1) * stride + k;
  const std::pair<const void*, size_t> outs[] = {{boxes + 4 * offset, rows * 16}, {labels + offset, rows * 4}};
  const std::pair<const void*, size_t> ins[] = {{idx + offset, rows * 4}, {reg, (size_t)N * image * 4}, {base, (size_t)A * 16},
                                                {image_hw, (size_t)N * 8}};
  bool clash = overlaps(outs[0].first, outs[0].second, outs[1].first, outs[1].second);
  for (int o = 0; o < 2; o++)
    for (int q = 0; q < 4; q++) clash = clash || overlaps(outs[o].first, outs[o].second, ins[q].first, ins[q].second);
  if (clash) {
    set_error("%s: boxes and labels must not overlap idx, reg, base, image_hw or each other", name);
    return WINO_E_ARG;
  }
  a->idx = idx, a->reg = reg, a->base = base, a->image_hw = image_hw, a->boxes = boxes, a->labels = labels;
  a->total = (unsigned)((long long)N * k), a->k = (unsigned)k;
  a->A = (unsigned)A, a->K = (unsigned)K, a->w = (unsigned)w, a->limit = (unsigned)(limit * A * K);
  a->ld = (unsigned)ld_r, a->pitch = (unsigned)pitch, a->image_elems = (long long)image;
  a->stride = stride, a->offset = offset;
  a->stride_x = (float)stride_x, a->stride_y = (float)stride_y;
  a->wts = DecodeWeights{1.f, 1.f, 1.f, 1.f, 0.f};
  a->divk = make_fastdiv(a->k), a->divK = make_fastdiv(a->K), a->divA = make_fastdiv(a->A), a->divW = make_fastdiv(a->w);
  *launch = true;
  return WINO_OK;
}

}  // namespace wino
