// RetinaNet's decode: boxes and labels of the anchors a level's top-k kept, read where the head left them.  One kernel in
// plain HIP: no MFMA, no inline assembly, no scratch, no hand-off between workgroups.  The entry point owns no state and
// can be captured into a graph as it is.
//
// The rows, the index arithmetic and the checks are decode_rows.h's, shared with fcos.hip.
// wino_retina_decode_hw: row j < k of image i holds idx = a flat index into the level's (h w A) x K class logits, as
//   wino_select_topk_map_hw writes it (cols = A K), or a negative number past the kept count.
//     anchor = idx / K, label = idx % K, pixel = anchor / A, a = anchor % A, (y, x) = (pixel / w, pixel % w)
//   The four deltas of anchor a lie at columns 4a .. 4a + 3 of pixel (1 + y, 1 + x) of the padded regression map
//   [N][h+2][w+2][ld_r]; the anchor is base[a] shifted by (x stride_x, y stride_y); the box is decode_box() of
//   box_decode_math.h with weights (1, 1, 1, 1): the arithmetic of boxes.hip's box_decode_kernel, so the result is that
//   kernel's in grid mode at the same anchor, bit for bit.  A row with idx < 0, or with an index past the level (which
//   the select never writes), gets a zero box and label -1 and reads nothing of the map.  One thread per row, one 16-byte
//   store per box: a NaN delta stays in its own row.
#include "decode_rows.h"

#pragma clang fp contract(off)

namespace wino {
namespace {

__global__ __launch_bounds__(256) void retina_decode_kernel(const DecodeRowsArgs a) {
  decode_row(a, [&a](f32x4 anc, float d0, float d1, float d2, float d3, float Himg, float Wimg) {
    return decode_box(anc, d0, d1, d2, d3, a.wts, Himg, Wimg);
  });
}

}  // namespace
}  // namespace wino

using namespace wino;

extern "C" int wino_retina_decode_hw(const int* idx, int N, int k, long stride, long offset, const float* reg, int h, int w,
                                     int ld_r, int A, int K, const float* base, int stride_y, int stride_x,
                                     const float* image_hw, float clamp, float* boxes, int* labels, wino_stream_t s) {
  DecodeRowsArgs a;
  bool launch;
  if (int rc = decode_rows_args("retina_decode", &clamp, idx, N, k, stride, offset, reg, h, w, ld_r, A, K, base, stride_y,
                                stride_x, image_hw, boxes, labels, &a, &launch))
    return rc;
  if (!launch) return WINO_OK;
  a.wts.clamp = clamp;
  hipLaunchKernelGGL(retina_decode_kernel, dim3((a.total + 255u) / 256u), dim3(256), 0, (hipStream_t)s, a);
  return launch_status("retina_decode_kernel");
}
