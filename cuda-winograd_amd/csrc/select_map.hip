// wino_select_topk_map_hw: the segmented top-k of select.hip on a padded NHWC map [N][h+2][w+2][ld], in place.  Segment i
// is image i's h w cols interior scores, element j = (y w + x) cols + c at map[i][1 + y][1 + x][c]; the kernels are
// select_kernel.h's with MAP = true, where place() turns j into that address with two multiply-highs (no division, no
// per-row walk: measured, a pass costs what the flat form's costs).  The ring and the pad columns have no index, so no pass reads them.
// Same launches, workspace and order as the flat form; no library-owned scratch, no hand-off between workgroups.
#include "select_kernel.h"

using namespace wino;

namespace {
// One map call's figures; false: outside the limits.  n <= 2^31 - 1 keeps an index in idx's int32 and leaves the top
// composite-key bit patterns free; the map itself may be far longer than 2^32 bytes (image x image_elems is 64-bit).
struct MapDims {
  long long n, image_elems;
  unsigned pitch;
};
bool map_dims(int N, int h, int w, int cols, int ld, int k, MapDims* d) {
  if (N < 0 || N > SEL_MAX_SEGMENTS || h < 1 || w < 1 || cols < 1 || ld < cols || k < 1 || k > SEL_MAX_K) return false;
  d->n = (long long)h * w;   // (< 2^62)
  if (d->n > 0x7fffffffll || (d->n *= cols) > 0x7fffffffll) return false;
  const unsigned long long pitch = (unsigned long long)(w + 2ll) * (unsigned long long)ld;
  if (pitch >= (1ull << 32)) return false;
  const unsigned long long image = (unsigned long long)(h + 2ll) * pitch;
  if (image >= (1ull << 40)) return false;
  d->pitch = (unsigned)pitch, d->image_elems = (long long)image;
  return true;
}
}  // namespace

extern "C" int wino_select_topk_map_hw(const float* map, int N, int h, int w, int cols, int ld, int k, int use_thresh,
                                       float score_thresh, int* idx, float* vals, int* count, long out_stride,
                                       long out_offset, void* workspace, size_t workspace_bytes, wino_stream_t s) {
  MapDims d;
  SelectArgs a;
  SelectLayout L;
  if (h >= 1 && w >= 1 && cols >= 1 && (long long)h * w > 0x7fffffffll / cols) {
    set_error("select_topk_map: a segment of h w cols = %d x %d x %d scores is longer than 2^31 - 1: an index would not "
              "fit idx's int32", h, w, cols);
    return WINO_E_SHAPE;
  }
  bool ok = map_dims(N, h, w, cols, ld, k, &d);
  const int n = ok ? (int)d.n : 0;
  ok = ok && select_layout(N, 1, &n, &k, &a, &L) && out_offset >= 0 && out_stride < (1ll << 31) &&
       out_offset <= out_stride && k <= out_stride - out_offset;
  if (!ok) {
    set_error("select_topk_map: unsupported shape N=%d h=%d w=%d cols=%d ld=%d k=%d out_stride=%ld out_offset=%ld (need "
              "0 <= N <= %d, h, w >= 1, 1 <= cols <= ld, 1 <= k <= %d, (w + 2) ld < 2^32, (h + 2)(w + 2) ld < 2^40, "
              "0 <= out_offset, out_offset + k <= out_stride < 2^31)", N, h, w, cols, ld, k, out_stride, out_offset,
              SEL_MAX_SEGMENTS, SEL_MAX_K);
    return WINO_E_SHAPE;
  }
  if (N == 0) return WINO_OK;
  if (int rc = check_nonnull(map, idx, count)) return rc;
  if (int rc = check_aligned16(map, idx, vals, count)) return rc;
  if (use_thresh && score_thresh != score_thresh) {
    set_error("select_topk_map: score_thresh is NaN");
    return WINO_E_ARG;
  }
  if (L.total) {
    if (int rc = check_workspace(workspace, workspace_bytes, L.total)) return rc;
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) {
      set_error("tensor pointers must be 16-byte aligned (workspace)");
      return WINO_E_ARG;
    }
  }
  const size_t map_b = (size_t)N * (size_t)d.image_elems * 4;
  const size_t out_b = ((size_t)(N - 1) * out_stride + k) * 4;
  const std::pair<const void*, size_t> outs[] = {{idx + out_offset, out_b}, {vals ? vals + out_offset : nullptr, out_b},
                                                 {count, (size_t)N * 4}, {L.total ? workspace : nullptr, L.total}};
  bool clash = false;
  for (int o = 0; o < 4; o++) {
    if (!outs[o].first) continue;
    clash = clash || overlaps(outs[o].first, outs[o].second, map, map_b);
    for (int p = o + 1; p < 4; p++)
      clash = clash || (outs[p].first && overlaps(outs[o].first, outs[o].second, outs[p].first, outs[p].second));
  }
  if (clash) {
    set_error("select_topk_map: idx, vals, count and workspace must not overlap the map or each other");
    return WINO_E_ARG;
  }
  a.scores = map, a.boxes_in = nullptr, a.idx = idx, a.vals = vals, a.count = count, a.boxes_out = nullptr;
  a.hdr = (unsigned*)workspace;
  a.eq = (unsigned*)((char*)workspace + L.hdr_bytes);
  a.cand = (u64*)((char*)workspace + L.hdr_bytes + L.eq_bytes);
  a.image_stride = d.image_elems, a.out_stride = out_stride, a.boxes_image_stride = 0;
  a.eq_image = L.eq_image, a.cand_image = L.cand_image;
  a.parts = 1, a.longs = L.longs, a.use_thresh = use_thresh ? 1 : 0, a.thresh = score_thresh;
  a.off[0] = 0, a.n[0] = n, a.k[0] = k, a.kbase[0] = (int)out_offset;
  for (int p = 1; p < SEL_MAX_PARTS; p++)
    a.off[p] = a.eq_off[p] = a.cand_off[p] = 0, a.n[p] = a.k[p] = a.kbase[p] = 0, a.lp[p] = -1;
  a.cols = (unsigned)cols, a.map_w = (unsigned)w, a.map_ld = (unsigned)ld, a.map_pitch = d.pitch;
  a.div_cols = make_fastdiv(a.cols), a.div_w = make_fastdiv(a.map_w);
  return launch_select<true>(a, L, (unsigned)N, (hipStream_t)s);
}
