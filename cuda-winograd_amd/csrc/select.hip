// Segmented top-k and sort: what a detector needs between its heads and the NMS, without torch's topk / sort / gather
// and with an order that is a function of the inputs.  Plain HIP: no MFMA, no inline assembly, no library-owned scratch,
// no hand-off between workgroups inside a launch.  The entry point owns no state and can be captured into a graph.
//
// wino_select_topk_hw: S = N x parts independent segments; image i, part p reads n[p] fp32 scores at scores +
//   i image_stride + off[p] and keeps the best min(k[p], candidates) of them, best first, in the total order
//     NaN > +Inf > ... > +0 == -0 > ... > -Inf, equal scores (and all NaNs among themselves) to the lower index:
//   torch.sort(descending=True, stable=True) truncated to k.  The order is that of the 64-bit composite key
//     (orderable(score) << 32) | (0xffffffff - index),  orderable(x) = ~bits when the sign bit is set, else
//     bits | 0x80000000, with -0 mapped to +0 and every NaN to 0xffffffff first;
//   it is unique per element, so any sort of it gives the one order.  orderable() of a candidate is never 0 (-Inf gives
//   0x007fffff), and key 0 stands for "no candidate": an element past n, or one that fails score >= score_thresh.
//
//   select_sort_kernel, one workgroup of 1024 threads per segment, loads up to 8192 composite keys into LDS (64 KiB),
//   padded with zeros to a power of two, sorts them descending with a bitonic network, counts the non-zero keys and
//   writes idx / vals / boxes_out rows and the segment's count.  A segment of n <= 8192 takes its keys straight from
//   the scores: one launch.  A longer one takes them from the workspace, where the six launches before it have put
//   the composite keys of exactly its best min(k, candidates) elements:
//     select_zero_kernel: the segment's histograms and list length in the workspace start at zero.
//     select_hist_kernel x 3: radix select on orderable(score), digits of 11, 11 and 10 bits from the top.  Workgroups
//       of 256 threads take chunks of 2048 scores, count digits in LDS and add the non-zero bins to the segment's
//       histogram in the workspace.  Nobody writes a pass's result down: each later workgroup finds the digit that holds
//       the k-th key again from the finished histograms (find_digit: a suffix scan over 256 partial sums).
//     select_count_kernel: T = the k-th key's orderable value; per chunk, the number of elements equal to T.
//     select_gather_kernel: per chunk, every element above T, and those equal to T whose rank among the segment's
//       equals in index order (the earlier chunks' counts, then a scan inside the chunk) is below what is still needed,
//       are appended to the segment's candidate list (one global atomic per wave and round).
//   All equal keys cost the same as all distinct ones: every pass reads each score once, whatever the values are.
//   A segment with fewer candidates than k takes them all (T = 0).
//
// The kernels, the workspace layout and the launch sequence live in select_kernel.h as templates on the form of the
// input; this file instantiates the flat form, select_map.hip the padded-map form (wino_select_topk_map_hw).
#include "select_kernel.h"

using namespace wino;

extern "C" int wino_select_topk_hw(const float* scores, int N, long image_stride, int parts, const long* off_host,
                                   const int* n_host, const int* k_host, int use_thresh, float score_thresh, int* idx,
                                   float* vals, int* count, long out_stride, const float* boxes_in,
                                   long boxes_image_stride, float* boxes_out, void* workspace, size_t workspace_bytes,
                                   wino_stream_t s) {
  SelectArgs a;
  SelectLayout L;
  if (int rc = check_nonnull(off_host, n_host, k_host)) return rc;
  bool ok = select_layout(N, parts, n_host, k_host, &a, &L);
  long long ksum = 0, reach = 0;
  if (ok) {
    ok = image_stride >= 0 && image_stride < (1ll << 31) && (long long)N * parts <= SEL_MAX_SEGMENTS;
    for (int p = 0; p < parts && ok; p++) {
      ok = off_host[p] >= 0 && off_host[p] <= image_stride && n_host[p] <= image_stride - off_host[p] &&
           (!boxes_in || (long long)off_host[p] + n_host[p] <= boxes_image_stride);
      a.off[p] = off_host[p], a.n[p] = n_host[p], a.k[p] = k_host[p], a.kbase[p] = (int)ksum;
      ksum += k_host[p];
      if ((long long)off_host[p] + n_host[p] > reach) reach = (long long)off_host[p] + n_host[p];
    }
    ok = ok && ksum <= out_stride;
  }
  if (!ok) {
    set_error("select_topk: unsupported shape N=%d image_stride=%ld parts=%d out_stride=%ld boxes_image_stride=%ld (need "
              "N >= 0, 1 <= parts <= %d, N parts <= %d, n[p] >= 0, 1 <= k[p] <= %d, 0 <= off[p], off[p] + n[p] <= "
              "image_stride < 2^31 (and <= boxes_image_stride with boxes_in), sum k[p] <= out_stride)", N, image_stride,
              parts, out_stride, boxes_image_stride, SEL_MAX_PARTS, SEL_MAX_SEGMENTS, SEL_MAX_K);
    return WINO_E_SHAPE;
  }
  if (N == 0) return WINO_OK;
  if (int rc = check_nonnull(idx, count)) return rc;
  if (reach > 0)
    if (int rc = check_nonnull(scores)) return rc;
  if (boxes_in)
    if (int rc = check_nonnull(boxes_out)) return rc;
  if (int rc = check_aligned16(scores, idx, vals, count)) return rc;
  if (int rc = check_aligned16(boxes_in, boxes_out)) return rc;
  if (use_thresh && score_thresh != score_thresh) {
    set_error("select_topk: score_thresh is NaN");
    return WINO_E_ARG;
  }
  if (L.total) {
    if (int rc = check_workspace(workspace, workspace_bytes, L.total)) return rc;
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) {
      set_error("tensor pointers must be 16-byte aligned (workspace)");
      return WINO_E_ARG;
    }
  }
  const size_t in_elems = (size_t)(N - 1) * image_stride + reach;
  const size_t out_elems = (size_t)(N - 1) * out_stride + ksum;
  const size_t boxes_in_b = boxes_in ? ((size_t)(N - 1) * boxes_image_stride + reach) * 16 : 0;
  const std::pair<const void*, size_t> outs[] = {{idx, out_elems * 4}, {vals, out_elems * 4},
                                                 {count, (size_t)N * parts * 4},
                                                 {boxes_in ? boxes_out : nullptr, out_elems * 16},
                                                 {L.total ? workspace : nullptr, L.total}};
  const std::pair<const void*, size_t> ins[] = {{scores, in_elems * 4}, {boxes_in, boxes_in_b}};
  bool clash = false;
  for (int o = 0; o < 5; o++) {
    if (!outs[o].first) continue;
    for (int i = 0; i < 2; i++)
      clash = clash || (ins[i].first && ins[i].second && overlaps(outs[o].first, outs[o].second, ins[i].first, ins[i].second));
    for (int p = o + 1; p < 5; p++)
      clash = clash || (outs[p].first && overlaps(outs[o].first, outs[o].second, outs[p].first, outs[p].second));
  }
  if (clash) {
    set_error("select_topk: idx, vals, count, boxes_out and workspace must not overlap an input or each other");
    return WINO_E_ARG;
  }
  a.scores = scores, a.boxes_in = (const f32x4*)boxes_in, a.idx = idx, a.vals = vals, a.count = count;
  a.boxes_out = boxes_in ? (f32x4*)boxes_out : nullptr;
  a.hdr = (unsigned*)workspace;
  a.eq = (unsigned*)((char*)workspace + L.hdr_bytes);
  a.cand = (u64*)((char*)workspace + L.hdr_bytes + L.eq_bytes);
  a.image_stride = image_stride, a.out_stride = out_stride, a.boxes_image_stride = boxes_image_stride;
  a.eq_image = L.eq_image, a.cand_image = L.cand_image;
  a.parts = parts, a.longs = L.longs, a.use_thresh = use_thresh ? 1 : 0, a.thresh = score_thresh;
  a.cols = a.map_w = a.map_ld = a.map_pitch = 0u, a.div_cols = a.div_w = make_fastdiv(1u);
  for (int p = parts; p < SEL_MAX_PARTS; p++)
    a.off[p] = a.eq_off[p] = a.cand_off[p] = 0, a.n[p] = a.k[p] = a.kbase[p] = 0, a.lp[p] = -1;
  return launch_select<false>(a, L, (unsigned)(N * parts), (hipStream_t)s);
}
