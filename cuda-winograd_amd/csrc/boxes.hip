// Box decoding and batched non-maximum suppression: what a two-stage detector needs between its heads' GEMMs and
// RoIAlign, without a host round trip and with fixed-size outputs.  Three kernels in plain HIP: no MFMA, no inline
// assembly, no library-owned scratch, no tickets, no hand-off between workgroups.  Neither entry point owns state, so both
// can be captured into a graph as they are.
//
// wino_box_decode_hw: torchvision's BoxCoder.decode_single followed by clip_boxes_to_image, operation by operation in
//   fp32, on rows of a GEMM output read in place.  head [rows][ld], rows = N x rows_per_image; anchor a of row r has its
//   deltas at columns delta_col + 4a .. + 3 and, with score_col >= 0, its score at column score_col + a.
//     w = ax2 - ax1, h = ay2 - ay1, cx = ax1 + .5 w, cy = ay1 + .5 h
//     dx = d0 / wx, dy = d1 / wy, dw = min(d2 / ww, clamp), dh = min(d3 / wh, clamp)
//     pcx = dx w + cx, pcy = dy h + cy, pw = exp(dw) w, ph = exp(dh) h
//     box = (pcx - .5 pw, pcy - .5 ph, pcx + .5 pw, pcy + .5 ph), x clamped to [0, W_img], y to [0, H_img] of the row's image
//   min and the clamps are written as compares that a NaN fails, so a NaN delta reaches the coordinates it feeds, as
//   torch.clamp lets it (fminf / fmaxf would return the other operand).  One thread per box, one 16-byte store per box.
//   grid mode (grid_h, grid_w >= 1): anchors is [A][4] base anchors, row (n, y, x) of the grid_h x grid_w level takes
//     base[a] + (x stride_x, y stride_y, x stride_x, y stride_y): torchvision's AnchorGenerator in the NHWC row order.
//   boxes mode (grid_h == grid_w == 0): anchors is [rows][4], the same box for every a (the second stage: a = class).
//   Box (n, j, a), j the row within its image, goes to boxes[n boxes_image_stride + boxes_offset + j A + a] (in boxes of
//   16 bytes) and its raw score to scores[n scores_image_stride + scores_offset + j A + a].
//
// wino_batched_nms_hw: greedy NMS over S independent segments of R boxes; priority is index order (the caller sorts).
//   candidate(i) = x2 - x1 >= min_size && y2 - y1 >= min_size && (no scores || score >= score_thresh): a NaN fails every
//   compare, so a box with a NaN coordinate or score is never kept and never suppresses.  Walking i upwards, a candidate
//   that is not suppressed is kept and suppresses every later j of its group with inter / (area_i + area_j - inter) >
//   iou_thresh, inter = max(min(x2) - max(x1), 0) max(min(y2) - max(y1), 0): torchvision's form, in fp32, uncontracted.
//   The walk stops at max_out kept.
//
//   nms_mask_kernel writes the upper triangle of the suppression matrix into the workspace: R rows of nb = ceil(R / 64)
//   64-bit words per segment, bit j % 64 of word j / 64 of row i set when j > i suppresses under i.  Words left of the
//   diagonal are not written, and what the scan reads of them it drops.  A workgroup of four waves takes one block of
//   64 rows and four blocks of 64 columns; a lane owns a row, the wave's 64 column boxes are broadcast from LDS.
//
//   nms_scan_kernel, one workgroup of 1024 threads per segment (at most 2^22 - 1 segments per launch, each launch told
//   its first segment), walks the 64-row blocks.  `removed` (one bit per box,
//   in LDS) starts as the complement of the candidate bits.  Per block b: every wave holds the block's diagonal word of
//   row b 64 + lane in its lane and resolves the block in scalar registers (count trailing zeros of the live bits, read
//   lane i's word, clear what it suppresses); wave 0 writes the kept rows' outputs from the boxes it holds by lane; then
//   thread (word w, part p) ORs the kept ones of its 64 / PARTS rows' words w > b into removed[w] (one LDS atomic).
//   No global load's address depends on a decision: the diagonal words, wave 0's boxes and the threads' row words of
//   block b + 1 are requested before block b is resolved (two register sets of up to 16 words; at 32 rows per thread,
//   W = 512, one set, requested as soon as block b's words are consumed and so before block b + 1 is resolved), so
//   the chain from block to block is a barrier, an LDS read, the scalar loop and an LDS atomic.  The template argument W (64, 128, 256, 512 >= nb) is the number of threads along the words;
//   the other 1024 / W split the block's rows.
#include <cmath>

#include "box_decode_math.h"   // decode_box and grid_anchor: the decode arithmetic, shared with retina.hip
#include "wino_common.h"

#pragma clang fp contract(off)   // torch's arithmetic operation by operation: no product folded into a sum

namespace wino {
namespace {

typedef unsigned long long u64;
constexpr int NMS_MAX_R = 32768;
constexpr int NMS_MAX_WORDS = NMS_MAX_R / 64;
constexpr int SCAN_THREADS = 1024;
// HIP takes fewer than 2^32 threads along x, and the scan has one workgroup of SCAN_THREADS per segment: a launch of
// 2^22 segments is refused, and a larger count wraps (S = 2^24 - 1 ran as 2^22 - 1 workgroups and reported no error)
constexpr int SCAN_MAX_SEGMENTS = (1 << 22) - 1;
constexpr int MASK_WAVES = 4;

// ---- decode ----------------------------------------------------------------------------------------------------------------
struct DecodeArgs {
  const float* head;
  const float* anchors;
  const float* image_hw;
  float* boxes;
  float* scores;
  unsigned total;            // N x rows_per_image x A
  unsigned rpi, A, grid_w;   // grid_w == 0: boxes mode
  int ld, delta_col, score_col;
  float stride_x, stride_y;
  DecodeWeights k;
  long long bstride, boff, sstride, soff;
  FastDiv divA, divRpi, divW;
};

__global__ __launch_bounds__(256) void box_decode_kernel(const DecodeArgs a) {
  const unsigned t = blockIdx.x * 256u + threadIdx.x;
  if (t >= a.total) return;
  const unsigned r = fastdiv(t, a.divA), an = t - r * a.A;
  const unsigned n = fastdiv(r, a.divRpi), j = r - n * a.rpi;
  f32x4 anc;
  if (a.grid_w) {
    const unsigned y = fastdiv(j, a.divW), x = j - y * a.grid_w;
    anc = grid_anchor(((const f32x4*)a.anchors)[an], x, y, a.stride_x, a.stride_y);
  } else {
    anc = ((const f32x4*)a.anchors)[(size_t)r];
  }
  const float* row = a.head + (size_t)r * (size_t)a.ld;
  const float* d = row + a.delta_col + 4 * an;
  const float d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3];
  const float Himg = a.image_hw[2 * (size_t)n], Wimg = a.image_hw[2 * (size_t)n + 1];
  const f32x4 box = decode_box(anc, d0, d1, d2, d3, a.k, Himg, Wimg);
  const size_t in_image = (size_t)j * a.A + an;
  ((f32x4*)a.boxes)[(size_t)((long long)n * a.bstride + a.boff) + in_image] = box;
  if (a.score_col >= 0) a.scores[(size_t)((long long)n * a.sstride + a.soff) + in_image] = row[a.score_col + an];
}

// ---- NMS -------------------------------------------------------------------------------------------------------------------
struct NmsArgs {
  const f32x4* boxes;
  const float* scores;
  const int* groups;
  u64* mask;
  int* keep;
  int* count;
  float* rois;
  int S, R, nb, max_out;
  int s0;   // the scan launch's first segment (the mask kernel takes all S at once)
  float iou, min_size, score_thresh;
};

__global__ __launch_bounds__(64 * MASK_WAVES) void nms_mask_kernel(const NmsArgs a) {
  __shared__ f32x4 cbox[MASK_WAVES][64];
  __shared__ int cgrp[MASK_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = blockIdx.x / a.nb, rb = blockIdx.x - s * a.nb;
  if ((int)blockIdx.y * MASK_WAVES + MASK_WAVES - 1 < rb) return;   // (the whole workgroup: left of the diagonal)
  const int cb = blockIdx.y * MASK_WAVES + wave;
  const size_t seg = (size_t)s * (size_t)a.R;
  const int i = rb * 64 + lane, j0 = cb * 64;
  const bool work = cb >= rb && cb < a.nb;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if (work) {
    const int j = j0 + lane;
    cbox[wave][lane] = j < a.R ? a.boxes[seg + j] : zero;
    cgrp[wave][lane] = (a.groups && j < a.R) ? a.groups[seg + j] : 0;
  }
  __syncthreads();
  if (!work || i >= a.R) return;
  const f32x4 bi = a.boxes[seg + i];
  const int gi = a.groups ? a.groups[seg + i] : 0;
  const float area_i = (bi.z - bi.x) * (bi.w - bi.y);
  u64 bits = 0;
  for (int jj = 0; jj < 64; jj++) {
    const f32x4 bj = cbox[wave][jj];
    const float area_j = (bj.z - bj.x) * (bj.w - bj.y);
    const float iw = fmaxf(fminf(bi.z, bj.z) - fmaxf(bi.x, bj.x), 0.f);
    const float ih = fmaxf(fminf(bi.w, bj.w) - fmaxf(bi.y, bj.y), 0.f);
    const float inter = iw * ih;
    const float iou = inter / (area_i + area_j - inter);
    const int j = j0 + jj;
    if (j > i && j < a.R && cgrp[wave][jj] == gi && iou > a.iou) bits |= 1ull << jj;
  }
  a.mask[(seg + i) * (size_t)a.nb + cb] = bits;
}

__device__ __forceinline__ u64 uniform64(u64 v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 readlane64(u64 v, int l) {   // l is wave-uniform
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, l), hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), l);
  return ((u64)hi << 32) | lo;
}

template <int W>
__global__ __launch_bounds__(SCAN_THREADS) void nms_scan_kernel(const NmsArgs a) {
  constexpr int PARTS = SCAN_THREADS / W, RPT = 64 / PARTS;   // threads along a block's rows, rows per thread
  constexpr bool TWO_SETS = RPT <= 16;   // (two sets of 32 64-bit words would not fit a thread's 128 registers)
  __shared__ u64 removed[NMS_MAX_WORDS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = a.s0 + (int)blockIdx.x, R = a.R, nb = a.nb;
  const size_t seg = (size_t)s * (size_t)R;
  const u64* mask = a.mask + seg * (size_t)nb;
  const f32x4* boxes = a.boxes + seg;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  for (int w0 = wave; w0 < nb; w0 += SCAN_THREADS / 64) {   // removed = not a candidate (rows past R included)
    const int i = w0 * 64 + lane;
    bool c = false;
    if (i < R) {
      const f32x4 bx = boxes[i];
      c = (bx.z - bx.x >= a.min_size) && (bx.w - bx.y >= a.min_size);
      if (a.scores) c = c && (a.scores[seg + i] >= a.score_thresh);
    }
    const u64 cand = __ballot(c);
    if (lane == 0) removed[w0] = ~cand;
  }

  const int w = tid % W, row0 = (tid / W) * RPT;
  // What block b needs from memory, all at addresses known up front.  The threads' row words are loaded without a
  // condition, from the row clamped to R - 1 and the word clamped to nb - 1 (inside the segment's matrix): a row past R
  // is never kept, and the OR below drops every word that is not right of the diagonal.
  // (32-bit byte offsets from the segment's uniform base: one matrix is at most 32768 x 512 x 8 bytes = 128 MiB)
  const unsigned column = (unsigned)(w < nb ? w : nb - 1) * 8u, pitch = (unsigned)nb * 8u;
  auto load_rows = [&](int b, u64 (&v)[RPT]) {
#pragma unroll
    for (int r = 0; r < RPT; r++) {
      const int i = b * 64 + row0 + r;
      v[r] = *(const u64*)((const char*)mask + ((unsigned)(i < R ? i : R - 1) * pitch + column));
    }
  };
  auto load_diag = [&](int b) -> u64 {
    const int i = b * 64 + lane;
    return i < R ? mask[(size_t)i * nb + b] : 0ull;
  };
  auto load_box = [&](int b) -> f32x4 {
    const int i = b * 64 + lane;
    return (wave == 0 && a.rois && i < R) ? boxes[i] : zero;
  };

  u64 cur[RPT], nxt[RPT];
  u64 diag = load_diag(0), diag_n = 0;
  f32x4 box = load_box(0), box_n = zero;
  load_rows(0, cur);
  int count = 0;
  int* keep = a.keep + (size_t)s * (size_t)a.max_out;
  float* rois = a.rois ? a.rois + (size_t)s * (size_t)a.max_out * 5 : nullptr;

  for (int b = 0; b < nb; b++) {
    const bool more = b + 1 < nb;
    if (more) {
      diag_n = load_diag(b + 1);
      box_n = load_box(b + 1);
      if (TWO_SETS) load_rows(b + 1, nxt);
    }
    __syncthreads();   // removed[b] is final: the candidates' words, and every earlier block's ORs
    u64 alive = ~uniform64(removed[b]);
    u64 K = 0;
    int left = a.max_out - count;
    while (alive != 0 && left > 0) {   // scalar: every wave resolves the block for itself
      const int i = __builtin_ctzll(alive);
      K |= 1ull << i;
      left--;
      alive &= ~(readlane64(diag, i) | (1ull << i));
    }
    if (wave == 0 && ((K >> lane) & 1)) {
      const int pos = count + __popcll(K & ((1ull << lane) - 1));
      keep[pos] = b * 64 + lane;
      if (rois) {
        float* o = rois + (size_t)pos * 5;
        o[0] = (float)s, o[1] = box.x, o[2] = box.y, o[3] = box.z, o[4] = box.w;
      }
    }
    count += __popcll(K);
    u64 acc = 0;
    const unsigned mine = (unsigned)(K >> row0);   // this thread's RPT <= 32 rows
#pragma unroll
    for (int r = 0; r < RPT; r++) acc |= ((mine >> r) & 1) ? cur[r] : 0ull;
    if (w > b && w < nb && acc) atomicOr(&removed[w], acc);
    if (count >= a.max_out || !more) break;
    diag = diag_n, box = box_n;
    if (TWO_SETS) {
#pragma unroll
      for (int r = 0; r < RPT; r++) cur[r] = nxt[r];
    } else {
      load_rows(b + 1, cur);
    }
  }

  for (int p = count + tid; p < a.max_out; p += SCAN_THREADS) {
    keep[p] = -1;
    if (rois) {
      float* o = rois + (size_t)p * 5;
      o[0] = -1.f, o[1] = 0.f, o[2] = 0.f, o[3] = 0.f, o[4] = 0.f;
    }
  }
  if (tid == 0) a.count[s] = count;
}

template <int W>
int launch_scan(NmsArgs a, hipStream_t s) {   // launches of at most SCAN_MAX_SEGMENTS segments, each from its own s0
  for (a.s0 = 0; a.s0 < a.S; a.s0 += SCAN_MAX_SEGMENTS) {
    const int n = a.S - a.s0 < SCAN_MAX_SEGMENTS ? a.S - a.s0 : SCAN_MAX_SEGMENTS;
    hipLaunchKernelGGL(nms_scan_kernel<W>, dim3((unsigned)n), dim3(SCAN_THREADS), 0, s, a);
    if (int rc = launch_status("nms_scan_kernel")) return rc;
  }
  return WINO_OK;
}

bool finite_nonzero(float v) { return std::isfinite(v) && v != 0.f; }

}  // namespace
}  // namespace wino

using namespace wino;

extern "C" int wino_box_decode_hw(const float* head, int N, int rows_per_image, int ld, int A, int delta_col,
                                  int score_col, const float* anchors, int grid_h, int grid_w, int stride_y, int stride_x,
                                  const float* image_hw, float wx, float wy, float ww, float wh, float clamp, float* boxes,
                                  long boxes_image_stride, long boxes_offset, float* scores, long scores_image_stride,
                                  long scores_offset, wino_stream_t s) {
  const bool grid = grid_h != 0 || grid_w != 0;
  const bool want_scores = score_col >= 0;
  // (N rows_per_image < 2^31 first: the product with A then stays far inside 64 bits)
  const long long rows_ll = (long long)(N > 0 ? N : 0) * (rows_per_image > 0 ? rows_per_image : 0);
  const long long per_image = (long long)rows_per_image * A;
  if (N < 0 || rows_per_image < 0 || ld < 1 || A < 1 || delta_col < 0 || (long long)delta_col + 4ll * A > ld ||
      (want_scores && (long long)score_col + A > ld) ||
      (grid && (grid_h < 1 || grid_w < 1 || stride_y < 1 || stride_x < 1 ||
                (long long)grid_h * grid_w != rows_per_image)) ||
      rows_ll >= (1ll << 31) || rows_ll * A >= (1ll << 31)) {
    set_error("box_decode: unsupported shape N=%d rows_per_image=%d ld=%d A=%d delta_col=%d score_col=%d grid_h=%d "
              "grid_w=%d stride_y=%d stride_x=%d (need N, rows_per_image >= 0, A >= 1, delta_col >= 0, delta_col + 4 A "
              "<= ld, score_col < 0 or score_col + A <= ld, grid_h = grid_w = 0 or grid_h grid_w == rows_per_image with "
              "strides >= 1, N rows_per_image A < 2^31)", N, rows_per_image, ld, A, delta_col, score_col, grid_h, grid_w,
              stride_y, stride_x);
    return WINO_E_SHAPE;
  }
  if (boxes_offset < 0 || boxes_image_stride < per_image || boxes_image_stride - per_image < boxes_offset ||
      (want_scores && (scores_offset < 0 || scores_image_stride < per_image ||
                       scores_image_stride - per_image < scores_offset))) {
    set_error("box_decode: unsupported shape boxes_image_stride=%ld boxes_offset=%ld scores_image_stride=%ld "
              "scores_offset=%ld: an image's %lld boxes must fit between the offset and the stride", boxes_image_stride,
              boxes_offset, scores_image_stride, scores_offset, per_image);
    return WINO_E_SHAPE;
  }
  if (N == 0 || rows_per_image == 0) return WINO_OK;
  if (int rc = check_nonnull(head, anchors, image_hw, boxes)) return rc;
  if (want_scores)
    if (int rc = check_nonnull(scores)) return rc;
  if (int rc = check_aligned16(head, anchors, image_hw, boxes)) return rc;
  if (want_scores)
    if (int rc = check_aligned16(scores)) return rc;
  if (!finite_nonzero(wx) || !finite_nonzero(wy) || !finite_nonzero(ww) || !finite_nonzero(wh) || clamp != clamp) {
    set_error("box_decode: weights (%g, %g, %g, %g) must be finite and not zero, clamp=%g not NaN", (double)wx, (double)wy,
              (double)ww, (double)wh, (double)clamp);
    return WINO_E_ARG;
  }
  const size_t rows = (size_t)N * rows_per_image;
  const size_t head_b = rows * ld * sizeof(float), hw_b = (size_t)N * 2 * sizeof(float);
  const size_t anchors_b = (grid ? (size_t)A : rows) * 16;
  const float* boxes0 = boxes + 4 * boxes_offset;
  const size_t boxes_b = ((size_t)(N - 1) * boxes_image_stride + per_image) * 16;
  const float* scores0 = want_scores ? scores + scores_offset : nullptr;
  const size_t scores_b = want_scores ? ((size_t)(N - 1) * scores_image_stride + per_image) * 4 : 0;
  bool clash = overlaps(boxes0, boxes_b, head, head_b) || overlaps(boxes0, boxes_b, anchors, anchors_b) ||
               overlaps(boxes0, boxes_b, image_hw, hw_b);
  if (want_scores)
    clash = clash || overlaps(scores0, scores_b, head, head_b) || overlaps(scores0, scores_b, anchors, anchors_b) ||
            overlaps(scores0, scores_b, image_hw, hw_b) || overlaps(scores0, scores_b, boxes0, boxes_b);
  if (clash) {
    set_error("box_decode: boxes and scores must not overlap head, anchors, image_hw or each other");
    return WINO_E_ARG;
  }
  DecodeArgs a;
  a.head = head, a.anchors = anchors, a.image_hw = image_hw, a.boxes = boxes, a.scores = scores;
  a.total = (unsigned)((long long)N * per_image);
  a.rpi = (unsigned)rows_per_image, a.A = (unsigned)A, a.grid_w = grid ? (unsigned)grid_w : 0u;
  a.ld = ld, a.delta_col = delta_col, a.score_col = want_scores ? score_col : -1;
  a.stride_x = (float)stride_x, a.stride_y = (float)stride_y;
  a.k = DecodeWeights{wx, wy, ww, wh, clamp};
  a.bstride = boxes_image_stride, a.boff = boxes_offset, a.sstride = scores_image_stride, a.soff = scores_offset;
  a.divA = make_fastdiv(a.A), a.divRpi = make_fastdiv(a.rpi), a.divW = make_fastdiv(grid ? a.grid_w : 1u);
  hipLaunchKernelGGL(box_decode_kernel, dim3((a.total + 255u) / 256u), dim3(256), 0, (hipStream_t)s, a);
  return launch_status("box_decode_kernel");
}

extern "C" int wino_batched_nms_hw(const float* boxes, const float* scores, const int* groups, int S, int R,
                                   float iou_thresh, float min_size, float score_thresh, int max_out, int* keep, int* count,
                                   float* rois_out, void* workspace, size_t workspace_bytes, wino_stream_t s) {
  const int nb = R > 0 ? (R + 63) / 64 : 0;
  // S ceil(R / 64) workgroups of 256 threads: HIP takes fewer than 2^32 threads along x (the scan, one workgroup of 1024
  // threads per segment, is cut into launches of at most SCAN_MAX_SEGMENTS)
  if (S < 0 || R < 0 || R > NMS_MAX_R || max_out < 1 || (long long)S * (nb > 0 ? nb : 1) >= (1ll << 24)) {
    set_error("batched_nms: unsupported shape S=%d R=%d max_out=%d (need S >= 0, 0 <= R <= %d, max_out >= 1, "
              "S ceil(R / 64) < 2^24)", S, R, max_out, NMS_MAX_R);
    return WINO_E_SHAPE;
  }
  if (S == 0) return WINO_OK;
  if (R == 0) {   // nothing to launch: every segment keeps nothing (keep = -1 is all bytes 0xFF; rois_out is not written)
    if (int rc = check_nonnull(count)) return rc;
    WINO_HIP(hipMemsetAsync(count, 0, (size_t)S * sizeof(int), (hipStream_t)s));
    if (keep) WINO_HIP(hipMemsetAsync(keep, 0xFF, (size_t)S * max_out * sizeof(int), (hipStream_t)s));
    return WINO_OK;
  }
  if (int rc = check_nonnull(boxes, keep, count)) return rc;
  if (int rc = check_aligned16(boxes, scores, groups, keep)) return rc;
  if (int rc = check_aligned16(count, rois_out)) return rc;
  if (iou_thresh != iou_thresh || min_size != min_size || score_thresh != score_thresh) {
    set_error("batched_nms: iou_thresh=%g min_size=%g score_thresh=%g: a threshold is NaN", (double)iou_thresh,
              (double)min_size, (double)score_thresh);
    return WINO_E_ARG;
  }
  const size_t n = (size_t)S * R, need = n * nb * sizeof(u64);
  if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
  if (reinterpret_cast<uintptr_t>(workspace) & 15u) {
    set_error("tensor pointers must be 16-byte aligned (workspace)");
    return WINO_E_ARG;
  }
  const size_t keep_b = (size_t)S * max_out * sizeof(int), count_b = (size_t)S * sizeof(int);
  const size_t rois_b = rois_out ? (size_t)S * max_out * 5 * sizeof(float) : 0;
  const std::pair<const void*, size_t> outs[] = {{keep, keep_b}, {count, count_b}, {rois_out, rois_b}, {workspace, need}};
  const std::pair<const void*, size_t> ins[] = {{boxes, n * 16}, {scores, scores ? n * 4 : 0}, {groups, groups ? n * 4 : 0}};
  bool clash = false;
  for (int o = 0; o < 4; o++) {
    if (!outs[o].first) continue;
    for (int i = 0; i < 3; i++)
      clash = clash || (ins[i].first && overlaps(outs[o].first, outs[o].second, ins[i].first, ins[i].second));
    for (int p = o + 1; p < 4; p++)
      clash = clash || (outs[p].first && overlaps(outs[o].first, outs[o].second, outs[p].first, outs[p].second));
  }
  if (clash) {
    set_error("batched_nms: keep, count, rois_out and workspace must not overlap an input or each other");
    return WINO_E_ARG;
  }
  NmsArgs a;
  a.boxes = (const f32x4*)boxes, a.scores = scores, a.groups = groups, a.mask = (u64*)workspace;
  a.keep = keep, a.count = count, a.rois = rois_out;
  a.S = S, a.R = R, a.nb = nb, a.max_out = max_out, a.s0 = 0;
  a.iou = iou_thresh, a.min_size = min_size, a.score_thresh = score_thresh;
  hipLaunchKernelGGL(nms_mask_kernel, dim3((unsigned)(S * nb), (unsigned)((nb + MASK_WAVES - 1) / MASK_WAVES)),
                     dim3(64 * MASK_WAVES), 0, (hipStream_t)s, a);
  if (int rc = launch_status("nms_mask_kernel")) return rc;
  if (nb <= 64) return launch_scan<64>(a, (hipStream_t)s);
  if (nb <= 128) return launch_scan<128>(a, (hipStream_t)s);
  if (nb <= 256) return launch_scan<256>(a, (hipStream_t)s);
  return launch_scan<512>(a, (hipStream_t)s);
}
