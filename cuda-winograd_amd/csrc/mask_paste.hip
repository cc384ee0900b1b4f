// Mask R-CNN's mask selection and paste: torchvision's maskrcnn_inference + paste_masks_in_image(padding = 1) (its CPU
// path: expand_masks, expand_boxes, .to(int64), paste_mask_in_image), operation by operation, in one launch.
//
// wino_mask_paste_hw: for every detection r = n D + d, select the mask of class labels[r] out of the mask head's logits,
//   apply the sigmoid and paste it into plane (n, d) of out [N][D][H][W] (fp32) and / or binary [N][D][H][W] (uint8,
//   value > threshold).  Every byte of every plane is written.
//   logits   PLANES:    [R][classes][M][M]
//            GEMM_ROWS: [R P P 4][ld], rows ordered (r, y, x, dy, dx), M = 2 P: pixel (Y, X) of class c is
//                       logits[(((r P + (Y >> 1)) P + (X >> 1)) 4 + (Y & 1) 2 + (X & 1)) ld + c]
//   label    outside [0, classes): the plane is all zeros and no logit and no box is read (a padding row's -1)
//   image    (im_h, im_w) = image_hw[n] truncated to int and clamped to [0, H] x [0, W]; the plane beyond it is zero
//   box      scale = float(M + 2) / M;  w_half = (x2 - x1) 0.5 scale, x_c = (x2 + x1) 0.5;  ex1 = x_c - w_half, ex2 = x_c +
//            w_half, likewise y, in fp32 and uncontracted;  b = (int) e truncates toward zero (-0.5 -> 0, as .to(int64)).
//            Named deviation: e is clamped to +-2^30 before the conversion and the integers below are 64-bit (torch would
//            have to allocate w x h for such a box).  A box with a coordinate that is not finite gives NaN in the whole
//            image window [0, im_h) x [0, im_w) and reads no logit.
//   size     w = max(bx2 - bx1 + 1, 1), h likewise
//   window   x0 = max(bx1, 0), x1e = min(bx2 + 1, im_w), likewise y; empty: a zero plane
//   value    inside the window, at d = (y - by1, x - bx1): the bilinear align_corners=False resize to h x w of the
//            (M + 2)^2 map that holds 1 / (1 + exp(-logit)) with a ring of zeros, with resize.hip's exact integer source
//            coordinates per axis (in = M + 2, out = w or h): num = max((2 d + 1) in - out, 0), i0 = num / (2 out),
//            i1 = min(i0 + 1, in - 1), lambda = float(num - i0 2 out) / float(2 out); value = (1-ly)((1-lx) a + lx b) +
//            ly((1-lx) c + lx d) in fp32, all four taps always multiplied: a NaN logit reaches exactly the pixels whose
//            taps include it.  Outside the window: 0.
//
// A store-bound kernel: at N = 2, D = 100, 800 x 1344 the planes are 860 MB and the selected logits 0.6 MB.  One workgroup
// of four waves owns ROWS output rows of one plane; everything about the box is the same for the whole workgroup.
//   A block that misses the window (most of the grid) reads no logit and writes its rows, which are contiguous, as one
//   span of zeros.
//   A block that meets it stages, once, the source rows its output rows tap, all M + 2 columns, as probabilities in LDS
//   (16 KB static: (M + 2)^2 <= 4096 floats; the sigmoid is computed once per mask element), then wave v forms rows v,
//   v + 4, ... from there.
// Spans are stored by alignment, not by x: a scalar head up to the first 16-byte boundary, 16-byte stores (four fp32 or
// sixteen uint8 per lane, neighbouring lanes on neighbouring 16 bytes), a scalar tail.  Both bases are 16-byte aligned,
// so the boundary follows from the element index alone.  With both outputs each is its own pass over the span; the bytes
// compare the same fp32 values the fp32 pass stored (the same uncontracted operations on the same operands).
#include <cmath>

#include "wino_common.h"

#pragma clang fp contract(off)   // torch's box arithmetic operation by operation; and the two passes bit for bit alike

namespace wino {
namespace {

constexpr int ROWS = 16;            // output rows per workgroup (measured: 64 rows for the bytes alone, the same bytes per
                                    // workgroup, take 157 us where 16 take 94 us: fewer, longer window blocks balance worse)
constexpr int THREADS = 256;
constexpr int MAX_M = 62;
constexpr int MAX_SRC = MAX_M + 2;  // side of the zero-ringed probability map
constexpr long long MAX_BLOCKS = 1ll << 22;   // workgroups per launch (HIP takes fewer than 2^32 threads along x)

struct PasteArgs {
  const float* logits;
  const int* labels;
  const float* boxes;
  const float* image_hw;
  float* out;
  unsigned char* bin;
  long long first;       // the launch's first work item; item = plane * rowblocks + row block
  int D, H, W, M, classes, ld, layout, rowblocks;
  float scale, threshold;
};

struct Coord {
  int i0, i1;
  float lam;
};
// I = int while 2 out in < 2^31, long long beyond (out reaches 2^31 + 1 under the +-2^30 clamp)
template <class I>
__device__ __forceinline__ Coord coord(I d, int in, I out) {
  I num = (2 * d + 1) * in - out;
  if (num < 0) num = 0;
  const I two = 2 * out;
  const I q = num / two;
  Coord c;
  c.i0 = (int)q;
  c.i1 = c.i0 + 1 < in ? c.i0 + 1 : in - 1;
  c.lam = (float)(num - q * two) / (float)two;
  return c;
}

__device__ __forceinline__ float lerp2(float a, float b, float c, float d, float lx, float ly) {
  const float top = (1.f - lx) * a + lx * b;
  const float bot = (1.f - lx) * c + lx * d;
  return (1.f - ly) * top + ly * bot;
}

// expand_boxes' one axis, then .to(int64) with the clamp
__device__ __forceinline__ void expand(float lo, float hi, float scale, long long* b1, long long* b2) {
  const float half = (hi - lo) * 0.5f * scale;
  const float c = (hi + lo) * 0.5f;
  const float lim = 1073741824.f;
  float e1 = c - half, e2 = c + half;
  e1 = e1 < -lim ? -lim : (e1 > lim ? lim : e1);
  e2 = e2 < -lim ? -lim : (e2 > lim ? lim : e2);
  *b1 = (long long)e1;
  *b2 = (long long)e2;
}

// `len` elements from `p` on, element j = val(j), by threads t = 0 .. nt - 1.
template <class F>
__device__ __forceinline__ void store_span(float* p, int len, int t, int nt, F val) {
  int head = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2;
  head = head < len ? head : len;
  const int groups = (len - head) >> 2, tail0 = head + 4 * groups;
  if (t < head) p[t] = val(t);
  if (t < len - tail0) p[tail0 + t] = val(tail0 + t);
  for (int g = t; g < groups; g += nt) {
    const int j = head + 4 * g;
    f32x4 v;
    v[0] = val(j), v[1] = val(j + 1), v[2] = val(j + 2), v[3] = val(j + 3);
    *(f32x4*)(p + j) = v;
  }
}

template <class F>
__device__ __forceinline__ void store_span(unsigned char* p, int len, int t, int nt, F val) {
  int head = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u);
  head = head < len ? head : len;
  const int groups = (len - head) >> 4, tail0 = head + 16 * groups;
  if (t < head) p[t] = val(t);
  if (t < len - tail0) p[tail0 + t] = val(tail0 + t);   // (at most 15 of each: nt >= 64)
  for (int g = t; g < groups; g += nt) {
    const int j = head + 16 * g;
    unsigned w[4];
#pragma unroll
    for (int k = 0; k < 4; k++)
      w[k] = (unsigned)val(j + 4 * k) | ((unsigned)val(j + 4 * k + 1) << 8) | ((unsigned)val(j + 4 * k + 2) << 16) |
             ((unsigned)val(j + 4 * k + 3) << 24);
    *(uint4*)(p + j) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// One output row of a block that meets the window, columns [x0, x1e) from the staged rows p0 / p1 (nullptr: NaN).
template <class I>
__device__ __forceinline__ void paste_row(const PasteArgs& a, float* orow, unsigned char* brow, int lane, const float* p0,
                                          const float* p1, float ly, int x0, int x1e, long long bx1, long long w) {
  const int in = a.M + 2;
  auto val = [&](int x) -> float {
    if (x < x0 || x >= x1e) return 0.f;
    if (!p0) return __builtin_nanf("");
    const Coord cx = coord<I>((I)(x - bx1), in, (I)w);
    return lerp2(p0[cx.i0], p0[cx.i1], p1[cx.i0], p1[cx.i1], cx.lam, ly);
  };
  if (orow) store_span(orow, a.W, lane, 64, val);
  if (brow) {
    const float thr = a.threshold;
    store_span(brow, a.W, lane, 64, [&](int x) -> unsigned char { return val(x) > thr ? 1 : 0; });
  }
}

__global__ __launch_bounds__(THREADS) void mask_paste_kernel(const PasteArgs a) {
  __shared__ float prob[MAX_SRC * MAX_SRC];
  const int tid = threadIdx.x;
  const long long item = a.first + blockIdx.x;
  const long long plane = item / a.rowblocks;
  const int rb = (int)(item - plane * a.rowblocks);
  const int n = (int)(plane / a.D);
  const int y_first = rb * ROWS, y_end = y_first + ROWS < a.H ? y_first + ROWS : a.H;
  const size_t base = (size_t)plane * a.H * a.W + (size_t)y_first * a.W;
  float* const ob = a.out ? a.out + base : nullptr;
  unsigned char* const bb = a.bin ? a.bin + base : nullptr;

  // ---- the plane's window: the same for every thread
  const int label = a.labels[plane];
  bool hit = label >= 0 && label < a.classes, finite = true;
  long long bx1 = 0, by1 = 0, w = 1, h = 1;
  int x0 = 0, x1e = 0, y0 = 0, y1e = 0;
  if (hit) {
    float fh = a.image_hw[2 * n], fw = a.image_hw[2 * n + 1];
    fh = fh > 0.f ? (fh < (float)a.H ? fh : (float)a.H) : 0.f;   // (a NaN fails the first compare: 0)
    fw = fw > 0.f ? (fw < (float)a.W ? fw : (float)a.W) : 0.f;
    const int im_h = (int)fh, im_w = (int)fw;
    const f32x4 box = *(const f32x4*)(a.boxes + 4 * plane);
    finite = fabsf(box[0]) < INFINITY && fabsf(box[1]) < INFINITY && fabsf(box[2]) < INFINITY && fabsf(box[3]) < INFINITY;
    if (finite) {
      long long bx2, by2;
      expand(box[0], box[2], a.scale, &bx1, &bx2);
      expand(box[1], box[3], a.scale, &by1, &by2);
      w = bx2 - bx1 + 1 > 1 ? bx2 - bx1 + 1 : 1;
      h = by2 - by1 + 1 > 1 ? by2 - by1 + 1 : 1;
      x0 = (int)(bx1 > 0 ? (bx1 < im_w ? bx1 : im_w) : 0);
      y0 = (int)(by1 > 0 ? (by1 < im_h ? by1 : im_h) : 0);
      x1e = (int)(bx2 + 1 < im_w ? (bx2 + 1 > 0 ? bx2 + 1 : 0) : im_w);
      y1e = (int)(by2 + 1 < im_h ? (by2 + 1 > 0 ? by2 + 1 : 0) : im_h);
    } else {
      x1e = im_w, y1e = im_h;
    }
    const int ya = y0 > y_first ? y0 : y_first, yb = y1e < y_end ? y1e : y_end;
    hit = x0 < x1e && ya < yb;
  }

  if (!hit) {   // the block's rows are one contiguous span
    const int len = (y_end - y_first) * a.W;
    if (ob) store_span(ob, len, tid, THREADS, [](int) -> float { return 0.f; });
    const unsigned char zero = 0.f > a.threshold ? 1 : 0;   // (a negative threshold: the zeros are above it too)
    if (bb) store_span(bb, len, tid, THREADS, [zero](int) -> unsigned char { return zero; });
    return;
  }

  const int in = a.M + 2;
  const bool small = w < (1 << 23) && h < (1 << 23);   // 2 out in < 2^30: 32-bit coordinates
  const int ya = y0 > y_first ? y0 : y_first, yb = y1e < y_end ? y1e : y_end;   // the block's rows inside the window
  int r_lo = 0;
  if (finite) {
    // the source rows rows ya .. yb - 1 tap (i0 and i1 do not decrease with y), as probabilities with the zero ring
    const Coord ca = coord<long long>(ya - by1, in, h), cb = coord<long long>(yb - 1 - by1, in, h);
    r_lo = ca.i0;
    const int cells = (cb.i1 - r_lo + 1) * in;
    const int M = a.M, P = M >> 1;
    for (int u = tid; u < cells; u += THREADS) {
      const int row = r_lo + u / in, col = u % in;
      const int Y = row - 1, X = col - 1;
      float p = 0.f;
      if (Y >= 0 && Y < M && X >= 0 && X < M) {
        const size_t idx =
            a.layout == WINO_MASK_LAYOUT_PLANES
                ? (((size_t)plane * a.classes + label) * M + Y) * M + X
                : ((((size_t)plane * P + (Y >> 1)) * P + (X >> 1)) * 4 + (Y & 1) * 2 + (X & 1)) * (size_t)a.ld + label;
        p = 1.f / (1.f + expf(-a.logits[idx]));
      }
      prob[u] = p;
    }
    __syncthreads();
  }

  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int y = y_first + wave; y < y_end; y += THREADS / 64) {
    const size_t off = (size_t)(y - y_first) * a.W;
    float* const orow = ob ? ob + off : nullptr;
    unsigned char* const brow = bb ? bb + off : nullptr;
    const bool inside = y >= ya && y < yb;
    const int rx0 = inside ? x0 : 0, rx1e = inside ? x1e : 0;   // (a row off the window: all zeros)
    const float *p0 = nullptr, *p1 = nullptr;
    float ly = 0.f;
    if (inside && finite) {
      const Coord cy = coord<long long>(y - by1, in, h);
      p0 = prob + (cy.i0 - r_lo) * in;
      p1 = prob + (cy.i1 - r_lo) * in;
      ly = cy.lam;
    }
    if (small)
      paste_row<int>(a, orow, brow, lane, p0, p1, ly, rx0, rx1e, bx1, w);
    else
      paste_row<long long>(a, orow, brow, lane, p0, p1, ly, rx0, rx1e, bx1, w);
  }
}

}  // namespace
}  // namespace wino

using namespace wino;

extern "C" int wino_mask_paste_hw(const float* logits, int layout, const int* labels, const float* boxes,
                                  const float* image_hw, int N, int D, int classes, int M, int ld, int H, int W,
                                  float threshold, float* out, void* binary, wino_stream_t s) {
  if (layout != WINO_MASK_LAYOUT_PLANES && layout != WINO_MASK_LAYOUT_GEMM_ROWS) {
    set_error("mask_paste: layout=%d is neither WINO_MASK_LAYOUT_PLANES nor WINO_MASK_LAYOUT_GEMM_ROWS", layout);
    return WINO_E_ARG;
  }
  const bool rows = layout == WINO_MASK_LAYOUT_GEMM_ROWS;
  if (N < 0 || D < 0 || classes < 1 || M < 1 || M > MAX_M || H < 1 || W < 1 || (rows && ((M & 1) || classes > ld)) ||
      (long long)H * W >= (1ll << 31)) {
    set_error("mask_paste: unsupported shape N=%d D=%d classes=%d M=%d ld=%d H=%d W=%d (need N, D >= 0, classes >= 1, "
              "1 <= M <= %d, H, W >= 1, H W < 2^31; GEMM_ROWS: M even, classes <= ld)", N, D, classes, M, ld, H, W, MAX_M);
    return WINO_E_SHAPE;
  }
  if (N == 0 || D == 0) return WINO_OK;
  if (int rc = check_nonnull(logits, labels, boxes, image_hw)) return rc;
  if (!out && !binary) {
    set_error("mask_paste: out and binary are both NULL");
    return WINO_E_ARG;
  }
  if (int rc = check_aligned16(logits, labels, boxes, image_hw, out, (const char*)binary)) return rc;
  if (threshold != threshold) {
    set_error("mask_paste: threshold is NaN");
    return WINO_E_ARG;
  }
  const size_t R = (size_t)N * D, pix = (size_t)H * W;
  const size_t logits_b = (rows ? R * M * M * (size_t)ld : R * classes * M * M) * sizeof(float);
  const size_t out_b = out ? R * pix * sizeof(float) : 0, bin_b = binary ? R * pix : 0;
  const std::pair<const void*, size_t> ins[4] = {
      {logits, logits_b}, {labels, R * sizeof(int)}, {boxes, R * 16}, {image_hw, (size_t)N * 2 * sizeof(float)}};
  bool clash = out && binary && overlaps(out, out_b, binary, bin_b);
  for (const auto& in : ins)
    clash = clash || (out && overlaps(out, out_b, in.first, in.second)) ||
            (binary && overlaps(binary, bin_b, in.first, in.second));
  if (clash) {
    set_error("mask_paste: out and binary must not overlap logits, labels, boxes, image_hw or each other");
    return WINO_E_ARG;
  }
  PasteArgs a;
  a.logits = logits, a.labels = labels, a.boxes = boxes, a.image_hw = image_hw;
  a.out = out, a.bin = (unsigned char*)binary;
  a.D = D, a.H = H, a.W = W, a.M = M, a.classes = classes, a.ld = ld, a.layout = layout;
  a.rowblocks = (H + ROWS - 1) / ROWS;
  a.scale = (float)((double)(M + 2) / M);   // (expand_masks divides in double; torch multiplies by it as fp32)
  a.threshold = threshold;
  const long long items = (long long)R * a.rowblocks;
  for (a.first = 0; a.first < items; a.first += MAX_BLOCKS) {
    const long long nb = items - a.first < MAX_BLOCKS ? items - a.first : MAX_BLOCKS;
    hipLaunchKernelGGL(mask_paste_kernel, dim3((unsigned)nb), dim3(THREADS), 0, (hipStream_t)s, a);
    if (int rc = launch_status("mask_paste_kernel")) return rc;
  }
  return WINO_OK;
}
