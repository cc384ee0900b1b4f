// Bilinear resize (torch's align_corners=False rule) of the class scores, with the label map in the same launch.
//
// wino_resize_bilinear_hw:  src [N][h(+2)][w(+2)][ld] (NHWC, the first C of ld columns) -> out [N][C][Ho][Wo] (NCHW,
//   torch's layout) and / or labels [N][Ho][Wo] (int32, the index of the largest of the C interpolated values).
//
// Coordinates are integers: per axis, with `in`, `out` the sizes and d the output index, num = max((2d+1) in - out, 0),
// i0 = num / (2 out), i1 = min(i0 + 1, in - 1), lambda = float(num - i0 * 2 out) / float(2 out).  No floating-point
// coordinate exists anywhere, so the taps are the right ones at any size (torch's fp32 source coordinate is off by
// 1e-4 relative beyond a few thousand pixels).  The value is (1-ly)((1-lx) a + lx b) + ly((1-lx) c + lx d) in fp32
// (the compiler contracts the sums into FMAs); all four taps are always multiplied, so a NaN or Inf under a zero
// weight still reaches the output (0 * NaN), as in torch when the sizes differ -- and here also when they are equal,
// where torch copies.
//
// Two forms, a pure function of the shape (plan_resize):
//   STAGED  The layer is an NHWC -> NCHW transpose with a 4-tap filter.  A workgroup owns R output rows x an x-segment
//           of S pixels of one image.  It loads the source rows i0(first row) .. i1(last row), columns i0(first x) ..
//           i1(last x), with 16-byte loads along the channels, into LDS as [row][class][column] with an odd column
//           pitch: the epilogue's lanes, neighbours in x, read neighbouring (or equal: broadcast) columns of one class
//           row, so no two lanes of a read meet on a bank with different addresses, and the odd pitch spreads the
//           loader's four 4-byte writes per lane.  Wave v of eight takes rows v, v + 8, ...: a row's y-coordinate is
//           wave-uniform.  A lane owns four consecutive x of the segment and computes their coordinates once.  Per
//           class it stores its four values with one 16-byte store when the address allows it (a row of an odd Wo
//           that starts off 16 bytes, or the last pixels of a row, go out as 4-byte stores), and carries the running
//           maximum for the labels, stored four at a time the same way.
//   DIRECT  Each lane owns one output column, walks output rows and gathers its four taps from global memory per
//           class.  Correct for every legal shape; taken when no block of one output row x 64 pixels fits in 64 KB of
//           LDS, or when an axis shrinks by more than 4x (most of a staged span would never be read).
#include "resize_coord.h"
#include "wino_common.h"

namespace wino {
namespace {

constexpr int LDS_LIMIT = 64 << 10;   // bytes per workgroup: two workgroups per CU
constexpr int STAGED_WAVES = 8;       // waves of a staged workgroup: one per output row of a full block
constexpr int STAGED_THREADS = 64 * STAGED_WAVES;
constexpr int MAX_DOWN = 4;           // staged up to this down-scale factor per axis

// torch.argmax's order: larger wins, a tie keeps the lower index, a NaN beats every number and the first NaN stays.
// Branch-free (selects); the running maximum starts at -Inf with index 0, so class 0 needs no case of its own: a
// first value of -Inf leaves index 0, a first NaN takes it.
__device__ __forceinline__ void take_max(float v, int c, float& best, int& idx) {
  const bool take = (v > best) | ((v != v) & (best == best));
  best = take ? v : best;
  idx = take ? c : idx;
}

// Source rows / columns that `n` consecutive outputs of an axis span at most: i0 moves by at most ceil((n-1) in / out),
// plus i0's own row and i1's.
inline long span_max(int n, int in, int out) {
  const long s = ((long)(n - 1) * in + out - 1) / out + 2;
  return s < in ? s : in;
}

struct Plan {
  int form;
  int R, S, segs;          // staged: output rows and pixels per workgroup, segments per row
  int rows_max, pitch;     // staged: source rows held, column pitch (odd, >= the columns held)
  int lds_bytes;
};

long staged_bytes(int h, int w, int C, int Ho, int Wo, int R, int S, int* rows_max, int* pitch) {
  const long rows = span_max(R, h, Ho), cols = span_max(S, w, Wo) | 1;
  *rows_max = (int)rows;
  *pitch = (int)cols;
  return rows * cols * C * 4;
}

// The shape rules are the caller's.  Staged candidates: R from 8 down, S from the balanced segment (at most 256
// pixels, a multiple of 4) down to 64.
Plan plan_resize(int h, int w, int C, int Ho, int Wo) {
  Plan p = {WINO_RESIZE_FORM_DIRECT, 0, 0, 0, 0, 0, 0};
  int rm, pt;
  if ((long)h > (long)MAX_DOWN * Ho || (long)w > (long)MAX_DOWN * Wo) return p;
  if (staged_bytes(h, w, C, Ho, Wo, 1, 64, &rm, &pt) > LDS_LIMIT) return p;
  const int segs0 = (Wo + 255) / 256;
  const int S0 = ((Wo + segs0 - 1) / segs0 + 3) / 4 * 4;
  const int cand[3] = {S0, 128, 64};
  for (int R = 8; R >= 1; R >>= 1)
    for (int S : cand) {
      if (S > S0) continue;
      const long b = staged_bytes(h, w, C, Ho, Wo, R, S, &rm, &pt);
      if (b > LDS_LIMIT) continue;
      p = {WINO_RESIZE_FORM_STAGED, R, S, (Wo + S - 1) / S, rm, pt, (int)b};
      return p;
    }
  // S0 < 64 and it did not fit although a 64-pixel block does: cannot happen (a narrower segment spans no more)
  return p;
}

__global__ __launch_bounds__(STAGED_THREADS, 6) void resize_staged_kernel(const float* __restrict__ src,
                                                                       float* __restrict__ out, int* __restrict__ labels,
                                                                       int h, int w, int C, int ld, int pad, int Ho, int Wo,
                                                                       int R, int S, int segs, int rows_max, int pitch) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  const int seg = blockIdx.x % segs, rb = blockIdx.x / segs;
  const int y_first = rb * R, x_first = seg * S;
  if (y_first >= Ho || x_first >= Wo) return;
  const int y_last = (y_first + R < Ho ? y_first + R : Ho) - 1;
  const int x_last = (x_first + S < Wo ? x_first + S : Wo) - 1;
  const int ys0 = coord(y_first, h, Ho).i0, xs0 = coord(x_first, w, Wo).i0;
  const int nr = coord(y_last, h, Ho).i1 - ys0 + 1, nc = coord(x_last, w, Wo).i1 - xs0 + 1;
  if (nr > rows_max || nc > pitch) return;   // (span_max bounds both: never taken; nothing is written out of the LDS)

  const int RW = w + 2 * pad;
  const float* sn = src + (size_t)blockIdx.y * (h + 2 * pad) * RW * ld;
  const int c4n = (C + 3) >> 2;              // 16-byte units per pixel: c4n * 4 <= ld
  const unsigned units = (unsigned)nr * nc * c4n;
  for (unsigned u = tid; u < units; u += (unsigned)STAGED_THREADS) {
    const unsigned pix = u / c4n, c4 = u - pix * c4n;
    const unsigned row = pix / nc, col = pix - row * nc;
    const f32x4 v = *(const f32x4*)(sn + ((size_t)(ys0 + row + pad) * RW + (xs0 + col + pad)) * ld + c4 * 4);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int c = (int)c4 * 4 + i;
      if (c < C) lds[(row * C + c) * pitch + col] = v[i];
    }
  }
  __syncthreads();

  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int x = x_first + 4 * lane;
  const int valid = x > x_last ? 0 : (x_last - x + 1 < 4 ? x_last - x + 1 : 4);
  int c0[4], c1[4];
  float lx[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const Coord cx = coord(x + j <= x_last ? x + j : x_last, w, Wo);   // (lanes past the segment stay inside it)
    c0[j] = cx.i0 - xs0;
    c1[j] = cx.i1 - xs0;
    lx[j] = cx.lam;
  }
  const size_t plane = (size_t)Ho * Wo;
  float* on = out ? out + (size_t)blockIdx.y * C * plane : nullptr;
  int* ln = labels ? labels + (size_t)blockIdx.y * plane : nullptr;
  for (int y = y_first + wave; y <= y_last; y += STAGED_WAVES) {
    const Coord cy = coord(y, h, Ho);
    const float* p0 = lds + (cy.i0 - ys0) * C * pitch;
    const float* p1 = lds + (cy.i1 - ys0) * C * pitch;
    const size_t off = (size_t)y * Wo + x;
    float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int idx[4] = {0, 0, 0, 0};
    // Not unrolled, and built for six waves per SIMD (launch bounds): measured at N = 8, 65x65x21 -> 520x520, unrolling
    // by 3 (98 VGPRs, four waves) costs 12 % against this loop (69 VGPRs); at N = 1 the two are equal.
#pragma unroll 1
    for (int c = 0; c < C; c++, p0 += pitch, p1 += pitch) {
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; j++) v[j] = lerp2(p0[c0[j]], p0[c1[j]], p1[c0[j]], p1[c1[j]], lx[j], cy.lam);
      if (on) {
        float* o = on + (size_t)c * plane + off;
        if (valid == 4 && (reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
          *(f32x4*)o = v;
        } else {
#pragma unroll
          for (int j = 0; j < 4; j++)
            if (j < valid) o[j] = v[j];
        }
      }
      if (ln) {
#pragma unroll
        for (int j = 0; j < 4; j++) take_max(v[j], c, best[j], idx[j]);
      }
    }
    if (ln) {
      int* o = ln + off;
      if (valid == 4 && (reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
        *(int4*)o = make_int4(idx[0], idx[1], idx[2], idx[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (j < valid) o[j] = idx[j];
      }
    }
  }
}

// grid.x = xchunks * rowgroups: 256 output columns of one row group; a lane's column is fixed, rows stride by rowgroups
__global__ __launch_bounds__(256) void resize_direct_kernel(const float* __restrict__ src, float* __restrict__ out,
                                                            int* __restrict__ labels, int h, int w, int C, int ld,
                                                            int pad, int Ho, int Wo, int xchunks) {
  const int xc = blockIdx.x % xchunks, rg = blockIdx.x / xchunks, rgs = gridDim.x / xchunks;
  const int x = xc * 256 + (int)threadIdx.x;
  if (x >= Wo) return;
  const Coord cx = coord(x, w, Wo);
  const int RW = w + 2 * pad;
  const float* sn = src + (size_t)blockIdx.y * (h + 2 * pad) * RW * ld;
  const size_t plane = (size_t)Ho * Wo;
  float* on = out ? out + (size_t)blockIdx.y * C * plane : nullptr;
  int* ln = labels ? labels + (size_t)blockIdx.y * plane : nullptr;
  for (int y = rg; y < Ho; y += rgs) {
    const Coord cy = coord(y, h, Ho);
    const float* r0 = sn + (size_t)(cy.i0 + pad) * RW * ld;
    const float* r1 = sn + (size_t)(cy.i1 + pad) * RW * ld;
    const size_t k0 = (size_t)(cx.i0 + pad) * ld, k1 = (size_t)(cx.i1 + pad) * ld;
    const size_t off = (size_t)y * Wo + x;
    float best = -INFINITY;
    int idx = 0;
    for (int c = 0; c < C; c++) {
      const float v = lerp2(r0[k0 + c], r0[k1 + c], r1[k0 + c], r1[k1 + c], cx.lam, cy.lam);
      if (on) on[(size_t)c * plane + off] = v;
      take_max(v, c, best, idx);
    }
    if (ln) ln[off] = idx;
  }
}

// The rules both entry points share; want_out / want_labels say which images must fit 32-bit offsets.
int check_resize_shape(int N, int h, int w, int C, int ld, int in_padded, int Ho, int Wo, bool want_out,
                       bool want_labels) {
  if (N < 1 || h < 1 || w < 1 || Ho < 1 || Wo < 1 || C < 1 || C > ld || (ld % 4) != 0 ||
      (in_padded != 0 && in_padded != 1)) {
    set_error("resize: unsupported shape N=%d h=%d w=%d C=%d ld=%d in_padded=%d Ho=%d Wo=%d (need N, h, w, Ho, Wo >= 1, "
              "1 <= C <= ld, ld %% 4 == 0, in_padded 0 or 1)", N, h, w, C, ld, in_padded, Ho, Wo);
    return WINO_E_SHAPE;
  }
  const unsigned long long lim = 1ull << 31;
  const unsigned long long pix_in = (unsigned long long)(h + 2ll * in_padded) * (unsigned long long)(w + 2ll * in_padded);
  const unsigned long long pix_out = (unsigned long long)Ho * Wo;
  if (pix_in >= lim || pix_in * ld >= lim || pix_out >= lim || (want_out && pix_out * C >= lim)) {
    set_error("resize: one image of src %dx%dx%d, of out %dx%dx%d or of labels exceeds 32-bit offsets", h, w, ld, C, Ho,
              Wo);
    return WINO_E_SHAPE;
  }
  (void)want_labels;   // (labels' image is the smallest of the three: covered by pix_out)
  if (2ull * Ho * h >= lim || 2ull * Wo * w >= lim) {
    set_error("resize: 2*Ho*h = %llu or 2*Wo*w = %llu is not below 2^31", 2ull * Ho * h, 2ull * Wo * w);
    return WINO_E_SHAPE;
  }
  return WINO_OK;
}

}  // namespace
}  // namespace wino

using namespace wino;

extern "C" {

int wino_resize_bilinear_plan(int h, int w, int C, int ld, int Ho, int Wo, int want_out, int want_labels, int* form) {
  if (!form) {
    set_error("NULL pointer");
    return WINO_E_ARG;
  }
  if (!want_out && !want_labels) {
    set_error("resize: neither out nor labels is wanted");
    return WINO_E_ARG;
  }
  if (int rc = check_resize_shape(1, h, w, C, ld, 0, Ho, Wo, want_out != 0, want_labels != 0)) return rc;
  *form = plan_resize(h, w, C, Ho, Wo).form;
  return WINO_OK;
}

int wino_resize_bilinear_hw(const float* src, float* out, int* labels, int N, int h, int w, int C, int ld,
                            int in_padded, int Ho, int Wo, wino_stream_t s) {
  if (int rc = check_nonnull(src)) return rc;
  if (!out && !labels) {
    set_error("resize: out and labels are both NULL");
    return WINO_E_ARG;
  }
  if (int rc = check_aligned16(src, out, labels)) return rc;
  if (int rc = check_resize_shape(N, h, w, C, ld, in_padded, Ho, Wo, out != nullptr, labels != nullptr)) return rc;
  const size_t img_in = (size_t)(h + 2 * in_padded) * (w + 2 * in_padded) * ld;
  const size_t img_lab = (size_t)Ho * Wo, img_out = img_lab * C;
  const size_t in_b = (size_t)N * img_in * sizeof(float);
  const size_t out_b = out ? (size_t)N * img_out * sizeof(float) : 0, lab_b = labels ? (size_t)N * img_lab * sizeof(int) : 0;
  if ((out && overlaps(src, in_b, out, out_b)) || (labels && overlaps(src, in_b, labels, lab_b)) ||
      (out && labels && overlaps(out, out_b, labels, lab_b))) {
    set_error("src, out and labels must not overlap");
    return WINO_E_ARG;
  }
  const Plan p = plan_resize(h, w, C, Ho, Wo);
  if (p.form == WINO_RESIZE_FORM_STAGED) {
    int dev, cus;
    if (int rc = current_device(&dev, &cus)) return rc;
    if (int rc = lds_cap_once<resize_staged_kernel>(dev, LDS_LIMIT)) return rc;
  }
  for (int n0 = 0; n0 < N; n0 += 65535) {   // gridDim.y
    const int n = N - n0 < 65535 ? N - n0 : 65535;
    const float* sp = src + (size_t)n0 * img_in;
    float* op = out ? out + (size_t)n0 * img_out : nullptr;
    int* lp = labels ? labels + (size_t)n0 * img_lab : nullptr;
    if (p.form == WINO_RESIZE_FORM_STAGED) {
      const unsigned blocks = (unsigned)p.segs * (unsigned)((Ho + p.R - 1) / p.R);
      hipLaunchKernelGGL(resize_staged_kernel, dim3(blocks, (unsigned)n), dim3(STAGED_THREADS), (size_t)p.lds_bytes, (hipStream_t)s,
                         sp, op, lp, h, w, C, ld, in_padded, Ho, Wo, p.R, p.S, p.segs, p.rows_max, p.pitch);
      if (int rc = launch_status("resize_staged_kernel")) return rc;
    } else {
      const int xchunks = (Wo + 255) / 256;
      int rgs = 2048 / xchunks;
      rgs = rgs < 1 ? 1 : rgs > Ho ? Ho : rgs;
      hipLaunchKernelGGL(resize_direct_kernel, dim3((unsigned)xchunks * rgs, (unsigned)n), dim3(256), 0, (hipStream_t)s,
                         sp, op, lp, h, w, C, ld, in_padded, Ho, Wo, xchunks);
      if (int rc = launch_status("resize_direct_kernel")) return rc;
    }
  }
  return WINO_OK;
}

}  // extern "C"
