// Depthwise 3x3 convolution (stride 1 or 2, pad 1) + folded BN + activation on the padded NHWC maps
// [N][h+2][w+2][C] fp32 that the 3x3 layers and the WINO_C_PADDED 1x1 layers write:
//   out[n][y][x][c] = act(bnScale[c] * sum_{dy,dx} w_taps[dy][dx][c] * min(in[n][s y + dy][s x + dx][c], in_cap) + bnBias[c])
// Plain HIP: no MFMA (a contraction of length nine and nothing shared between channels leaves the matrix pipe nothing
// to do; the layer moves 8 bytes per 18 FLOP and is bound by memory), no inline assembly, no atomics, no scratch.
//
// Lanes and channels.  A workgroup of 256 threads owns TH x TW output pixels of one image for a channel block of CB
// channels (64 or 16).  Thread t is quad t % QPP (QPP = CB / 4) of tile column (t / QPP) % TW in row group
// t / (QPP TW): a thread's channel quad never changes, so its nine tap quads, its bias and its scale quad (44 VGPRs) are
// loaded once; neighbouring lanes hold neighbouring quads, so every global and LDS access is 16 bytes and a wave's
// accesses are whole runs of CB channels of consecutive pixels.  A quad at or past C (a ragged last block, C % 4 == 0)
// idles.
//
// LDS.  The workgroup first stages the (s (TH-1) + 3) x (s (TW-1) + 3) x CB input patch, in_cap applied to interior
// pixels on the way in (the ring is taken as it is: the zero ring stays zero under any cap); positions outside the
// padded input are staged as 0 and feed only outputs that are never stored.  After one barrier every thread walks down
// its RPL = TH / row groups output rows with a 3 x 3 window of quads in registers: 3 s new LDS reads per output (the
// 16-channel form has one row per thread and reads all nine).
//
// Arithmetic order, part of the contract: acc = 0, then acc = fma(w[dy][dx], v[dy][dx], acc) in tap order (0,0) ..
// (2,2), y = fma(scale, acc, bias), the activation.  Every instantiation gives the same bits.
//
// Ring.  Workgroups on an edge of the tile grid write their segment of the output ring as zeros.
//
// Instantiations, stride x CB (wino_dwconv3x3_plan names the one a call takes, WINO_DW_CB = 64 | 16 forces CB):
//   <1, 64>  8 x 8 tile, 2 row groups of 4 rows, 10 x 10 x 64 patch: 25600 bytes
//   <2, 64>  4 x 8 tile, 2 row groups of 2 rows,  9 x 17 x 64 patch: 39168 bytes
//   <1, 16>  8 x 8 tile, 8 row groups of 1 row,  10 x 10 x 16 patch:  6400 bytes
//   <2, 16>  8 x 8 tile, 8 row groups of 1 row,  17 x 17 x 16 patch: 18496 bytes
// The rule between the blocks: DESIGN.md section 3.2u.
#include <cmath>

#include "wino_common.h"

#pragma clang fp contract(off)

namespace wino {
namespace {

constexpr int DW_THREADS = 256;
constexpr int DW_TW = 8;
__host__ __device__ constexpr int dw_tile_h(int stride, int cb) { return stride == 2 && cb == 64 ? 4 : 8; }

template <int STRIDE, int CB>
struct DwTile {
  static constexpr int QPP = CB / 4;                      // channel quads of a pixel
  static constexpr int TW = DW_TW, TH = dw_tile_h(STRIDE, CB);
  static constexpr int RG = DW_THREADS / (QPP * TW);      // row groups
  static constexpr int RPL = TH / RG;                     // output rows of a thread
  static constexpr int IH = STRIDE * (TH - 1) + 3, IW = STRIDE * (TW - 1) + 3;
  static constexpr unsigned ITEMS = IH * IW * QPP;        // quads of the patch
  static_assert(RG * RPL == TH && RG * QPP * TW == DW_THREADS, "the threads tile the tile");
};

struct DwArgs {
  const float* in;
  const float* w;            // [3][3][C]
  const float* bias;
  const float* scale;
  float* out;
  long long in_image, out_image;   // elements of one padded image
  unsigned Hin, Win, H, W, C;
  unsigned tiles_y, tiles_x, cblks;
  int act;
  float cap;
  FastDiv divC, divX, divY;
};

// NaN-propagating, as relu_nan: a NaN fails every compare and passes through
__device__ __forceinline__ float cap_nan(float v, float cap) { return v > cap ? cap : v; }
__device__ __forceinline__ float act_nan(float y, int act) {
  if (act == WINO_ACT_NONE) return y;
  y = relu_nan(y);
  return act == WINO_ACT_RELU6 ? cap_nan(y, 6.0f) : y;
}

// blockIdx.x = ((n tiles_y + ty) tiles_x + tx) cblks + cblk
template <int STRIDE, int CB>
__global__ __launch_bounds__(DW_THREADS) void dw_kernel(const DwArgs a) {
  using T = DwTile<STRIDE, CB>;
  __shared__ f32x4 patch[T::ITEMS];
  const unsigned t = threadIdx.x;
  unsigned r = fastdiv(blockIdx.x, a.divC);
  const unsigned cblk = blockIdx.x - r * a.cblks;
  const unsigned r2 = fastdiv(r, a.divX), tx = r - r2 * a.tiles_x;
  const unsigned n = fastdiv(r2, a.divY), ty = r2 - n * a.tiles_y;
  const unsigned q = t % T::QPP, c = cblk * CB + 4u * q;
  const bool live = c < a.C;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  // the thread's constants, asked for before the patch so that they arrive under it
  f32x4 wt[9], bs = zero, sc = zero;
#pragma unroll
  for (int k = 0; k < 9; k++) wt[k] = zero;
  if (live) {
#pragma unroll
    for (int k = 0; k < 9; k++) wt[k] = *(const f32x4*)(a.w + (size_t)k * a.C + c);
    bs = *(const f32x4*)(a.bias + c), sc = *(const f32x4*)(a.scale + c);
  }

  // ---- stage the input patch: padded input rows iy0 .., columns ix0 ..
  const float* img = a.in + (size_t)n * (size_t)a.in_image;
  const unsigned iy0 = ty * (T::TH * STRIDE), ix0 = tx * (T::TW * STRIDE);
  const unsigned pitch = (a.Win + 2u) * a.C;
  for (unsigned e0 = t; e0 < T::ITEMS; e0 += 4u * DW_THREADS) {
    f32x4 v[4];
    bool inner[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const unsigned e = e0 + (unsigned)u * DW_THREADS;
      const unsigned pix = e / T::QPP, py = pix / T::IW, px = pix - py * T::IW;
      const unsigned gy = iy0 + py, gx = ix0 + px;
      v[u] = zero;
      inner[u] = gy - 1u < a.Hin && gx - 1u < a.Win;
      if (live && e < T::ITEMS && gy <= a.Hin + 1u && gx <= a.Win + 1u) v[u] = *(const f32x4*)(img + (gy * pitch + gx * a.C + c));
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const unsigned e = e0 + (unsigned)u * DW_THREADS;
      if (e < T::ITEMS) {
        f32x4 x = v[u];
        if (inner[u]) {
#pragma unroll
          for (int j = 0; j < 4; j++) x[j] = cap_nan(x[j], a.cap);
        }
        patch[e] = x;
      }
    }
  }
  __syncthreads();
  if (!live) return;   // (no barrier follows)

  // ---- the thread's column of outputs
  float* oimg = a.out + (size_t)n * (size_t)a.out_image;
  const unsigned opitch = (a.W + 2u) * a.C;
  const unsigned col = (t / T::QPP) % T::TW, g = t / (T::QPP * T::TW);
  const unsigned ox = tx * T::TW + col, oy0 = ty * T::TH + g * T::RPL;
  const f32x4* p = patch + ((g * T::RPL * STRIDE) * T::IW + col * STRIDE) * T::QPP + q;
  constexpr int KEEP = 3 - STRIDE;   // window rows an output hands to the next one below it
  f32x4 win[3][3];
#pragma unroll
  for (int i = 0; i < KEEP; i++)
#pragma unroll
    for (int dx = 0; dx < 3; dx++) win[i][dx] = p[(i * T::IW + dx) * T::QPP];
#pragma unroll
  for (int j = 0; j < T::RPL; j++) {
#pragma unroll
    for (int i = KEEP; i < 3; i++)
#pragma unroll
      for (int dx = 0; dx < 3; dx++) win[i][dx] = p[((j * STRIDE + i) * T::IW + dx) * T::QPP];
    f32x4 y;
#pragma unroll
    for (int ch = 0; ch < 4; ch++) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < 9; k++) acc = __builtin_fmaf(wt[k][ch], win[k / 3][k % 3][ch], acc);
      y[ch] = act_nan(__builtin_fmaf(sc[ch], acc, bs[ch]), a.act);
    }
    const unsigned oy = oy0 + (unsigned)j;
    if (oy < a.H && ox < a.W) *(f32x4*)(oimg + ((oy + 1u) * opitch + (ox + 1u) * a.C + c)) = y;
#pragma unroll
    for (int i = 0; i < KEEP; i++)
#pragma unroll
      for (int dx = 0; dx < 3; dx++) win[i][dx] = win[i + STRIDE][dx];
  }

  // ---- the output ring: an edge tile zeroes the ring pixels of its tile grown by one pixel on every side
  if (ty == 0u || tx == 0u || ty + 1u == a.tiles_y || tx + 1u == a.tiles_x) {
    constexpr unsigned EW = T::TW + 2, EITEMS = (T::TH + 2) * EW * T::QPP;
    for (unsigned e = t; e < EITEMS; e += DW_THREADS) {
      const unsigned pix = e / T::QPP, ey = pix / EW, ex = pix - ey * EW;
      const unsigned py = ty * T::TH + ey, px = tx * T::TW + ex;   // padded output coordinates
      const bool ring = py == 0u || px == 0u || py == a.H + 1u || px == a.W + 1u;
      if (ring && py <= a.H + 1u && px <= a.W + 1u) *(f32x4*)(oimg + (py * opitch + px * a.C + c)) = zero;
    }
  }
}

// ---- host: limits and the plan ----------------------------------------------------------------------------------------
struct DwPlan {
  int cb, th, tw;
  unsigned H, W, tiles_y, tiles_x, cblks;
  unsigned long long in_image, out_image, grid;
};

unsigned long long dw_grid(int N, unsigned H, unsigned W, int C, int stride, int cb, DwPlan* p) {
  p->cb = cb, p->th = dw_tile_h(stride, cb), p->tw = DW_TW;
  p->tiles_y = (H + (unsigned)p->th - 1u) / (unsigned)p->th, p->tiles_x = (W + (unsigned)p->tw - 1u) / (unsigned)p->tw;
  p->cblks = ((unsigned)C + (unsigned)cb - 1u) / (unsigned)cb;
  return p->grid = (unsigned long long)N * p->tiles_y * p->tiles_x * p->cblks;
}

// WINO_OK, or the layer's refusal of the shape (the error text set)
int dw_plan(int N, int Hin, int Win, int C, int stride, int cus, DwPlan* p) {
  if (N < 0 || Hin < 1 || Win < 1 || C < 4 || C % 4) {
    set_error("dwconv3x3: unsupported shape N=%d Hin=%d Win=%d C=%d (need N >= 0, Hin, Win >= 1, C a multiple of 4)", N, Hin,
              Win, C);
    return WINO_E_SHAPE;
  }
  if (stride != 1 && stride != 2) {
    set_error("dwconv3x3: stride must be 1 or 2, got %d", stride);
    return WINO_E_ARG;
  }
  p->H = (unsigned)(Hin - 1) / (unsigned)stride + 1u, p->W = (unsigned)(Win - 1) / (unsigned)stride + 1u;
  p->in_image = (unsigned long long)(Hin + 2ll) * (unsigned long long)(Win + 2ll) * (unsigned long long)C;
  p->out_image = (unsigned long long)(p->H + 2ull) * (p->W + 2ull) * (unsigned long long)C;
  if (p->in_image >= (1ull << 31)) {
    set_error("dwconv3x3: one padded image must stay below 2^31 elements (Hin=%d Win=%d C=%d)", Hin, Win, C);
    return WINO_E_SHAPE;
  }
  // 16 channels per workgroup when 64 would leave compute units without one
  const int forced = knobs().dw_cb;
  DwPlan wide;
  const unsigned long long grid64 = dw_grid(N, p->H, p->W, C, stride, 64, &wide);
  const int cb = forced == 64 || forced == 16 ? forced : (grid64 < (unsigned long long)cus ? 16 : 64);
  if (dw_grid(N, p->H, p->W, C, stride, cb, p) > 0x7fffffffull) {
    set_error("dwconv3x3: %llu workgroups (N=%d Hin=%d Win=%d C=%d): the launch holds 2^31 - 1", p->grid, N, Hin, Win, C);
    return WINO_E_SHAPE;
  }
  return WINO_OK;
}

template <int STRIDE, int CB>
int dw_launch(const DwArgs& a, unsigned grid, hipStream_t s) {
  hipLaunchKernelGGL((dw_kernel<STRIDE, CB>), dim3(grid), dim3(DW_THREADS), 0, s, a);
  return launch_status("dw_kernel");
}

}  // namespace
}  // namespace wino

using namespace wino;

extern "C" int wino_dwconv3x3_plan(int N, int Hin, int Win, int C, int stride, int cus, int* cb, int* tile_h, int* tile_w,
                                   int* tiles_y, int* tiles_x) {
  if (int rc = check_nonnull(cb, tile_h, tile_w, tiles_y, tiles_x)) return rc;
  if (cus < 1) {
    set_error("dwconv3x3_plan: cus must be >= 1");
    return WINO_E_ARG;
  }
  DwPlan p;
  if (int rc = dw_plan(N, Hin, Win, C, stride, cus, &p)) return rc;
  *cb = p.cb, *tile_h = p.th, *tile_w = p.tw, *tiles_y = (int)p.tiles_y, *tiles_x = (int)p.tiles_x;
  return WINO_OK;
}

extern "C" int wino_dwconv3x3_bn_act_hw(const float* in, const float* w_taps, const float* bnBias, const float* bnScale,
                                        float* out, int N, int Hin, int Win, int C, int stride, int act, float in_cap,
                                        wino_stream_t s) {
  DwPlan p;
  if (int rc = dw_plan(N, Hin, Win, C, stride, 256, &p)) return rc;   // the limits do not depend on the device
  if (act != WINO_ACT_NONE && act != WINO_ACT_RELU && act != WINO_ACT_RELU6) {
    set_error("dwconv3x3: unknown act %d", act);
    return WINO_E_ARG;
  }
  if (std::isnan(in_cap)) {
    set_error("dwconv3x3: in_cap must not be NaN (+inf switches it off)");
    return WINO_E_ARG;
  }
  if (N == 0) return WINO_OK;
  if (int rc = check_nonnull(in, w_taps, bnBias, bnScale, out)) return rc;
  if (int rc = check_aligned16(in, w_taps, bnBias, bnScale, out)) return rc;
  const size_t in_b = (size_t)N * (size_t)p.in_image * 4, out_b = (size_t)N * (size_t)p.out_image * 4, vec_b = (size_t)C * 4;
  if (overlaps(in, in_b, out, out_b) || overlaps(w_taps, 9 * vec_b, out, out_b) || overlaps(bnBias, vec_b, out, out_b) ||
      overlaps(bnScale, vec_b, out, out_b)) {
    set_error("dwconv3x3: out must not overlap in, w_taps or the BN vectors");
    return WINO_E_ARG;
  }
  int dev = 0, cus = 256;
  if (int rc = current_device(&dev, &cus)) return rc;
  if (int rc = dw_plan(N, Hin, Win, C, stride, cus, &p)) return rc;
  DwArgs a;
  a.in = in, a.w = w_taps, a.bias = bnBias, a.scale = bnScale, a.out = out;
  a.in_image = (long long)p.in_image, a.out_image = (long long)p.out_image;
  a.Hin = (unsigned)Hin, a.Win = (unsigned)Win, a.H = p.H, a.W = p.W, a.C = (unsigned)C;
  a.tiles_y = p.tiles_y, a.tiles_x = p.tiles_x, a.cblks = p.cblks;
  a.act = act, a.cap = in_cap;
  a.divC = make_fastdiv(p.cblks), a.divX = make_fastdiv(p.tiles_x), a.divY = make_fastdiv(p.tiles_y);
  const unsigned grid = (unsigned)p.grid;
  hipStream_t st = (hipStream_t)s;
  if (p.cb == 64) return stride == 1 ? dw_launch<1, 64>(a, grid, st) : dw_launch<2, 64>(a, grid, st);
  return stride == 1 ? dw_launch<1, 16>(a, grid, st) : dw_launch<2, 16>(a, grid, st);
}
