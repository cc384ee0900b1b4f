// Depthwise K x K convolution, K = 3 or 5 (stride 1 or 2, pad K / 2) + folded BN + activation on the padded NHWC maps
// [N][h+2][w+2][C] fp32, with an activation applied to the input as it is staged and, optionally, the per-tile channel
// sums of what the launch stored (the squeeze of a squeeze-excite block):
//   out[n][y][x][c] = act(bnScale[c] * sum_{dy,dx} w_taps[dy][dx][c] * in_act(in[n][s y + dy - K/2 + 1][s x + dx - K/2 + 1][c]) + bnBias[c])
// (padded input coordinates; a position outside the padded input counts as 0).  The layer of MobileNetV3's blocks;
// depthwise.hip, the 3x3 of MobileNetV2, stays as it is.  Plain HIP: no MFMA (25 taps share nothing between channels any
// more than nine do), no inline assembly, no atomics, no scratch.
//
// Lanes and channels, as in depthwise.hip.  A workgroup of 256 threads owns TH x TW output pixels of one image for a
// block of CB channels (64 or 16).  Thread t is quad t % QPP (QPP = CB / 4) of tile column (t / QPP) % TW in row group
// t / (QPP TW); its channel quad never changes, so its bias and scale quads and, for K = 3, its nine tap quads live in
// registers, and every global and LDS access is 16 bytes.
//
// LDS.  The workgroup stages the (s (TH-1) + K) x (s (TW-1) + K) x CB input patch once, in_act applied to interior
// pixels on the way in (the ring is taken as read: every in_act maps 0 to 0).  The maps carry one ring pixel and a 5 x 5
// reaches two, so the patch starts K/2 - 1 pixels outside the padded input; positions outside it are staged as 0 and,
// unlike in the 3x3, feed outputs that are stored.
//
// Streaming rows.  A 5 x 5 register window would be 100 VGPRs.  Instead a thread walks down the s (RPL-1) + K patch rows
// of its column once and feeds each row's K quads into the accumulators of the output rows o the row touches
// (dy = r - s o in [0, K)), so it holds one row and RPL accumulators.  Each accumulator still receives its products in
// tap order (0,0) .. (K-1,K-1): rows arrive in rising dy and dx rises inside a row.  The contract: acc = 0, K K fma in
// tap order, y = fma(scale, acc, bias), the activation -- every instantiation gives the same map bits, and K = 3 with
// in_act NONE the bits of wino_dwconv3x3_bn_act_hw.
//
// Taps.  K = 3: nine quads in registers, the walk fully unrolled.  K = 5 (TAPS_LDS): 25 quads would be 100 VGPRs, and the
// compiler hoists an unrolled walk's LDS reads on top of them (213 to 256 VGPRs, or spills when held to fewer), so the
// workgroup keeps a copy of its taps in LDS, [25][QPP] quads beside the patch, and the row loop stays rolled: per row K
// data quads, then per touched output row K tap quads and 4 K fma.  60 to 74 VGPRs; the price is LDS traffic.
//
// Pool partials (POOL).  Each thread adds up the outputs it stored (post-activation; a pixel past H or W adds nothing)
// in row order; after a barrier the sums go through the first 4 KiB of the patch and quad q's thread adds the 256 / QPP
// of them in (row group, column) order and stores one quad of pool_partials[n][tile][C].  No atomics: deterministic.
// The tiles of the two channel blocks differ, so their partials may.
//
// Instantiations, K x stride x CB x pool (wino_dwconv_plan names the one a call takes, WINO_DW_CB forces CB); tile and
// patch bytes, the same with and without the pool (K = 5 adds its tap copy, 25 CB 4 bytes):
//   K = 3  <1, 64> 8 x 8, 10 x 10 x 64: 25600   <2, 64> 4 x 8,  9 x 17 x 64: 39168
//          <1, 16> 8 x 8, 10 x 10 x 16:  6400   <2, 16> 8 x 8, 17 x 17 x 16: 18496
//   K = 5  <1, 64> 8 x 8, 12 x 12 x 64: 36864   <2, 64> 4 x 8, 11 x 19 x 64: 53504
//          <1, 16> 8 x 8, 12 x 12 x 16:  9216   <2, 16> 8 x 8, 19 x 19 x 16: 23104
// The tile rule is the 3x3's; DESIGN.md section 3.2v has the registers and the occupancy of each.
#include "wino_act.h"

#pragma clang fp contract(off)

namespace wino {
namespace {

constexpr int DX_THREADS = 256;
constexpr int DX_TW = 8;
__host__ __device__ constexpr int dx_tile_h(int stride, int cb) { return stride == 2 && cb == 64 ? 4 : 8; }

template <int K, int STRIDE, int CB>
struct DxTile {
  static constexpr int QPP = CB / 4;                      // channel quads of a pixel
  static constexpr int TW = DX_TW, TH = dx_tile_h(STRIDE, CB);
  static constexpr int RG = DX_THREADS / (QPP * TW);      // row groups
  static constexpr int RPL = TH / RG;                     // output rows of a thread
  static constexpr int NR = STRIDE * (RPL - 1) + K;       // patch rows a thread walks
  static constexpr int IH = STRIDE * (TH - 1) + K, IW = STRIDE * (TW - 1) + K;
  static constexpr unsigned ITEMS = IH * IW * QPP;        // quads of the patch
  static constexpr bool TAPS_LDS = K == 5;                // the taps live in LDS, not in registers
  static constexpr unsigned OFF = K / 2 - 1;              // the patch starts this far outside the padded input
  static_assert(RG * RPL == TH && RG * QPP * TW == DX_THREADS, "the threads tile the tile");
  static_assert(ITEMS >= (unsigned)DX_THREADS, "the pool's sums fit the patch");
};

struct DxArgs {
  const float* in;
  const float* w;            // [K][K][C]
  const float* bias;
  const float* scale;
  float* out;
  float* pool;               // [N][tiles_y tiles_x][C] or null
  long long in_image, out_image;   // elements of one padded image
  unsigned Hin, Win, H, W, C;
  unsigned tiles_y, tiles_x, cblks;
  int act, in_act;
  FastDiv divC, divX, divY;
};

// blockIdx.x = ((n tiles_y + ty) tiles_x + tx) cblks + cblk
template <int K, int STRIDE, int CB, bool POOL>
__global__ __launch_bounds__(DX_THREADS) void dwx_kernel(const DxArgs a) {
  using T = DxTile<K, STRIDE, CB>;
  __shared__ f32x4 patch[T::ITEMS];
  __shared__ f32x4 taps[T::TAPS_LDS ? K * K * T::QPP : 1];
  const unsigned t = threadIdx.x;
  unsigned r = fastdiv(blockIdx.x, a.divC);
  const unsigned cblk = blockIdx.x - r * a.cblks;
  const unsigned r2 = fastdiv(r, a.divX), tx = r - r2 * a.tiles_x;
  const unsigned n = fastdiv(r2, a.divY), ty = r2 - n * a.tiles_y;
  const unsigned q = t % T::QPP, c = cblk * CB + 4u * q;
  const bool live = c < a.C;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  // the thread's constants, asked for before the patch so that they arrive under it; the 25 tap quads of a 5 x 5 go to
  // LDS instead (TAPS_LDS), [tap][quad], and are read back per product
  constexpr int NW = T::TAPS_LDS ? 1 : K * K;
  f32x4 wt[NW], bs = zero, sc = zero;
#pragma unroll
  for (int k = 0; k < NW; k++) wt[k] = zero;
  if (live) {
    if (!T::TAPS_LDS) {
#pragma unroll
      for (int k = 0; k < NW; k++) wt[k] = *(const f32x4*)(a.w + (size_t)k * a.C + c);
    }
    bs = *(const f32x4*)(a.bias + c), sc = *(const f32x4*)(a.scale + c);
  }
  if (T::TAPS_LDS) {
    for (unsigned e = t; e < (unsigned)(K * K * T::QPP); e += DX_THREADS) {
      const unsigned k = e / T::QPP, cc = cblk * CB + 4u * (e % T::QPP);
      taps[e] = cc < a.C ? *(const f32x4*)(a.w + (size_t)k * a.C + cc) : zero;
    }
  }

  // ---- stage the input patch: padded input rows iy0 - OFF .., columns ix0 - OFF .. (unsigned: a coordinate before the
  // padded input wraps to a huge one and fails the same compares as one past it)
  const float* img = a.in + (size_t)n * (size_t)a.in_image;
  const unsigned iy0 = ty * (T::TH * STRIDE) - T::OFF, ix0 = tx * (T::TW * STRIDE) - T::OFF;
  const unsigned pitch = (a.Win + 2u) * a.C;
  for (unsigned e0 = t; e0 < T::ITEMS; e0 += 4u * DX_THREADS) {
    f32x4 v[4];
    bool inner[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const unsigned e = e0 + (unsigned)u * DX_THREADS;
      const unsigned pix = e / T::QPP, py = pix / T::IW, px = pix - py * T::IW;
      const unsigned gy = iy0 + py, gx = ix0 + px;
      v[u] = zero;
      inner[u] = gy - 1u < a.Hin && gx - 1u < a.Win;
      if (live && e < T::ITEMS && gy <= a.Hin + 1u && gx <= a.Win + 1u) v[u] = *(const f32x4*)(img + (gy * pitch + gx * a.C + c));
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const unsigned e = e0 + (unsigned)u * DX_THREADS;
      if (e < T::ITEMS) patch[e] = inner[u] ? act_apply4(v[u], a.in_act) : v[u];
    }
  }
  __syncthreads();

  float* oimg = a.out + (size_t)n * (size_t)a.out_image;
  const unsigned opitch = (a.W + 2u) * a.C;
  f32x4 psum = zero;
  if (live) {
    // ---- the thread's column of outputs: one walk down its patch rows
    const unsigned col = (t / T::QPP) % T::TW, g = t / (T::QPP * T::TW);
    const unsigned ox = tx * T::TW + col, oy0 = ty * T::TH + g * T::RPL;
    const f32x4* p = patch + ((g * T::RPL * STRIDE) * T::IW + col * STRIDE) * T::QPP + q;
    f32x4 acc[T::RPL];
#pragma unroll
    for (int o = 0; o < T::RPL; o++) acc[o] = zero;
    if constexpr (!T::TAPS_LDS) {
#pragma unroll
      for (int row = 0; row < T::NR; row++) {
#pragma unroll
        for (int dx = 0; dx < K; dx++) {
          const f32x4 v = p[(row * T::IW + dx) * T::QPP];
#pragma unroll
          for (int o = 0; o < T::RPL; o++) {
            const int dy = row - STRIDE * o;
            if (dy >= 0 && dy < K) {
#pragma unroll
              for (int ch = 0; ch < 4; ch++) acc[o][ch] = __builtin_fmaf(wt[dy * K + dx][ch], v[ch], acc[o][ch]);
            }
          }
        }
      }
    } else {
      // a loop the compiler keeps rolled: unrolled, it hoists every LDS read of the walk and takes 213 to 256 VGPRs
#pragma unroll 1
      for (int row = 0; row < T::NR; row++) {
        f32x4 v[K];
#pragma unroll
        for (int dx = 0; dx < K; dx++) v[dx] = p[(row * T::IW + dx) * T::QPP];
#pragma unroll
        for (int o = 0; o < T::RPL; o++) {
          const int dy = row - STRIDE * o;   // (uniform over the workgroup)
          if (dy >= 0 && dy < K) {
            const f32x4* w = taps + dy * (K * T::QPP) + q;
#pragma unroll
            for (int dx = 0; dx < K; dx++) {
              const f32x4 wq = w[dx * T::QPP];
#pragma unroll
              for (int ch = 0; ch < 4; ch++) acc[o][ch] = __builtin_fmaf(wq[ch], v[dx][ch], acc[o][ch]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int o = 0; o < T::RPL; o++) {
      f32x4 y;
#pragma unroll
      for (int ch = 0; ch < 4; ch++) y[ch] = act_apply(__builtin_fmaf(sc[ch], acc[o][ch], bs[ch]), a.act);
      const unsigned oy = oy0 + (unsigned)o;
      if (oy < a.H && ox < a.W) {
        *(f32x4*)(oimg + ((oy + 1u) * opitch + (ox + 1u) * a.C + c)) = y;
        if (POOL) psum += y;
      }
    }

    // ---- the output ring: an edge tile zeroes the ring pixels of its tile grown by one pixel on every side
    if (ty == 0u || tx == 0u || ty + 1u == a.tiles_y || tx + 1u == a.tiles_x) {
      constexpr unsigned EW = T::TW + 2, EITEMS = (T::TH + 2) * EW * T::QPP;
      for (unsigned e = t; e < EITEMS; e += DX_THREADS) {
        const unsigned pix = e / T::QPP, ey = pix / EW, ex = pix - ey * EW;
        const unsigned py = ty * T::TH + ey, px = tx * T::TW + ex;   // padded output coordinates
        const bool ring = py == 0u || px == 0u || py == a.H + 1u || px == a.W + 1u;
        if (ring && py <= a.H + 1u && px <= a.W + 1u) *(f32x4*)(oimg + (py * opitch + px * a.C + c)) = zero;
      }
    }
  }

  // ---- the tile's channel sums: thread sums [row group][column][quad] through the patch, added in that order
  if (POOL) {
    __syncthreads();   // every thread is done with the patch
    patch[t] = psum;
    __syncthreads();
    if (t < T::QPP && live) {
      f32x4 s = patch[t];
#pragma unroll 8
      for (unsigned i = 1; i < DX_THREADS / T::QPP; i++) s += patch[t + i * T::QPP];
      const size_t tile = (size_t)n * (a.tiles_y * a.tiles_x) + (ty * a.tiles_x + tx);
      *(f32x4*)(a.pool + tile * a.C + c) = s;
    }
  }
}

// ---- host: limits and the plan ----------------------------------------------------------------------------------------
struct DxPlan {
  int cb, th, tw;
  unsigned H, W, tiles_y, tiles_x, cblks;
  unsigned long long in_image, out_image, grid;
};

unsigned long long dx_grid(int N, unsigned H, unsigned W, int C, int stride, int cb, DxPlan* p) {
  p->cb = cb, p->th = dx_tile_h(stride, cb), p->tw = DX_TW;
  p->tiles_y = (H + (unsigned)p->th - 1u) / (unsigned)p->th, p->tiles_x = (W + (unsigned)p->tw - 1u) / (unsigned)p->tw;
  p->cblks = ((unsigned)C + (unsigned)cb - 1u) / (unsigned)cb;
  return p->grid = (unsigned long long)N * p->tiles_y * p->tiles_x * p->cblks;
}

// WINO_OK, or the layer's refusal of the shape (the error text set)
int dx_plan(int N, int Hin, int Win, int C, int K, int stride, int cus, DxPlan* p) {
  if (N < 0 || Hin < 1 || Win < 1 || C < 4 || C % 4) {
    set_error("dwconv: unsupported shape N=%d Hin=%d Win=%d C=%d (need N >= 0, Hin, Win >= 1, C a multiple of 4)", N, Hin, Win,
              C);
    return WINO_E_SHAPE;
  }
  if (K != 3 && K != 5) {
    set_error("dwconv: K must be 3 or 5, got %d", K);
    return WINO_E_ARG;
  }
  if (stride != 1 && stride != 2) {
    set_error("dwconv: stride must be 1 or 2, got %d", stride);
    return WINO_E_ARG;
  }
  p->H = (unsigned)(Hin - 1) / (unsigned)stride + 1u, p->W = (unsigned)(Win - 1) / (unsigned)stride + 1u;
  p->in_image = (unsigned long long)(Hin + 2ll) * (unsigned long long)(Win + 2ll) * (unsigned long long)C;
  p->out_image = (unsigned long long)(p->H + 2ull) * (p->W + 2ull) * (unsigned long long)C;
  if (p->in_image >= (1ull << 31)) {
    set_error("dwconv: one padded image must stay below 2^31 elements (Hin=%d Win=%d C=%d)", Hin, Win, C);
    return WINO_E_SHAPE;
  }
  // the 3x3's rule: 16 channels per workgroup when 64 would leave compute units without one
  const int forced = knobs().dw_cb;
  DxPlan wide;
  const unsigned long long grid64 = dx_grid(N, p->H, p->W, C, stride, 64, &wide);
  const int cb = forced == 64 || forced == 16 ? forced : (grid64 < (unsigned long long)cus ? 16 : 64);
  if (dx_grid(N, p->H, p->W, C, stride, cb, p) > 0x7fffffffull) {
    set_error("dwconv: %llu workgroups (N=%d Hin=%d Win=%d C=%d): the launch holds 2^31 - 1", p->grid, N, Hin, Win, C);
    return WINO_E_SHAPE;
  }
  return WINO_OK;
}

template <int K, int STRIDE, int CB>
int dx_launch(const DxArgs& a, unsigned grid, hipStream_t s) {
  if (a.pool)
    hipLaunchKernelGGL((dwx_kernel<K, STRIDE, CB, true>), dim3(grid), dim3(DX_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL((dwx_kernel<K, STRIDE, CB, false>), dim3(grid), dim3(DX_THREADS), 0, s, a);
  return launch_status("dwx_kernel");
}
template <int K>
int dx_launch_k(const DxArgs& a, int stride, int cb, unsigned grid, hipStream_t s) {
  if (cb == 64) return stride == 1 ? dx_launch<K, 1, 64>(a, grid, s) : dx_launch<K, 2, 64>(a, grid, s);
  return stride == 1 ? dx_launch<K, 1, 16>(a, grid, s) : dx_launch<K, 2, 16>(a, grid, s);
}

}  // namespace
}  // namespace wino

using namespace wino;

extern "C" int wino_dwconv_plan(int N, int Hin, int Win, int C, int K, int stride, int cus, int* cb, int* tile_h, int* tile_w,
                                int* tiles_y, int* tiles_x) {
  if (int rc = check_nonnull(cb, tile_h, tile_w, tiles_y, tiles_x)) return rc;
  if (cus < 1) {
    set_error("dwconv_plan: cus must be >= 1");
    return WINO_E_ARG;
  }
  DxPlan p;
  if (int rc = dx_plan(N, Hin, Win, C, K, stride, cus, &p)) return rc;
  *cb = p.cb, *tile_h = p.th, *tile_w = p.tw, *tiles_y = (int)p.tiles_y, *tiles_x = (int)p.tiles_x;
  return WINO_OK;
}

extern "C" int wino_dwconv_bn_act_hw(const float* in, const float* w_taps, const float* bnBias, const float* bnScale,
                                     float* out, float* pool_partials, int N, int Hin, int Win, int C, int K, int stride,
                                     int act, int in_act, int pool_tiles, wino_stream_t s) {
  DxPlan p;
  if (int rc = dx_plan(N, Hin, Win, C, K, stride, 256, &p)) return rc;   // the limits do not depend on the device
  if (!act_keeps_zero(act) || !act_keeps_zero(in_act)) {
    set_error("dwconv: act %d / in_act %d: each is WINO_ACT_NONE, _RELU, _RELU6 or _HARDSWISH", act, in_act);
    return WINO_E_ARG;
  }
  if (N == 0) return WINO_OK;
  if (int rc = check_nonnull(in, w_taps, bnBias, bnScale, out)) return rc;
  if (int rc = check_aligned16(in, w_taps, bnBias, bnScale, out, pool_partials)) return rc;
  int dev = 0, cus = 256;
  if (int rc = current_device(&dev, &cus)) return rc;
  if (int rc = dx_plan(N, Hin, Win, C, K, stride, cus, &p)) return rc;
  const size_t in_b = (size_t)N * (size_t)p.in_image * 4, out_b = (size_t)N * (size_t)p.out_image * 4, vec_b = (size_t)C * 4;
  const size_t pool_b = pool_partials ? (size_t)N * p.tiles_y * p.tiles_x * vec_b : 0;
  if (pool_partials && (long long)pool_tiles != (long long)p.tiles_y * p.tiles_x) {
    set_error("dwconv: pool_tiles = %d, the launch's plan has %u x %u tiles", pool_tiles, p.tiles_y, p.tiles_x);
    return WINO_E_ARG;
  }
  for (const void* w : {(const void*)out, (const void*)pool_partials}) {
    const size_t w_b = w == out ? out_b : pool_b;
    if (w && (overlaps(in, in_b, w, w_b) || overlaps(w_taps, (size_t)K * K * vec_b, w, w_b) || overlaps(bnBias, vec_b, w, w_b) ||
              overlaps(bnScale, vec_b, w, w_b) || (w != out && overlaps(out, out_b, w, w_b)))) {
      set_error("dwconv: out and pool_partials must not overlap in, w_taps, the BN vectors or each other");
      return WINO_E_ARG;
    }
  }
  DxArgs a;
  a.in = in, a.w = w_taps, a.bias = bnBias, a.scale = bnScale, a.out = out, a.pool = pool_partials;
  a.in_image = (long long)p.in_image, a.out_image = (long long)p.out_image;
  a.Hin = (unsigned)Hin, a.Win = (unsigned)Win, a.H = p.H, a.W = p.W, a.C = (unsigned)C;
  a.tiles_y = p.tiles_y, a.tiles_x = p.tiles_x, a.cblks = p.cblks;
  a.act = act, a.in_act = in_act;
  a.divC = make_fastdiv(p.cblks), a.divX = make_fastdiv(p.tiles_x), a.divY = make_fastdiv(p.tiles_y);
  const unsigned grid = (unsigned)p.grid;
  hipStream_t st = (hipStream_t)s;
  return K == 3 ? dx_launch_k<3>(a, stride, p.cb, grid, st) : dx_launch_k<5>(a, stride, p.cb, grid, st);
}
