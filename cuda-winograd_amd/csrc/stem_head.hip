// The two ends of a torchvision ResNet: the stem and the classifier head.
//
// Stem, one launch:  out = maxpool3x3_s2_p1(relu(bn(conv7x7_s2_p3(x, w))))
//   x [N][3][H][W] (NCHW, as images come from torch), w [K][3][7][7] packed by wino_stem_filter_pack,
//   conv grid Hc = (H-1)/2 + 1, pooled grid Hp = (Hc-1)/2 + 1 (the same for W),
//   out [N][Hp][Wp][K] or, out_padded, [N][Hp+2][Wp+2][K] with its ring written 0.
// A workgroup owns a TP x TP tile of pooled outputs of one image and KC output channels.  It
//   1. stages the input patch the tile reads, (4TP+7)^2 pixels x 3 channels, in LDS, zeros outside the image;
//   2. computes the (2TP+1)^2 conv outputs the tile's pool windows cover as an implicit GEMM on
//      v_mfma_f32_16x16x4_f32 (exact f32): rows = conv pixels, columns = channels, k = (ky, kx, c) flattened,
//      147 values + 1 zero = 37 k-steps; each lane keeps its column's 37 filter values in registers;
//   3. applies BN and ReLU and writes the conv tile to LDS over the patch (conv pixels outside the conv grid are 0:
//      after a ReLU a max that starts from 0 equals torch's -inf pool padding);
//   4. takes the 3x3 stride-2 max of each pooled output from LDS and stores 16 bytes per lane.
// Neighbouring tiles share a conv row and column, which both compute (recompute 13 % at TP = 8); the conv output
// never reaches memory.  Two forms: TP = 8 with KC = 64 (throughput) and TP = 4 with KC = 16 (small batches:
// 16x the workgroups, so one image still spreads over the CUs).  wino_stem_plan says which one a shape takes.
// Addressing: each workgroup re-bases its image's input and output pointers in 64 bits; inside an image, offsets
// are 32-bit (3*H*W and the image's output elements are checked to stay below 2^31).
//
// Head, two or three launches:  logits = mean_hw(feat) . Wfc^T + b
//   avgpool_kernel writes pooled [N][C] into the workspace (a padded feat's ring is not read); the 1x1 GEMM
//   (wino_conv1x1_bn, M = N, Cin = C, Kout = classes rounded up to 64) multiplies it by the packed [C][Kp] filter
//   with BN scale 1 and the FC bias as BN bias; trim_kernel copies the first `classes` columns to out unless
//   classes is already a multiple of 64, when the GEMM writes out directly.
#include "wino_common.h"

namespace wino {
namespace {

constexpr int STEM_KSTEPS = 37;   // 147 k values (7 x 7 taps x 3 channels) + 1 zero
constexpr int STEM_KPAD = 4 * STEM_KSTEPS;

// packed stem filter: [K/16][37][64] -- element (nt, s, lane) is w[16 nt + (lane & 15)][c][ky][kx] with
// k = 4 s + (lane >> 4) = (ky * 7 + kx) * 3 + c, so lane `lane` of k-step s loads its B operand from one
// coalesced row; then bnBias [K], bnScale [K]
size_t stem_elems(int K) { return (size_t)K * (STEM_KPAD + 2); }

__global__ void stem_pack_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                 const float* __restrict__ scale, float* __restrict__ packed, int K) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int nf = K * STEM_KPAD;
  if (i >= nf + 2 * K) return;
  if (i >= nf) {
    packed[i] = i < nf + K ? bias[i - nf] : scale[i - nf - K];
    return;
  }
  const int nt = i / (STEM_KSTEPS * 64), r = i - nt * (STEM_KSTEPS * 64);
  const int s = r >> 6, lane = r & 63;
  const int k = 4 * s + (lane >> 4), ko = 16 * nt + (lane & 15);
  float v = 0.f;
  if (k < 147) {
    const int ky = k / 21, kx = (k / 3) % 7, c = k % 3;
    v = w[((ko * 3 + c) * 7 + ky) * 7 + kx];
  }
  packed[i] = v;
}

struct StemGeo {
  int H, W, Hc, Wc, Hp, Wp, K;
  int tiles_y, tiles_x, groups;   // pooled tiles per image, channel groups of KC
  int padded;
};

template <int TP, int KC>
struct StemShape {
  static constexpr int CR = 2 * TP + 1;              // conv rows (and columns) a tile needs
  static constexpr int NPIX = CR * CR;
  static constexpr int MT = (NPIX + 15) / 16;        // 16-row MFMA tiles
  static constexpr int PR = 2 * CR + 5;              // input patch rows (and columns)
  static constexpr int PATCH = 3 * PR * PR;          // [row][col][c]
  static constexpr int PPT = (PATCH + 255) / 256;   // patch values per thread
  static constexpr int NT = KC / 16;                 // 16-column MFMA tiles
  static constexpr int WPN = 4 / NT;                 // waves per column tile
  static constexpr int MPW = (MT + WPN - 1) / WPN;   // row tiles per wave
  static constexpr int CS = KC + 4;                  // conv tile row stride in LDS (floats; 16-byte reads)
  static constexpr int CONV = NPIX * CS;
  static constexpr int LDS = PATCH > CONV ? PATCH : CONV;
  static_assert(NT * WPN == 4, "4 waves split over the column tiles");
};

template <int TP, int KC>
__global__ __launch_bounds__(256) void stem_kernel(const float* __restrict__ x, const float* __restrict__ packed,
                                                   float* __restrict__ out, StemGeo g) {
  using S = StemShape<TP, KC>;
  __shared__ __attribute__((aligned(16))) float lds[S::LDS];   // input patch, then the conv tile over it
  __shared__ int koff[STEM_KPAD];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int b = blockIdx.x;
  const int grp = b % g.groups;
  b /= g.groups;
  const int tx = b % g.tiles_x;
  b /= g.tiles_x;
  const int ty = b % g.tiles_y;
  const int n = b / g.tiles_y;
  const int k0 = grp * KC;
  const int py0 = ty * TP, px0 = tx * TP;
  const int cy0 = 2 * py0 - 1, cx0 = 2 * px0 - 1;   // first conv row / column of the tile
  const int iy0 = 2 * cy0 - 3, ix0 = 2 * cx0 - 3;   // first input row / column of the patch

  // this lane's B operands: column 16 nt + (lane & 15) of the group, all 37 k-steps
  const int nt = wave % S::NT, mg = wave / S::NT;
  float bv[STEM_KSTEPS];
  {
    const float* bp = packed + ((size_t)(k0 / 16 + nt) * STEM_KSTEPS) * 64 + lane;
#pragma unroll
    for (int s = 0; s < STEM_KSTEPS; ++s) bv[s] = bp[s * 64];
  }

  // 1. the input patch (any row alignment: 4-byte loads, consecutive lanes on consecutive columns); every load of
  // the thread is issued before the first LDS write, so the patch costs one memory latency, not S::PPT of them
  const float* xn = x + (size_t)n * 3 * g.H * g.W;
  {
    float v[S::PPT];
#pragma unroll
    for (int i = 0; i < S::PPT; ++i) {
      const int e = tid + 256 * i;
      const int c = e / (S::PR * S::PR), rc = e - c * (S::PR * S::PR);
      const int r = rc / S::PR, col = rc - r * S::PR;
      const int iy = iy0 + r, ix = ix0 + col;
      v[i] = 0.f;
      if (e < S::PATCH && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W) v[i] = xn[(c * g.H + iy) * g.W + ix];
    }
#pragma unroll
    for (int i = 0; i < S::PPT; ++i) {
      const int e = tid + 256 * i;
      const int c = e / (S::PR * S::PR), rc = e - c * (S::PR * S::PR);
      if (e < S::PATCH) lds[rc * 3 + c] = v[i];
    }
  }
  for (int k = tid; k < STEM_KPAD; k += 256) {
    // the padding k reads the pixel's own first value: finite, and its filter row is 0
    koff[k] = k < 147 ? ((k / 21) * S::PR + (k / 3) % 7) * 3 + k % 3 : 0;
  }
  __syncthreads();

  // 2. the conv tile: wave (nt, mg) owns column tile nt and row tiles mg, mg + WPN, ...
  int pix[S::MPW];
#pragma unroll
  for (int j = 0; j < S::MPW; ++j) {
    const int p = (mg + S::WPN * j) * 16 + (lane & 15);
    const int q = p < S::NPIX ? p : 0;
    const int ci = q / S::CR, cj = q - ci * S::CR;
    pix[j] = (2 * ci * S::PR + 2 * cj) * 3;
  }
  f32x4 acc[S::MPW];
#pragma unroll
  for (int j = 0; j < S::MPW; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < STEM_KSTEPS; ++s) {
    const int ko = koff[4 * s + (lane >> 4)];
#pragma unroll
    for (int j = 0; j < S::MPW; ++j) {
      if (mg + S::WPN * j < S::MT) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(lds[pix[j] + ko], bv[s], acc[j], 0, 0, 0);
    }
  }
  __syncthreads();   // every wave is done with the patch: the conv tile goes over it

  // 3. BN + ReLU into LDS; a conv pixel outside the conv grid is the pool's padding: 0
  {
    const int ch = nt * 16 + (lane & 15);
    const float bs = packed[(size_t)g.K * STEM_KPAD + k0 + ch];
    const float sc = packed[(size_t)g.K * STEM_KPAD + g.K + k0 + ch];
#pragma unroll
    for (int j = 0; j < S::MPW; ++j) {
      const int mt = mg + S::WPN * j;
      if (mt >= S::MT) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int p = mt * 16 + (lane >> 4) * 4 + i;
        if (p >= S::NPIX) continue;
        const int ci = p / S::CR, cj = p - ci * S::CR;
        const int cy = cy0 + ci, cx = cx0 + cj;
        float v = relu_nan(acc[j][i] * sc + bs);
        if (cy < 0 || cy >= g.Hc || cx < 0 || cx >= g.Wc) v = 0.f;
        lds[p * S::CS + ch] = v;
      }
    }
  }
  __syncthreads();

  // 4. pool and store.  Output cells of this tile: its pooled pixels, plus, in the padded layout, the ring cells
  // next to it (the tiles along an edge write the ring).
  const int pad = g.padded;
  const int OW = g.Wp + 2 * pad;
  const int rlo = (pad && ty == 0) ? 0 : py0 + pad;
  const int rhi = py0 + TP >= g.Hp ? g.Hp + 2 * pad : py0 + TP + pad;
  const int clo = (pad && tx == 0) ? 0 : px0 + pad;
  const int chi = px0 + TP >= g.Wp ? g.Wp + 2 * pad : px0 + TP + pad;
  const int ncol = chi - clo;
  const int cells = (rhi - rlo) * ncol * (KC / 4);
  float* on = out + (size_t)n * (g.Hp + 2 * pad) * OW * g.K + k0;
  for (int e = tid; e < cells; e += 256) {
    const int q = e % (KC / 4), cell = e / (KC / 4);
    const int r = rlo + cell / ncol, col = clo + cell % ncol;
    f32x4 m = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool ring = pad && (r == 0 || r == g.Hp + 1 || col == 0 || col == g.Wp + 1);
    if (!ring) {
      const int li = 2 * (r - pad - py0), lj = 2 * (col - pad - px0);   // the window's first conv row / column
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(&lds[((li + dy) * S::CR + lj + dx) * S::CS + 4 * q]);
          m = f32x4{max_nan(m.x, v.x), max_nan(m.y, v.y), max_nan(m.z, v.z), max_nan(m.w, v.w)};
        }
    }
    *reinterpret_cast<f32x4*>(on + ((size_t)r * OW + col) * g.K + 4 * q) = m;
  }
}

enum { STEM_AUTO = 0, STEM_BIG = 1, STEM_SMALL = 2 };
constexpr int BIG_TP = 8, BIG_KC = 64, SMALL_TP = 4, SMALL_KC = 16;

long stem_workgroups(int N, int Hp, int Wp, int K, int tp, int kc) {
  return (long)N * ((Hp + tp - 1) / tp) * ((Wp + tp - 1) / tp) * (K / kc);
}

// The big form once it fills every CU twice over (two of its workgroups fit a CU's LDS); below that the small
// form's 16x more workgroups finish sooner.
int stem_form(int N, int Hp, int Wp, int K, int cus, const Knobs& kn) {
  if (kn.stem_form == STEM_BIG || kn.stem_form == STEM_SMALL) return kn.stem_form;
  return stem_workgroups(N, Hp, Wp, K, BIG_TP, BIG_KC) >= 2l * cus ? STEM_BIG : STEM_SMALL;
}

int check_stem(int N, int H, int W, int K, int padded, StemGeo* g) {
  if (N < 1 || H < 1 || W < 1 || K < 64 || K % 64 || (padded != 0 && padded != 1)) {
    set_error("stem: unsupported shape N=%d H=%d W=%d K=%d out_padded=%d (need N, H, W >= 1, K %% 64 == 0, "
              "out_padded 0 or 1)", N, H, W, K, padded);
    return WINO_E_SHAPE;
  }
  g->H = H, g->W = W, g->K = K, g->padded = padded;
  g->Hc = (H - 1) / 2 + 1, g->Wc = (W - 1) / 2 + 1;
  g->Hp = (g->Hc - 1) / 2 + 1, g->Wp = (g->Wc - 1) / 2 + 1;
  const long img_in = 3l * H * W, img_out = (long)(g->Hp + 2) * (g->Wp + 2) * K;
  if (img_in >= (1l << 31) || img_out >= (1l << 31) ||
      stem_workgroups(N, g->Hp, g->Wp, K, SMALL_TP, SMALL_KC) >= (1l << 31)) {
    set_error("stem: one image of %dx%d (or its output, or the grid) exceeds 32-bit offsets", H, W);
    return WINO_E_SHAPE;
  }
  return WINO_OK;
}

template <int TP, int KC>
int launch_stem(const float* x, const float* packed, float* out, int N, StemGeo g, hipStream_t s) {
  g.tiles_y = (g.Hp + TP - 1) / TP, g.tiles_x = (g.Wp + TP - 1) / TP, g.groups = g.K / KC;
  const long wgs = stem_workgroups(N, g.Hp, g.Wp, g.K, TP, KC);
  hipLaunchKernelGGL((stem_kernel<TP, KC>), dim3((unsigned)wgs), dim3(256), 0, s, x, packed, out, g);
  return launch_status("stem_kernel");
}

// ---- head ----
int head_cols(int classes) { return (classes + 63) / 64 * 64; }
size_t pooled_bytes(int N, int C) { return ((size_t)N * C * sizeof(float) + 255) / 256 * 256; }

// packed head: B = Wfc^T [C][Kp] (columns >= classes are 0), then bias [Kp] (0 past classes), scale [Kp] (1)
__global__ void head_pack_kernel(const float* __restrict__ wfc, const float* __restrict__ bfc,
                                 float* __restrict__ packed, int C, int classes, int Kp) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long nb = (long)C * Kp;
  if (i >= nb + 2l * Kp) return;
  if (i >= nb) {
    const int j = (int)((i - nb) % Kp);
    packed[i] = i < nb + Kp ? (j < classes ? bfc[j] : 0.f) : 1.f;
    return;
  }
  const int c = (int)(i / Kp), j = (int)(i - (long)c * Kp);
  packed[i] = j < classes ? wfc[(size_t)j * C + c] : 0.f;
}

// pooled[n][c] = mean over the H x W interior of feat[n]; one thread per (image, channel), channels on lanes
__global__ void avgpool_kernel(const float* __restrict__ feat, float* __restrict__ pooled, int N, int H, int W, int C,
                               int pad) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const int RW = W + 2 * pad;
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const float* f = feat + (size_t)n * (H + 2 * pad) * RW * C + c;
    // four partial sums, eight loads in flight: the map is a handful of pixels, so latency is the cost
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
    const int P = H * W;
#pragma unroll 8
    for (int p = 0; p < P; ++p) {
      const int y = p / W, xx = p - y * W;
      sum[p & 3] += f[((size_t)(y + pad) * RW + xx + pad) * C];
    }
    pooled[(size_t)n * C + c] = ((sum[0] + sum[1]) + (sum[2] + sum[3])) / (float)P;
  }
}

__global__ void trim_kernel(const float* __restrict__ src, float* __restrict__ dst, int N, int classes, int Kp) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)N * classes) return;
  const long n = i / classes;
  dst[i] = src[n * Kp + (i - n * classes)];
}

int check_head(int N, int H, int W, int C, int classes, int padded) {
  if (N < 1 || H < 1 || W < 1 || C < 32 || C % 32 || classes < 1 || (padded != 0 && padded != 1)) {
    set_error("head: unsupported shape N=%d H=%d W=%d C=%d classes=%d in_padded=%d (need N, H, W, classes >= 1, "
              "C %% 32 == 0, in_padded 0 or 1)", N, H, W, C, classes, padded);
    return WINO_E_SHAPE;
  }
  if ((long)H * W >= (1l << 24) || classes > (1 << 24) || (long)N * head_cols(classes) >= (1l << 31) ||
      (long)N * C >= (1l << 31)) {
    set_error("head: shape N=%d H=%d W=%d C=%d classes=%d out of range", N, H, W, C, classes);
    return WINO_E_SHAPE;
  }
  return WINO_OK;
}

}  // namespace

int launch_avgpool(const float* feat, float* pooled, int N, int H, int W, int C, int pad, hipStream_t s) {
  hipLaunchKernelGGL(avgpool_kernel, dim3((unsigned)((C + 255) / 256), (unsigned)(N < 65535 ? N : 65535)), dim3(256), 0,
                     s, feat, pooled, N, H, W, C, pad);
  return launch_status("avgpool_kernel");
}

}  // namespace wino

using namespace wino;

extern "C" {

size_t wino_stem_filter_elems(int K) {
  if (K < 64 || K % 64) return 0;
  return stem_elems(K);
}

int wino_stem_filter_pack(const float* w, const float* bnBias, const float* bnScale, float* packed, int K,
                          wino_stream_t s) {
  if (int rc = check_nonnull(w, bnBias, bnScale, packed)) return rc;
  if (int rc = check_aligned16(packed)) return rc;
  if (K < 64 || K % 64 || K > (1 << 20)) { set_error("stem pack: unsupported K=%d (need K %% 64 == 0)", K); return WINO_E_SHAPE; }
  const int total = (int)stem_elems(K);
  hipLaunchKernelGGL(stem_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)s, w, bnBias,
                     bnScale, packed, K);
  return launch_status("stem_pack_kernel");
}

int wino_stem_plan(int N, int H, int W, int K, int cus, int* form) {
  if (!form || cus < 1) { set_error("NULL pointer or cus < 1"); return WINO_E_ARG; }
  StemGeo g;
  if (int rc = check_stem(N, H, W, K, 0, &g)) return rc;
  *form = stem_form(N, g.Hp, g.Wp, K, cus, knobs());
  return WINO_OK;
}

int wino_stem_hw(const float* x, const float* packed, float* out, int N, int H, int W, int K, int out_padded,
                 wino_stream_t s) {
  if (int rc = check_nonnull(x, packed, out)) return rc;
  if (int rc = check_aligned16(x, packed, out)) return rc;
  StemGeo g;
  if (int rc = check_stem(N, H, W, K, out_padded, &g)) return rc;
  const size_t in_b = (size_t)N * 3 * H * W * sizeof(float);
  const size_t out_b = (size_t)N * (g.Hp + 2 * out_padded) * (g.Wp + 2 * out_padded) * K * sizeof(float);
  if (any_overlap({{x, in_b}, {packed, stem_elems(K) * sizeof(float)}, {out, out_b}})) {
    set_error("x, the packed filter and out must not overlap");
    return WINO_E_ARG;
  }
  int dev = 0, cus = 0;
  if (int rc = current_device(&dev, &cus)) return rc;
  if (stem_form(N, g.Hp, g.Wp, K, cus, knobs()) == STEM_BIG)
    return launch_stem<BIG_TP, BIG_KC>(x, packed, out, N, g, (hipStream_t)s);
  return launch_stem<SMALL_TP, SMALL_KC>(x, packed, out, N, g, (hipStream_t)s);
}

size_t wino_head_elems(int C, int classes) {
  if (C < 32 || C % 32 || classes < 1 || classes > (1 << 24)) return 0;
  return ((size_t)C + 2) * (size_t)head_cols(classes);
}

int wino_head_pack(const float* wfc, const float* bfc, float* packed, int C, int classes, wino_stream_t s) {
  if (int rc = check_nonnull(wfc, bfc, packed)) return rc;
  if (int rc = check_aligned16(packed)) return rc;
  if (!wino_head_elems(C, classes) || wino_head_elems(C, classes) >= (1ul << 31)) {
    set_error("head pack: unsupported C=%d classes=%d (need C %% 32 == 0, classes >= 1)", C, classes);
    return WINO_E_SHAPE;
  }
  const long total = (long)wino_head_elems(C, classes);
  hipLaunchKernelGGL(head_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)s, wfc, bfc,
                     packed, C, classes, head_cols(classes));
  return launch_status("head_pack_kernel");
}

size_t wino_head_workspace_bytes(int N, int C, int classes) {
  if (N < 1 || C < 1 || classes < 1) return 0;
  return pooled_bytes(N, C) + (size_t)N * head_cols(classes) * sizeof(float);
}

int wino_head_prepare(int N, int C, int classes, wino_stream_t s) {
  if (int rc = check_head(N, 1, 1, C, classes, 0)) return rc;
  return wino_conv1x1_prepare(N, C, head_cols(classes), s);
}

int wino_avgpool_fc_hw(const float* feat, const float* packed, float* out, int N, int H, int W, int C, int classes,
                       int in_padded, void* workspace, size_t workspace_bytes, wino_stream_t s) {
  if (int rc = check_nonnull(feat, packed, out, workspace)) return rc;
  if (int rc = check_aligned16(feat, packed, out, workspace)) return rc;
  if (int rc = check_head(N, H, W, C, classes, in_padded)) return rc;
  const size_t need = wino_head_workspace_bytes(N, C, classes);
  if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
  const int Kp = head_cols(classes);
  const size_t feat_b = (size_t)N * (H + 2 * in_padded) * (W + 2 * in_padded) * C * sizeof(float);
  if (any_overlap({{feat, feat_b}, {packed, wino_head_elems(C, classes) * sizeof(float)},
                   {out, (size_t)N * classes * sizeof(float)}, {workspace, need}})) {
    set_error("feat, the packed head, out and the workspace must not overlap");
    return WINO_E_ARG;
  }
  float* pooled = (float*)workspace;
  float* logits = Kp == classes ? out : (float*)((char*)workspace + pooled_bytes(N, C));
  const hipStream_t st = (hipStream_t)s;
  if (int rc = launch_avgpool(feat, pooled, N, H, W, C, in_padded, st)) return rc;
  const float* bias = packed + (size_t)C * Kp;
  if (int rc = wino_conv1x1_bn(pooled, packed, bias, bias + Kp, logits, N, C, Kp, 0, s)) return rc;
  if (logits == out) return WINO_OK;
  const long total = (long)N * classes;
  hipLaunchKernelGGL(trim_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, logits, out, N, classes, Kp);
  return launch_status("trim_kernel");
}

}  // extern "C"
