// Grouped 3x3 convolution (stride 1 or 2, pad 1) + folded BN (+ReLU), gfx950: the middle layer of a ResNeXt block.
//   out = act(bnScale[k] * conv3x3_grouped(in, w) + bnBias[k])
//   in  [N][Hin+2][Win+2][C] with a zero ring, out [N][H+2][W+2][C] with its ring written 0, H = (Hin-1)/stride + 1
//   C -> C in `groups` groups of Cg = C / groups channels; C % 64 == 0, Cg in {4, 8, 16, 32, 64}
// With these a 64-channel output block reads exactly its own 64 input channels, so a workgroup owns a tile of output
// pixels x one 64-channel block and the activation is read once, plus the tile's halo.  One direct kernel, an implicit
// GEMM on v_mfma_f32_16x16x4_f32 (exact f32) summed over the nine taps:
//   1. the input patch of the tile, (S (OH-1) + 3) x (S (OW-1) + 3) pixels x 64 channels, is staged in LDS once (16-byte
//      loads, all issued before the first LDS write; pixels outside the padded input are written 0), at 68 floats a
//      pixel so that the 16 pixels of an MFMA tile start on different banks;
//   2. wave w owns the 16 output channels 16 w .. 16 w + 15 of the block and every 16-pixel row tile of the
//      workgroup's tile.  At Cg = 32 / 64 a column tile contracts over the KC = 32 / 64 channels of its group: one
//      ds_read_b128 feeds four MFMAs, a lane's four values are the channels 4 h + 0..3 (h = lane >> 4) of its pixel,
//      MFMA j takes element j, and the packed filter holds the same k order.  At Cg <= 16 a column tile covers 16 / Cg
//      whole groups and contracts over its own 16 input channels, four MFMAs a tap, MFMA j over the channels
//      4 j .. 4 j + 3 (one group's, or part of one), each into an accumulator of its own; a lane's four output
//      channels 4 h .. 4 h + 3 then take the sum of the accumulators of their own group, by a select.  A group's
//      output never meets another group's activation, not even times 0: 0 * NaN is NaN (DESIGN.md section 1,
//      "Non-finite values").  The filters come as fragments in that order straight from L2: 16 bytes a lane per
//      (tap, 16 channels);
//   3. the filter is the MFMA's A operand and the pixels its B operand (conv1x1_kernel.h), so a lane ends up with four
//      consecutive output channels of one pixel: BN, ReLU and one 16-byte store.  Pixels past H or W are not stored;
//   4. the workgroups along an image's edge write the ring cells next to their tile as 0.
// Stride and tile shape are template parameters of the one body: S; TW = 16 (a row tile is 16 pixels of one output
// row) or 8 (two rows of 8: feature maps such as 56 and 7, which 16 would pad by more); KC.  S = 1 runs four row tiles
// a workgroup, S = 2 two (the patch is four times the tile).
// Addressing: every workgroup re-bases its image's input and output in 64 bits; inside an image offsets are 32-bit
// (one padded input image is checked to stay below 2^31 elements; the output image is never larger).
// No library scratch, no tickets: the layer needs no prepare.
#include "conv3x3_grouped.h"

namespace wino {
namespace {

struct GroupedArgs {
  int Hin, Win, H, W, C;
  int tiles_y, tiles_x, cblocks;
  int relu;
  int Cg;
};

template <int S, int TW, int KC>
struct GroupedShape {
  static constexpr int RT = S == 1 ? 4 : 2;     // 16-pixel MFMA row tiles of a workgroup
  static constexpr int RPT = 16 / TW;           // output rows of a row tile
  static constexpr int OH = RT * RPT, OW = TW;  // the workgroup's output tile
  static constexpr int PH = S * (OH - 1) + 3, PW = S * (OW - 1) + 3;   // its input patch
  static constexpr int PS = 68;                 // floats per patch pixel in LDS (64 + 4: 16-byte rows, banks spread)
  static constexpr int PIECES = PH * PW * 16;   // 16-byte pieces of the patch
  static constexpr int PPT = (PIECES + 255) / 256;
  static constexpr int KG = KC / 16;            // 16-channel chunks of a column tile's contraction
  // resident waves per SIMD the registers are held to (= workgroups per CU): what the patch leaves room for at
  // S = 2 (45 KB), and at S = 1 what the unrolled tap loop fits without a spill: KC = 64 (MFMA-bound there), and
  // KC = 16 with its four accumulators a row tile
  static constexpr int WAVES = S == 2 ? 3 : KC == 64 ? 2 : KC == 16 ? 3 : 4;
  static_assert(TW == 8 || TW == 16, "a row tile is 16 pixels: one row of 16 or two of 8");
  static_assert(KC == 16 || KC == 32 || KC == 64, "a column tile contracts over 16, 32 or 64 channels");
  static_assert(PH * PW * PS * 4 <= 64 * 1024, "static LDS");
};

// packed filter: [C/16 column tiles][9 taps][KC/16][64 lanes][4] -- element (ct, tap, kg, lane, j) is the tap's weight
// from input channel ci = 64 (ct / 4) + kbase + 16 kg + 4 (lane >> 4) + j, kbase = (16 (ct % 4) / KC) KC, to output
// channel ko = 16 ct + (lane & 15); KC = 16: MFMA j contracts over 4 j .. 4 j + 3, ci = 64 (ct / 4) + kbase + 4 j +
// (lane >> 4); 0 when ci is not in ko's group (Cg < 16: rows of an accumulator that the kernel never selects)
__global__ void grouped_pack_kernel(const float* __restrict__ w, float* __restrict__ packed, int C, int Cg, int KC) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 9l * C * KC) return;
  const int KG = KC / 16;
  const int j = (int)(i & 3), lane = (int)((i >> 2) & 63);
  long r = i >> 8;
  const int kg = (int)(r % KG);
  r /= KG;
  const int tap = (int)(r % 9), ct = (int)(r / 9);
  const int ko = 16 * ct + (lane & 15);
  const int ci = 64 * (ct / 4) + (16 * (ct % 4) / KC) * KC + 16 * kg + (KC == 16 ? 4 * j + (lane >> 4) : 4 * (lane >> 4) + j);
  const int g0 = (ko / Cg) * Cg;
  packed[i] = (ci >= g0 && ci < g0 + Cg) ? w[((size_t)ko * Cg + (ci - g0)) * 9 + tap] : 0.f;
}

template <int S, int TW, int KC>
__global__ __launch_bounds__(256, (GroupedShape<S, TW, KC>::WAVES)) void conv3x3_grouped_kernel(
    const float* __restrict__ in, const float* __restrict__ packed, const float* __restrict__ bnBias,
    const float* __restrict__ bnScale, float* __restrict__ out, GroupedArgs g) {
  using G = GroupedShape<S, TW, KC>;
  __shared__ __attribute__((aligned(16))) float lds[G::PH * G::PW * G::PS];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned b = blockIdx.x;
  const int cb = (int)(b % (unsigned)g.cblocks);
  b /= (unsigned)g.cblocks;
  const int tx = (int)(b % (unsigned)g.tiles_x);
  b /= (unsigned)g.tiles_x;
  const int ty = (int)(b % (unsigned)g.tiles_y);
  const int n = (int)(b / (unsigned)g.tiles_y);
  const int oy0 = ty * G::OH, ox0 = tx * G::OW;
  const int IH = g.Hin + 2, IW = g.Win + 2;

  // 1. the patch: padded input rows S oy0 .., columns S ox0 .., the block's 64 channels
  {
    const float* in_n = in + (size_t)n * IH * IW * g.C + cb * 64;
    f32x4 v[G::PPT];
#pragma unroll
    for (int i = 0; i < G::PPT; ++i) {
      const int e = tid + 256 * i;
      const int pix = e >> 4, q = e & 15;
      const int r = pix / G::PW, c = pix - r * G::PW;
      const int iy = S * oy0 + r, ix = S * ox0 + c;
      v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (e < G::PIECES && iy < IH && ix < IW) v[i] = *reinterpret_cast<const f32x4*>(in_n + ((iy * IW + ix) * g.C + 4 * q));
    }
#pragma unroll
    for (int i = 0; i < G::PPT; ++i) {
      const int e = tid + 256 * i;
      if (e < G::PIECES) *reinterpret_cast<f32x4*>(&lds[(e >> 4) * G::PS + 4 * (e & 15)]) = v[i];
    }
  }
  __syncthreads();

  // 2. nine taps of [16 pixels x KC] . [KC x 16] per row tile
  const int p = lane & 15, h = lane >> 4;
  const int ly = TW == 16 ? 0 : p >> 3, lx = TW == 16 ? p : p & 7;   // the lane's pixel inside a row tile
  const int kbase = (16 * wave / KC) * KC;
  int pb[G::RT];
#pragma unroll
  for (int t = 0; t < G::RT; ++t) pb[t] = (S * (t * G::RPT + ly) * G::PW + S * lx) * G::PS + kbase + (KC == 16 ? h : 4 * h);
  const float* fp = packed + (size_t)(cb * 4 + wave) * (9 * G::KG * 256) + lane * 4;
  constexpr int NA = KC == 16 ? 4 : 1;   // accumulators per row tile: one per MFMA of a tap at KC = 16
  f32x4 acc[NA][G::RT];
#pragma unroll
  for (int q = 0; q < NA; ++q)
#pragma unroll
    for (int t = 0; t < G::RT; ++t) acc[q][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int toff = ((tap / 3) * G::PW + tap % 3) * G::PS;
#pragma unroll
    for (int kg = 0; kg < G::KG; ++kg) {
      const f32x4 f = *reinterpret_cast<const f32x4*>(fp + (tap * G::KG + kg) * 256);
      f32x4 a[G::RT];
#pragma unroll
      for (int t = 0; t < G::RT; ++t) {
        if constexpr (KC == 16) {
#pragma unroll
          for (int j = 0; j < 4; ++j) a[t][j] = lds[pb[t] + toff + 4 * j];
        } else {
          a[t] = *reinterpret_cast<const f32x4*>(&lds[pb[t] + toff + 16 * kg]);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < G::RT; ++t)
          acc[KC == 16 ? j : 0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(f[j], a[t][j], acc[KC == 16 ? j : 0][t], 0, 0, 0);
    }
  }

  // 3. BN, ReLU, one 16-byte store per row tile: channels ch .. ch + 3 of the lane's pixel
  const int OWp = g.W + 2;
  float* out_n = out + (size_t)n * (g.H + 2) * OWp * g.C;
  {
    const int ch = cb * 64 + 16 * wave + 4 * h;
    float bs[4], sc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) bs[i] = bnBias[ch + i], sc[i] = bnScale[ch + i];
#pragma unroll
    for (int t = 0; t < G::RT; ++t) {
      const int oy = oy0 + t * G::RPT + ly, ox = ox0 + lx;
      f32x4 sum = acc[0][t];
      if constexpr (KC == 16) {   // the accumulators of the lane's own group (channels 4 h ..: group 4 h / Cg)
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        sum = 0 == (4 * h) / g.Cg ? sum : zero;
#pragma unroll
        for (int j = 1; j < 4; ++j) sum += (4 * j) / g.Cg == (4 * h) / g.Cg ? acc[j][t] : zero;
      }
      f32x4 r;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float y = sum[i] * sc[i] + bs[i];
        r[i] = g.relu ? relu_nan(y) : y;
      }
      if (oy < g.H && ox < g.W) *reinterpret_cast<f32x4*>(out_n + (((oy + 1) * OWp + ox + 1) * g.C + ch)) = r;
    }
  }

  // 4. the ring cells next to a tile on the image's edge
  const bool last_y = oy0 + G::OH >= g.H, last_x = ox0 + G::OW >= g.W;
  if (ty == 0 || tx == 0 || last_y || last_x) {
    const int rlo = ty == 0 ? 0 : oy0 + 1, rhi = last_y ? g.H + 2 : oy0 + G::OH + 1;
    const int clo = tx == 0 ? 0 : ox0 + 1, chi = last_x ? g.W + 2 : ox0 + G::OW + 1;
    const int ncol = chi - clo;
    const int cells = (rhi - rlo) * ncol * 16;
    for (int e = tid; e < cells; e += 256) {
      const int q = e & 15, cell = e >> 4;
      const int r = rlo + cell / ncol, c = clo + cell % ncol;
      if (r == 0 || r == g.H + 1 || c == 0 || c == g.W + 1)
        *reinterpret_cast<f32x4*>(out_n + ((r * OWp + c) * g.C + cb * 64 + 4 * q)) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
}

bool legal_channels(int C, int groups) {
  if (C <= 0 || C % 64 || groups < 1 || C % groups) return false;
  const int Cg = C / groups;
  return Cg == 4 || Cg == 8 || Cg == 16 || Cg == 32 || Cg == 64;
}

using GroupedKernel = void (*)(const float*, const float*, const float*, const float*, float*, GroupedArgs);
template <int S, int TW>
constexpr GroupedKernel GROUPED_BY_KC[3] = {conv3x3_grouped_kernel<S, TW, 16>, conv3x3_grouped_kernel<S, TW, 32>,
                                            conv3x3_grouped_kernel<S, TW, 64>};

}  // namespace

int check_grouped(int N, int Hin, int Win, int C, int groups, int stride, GroupedGeom* g) {
  if (stride != 1 && stride != 2) { set_error("grouped 3x3: stride %d (need 1 or 2)", stride); return WINO_E_ARG; }
  if (N < 1 || Hin < 1 || Win < 1) { set_error("grouped 3x3: bad N=%d Hin=%d Win=%d", N, Hin, Win); return WINO_E_SHAPE; }
  if (!legal_channels(C, groups)) {
    set_error("grouped 3x3: unsupported C=%d groups=%d (need C %% 64 == 0 and C / groups in {4, 8, 16, 32, 64})", C, groups);
    return WINO_E_SHAPE;
  }
  const unsigned long long img = ((unsigned long long)Hin + 2) * ((unsigned long long)Win + 2) * (unsigned long long)C;
  if (img >= (1ull << 31)) {
    set_error("grouped 3x3: one padded %dx%d image of %d channels reaches 2^31 elements", Hin, Win, C);
    return WINO_E_SHAPE;
  }
  const int H = (Hin - 1) / stride + 1, W = (Win - 1) / stride + 1, Cg = C / groups;
  // 8-wide tiles where 16-wide ones would pad the row by more
  const int TW = (W + 7) / 8 * 8 < (W + 15) / 16 * 16 ? 8 : 16;
  const int OH = (stride == 1 ? 4 : 2) * (16 / TW);
  const int tiles_y = (H + OH - 1) / OH, tiles_x = (W + TW - 1) / TW;
  if ((unsigned long long)N * tiles_y * tiles_x * (C / 64) >= (1ull << 31)) {
    set_error("grouped 3x3: %d images of %dx%d tiles x %d channel blocks reach 2^31 workgroups", N, tiles_y, tiles_x, C / 64);
    return WINO_E_SHAPE;
  }
  *g = GroupedGeom{N, Hin, Win, C, groups, Cg, stride, H, W, Cg < 16 ? 16 : Cg, TW, tiles_y, tiles_x};
  return WINO_OK;
}

}  // namespace wino

using namespace wino;

extern "C" {

size_t wino_conv3x3_grouped_filter_elems(int C, int groups) {
  if (!legal_channels(C, groups)) return 0;
  const int Cg = C / groups;
  return (size_t)9 * C * (Cg < 16 ? 16 : Cg);
}

int wino_conv3x3_grouped_filter_pack(const float* w, float* packed, int C, int groups, wino_stream_t s) {
  if (int rc = check_nonnull(w, packed)) return rc;
  if (int rc = check_aligned16(packed)) return rc;
  const size_t total = wino_conv3x3_grouped_filter_elems(C, groups);
  if (!total) {
    set_error("grouped 3x3 filter: unsupported C=%d groups=%d (need C %% 64 == 0 and C / groups in {4, 8, 16, 32, 64})", C, groups);
    return WINO_E_SHAPE;
  }
  const int Cg = C / groups;
  hipLaunchKernelGGL(grouped_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)s, w, packed, C,
                     Cg, Cg < 16 ? 16 : Cg);
  return launch_status("grouped_pack_kernel");
}

int wino_conv3x3_grouped_plan(int N, int Hin, int Win, int C, int groups, int stride, int* tile_w, int* kc,
                              int* tiles_y, int* tiles_x) {
  if (!tile_w || !kc || !tiles_y || !tiles_x) {
    set_error("NULL pointer");
    return WINO_E_ARG;
  }
  GroupedGeom g;
  if (int rc = check_grouped(N, Hin, Win, C, groups, stride, &g)) return rc;
  *tile_w = g.TW, *kc = g.KC, *tiles_y = g.tiles_y, *tiles_x = g.tiles_x;
  return WINO_OK;
}

int wino_conv3x3_grouped_bn_relu_hw(const float* in, const float* packed, const float* bnBias, const float* bnScale,
                                    float* out, int N, int Hin, int Win, int C, int groups, int stride, int relu,
                                    wino_stream_t s) {
  if (int rc = check_nonnull(in, packed, bnBias, bnScale, out)) return rc;
  if (int rc = check_aligned16(in, packed, out)) return rc;
  GroupedGeom g;
  if (int rc = check_grouped(N, Hin, Win, C, groups, stride, &g)) return rc;
  if (overlaps(in, padded_bytes(N, Hin, Win, C), out, padded_bytes(N, g.H, g.W, C))) {
    set_error("grouped 3x3: in and out overlap");
    return WINO_E_ARG;
  }
  const int kc = g.KC == 16 ? 0 : g.KC == 32 ? 1 : 2;
  const GroupedKernel kernel = stride == 1 ? (g.TW == 16 ? GROUPED_BY_KC<1, 16>[kc] : GROUPED_BY_KC<1, 8>[kc])
                                           : (g.TW == 16 ? GROUPED_BY_KC<2, 16>[kc] : GROUPED_BY_KC<2, 8>[kc]);
  const GroupedArgs a{Hin, Win, g.H, g.W, C, g.tiles_y, g.tiles_x, C / 64, relu != 0, g.Cg};
  const unsigned wgs = (unsigned)((unsigned long long)N * g.tiles_y * g.tiles_x * (C / 64));
  hipLaunchKernelGGL(kernel, dim3(wgs), dim3(256), 0, (hipStream_t)s, in, packed, bnBias, bnScale, out, a);
  return launch_status("conv3x3_grouped_kernel");
}

}  // extern "C"
