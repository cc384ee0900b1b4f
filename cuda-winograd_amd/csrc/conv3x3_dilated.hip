// Stride-1 3x3 convolution with dilation d and padding d + folded BN (+ReLU), gfx950: the 3x3 of the bottlenecks in
// layer3 / layer4 of torchvision's segmentation backbones (replace_stride_with_dilation).  Over the library's padded
// layout -- a zero ring of width ONE, whatever d -- it is the GEMM
//   out[m][k] = act( bnScale[k] * sum_{tap, c} in[pixel(m, tap)][c] * w_taps[tap][c][k] + bnBias[k] )
// of M = N*H*W output pixels, K = 9 C and Kout = K, where tap (dy, dx) of output pixel (y, x) is input pixel
// (y + d(dy-1), x + d(dx-1)) when that lies inside the image and a zero otherwise.  The tiled 1x1 kernel runs it in
// operand form A_DIL (conv1x1_kernel.h): the LDS-DMA pipeline, MFMA loop, stream-K hand-off and ring pass of A_TAPS with
// per-lane, per-tap A offsets.  This file instantiates that form's four tiled kernels ({4, 8 waves} x {plain,
// stream-K}) and no other; there is no latency form (launch_1x1 would instantiate its 18 kernels): the plan is
// plan_1x1 of the GEMM with the latency choice off, launched through launch_tiled_1x1.
#include "conv3x3_dilated.h"

namespace wino {

using namespace gemm1x1;

// The layer's geometry, checked once.  Every 32-bit quantity of the addressing is bounded here: the pixel row index
// (M < 2^31, one padded image < 2^31 pixels), a 112-row tile's buffer-descriptor window over the padded input with the
// taps' reach to either side, B's descriptor and the ring pass's 16-byte units.
int check_dilated(int N, int H, int W, int C, int K, int dilation, DilGeom* g) {
  if (N < 1 || H < 1 || W < 1) { set_error("dilated 3x3: bad N=%d H=%d W=%d", N, H, W); return WINO_E_SHAPE; }
  if (C <= 0 || K <= 0 || C % 32 || K % 64) {
    set_error("dilated 3x3: unsupported channels C=%d K=%d (need C %% 32 == 0, K %% 64 == 0)", C, K);
    return WINO_E_SHAPE;
  }
  if (dilation < 1) { set_error("dilated 3x3: dilation %d (need >= 1)", dilation); return WINO_E_SHAPE; }
  if (H > 4094 || W > 4094) { set_error("dilated 3x3: unsupported feature map %dx%d", H, W); return WINO_E_SHAPE; }
  const unsigned long long M = (unsigned long long)N * H * W, Wp = (unsigned long long)W + 2;
  if (M >= (1ull << 31)) { set_error("dilated 3x3: N*H*W = %llu pixel rows (need < 2^31)", M); return WINO_E_SHAPE; }
  if (((unsigned long long)H + 2) * Wp >= (1ull << 31)) { set_error("dilated 3x3: input image too large"); return WINO_E_SHAPE; }
  // a tile's window: consecutive rows' centre pixels are at most 2 (W+2) + 3 padded pixels apart (the step to the next
  // image; 1 inside a line, 3 to the next line), and the taps reach d (W+2) + d pixels to either side of them
  const unsigned long long reach = (unsigned long long)dilation * (Wp + 1);
  const unsigned long long a_win = ((unsigned long long)(BM - 1) * (2 * Wp + 3) + 2 * reach + 1) * C * sizeof(float);
  const unsigned long long b = 9ull * C * K * sizeof(float);
  const unsigned long long ring = (unsigned long long)N * (2ull * (W + 2) + 2ull * H) * (K / 4);
  if (a_win >= FOUR_GIB || b >= FOUR_GIB || ring >= FOUR_GIB) {
    set_error("dilated 3x3: a tile's window, the filter matrix or the ring pass reaches 2^32 (W=%d C=%d K=%d dilation=%d)",
              W, C, K, dilation);
    return WINO_E_SHAPE;
  }
  if ((M + BM - 1) / BM > (1ull << 24)) { set_error("dilated 3x3: M too large"); return WINO_E_SHAPE; }
  *g = DilGeom{N, H, W, C, K, dilation, (long)M};
  return WINO_OK;
}

namespace {

// plan_1x1 of the GEMM (N*H*W, 9C, K), tiled forms only
Plan1x1 plan_dilated(const DilGeom& g, int cus, const Knobs& kn) {
  Plan1x1 p = plan_1x1(g.M, 9 * g.C, g.K, 1, cus, kn);
  p.small.use = false;
  return p;
}

}  // namespace

int launch_dilated(const DilGeom& g, const float* in, const float* w_taps, const float* bnBias, const float* bnScale,
                   float* out, bool relu, bool out_padded, hipStream_t s) {
  int dev = 0, cus = 0;
  if (int rc = current_device(&dev, &cus)) return rc;
  const ProjGeo xg{nullptr, 0u, 0u, (unsigned)g.d, g.C, g.W + 2};
  const int flags = (relu ? WINO_RELU : 0) | WINO_A_PADDED | (out_padded ? WINO_C_PADDED : 0);
  const Plan1x1 p = plan_dilated(g, cus, knobs());
  const Operands1x1 o{in, w_taps, bnBias, bnScale, nullptr, out, g.M, 9 * g.C, g.K, flags, make_padgeo(g.H, g.W), xg};
  return (p.four ? launch_tiled_1x1<4, A_DIL, RES_NONE> : launch_tiled_1x1<8, A_DIL, RES_NONE>)(p, dev, o, s);
}

}  // namespace wino

using namespace wino;

extern "C" {

int wino_conv3x3_dilated_bn_relu_hw(const float* in, const float* w_taps, const float* bnBias, const float* bnScale,
                                    float* out, int N, int H, int W, int C, int K, int dilation, int relu,
                                    wino_stream_t s) {
  if (int rc = check_nonnull(in, w_taps, bnBias, bnScale, out)) return rc;
  if (int rc = check_aligned16(in, w_taps, out)) return rc;
  DilGeom g;
  if (int rc = check_dilated(N, H, W, C, K, dilation, &g)) return rc;
  if (overlaps(in, padded_bytes(N, H, W, C), out, padded_bytes(N, H, W, K))) {
    set_error("dilated 3x3: in and out overlap");
    return WINO_E_ARG;
  }
  return launch_dilated(g, in, w_taps, bnBias, bnScale, out, relu != 0, true, (hipStream_t)s);
}

int wino_conv3x3_dilated_prepare_hw(int N, int H, int W, int C, int K, int dilation, wino_stream_t s) {
  DilGeom g;
  if (int rc = check_dilated(N, H, W, C, K, dilation, &g)) return rc;
  int dev = 0, cus = 0;
  if (int rc = current_device(&dev, &cus)) return rc;
  const Plan1x1 p = plan_dilated(g, cus, knobs());
  if (!p.sk) return WINO_OK;
  SkBufs bufs;
  return tiled_scratch(dev, (hipStream_t)s, p, &bufs);
}

int wino_conv3x3_dilated_plan(int N, int H, int W, int C, int K, int dilation, int cus, int* form) {
  if (!form || cus < 1) { set_error("bad argument"); return WINO_E_ARG; }
  DilGeom g;
  if (int rc = check_dilated(N, H, W, C, K, dilation, &g)) return rc;
  *form = plan_dilated(g, cus, knobs()).sk ? WINO_1X1_FORM_STREAM_K : WINO_1X1_FORM_TILED;
  return WINO_OK;
}

}  // extern "C"
