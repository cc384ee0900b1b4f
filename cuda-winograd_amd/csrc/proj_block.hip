// The projection (downsampling) bottleneck's own pieces: the geometry check, the packed fused tail, and the two 1x1
// launches in the operand forms only this block uses.  ResNet v1 placement (the stride on the first 1x1 and on the
// projection, the 3x3 at stride 1 on the output grid):
//   xs  = x[:, ::s, ::s, :]                                   (never materialised)
//   t1  = relu(bn1(xs . w1))              padded [N][H+2][W+2][Cm]   (workspace)
//   t2  = relu(bn2(conv3x3(t1, U2)))      padded [N][H+2][W+2][Cm]   (workspace)
//   out = relu(bn3(t2 . w3) + bnp(xs . wp))     [N][H][W][C4]
// The strided first 1x1 (A_STRIDED; s = 1 is the plain 1x1 entry point) and the FUSED TAIL -- one GEMM of K = Cm + Cin
// whose k-steps read t2 first and the strided x after it (conv1x1_kernel.h, A_TWO), against the stacked, scale-folded
// [bn3Scale . w3 ; bnpScale . wp] with the summed bias: the shortcut is accumulated in the same registers as the last
// 1x1 and never reaches memory.  The kernels are the 1x1 kernel templates with the operand form as a template
// argument, launched by the same launch_1x1 as conv1x1.hip's (conv1x1_launch.h).  This file's calls instantiate those
// forms here; conv1x1.hip instantiates only A_PLAIN.
// The blocks themselves -- this one, the v1.5 and the grouped placements, which end in the same tail -- are composed in
// bottleneck.hip.
#include "proj_block.h"

namespace wino {

using namespace gemm1x1;

namespace {

// packed = [bn3Scale . w3 ; bnpScale . wp] ([Cm + Cin][C4], row-major), then bn3Bias + bnpBias, then C4 ones (the
// tail's BN scale: the scales are folded into the matrix).  One thread per element.
__global__ void proj_tail_pack_kernel(const float* __restrict__ w3, const float* __restrict__ b3,
                                      const float* __restrict__ s3, const float* __restrict__ wp,
                                      const float* __restrict__ bp, const float* __restrict__ sp,
                                      float* __restrict__ packed, int Cm, int Cin, int C4) {
  const long total = (long)(Cm + Cin + 2) * C4;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long r = i / C4;
  const int k = (int)(i - r * C4);
  float v;
  if (r < Cm) v = s3[k] * w3[i];
  else if (r < Cm + Cin) v = sp[k] * wp[i - (long)Cm * C4];
  else if (r == Cm + Cin) v = b3[k] + bp[k];
  else v = 1.f;
  packed[i] = v;
}

}  // namespace

// The block's geometry, checked once.  Every 32-bit quantity the strided / two-source addressing creates is bounded
// here: the pixel row index (M < 2^31, one input image < 2^31 pixels), the buffer-descriptor windows of a 112-row tile
// over the strided x and over the padded t2, the ring pass's 16-byte units, and B's descriptor.
int check_proj(int N, int Hin, int Win, int Cin, int Cm, int C4, int stride, ProjGeom* g) {
  if (stride != 1 && stride != 2) { set_error("projection block: stride %d (need 1 or 2)", stride); return WINO_E_ARG; }
  if (N < 1 || Hin < 1 || Win < 1) { set_error("projection block: bad N=%d Hin=%d Win=%d", N, Hin, Win); return WINO_E_SHAPE; }
  if (Cin <= 0 || Cm <= 0 || C4 <= 0 || Cin % 32 || Cm % 64 || C4 % 64) {
    set_error("projection block: unsupported channels Cin=%d Cm=%d C4=%d (need Cin %% 32 == 0, Cm %% 64 == 0, C4 %% 64 == 0)",
              Cin, Cm, C4);
    return WINO_E_SHAPE;
  }
  const int H = (Hin - 1) / stride + 1, W = (Win - 1) / stride + 1;
  if (H > 4094 || W > 4094) { set_error("projection block: unsupported feature map %dx%d", H, W); return WINO_E_SHAPE; }
  const unsigned long long M = (unsigned long long)N * H * W;
  if (M >= (1ull << 31)) { set_error("projection block: N*H*W = %llu pixel rows (need < 2^31)", M); return WINO_E_SHAPE; }
  if ((unsigned long long)Hin * Win >= (1ull << 31)) { set_error("projection block: input image too large"); return WINO_E_SHAPE; }
  // a tile's window over the strided x: consecutive pixel rows are at most s*Win input pixels apart
  const unsigned long long x_win = ((unsigned long long)(BM - 1) * stride * Win + 1) * Cin * sizeof(float);
  // ... and over the padded t2: at most 2(W+2)+3 padded pixels apart (the step to the next image)
  const unsigned long long t_win = ((unsigned long long)(BM - 1) * (2ull * (W + 2) + 3) + 1) * Cm * sizeof(float);
  // the first launch's ring pass (t1's zero ring) counts 16-byte units in 32 bits
  const unsigned long long ring = (unsigned long long)N * (2ull * (W + 2) + 2ull * H) * (Cm / 4);
  const unsigned long long b_tail = (unsigned long long)(Cm + Cin) * C4 * sizeof(float);
  const unsigned long long b_first = (unsigned long long)Cin * Cm * sizeof(float);
  if (x_win >= FOUR_GIB || t_win >= FOUR_GIB || ring >= FOUR_GIB || b_tail >= FOUR_GIB || b_first >= FOUR_GIB) {
    set_error("projection block: a tile's window or a filter matrix reaches 4 GiB (Win=%d Cin=%d Cm=%d C4=%d)", Win, Cin, Cm, C4);
    return WINO_E_SHAPE;
  }
  if ((M + BM - 1) / BM > (1ull << 24)) { set_error("projection block: M too large"); return WINO_E_SHAPE; }
  *g = ProjGeom{N, Hin, Win, Cin, Cm, C4, stride, H, W, (long)M};
  return WINO_OK;
}

namespace {

static ProjGeo proj_geo(const ProjGeom& g, const float* x) {
  return ProjGeo{x, (unsigned)g.Hin * (unsigned)g.Win, (unsigned)(g.s * g.Win), (unsigned)g.s, g.Cin, g.Cm};
}

// The plans of the two 1x1 launches: the planner and the launch models see each as one GEMM, the tail with
// K = Cm + Cin.  The latency form's K split must cut both of the tail's sources into 16-channel chunks; a split the
// planner finds legal for K is legal for both, since Cm % 64 == 0 makes K % (16 KS) == Cin % (16 KS) for KS <= 4.
static Plan1x1 plan_first(const ProjGeom& g, int cus, const Knobs& kn) { return plan_1x1(g.M, g.Cin, g.Cm, 1, cus, kn); }
static Plan1x1 plan_tail(const ProjGeom& g, int cus, const Knobs& kn) { return plan_1x1(g.M, g.Cm + g.Cin, g.C4, 1, cus, kn); }
static int form_of(const Plan1x1& p) { return p.small.use ? WINO_1X1_FORM_LATENCY : p.sk ? WINO_1X1_FORM_STREAM_K : WINO_1X1_FORM_TILED; }

}  // namespace

// the first 1x1 at full input resolution (the v1.5 and the grouped placements): its pixel rows, row tiles and ring pass
int check_first_1x1_full(int N, int Hin, int Win, int Cm) {
  const unsigned long long M1 = (unsigned long long)N * Hin * Win;
  const unsigned long long ring1 = (unsigned long long)N * (2ull * (Win + 2) + 2ull * Hin) * (Cm / 4);
  if (Hin > 4094 || Win > 4094 || M1 >= (1ull << 31) || (M1 + BM - 1) / BM > (1ull << 24) || ring1 >= FOUR_GIB) {
    set_error("projection block: the first 1x1 at %dx%d x %d images is too large for one launch", Hin, Win, N);
    return WINO_E_SHAPE;
  }
  return WINO_OK;
}

// the strided first 1x1 (A_STRIDED): t1 = relu(bn1(xs . w1)), padded [N][H+2][W+2][Cm]; the plain layer's plan at M = N*H*W
int launch_first_strided(const ProjGeom& g, const float* x, const float* w1, const float* bnBias, const float* bnScale,
                         float* t1, hipStream_t s) {
  int dev = 0, cus = 0;
  if (int rc = current_device(&dev, &cus)) return rc;
  return launch_1x1<A_STRIDED>(plan_first(g, cus, knobs()), dev,
                               {x, w1, bnBias, bnScale, nullptr, t1, g.M, g.Cin, g.Cm, WINO_RELU | WINO_C_PADDED,
                                make_padgeo(g.H, g.W), proj_geo(g, x)},
                               s);
}

// the fused tail (A_TWO): out = relu(t2 . [bn3Scale w3] + xs . [bnpScale wp] + bias), t2 padded [N][H+2][W+2][Cm]
int launch_proj_tail(const ProjGeom& g, const float* t2, const float* tail_packed, const float* x, float* out,
                     hipStream_t s) {
  int dev = 0, cus = 0;
  if (int rc = current_device(&dev, &cus)) return rc;
  const float* bias = tail_packed + (size_t)(g.Cm + g.Cin) * g.C4;
  return launch_1x1<A_TWO>(plan_tail(g, cus, knobs()), dev,
                           {t2, tail_packed, bias, bias + g.C4, nullptr, out, g.M, g.Cm + g.Cin, g.C4,
                            WINO_RELU | WINO_A_PADDED, make_padgeo(g.H, g.W), proj_geo(g, x)},
                           s);
}

int prepare_proj_tail(const ProjGeom& g, hipStream_t s) {
  int dev = 0, cus = 0;
  if (int rc = current_device(&dev, &cus)) return rc;
  const Plan1x1 pt = plan_tail(g, cus, knobs());
  SkBufs bufs;
  return pt.sk ? tiled_scratch(dev, s, pt, &bufs) : WINO_OK;
}

}  // namespace wino

using namespace wino;

extern "C" {

size_t wino_proj_tail_elems(int Cm, int Cin, int C4) {
  if (Cm <= 0 || Cin <= 0 || C4 <= 0) return 0;
  return (size_t)(Cm + Cin + 2) * (size_t)C4;
}

int wino_proj_tail_pack(const float* w3, const float* bn3Bias, const float* bn3Scale, const float* wp,
                        const float* bnpBias, const float* bnpScale, float* packed, int Cm, int Cin, int C4, wino_stream_t s) {
  if (int rc = check_nonnull(w3, bn3Bias, bn3Scale, wp, bnpBias, bnpScale, packed)) return rc;
  if (int rc = check_aligned16(packed)) return rc;
  if (Cm <= 0 || Cin <= 0 || C4 <= 0 || Cin % 32 || Cm % 64 || C4 % 64 ||
      (unsigned long long)(Cm + Cin) * C4 * sizeof(float) >= FOUR_GIB) {
    set_error("projection tail: unsupported shape Cm=%d Cin=%d C4=%d (need Cin %% 32 == 0, Cm %% 64 == 0, C4 %% 64 == 0)",
              Cm, Cin, C4);
    return WINO_E_SHAPE;
  }
  const long total = (long)(Cm + Cin + 2) * C4;
  hipLaunchKernelGGL(proj_tail_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)s, w3,
                     bn3Bias, bn3Scale, wp, bnpBias, bnpScale, packed, Cm, Cin, C4);
  return launch_status("proj_tail_pack_kernel");
}

int wino_proj_tail_plan(int N, int Hin, int Win, int Cin, int Cm, int C4, int stride, int cus, int* first_form,
                        int* tail_form) {
  if (!first_form || !tail_form || cus < 1) { set_error("bad argument"); return WINO_E_ARG; }
  ProjGeom g;
  if (int rc = check_proj(N, Hin, Win, Cin, Cm, C4, stride, &g)) return rc;
  const Knobs kn = knobs();
  *first_form = form_of(plan_first(g, cus, kn));   // (stride 1 runs the plain 1x1 entry point: the same plan)
  *tail_form = form_of(plan_tail(g, cus, kn));
  return WINO_OK;
}

}  // extern "C"
