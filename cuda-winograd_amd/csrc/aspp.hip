// Atrous spatial pyramid pooling (torchvision's DeepLabV3 head, ASPP) and the join in its middle, gfx950.
//
//   wino_conv1x1_cat_bn_hw   out = act(bnScale * (cat(src_0 .. src_{S-1}) . w) + bias_per_image[n])      (one launch)
//   wino_aspp_hw             the five branches, the join and the projection                              (eight launches)
//
// ASPP concatenates five branches of Cb channels and projects the 5 Cb channels to Kout.  Neither the concatenated
// tensor nor the broadcast of the pooled branch exists here:
//  * the projection is ONE GEMM whose K range runs through the four spatial branches in turn -- the tiled 1x1 kernel
//    in operand form A_CAT (conv1x1_kernel.h): one descriptor per tile that spans all sources, the source's offset in
//    the scalar k-step offset, so stream-K ranges cut anywhere;
//  * the pooled branch is constant over an image, so its share of the projection is a per-image bias,
//    bias[n] = prScale * (pooled_branch[n] . w_proj[4 Cb ..]) + prBias, folded by two GEMMs of M = N rows and added in
//    A_CAT's epilogue, which reads its bias by the output row's image.
// This file instantiates A_CAT's four tiled kernels ({4, 8 waves} x {plain, stream-K}) and no others; there is no
// latency form.  The plan is plan_1x1 of the GEMM (N*H*W, S*Cs, Kout) with the latency choice off.
#include "conv3x3_dilated.h"

namespace wino {
namespace {

using namespace gemm1x1;

constexpr int CAT_MIN_SOURCES = 2, CAT_MAX_SOURCES = 8;

struct CatGeom {
  int N, H, W, S, Cs, Kout, flags;
  long M, stride;
};

// The concat layer's GEMM: the plain layer's limits (check_1x1_hw) at Cin = S Cs.  What prepare and the plan query check.
int check_cat_gemm(int N, int H, int W, int sources, int Cs, int Kout, CatGeom* g) {
  if (N < 1 || H < 1 || W < 1) { set_error("concat 1x1: bad N=%d H=%d W=%d", N, H, W); return WINO_E_SHAPE; }
  if (sources < CAT_MIN_SOURCES || sources > CAT_MAX_SOURCES) {
    set_error("concat 1x1: %d sources (need %d .. %d)", sources, CAT_MIN_SOURCES, CAT_MAX_SOURCES);
    return WINO_E_SHAPE;
  }
  if (Cs <= 0 || Kout <= 0 || Cs % 32 || Kout % 64) {
    set_error("concat 1x1: unsupported channels Cs=%d Kout=%d (need Cs %% 32 == 0, Kout %% 64 == 0)", Cs, Kout);
    return WINO_E_SHAPE;
  }
  if ((long)sources * Cs >= (1l << 31)) { set_error("concat 1x1: sources * Cs too large"); return WINO_E_SHAPE; }
  if (int rc = check_1x1_hw(N, H, W, sources * Cs, Kout)) return rc;
  const unsigned long long M = (unsigned long long)N * H * W;
  if (M >= (1ull << 31)) { set_error("concat 1x1: N*H*W = %llu pixel rows (need < 2^31)", M); return WINO_E_SHAPE; }
  *g = CatGeom{N, H, W, sources, Cs, Kout, 0, (long)M, 0};
  return WINO_OK;
}
// The launch's geometry: the GEMM, then the sources' spacing and the tile's descriptor window -- a 112-row tile's rows of
// source 0 (padded: consecutive rows' pixels are at most 2 (W+2) + 3 padded pixels apart) plus (S-1) * src_stride floats
// -- which a 32-bit byte offset must span.
int check_cat(int N, int H, int W, int sources, int Cs, int Kout, long src_stride, int flags, CatGeom* g) {
  if (int rc = check_cat_gemm(N, H, W, sources, Cs, Kout, g)) return rc;
  const bool padded = flags & WINO_A_PADDED;
  const unsigned long long M = (unsigned long long)g->M, Wp = (unsigned long long)W + 2;
  const unsigned long long src_elems = (padded ? (unsigned long long)N * (H + 2) * Wp : M) * Cs;
  if (src_stride < 0 || src_stride % 4) {
    set_error("concat 1x1: src_stride %ld floats (need a multiple of 4)", src_stride);
    return WINO_E_SHAPE;
  }
  if ((unsigned long long)src_stride < src_elems) {
    set_error("concat 1x1: src_stride %ld floats is smaller than a source (%llu)", src_stride, src_elems);
    return WINO_E_SHAPE;
  }
  const unsigned long long rows = padded ? (unsigned long long)(BM - 1) * (2 * Wp + 3) + 1 : (unsigned long long)BM;
  // (compared in floats first: src_stride * 4 must not overflow 64 bits either)
  if ((unsigned long long)src_stride >= FOUR_GIB ||
      (rows * Cs + (unsigned long long)(sources - 1) * src_stride) * sizeof(float) >= FOUR_GIB) {
    set_error("concat 1x1: a tile's window over all sources reaches 2^32 bytes (src_stride=%ld sources=%d W=%d Cs=%d)",
              src_stride, sources, W, Cs);
    return WINO_E_SHAPE;
  }
  g->flags = flags;
  g->stride = src_stride;
  return WINO_OK;
}

// plan_1x1 of the GEMM (N*H*W, S*Cs, Kout), tiled forms only
Plan1x1 plan_cat(const CatGeom& g, int cus, const Knobs& kn) {
  Plan1x1 p = plan_1x1(g.M, g.S * g.Cs, g.Kout, 1, cus, kn);
  p.small.use = false;
  return p;
}

constexpr int CAT_FLAGS = WINO_RELU | WINO_A_PADDED | WINO_C_PADDED;

size_t cat_src_bytes(const CatGeom& g) {
  const size_t one = (g.flags & WINO_A_PADDED) ? padded_bytes(g.N, g.H, g.W, g.Cs) : (size_t)g.M * g.Cs * sizeof(float);
  return (size_t)(g.S - 1) * g.stride * sizeof(float) + one;
}
size_t cat_out_bytes(const CatGeom& g) {
  return (g.flags & WINO_C_PADDED) ? padded_bytes(g.N, g.H, g.W, g.Kout) : (size_t)g.M * g.Kout * sizeof(float);
}

int launch_cat(const CatGeom& g, const float* src, const float* w, const float* bias_per_image, const float* bnScale,
               float* out, hipStream_t s) {
  int dev = 0, cus = 0;
  if (int rc = current_device(&dev, &cus)) return rc;
  ProjGeo xg = {};
  xg.s = (unsigned)g.S;
  xg.cx = g.Cs;
  const Plan1x1 p = plan_cat(g, cus, knobs());
  Operands1x1 o{src, w, bias_per_image, bnScale, nullptr, out, g.M, g.S * g.Cs, g.Kout, g.flags, make_padgeo(g.H, g.W), xg};
  o.batchA = g.stride;
  return (p.four ? launch_tiled_1x1<4, A_CAT, RES_NONE> : launch_tiled_1x1<8, A_CAT, RES_NONE>)(p, dev, o, s);
}

int prepare_cat(const CatGeom& g, hipStream_t s) {
  int dev = 0, cus = 0;
  if (int rc = current_device(&dev, &cus)) return rc;
  const Plan1x1 p = plan_cat(g, cus, knobs());
  if (!p.sk) return WINO_OK;
  SkBufs bufs;
  return tiled_scratch(dev, s, p, &bufs);
}

// ---- the module ----
constexpr int ASPP_SPATIAL = 4;   // branch 0 and the three dilated ones: the sources of the join
size_t round256(size_t b) { return (b + 255) / 256 * 256; }
struct AsppGeom {
  int N, H, W, Cin, Cb, Kout;
  DilGeom dil[3];
  CatGeom cat;
  size_t pooled_b, branch_b, bias_b, slot_b;   // the workspace: pooled [N][Cin], its branch [N][Cb], bias [N][Kout], 4 slots
  size_t need() const { return pooled_b + branch_b + bias_b + ASPP_SPATIAL * slot_b; }
};

// every layer's shape check, in launch order
int check_aspp(int N, int H, int W, int Cin, int Cb, int Kout, const int rates[3], AsppGeom* g) {
  if (N < 1 || H < 1 || W < 1 || Cin < 1 || Cb < 1 || Kout < 1) {
    set_error("aspp: bad N=%d H=%d W=%d Cin=%d Cb=%d Kout=%d", N, H, W, Cin, Cb, Kout);
    return WINO_E_SHAPE;
  }
  if ((long)H * W >= (1l << 24) || (long)N * Cin >= (1l << 31)) {   // the average pool's counters
    set_error("aspp: shape N=%d H=%d W=%d Cin=%d out of range", N, H, W, Cin);
    return WINO_E_SHAPE;
  }
  if (int rc = check_1x1_hw(N, 1, 1, Cin, Cb)) return rc;      // the pooled branch, M = N
  if (int rc = check_1x1_hw(N, 1, 1, Cb, Kout)) return rc;     // its share of the projection, M = N
  if (int rc = check_1x1_hw(N, H, W, Cin, Cb)) return rc;      // branch 0
  for (int i = 0; i < 3; i++)
    if (int rc = check_dilated(N, H, W, Cin, Cb, rates[i], &g->dil[i])) return rc;
  const long M = (long)N * H * W;
  if (int rc = check_cat(N, H, W, ASPP_SPATIAL, Cb, Kout, M * Cb, WINO_RELU | WINO_C_PADDED, &g->cat)) return rc;
  g->N = N, g->H = H, g->W = W, g->Cin = Cin, g->Cb = Cb, g->Kout = Kout;
  g->pooled_b = round256((size_t)N * Cin * sizeof(float));
  g->branch_b = round256((size_t)N * Cb * sizeof(float));
  g->bias_b = round256((size_t)N * Kout * sizeof(float));
  g->slot_b = (size_t)M * Cb * sizeof(float);
  return WINO_OK;
}

}  // namespace
}  // namespace wino

using namespace wino;

extern "C" {

int wino_conv1x1_cat_bn_hw(const float* src, long src_stride, const float* w, const float* bias_per_image,
                           const float* bnScale, float* out, int N, int H, int W, int sources, int Cs, int Kout,
                           int flags, wino_stream_t s) {
  if (int rc = check_nonnull(src, w, bias_per_image, bnScale, out)) return rc;
  if (int rc = check_aligned16(src, w, bias_per_image, out)) return rc;
  if (flags & ~CAT_FLAGS) { set_error("concat 1x1: unknown flag bits 0x%x", flags); return WINO_E_ARG; }
  CatGeom g;
  if (int rc = check_cat(N, H, W, sources, Cs, Kout, src_stride, flags, &g)) return rc;
  if (any_overlap({{src, cat_src_bytes(g)}, {out, cat_out_bytes(g)}, {bias_per_image, (size_t)N * Kout * sizeof(float)}})) {
    set_error("concat 1x1: the sources, bias_per_image and out overlap");
    return WINO_E_ARG;
  }
  return launch_cat(g, src, w, bias_per_image, bnScale, out, (hipStream_t)s);
}

int wino_conv1x1_cat_prepare_hw(int N, int H, int W, int sources, int Cs, int Kout, wino_stream_t s) {
  CatGeom g;
  if (int rc = check_cat_gemm(N, H, W, sources, Cs, Kout, &g)) return rc;
  return prepare_cat(g, (hipStream_t)s);
}

int wino_conv1x1_cat_plan(int N, int H, int W, int sources, int Cs, int Kout, int cus, int* form) {
  if (!form || cus < 1) { set_error("bad argument"); return WINO_E_ARG; }
  CatGeom g;
  if (int rc = check_cat_gemm(N, H, W, sources, Cs, Kout, &g)) return rc;
  *form = plan_cat(g, cus, knobs()).sk ? WINO_1X1_FORM_STREAM_K : WINO_1X1_FORM_TILED;
  return WINO_OK;
}

int wino_aspp_hw(const float* in, const float* w0, const float* bn0Bias, const float* bn0Scale, const float* w1_taps,
                 const float* bn1Bias, const float* bn1Scale, const float* w2_taps, const float* bn2Bias,
                 const float* bn2Scale, const float* w3_taps, const float* bn3Bias, const float* bn3Scale,
                 const float* w_pool, const float* bnpBias, const float* bnpScale, const float* w_proj,
                 const float* bnBias, const float* bnScale, float* out, int N, int H, int W, int Cin, int Cb, int Kout,
                 int d1, int d2, int d3, void* workspace, size_t workspace_bytes, wino_stream_t s) {
  if (int rc = check_nonnull(in, w0, bn0Bias, bn0Scale, w1_taps, bn1Bias, bn1Scale, w2_taps, bn2Bias, bn2Scale, w3_taps,
                             bn3Bias, bn3Scale, w_pool, bnpBias, bnpScale, w_proj, bnBias, bnScale, out))
    return rc;
  if (int rc = check_aligned16(in, w0, w1_taps, w2_taps, w3_taps, w_pool, w_proj, out, workspace)) return rc;
  const int rates[3] = {d1, d2, d3};
  AsppGeom g;
  if (int rc = check_aspp(N, H, W, Cin, Cb, Kout, rates, &g)) return rc;
  if (int rc = check_workspace(workspace, workspace_bytes, g.need())) return rc;
  if (any_overlap({{in, padded_bytes(N, H, W, Cin)}, {out, padded_bytes(N, H, W, Kout)}, {workspace, g.need()}})) {
    set_error("aspp: in, out and the workspace overlap");
    return WINO_E_ARG;
  }
  const hipStream_t hs = (hipStream_t)s;
  float* pooled = (float*)workspace;
  float* branch = (float*)((char*)pooled + g.pooled_b);
  float* bias = (float*)((char*)branch + g.branch_b);
  float* slots = (float*)((char*)bias + g.bias_b);
  const long slot = g.cat.stride;
  // the pooled branch, folded into the projection's per-image bias: bias[n] = bnScale * (branch[n] . w_proj[4 Cb ..]) + bnBias
  if (int rc = launch_avgpool(in, pooled, N, H, W, Cin, 1, hs)) return rc;
  if (int rc = wino_conv1x1_bn(pooled, w_pool, bnpBias, bnpScale, branch, N, Cin, Cb, 1, s)) return rc;
  if (int rc = wino_conv1x1_bn(branch, w_proj + (size_t)ASPP_SPATIAL * Cb * Kout, bnBias, bnScale, bias, N, Cb, Kout, 0, s))
    return rc;
  // the four spatial branches into their unpadded slots: nothing reads a ring there, so no ring pass runs
  if (int rc = wino_conv1x1_bn_ex_hw(in, w0, bn0Bias, bn0Scale, NULL, slots, N, H, W, Cin, Cb, WINO_RELU | WINO_A_PADDED, s))
    return rc;
  const float* taps[3] = {w1_taps, w2_taps, w3_taps};
  const float* tb[3] = {bn1Bias, bn2Bias, bn3Bias};
  const float* ts[3] = {bn1Scale, bn2Scale, bn3Scale};
  for (int i = 0; i < 3; i++)
    if (int rc = launch_dilated(g.dil[i], in, taps[i], tb[i], ts[i], slots + (i + 1) * slot, true, false, hs)) return rc;
  // the join and the projection
  return launch_cat(g.cat, slots, w_proj, bias, bnScale, out, hs);
}

int wino_aspp_prepare_hw(int N, int H, int W, int Cin, int Cb, int Kout, int d1, int d2, int d3, wino_stream_t s) {
  const int rates[3] = {d1, d2, d3};
  AsppGeom g;
  if (int rc = check_aspp(N, H, W, Cin, Cb, Kout, rates, &g)) return rc;
  if (int rc = wino_conv1x1_prepare(N, Cin, Cb, s)) return rc;
  if (int rc = wino_conv1x1_prepare(N, Cb, Kout, s)) return rc;
  if (int rc = wino_conv1x1_prepare(g.cat.M, Cin, Cb, s)) return rc;
  for (int i = 0; i < 3; i++)
    if (int rc = wino_conv3x3_dilated_prepare_hw(N, H, W, Cin, Cb, rates[i], s)) return rc;
  return prepare_cat(g.cat, (hipStream_t)s);
}

}  // extern "C"
