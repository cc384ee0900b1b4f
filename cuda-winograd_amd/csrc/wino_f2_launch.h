// The 3x3 F(2x2,3x3) layers' launch plan and launcher, shared by the translation units that launch them:
// wino_f2_fused.hip (the plain epilogue, EPI = EPI_PLAIN), conv3x3_res.hip (the residual epilogue, EPI = EPI_RES: the
// second 3x3 of a ResNet basic block) and conv3x3_pool.hip (the pooled epilogue, EPI = EPI_POOL: a VGG layer followed
// by MaxPool2d(2, 2)).  A template is instantiated where it is used, so each file compiles the kernels of its
// own epilogue and no others.  The planner (plan_3x3, plan_3x3_here) is defined once, in wino_f2_plan.hip: a residual
// launch and a pooled launch take exactly the plan of the plain layer of the same shape.
#pragma once
#include "wino_f2_small_kernel.h"

namespace wino {
using namespace fused;

inline int check_ck(int C, int K) {
  if (C <= 0 || K <= 0 || (C % 8) != 0 || (K % 64) != 0) {
    set_error("unsupported channels C=%d K=%d (need C %% 8 == 0, K %% 64 == 0)", C, K);
    return WINO_E_SHAPE;
  }
  return WINO_OK;
}

// ---------------------------------------------------------------------------------
// Stream-K scratch of this kernel: 2 slabs of SLAB_BYTES per logical workgroup, one ticket counter
// per (item, wave); the per-(device, stream) set lives in wino_runtime.hip (sk_scratch).
// ---------------------------------------------------------------------------------
inline int sk_workspace(int dev, hipStream_t s, int G, size_t items, SkBufs* bufs) {
  const size_t wgs = G < 256 ? 256 : (size_t)G;
  return sk_scratch(dev, s, 2 * wgs * SLAB_BYTES, items * 8, bufs);
}

// The largest batch one launch takes: the kernels address the tensors with 32-bit byte offsets
// (both tensors must stay below 4 GiB) and the stream-K bookkeeping counts chunk iterations in
// 32 bits.  Larger batches are split by the launcher (images are independent).
inline long long conv3x3_batch_limit(int H, int W, int C, int K) {
  const unsigned long long per_image = (unsigned long long)(H + 2) * (W + 2) * (unsigned long long)(C > K ? C : K) * sizeof(float);
  long long n = (long long)((FOUR_GIB - 1) / per_image);
  const long long tiles = (long long)((H + 1) / 2) * ((W + 1) / 2);
  const long long per_tb = (long long)(K / KB) * (C / BC);               // chunk iterations per 64-tile block
  const long long max_tb = ((1ll << 31) - 1) / per_tb - 1;
  const long long n_iter = max_tb * TB / tiles;
  if (n > n_iter) n = n_iter;
  if (n > (1ll << 30)) n = 1ll << 30;
  return n;
}

// one launch
inline int check_conv3x3(int N, int H, int W, int C, int K) {
  if (int rc = check_conv3x3_dims(H, W, C, K)) return rc;
  if (N < 1 || N > conv3x3_batch_limit(H, W, C, K)) {
    set_error("bad batch N=%d (one launch takes 1..%lld images of this shape: input/output below 4 GiB)", N,
              conv3x3_batch_limit(H, W, C, K));
    return WINO_E_SHAPE;
  }
  return WINO_OK;
}

// The latency kernel's form for one launch (wino_f2_small_kernel.h), or use = false: the throughput kernel runs.  The
// policy is small_plan's (wino_f2_plan.hip).
struct SmallPlan {
  bool use;
  int split, nT16;       // nT16: blocks of 16 tiles
  size_t blocks;
  int ct;                // MFMA tiles per wave, side by side
  double t_us;           // the model's time
};

inline int small_scratch(int dev, hipStream_t s, const SmallPlan& pl, SkBufs* bufs) {
  bufs->slabs = nullptr; bufs->tickets = nullptr; bufs->err = nullptr;
  if (pl.split <= 1) return WINO_OK;
  return sk_scratch(dev, s, pl.blocks * pl.split * pl.ct * SMALL_SLAB_BYTES, pl.blocks, bufs);
}

// The plan of one launch, read by every consumer -- the launch, prepare, the clock probe and the wino_conv3x3_*plan*
// queries: the latency kernel's form and, when that kernel does not run or `throughput` asks for it all the same, the
// throughput kernel's grid and work layout.
struct Plan3x3 {
  SmallPlan small;
  Geo geo;
  int G;            // logical workgroups of the throughput kernel
  long long items;
  FusedParams fp;   // its shape and work layout; the tensor and scratch pointers are filled in at launch
};
Plan3x3 plan_3x3(int N, int H, int W, int C, int K, int cus, const Knobs& kn, bool throughput);
// the plan of a launch on the current device; *dev receives the device
int plan_3x3_here(int N, int H, int W, int C, int K, bool throughput, int* dev, Plan3x3* p);

// the latency kernel's instantiations by [CT / 2]: the 14x14 form (GEN = false; it has no pooled epilogue) and the
// general one
template <int EPI>
constexpr decltype(&wino_f2_small_kernel<1, false, false, EPI>) SMALL_3X3_FIXED14[3] = {
    wino_f2_small_kernel<1, false, false, EPI>, wino_f2_small_kernel<2, false, false, EPI>,
    wino_f2_small_kernel<4, false, false, EPI>};
template <int EPI>
constexpr decltype(&wino_f2_small_kernel<1, true, false, EPI>) SMALL_3X3_GENERAL[3] = {
    wino_f2_small_kernel<1, true, false, EPI>, wino_f2_small_kernel<2, true, false, EPI>,
    wino_f2_small_kernel<4, true, false, EPI>};

template <bool GEN, bool TAIL, int EPI>
int launch_fused(const FusedArgs<EPI == EPI_RES>& prm, int G, int dev, hipStream_t s) {
  // all 160 KB of the CU's LDS
  if (int rc = lds_cap_once<wino_f2_fused_kernel<0, GEN, TAIL, EPI>>(dev, LDS_BYTES)) return rc;
  hipLaunchKernelGGL((wino_f2_fused_kernel<0, GEN, TAIL, EPI>), dim3(G), dim3(NTHREADS), LDS_BYTES, s, prm);
  const int rc = launch_status("wino_f2_fused_kernel");
  if (rc) sk_mark_failed(dev, s);   // the launch held the stream's scratch
  return rc;
}

// One launch of `plan_3x3_here`'s plan, with the epilogue EPI.  EPI_RES: out = act(bnScale*conv + bnBias + res), res
// padded like out (EPI_PLAIN and EPI_POOL do not read res).  EPI_POOL: out = maxpool2x2_s2(act(bnScale*conv + bnBias)),
// [N][H/2+2][W/2+2][K].  The plan is the plain layer's in every form.
template <int EPI>
int conv3x3_launch_one(const float* in, const float* U, const float* bnBias, const float* bnScale, const float* res,
                       float* out, int N, int H, int W, int C, int K, int relu, hipStream_t s) {
  constexpr bool RES = EPI == EPI_RES;
  if (int rc = check_conv3x3(N, H, W, C, K)) return rc;
  const bool fixed14 = H == WINO_PQ && W == WINO_PQ;
  int dev = 0;
  Plan3x3 p;
  if (int rc = plan_3x3_here(N, H, W, C, K, false, &dev, &p)) return rc;
  if (p.small.use) {
    const SmallPlan& sp = p.small;
    SkBufs bufs;
    if (int rc = small_scratch(dev, s, sp, &bufs)) return rc;
    SmallArgs<RES> prm;
    static_cast<SmallParams&>(prm) = {in, U, bnBias, bnScale, out, N, C, K, relu, bufs.slabs, bufs.tickets, bufs.err, nullptr, p.geo};
    if constexpr (RES) prm.res = res;
    const dim3 grid(K / (16 * sp.ct), sp.nT16, sp.split), block(64 * SMALL_WAVES);   // x = out-channel block: see the kernel
    // (a pooled 14x14 launch takes the general form: the 14x14 one writes its ring per tile, for a 16x16 output)
    if constexpr (EPI == EPI_POOL)
      hipLaunchKernelGGL((SMALL_3X3_GENERAL<EPI>[sp.ct >> 1]), grid, block, 0, s, prm);
    else
      hipLaunchKernelGGL((fixed14 ? SMALL_3X3_FIXED14<EPI>[sp.ct >> 1] : SMALL_3X3_GENERAL<EPI>[sp.ct >> 1]), grid, block, 0, s, prm);
    const int rc = launch_status("wino_f2_small_kernel");
    if (rc && sp.split > 1) sk_mark_failed(dev, s);
    return rc;
  }
  SkBufs bufs;
  if (int rc = sk_workspace(dev, s, p.G, (size_t)p.items, &bufs)) return rc;
  FusedArgs<RES> prm;
  static_cast<FusedParams&>(prm) = p.fp;
  prm.in = in, prm.Uq = U, prm.relu = relu, prm.bnBias = bnBias, prm.bnScale = bnScale, prm.out = out;
  prm.slabs = bufs.slabs, prm.tickets = bufs.tickets, prm.err = bufs.err;
  if constexpr (RES) prm.res = res;
  // whole items only (no stream-K tail): the kernel variant without the hand-off in its epilogue
  if (p.items % p.G == 0)
    return fixed14 ? launch_fused<false, false, EPI>(prm, p.G, dev, s) : launch_fused<true, false, EPI>(prm, p.G, dev, s);
  return fixed14 ? launch_fused<false, true, EPI>(prm, p.G, dev, s) : launch_fused<true, true, EPI>(prm, p.G, dev, s);
}

// Any batch: batches whose tensors would reach 4 GiB go out as several launches of whole images
// (a multiple of 64 images each, so that every launch but the last fills its 64-tile blocks).  The residual has
// K channels, like out: it advances with out, and the per-image limit already covers it.  POOL: the output image is
// the pooled one, (H/2+2) x (W/2+2) x K -- smaller than the un-pooled image the limit is taken from.
// The caller has checked the pointers.
template <int EPI>
int conv3x3_launch(const float* in, const float* U, const float* bnBias, const float* bnScale, const float* res,
                   float* out, int N, int H, int W, int C, int K, int relu, hipStream_t s) {
  constexpr bool RES = EPI == EPI_RES, POOL = EPI == EPI_POOL;
  if (int rc = check_conv3x3_dims(H, W, C, K)) return rc;
  if (N < 1) { set_error("bad batch N=%d", N); return WINO_E_SHAPE; }
  long long step = conv3x3_batch_limit(H, W, C, K);
  if (N <= step) return conv3x3_launch_one<EPI>(in, U, bnBias, bnScale, res, out, N, H, W, C, K, relu, s);
  if (step > 64) step -= step % 64;
  const size_t in_img = (size_t)(H + 2) * (W + 2) * C;
  const size_t out_img = POOL ? (size_t)(H / 2 + 2) * (W / 2 + 2) * K : (size_t)(H + 2) * (W + 2) * K;
  for (long long n0 = 0; n0 < N; n0 += step) {
    const int n = (int)(N - n0 < step ? N - n0 : step);
    if (int rc = conv3x3_launch_one<EPI>(in + (size_t)n0 * in_img, U, bnBias, bnScale, RES ? res + (size_t)n0 * out_img : nullptr,
                                         out + (size_t)n0 * out_img, n, H, W, C, K, relu, s)) return rc;
  }
  return WINO_OK;
}

}  // namespace wino
