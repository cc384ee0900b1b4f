// Fused Winograd F(2x2,3x3) convolution + folded BN + ReLU for gfx950 (MI355X): the filter transforms, prepare, the
// plain layer's launch entry points and the clock probe.  The kernel is wino_f2_fused_kernel.h, the launcher
// wino_f2_launch.h, the launch planner wino_f2_plan.hip.
//
// Replaces the reference's three launches
//   kernel_{128,256}_winograd_BtdB -> kernel_*_OuterProduct_* -> kernel_*_winograd_AtIA
//   (Kernel128_winograd.cu:28-213, Kernel256_winograd.cu:27-218)
// with ONE kernel; the Winograd-domain tensors V (input) and M (products) never touch
// memory.  Design:
//
//   item       = TB=64 tiles x KB=64 out-channels x all 16 Winograd points; C is streamed in
//                chunks of BC=8 channels ("chunk iterations").  The launch is balanced by
//                iterations: whole-item rounds + a stream-K tail (wino_f2_fused_kernel.h).
//   workgroup  = 512 threads = 8 waves (2 per SIMD), all 160 KB of the CU's LDS.
//   wave (wt,ph) = 16 tiles x all 64 out-channels x 8 of the 16 points (rows 2 ph, 2 ph + 1 of the point grid)
//                = 32 accumulator tiles of v_mfma_f32_16x16x4_f32 (128 acc VGPRs); no two waves repeat a
//                  transform (round 1: 16 tiles x 32 out-channels x 16 points, B^T d B twice per tile block).
//   per chunk  : LDS-DMA (buffer_load_dwordx4 ... lds) stages
//                  raw[64 tiles][16 px][8 c]   (the 4x4 input patches, 32 KB, 2 stages)
//                  U  [16 pts][64 k][8 c]      (pre-packed filter chunk, 32 KB, 3 stages)
//                two iterations ahead of the MFMAs, continuously across items.
//   A operand  : each lane reads 3 of its tile's 4 patch rows for 2 channels (12 x ds_read_b64, addresses held
//                as absolute LDS pointers in registers) and applies its half of B^T d B in registers (16 packed
//                operations) -> V[8 pts]; no cross-lane traffic is needed because the MFMA A-fragment wants
//                exactly "one tile row, one channel" per lane.
//   B operand  : ds_read_b64 of the packed filter chunk.
//   loop       : two copies of the body, one per raw-stage parity (the stage is an immediate of the patch reads).
//   epilogue   : the wave's partial A^T m A (its two point rows) in-lane; the halves of a (tile, out-channel)
//                meet through LDS (wave pair w, w ^ 1), after which wave (wt, ph) owns 16 tiles x 32
//                out-channels: scale*y+bias, ReLU; the tiles go through the wave's own 8 KB of LDS and leave as
//                whole 128-byte runs of the padded NHWC output; the zero ring is written once per
//                launch by a flat ring pass.
// Small batches (the reference's N = 1) take wino_f2_small_kernel.h instead; feature maps other
// than 14x14 run the same kernel with the geometry in its arguments (GEN = true).
//
// LDS bank-conflict avoidance is done by XOR-permuting 16-byte units, applied on the DMA
// *source* address for the raw patches (the LDS destination of an LDS-DMA is lane-linear)
// and baked into the packed filter layout for U.
#include "wino_f2_launch.h"

namespace wino {
namespace {

using namespace fused;

// Position (in floats, 0..7) inside the 8-channel group of the packed filter at which
// channel `cl` (0..7) of out-channel `kl` (0..63 within the k-block) is stored: the
// 8-byte quarter index is XORed with 2*bit3(kl) so that the B-fragment ds_read_b64 of
// lanes (n, h) and (n+8, h) hit different bank groups.
__host__ __device__ constexpr int u_pos(int kl, int cl) {
  return ((((cl >> 1) ^ (((kl >> 3) & 1) << 1)) << 1) | (cl & 1));
}

__host__ __device__ inline size_t u_index(int C, int K, int e, int c, int k) {
  (void)C;
  const int it = c >> 3, cl = c & 7, kb = k >> 6, kl = k & 63;
  return ((((size_t)it * (K >> 6) + kb) * 16 + e) * 64 + kl) * 8 + u_pos(kl, cl);
}

// ---------------------------------------------------------------------------------
// Filter transforms (offline; reference: data_generator.py:63-78)
// ---------------------------------------------------------------------------------
__device__ __forceinline__ void f2_from_taps(const double g[3][3], double u[4][4]) {
  // G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]];  u = G g G^T
  double t[4][3];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    t[0][j] = g[0][j];
    t[1][j] = 0.5 * (g[0][j] + g[1][j] + g[2][j]);
    t[2][j] = 0.5 * (g[0][j] - g[1][j] + g[2][j]);
    t[3][j] = g[2][j];
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    u[i][0] = t[i][0];
    u[i][1] = 0.5 * (t[i][0] + t[i][1] + t[i][2]);
    u[i][2] = 0.5 * (t[i][0] - t[i][1] + t[i][2]);
    u[i][3] = t[i][2];
  }
}

__global__ void filter_transform_f2_kernel(const float* __restrict__ w, float* __restrict__ U,
                                           int C, int K) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= C * K) return;
  const int k = idx / C, c = idx - k * C;
  double g[3][3], u[4][4];
  const float* p = w + (size_t)idx * 9;  // [K][C][3][3]
#pragma unroll
  for (int i = 0; i < 9; i++) g[i / 3][i % 3] = (double)p[i];
  f2_from_taps(g, u);
#pragma unroll
  for (int e = 0; e < 16; e++) U[u_index(C, K, e, c, k)] = (float)u[e >> 2][e & 3];
}

// u36 [36][C][K] = G4 g G4^T  ->  g = L u36 L^T with L = [[4,0,0,0,0,0],[0,-3,3,0,0,0],[0,0,0,0,0,1]]
// (L G4 = I for the reference's G4, data_generator.py:65), then the F(2x2) transform.
__global__ void filter_import_f4_kernel(const float* __restrict__ u36, float* __restrict__ U,
                                        int C, int K) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // c*K + k  (k fastest: coalesced)
  if (idx >= C * K) return;
  const int c = idx / K, k = idx - c * K;
  double m[6][6];
#pragma unroll
  for (int e = 0; e < 36; e++) m[e / 6][e % 6] = (double)u36[(size_t)e * C * K + idx];
  double t[3][6];
#pragma unroll
  for (int j = 0; j < 6; j++) {
    t[0][j] = 4.0 * m[0][j];
    t[1][j] = 3.0 * (m[2][j] - m[1][j]);
    t[2][j] = m[5][j];
  }
  double g[3][3], u[4][4];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    g[i][0] = 4.0 * t[i][0];
    g[i][1] = 3.0 * (t[i][2] - t[i][1]);
    g[i][2] = t[i][5];
  }
  f2_from_taps(g, u);
#pragma unroll
  for (int e = 0; e < 16; e++) U[u_index(C, K, e, c, k)] = (float)u[e >> 2][e & 3];
}

}  // namespace
}  // namespace wino

using namespace wino;

extern "C" {

size_t wino_filter_f2_elems(int C, int K) { return (size_t)16 * C * K; }

long wino_filter_f2_index(int C, int K, int e, int c, int k) {
  if (C <= 0 || K <= 0 || (C % 8) || (K % 64) || e < 0 || e >= 16 || c < 0 || c >= C || k < 0 || k >= K)
    return -1;
  return (long)u_index(C, K, e, c, k);
}

int wino_filter_transform_f2(const float* w_kcrs, float* U, int C, int K, wino_stream_t s) {
  if (int rc = check_nonnull(w_kcrs, U)) return rc;
  if (int rc = check_aligned16(U)) return rc;
  if (int rc = check_ck(C, K)) return rc;
  const int n = C * K;
  hipLaunchKernelGGL(filter_transform_f2_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     (hipStream_t)s, w_kcrs, U, C, K);
  return launch_status("filter_transform_f2_kernel");
}

int wino_filter_import_f4(const float* u36, float* U, int C, int K, wino_stream_t s) {
  if (int rc = check_nonnull(u36, U)) return rc;
  if (int rc = check_aligned16(U)) return rc;
  if (int rc = check_ck(C, K)) return rc;
  const int n = C * K;
  hipLaunchKernelGGL(filter_import_f4_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     (hipStream_t)s, u36, U, C, K);
  return launch_status("filter_import_f4_kernel");
}

}  // extern "C"

static int conv3x3_prepare(int N, int H, int W, int C, int K, hipStream_t s) {
  if (int rc = check_conv3x3_dims(H, W, C, K)) return rc;
  if (N < 1) { set_error("bad batch N=%d", N); return WINO_E_SHAPE; }
  {   // a batch the launcher splits: its largest launch decides the scratch
    long long step = conv3x3_batch_limit(H, W, C, K);
    if (N > step) N = (int)(step > 64 ? step - step % 64 : step);
  }
  if (int rc = check_conv3x3(N, H, W, C, K)) return rc;
  int dev = 0;
  Plan3x3 p;
  if (int rc = plan_3x3_here(N, H, W, C, K, false, &dev, &p)) return rc;
  SkBufs bufs;
  if (p.small.use) return small_scratch(dev, s, p.small, &bufs);
  return sk_workspace(dev, s, p.G, (size_t)p.items, &bufs);
}

// Diagnostic: the throughput kernel's stamped build (ABLATE = PROBE_CLOCK: s_memtime / s_memrealtime at the start
// and at the end of every workgroup's main loop, each pair stored at once, CLK_WORDS per workgroup in `stamps`
// (wino_probe.h); the outputs are the product kernel's).  bench.py runs it right
// after its timed region to report the clock the chip holds inside THIS kernel under sustained load.
static int conv3x3_clock_probe(const float* in, const float* U, const float* bnBias, const float* bnScale,
                               float* out, int N, int C, int K, unsigned long long* stamps, int* workgroups,
                               hipStream_t s) {
  if (int rc = check_nonnull(in, U, bnBias, bnScale, out, stamps, workgroups)) return rc;
  if (int rc = check_conv3x3(N, WINO_PQ, WINO_PQ, C, K)) return rc;
  int dev = 0;
  Plan3x3 p;
  if (int rc = plan_3x3_here(N, WINO_PQ, WINO_PQ, C, K, true, &dev, &p)) return rc;
  if (p.G > 2048) { set_error("clock probe: grid %d exceeds the stamp buffer", p.G); return WINO_E_SHAPE; }
  SkBufs bufs;
  if (int rc = sk_workspace(dev, s, p.G, (size_t)p.items, &bufs)) return rc;
  FusedParams prm = p.fp;
  prm.in = in, prm.Uq = U, prm.relu = 1, prm.bnBias = bnBias, prm.bnScale = bnScale, prm.out = out;
  prm.slabs = bufs.slabs, prm.tickets = bufs.tickets, prm.err = bufs.err, prm.dbg = stamps;
  if (int rc = lds_cap_once<wino_f2_fused_kernel<PROBE_CLOCK, false>>(dev, LDS_BYTES)) return rc;
  hipLaunchKernelGGL((wino_f2_fused_kernel<PROBE_CLOCK, false>), dim3(p.G), dim3(NTHREADS), LDS_BYTES, s, prm);
  *workgroups = p.G;
  return launch_status("wino_f2_fused_kernel (stamped)");
}

extern "C" {

int wino_diag_conv3x3_clock(const float* in, const float* U, const float* bnBias, const float* bnScale,
                            float* out, int N, int C, int K, unsigned long long* stamps_dev,
                            int* workgroups, wino_stream_t s) {
  return conv3x3_clock_probe(in, U, bnBias, bnScale, out, N, C, K, stamps_dev, workgroups, (hipStream_t)s);
}

int wino_diag_last_clock(int kernel, wino_stream_t s, unsigned long long stamps[4]) {
  if (!stamps || (kernel != 0 && kernel != 1)) { set_error("bad argument"); return WINO_E_ARG; }
  WINO_HIP(hipStreamSynchronize((hipStream_t)s));
  if (kernel == 1) return wino::last_clock_1x1(stamps);
  WINO_HIP(hipMemcpyFromSymbol(stamps, HIP_SYMBOL(wino::fused::wino_clk_slot_3x3), 4 * sizeof(unsigned long long)));
  return WINO_OK;
}

int wino_conv3x3_prepare(int N, int C, int K, wino_stream_t s) {
  return conv3x3_prepare(N, WINO_PQ, WINO_PQ, C, K, (hipStream_t)s);
}

int wino_conv3x3_prepare_hw(int N, int H, int W, int C, int K, wino_stream_t s) {
  return conv3x3_prepare(N, H, W, C, K, (hipStream_t)s);
}

int wino_conv3x3_bn_relu(const float* in, const float* U, const float* bnBias,
                         const float* bnScale, float* out, int N, int C, int K, int relu,
                         wino_stream_t s) {
  return wino_conv3x3_bn_relu_hw(in, U, bnBias, bnScale, out, N, WINO_PQ, WINO_PQ, C, K, relu, s);
}

int wino_conv3x3_bn_relu_hw(const float* in, const float* U, const float* bnBias,
                            const float* bnScale, float* out, int N, int H, int W, int C, int K,
                            int relu, wino_stream_t s) {
  if (int rc = check_nonnull(in, U, bnBias, bnScale, out)) return rc;
  if (int rc = check_aligned16(in, U, out)) return rc;
  return conv3x3_launch<false>(in, U, bnBias, bnScale, nullptr, out, N, H, W, C, K, relu, (hipStream_t)s);
}

}  // extern "C"
