/*
 * winograd_mi355x.h -- C-ABI of libwinograd_mi355x.so
 *
 * MI355X (gfx950) native fused Winograd F(2x2,3x3) conv + BN + ReLU and
 * 1x1-conv GEMM + BN (+ReLU).  Plain C: pointers, sizes, ints.  No HIP or
 * torch types; a stream is passed as an opaque `void*` (a hipStream_t, NULL =
 * the default stream).  All `float*` tensor arguments are DEVICE pointers
 * unless a name ends in `_host`.
 *
 * Every function returns WINO_OK (0) or a negative WINO_E_* code;
 * wino_last_error_string() describes the last failure of the calling thread.
 * Nothing here falls back to the CPU: without a usable GPU every compute entry
 * point fails with WINO_E_HIP.
 *
 * Reference interface each group replaces (paths into bssrdf/CUDA-Winograd):
 *   runtime plumbing   cudaSetDevice (Test.c:15), cudaMalloc/cudaMemset/cudaMemcpy/
 *                      cudaFree/cudaDeviceSynchronize/cudaGetErrorName
 *                      (Kernel128_winograd.cu:236-286)
 *   filter transforms  data_generator.py:63-78 (offline G g G^T)
 *   wino_conv3x3_*     the three launches kernel_{128,256}_winograd_BtdB ->
 *                      kernel_*_OuterProduct_* -> kernel_*_winograd_AtIA
 *                      (Kernel128_winograd.cu:263-265, Kernel256_winograd.cu:266-268)
 *   wino_conv1x1_bn    kernel_512_one_128 / kernel_128_one_512 (Kernel128_one.cu:98,316),
 *                      kernel_1024_one_256 / kernel_256_one_1024 (Kernel256_one.cu:100,318)
 *   wino_conv3x3_direct  the comparator role cuDNN plays in the reference
 *                      (Kernel128_winograd.cu:382-404), as an independent
 *                      non-Winograd GPU kernel
 * The six argument-less reference entry points themselves are declared in
 * Kernel128_winograd.h, Kernel256_winograd.h, Kernel128_one.h, Kernel256_one.h
 * (same directory) and exported by the same library.
 */
#ifndef WINOGRAD_MI355X_H
#define WINOGRAD_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped when an existing entry point changes meaning or signature; additions leave it alone.
 * Added since the first cut of version 1 (all additive): wino_conv3x3_prepare(_hw),
 * wino_conv3x3_bn_relu_hw, wino_conv3x3_direct_hw, wino_conv3x3_plan, wino_conv3x3_f4_*,
 * wino_conv1x1_prepare, wino_conv1x1_plan, wino_conv1x1_bn_ex_hw, wino_residual_block_hw,
 * wino_residual_block_workspace_bytes_hw; wino_stream_destroy now also releases the stream's
 * scratch; wino_conv3x3_bn_relu(_hw) take any batch (they used to reject tensors of 4 GiB);
 * wino_last_status_name, wino_debug_reload_knobs, wino_residual_block_prepare(_hw),
 * wino_driver_set_gpu_alias, wino_driver_set_stdout_compat, wino_driver_cpu_baseline,
 * wino_diag_conv3x3_clock, wino_debug_tickets_in_use, wino_stream_check, wino_stream_reset_scratch,
 * wino_debug_poison_ticket, wino_diag_last_clock, wino_conv3x3_small_plan, wino_conv1x1_small_plan,
 * wino_conv3x3_plan_groups, wino_conv1x1_small_plan2, wino_conv3x3_small_plan2, wino_debug_conv1x1_models,
 * WINO_E_STATE, wino_proj_tail_elems, wino_proj_tail_pack, wino_proj_block_workspace_bytes_hw,
 * wino_proj_block_prepare_hw, wino_proj_block_hw, wino_proj_tail_plan, WINO_1X1_FORM_*,
 * wino_conv3x3_s2_bn_relu_hw, wino_conv3x3_s2_prepare_hw, wino_conv3x3_s2_plan, wino_proj_block_v15_hw,
 * wino_proj_block_v15_workspace_bytes_hw, wino_proj_block_v15_prepare_hw, wino_conv3x3_bn_add_relu_hw,
 * wino_basic_block_workspace_bytes_hw, wino_basic_block_hw, wino_basic_block_prepare_hw, wino_s2_proj_elems,
 * wino_s2_proj_pack, wino_conv3x3_s2_proj_bn_relu_hw, wino_basic_block_s2_workspace_bytes_hw, wino_basic_block_s2_hw,
 * wino_basic_block_s2_prepare_hw, wino_stem_filter_elems, wino_stem_filter_pack, wino_stem_hw, wino_stem_plan,
 * wino_head_elems, wino_head_pack, wino_head_workspace_bytes, wino_head_prepare, wino_avgpool_fc_hw,
 * wino_conv3x3_bn_relu_pool_hw, wino_image_pack_hw, wino_avgpool7_flatten_hw, wino_conv3x3_grouped_filter_elems,
 * wino_conv3x3_grouped_filter_pack, wino_conv3x3_grouped_bn_relu_hw, wino_grouped_residual_block_hw,
 * wino_grouped_residual_block_prepare_hw, wino_grouped_proj_block_hw, wino_grouped_proj_block_prepare_hw,
 * WINO_RESIDUAL_UP2, wino_fpn_level_hw, wino_fpn_level_prepare_hw, wino_conv3x3_dilated_bn_relu_hw,
 * wino_conv3x3_dilated_prepare_hw, wino_conv3x3_dilated_plan, wino_dilated_residual_block_hw,
 * wino_dilated_residual_block_prepare_hw, wino_dilated_proj_block_hw, wino_dilated_proj_block_prepare_hw,
 * wino_conv1x1_cat_bn_hw, wino_conv1x1_cat_prepare_hw, wino_conv1x1_cat_plan, wino_aspp_hw,
 * wino_aspp_prepare_hw, wino_conv3x3_grouped_plan, wino_box_decode_hw, wino_batched_nms_hw,
 * wino_mask_paste_hw, WINO_MASK_LAYOUT_*, wino_select_topk_hw, wino_roi_align_launches,
 * wino_image_transform_hw, WINO_IMAGE_*, WINO_TRANSFORM_MAX_IMAGES, wino_transform_size,
 * wino_select_topk_map_hw, wino_retina_decode_hw, wino_groupnorm_relu_hw,
 * wino_groupnorm_plan, WINO_GN_FORM_*, wino_fcos_score_map_hw, wino_fcos_decode_hw,
 * wino_keypoints_hw, WINO_KP_LAYOUT_*, wino_roi_align_hw.  The library-owned stream-K scratch is never freed or moved while its
 * stream lives (it used to be reallocated when a larger shape arrived).  wino_residual_block(_hw) now also check every
 * pointer and both 1x1 layers' shapes before their first launch, and they and wino_proj_block(_v15)_hw refuse a
 * workspace that overlaps x or out (WINO_E_ARG): such calls used to launch part of the block, or to return WINO_OK
 * with a corrupted result. */
#define WINO_ABI_VERSION 1

enum {
  WINO_OK = 0,
  WINO_E_HIP = -1,       /* a HIP runtime call failed (no device, OOM, launch error) */
  WINO_E_SHAPE = -2,     /* unsupported / inconsistent shape argument */
  WINO_E_ARG = -3,       /* NULL pointer, bad enum, workspace too small, a tensor pointer that is not 16-byte aligned
                            (the kernels move 16 bytes per lane; wino_malloc / hipMalloc give 256; BN vectors need 4).
                            Pass a 256-byte-aligned workspace (what wino_malloc gives): the blocks carve their
                            intermediates from it.  16 is the checked minimum */
  WINO_E_STATE = -4,     /* the stream's library-owned scratch cannot be trusted (an earlier launch on it
                            failed or was aborted): wino_stream_reset_scratch() recovers */
};

/* geometry fixed by the reference's 14x14 stage */
#define WINO_HW 16        /* padded input / output extent */
#define WINO_PQ 14        /* valid output extent          */
#define WINO_TILES 49     /* F(2x2) tiles per image (7x7) */

typedef void* wino_stream_t;

/* ---- runtime plumbing (thin wrappers so that C hosts need no HIP headers) ---- */
int wino_abi_version(void);
const char* wino_last_error_string(void);
/* hipGetErrorName() of the status the calling thread's most recent memcpy / synchronise wrapper got
 * ("hipSuccess" when it worked): the line the reference prints after each copy-back,
 * cudaGetErrorName(cudaMemcpy(...)) (Kernel128_winograd.cu:274-275,408-409). */
const char* wino_last_status_name(void);
int wino_device_count(int* count);
int wino_set_device(int device);
int wino_device_name(int device, char* buf, size_t buflen);
int wino_malloc(void** dptr, size_t bytes);
int wino_free(void* dptr);
int wino_memset(void* dptr, int value, size_t bytes);
int wino_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes);
int wino_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes);
int wino_memcpy_d2d(void* dst_dev, const void* src_dev, size_t bytes);
int wino_device_synchronize(void);
int wino_stream_create(wino_stream_t* stream);
int wino_stream_destroy(wino_stream_t stream);   /* waits for the stream, frees the library's scratch of it */
int wino_stream_synchronize(wino_stream_t stream);
/* Fail-fast contract for the one piece of state the library keeps (the reference keeps none: every call
 * re-allocates, Kernel128_winograd.cu:236-256, and a CUDA error exits, :16-22).  The stream-K / split-C
 * kernels hand partial sums between workgroups through ticket counters that must be zero when a launch
 * begins; every launch returns them to zero.  A launch that fails on the host side, or a kernel that draws
 * a ticket on a counter that cannot have been zero at launch (a launch that died mid-way before it), puts
 * the (device, stream) into an error state: from then on every compute entry point on that stream returns
 * WINO_E_STATE instead of computing with counters it cannot trust.
 *   wino_stream_check          waits for the stream; WINO_OK or WINO_E_STATE
 *   wino_stream_reset_scratch  waits for the stream, zeroes its counters (slabs are kept), clears the state */
int wino_stream_check(wino_stream_t stream);
int wino_stream_reset_scratch(wino_stream_t stream);
/* events: timing on the stream the kernels run on (hipEvent based) */
int wino_event_create(void** event);
int wino_event_destroy(void* event);
int wino_event_record(void* event, wino_stream_t stream);
int wino_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on `stop` */

/* ---- 3x3: Winograd-domain filters ------------------------------------------ */
/* Number of floats of the packed F(2x2,3x3) filter buffer `U` for C in-channels and
 * K out-channels (= 16*C*K).  Its internal layout ([C/8][K/64][16][64][8], LDS-bank
 * swizzled) is private to the library. */
size_t wino_filter_f2_elems(int C, int K);
/* Position (in floats) of Winograd point e (0..15 = 4*row+col of G g G^T), in-channel c, out-channel k
 * inside the packed buffer; -1 for out-of-range arguments.  Host-side, no GPU needed. */
long wino_filter_f2_index(int C, int K, int e, int c, int k);
/* w_kcrs: [K][C][3][3] (weight_NCHW_C_K.bin) -> U.  G g G^T evaluated in fp64, stored fp32. */
int wino_filter_transform_f2(const float* w_kcrs, float* U, int C, int K, wino_stream_t s);
/* u36: the reference's pre-transformed F(4x4,3x3) weights [36][C][K]
 * (weight_winograd_C_K.bin, data_generator.py:63-78).  The 3x3 taps are recovered
 * exactly (g = L u L^T, L = left inverse of the reference's G) and re-transformed to
 * F(2x2,3x3), so the reference's weight file is consumed as is. */
int wino_filter_import_f4(const float* u36, float* U, int C, int K, wino_stream_t s);

/* ---- 3x3 conv + folded BN + ReLU ---------------------------------------------
 * in  [N][16][16][C]   NHWC, ring included (a valid conv of the 16x16 image)
 * U   from wino_filter_transform_f2 / wino_filter_import_f4
 * out [N][16][16][K]   14x14 result at [1..14][1..14], ring written as 0
 *                       (= the next 3x3 layer's padded input, Kernel128_winograd.cu:163)
 * out = relu(bnScale[k] * conv + bnBias[k]);  argument order (in, bias, scale, out)
 * follows kernel_*_winograd_AtIA (Kernel128_winograd.cu:123).
 * Constraints: C % 8 == 0, K % 64 == 0, N >= 1, and C * K < 2^26: the filter matrix U (16 C K floats, read through
 * one 32-bit buffer descriptor) stays below 4 GiB -- C = K = 8192 is refused (WINO_E_SHAPE), C = 8192 with K = 8128
 * runs.  Every entry point built on this layer (the residual 3x3, the basic blocks, the bottleneck and v1 projection
 * blocks) refuses such a shape before its first launch.  One launch.  The throughput kernel splits the
 * work evenly over the CUs (stream-K) and hands partial sums between workgroups through a small
 * scratch buffer the LIBRARY owns, one per (device, stream), allocated at the first call that needs
 * it (a synchronous hipMalloc).  Launches on one stream serialise, so they share it safely; two
 * host threads must not launch on the SAME stream concurrently. */
int wino_conv3x3_bn_relu(const float* in, const float* U, const float* bnBias,
                         const float* bnScale, float* out, int N, int C, int K, int relu,
                         wino_stream_t s);
/* Any N >= 1: one launch addresses its tensors with 32-bit byte offsets, so a batch whose input or
 * output would reach 4 GiB (N >= 16384 at 256 channels) goes out as several launches of whole images
 * on `s`.  wino_conv3x3_plan describes one launch and rejects such a batch. */
/* Allocates that scratch for (current device, `s`) and this shape ahead of time -- e.g. before
 * capturing wino_conv3x3_bn_relu / wino_residual_block into a HIP graph, where an allocation inside
 * the capture is not allowed.  Optional otherwise. */
int wino_conv3x3_prepare(int N, int C, int K, wino_stream_t s);

/* Other feature-map sizes (ResNet's 56x56 and 28x28 stages; the reference hard-codes
 * 14x14): H x W outputs (odd sizes such as the 7x7 stage included: the last tile row / column is
 * clipped), in [N][H+2][W+2][C], out [N][H+2][W+2][K] with the result at [1..H][1..W] and the ring
 * written as 0.  Same kernel, same packed filters; H = W = 14 is exactly
 * wino_conv3x3_bn_relu.  Small batches take the latency kernel at every feature map, as at 14x14. */
int wino_conv3x3_bn_relu_hw(const float* in, const float* U, const float* bnBias,
                            const float* bnScale, float* out, int N, int H, int W, int C, int K,
                            int relu, wino_stream_t s);
int wino_conv3x3_prepare_hw(int N, int H, int W, int C, int K, wino_stream_t s);

/* Host-side only (no GPU needed): the launch plan of the throughput kernel on a device with `cus`
 * compute units -- `grid` logical workgroups run `rounds` whole items each (item = 64 tiles x 64
 * out-channels, `iters_per_item` = C/8 chunk iterations) and share `tail_iters` further iterations
 * as a stream-K tail: workgroup l takes tail iterations [l*tail_iters/grid, (l+1)*tail_iters/grid). */
int wino_conv3x3_plan(int N, int H, int W, int C, int K, int cus, int* grid, int* rounds, long* tail_iters,
                      int* iters_per_item);
/* Host-side only: how that launch cuts and places its tail.  *groups = 1: one item-major list of tail_iters iterations
 * as described above; K/64 (taken whenever grid is a multiple of it): one list per out-channel block -- group k owns
 * the tail items of k-block k (item rounds*grid + groups*j + k, j = 0, 1, ...: one per tile block) and tail_iters /
 * groups iterations, cut into Gp = grid / groups equal ranges.  The workgroup l = groups*j + k at position j of group
 * k runs range  (phase_inv * (j / phase_copies)) % phase_period + phase_period * (j % phase_copies)  of its group: a
 * permutation of 0 .. Gp-1 (the identity for period 1) that gives the workgroups of one XCD -- consecutive positions
 * -- ranges starting at consecutive channel phases.  The groups' workgroups at one position walk the same tile blocks
 * and channel chunks in step and share the patches in the XCD's L2; neighbours in phase share the filter chunks. */
int wino_conv3x3_plan_groups(int N, int H, int W, int C, int K, int cus, int* groups, int* phase_period, int* phase_inv,
                             int* phase_copies);
/* Host-side only: whether this shape takes the latency kernel instead (small batches of any feature map: the
 * reference's own N = 1), and in which form: *point_rows (always 2 rows of the 4x4 point grid per wave task)
 * and *split (workgroups that share one 16-tile x 16-out-channel block's contraction, meeting through
 * library-owned slabs + tickets when > 1); *workgroups = blocks x split. */
int wino_conv3x3_small_plan(int N, int H, int W, int C, int K, int cus, int* use, int* point_rows, int* split,
                            int* workgroups);
/* The same with the block width: a wave holds *col_tiles MFMA tiles side by side (a block = 16 tiles x
 * 16 col_tiles out-channels; 1 at the reference's N = 1, 2 or 4 for the batches between that and the
 * throughput kernel's range). */
int wino_conv3x3_small_plan2(int N, int H, int W, int C, int K, int cus, int* use, int* point_rows, int* split,
                             int* col_tiles, int* workgroups);

/* ---- F(4x4,3x3) compatibility path ------------------------------
 * The reference's own three-stage arithmetic on its own pre-transformed weight file, consumed as is:
 * u36 = weight_winograd_C_K.bin, [36][C][K] (data_generator.py:63-78).  V = B^T d B (6x6 patches, 16
 * tiles per image), M_e = V_e . U_e for the 36 points (one batched MFMA GEMM launch), out = relu(scale *
 * A^T M A + bias) clipped to 14x14 (Kernel128_winograd.cu:28-213).  V and M live in `workspace`
 * (wino_conv3x3_f4_workspace_bytes), like the reference's t_input / ip buffers.  Same in / out layout as
 * wino_conv3x3_bn_relu.  Unfused and HBM-bound by design; the product path is the fused F(2x2) kernel.
 * Constraints: C % 32 == 0, K % 64 == 0. */
size_t wino_conv3x3_f4_workspace_bytes(int N, int C, int K);
int wino_conv3x3_f4_bn_relu(const float* in, const float* u36, const float* bnBias, const float* bnScale,
                            float* out, int N, int C, int K, int relu, void* workspace,
                            size_t workspace_bytes, wino_stream_t s);

/* Independent comparator: direct (non-Winograd) 3x3 conv + BN + ReLU on the GPU,
 * w_kcrs [K][C][3][3]; same in/out layout as above.  Slow by design. */
int wino_conv3x3_direct(const float* in, const float* w_kcrs, const float* bnBias,
                        const float* bnScale, float* out, int N, int C, int K, int relu,
                        wino_stream_t s);

int wino_conv3x3_direct_hw(const float* in, const float* w_kcrs, const float* bnBias,
                           const float* bnScale, float* out, int N, int H, int W, int C, int K,
                           int relu, wino_stream_t s);

/* ---- 1x1 conv as GEMM + folded BN (+ReLU) --------------------------------------
 * A [M][Cin] (M = N*196 pixels, HWC flat), B [Cin][Kout] row-major, C [M][Kout].
 * C = bnScale[k]*(A.B) + bnBias[k], ReLU if `relu`.  Argument order as the reference
 * kernels (A, B, bnBias, bnScale, C), Kernel128_one.cu:24.
 * Constraints: Cin % 32 == 0, Kout % 64 == 0 (workgroups are 128 columns wide when Kout % 128 == 0
 * and both dimensions exceed 128, 64 columns otherwise), M >= 1 (any M: the last row tile is ragged). */
int wino_conv1x1_bn(const float* A, const float* B, const float* bnBias, const float* bnScale,
                    float* C, long M, int Cin, int Kout, int relu, wino_stream_t s);
/* Extended form used when layers are chained (the residual block):
 *   WINO_RELU          ReLU after BN (+ residual)
 *   WINO_A_PADDED      A's rows are the 14x14 interior pixels of a padded [N][16][16][Cin] tensor
 *                      (what wino_conv3x3_bn_relu writes), M = N*196
 *   WINO_C_PADDED      C's rows go to the interior of a padded [N][16][16][Kout] tensor and the ring
 *                      is written as 0 (what wino_conv3x3_bn_relu reads), M = N*196
 *   WINO_ADD_RESIDUAL  C = act(bnScale*(A.B) + bnBias + residual), residual [M][Kout] unpadded
 * The reference has no such glue: its 1x1 layers are unpadded [196][C] and its 3x3 layers padded
 * [16][16][C], and no kernel adds the skip connection. */
#define WINO_RELU 1
#define WINO_A_PADDED 2
#define WINO_C_PADDED 4
#define WINO_ADD_RESIDUAL 8
/* wino_conv1x1_bn_ex_hw only, and only together with WINO_ADD_RESIDUAL (WINO_E_ARG otherwise): `residual` is the PADDED
 * coarser map [N][Hc+2][Wc+2][Kout], Hc = (H+1)/2, Wc = (W+1)/2, and output pixel (n, y, x) adds its pixel
 * (n, y>>1, x>>1) before the ReLU -- for this size pair exactly torch's F.interpolate(size=(H, W), mode="nearest"), the
 * top-down sum of a Feature Pyramid Network, without the upsampled tensor ever existing.  The residual's ring is never
 * read.  Combines freely with WINO_RELU, WINO_A_PADDED and WINO_C_PADDED; the launch plan is the plain layer's. */
#define WINO_RESIDUAL_UP2 16
int wino_conv1x1_bn_ex(const float* A, const float* B, const float* bnBias, const float* bnScale,
                       const float* residual, float* C, long M, int Cin, int Kout, int flags,
                       wino_stream_t s);
/* The same for any feature-map size: A [N*H*W][Cin] or, with WINO_A_PADDED,
 * [N][H+2][W+2][Cin]; C [N*H*W][Kout] or, with WINO_C_PADDED, [N][H+2][W+2][Kout] with its ring
 * written as 0 -- the layouts wino_conv3x3_bn_relu_hw reads and writes.  H = W = 14 is exactly
 * wino_conv1x1_bn_ex with M = N*196. */
int wino_conv1x1_bn_ex_hw(const float* A, const float* B, const float* bnBias, const float* bnScale,
                          const float* residual, float* C, int N, int H, int W, int Cin, int Kout,
                          int flags, wino_stream_t s);
/* Shapes whose tile count leaves the last round of workgroups mostly empty (the reference's
 * 512->128 and 1024->256 layers at N = 128: 448 tiles on 256 CUs) are launched in stream-K form
 * and use library-owned scratch of stream `s`, allocated on the first such launch.  Call this
 * once per (shape, stream) before capturing the layer into a HIP graph; it launches nothing.
 * Results do not depend on the launch form chosen beyond fp32 summation order, and are bitwise
 * reproducible from launch to launch.  WINO_1X1_SK=0 in the environment disables the form. */
int wino_conv1x1_prepare(long M, int Cin, int Kout, wino_stream_t s);
/* Host-side only (no GPU needed): the launch form of this shape on a device with `cus` compute
 * units.  The output is `row_tiles` x `col_blocks` tiles (112 rows x 64 or 128 columns) of
 * `k_steps` = Cin/32 pipeline steps.  stream_k = 0: `grid` workgroups, one whole tile each (some of
 * the grid may be padding).  stream_k = 1: the (row tile, k-step) space is cut into grid/col_blocks
 * equal ranges -- range r covers [r*T/R, (r+1)*T/R) of T = row_tiles*k_steps, R = grid/col_blocks --
 * and logical workgroup r*col_blocks + nb runs range r for column block nb. */
int wino_conv1x1_plan(long M, int Cin, int Kout, int cus, int* grid, int* row_tiles, int* col_blocks,
                      int* k_steps, int* stream_k);
/* Host-side only: layers with few pixel rows -- the reference's own M = 196 -- take a latency form instead of the
 * tiled kernel wino_conv1x1_plan describes, plain ones (wino_conv1x1_bn) and chained ones (wino_conv1x1_bn_ex /
 * _ex_hw: padded input, padded output with its ring pass, residual) alike: blocks of 16 row_tiles x 16 col_tiles
 * outputs (row_tiles 1 or 2, col_tiles 1, 2 or 4: wino_conv1x1_small_plan2), 4 waves per workgroup, a block's K
 * loop split over *k_split of them (4, 2 or 1).  *use = 0: the tiled kernel runs. */
int wino_conv1x1_small_plan(long M, int Cin, int Kout, int cus, int* use, int* k_split, int* workgroups);
/* The same with the block shape: a wave holds *row_tiles x *col_tiles MFMA tiles (16 x 16 each; 1 x 1 at M = 196,
 * larger blocks up to 2 x 4 -- fewer operand bytes per FLOP -- from a few images on). */
int wino_conv1x1_small_plan2(long M, int Cin, int Kout, int cus, int* use, int* k_split, int* row_tiles, int* col_tiles,
                             int* workgroups);
/* Host-side only (developer aid): the two launch models' times for this shape, the latency form's best candidate and the
 * tiled kernel's, in microseconds; the latency form is taken while the first beats the second by the policy's margin. */
int wino_debug_conv1x1_models(long M, int Cin, int Kout, int cus, double* t_latency_us, double* t_tiled_us);

/* ---- ResNet bottleneck block of the 14x14 stage (BASELINE.json configs[4]) ---------
 * out = relu( bn3(conv1x1(relu(bn2(conv3x3(relu(bn1(conv1x1(x, w1))), U2))), w3)) + x )
 * x, out [N][14][14][C4] (unpadded, = [N*196][C4]); w1 [C4][Cm], w3 [Cm][C4] (the reference's
 * [Cin][Kout] 1x1 layout); U2 = packed F(2x2,3x3) filters of the Cm->Cm 3x3 layer; all BN folded.
 * Three launches on `s`, intermediates in `workspace` (wino_residual_block_workspace_bytes), which must not overlap x
 * or out (x is read again as the residual by the last launch). */
size_t wino_residual_block_workspace_bytes(int N, int Cm);
int wino_residual_block(const float* x, const float* w1, const float* bn1Bias, const float* bn1Scale,
                        const float* U2, const float* bn2Bias, const float* bn2Scale,
                        const float* w3, const float* bn3Bias, const float* bn3Scale, float* out,
                        int N, int C4, int Cm, void* workspace, size_t workspace_bytes,
                        wino_stream_t s);
/* The block at any feature-map size (ResNet's 56x56 / 28x28 / 7x7 stages):
 * x, out [N][H][W][C4].  H = W = 14 is exactly wino_residual_block. */
size_t wino_residual_block_workspace_bytes_hw(int N, int H, int W, int Cm);
int wino_residual_block_hw(const float* x, const float* w1, const float* bn1Bias, const float* bn1Scale,
                           const float* U2, const float* bn2Bias, const float* bn2Scale,
                           const float* w3, const float* bn3Bias, const float* bn3Scale, float* out,
                           int N, int H, int W, int C4, int Cm, void* workspace, size_t workspace_bytes,
                           wino_stream_t s);

/* Allocates the library-owned scratch the block's three launches on stream `s` will use, ahead of a
 * graph capture (the block's analogue of wino_conv3x3_prepare / wino_conv1x1_prepare). */
int wino_residual_block_prepare(int N, int C4, int Cm, wino_stream_t s);
int wino_residual_block_prepare_hw(int N, int H, int W, int C4, int Cm, wino_stream_t s);

/* ---- ResNet projection (downsampling) bottleneck block: the first block of every stage ----------------
 * ResNet v1 placement: the stride s sits on the first 1x1 and on the projection shortcut, the 3x3 runs at
 * stride 1 on the output grid (the Winograd kernel above).  With H = (Hin-1)/s + 1, W = (Win-1)/s + 1 and
 * xs = x[:, ::s, ::s, :] (never materialised):
 *   out = relu( bn3(conv1x1(relu(bn2(conv3x3(relu(bn1(conv1x1(xs, w1))), U2))), w3)) + bnp(conv1x1(xs, wp)) )
 * x [N][Hin][Win][Cin], out [N][H][W][C4] (unpadded); w1 [Cin][Cm]; U2 = packed F(2x2,3x3) filters Cm -> Cm.
 * The last 1x1 and the projection run as ONE GEMM of K = Cm + Cin (the shortcut never reaches memory) against
 * `tail_packed`: w3 [Cm][C4], wp [Cin][C4] and the two folded BNs packed by wino_proj_tail_pack
 * (wino_proj_tail_elems floats; the layout is private to the library, like U's).
 * Constraints: stride 1 or 2, Cin % 32 == 0, Cm % 64 == 0, C4 % 64 == 0; shapes whose 32-bit tile windows,
 * pixel rows or ring pass would overflow are rejected (WINO_E_SHAPE).  Three launches on `s`; the padded
 * intermediates live in `workspace` (wino_proj_block_workspace_bytes_hw(N, H, W, Cm), H x W the OUTPUT grid), which
 * must not overlap x (read again by the last launch for the shortcut) or out.
 * v1.5 placement (stride on the 3x3, torchvision): wino_proj_block_v15_hw below. */
size_t wino_proj_tail_elems(int Cm, int Cin, int C4);
int wino_proj_tail_pack(const float* w3, const float* bn3Bias, const float* bn3Scale, const float* wp,
                        const float* bnpBias, const float* bnpScale, float* tail_packed, int Cm, int Cin, int C4,
                        wino_stream_t s);
size_t wino_proj_block_workspace_bytes_hw(int N, int H, int W, int Cm);
int wino_proj_block_hw(const float* x, const float* w1, const float* bn1Bias, const float* bn1Scale,
                       const float* U2, const float* bn2Bias, const float* bn2Scale, const float* tail_packed,
                       float* out, int N, int Hin, int Win, int Cin, int Cm, int C4, int stride,
                       void* workspace, size_t workspace_bytes, wino_stream_t s);
/* Allocates the library-owned scratch of the block's three launches on `s`, ahead of a graph capture. */
int wino_proj_block_prepare_hw(int N, int Hin, int Win, int Cin, int Cm, int C4, int stride, wino_stream_t s);
/* Host-side only: the form each of the block's two 1x1 launches takes on a device with `cus` CUs -- the strided
 * first 1x1 (Cin -> Cm) and the fused tail (K = Cm + Cin -> C4): one of WINO_1X1_FORM_*. */
#define WINO_1X1_FORM_TILED 0      /* the tiled kernel, one whole tile per workgroup */
#define WINO_1X1_FORM_STREAM_K 1   /* the tiled kernel in stream-K / split-K form */
#define WINO_1X1_FORM_LATENCY 2    /* the latency kernel (wino_conv1x1_small_plan2) */
int wino_proj_tail_plan(int N, int Hin, int Win, int Cin, int Cm, int C4, int stride, int cus, int* first_form,
                        int* tail_form);

/* ---- stride-2 3x3 convolution + BN (+ReLU): the 3x3 of the v1.5 projection block ----------------------
 * A stride-2, pad-1 3x3 as an implicit GEMM of M = N*H*W, K = 9*C (the 1x1 GEMM kernels reading the input
 * through the nine taps; F(2x2,3x3) has no stride-2 form).  H = (Hin-1)/2 + 1, W = (Win-1)/2 + 1.
 *   in      [N][Hin+2][Win+2][C] with a zero ring (what WINO_C_PADDED layers write)
 *   w_taps  [3][3][C][K]: tap (dy, dx) of input channel c to output channel k -- torch's w.permute(2, 3, 1, 0)
 *   out     [N][H+2][W+2][K], the result at [1..H][1..W] and the ring written as 0 (wino_conv3x3_bn_relu_hw's layout)
 * Constraints: C % 32 == 0, K % 64 == 0.  Shapes whose pixel rows (N*H*W < 2^31), tile windows over `in`, filter
 * matrix or ring pass would overflow 32 bits are rejected (WINO_E_SHAPE).  One launch on `s`; it takes the latency,
 * tiled or stream-K form the 1x1 planner picks for the GEMM (N*H*W, 9*C, K) (WINO_1X1_* knobs apply). */
int wino_conv3x3_s2_bn_relu_hw(const float* in, const float* w_taps, const float* bnBias, const float* bnScale,
                               float* out, int N, int Hin, int Win, int C, int K, int relu, wino_stream_t s);
/* Allocates the layer's stream-K scratch on `s` ahead of a graph capture. */
int wino_conv3x3_s2_prepare_hw(int N, int Hin, int Win, int C, int K, wino_stream_t s);
/* Host-side only: the form the layer takes on a device with `cus` CUs, one of WINO_1X1_FORM_*. */
int wino_conv3x3_s2_plan(int N, int Hin, int Win, int C, int K, int cus, int* form);

/* ---- ResNet v1.5 projection block (torchvision's placement): the stride on the 3x3 ----------------------
 *   out = relu( bn3(conv1x1(relu(bn2(conv3x3_s2(relu(bn1(conv1x1(x, w1))), w2_taps))), w3)) + bnp(conv1x1(xs, wp)) )
 * with xs = x[:, ::2, ::2, :].  x [N][Hin][Win][Cin], out [N][H][W][C4] (H, W as for the stride-2 3x3); w1 [Cin][Cm];
 * w2_taps [3][3][Cm][Cm] (wino_conv3x3_s2_bn_relu_hw); tail_packed from wino_proj_tail_pack, as for the v1 block.
 * Three launches on `s`: the 1x1 at full input resolution, the stride-2 3x3, and the v1 block's fused tail at stride 2.
 * The stride is always 2: at stride 1 the two placements are the same network (wino_proj_block_hw).  Constraints:
 * those of wino_proj_block_hw at stride 2 and of the two layers.  The padded intermediates -- t1 [N][Hin+2][Win+2][Cm],
 * then t2 [N][H+2][W+2][Cm] -- live in `workspace` (wino_proj_block_v15_workspace_bytes_hw), which must not overlap x
 * or out. */
size_t wino_proj_block_v15_workspace_bytes_hw(int N, int Hin, int Win, int Cm);
int wino_proj_block_v15_hw(const float* x, const float* w1, const float* bn1Bias, const float* bn1Scale,
                           const float* w2_taps, const float* bn2Bias, const float* bn2Scale, const float* tail_packed,
                           float* out, int N, int Hin, int Win, int Cin, int Cm, int C4, void* workspace,
                           size_t workspace_bytes, wino_stream_t s);
/* Allocates the library-owned scratch of the block's three launches on `s`, ahead of a graph capture. */
int wino_proj_block_v15_prepare_hw(int N, int Hin, int Win, int Cin, int Cm, int C4, wino_stream_t s);

/* Independent comparator for the 1x1 layers: one thread per output, fp32 FMA loop. */
int wino_conv1x1_direct(const float* A, const float* B, const float* bnBias,
                        const float* bnScale, float* C, long M, int Cin, int Kout, int relu,
                        wino_stream_t s);

/* ---- driver configuration for the argument-less reference entry points ---------
 * kernel_128() & co take no arguments (Kernel128_winograd.h:20); batch size, GPU count
 * and verbosity come from here (defaults N=1, 1 GPU = the reference's behaviour) or
 * from the environment (WINO_BATCH, WINO_GPUS, WINO_QUIET) at first use. */
int wino_driver_set_batch(int N);
int wino_driver_set_gpus(int ngpu);
int wino_driver_set_quiet(int quiet);
int wino_driver_get_batch(void);
int wino_driver_get_gpus(void);
/* Last call's unpacked results (the packed int overflows at 65.5 ms, Test.c:46-47). */
typedef struct {
  double mine_us;        /* custom path, wall clock launch..sync (max over GPUs) */
  double comparator_us;  /* direct-conv comparator, same protocol */
  double max_abs_err;    /* output_checker semantics (util.c:46-63) over all images */
  double max_rel_err;    /* max|diff| / max|comparator| */
  long error_cnt;        /* |diff| > 1e-5, reference threshold */
  double flops;          /* algorithmic FLOPs of the layer call (2*N*P*Q*K*C*R*S) */
  int N, gpus;
  double steady_us;      /* mean of 100 further back-to-back launches (warm), max over GPUs */
} wino_driver_result;
int wino_driver_last_result(wino_driver_result* r);
/* The custom path's output of the last kernel_*() call, on the host: [N][16][16][K] (3x3, ring 0) or
 * [N*196][Kout] (1x1); *elems receives the element count.  Valid until the next kernel_*() call.
 * NULL before the first call.  (The reference keeps this in a local array, Kernel128_winograd.cu:257.) */
const float* wino_driver_last_output(size_t* elems);
/* The packed return value of the kernel_*() entry points, (mine << 16) | comparator
 * (Kernel128_winograd.cu:433), with the custom half clamped to 0x7FFF and the comparator half to
 * 0xFFFF so that the reference's signed decode `res >> 16`, `res & 0xFFFF` (Test.c:46-47) never
 * sees a negative number. */
int wino_driver_pack_times(uint64_t mine_us, uint64_t comparator_us);
/* Developer knob (WINO_GPUS_ALIAS=1): job g of a multi-GPU call runs on device g % visible, so the
 * threaded batch-split path (one host thread + one stream per job, common start barrier) can be
 * exercised on a box with fewer GPUs than requested. */
int wino_driver_set_gpu_alias(int on);
/* WINO_STDOUT_COMPAT=1: the per-call lines carry the reference's exact labels -- "cuDNN TotalTime =
 * %d us" and cuda-prefixed status names (Kernel128_winograd.cu:270-275,404-409) -- for scrapers written
 * against the reference; ./Test then also prints "[cuDNN: %d us]" (Test.c:50-53) and nothing extra.
 * The comparator behind that label is this library's direct-convolution kernel, not cuDNN. */
int wino_driver_set_stdout_compat(int on);
int wino_driver_get_stdout_compat(void);
/* CPU baseline of the layer the LAST kernel_*() call ran (same inputs, same N): naive im2col +
 * three-loop SGEMM + folded BN (+ReLU) on all host cores, timed with the wall clock (one warm-up,
 * then repetitions for about half a second), and diffed against that call's GPU output.
 * A reported baseline, never a fallback: nothing the library returns comes from it. */
typedef struct {
  double us;             /* mean wall time of one CPU pass over the layer */
  double gflops;         /* algorithmic FLOPs / us */
  int threads;           /* host threads used = cores this process may run on */
  int reps;
  double max_abs_diff;   /* max |GPU - CPU| over the valid outputs */
  double max_rel_diff;   /* ... / max |CPU| */
} wino_cpu_baseline_result;
int wino_driver_cpu_baseline(wino_cpu_baseline_result* r);

/* ---- ResNet basic block (ResNet-18 / -34) -----------------------------------------------------
 * out = act(bnScale*conv3x3(in, U) + bnBias + residual): the second 3x3 of a ResNet basic block.
 * in [N][H+2][W+2][C]; residual, out [N][H+2][W+2][K] (result at [1..H][1..W], out's ring written 0,
 * residual's ring not read).  Constraints of wino_conv3x3_bn_relu_hw.  out may BE residual (in place);
 * any other overlap among in, residual and out is WINO_E_ARG.
 * In place is safe: each residual element is read only by the lane that stores the output at the same offset,
 * just before that store, and the ring pass writes zeros onto a ring that is not read.  The launch takes exactly the
 * plan of wino_conv3x3_bn_relu_hw at the same shape (wino_conv3x3_plan / wino_conv3x3_small_plan2 describe it, and
 * wino_conv3x3_prepare_hw prepares it); the ReLU (relu != 0) is applied after the add. */
int wino_conv3x3_bn_add_relu_hw(const float* in, const float* U, const float* bnBias, const float* bnScale,
                                const float* residual, float* out, int N, int H, int W, int C, int K,
                                int relu, wino_stream_t s);

/* Identity basic block: out = relu(bn2(conv3x3(relu(bn1(conv3x3(x, U1))), U2)) + x).
 * x, out [N][H+2][W+2][C] with a zero ring (out's ring written 0: out is the next block's x); U1, U2 from
 * wino_filter_transform_f2 (C -> C).  Two launches; t1 [N][H+2][W+2][C] lives in workspace.
 * out may be x (in place: a chain of blocks then needs one activation tensor and one workspace); workspace must
 * not overlap x or out; any other overlap of x and out is WINO_E_ARG.  Constraints of wino_conv3x3_bn_relu_hw with
 * K = C (C % 64 == 0).  wino_basic_block_prepare_hw reserves the stream's scratch for both launches (before a
 * graph capture). */
size_t wino_basic_block_workspace_bytes_hw(int N, int H, int W, int C);
int wino_basic_block_hw(const float* x, const float* U1, const float* bn1Bias, const float* bn1Scale,
                        const float* U2, const float* bn2Bias, const float* bn2Scale, float* out,
                        int N, int H, int W, int C, void* workspace, size_t workspace_bytes, wino_stream_t s);
int wino_basic_block_prepare_hw(int N, int H, int W, int C, wino_stream_t s);

/* Downsampling basic block (the first block of ResNet-18 / -34's conv3, conv4, conv5; torchvision's BasicBlock with
 * `downsample`), H = (Hin-1)/2 + 1, W = (Win-1)/2 + 1:
 *   t1  = relu(bn1(conv3x3_s2(x, w_taps)))      C -> K, stride 2, pad 1
 *   sc  = bnd(conv1x1_s2(x, wd))                C -> K, stride 2, no padding, no ReLU
 *   out = relu(bn2(conv3x3(t1, U2)) + sc)       K -> K
 * The shortcut reads the pixel the stride-2 3x3's centre tap reads, so it runs inside the stride-2 3x3's launch as
 * extra workgroups over that tap's k-range.  `packed` holds w_taps [3][3][C][K] (wino_conv3x3_s2_bn_relu_hw's
 * format), wd [C][K] and the four BN vectors (bias, scale: not folded into the filters), as wino_s2_proj_pack writes
 * it (wino_s2_proj_elems floats; the layout is private to the library).
 * wino_conv3x3_s2_proj_bn_relu_hw is the fused layer on its own, one launch: in [N][Hin+2][Win+2][C] with a zero
 * ring; t1 [N][H+2][W+2][K] exactly as wino_conv3x3_s2_bn_relu_hw(relu = 1) writes it (bitwise; ring written 0);
 * sc [N][H+2][W+2][K], the interior written, the ring not touched.  It takes the stride-2 layer's plan unchanged
 * (wino_conv3x3_s2_plan describes it, wino_conv3x3_s2_prepare_hw prepares it).
 * wino_basic_block_s2_hw is the block, two launches: the fused layer writes t1 into `workspace`
 * (wino_basic_block_s2_workspace_bytes_hw(N, Hin, Win, K) bytes) and sc into out's interior, then
 * wino_conv3x3_bn_add_relu_hw(t1, U2, bn2, residual = out, out = out) runs in place.  x [N][Hin+2][Win+2][C] with a
 * zero ring (what wino_basic_block_hw takes and writes); out [N][H+2][W+2][K] with its ring written 0: the next
 * identity block's x as it stands.  U2 from wino_filter_transform_f2 (K -> K).  Constraints: C % 32 == 0,
 * K % 64 == 0, those of the stride-2 layer and of the K -> K 3x3 on the H x W grid; x, out, workspace and packed must
 * not overlap (WINO_E_ARG).  wino_basic_block_s2_prepare_hw reserves the stream's scratch of both launches (before a
 * graph capture). */
size_t wino_s2_proj_elems(int C, int K);
int wino_s2_proj_pack(const float* w_taps, const float* bn1Bias, const float* bn1Scale, const float* wd,
                      const float* bndBias, const float* bndScale, float* packed, int C, int K, wino_stream_t s);
int wino_conv3x3_s2_proj_bn_relu_hw(const float* in, const float* packed, float* t1, float* sc, int N, int Hin,
                                    int Win, int C, int K, wino_stream_t s);
size_t wino_basic_block_s2_workspace_bytes_hw(int N, int Hin, int Win, int K);
int wino_basic_block_s2_hw(const float* x, const float* packed, const float* U2, const float* bn2Bias,
                           const float* bn2Scale, float* out, int N, int Hin, int Win, int C, int K,
                           void* workspace, size_t workspace_bytes, wino_stream_t s);
int wino_basic_block_s2_prepare_hw(int N, int Hin, int Win, int C, int K, wino_stream_t s);

/* ---- ResNet stem: conv 7x7 stride 2 pad 3 (3 -> K) + BN + ReLU + max-pool 3x3 stride 2 pad 1, one launch ----------
 *   x    [N][3][H][W], NCHW as images come from torch; any H, W >= 1 (rows need no alignment, the base pointer does)
 *   out  [N][Hp][Wp][K] (out_padded = 0: what wino_proj_block_hw / wino_residual_block_hw take) or
 *        [N][Hp+2][Wp+2][K] with its ring written 0 (out_padded = 1: what wino_basic_block_hw takes),
 *        Hc = (H-1)/2 + 1, Hp = (Hc-1)/2 + 1, the same for W (224 -> 112 -> 56)
 * `packed` holds torch's w [K][3][7][7] and the BN vectors (bias, scale; not folded into the filter, the scale may be
 * negative: BN and ReLU come before the max) as wino_stem_filter_pack writes them (wino_stem_filter_elems(K) floats;
 * the layout is private to the library).  Constraints: K % 64 == 0; one image's input and output each below 2^31
 * elements (any batch: every image is addressed from its own 64-bit base).  x, packed and out must not overlap.
 * The contraction runs on the f32 MFMA (exact f32); the conv output never reaches memory.  No stream scratch.
 * wino_stem_plan (host-side only): the form this shape takes on a device with `cus` CUs -- WINO_STEM_FORM_BIG
 * (8x8 pooled outputs x 64 channels per workgroup) or WINO_STEM_FORM_SMALL (4x4 x 16, small batches); the
 * WINO_STEM_FORM developer knob (1 / 2) forces one. */
#define WINO_STEM_FORM_BIG 1
#define WINO_STEM_FORM_SMALL 2
size_t wino_stem_filter_elems(int K);
int wino_stem_filter_pack(const float* w, const float* bnBias, const float* bnScale, float* packed, int K,
                          wino_stream_t s);
int wino_stem_hw(const float* x, const float* packed, float* out, int N, int H, int W, int K, int out_padded,
                 wino_stream_t s);
int wino_stem_plan(int N, int H, int W, int K, int cus, int* form);

/* ---- ResNet classifier head: global average pool + fully connected layer ------------------------------------
 *   logits [N][classes] = mean_hw(feat) . Wfc^T + b
 * feat [N][H][W][C], or [N][H+2][W+2][C] with in_padded = 1 (the ring is not read).  `packed` holds torch's
 * Wfc [classes][C] and b [classes] as wino_head_pack writes them (wino_head_elems floats; the class count is
 * padded to a multiple of 64 inside).  An average-pool launch writes the pooled [N][C] into `workspace`
 * (wino_head_workspace_bytes), the 1x1 GEMM (wino_conv1x1_bn with BN scale 1 and the FC bias as BN bias)
 * multiplies it, and a trim launch copies the first `classes` columns to out (when classes % 64 != 0).
 * Constraints: C % 32 == 0, classes >= 1.  feat, packed, out and workspace must not overlap.  The GEMM may take
 * its stream-K form: wino_head_prepare reserves the stream's scratch ahead of a graph capture. */
size_t wino_head_elems(int C, int classes);
int wino_head_pack(const float* wfc, const float* bfc, float* packed, int C, int classes, wino_stream_t s);
size_t wino_head_workspace_bytes(int N, int C, int classes);
int wino_head_prepare(int N, int C, int classes, wino_stream_t s);
int wino_avgpool_fc_hw(const float* feat, const float* packed, float* out, int N, int H, int W, int C, int classes,
                       int in_padded, void* workspace, size_t workspace_bytes, wino_stream_t s);

/* ---- VGG: the pooled 3x3 layer and the two memory-bound kernels around the convolutions --------------------------
 * wino_conv3x3_bn_relu_pool_hw, one launch:  out = maxpool2x2_s2(act(bnScale*conv3x3(in, U) + bnBias))
 *   in   [N][H+2][W+2][C] with a zero ring, U from wino_filter_transform_f2: as for wino_conv3x3_bn_relu_hw
 *   out  [N][H/2+2][W/2+2][K], the pooled map at [1..H/2][1..W/2], its ring written 0 (what the next 3x3 layer reads)
 * H/2 and W/2 floor (torch's MaxPool2d(2, 2)): for odd H or W the clipped last tile row / column is dropped.  An
 * F(2x2) tile is one pooling window, so the max is taken in the epilogue, in the lane that holds the tile, after the
 * stream-K gather, BN and the ReLU; the un-pooled activation never reaches memory.  The launch takes exactly the plan
 * of the plain layer of the same (N, H, W, C, K): wino_conv3x3_plan / _small_plan2 describe it, wino_conv3x3_prepare_hw
 * reserves its scratch.  Constraints: those of wino_conv3x3_bn_relu_hw, and H, W >= 2; in and out must not overlap
 * (WINO_E_ARG).  Any batch (tensors of 4 GiB and more go out as several launches of whole images).
 *
 * wino_image_pack_hw, one launch:  x [N][Cin][H][W] (NCHW, as images come from torch) ->
 *   out [N][H+2][W+2][Cpad] with channels Cin .. Cpad-1 and the ring written 0 -- the first 3x3 layer's input; its
 *   filter is zero-padded to [K][Cpad][3][3] before wino_filter_transform_f2.  1 <= Cin <= Cpad, Cpad % 8 == 0,
 *   H, W >= 1; one image's input and output each below 2^31 elements.  x and out must not overlap.
 *
 * wino_avgpool7_flatten_hw, one launch:  torch's AdaptiveAvgPool2d((7, 7)) and flatten
 *   feat [N][H][W][C], or [N][H+2][W+2][C] with in_padded = 1 (the ring is not read)
 *   out  [N][49*C] in (h, w, c) order: bin (i, j) is the mean over rows floor(i*H/7) .. ceil((i+1)*H/7) - 1 and the
 *        same for columns (a 1x1 map is replicated 49 times).  The first FC's weight columns are permuted from torch's
 *        (c, h, w) to this order once, at pack time.
 *   H, W >= 1 with H * W < 2^24, C % 4 == 0; one image's input and output each below 2^31 elements (any batch: every
 *   image is addressed from its own 64-bit base).  feat and out must not overlap. */
int wino_conv3x3_bn_relu_pool_hw(const float* in, const float* U, const float* bnBias, const float* bnScale,
                                 float* out, int N, int H, int W, int C, int K, int relu, wino_stream_t s);
int wino_image_pack_hw(const float* x, float* out, int N, int Cin, int H, int W, int Cpad, wino_stream_t s);
int wino_avgpool7_flatten_hw(const float* feat, float* out, int N, int H, int W, int C, int in_padded,
                             wino_stream_t s);

/* ---- grouped 3x3 convolution + BN (+ReLU) and the ResNeXt bottleneck blocks ---------------------------------------
 *   out = act(bnScale[k] * conv3x3_grouped(in, w) + bnBias[k]),  stride 1 or 2, pad 1, C -> C channels in `groups`
 *   groups of Cg = C / groups: output channel k reads input channels (k / Cg) * Cg .. + Cg - 1
 *   in      [N][Hin+2][Win+2][C] with a zero ring (what WINO_C_PADDED layers write)
 *   packed  from wino_conv3x3_grouped_filter_pack (wino_conv3x3_grouped_filter_elems(C, groups) floats, 0 for an
 *           illegal shape; the layout is private to the library), of torch's w [C][Cg][3][3]
 *   out     [N][H+2][W+2][C], the result at [1..H][1..W], the ring written 0; H = (Hin-1)/stride + 1, the same for W
 * Constraints: C % 64 == 0 and Cg in {4, 8, 16, 32, 64} -- every 3x3 of resnext50_32x4d, resnext101_32x8d and
 * resnext101_64x4d -- so that a 64-channel output block reads exactly its own 64 input channels; anything else (a
 * `groups` that does not divide C, Cg = 2, groups = 1 at C > 64) is WINO_E_SHAPE; a stride other than 1 or 2 is
 * WINO_E_ARG.  Any N: every image is addressed from its own 64-bit base, and one padded input image must stay below
 * 2^31 elements (WINO_E_SHAPE).  in and out must not overlap (WINO_E_ARG).  One launch, an implicit GEMM on the f32 MFMA
 * (exact f32; there is no bf16 path); no stream scratch, so there is no prepare.  BN stays in its two vectors.
 * wino_conv3x3_grouped_plan (host only) answers the launch the layer takes, a function of the shape alone, from the
 * geometry the launcher itself reads: the kernel is one body compiled for stride x tile width x contraction width, with
 *   tile_w   8 or 16 output columns per workgroup tile, whichever pads the output row by less
 *   kc       16, 32 or 64 input channels per 16-channel column tile: max(Cg, 16)
 *   tiles_y, tiles_x   the tiles of one image; a tile is (stride 1: 4, stride 2: 2) * 16 / tile_w rows high
 * and returns what the layer would for the shape (WINO_E_SHAPE / WINO_E_ARG, WINO_E_ARG for a NULL pointer).
 *
 * wino_grouped_residual_block_hw: wino_residual_block_hw with this layer in the middle (wg from
 * wino_conv3x3_grouped_filter_pack(Cm, groups)); x, out [N][H][W][C4].
 * wino_grouped_proj_block_hw: the projection bottleneck in torchvision's placement -- the first 1x1 at the full
 * Hin x Win, this layer at `stride` (1 or 2), then the fused tail of wino_proj_block_hw (tail_packed from
 * wino_proj_tail_pack); x [N][Hin][Win][Cin], out [N][H][W][C4].
 * Every argument, shape and overlap is checked before the first launch.  The blocks' intermediates are exactly their
 * dense counterparts', so their workspaces are sized by the dense blocks' queries:
 *   wino_grouped_residual_block_hw          wino_residual_block_workspace_bytes_hw(N, H, W, Cm)
 *   wino_grouped_proj_block_hw, stride 1    wino_proj_block_workspace_bytes_hw(N, H, W, Cm)
 *   wino_grouped_proj_block_hw, stride 2    wino_proj_block_v15_workspace_bytes_hw(N, Hin, Win, Cm)
 * A smaller workspace, or one that overlaps x or out, is WINO_E_ARG.  The *_prepare_hw entry points reserve the stream-K
 * scratch of the blocks' two 1x1 launches ahead of a graph capture. */
size_t wino_conv3x3_grouped_filter_elems(int C, int groups);
int wino_conv3x3_grouped_filter_pack(const float* w, float* packed, int C, int groups, wino_stream_t s);
int wino_conv3x3_grouped_bn_relu_hw(const float* in, const float* packed, const float* bnBias, const float* bnScale,
                                    float* out, int N, int Hin, int Win, int C, int groups, int stride, int relu,
                                    wino_stream_t s);
int wino_conv3x3_grouped_plan(int N, int Hin, int Win, int C, int groups, int stride, int* tile_w, int* kc,
                              int* tiles_y, int* tiles_x);
int wino_grouped_residual_block_hw(const float* x, const float* w1, const float* bn1Bias, const float* bn1Scale,
                                   const float* wg, const float* bn2Bias, const float* bn2Scale, const float* w3,
                                   const float* bn3Bias, const float* bn3Scale, float* out, int N, int H, int W, int C4,
                                   int Cm, int groups, void* workspace, size_t workspace_bytes, wino_stream_t s);
int wino_grouped_residual_block_prepare_hw(int N, int H, int W, int C4, int Cm, int groups, wino_stream_t s);
int wino_grouped_proj_block_hw(const float* x, const float* w1, const float* bn1Bias, const float* bn1Scale,
                               const float* wg, const float* bn2Bias, const float* bn2Scale, const float* tail_packed,
                               float* out, int N, int Hin, int Win, int Cin, int Cm, int C4, int groups, int stride,
                               void* workspace, size_t workspace_bytes, wino_stream_t s);
int wino_grouped_proj_block_prepare_hw(int N, int Hin, int Win, int Cin, int Cm, int C4, int groups, int stride,
                                       wino_stream_t s);

/* ---- Feature Pyramid Network (torchvision's FeaturePyramidNetwork on a ResNet's four stage outputs) ----------------
 * One pyramid level, two launches on `s`:
 *   inner = conv1x1(c, wl) + lBias [+ nearest_upsample(top)]     Cin -> Cf, no ReLU   (the lateral and the top-down sum)
 *   P     = conv3x3(inner, U) + oBias                            Cf -> Cf, no ReLU   (Winograd: wino_conv3x3_bn_relu_hw)
 *   c      the stage output, [N][H][W][Cin] or, c_padded != 0, [N][H+2][W+2][Cin] (ResNet-18 / -34's layout)
 *   wl     [Cin][Cf]; U from wino_filter_transform_f2 (Cf -> Cf)
 *   lBias, oBias   the convolutions' biases; lScale, oScale: the layers' bnScale vectors, which an FPN fills with ones
 *   top    the coarser level's `inner`, padded [N][Hc+2][Wc+2][Cf] with Hc = (H+1)/2, Wc = (W+1)/2 (its ring is not
 *          read), added through WINO_RESIDUAL_UP2; NULL on the coarsest level
 *   inner, P   padded [N][H+2][W+2][Cf], their rings written 0
 * Every argument is checked before the first launch: Cin % 32 == 0, Cf % 64 == 0, the constraints of
 * wino_conv1x1_bn_ex_hw and wino_conv3x3_bn_relu_hw (C * K < 2^26 among them); c, top, inner and P must not overlap
 * (WINO_E_ARG).  wino_fpn_level_prepare_hw reserves the stream scratch of both launches (before a graph capture). */
int wino_fpn_level_hw(const float* c, const float* wl, const float* lBias, const float* lScale, const float* top,
                      float* inner, const float* U, const float* oBias, const float* oScale, float* P, int N, int H,
                      int W, int Cin, int Cf, int c_padded, wino_stream_t s);
int wino_fpn_level_prepare_hw(int N, int H, int W, int Cin, int Cf, wino_stream_t s);

/* ---- dilated 3x3 and the dilated bottleneck blocks (the segmentation backbones: torchvision's fcn_resnet* and
 * deeplabv3_resnet* build layer3 / layer4 with replace_stride_with_dilation) ------------------------------------------
 *   out = act(bnScale[k] * conv3x3(in, w, stride 1, padding d, dilation d) + bnBias[k])
 *   in      [N][H+2][W+2][C] with a zero ring of width ONE -- the library's padded layout, what WINO_C_PADDED layers
 *           write -- whatever the dilation: a tap outside the image is a zero, not a read d pixels out
 *   w_taps  [3][3][C][K], the stride-2 layer's format (wino_conv3x3_s2_bn_relu_hw)
 *   out     [N][H+2][W+2][K]: the result in the interior, the ring written 0
 * C % 32 == 0, K % 64 == 0, dilation >= 1 (one that exceeds the map is legal: only the centre tap then sees data);
 * N*H*W < 2^31, H, W <= 4094, one padded image < 2^31 pixels, and a row tile's window with the taps' reach of
 * dilation * (W+2) + dilation pixels to either side, the filter matrix and the ring pass below 2^32 (WINO_E_SHAPE);
 * in and out must not overlap (WINO_E_ARG).  The layer is the GEMM (N*H*W, 9C, K) on the tiled 1x1 kernel (operand
 * form A_DIL), whole tiles or stream-K; it has no latency form.  wino_conv3x3_dilated_plan (host only) answers
 * WINO_1X1_FORM_TILED or WINO_1X1_FORM_STREAM_K. */
int wino_conv3x3_dilated_bn_relu_hw(const float* in, const float* w_taps, const float* bnBias, const float* bnScale,
                                    float* out, int N, int H, int W, int C, int K, int dilation, int relu,
                                    wino_stream_t s);
int wino_conv3x3_dilated_prepare_hw(int N, int H, int W, int C, int K, int dilation, wino_stream_t s);
int wino_conv3x3_dilated_plan(int N, int H, int W, int C, int K, int dilation, int cus, int* form);
/* The bottleneck blocks with the dilated 3x3 in the middle, stride 1, input and output on one H x W grid:
 *   wino_dilated_residual_block_hw   out = relu(bn3(conv1x1(relu(bn2(conv3x3_dil(relu(bn1(conv1x1(x, w1))), w2_taps))), w3)) + x)
 *   wino_dilated_proj_block_hw       the same with the projection shortcut, in the fused tail (wino_proj_tail_pack, stride 1)
 * x [N][H][W][C4 or Cin], out [N][H][W][C4]; w2_taps [3][3][Cm][Cm].  Their intermediates are the dense blocks':
 * workspaces of wino_residual_block_workspace_bytes_hw(N, H, W, Cm) and wino_proj_block_workspace_bytes_hw(N, H, W, Cm)
 * bytes.  Checks, their order and *_prepare_hw as for the other bottleneck blocks. */
int wino_dilated_residual_block_hw(const float* x, const float* w1, const float* bn1Bias, const float* bn1Scale,
                                   const float* w2_taps, const float* bn2Bias, const float* bn2Scale, const float* w3,
                                   const float* bn3Bias, const float* bn3Scale, float* out, int N, int H, int W, int C4,
                                   int Cm, int dilation, void* workspace, size_t workspace_bytes, wino_stream_t s);
int wino_dilated_residual_block_prepare_hw(int N, int H, int W, int C4, int Cm, int dilation, wino_stream_t s);
int wino_dilated_proj_block_hw(const float* x, const float* w1, const float* bn1Bias, const float* bn1Scale,
                               const float* w2_taps, const float* bn2Bias, const float* bn2Scale,
                               const float* tail_packed, float* out, int N, int H, int W, int Cin, int Cm, int C4,
                               int dilation, void* workspace, size_t workspace_bytes, wino_stream_t s);
int wino_dilated_proj_block_prepare_hw(int N, int H, int W, int Cin, int Cm, int C4, int dilation, wino_stream_t s);

/* ---- the concat projection and the ASPP module (torchvision's deeplabv3_resnet* head) --------------------------------
 * The 1x1 layer behind a channel concatenation that is never made:
 *   out[m][k] = act(bnScale[k] * sum_{j < sources} sum_{c < Cs} src_j[row(m)][c] * w[j*Cs + c][k] + bias_per_image[n(m)][k])
 *   src             source j is the [N][H][W][Cs] tensor at src + j * src_stride floats ([N][H+2][W+2][Cs] with
 *                   WINO_A_PADDED; its ring is never read).  src_stride % 4 == 0 and at least a source's size; what lies
 *                   between two sources is never read
 *   w               [sources * Cs][Kout], the matrix the concatenated tensor would meet
 *   bias_per_image  [N][Kout], 16-byte aligned: output row m adds the row of its image n(m) = m / (H*W) -- the place of
 *                   a branch that is constant over an image (ASPP's pooled one), folded by the caller
 *   out             [N*H*W][Kout], or [N][H+2][W+2][Kout] with its ring written 0 (WINO_C_PADDED)
 * flags: a subset of WINO_RELU | WINO_A_PADDED | WINO_C_PADDED (anything else: WINO_E_ARG).  2 <= sources <= 8,
 * Cs % 32 == 0, Kout % 64 == 0 and the limits of wino_conv1x1_bn_ex_hw at Cin = sources * Cs (H, W <= 4094 with or
 * without padded operands).  One buffer descriptor per 112-row tile spans all sources:
 *   (rows * Cs + (sources - 1) * src_stride) * 4 bytes < 2^32, rows = 112, or 111 * (2 (W+2) + 3) + 1 with WINO_A_PADDED
 * (WINO_E_SHAPE otherwise, like every other shape refusal here).  The sources, bias_per_image and out must not overlap
 * (WINO_E_ARG).  One launch of the tiled 1x1 kernel (operand form A_CAT), whole tiles or stream-K; there is no latency
 * form.  wino_conv1x1_cat_plan (host only) answers WINO_1X1_FORM_TILED or WINO_1X1_FORM_STREAM_K: the plan of the GEMM
 * (N*H*W, sources * Cs, Kout), as wino_conv1x1_plan reports it. */
int wino_conv1x1_cat_bn_hw(const float* src, long src_stride, const float* w, const float* bias_per_image,
                           const float* bnScale, float* out, int N, int H, int W, int sources, int Cs, int Kout,
                           int flags, wino_stream_t s);
int wino_conv1x1_cat_prepare_hw(int N, int H, int W, int sources, int Cs, int Kout, wino_stream_t s);
int wino_conv1x1_cat_plan(int N, int H, int W, int sources, int Cs, int Kout, int cus, int* form);
/* Atrous spatial pyramid pooling:
 *   out = relu(bn(conv1x1(cat(b0, b1, b2, b3, broadcast(bp)), w_proj)))
 *   b0 = relu(bn0(conv1x1(in, w0)));  b_i = relu(bn_i(conv3x3(in, w_i, dilation d_i)));  bp = relu(bnp(conv1x1(mean_hw(in), w_pool)))
 *   in       [N][H+2][W+2][Cin], zero ring;  out [N][H+2][W+2][Kout], ring written 0
 *   w0, w_pool  [Cin][Cb];  w1_taps .. w3_taps  [3][3][Cin][Cb] (the stride-2 layer's format)
 *   w_proj   [5 * Cb][Kout]: the rows of b0 .. b3, then the pooled branch's Cb rows
 * Eight launches on `s`: the average pool, two 1x1 layers of N rows that fold the pooled branch into a per-image bias
 * bnScale * (bp . w_proj[4 Cb ..]) + bnBias, the four spatial branches into unpadded slots of the workspace, and
 * wino_conv1x1_cat_bn_hw over the slots with that bias.  Cin % 32 == 0, Cb % 64 == 0, Kout % 64 == 0, every d_i >= 1,
 * H*W < 2^24, and each layer's own limits, all checked before the first launch (WINO_E_SHAPE).  The workspace, 16-byte
 * aligned, holds at least
 *   r256(4 N Cin) + r256(4 N Cb) + r256(4 N Kout) + 4 * (4 N H W Cb)   bytes (r256: rounded up to a multiple of 256)
 * -- the pooled vector, its branch, the per-image bias and the four slots; the Python wrapper's aspp_workspace_bytes
 * is this formula.  A smaller one, or an overlap among in, out and the workspace, is WINO_E_ARG.  wino_aspp_prepare_hw reserves the stream
 * scratch of every launch (before a graph capture). */
int wino_aspp_hw(const float* in, const float* w0, const float* bn0Bias, const float* bn0Scale, const float* w1_taps,
                 const float* bn1Bias, const float* bn1Scale, const float* w2_taps, const float* bn2Bias,
                 const float* bn2Scale, const float* w3_taps, const float* bn3Bias, const float* bn3Scale,
                 const float* w_pool, const float* bnpBias, const float* bnpScale, const float* w_proj,
                 const float* bnBias, const float* bnScale, float* out, int N, int H, int W, int Cin, int Cb, int Kout,
                 int d1, int d2, int d3, void* workspace, size_t workspace_bytes, wino_stream_t s);
int wino_aspp_prepare_hw(int N, int H, int W, int Cin, int Cb, int Kout, int d1, int d2, int d3, wino_stream_t s);

/* ---- bilinear resize and label map: the output stage of a segmentation network -----------------
 * torch's F.interpolate(mode="bilinear", align_corners=False) of the class scores, and / or the argmax over the classes
 * of the resized scores, in one launch:
 *   src     [N][h][w][ld], or with in_padded = 1 the padded [N][h+2][w+2][ld] (the ring is never read); the first C of
 *           the ld columns are the classes
 *   out     [N][C][Ho][Wo] fp32, NCHW (torch's layout), or NULL
 *   labels  [N][Ho][Wo] int32: the index of the largest of the C resized values of a pixel; a tie goes to the lowest
 *           index, a NaN counts as larger than every number and the first NaN wins (torch.argmax); or NULL
 * Source coordinates are exact integers: per axis, num = max((2 d + 1) in - out, 0), i0 = num / (2 out), i1 =
 * min(i0 + 1, in - 1), lambda = float(num - i0 * 2 out) / float(2 out); value = (1-ly)((1-lx) a + lx b) + ly((1-lx) c +
 * lx d) in fp32, all four taps always multiplied (a NaN or Inf under a zero weight still reaches the output, also when
 * Ho == h and Wo == w, where torch copies instead).  With both outputs the labels are taken from the stored values.
 * No workspace and no stream scratch: the call can be captured into a graph as it is.
 * N, h, w, Ho, Wo >= 1, 1 <= C <= ld, ld % 4 == 0, in_padded 0 or 1, one image of src, out and labels below 2^31
 * elements, 2 Ho h and 2 Wo w below 2^31 (WINO_E_SHAPE otherwise); src NULL, out and labels both NULL, a pointer that
 * is not 16-byte aligned, or any overlap among src, out and labels is WINO_E_ARG.  Any N.
 * wino_resize_bilinear_plan (host only) answers the form the launch takes, a function of the shape alone: STAGED (a
 * workgroup stages the source rows of a block of output rows x an x-segment in LDS and writes class planes with 16-byte
 * stores) or DIRECT (every lane gathers its taps from global memory: when no block of one output row x 64 pixels fits
 * in 64 KB of LDS, or an axis shrinks by more than 4x). */
#define WINO_RESIZE_FORM_STAGED 1
#define WINO_RESIZE_FORM_DIRECT 2
int wino_resize_bilinear_hw(const float* src, float* out, int* labels, int N, int h, int w, int C, int ld,
                            int in_padded, int Ho, int Wo, wino_stream_t s);
int wino_resize_bilinear_plan(int h, int w, int C, int ld, int Ho, int Wo, int want_out, int want_labels, int* form);

/* ---- multi-scale RoIAlign: the pooling stage of a two-stage detector ----------------------------
 * torchvision's roi_align(..., aligned=False) over 1 to 4 pyramid levels with MultiScaleRoIAlign's level assignment, all
 * boxes of all images and levels in one launch:
 *   f0..f3      the level maps, finest first, [N][h_l][w_l][C], or with in_padded = 1 the padded [N][h_l+2][w_l+2][C] that
 *               wino_fpn_level_hw writes (the ring is never read: RoIAlign clamps to the border pixel); pointers beyond
 *               `levels` are ignored
 *   hw_host     HOST array [levels][2] of (h_l, w_l);  scale_host: HOST array [levels] of spatial_scale.  With levels > 1,
 *               scale_host[l] must be exactly 2^-(k0+l) for an integer k0 (torchvision's LevelMapper assumes it); one
 *               level takes any finite positive scale
 *   rois        DEVICE [R][5] fp32 (batch index, x1, y1, x2, y2) in image pixels, torchvision's Tensor[K, 5]
 *   out         [R][P][P][C], or with out_padded = 1 [R][P+2][P+2][C] with the ring written as exact 0: the layout
 *               wino_conv3x3_bn_relu_hw reads at N = R.  The unpadded form at P = 7 is the A matrix [R][49 C] of a
 *               detector's first FC layer
 * Arithmetic (fp32, torchvision's CPU kernel operation by operation): s = the level's scale; sx = x1 s, ... ; roi_w =
 * max(ex - sx, 1); bin = roi / P; sampling x sampling samples per bin at start + p bin + (i + .5) bin / sampling.  A
 * sample with y < -1 || y > h || x < -1 || x > w contributes 0; otherwise clamp at 0, low = (int)v, at low >= size - 1
 * both taps are size - 1 and the fraction 0; value = hy hx a + hy lx b + ly hx c + ly lx d with all four taps always
 * multiplied (a NaN under a zero weight reaches the output); the bin is the sum of its samples / sampling^2.
 * Level (levels > 1): clamp(floor(canonical_level + log2(sqrt(area) / canonical_scale) + 1e-6), k0, k0 + levels - 1) - k0
 * with area = (x2 - x1)(y2 - y1) in fp32, evaluated as the number of area thresholds (canonical_scale 2^(k0 + j -
 * canonical_level - 1e-6))^2 the area reaches (computed on the host in double, compared as floats: it can differ from
 * torch's fp32 log2 only within about 1e-6 relative of a threshold); an area <= 0 or NaN takes level 0 (undefined in torch).
 * A box whose batch index is not an integer in [0, N) reads nothing and gets zeros; otherwise a box with a non-finite
 * coordinate reads nothing and gets NaN in its P x P x C outputs (ring 0).  Every tap address is clamped into the box's
 * own image, and no box changes a bit of another box's output.
 * 1 <= levels <= 4, N, C >= 1, C % 4 == 0, 1 <= P <= 64, 1 <= sampling <= 4 (torchvision's adaptive sampling_ratio <= 0
 * is not supported), R >= 0, in_padded and out_padded 0 or 1, h_l, w_l >= 1, one image of a level map and one box's
 * output below 2^31 elements (WINO_E_SHAPE otherwise); any R (the output may pass 4 GiB).  R == 0 is WINO_OK and launches
 * nothing.  A NULL or not 16-byte-aligned pointer, an overlap of out with a level map or with rois, a bad scale_host
 * sequence, or a canonical_scale that is not finite and positive is WINO_E_ARG.  No workspace and no stream scratch: the
 * call can be captured into a graph as it is.
 * A call whose R (P + 2 out_padded)^2 output positions pass 2^31 runs as several launches of whole boxes, each from its
 * own rois and out base.  wino_roi_align_launches (host only) answers how many launches R boxes take; the developer knob
 * WINO_ROI_LAUNCH_TASKS = t > 0 lowers the 2^31 to t (one box per launch at the least), a value <= 0 is ignored. */
int wino_roi_align_hw(const float* f0, const float* f1, const float* f2, const float* f3, const int* hw_host,
                      const float* scale_host, int levels, int N, int C, int in_padded, const float* rois, int R, int P,
                      int sampling, float canonical_scale, int canonical_level, float* out, int out_padded,
                      wino_stream_t s);
int wino_roi_align_launches(int R, int P, int out_padded, long* launches);

/* ---- box decoding and batched non-maximum suppression (boxes.hip) --------------------------------
 * wino_box_decode_hw: torchvision's BoxCoder.decode_single followed by clip_boxes_to_image, in fp32 operation by
 * operation, on rows of a GEMM output read in place: one HIP launch, one thread and one 16-byte store per box.
 *   head        DEVICE [N * rows_per_image][ld]; anchor a of a row has its four deltas at columns delta_col + 4 a .. + 3
 *               and, when score_col >= 0, its score at column score_col + a
 *   anchors     grid mode (grid_h, grid_w >= 1, grid_h * grid_w == rows_per_image): DEVICE [A][4] base anchors; row
 *               (n, y, x) takes base[a] + (x stride_x, y stride_y, x stride_x, y stride_y), torchvision's AnchorGenerator
 *               in the order (y, x, a), the row order of an NHWC head output.  boxes mode (grid_h == grid_w == 0):
 *               DEVICE [N * rows_per_image][4], the same box for every a (the second stage, a = class)
 *   image_hw    DEVICE [N][2] floats (H_img, W_img): the clip window of the row's own image
 *   wx..wh      BoxCoder's weights; clamp: its bbox_xform_clip, log(1000 / 16) in torchvision
 *   boxes       box (n, j, a), j the row within its image, is stored at boxes + 4 (n boxes_image_stride + boxes_offset +
 *               j A + a): strides and offsets count boxes, so that a level writes its slice of an [N][total][4] tensor
 *   scores      with score_col >= 0 the raw score column, no activation, at scores + n scores_image_stride +
 *               scores_offset + j A + a; ignored (may be NULL) otherwise
 * w = ax2 - ax1, h = ay2 - ay1, cx = ax1 + .5 w, cy = ay1 + .5 h;  dx = d0 / wx, dy = d1 / wy, dw = min(d2 / ww, clamp),
 * dh = min(d3 / wh, clamp);  pcx = dx w + cx, pcy = dy h + cy, pw = exp(dw) w, ph = exp(dh) h;  box = (pcx - .5 pw,
 * pcy - .5 ph, pcx + .5 pw, pcy + .5 ph) with x clamped to [0, W_img] and y to [0, H_img].  A NaN delta reaches the
 * coordinates it feeds, as under torch.clamp, and no other box changes a bit.
 * N, rows_per_image >= 0 (either 0: WINO_OK, nothing launched), ld, A >= 1, delta_col >= 0, delta_col + 4 A <= ld,
 * score_col + A <= ld, strides >= 1 in grid mode, N rows_per_image A < 2^31, an image's rows_per_image A boxes between
 * its offset and its image stride (WINO_E_SHAPE otherwise).  A NULL or not 16-byte-aligned pointer, a weight that is zero
 * or not finite, a NaN clamp, or an output that overlaps an input or the other output is WINO_E_ARG.  No workspace and no
 * stream scratch: the call can be captured into a graph as it is. */
int wino_box_decode_hw(const float* head, int N, int rows_per_image, int ld, int A, int delta_col, int score_col,
                       const float* anchors, int grid_h, int grid_w, int stride_y, int stride_x, const float* image_hw,
                       float wx, float wy, float ww, float wh, float clamp, float* boxes, long boxes_image_stride,
                       long boxes_offset, float* scores, long scores_image_stride, long scores_offset, wino_stream_t s);
/* wino_batched_nms_hw: greedy non-maximum suppression over S independent segments of R boxes each, entirely on the
 * device and with fixed-size outputs: two launches (the suppression bit matrix, then one workgroup per segment that
 * walks it; from S = 2^22 on the walk is cut into launches of at most 2^22 - 1 segments), no host read.  Priority is index order within a segment: the caller sorts, and that is part of the contract.
 *   boxes       DEVICE [S][R][4] (x1, y1, x2, y2);  scores: DEVICE [S][R] or NULL;  groups: DEVICE [S][R] int32 or NULL
 *   candidate(i) = x2 - x1 >= min_size && y2 - y1 >= min_size && (scores == NULL || score >= score_thresh); a NaN fails
 *               every compare, so a box with a NaN coordinate or score is never kept and never suppresses
 *   Walking i = 0 .. R - 1: a candidate that is not suppressed is kept; a kept box suppresses every later candidate j of
 *   the same group with inter / (area_i + area_j - inter) > iou_thresh, inter = max(min(x2) - max(x1), 0) *
 *   max(min(y2) - max(y1), 0), torchvision's form in fp32; the walk stops at max_out kept.
 *   keep        DEVICE [S][max_out] int32: the kept indices, ascending, then -1
 *   count       DEVICE [S] int32
 *   rois_out    NULL, or DEVICE [S][max_out][5]: (float(segment), box) for kept rows, (-1, 0, 0, 0, 0) after them:
 *               wino_roi_align_hw's rois as they stand (a row of index -1 pools zeros)
 *   workspace   S * R * ceil(R / 64) * 8 bytes (the bit matrix: R rows of ceil(R / 64) 64-bit words per segment); its
 *               contents before the call do not matter
 * A segment never reads or writes another segment's data.  S >= 0, 0 <= R <= 32768, max_out >= 1, S ceil(R / 64) < 2^24
 * (the mask kernel's workgroups; WINO_E_SHAPE otherwise).  S == 0 or R == 0 is WINO_OK and launches nothing; with R == 0
 * and S > 0 count is zeroed and keep, when given, filled with -1 by memsets, and rois_out is NOT written (the Python
 * wrapper fills it with padding rows).
 * A NULL boxes / keep / count, a pointer that is not 16-byte aligned, a NaN threshold, a workspace that is too small, or
 * an output (keep, count, rois_out, workspace) that overlaps an input or another output is WINO_E_ARG.  Every check
 * comes before the first launch.  No stream scratch: the call can be captured into a graph as it is. */
int wino_batched_nms_hw(const float* boxes, const float* scores, const int* groups, int S, int R, float iou_thresh,
                        float min_size, float score_thresh, int max_out, int* keep, int* count, float* rois_out,
                        void* workspace, size_t workspace_bytes, wino_stream_t s);

/* ---- mask selection and paste: the output stage of Mask R-CNN (mask_paste.hip) -------------------
 * torchvision's maskrcnn_inference followed by paste_masks_in_image(padding = 1) (CPU path: expand_masks, expand_boxes,
 * .to(int64), paste_mask_in_image), operation by operation, for all detections in one HIP launch: detection r = n D + d
 * takes the mask of class labels[r] out of the mask head's logits, applies the sigmoid and pastes it into plane (n, d).
 *   logits    DEVICE, read in place, in one of two layouts:
 *             WINO_MASK_LAYOUT_PLANES     [R][classes][M][M], torchvision's
 *             WINO_MASK_LAYOUT_GEMM_ROWS  [R P P 4][ld], rows ordered (r, y, x, dy, dx), M = 2 P: the output of the mask
 *                                         head's logits GEMM.  Pixel (Y, X) of class c is
 *                                         logits[(((r P + (Y >> 1)) P + (X >> 1)) 4 + (Y & 1) 2 + (X & 1)) ld + c]
 *             R = N D.  `ld` is ignored for PLANES
 *   labels    DEVICE [R] int32.  A label outside [0, classes) (a padding row's -1) makes the plane all zeros and reads no
 *             logit and no box
 *   boxes     DEVICE [R][4] fp32 (x1, y1, x2, y2)
 *   image_hw  DEVICE [N][2] floats (H_img, W_img) as in wino_box_decode_hw, truncated to int and clamped to [0, H] x
 *             [0, W]: torchvision's im_h, im_w.  The plane beyond it is zero
 *   out       [N][D][H][W] fp32 (torchvision's [D][1][H][W] per image), or NULL
 *   binary    [N][D][H][W] uint8 = value > threshold, or NULL.  With both outputs the bytes are those of the stored fp32
 *             values
 * Box (fp32, in this order, no product folded into a sum): scale = float(M + 2) / M; w_half = (x2 - x1) 0.5 scale, x_c =
 * (x2 + x1) 0.5; ex1 = x_c - w_half, ex2 = x_c + w_half, likewise y; bx1 = (int) ex1 ... truncate toward zero (-0.5 -> 0).
 * Named deviation: the expanded coordinates are clamped to +-2^30 before the conversion, and everything below is 64-bit
 * integer arithmetic (torch would have to allocate w x h for such a box).
 * w = max(bx2 - bx1 + 1, 1), h likewise.  Window: x0 = max(bx1, 0), x1e = min(bx2 + 1, im_w), likewise y; an empty window
 * gives a zero plane.  Inside the window the value at (y, x) is the bilinear align_corners=False resize to h x w, at
 * (y - by1, x - bx1), of the (M + 2)^2 map that holds 1 / (1 + exp(-logit)) (computed once per mask element) inside a ring
 * of zeros, with wino_resize_bilinear_hw's exact integer source coordinates per axis (in = M + 2, out = w or h) and its
 * value formula, all four taps always multiplied: a NaN logit reaches exactly the output pixels whose taps include it.
 * Outside the window the value is 0.  A box with a coordinate that is not finite gives NaN in the whole image window
 * [0, im_h) x [0, im_w) of its plane, reads no logit and changes no other plane.
 * 1 <= M <= 62; GEMM_ROWS: M even and classes <= ld; classes >= 1; N, D >= 0 (either 0: WINO_OK, nothing launched);
 * H, W >= 1 of any parity; one plane below 2^31 elements (WINO_E_SHAPE otherwise).  Any N D: planes are addressed from
 * 64-bit bases, the outputs may pass 4 GiB.  A NULL input, out and binary both NULL, a pointer that is not 16-byte
 * aligned, a layout that is neither of the two, a NaN threshold, or an output that overlaps an input or the other output
 * is WINO_E_ARG.  Every check comes before the launch.  No workspace and no stream scratch: the call can be captured
 * into a graph as it is. */
#define WINO_MASK_LAYOUT_PLANES 0
#define WINO_MASK_LAYOUT_GEMM_ROWS 1
int wino_mask_paste_hw(const float* logits, int layout, const int* labels, const float* boxes, const float* image_hw,
                       int N, int D, int classes, int M, int ld, int H, int W, float threshold, float* out, void* binary,
                       wino_stream_t s);

/* ---- heatmaps to keypoints: the output stage of Keypoint R-CNN (keypoints.hip) ---------------------
 * torchvision's heatmaps_to_keypoints -- there a Python loop over detections that reads each box size on the host,
 * allocates a [K][hc][wc] bicubic resize of the detection's heatmaps and takes an argmax over it -- for all R detections
 * and all K keypoints in one HIP launch, one workgroup per (r, k); the resized map is never stored.
 *   maps       DEVICE, read in place, in one of two layouts:
 *              WINO_KP_LAYOUT_PLANES       [R][K][M][M], torchvision's keypoint logits.  `ld` is ignored, bias is NULL
 *              WINO_KP_LAYOUT_DECONV_ROWS  [R P P][ld], M = 4 P: the partial products of ConvTranspose2d(C, K, 4, stride
 *                                          2, padding 1) as a GEMM writes them, row (r, iy, ix), column (ky 4 + kx) K + k,
 *                                          16 K <= ld.  The kernel forms low[k][oy][ox], 2P x 2P: the at most four
 *                                          elements with ky = (oy + 1) mod 2 or that + 2, iy = (oy + 1 - ky) / 2 in
 *                                          [0, P), likewise in x, summed in ascending (ky, kx), then + bias[k].  It
 *                                          upsamples low x2 with wino_resize_bilinear_hw's coordinates (in = 2P, out =
 *                                          4P: lambdas exactly 0, 0.25, 0.75) and value formula -- torch's
 *                                          interpolate(scale_factor=2, bilinear, align_corners=False) -- which gives
 *                                          the M x M plane PLANES would have held
 *   bias       DEVICE [K], required for DECONV_ROWS; NULL for PLANES
 *   rois       DEVICE [R][5] fp32 (n, x1, y1, x2, y2): the RoIAlign rows wino_batched_nms_hw writes into rois_out,
 *              padding rows (-1, 0, 0, 0, 0)
 *   keypoints  DEVICE [R][K][3] fp32 (x, y, 1);  scores  DEVICE [R][K] fp32
 * Box (fp32, in this order, no product folded into a sum): w = max(x2 - x1, 1), wc = (int) ceil(w), cw = w / wc; h, hc,
 * ch likewise.  Plane (r, k) is resized to hc x wc with torch's bicubic, align_corners=False: A = -0.75, taps at
 * i - 1 .. i + 2 with each index clamped into [0, M), all 16 taps always multiplied.  Named deviation: the source
 * coordinate is exact integer arithmetic like wino_resize_bilinear_hw's, but not clamped at 0: per axis num =
 * (2 d + 1) M - out, i = floor_div(num, 2 out), t = float(num - i 2 out) / float(2 out).  pos is the argmax over the
 * hc x wc values under torch.argmax's rules: a NaN is the greatest value, and among equal values the lowest flat index
 * y wc + x wins.  With x_i = pos mod wc, y_i = pos / wc: keypoints[r][k] = ((x_i + 0.5) cw + x1, (y_i + 0.5) ch + y1, 1),
 * scores[r][k] = the value at pos.  The order in which the 16 products are summed is the kernel's own.
 * Special rows.  !(n >= 0) (a padding row): all 3K + K outputs of the row are 0 and nothing else of the row is read.  A
 * box coordinate that is not finite, or wc or hc above max_side: NaN in all of the row's outputs and no map read (named
 * deviation: torch would have to allocate such a map; it cannot occur for boxes clipped to an image no larger than
 * max_side).  A NaN in a map reaches exactly the outputs whose taps include it and changes no other (r, k).
 * 1 <= M <= 64 (DECONV_ROWS: M = 4 P, 1 <= P <= 16, 16 K <= ld), K >= 1, 1 <= max_side <= 16384, R >= 0 (0: WINO_OK,
 * nothing launched); WINO_E_SHAPE otherwise.  maps may pass 2^31 elements: it is addressed from 64-bit bases.  A NULL
 * maps / rois / keypoints / scores, a bias that is NULL for DECONV_ROWS or given for PLANES, a pointer that is not 16-byte
 * aligned, a layout that is neither of the two, or an output that overlaps an input or the other output is WINO_E_ARG.
 * Every check comes before the launch.  No workspace and no stream scratch: the call can be captured into a graph as
 * it is. */
#define WINO_KP_LAYOUT_PLANES 0
#define WINO_KP_LAYOUT_DECONV_ROWS 1
int wino_keypoints_hw(const float* maps, int layout, const float* bias, const float* rois, int R, int K, int M, int ld,
                      int max_side, float* keypoints, float* scores, wino_stream_t s);

/* ---- image transform: the input stage of an R-CNN (image_transform.hip) ---------------------------
 * torchvision's GeneralizedRCNNTransform at test time -- normalise, resize, batch -- for N images of different sizes, in
 * one launch per WINO_TRANSFORM_MAX_IMAGES images (a larger N goes out as several launches of whole images):
 *   images_host  HOST array of N DEVICE pointers (read during the call, like wino_roi_align_hw's hw_host); image i is
 *                [C][h_i][w_i] contiguous, fp32 (dtype WINO_IMAGE_F32) or uint8 (WINO_IMAGE_U8), one dtype per call
 *   hw_host      HOST [N][2] ints (h_i, w_i)
 *   out_hw_host  HOST [N][2] ints (ho_i, wo_i): the size image i is resized to (wino_transform_size gives torchvision's)
 *   mean_host, std_host  HOST [C] floats
 *   out          DEVICE [N][C][Hb][Wb] fp32, NCHW (wino_stem_hw's input).  Plane (i, c) holds the resized image in its
 *                top-left ho_i x wo_i corner and 0 in the rest.  Every element of out is written: no memset is needed
 * Arithmetic, the contract.  A pixel is v = the float (fp32) or float(byte) / 255.0f (uint8).  The normalised tap is
 * t = (v - mean_c) * inv_c in fp32, inv_c = 1.0f / std_c computed once on the host in fp32 (the reciprocal form, not a
 * division per pixel: within 1.5 ulp of torchvision's (v - mean) / std).  The output is the bilinear
 * align_corners=False, no-antialias resize of the taps with wino_resize_bilinear_hw's coordinates and value formula:
 * per axis num = max((2 d + 1) in - out, 0), i0 = num / (2 out), i1 = min(i0 + 1, in - 1), lambda = float(num - i0 * 2
 * out) / float(2 out); value = (1-ly)((1-lx) a + lx b) + ly((1-lx) c + lx d) in fp32, all four taps always multiplied.
 * A NaN pixel therefore reaches exactly the outputs whose taps include it, also when ho == h and wo == w; the 0 of the
 * pad region is stored, never computed from a tap.  Normalising the taps and then interpolating is torchvision's order.
 * Named deviation from torchvision: the source coordinates are exact integers where torch computes an fp32 source
 * coordinate (scale * (d + 0.5) - 0.5, off by 1e-4 relative beyond a few thousand pixels, 7.6e-5 of the value range at
 * 480x640 -> 800x1066) -- the same deviation as wino_resize_bilinear_hw.  None other: the size rule below is torch's
 * bit for bit.
 * One form: a direct gather (a lane owns four consecutive output x of a row, 16-byte stores where the address allows,
 * 4-byte stores on the tails of an odd Wb; tiles wholly in the pad region only store zeros; uint8 taps go through a
 * per-workgroup table of the 256 normalised values per channel).  No workspace and no stream scratch: the descriptors
 * travel in the kernel's arguments and the call can be captured into a graph as it is.
 * N >= 0 (0: WINO_OK, nothing launched), 1 <= C <= 4, Hb, Wb >= 1, h, w, ho, wo >= 1, ho <= Hb, wo <= Wb, 2 ho h and 2 wo w
 * below 2^31, one image of out (C Hb Wb) and each source image (C h w) below 2^31 elements, ceil(Hb / 8) ceil(Wb / 256)
 * below 2^24 (the tiles of a plane are one launch's grid; WINO_E_SHAPE otherwise).  A
 * NULL pointer (a host array, out, or an image), a dtype that is neither of the two, out not 16-byte aligned, an fp32
 * image not 4-byte aligned (uint8 images need no alignment), a mean that is not finite, a std that is zero or not
 * finite or whose fp32 reciprocal is not finite (a denormal), or out overlapping any image is WINO_E_ARG.  Every check comes before the first launch.  Any N.
 *
 * wino_transform_size (host only): torchvision's _resize_image_and_masks followed by F.interpolate(scale_factor = s,
 * recompute_scale_factor = True), bit for bit.  `self_min_size / min_size` there is a Python float over an fp32 tensor,
 * which torch evaluates as reciprocal(tensor) * float, so s_min = fp32(fp32(1 / fp32(min(h, w))) * fp32(min_size)), s_max
 * the same over max(h, w) and max_size, s = min(s_min, s_max), ho = floor(double(h) * double(s)), wo likewise (a true
 * fp32 division gives 799 x 1066 for 480 x 640 at 800 / 1333 where torch gives 800 x 1066).  h, w, min_size, max_size
 * >= 1 and 1 <= ho, wo < 2^31 (WINO_E_SHAPE otherwise); a NULL out-parameter is WINO_E_ARG. */
#define WINO_TRANSFORM_MAX_IMAGES 32
#define WINO_IMAGE_F32 0
#define WINO_IMAGE_U8 1
int wino_image_transform_hw(const void* const* images_host, const int* hw_host, const int* out_hw_host, int N, int C,
                            int dtype, const float* mean_host, const float* std_host, float* out, int Hb, int Wb,
                            wino_stream_t s);
int wino_transform_size(int h, int w, int min_size, int max_size, int* ho, int* wo);

/* ---- segmented top-k and sort (select.hip) ---------------------------------------------------------
 * wino_select_topk_hw: S = N * parts independent segments, entirely on the device and with fixed-size outputs, no host
 * read.  Image i, part p reads n[p] fp32 scores at scores + i * image_stride + off[p].  Its candidates are all n[p]
 * elements, or with use_thresh != 0 only those with score >= score_thresh (a NaN score fails the compare, as in
 * wino_batched_nms_hw).  The segment keeps the best min(k[p], candidates) of them, best first, in this total order:
 *   1. NaN ranks above +Inf (torch's rule for a descending sort / topk);
 *   2. then the larger value; -0.0 and +0.0 are equal; denormals are ordered, not flushed;
 *   3. equal scores, and all NaNs among themselves, go to the lower index.
 * That is torch.sort(descending=True, stable=True) truncated to k[p]: the order of the 64-bit key (orderable(score) << 32)
 * | (0xffffffff - index), orderable(x) = ~bits when the sign bit is set, else bits | 0x80000000, with -0 mapped to +0 and
 * every NaN to 0xffffffff first.  The result is a function of the inputs alone.
 *   off_host, n_host, k_host   HOST arrays of `parts` entries (read during the call, like wino_roi_align_hw's hw_host)
 *   idx        DEVICE int32; image i, part p writes k[p] rows at i * out_stride + sum_{q<p} k[q] (the slots of a
 *              concatenation of the parts): off[p] + the index within the part, i.e. the index within the image's row;
 *              rows past the kept count hold -1
 *   vals       NULL, or DEVICE fp32 in the same slots: the input's own bits (-0.0 and NaN payloads survive); rows past
 *              the kept count hold 0.0
 *   count      DEVICE [N][parts] int32: the kept count
 *   boxes_in   NULL, or DEVICE [N][boxes_image_stride] rows of 4 floats indexed like the scores; boxes_out (same slots as
 *              idx, 16-byte rows) then gets the kept rows, zeros past the kept count.  boxes_out is ignored without it
 *   workspace  the bytes of the formula below (0 when every n[p] <= 8192: the workspace
 *              may then be NULL); its contents before the call do not matter
 * A segment of n[p] <= 8192 is one launch: one workgroup loads it into LDS, sorts the keys with a bitonic network and
 * writes whole rows.  A longer one first runs a radix select over many workgroups (three histogram passes of 11, 11 and
 * 10 bits, a count of the elements that tie with the k-th, an index-ordered gather of the winners into the workspace),
 * then the same sort: seven launches, the five in the middle each reading every score once whatever the values are.
 * A segment never reads or writes another segment's data.
 * 1 <= parts <= 8, N >= 0, N * parts <= 65535 (the launches carry the segment in the grid's y), n[p] >= 0,
 * 1 <= k[p] <= 8192, 0 <= off[p], off[p] + n[p] <= image_stride < 2^31 (and <= boxes_image_stride with boxes_in),
 * sum k[p] <= out_stride (WINO_E_SHAPE otherwise).  N == 0 is WINO_OK and launches nothing; n[p] == 0 gives count 0 and
 * idx -1.  A NULL or not 16-byte-aligned base pointer (off[p] may be any value: a segment need not start 16-byte
 * aligned), a NULL host array, a NaN score_thresh with use_thresh, a workspace that is too small, or an output or the
 * workspace that overlaps an input or another output is WINO_E_ARG.  Every check comes before the first launch.  No
 * stream scratch: the call can be captured into a graph as it is.
 * Workspace bytes, over the long parts L = {p : n[p] > 8192}, each term rounded up to a multiple of 16:
 *   N * |L| * 6148 * 4  (three histograms of 2048 words and four words of list length per long segment)
 *   + N * sum_L ceil(n[p] / 2048) * 4  (the ties per chunk)  + N * sum_L k[p] * 8  (the candidate keys).
 * It grows with every n[p] and k[p]; a smaller workspace is refused.  The Python wrapper's select_workspace_bytes
 * computes it, as nms_workspace_bytes does for wino_batched_nms_hw. */
int wino_select_topk_hw(const float* scores, int N, long image_stride, int parts, const long* off_host,
                        const int* n_host, const int* k_host, int use_thresh, float score_thresh, int* idx, float* vals,
                        int* count, long out_stride, const float* boxes_in, long boxes_image_stride, float* boxes_out,
                        void* workspace, size_t workspace_bytes, wino_stream_t s);

/* wino_select_topk_map_hw: the same select on a padded NHWC map, in place.  map is DEVICE [N][h+2][w+2][ld] fp32 (what
 * a 3x3 layer writes: interior at (1 + y, 1 + x), a ring of one pixel around it, ld - cols pad columns per pixel).
 * Segment i is image i's n = h * w * cols scores map[i][1 + y][1 + x][c], c < cols <= ld, and the index of one is
 *   (y * w + x) * cols + c
 * -- with cols = A * K and the head's channel a * K + k, torchvision's (N, HWA, K) flattening.  Order, NaN and +-0 rules,
 * the score_thresh candidates (>=), k <= 8192 and the fixed-size outputs are wino_select_topk_hw's with parts = 1:
 *   idx    DEVICE int32; image i writes k rows at i * out_stride + out_offset: the index above, -1 past the kept count
 *   vals   NULL, or DEVICE fp32 in the same slots: the score's own bits, 0.0 past the kept count
 *   count  DEVICE [N] int32
 * out_offset (like wino_box_decode_hw's boxes_offset) lets every level of a pyramid write its slice of one [N][sum k]
 * buffer; what lies outside the slice is not written.  The ring and the pad columns have no index: no launch reads them
 * as candidates, whatever they hold.  Offsets into the map are 64-bit (N * (h+2) * (w+2) * ld * 4 passes 4 GiB long
 * before n passes 2^31).  The launches are wino_select_topk_hw's: one for n <= 8192, seven beyond, each of the middle
 * five reading every score once; an element's address costs two multiply-highs, no division.
 * 0 <= N <= 65535, h, w >= 1, 1 <= cols <= ld, 1 <= k <= 8192, (w+2) * ld < 2^32, (h+2) * (w+2) * ld < 2^40,
 * 0 <= out_offset, out_offset + k <= out_stride < 2^31 (WINO_E_SHAPE otherwise); n = h * w * cols > 2^31 - 1 is refused
 * with a message of its own (an index would not fit idx).  Pointer, threshold, workspace and overlap rules as for
 * wino_select_topk_hw.  No stream scratch: capturable as it is.
 * The workspace is the formula above for the one part n = h * w * cols (0 when n <= 8192); the Python wrapper's
 * select_map_workspace_bytes computes it. */
int wino_select_topk_map_hw(const float* map, int N, int h, int w, int cols, int ld, int k, int use_thresh,
                            float score_thresh, int* idx, float* vals, int* count, long out_stride, long out_offset,
                            void* workspace, size_t workspace_bytes, wino_stream_t s);

/* ---- RetinaNet: decode only the selected anchors (retina.hip) -------------------------------------
 * wino_retina_decode_hw: rows offset .. offset + k of image i's idx [N][stride] (DEVICE int32, as
 * wino_select_topk_map_hw writes them with cols = A * K) name class k' = idx % K of anchor idx / K of an h x w level with
 * A anchors per pixel: pixel (idx / K) / A = y * w + x, anchor a = (idx / K) % A.  The deltas of anchor a are columns
 * 4a .. 4a + 3 of pixel (1 + y, 1 + x) of reg, DEVICE [N][h+2][w+2][ld_r] fp32; the anchor is base[a] (DEVICE [A][4])
 * shifted by (x * stride_x, y * stride_y); the box is wino_box_decode_hw's arithmetic with weights (1, 1, 1, 1) and
 * `clamp`, clipped to image_hw[i] (DEVICE [N][2]): bit for bit what wino_box_decode_hw writes in grid mode for that
 * anchor.  Writes the same rows of boxes (DEVICE [N][stride][4] fp32) and labels (DEVICE [N][stride] int32).  A row whose
 * idx is negative (past the kept count) or not below h * w * A * K gets a zero box and label -1 and reads no map.
 * N, k >= 0 (either 0: WINO_OK, nothing launched), N * k < 2^31, h, w, A, K >= 1, h * w * A * K <= 2^31 - 1,
 * 4 * A <= ld_r, (w+2) * ld_r < 2^32, (h+2) * (w+2) * ld_r < 2^40, strides >= 1, 0 <= offset, offset + k <= stride
 * (WINO_E_SHAPE otherwise).  A NULL or not 16-byte-aligned pointer, a NaN clamp, or an output that overlaps an input or
 * the other output is WINO_E_ARG.  No scratch: capturable as it is. */
int wino_retina_decode_hw(const int* idx, int N, int k, long stride, long offset, const float* reg, int h, int w,
                          int ld_r, int A, int K, const float* base, int stride_y, int stride_x, const float* image_hw,
                          float clamp, float* boxes, int* labels, wino_stream_t s);

/* ---- GroupNorm (+ ReLU) on a padded NHWC map (groupnorm.hip) ---------------------------------------
 * wino_groupnorm_relu_hw: torch's F.group_norm(x, G, gamma, beta, eps), then ReLU when relu != 0, on in, DEVICE
 * [N][h+2][w+2][C] fp32 (what a 3x3 layer writes), into out of the same shape.  Statistics per (image, group) over the
 * h * w * (C / G) interior values of the group's channels, biased variance;
 *   out = (in - mean) * (gamma / sqrt(var + eps)) + beta
 * gamma, beta DEVICE [C].  Interior only: no byte of either ring is read or written.  out == in (in place) is allowed;
 * any other overlap of in and out is WINO_E_ARG.  The statistics are Welford updates merged by Chan's formula in an
 * order that is a function of the shape and the form alone (no atomics): two launches give equal bits.  A NaN or Inf
 * element makes its own (image, group) NaN throughout and changes no bit elsewhere; the ReLU propagates NaN.
 * Two forms: WINO_GN_FORM_WHOLE, one launch, a workgroup owns an image's pixels for a block of groups and reads them
 * twice; WINO_GN_FORM_SPLIT, two launches, per-chunk (count, mean, M2, shift) partials in the caller's workspace, merged in
 * chunk order by every workgroup of the second.  wino_groupnorm_plan (host only) names the form and the chunks per image
 * for a device of `cus` CUs (chunks = 1 for the whole form); WINO_GN_FORM = whole | split forces one.
 * The workspace is a formula, like wino_select_topk_hw's: 0 bytes for the whole form, else N * min(h * w, 128) * 4 * G * 4,
 * enough on any device (the Python wrapper's groupnorm_workspace_bytes computes it from the plan).  workspace: 16-byte
 * aligned, at least that; it must not overlap an operand.
 * N >= 0 (0: WINO_OK, nothing launched), h, w >= 1, h * w < 2^31, C a multiple of 64, G a divisor of C with C / G a
 * power of two (1 .. C), (w+2) * C < 2^32, (h+2) * (w+2) * C < 2^40 (WINO_E_SHAPE otherwise; offsets are 64-bit, a map may
 * pass 4 GiB).  A NULL or not 16-byte-aligned pointer, an eps that is not finite and > 0, a workspace that is too small
 * or an overlap is WINO_E_ARG.  Every check comes before the first launch.  No stream scratch: capturable as it is. */
enum { WINO_GN_FORM_WHOLE = 1, WINO_GN_FORM_SPLIT = 2 };
int wino_groupnorm_plan(int N, int h, int w, int C, int G, int cus, int* form, int* chunks);
int wino_groupnorm_relu_hw(const float* in, const float* gamma, const float* beta, float* out, int N, int h, int w, int C,
                           int G, float eps, int relu, void* workspace, size_t workspace_bytes, wino_stream_t s);

/* ---- FCOS: score map and decode of the selected locations (fcos.hip) -----------------------------
 * wino_fcos_score_map_hw: in place on the class-logit map cls, DEVICE [N][h+2][w+2][ld_c] fp32: every interior element
 * in columns < K becomes sqrt(sigmoid(logit) * sigmoid(ctr)), ctr = column ctr_col of the same pixel of reg, DEVICE
 * [N][h+2][w+2][ld_r].  Pad columns and both rings are neither read nor written.  A NaN logit or centerness gives a NaN
 * score; a product that underflows in fp32 gives 0.  h, w, K >= 1, K <= ld_c, 0 <= ctr_col < ld_r, ld_c and ld_r
 * multiples of 4, both maps within (w+2) * ld < 2^32 and (h+2) * (w+2) * ld < 2^40, N * h * w * ceil(K / 4) < 2^31 (WINO_E_SHAPE
 * otherwise); N == 0 is WINO_OK.  NULL, misaligned or overlapping maps are WINO_E_ARG.  No scratch: capturable.
 *
 * wino_fcos_decode_hw: wino_retina_decode_hw's rows, outputs, limits, refusals and padding-row rule, with the
 * anchor-free decode: (l, t, r, b) = max(columns 4a .. 4a + 3, 0) (NaN-propagating), the shifted base anchor's
 * cx = 0.5 * (x1 + x2), cy = 0.5 * (y1 + y2), aw = x2 - x1, ah = y2 - y1, and
 *   box = (cx - l * aw, cy - t * ah, cx + r * aw, cy + b * ah)
 * in fp32 in this order without contraction (torchvision's BoxLinearCoder(normalize_by_size=True).decode), clipped to
 * image_hw[i]. */
int wino_fcos_score_map_hw(float* cls, const float* reg, int N, int h, int w, int K, int ld_c, int ld_r, int ctr_col,
                           wino_stream_t s);
int wino_fcos_decode_hw(const int* idx, int N, int k, long stride, long offset, const float* reg, int h, int w, int ld_r,
                        int A, int K, const float* base, int stride_y, int stride_x, const float* image_hw, float* boxes,
                        int* labels, wino_stream_t s);

/* ---- diagnostics (measurement infrastructure, not part of the reference interface) -------------
 * Re-reads the WINO_* developer knobs (the library reads them once per process). */
int wino_debug_reload_knobs(void);
/* Synchronises `s` and counts the non-zero stream-K ticket counters of its scratch on the current device
 * (0 when the stream has none).  Every launch leaves them at zero: a non-zero count between launches
 * means an item was never finalized (tests assert 0). */
int wino_debug_tickets_in_use(wino_stream_t s, long* nonzero);
/* Test hook: overwrites ticket counter `index` of the stream's scratch on the current device with `value`,
 * as a launch that died mid-way would leave it. */
int wino_debug_poison_ticket(wino_stream_t s, long index, unsigned value);
/* The clock the chip held inside the MOST RECENT launch of a product kernel on the current device:
 * workgroup 0 of every launch stores {s_memtime, s_memrealtime} at its entry and at its exit into a
 * 32-byte slot of the code object (four stores per launch; no output depends on them).  kernel: 0 = the
 * fused 3x3 throughput kernel, 1 = the 1x1 GEMM kernel.  Synchronises `s`, then stamps[0..3] = {cycles,
 * 100 MHz ticks} at entry, the same pair at exit: clock = (stamps[2] - stamps[0]) / (stamps[3] - stamps[1])
 * * 0.1 GHz.  bench.py reads it after the last launch of a timed burst -- the clock OF the timed region. */
int wino_diag_last_clock(int kernel, wino_stream_t s, unsigned long long stamps[4]);
/* The 3x3 throughput kernel's stamped build (same source, s_memtime / s_memrealtime around its main
 * loop): runs one launch of it on `s` with the arguments of wino_conv3x3_bn_relu and writes four
 * uint64 per workgroup to stamps_dev (at least 4 * 2048 uint64): {shader cycles, 100 MHz ticks} at the
 * start of its main loop and the same pair at its end.  *workgroups receives the number of
 * quadruples.  in-kernel clock = d(cycles) / d(ticks) * 0.1 GHz.  14x14 only. */
int wino_diag_conv3x3_clock(const float* in, const float* U, const float* bnBias, const float* bnScale,
                            float* out, int N, int C, int K, unsigned long long* stamps_dev,
                            int* workgroups, wino_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* WINOGRAD_MI355X_H */
