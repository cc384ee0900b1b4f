// The two small kernels of a squeeze-excite block and of MobileNetV3's classifier, beside the depthwise layer's pool
// partials (depthwise_ex.hip).  Plain HIP: no MFMA, no inline assembly, no atomics, no scratch.
//
// wino_fc_act_hw: a skinny fully connected layer for a handful of rows,
//   out[n][j] = act(sum_c W[j][c] x[n][c] + b[j]),   x[n][c] = x_scale * sum_p parts[n][p][c]  (p in index order)
// M = N is a few dozen rows at most against up to 2048 x J weights: the layer is bound by reading W once, so there is
// nothing for the matrix pipe.  A workgroup of four waves owns FC_JB = 8 outputs, two per wave, and keeps their rows
// of W in registers (lanes stride over c in quads: lane l holds quads l, l + 64, ..: FC_QL = 8 of them at C = 2048, 64
// VGPRs for the two rows), so W is read once per launch; it then walks the images in chunks of FC_NB = 8, staging the
// chunk's x in LDS (where the partial sums are added up and scaled) and, per (image, output), summing the lane's
// products in quad order by fma and the 64 lanes by a fixed xor butterfly (32, 16, .., 1), the chunk's sixteen butterflies
// side by side.  Nothing in an image's sum
// depends on the batch or on its place in a chunk: a row has the same bits alone and inside a batch.
//
// wino_act_scale_pool_hw: x = act(x) * gate[n][c] in place on a flat [N][H W][C] or padded [N][H+2][W+2][C] map (the ring
// of a padded one is not touched), and optionally the channel sums of what it stored over chunks of AS_PIX = 64 pixels,
// pool_partials[N][P][C], P = ceil(H W / 64) (wino_act_scale_pool_plan).  Memory-bound: a workgroup owns one image, 64
// channels and one pixel chunk; thread t is quad t % 16 of pixels t / 16 + 16 i, so a wave moves whole runs of 64
// channels of consecutive pixels in 16-byte accesses.  The sums: a thread's four pixels in order, then the sixteen
// threads of a quad in order through LDS.
#include "wino_act.h"

#pragma clang fp contract(off)

namespace wino {
namespace {

// ---- fc_act -----------------------------------------------------------------------------------------------------------
constexpr int FC_THREADS = 256, FC_WAVES = 4, FC_JW = 2, FC_JB = FC_WAVES * FC_JW;
constexpr int FC_NB = 8, FC_CMAX = 2048, FC_QL = FC_CMAX / 4 / 64;

struct FcArgs {
  const float* parts;   // [N][P][C]
  const float* W;       // [J][C]
  const float* b;       // [J]
  float* out;           // [N][J]
  float x_scale;
  int N, P, C, J, act;
};

// blockIdx.x: the block of FC_JB outputs
__global__ __launch_bounds__(FC_THREADS) void fc_act_kernel(const FcArgs a) {
  __shared__ f32x4 xs[FC_NB * FC_CMAX / 4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int CQ = a.C >> 2;   // quads of a row
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const int j0 = blockIdx.x * FC_JB + wave * FC_JW;

  f32x4 w[FC_JW][FC_QL];
#pragma unroll
  for (int jj = 0; jj < FC_JW; jj++)
#pragma unroll
    for (int i = 0; i < FC_QL; i++) {
      const int cq = lane + 64 * i;
      w[jj][i] = (j0 + jj < a.J && cq < CQ) ? *(const f32x4*)(a.W + (size_t)(j0 + jj) * a.C + 4 * cq) : zero;
    }
  float bj[FC_JW];
#pragma unroll
  for (int jj = 0; jj < FC_JW; jj++) bj[jj] = j0 + jj < a.J ? a.b[j0 + jj] : 0.f;

  for (int n0 = 0; n0 < a.N; n0 += FC_NB) {
    const int nb = min(FC_NB, a.N - n0);
    __syncthreads();   // the chunk before this one has been read
    // quad e = nl CQ + cq of the chunk; four quads and four partials per step are in flight, added in index order
    const int total = nb * CQ;
    for (int e0 = t; e0 < total; e0 += 4 * FC_THREADS) {
      const float* src[4];
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int e = min(e0 + u * FC_THREADS, total - 1), nl = e / CQ;
        src[u] = a.parts + (size_t)(n0 + nl) * a.P * a.C + 4 * (e - nl * CQ);
        v[u] = *(const f32x4*)src[u];
      }
#pragma unroll 4
      for (int p = 1; p < a.P; p++) {
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] += *(const f32x4*)(src[u] + (size_t)p * a.C);
      }
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (e0 + u * FC_THREADS < total) xs[e0 + u * FC_THREADS] = v[u] * a.x_scale;
    }
    __syncthreads();
    // the chunk's FC_NB x FC_JW sums side by side: their butterflies are independent chains that overlap
    float acc[FC_NB][FC_JW];
#pragma unroll
    for (int nl = 0; nl < FC_NB; nl++)
#pragma unroll
      for (int jj = 0; jj < FC_JW; jj++) acc[nl][jj] = 0.f;
#pragma unroll
    for (int i = 0; i < FC_QL; i++) {
      const int cq = lane + 64 * i;
      if (cq < CQ) {
#pragma unroll
        for (int nl = 0; nl < FC_NB; nl++) {
          if (nl < nb) {
            const f32x4 x = xs[nl * CQ + cq];
#pragma unroll
            for (int jj = 0; jj < FC_JW; jj++)
#pragma unroll
              for (int ch = 0; ch < 4; ch++) acc[nl][jj] = __builtin_fmaf(w[jj][i][ch], x[ch], acc[nl][jj]);
          }
        }
      }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
      for (int nl = 0; nl < FC_NB; nl++)
#pragma unroll
        for (int jj = 0; jj < FC_JW; jj++) acc[nl][jj] += __shfl_xor(acc[nl][jj], m, 64);
#pragma unroll
    for (int nl = 0; nl < FC_NB; nl++)
#pragma unroll
      for (int jj = 0; jj < FC_JW; jj++)
        if (lane == 0 && nl < nb && j0 + jj < a.J)
          a.out[(size_t)(n0 + nl) * a.J + (j0 + jj)] = act_apply(acc[nl][jj] + bj[jj], a.act);
  }
}

// ---- act_scale_pool ---------------------------------------------------------------------------------------------------
constexpr int AS_THREADS = 256, AS_CB = 64, AS_QPP = AS_CB / 4, AS_LANES = AS_THREADS / AS_QPP, AS_RP = 4;
constexpr int AS_PIX = AS_LANES * AS_RP;   // pixels of a chunk

struct AsArgs {
  float* x;
  const float* gate;    // [N][C] or null
  float* pool;          // [N][P][C] or null
  long long image;      // elements of one image of the map
  unsigned HW, W, C, P, cblks, pad;   // pad: 1 for a padded map
  int act;
  FastDiv divC, divP, divW;
};

// blockIdx.x = (n P + chunk) cblks + cblk
__global__ __launch_bounds__(AS_THREADS) void act_scale_pool_kernel(const AsArgs a) {
  __shared__ f32x4 red[AS_THREADS];
  const unsigned t = threadIdx.x, q = t % AS_QPP, pl = t / AS_QPP;
  unsigned r = fastdiv(blockIdx.x, a.divC);
  const unsigned cblk = blockIdx.x - r * a.cblks;
  const unsigned n = fastdiv(r, a.divP), chunk = r - n * a.P;
  const unsigned c = cblk * AS_CB + 4u * q;
  const bool live = c < a.C;
  const f32x4 one = {1.f, 1.f, 1.f, 1.f}, zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 psum = zero;
  if (live) {
    const f32x4 g = a.gate ? *(const f32x4*)(a.gate + (size_t)n * a.C + c) : one;
    float* img = a.x + (size_t)n * (size_t)a.image;
    f32x4 v[AS_RP];
    unsigned off[AS_RP];
    bool in[AS_RP];
#pragma unroll
    for (int i = 0; i < AS_RP; i++) {
      const unsigned p = chunk * AS_PIX + (unsigned)i * AS_LANES + pl;
      const unsigned y = fastdiv(p, a.divW), x = p - y * a.W;
      in[i] = p < a.HW;
      off[i] = ((y + a.pad) * (a.W + 2u * a.pad) + x + a.pad) * a.C + c;
      v[i] = zero;
      if (in[i]) v[i] = *(const f32x4*)(img + off[i]);
    }
#pragma unroll
    for (int i = 0; i < AS_RP; i++) {
      if (in[i]) {
        f32x4 y = act_apply4(v[i], a.act);
        if (a.gate) y *= g;
        *(f32x4*)(img + off[i]) = y;
        psum += y;
      }
    }
  }
  if (a.pool) {   // (uniform over the launch)
    red[t] = psum;
    __syncthreads();
    if (t < AS_QPP && live) {
      f32x4 s = red[t];
#pragma unroll
      for (int i = 1; i < AS_LANES; i++) s += red[t + i * AS_QPP];
      *(f32x4*)(a.pool + ((size_t)n * a.P + chunk) * a.C + c) = s;
    }
  }
}

int as_shape(int N, int H, int W, int C, int padded, unsigned long long* image, unsigned* P, unsigned long long* grid) {
  if (N < 0 || H < 1 || W < 1 || C < 4 || C % 4) {
    set_error("act_scale_pool: unsupported shape N=%d H=%d W=%d C=%d (need N >= 0, H, W >= 1, C a multiple of 4)", N, H, W, C);
    return WINO_E_SHAPE;
  }
  const unsigned long long pad = padded ? 2 : 0;
  *image = (H + pad) * (W + pad) * (unsigned long long)C;
  if (*image >= (1ull << 31)) {
    set_error("act_scale_pool: one image must stay below 2^31 elements (H=%d W=%d C=%d)", H, W, C);
    return WINO_E_SHAPE;
  }
  *P = (unsigned)(((unsigned long long)H * W + AS_PIX - 1) / AS_PIX);
  *grid = (unsigned long long)N * *P * (((unsigned)C + AS_CB - 1u) / AS_CB);
  if (*grid > 0x7fffffffull) {
    set_error("act_scale_pool: %llu workgroups (N=%d H=%d W=%d C=%d): the launch holds 2^31 - 1", *grid, N, H, W, C);
    return WINO_E_SHAPE;
  }
  return WINO_OK;
}

}  // namespace
}  // namespace wino

using namespace wino;

extern "C" int wino_fc_act_hw(const float* parts, float x_scale, const float* W, const float* b, float* out, int N, int P,
                              int C, int J, int act, wino_stream_t s) {
  if (N < 0 || P < 1 || C < 4 || C % 4 || C > FC_CMAX || J < 1 || J > (1 << 30)) {
    set_error("fc_act: unsupported shape N=%d P=%d C=%d J=%d (need N >= 0, P, J >= 1, C a multiple of 4 up to %d)", N, P, C, J,
              FC_CMAX);
    return WINO_E_SHAPE;
  }
  const unsigned long long parts_e = (unsigned long long)N * P * C, w_e = (unsigned long long)J * C;
  if (parts_e >= (1ull << 40)) {
    set_error("fc_act: operands too large (N=%d P=%d C=%d J=%d)", N, P, C, J);
    return WINO_E_SHAPE;
  }
  if (!act_known(act)) {
    set_error("fc_act: unknown act %d", act);
    return WINO_E_ARG;
  }
  if (N == 0) return WINO_OK;
  if (int rc = check_nonnull(parts, W, b, out)) return rc;
  if (int rc = check_aligned16(parts, W)) return rc;
  if ((reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(out)) & 3u) {
    set_error("fc_act: b and out must be 4-byte aligned");
    return WINO_E_ARG;
  }
  const size_t out_b = (size_t)N * J * 4;
  if (overlaps(parts, parts_e * 4, out, out_b) || overlaps(W, w_e * 4, out, out_b) || overlaps(b, (size_t)J * 4, out, out_b)) {
    set_error("fc_act: out must not overlap parts, W or b");
    return WINO_E_ARG;
  }
  FcArgs a;
  a.parts = parts, a.W = W, a.b = b, a.out = out, a.x_scale = x_scale;
  a.N = N, a.P = P, a.C = C, a.J = J, a.act = act;
  hipLaunchKernelGGL(fc_act_kernel, dim3((unsigned)((J + FC_JB - 1) / FC_JB)), dim3(FC_THREADS), 0, (hipStream_t)s, a);
  return launch_status("fc_act_kernel");
}

extern "C" int wino_act_scale_pool_plan(int N, int H, int W, int C, int padded, int* pix_chunk, int* parts) {
  if (int rc = check_nonnull(pix_chunk, parts)) return rc;
  unsigned long long image, grid;
  unsigned P;
  if (int rc = as_shape(N, H, W, C, padded, &image, &P, &grid)) return rc;
  *pix_chunk = AS_PIX, *parts = (int)P;
  return WINO_OK;
}

extern "C" int wino_act_scale_pool_hw(float* x, const float* gate, float* pool_partials, int N, int H, int W, int C, int padded,
                                      int act, int pool_parts, wino_stream_t s) {
  unsigned long long image, grid;
  unsigned P;
  if (int rc = as_shape(N, H, W, C, padded, &image, &P, &grid)) return rc;
  if (!act_known(act)) {
    set_error("act_scale_pool: unknown act %d", act);
    return WINO_E_ARG;
  }
  if (pool_partials && pool_parts != (int)P) {
    set_error("act_scale_pool: pool_parts = %d, the map has %u pixel chunks", pool_parts, P);
    return WINO_E_ARG;
  }
  if (N == 0) return WINO_OK;
  if (int rc = check_nonnull(x)) return rc;
  if (int rc = check_aligned16(x, gate, pool_partials)) return rc;
  const size_t x_b = (size_t)N * (size_t)image * 4, g_b = gate ? (size_t)N * C * 4 : 0;
  const size_t p_b = pool_partials ? (size_t)N * P * C * 4 : 0;
  if ((gate && overlaps(x, x_b, gate, g_b)) || (pool_partials && (overlaps(x, x_b, pool_partials, p_b) ||
                                                                  (gate && overlaps(gate, g_b, pool_partials, p_b))))) {
    set_error("act_scale_pool: x, gate and pool_partials must not overlap");
    return WINO_E_ARG;
  }
  AsArgs a;
  a.x = x, a.gate = gate, a.pool = pool_partials, a.image = (long long)image;
  a.HW = (unsigned)H * (unsigned)W, a.W = (unsigned)W, a.C = (unsigned)C, a.P = P, a.pad = padded ? 1u : 0u;
  a.cblks = ((unsigned)C + AS_CB - 1u) / AS_CB, a.act = act;
  a.divC = make_fastdiv(a.cblks), a.divP = make_fastdiv(P), a.divW = make_fastdiv((unsigned)W);
  hipLaunchKernelGGL(act_scale_pool_kernel, dim3((unsigned)grid), dim3(AS_THREADS), 0, (hipStream_t)s, a);
  return launch_status("act_scale_pool_kernel");
}
