// GroupNorm (+ ReLU) on the padded NHWC map [N][h+2][w+2][C] fp32 that the 3x3 layers write and read: torch's
// F.group_norm(x, G, gamma, beta, eps), statistics per (image, group) over h w cpg values (cpg = C / G, biased variance),
// y = (x - mean) * (gamma / sqrt(var + eps)) + beta, then the NaN-propagating ReLU.  Plain HIP: no MFMA, no inline
// assembly, no atomics, no scratch of the library's, no hand-off between workgroups.  Interior only: no byte of the ring
// is read or written.  out == in is allowed (every element is read and written by one thread).
//
// Lanes and channels.  A workgroup works on a channel block of cb channels, a power of two with cpg <= cb, cb | C,
// cb >= 32; its qpp = cb / 4 channel quads are spread over the threads so that item e = thread + k * THREADS is quad
// e % qpp of pixel e / qpp: with qpp <= THREADS a thread's quad never changes, beyond that (cpg > 4 THREADS) the block is
// one group.  Every global access is one 16-byte load or store; neighbouring lanes read neighbouring quads of a pixel
// row (cb = C = 256: one wave reads one pixel, 1 KiB, per load).
//
// Statistics.  Never E[x^2] - E[x]^2.  Every value is first taken relative to its group's shift, the value of the group's
// first channel at the image's first pixel (one subtraction, exact for values within a factor of two of it), so that
// the means the kernel carries are of the size of the spread and not of the offset; the apply subtracts the same shift.
// A NaN or Inf shift makes the group NaN, as the element itself would.  A thread runs Welford's update over its pixels
// for its four channels (one count, four means, four M2); the four are merged by Chan's formula into the thread's 1, 2
// or 4 groups (cpg >= 4, 2, 1), then across the lanes that share a group by an xor butterfly (operands ordered by lane,
// so both lanes compute the same bits), then across waves through LDS in wave order.  The order of every merge is a
// function of the shape and the form alone: two launches give equal bits.
//
// Two forms (wino_groupnorm_plan names the one a call takes, WINO_GN_FORM = whole | split forces one):
//   whole  one launch, N C / cb workgroups of 1024 threads with cb = max(cpg, 32) (128 bytes per pixel): a workgroup
//          reads every pixel of its image once for the statistics and a second time, from cache, to apply them.
//   split  two launches of 256 threads with cb = max(cpg, min(1024, the largest power of two in C)).  gn_stats_kernel
//          takes a run of cp interior pixels in row order (a chunk) and writes (count, mean, M2, shift) per (image, chunk,
//          group) to the workspace [N][chunks][4][G] (the apply kernel may not read the shift from the map: in place,
//          another workgroup may have overwritten it); gn_apply_kernel's workgroups take the same runs, each merging the
//          partials of its groups in chunk order (so every workgroup that touches a group has the same bits) before it
//          normalises its pixels.  No third launch, no workgroup waits for another.
// The rule between them: DESIGN.md section 3.2t.
#include <cmath>

#include "wino_common.h"

#pragma clang fp contract(off)

namespace wino {
namespace {

constexpr int GN_WHOLE = 1, GN_SPLIT = 2;
constexpr int WHOLE_THREADS = 1024, SPLIT_THREADS = 256;
constexpr unsigned GN_MAX_CHUNKS = 128;          // partials a workgroup of the apply kernel merges per group, at most
// whole while a workgroup's share of an image is at most this: measured at C = 256, G = 32, the
// one launch wins at 50 x 84 (0.5 MiB per workgroup, 35 us against 51) and loses at 100 x 168 (2.1 MiB, 112 against 69)
constexpr unsigned long long GN_WHOLE_BYTES = 1ull << 20;

struct Part {
  float n, mean, m2;
};

// Chan's merge of two (count, mean, M2); an empty side leaves the other's bits.
__device__ __forceinline__ Part chan(Part a, Part b) {
  Part r;
  r.n = a.n + b.n;
  const float f = r.n > 0.f ? b.n / r.n : 0.f;
  const float d = b.mean - a.mean;
  r.mean = a.mean + d * f;
  r.m2 = (a.m2 + b.m2) + (d * d) * (a.n * f);
  if (a.n == 0.f) r.mean = b.mean, r.m2 = b.m2;   // (0 * Inf is NaN: an empty side does not enter the arithmetic)
  if (b.n == 0.f) r.mean = a.mean, r.m2 = a.m2;
  return r;
}

struct GnArgs {
  const float* in;
  float* out;
  const float* gamma;
  const float* beta;
  float* ws;                 // split: [N][chunks][4][G]
  long long image_elems;     // (h + 2)(w + 2) C
  unsigned pitch, C, w, P;   // pitch = (w + 2) C, P = h w
  unsigned cp, chunks;       // pixels of a chunk, chunks of an image (whole: P, 1)
  unsigned cblks, lcb;       // channel blocks of C, log2 cb
  unsigned lq, lcpg;         // log2 qpp, log2 cpg
  unsigned nslots;           // groups of a thread: 1, 2, 4
  unsigned redmask;          // the bits of a thread's number its groups' statistics are reduced over
  unsigned G;
  int relu;
  float eps;
  FastDiv divW;
};

__device__ __forceinline__ size_t gn_offset(const GnArgs& a, unsigned c0, unsigned p0, unsigned long long e, unsigned qmask) {
  const unsigned quad = (unsigned)e & qmask, p = p0 + (unsigned)(e >> a.lq);
  const unsigned y = fastdiv(p, a.divW), x = p - y * a.w;
  return (size_t)(y + 1u) * a.pitch + (size_t)(x + 1u) * a.C + c0 + 4u * quad;
}

// The shifts of this thread's four channels: their groups' first channels at the image's first pixel.
__device__ __forceinline__ void gn_shift(const GnArgs& a, const float* img, unsigned c0, float (&K)[4]) {
  const unsigned c = c0 + 4u * (threadIdx.x & ((1u << a.lq) - 1u));
#pragma unroll
  for (int j = 0; j < 4; j++) K[j] = img[(size_t)a.pitch + a.C + (((c + (unsigned)j) >> a.lcpg) << a.lcpg)];
}

// (count, mean, M2) of this thread's groups over pixels p0 .. p1 of `img`, channels c0 .. c0 + cb: st[s], s < nslots,
// the same bits in every thread that shares the group.  The means are relative to the shifts K.
template <int THREADS>
__device__ __forceinline__ void gn_stats(const GnArgs& a, const float* img, unsigned c0, unsigned p0, unsigned p1, float* lds,
                                         const float (&K)[4], Part (&st)[4]) {
  const unsigned t = threadIdx.x, qmask = (1u << a.lq) - 1u;
  const unsigned long long items = (unsigned long long)(p1 - p0) << a.lq;
  unsigned cnt = 0;
  float mean[4] = {0.f, 0.f, 0.f, 0.f}, m2[4] = {0.f, 0.f, 0.f, 0.f};
  for (unsigned long long e0 = t; e0 < items; e0 += 4ull * THREADS) {
    f32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const unsigned long long e = e0 + (unsigned long long)u * THREADS;
      if (e < items) v[u] = *(const f32x4*)(img + gn_offset(a, c0, p0, e, qmask));
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      if (e0 + (unsigned long long)u * THREADS < items) {
        cnt++;
        const float rn = 1.0f / (float)cnt;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const float x = v[u][j] - K[j];
          const float d = x - mean[j];
          mean[j] = mean[j] + d * rn;
          m2[j] = m2[j] + d * (x - mean[j]);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; j++) st[j] = Part{(float)cnt, mean[j], m2[j]};
  if (a.nslots <= 2) {   // cpg >= 2: channels (0, 1) and (2, 3) are one group each
    st[0] = chan(st[0], st[1]);
    st[1] = chan(st[2], st[3]);
  }
  if (a.nslots == 1) st[0] = chan(st[0], st[1]);
  // across the lanes of a wave
  for (unsigned b = 0; b < 6; b++) {
    if (!((a.redmask >> b) & 1u)) continue;
    const bool upper = (t >> b) & 1u;
#pragma unroll
    for (int s = 0; s < 4; s++) {
      if ((unsigned)s < a.nslots) {
        const Part o = {__shfl_xor(st[s].n, 1 << b), __shfl_xor(st[s].mean, 1 << b), __shfl_xor(st[s].m2, 1 << b)};
        st[s] = upper ? chan(o, st[s]) : chan(st[s], o);
      }
    }
  }
  // across the waves, in wave order
  if (a.redmask >> 6) {
#pragma unroll
    for (int s = 0; s < 4; s++) {
      if ((unsigned)s < a.nslots) {
        lds[(3 * s + 0) * THREADS + t] = st[s].n;
        lds[(3 * s + 1) * THREADS + t] = st[s].mean;
        lds[(3 * s + 2) * THREADS + t] = st[s].m2;
      }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 4; s++) {
      if ((unsigned)s < a.nslots) {
        Part acc = {0.f, 0.f, 0.f};
        for (unsigned v = 0; v < THREADS / 64; v++) {
          const unsigned src = (v << 6) | (t & 63u);
          if (((src ^ t) & ~a.redmask) == 0u)
            acc = chan(acc, Part{lds[(3 * s + 0) * THREADS + src], lds[(3 * s + 1) * THREADS + src], lds[(3 * s + 2) * THREADS + src]});
        }
        st[s] = acc;
      }
    }
  }
}

// out = relu?(((in - K) - mean) * (rstd * gamma) + beta) on pixels p0 .. p1, channels c0 .. c0 + cb, from st of gn_stats'
// shape.
template <int THREADS>
__device__ __forceinline__ void gn_apply(const GnArgs& a, const float* img, float* dst, unsigned c0, unsigned p0, unsigned p1,
                                         const float (&K)[4], const Part (&st)[4]) {
  const unsigned t = threadIdx.x, qmask = (1u << a.lq) - 1u;
  const unsigned long long items = (unsigned long long)(p1 - p0) << a.lq;
  float sm[4], sr[4], mj[4], rj[4];
#pragma unroll
  for (int s = 0; s < 4; s++) {
    sm[s] = st[s].mean;
    sr[s] = 1.0f / sqrtf(st[s].m2 / st[s].n + a.eps);
  }
#pragma unroll
  for (int j = 0; j < 4; j++) {   // channel j belongs to slot j nslots / 4
    const unsigned s = ((unsigned)j * a.nslots) >> 2;
    mj[j] = s == 0 ? sm[0] : s == 1 ? sm[1] : s == 2 ? sm[2] : sm[3];
    rj[j] = s == 0 ? sr[0] : s == 1 ? sr[1] : s == 2 ? sr[2] : sr[3];
  }
  const bool fixed = (1u << a.lq) <= (unsigned)THREADS;   // the thread's quad never changes
  f32x4 g = {0.f, 0.f, 0.f, 0.f}, bt = g;
  if (fixed) {
    g = *(const f32x4*)(a.gamma + c0 + 4u * (t & qmask));
    bt = *(const f32x4*)(a.beta + c0 + 4u * (t & qmask));
  }
  for (unsigned long long e0 = t; e0 < items; e0 += 4ull * THREADS) {
    f32x4 v[4];
    size_t off[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const unsigned long long e = e0 + (unsigned long long)u * THREADS;
      off[u] = gn_offset(a, c0, p0, e < items ? e : 0ull, qmask);
      if (e < items) v[u] = *(const f32x4*)(img + off[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const unsigned long long e = e0 + (unsigned long long)u * THREADS;
      if (e < items) {
        if (!fixed) {
          g = *(const f32x4*)(a.gamma + c0 + 4u * ((unsigned)e & qmask));
          bt = *(const f32x4*)(a.beta + c0 + 4u * ((unsigned)e & qmask));
        }
        f32x4 y;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const float r = __builtin_fmaf((v[u][j] - K[j]) - mj[j], rj[j] * g[j], bt[j]);
          y[j] = a.relu ? relu_nan(r) : r;
        }
        *(f32x4*)(dst + off[u]) = y;
      }
    }
  }
}

__global__ __launch_bounds__(WHOLE_THREADS) void gn_whole_kernel(const GnArgs a) {
  __shared__ float lds[12 * WHOLE_THREADS];
  const unsigned n = blockIdx.x / a.cblks, c0 = (blockIdx.x - n * a.cblks) << a.lcb;
  const size_t base = (size_t)n * (size_t)a.image_elems;
  Part st[4];
  float K[4];
  gn_shift(a, a.in + base, c0, K);
  gn_stats<WHOLE_THREADS>(a, a.in + base, c0, 0u, a.P, lds, K, st);
  __syncthreads();   // in place: every thread holds its shifts and statistics before the first pixel is overwritten
  gn_apply<WHOLE_THREADS>(a, a.in + base, a.out + base, c0, 0u, a.P, K, st);
}

// blockIdx.x = (n chunks + k) cblks + cblk
struct GnBlock {
  unsigned n, k, c0, p0, p1;
};
__device__ __forceinline__ GnBlock gn_block(const GnArgs& a) {
  GnBlock b;
  const unsigned r = blockIdx.x / a.cblks;
  b.c0 = (blockIdx.x - r * a.cblks) << a.lcb;
  b.n = r / a.chunks, b.k = r - b.n * a.chunks;
  b.p0 = b.k * a.cp;
  b.p1 = a.P - b.p0 < a.cp ? a.P : b.p0 + a.cp;
  return b;
}
// the group of slot 0 of this thread
__device__ __forceinline__ unsigned gn_group0(const GnArgs& a, unsigned c0) {
  return (c0 + 4u * (threadIdx.x & ((1u << a.lq) - 1u))) >> a.lcpg;
}

__global__ __launch_bounds__(SPLIT_THREADS) void gn_stats_kernel(const GnArgs a) {
  __shared__ float lds[12 * SPLIT_THREADS];
  const GnBlock b = gn_block(a);
  Part st[4];
  float K[4];
  const float* img = a.in + (size_t)b.n * (size_t)a.image_elems;
  gn_shift(a, img, b.c0, K);
  gn_stats<SPLIT_THREADS>(a, img, b.c0, b.p0, b.p1, lds, K, st);
  if ((threadIdx.x & a.redmask) == 0u) {
    const unsigned step = 4u / a.nslots;   // channels of a slot, of the thread's four
    float* wp = a.ws + ((size_t)b.n * a.chunks + b.k) * 4u * a.G + gn_group0(a, b.c0);
#pragma unroll
    for (int s = 0; s < 4; s++) {
      if ((unsigned)s < a.nslots) {
        wp[s] = st[s].n;
        wp[a.G + s] = st[s].mean;
        wp[2u * a.G + s] = st[s].m2;
        wp[3u * a.G + s] = (unsigned)s * step == 0u ? K[0] : (unsigned)s * step == 1u ? K[1] : (unsigned)s * step == 2u ? K[2] : K[3];
      }
    }
  }
}

__global__ __launch_bounds__(SPLIT_THREADS) void gn_apply_kernel(const GnArgs a) {
  const GnBlock b = gn_block(a);
  const float* wp = a.ws + (size_t)b.n * a.chunks * 4u * a.G + gn_group0(a, b.c0);
  Part st[4] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  for (unsigned k = 0; k < a.chunks; k++) {
    const float* q = wp + (size_t)k * 4u * a.G;
#pragma unroll
    for (int s = 0; s < 4; s++)
      if ((unsigned)s < a.nslots) st[s] = chan(st[s], Part{q[s], q[a.G + s], q[2u * a.G + s]});
  }
  float K[4];
#pragma unroll
  for (int j = 0; j < 4; j++) K[j] = wp[3u * a.G + (((unsigned)j * a.nslots) >> 2)];   // chunk 0's copy
  const size_t base = (size_t)b.n * (size_t)a.image_elems;
  gn_apply<SPLIT_THREADS>(a, a.in + base, a.out + base, b.c0, b.p0, b.p1, K, st);
}

// ---- host: limits and the plan ----------------------------------------------------------------------------------------
unsigned log2u(unsigned v) {
  unsigned l = 0;
  while ((1u << l) < v) l++;
  return l;
}

struct GnPlan {
  int form;
  unsigned cb, cblks, chunks, cp;
  unsigned long long pitch, image;
  unsigned P, cpg;
};

// false: outside the limits (WINO_E_SHAPE)
bool gn_plan(int N, int h, int w, int C, int G, int cus, GnPlan* p) {
  if (N < 0 || h < 1 || w < 1 || C < 64 || C % 64 || G < 1 || G > C || C % G) return false;
  const unsigned cpg = (unsigned)(C / G);
  if (cpg & (cpg - 1u)) return false;
  p->pitch = (unsigned long long)(w + 2ll) * (unsigned long long)C;
  if (p->pitch >= (1ull << 32)) return false;
  p->image = (unsigned long long)(h + 2ll) * p->pitch;
  if (p->image >= (1ull << 40) || (long long)h * w >= (1ll << 31)) return false;
  p->P = (unsigned)((long long)h * w), p->cpg = cpg;
  const unsigned cb_whole = cpg > 32u ? cpg : 32u;
  const int forced = knobs().gn_form;
  p->form = forced == GN_WHOLE || forced == GN_SPLIT ? forced
                                                     : ((unsigned long long)p->P * cb_whole * 4ull <= GN_WHOLE_BYTES ? GN_WHOLE : GN_SPLIT);
  if (p->form == GN_WHOLE) {
    p->cb = cb_whole, p->chunks = 1u, p->cp = p->P;
  } else {
    const unsigned pow2 = (unsigned)C & (0u - (unsigned)C), wide = pow2 < 1024u ? pow2 : 1024u;
    p->cb = cpg > wide ? cpg : wide;
  }
  p->cblks = (unsigned)C / p->cb;
  if (p->form == GN_SPLIT) {
    // about two workgroups per CU, GN_MAX_CHUNKS partials per group at the most, whole passes of the workgroup's lanes
    const unsigned long long per_chunk = (unsigned long long)(N > 0 ? N : 1) * p->cblks;
    unsigned long long want = (2ull * (unsigned long long)(cus > 0 ? cus : 1) + per_chunk - 1ull) / per_chunk;
    want = want < 1ull ? 1ull : want > GN_MAX_CHUNKS ? GN_MAX_CHUNKS : want;
    const unsigned qpp = p->cb / 4u, pass = qpp < (unsigned)SPLIT_THREADS ? (unsigned)SPLIT_THREADS / qpp : 1u;
    unsigned long long cp = ((unsigned long long)p->P + want - 1ull) / want;
    cp = (cp + pass - 1ull) / pass * pass;
    p->cp = (unsigned)(cp < p->P ? cp : p->P);
    p->chunks = (p->P + p->cp - 1u) / p->cp;
  }
  return (unsigned long long)N * p->cblks * p->chunks <= 0x7fffffffull;
}

size_t gn_workspace_bytes(int N, const GnPlan& p, int G) {
  if (p.form == GN_WHOLE) return 0;
  const unsigned most = p.P < GN_MAX_CHUNKS ? p.P : GN_MAX_CHUNKS;   // whatever the device's CU count makes of it
  return (size_t)N * most * 4u * (size_t)G * sizeof(float);
}

}  // namespace
}  // namespace wino

using namespace wino;

extern "C" int wino_groupnorm_plan(int N, int h, int w, int C, int G, int cus, int* form, int* chunks) {
  if (int rc = check_nonnull(form, chunks)) return rc;
  GnPlan p;
  if (cus < 1 || !gn_plan(N, h, w, C, G, cus, &p)) {
    set_error("groupnorm_plan: unsupported shape N=%d h=%d w=%d C=%d G=%d cus=%d", N, h, w, C, G, cus);
    return WINO_E_SHAPE;
  }
  *form = p.form, *chunks = (int)p.chunks;
  return WINO_OK;
}

extern "C" int wino_groupnorm_relu_hw(const float* in, const float* gamma, const float* beta, float* out, int N, int h, int w,
                                      int C, int G, float eps, int relu, void* workspace, size_t workspace_bytes,
                                      wino_stream_t s) {
  GnPlan p;
  int dev = 0, cus = 256;
  bool ok = gn_plan(N, h, w, C, G, 256, &p);   // the limits do not depend on the device
  if (ok && N > 0) {
    if (int rc = current_device(&dev, &cus)) return rc;
    ok = gn_plan(N, h, w, C, G, cus, &p);
  }
  if (!ok) {
    set_error("groupnorm_relu: unsupported shape N=%d h=%d w=%d C=%d G=%d (need N >= 0, h, w >= 1, h w < 2^31, C a multiple "
              "of 64, G a divisor of C with C / G a power of two, (w + 2) C < 2^32, (h + 2)(w + 2) C < 2^40)", N, h, w, C, G);
    return WINO_E_SHAPE;
  }
  if (N == 0) return WINO_OK;
  if (int rc = check_nonnull(in, gamma, beta, out)) return rc;
  if (int rc = check_aligned16(in, gamma, beta, out)) return rc;
  if (!(eps > 0.f) || !std::isfinite(eps)) {
    set_error("groupnorm_relu: eps must be finite and > 0");
    return WINO_E_ARG;
  }
  const size_t need = gn_workspace_bytes(N, p, G);
  if (need) {
    if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) {
      set_error("tensor pointers must be 16-byte aligned (workspace)");
      return WINO_E_ARG;
    }
  }
  const size_t map_b = (size_t)N * (size_t)p.image * 4, vec_b = (size_t)C * 4;
  bool clash = (in != out && overlaps(in, map_b, out, map_b)) || overlaps(gamma, vec_b, out, map_b) ||
               overlaps(beta, vec_b, out, map_b);
  if (need)
    clash = clash || overlaps(workspace, need, in, map_b) || overlaps(workspace, need, out, map_b) ||
            overlaps(workspace, need, gamma, vec_b) || overlaps(workspace, need, beta, vec_b);
  if (clash) {
    set_error("groupnorm_relu: out must be in itself or not overlap it; gamma, beta and the workspace must not overlap "
              "out, and the workspace none of the operands");
    return WINO_E_ARG;
  }
  GnArgs a;
  a.in = in, a.out = out, a.gamma = gamma, a.beta = beta, a.ws = (float*)workspace;
  a.image_elems = (long long)p.image, a.pitch = (unsigned)p.pitch, a.C = (unsigned)C, a.w = (unsigned)w, a.P = p.P;
  a.cp = p.cp, a.chunks = p.chunks, a.cblks = p.cblks, a.lcb = log2u(p.cb);
  a.lq = a.lcb - 2u, a.lcpg = log2u(p.cpg);
  a.nslots = p.cpg >= 4u ? 1u : 4u / p.cpg;
  const unsigned threads = p.form == GN_WHOLE ? WHOLE_THREADS : SPLIT_THREADS;
  const unsigned qpp = 1u << a.lq, ql = p.cpg >= 4u ? p.cpg / 4u : 1u;
  a.redmask = 0u;
  for (unsigned b = 0; (1u << b) < threads; b++)
    if ((1u << b) < ql || (1u << b) >= qpp) a.redmask |= 1u << b;
  a.G = (unsigned)G, a.relu = relu ? 1 : 0, a.eps = eps, a.divW = make_fastdiv(a.w);
  const unsigned grid = (unsigned)N * p.cblks * p.chunks;
  if (p.form == GN_WHOLE) {
    hipLaunchKernelGGL(gn_whole_kernel, dim3(grid), dim3(WHOLE_THREADS), 0, (hipStream_t)s, a);
    return launch_status("gn_whole_kernel");
  }
  hipLaunchKernelGGL(gn_stats_kernel, dim3(grid), dim3(SPLIT_THREADS), 0, (hipStream_t)s, a);
  if (int rc = launch_status("gn_stats_kernel")) return rc;
  hipLaunchKernelGGL(gn_apply_kernel, dim3(grid), dim3(SPLIT_THREADS), 0, (hipStream_t)s, a);
  return launch_status("gn_apply_kernel");
}
