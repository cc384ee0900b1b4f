// The kernels, the workspace layout and the launch sequence of the segmented top-k and sort, as templates on the form
// of the input: select.hip instantiates the flat form (wino_select_topk_hw), select_map.hip the padded-map form
// (wino_select_topk_map_hw).  select.hip's opening comment describes the algorithm.
#pragma once
#include <cmath>

#include "wino_common.h"

namespace wino {
namespace {

typedef unsigned long long u64;
constexpr int SEL_MAX_PARTS = 8;
constexpr int SEL_MAX_K = 8192;             // keys one workgroup sorts in LDS
constexpr int SEL_SORT_THREADS = 1024;
constexpr int SEL_THREADS = 256;            // histogram, count and gather
constexpr int SEL_ROUNDS = 8;
constexpr int SEL_CHUNK = SEL_THREADS * SEL_ROUNDS;   // scores per workgroup and pass
constexpr int SEL_BINS = 2048;
constexpr int SEL_HDR = 3 * SEL_BINS + 4;   // per long segment: three histograms (the third uses 1024 bins), the list's length
constexpr int SEL_MAX_SEGMENTS = 65535;     // blockIdx.y carries the segment

struct SelectArgs {
  const float* scores;
  const f32x4* boxes_in;
  int* idx;
  float* vals;
  int* count;
  f32x4* boxes_out;
  unsigned* hdr;    // [N][longs][SEL_HDR]
  unsigned* eq;     // [N][eq_image]
  u64* cand;        // [N][cand_image]
  long long image_stride, out_stride, boxes_image_stride;
  long long eq_image, cand_image;
  long long off[SEL_MAX_PARTS], eq_off[SEL_MAX_PARTS], cand_off[SEL_MAX_PARTS];
  int n[SEL_MAX_PARTS], k[SEL_MAX_PARTS], kbase[SEL_MAX_PARTS];
  int lp[SEL_MAX_PARTS];   // the part's place among the long parts, -1: n <= SEL_MAX_K
  int parts, longs, use_thresh;
  float thresh;
  // map form (wino_select_topk_map_hw; one part): element j of the segment is column j % cols of pixel j / cols, row-major
  // over the h x w interior of a padded map [h+2][w+2][ld]; image_stride is then the map's, in floats and past 2^31
  unsigned cols, map_w, map_ld, map_pitch;   // map_pitch = (w + 2) ld
  FastDiv div_cols, div_w;
};

// Where element j of a segment lies behind its base: j itself in the flat form.  In the map form the ring and the pad
// columns have no index, so no pass can read them.  Two multiply-highs per element.
template <bool MAP>
__device__ __forceinline__ size_t place(const SelectArgs& a, unsigned j) {
  if (!MAP) return j;
  const unsigned p = fastdiv(j, a.div_cols), c = j - p * a.cols;
  const unsigned y = fastdiv(p, a.div_w), x = p - y * a.map_w;
  return (size_t)(y + 1u) * a.map_pitch + (size_t)(x + 1u) * a.map_ld + c;
}

__device__ __forceinline__ unsigned orderable(float v, int use_thresh, float thresh) {
  if (use_thresh && !(v >= thresh)) return 0u;   // (a NaN fails the compare)
  unsigned b = __float_as_uint(v);
  if ((b & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ u64 composite(unsigned key, unsigned index) {
  return key ? (((u64)key << 32) | (u64)(0xffffffffu - index)) : 0ull;
}

// The digit whose bin holds the k-th largest element of a finished histogram (bins = 1024 or 2048, k >= 1), and the
// rank kr >= 1 that is left inside that bin.  The whole workgroup of 256 threads calls it; false: fewer than k counted.
__device__ bool find_digit(const unsigned* hist, int bins, unsigned k, unsigned* scan, unsigned* res, unsigned& digit,
                           unsigned& kr) {
  const int tid = threadIdx.x, B = bins >> 8;
  unsigned v[8], sum = 0;
#pragma unroll
  for (int b = 0; b < 8; b++) {
    v[b] = b < B ? hist[tid * B + b] : 0u;
    sum += v[b];
  }
  scan[tid] = sum;
  if (tid == 0) res[0] = 0xffffffffu;
  __syncthreads();
  for (int d = 1; d < SEL_THREADS; d <<= 1) {   // inclusive suffix sums
    const unsigned add = tid + d < SEL_THREADS ? scan[tid + d] : 0u;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  const unsigned incl = scan[tid];
  unsigned acc = incl - sum;
  if (acc < k && k <= incl) {   // (one thread at most)
    bool found = false;
#pragma unroll
    for (int b = 7; b >= 0; b--) {
      if (b < B && !found) {
        if (acc + v[b] >= k) {
          res[0] = (unsigned)(tid * B + b);
          res[1] = k - acc;
          found = true;
        }
        acc += v[b];
      }
    }
  }
  __syncthreads();
  digit = res[0];
  kr = res[1];
  __syncthreads();
  return digit != 0xffffffffu;
}

// What the passes before `passes` have decided: prefix = the digits found so far, kr the rank left below them.
// Returns false when the segment has fewer than k candidates (it then takes them all).
__device__ bool resolve(const unsigned* hdr, int passes, unsigned k, unsigned* scan, unsigned* res, unsigned& prefix,
                        unsigned& kr) {
  unsigned d;
  prefix = 0u, kr = k;
  if (passes >= 1) {
    if (!find_digit(hdr, SEL_BINS, kr, scan, res, d, kr)) return false;
    prefix = d;
  }
  if (passes >= 2) {
    find_digit(hdr + SEL_BINS, SEL_BINS, kr, scan, res, d, kr);
    prefix = (prefix << 11) | d;
  }
  if (passes >= 3) {
    find_digit(hdr + 2 * SEL_BINS, SEL_BINS / 2, kr, scan, res, d, kr);
    prefix = (prefix << 10) | d;
  }
  return true;
}

struct Chunk {
  const float* sc;
  unsigned* hdr;
  long long seg;   // image x longs + the part's place
  unsigned n, k, first;
  int image, part;
};
// false (for the whole workgroup): not a long segment, or a chunk past its end
__device__ __forceinline__ bool chunk_of(const SelectArgs& a, Chunk& c) {
  const int s = blockIdx.y;
  c.image = s / a.parts, c.part = s - c.image * a.parts;
  if (a.lp[c.part] < 0) return false;
  c.n = (unsigned)a.n[c.part], c.k = (unsigned)a.k[c.part];
  const u64 first = (u64)blockIdx.x * SEL_CHUNK;
  if (first >= c.n) return false;
  c.first = (unsigned)first;
  c.sc = a.scores + (long long)c.image * a.image_stride + a.off[c.part];
  c.seg = (long long)c.image * a.longs + a.lp[c.part];
  c.hdr = a.hdr + c.seg * SEL_HDR;
  return true;
}

// The long segments' histograms and list lengths start at zero (a kernel, not a memset node: the call is the same
// sequence of launches eagerly and in a graph).
__global__ __launch_bounds__(SEL_THREADS) void select_zero_kernel(unsigned* hdr, const unsigned words) {
  const unsigned t = blockIdx.x * SEL_THREADS + threadIdx.x;
  if (t < words) hdr[t] = 0u;
}

template <bool MAP>
__global__ __launch_bounds__(SEL_THREADS) void select_hist_kernel(const SelectArgs a, const int pass) {
  __shared__ unsigned h[SEL_BINS];
  __shared__ unsigned scan[SEL_THREADS];
  __shared__ unsigned res[2];
  Chunk c;
  if (!chunk_of(a, c)) return;
  unsigned prefix, kr;
  if (!resolve(c.hdr, pass, c.k, scan, res, prefix, kr)) return;
  const int tid = threadIdx.x;
  for (int b = tid; b < SEL_BINS; b += SEL_THREADS) h[b] = 0u;
  __syncthreads();
#pragma unroll
  for (int e = 0; e < SEL_ROUNDS; e++) {
    const unsigned j = c.first + e * SEL_THREADS + tid;   // (first < n < 2^31: no wrap)
    if (j < c.n) {
      const unsigned key = orderable(c.sc[place<MAP>(a, j)], a.use_thresh, a.thresh);
      if (key) {
        if (pass == 0) atomicAdd(&h[key >> 21], 1u);
        else if (pass == 1) { if ((key >> 21) == prefix) atomicAdd(&h[(key >> 10) & 2047u], 1u); }
        else if ((key >> 10) == prefix) atomicAdd(&h[key & 1023u], 1u);
      }
    }
  }
  __syncthreads();
  unsigned* out = c.hdr + pass * SEL_BINS;
  for (int b = tid; b < SEL_BINS; b += SEL_THREADS)
    if (h[b]) atomicAdd(&out[b], h[b]);
}

template <bool MAP>
__global__ __launch_bounds__(SEL_THREADS) void select_count_kernel(const SelectArgs a) {
  __shared__ unsigned scan[SEL_THREADS];
  __shared__ unsigned res[2];
  __shared__ unsigned total;
  Chunk c;
  if (!chunk_of(a, c)) return;
  unsigned T, need;
  if (!resolve(c.hdr, 3, c.k, scan, res, T, need)) return;
  const int tid = threadIdx.x;
  if (tid == 0) total = 0u;
  __syncthreads();
  unsigned mine = 0;
#pragma unroll
  for (int e = 0; e < SEL_ROUNDS; e++) {
    const unsigned j = c.first + e * SEL_THREADS + tid;
    if (j < c.n && orderable(c.sc[place<MAP>(a, j)], a.use_thresh, a.thresh) == T) mine++;
  }
  if (mine) atomicAdd(&total, mine);
  __syncthreads();
  if (tid == 0) a.eq[(long long)c.image * a.eq_image + a.eq_off[c.part] + blockIdx.x] = total;
}

template <bool MAP>
__global__ __launch_bounds__(SEL_THREADS) void select_gather_kernel(const SelectArgs a) {
  __shared__ unsigned scan[SEL_THREADS];
  __shared__ unsigned res[2];
  __shared__ unsigned wsum[SEL_THREADS / 64];
  Chunk c;
  if (!chunk_of(a, c)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned T, need;
  const bool all = !resolve(c.hdr, 3, c.k, scan, res, T, need);
  unsigned before = 0;   // equals of the earlier chunks
  if (all) {
    T = 0u, need = 0u;
  } else {
    const unsigned* eq = a.eq + (long long)c.image * a.eq_image + a.eq_off[c.part];
    unsigned part = 0;
    for (unsigned b = tid; b < blockIdx.x; b += SEL_THREADS) part += eq[b];
    scan[tid] = part;
    __syncthreads();
    for (int d = SEL_THREADS / 2; d > 0; d >>= 1) {
      if (tid < d) scan[tid] += scan[tid + d];
      __syncthreads();
    }
    before = scan[0];
    __syncthreads();
  }
  unsigned* len = c.hdr + 3 * SEL_BINS;
  u64* cand = a.cand + (long long)c.image * a.cand_image + a.cand_off[c.part];
  const u64 below = (1ull << lane) - 1ull;
  for (int e = 0; e < SEL_ROUNDS; e++) {
    const unsigned j = c.first + e * SEL_THREADS + tid;
    const unsigned key = j < c.n ? orderable(c.sc[place<MAP>(a, j)], a.use_thresh, a.thresh) : 0u;
    const bool equal = !all && key == T;
    const u64 eb = __ballot(equal);
    if (lane == 0) wsum[wave] = (unsigned)__popcll(eb);
    __syncthreads();
    unsigned rank = before + (unsigned)__popcll(eb & below), round = 0;
#pragma unroll
    for (int w = 0; w < SEL_THREADS / 64; w++) {
      rank += w < wave ? wsum[w] : 0u;
      round += wsum[w];
    }
    before += round;
    __syncthreads();
    const bool take = key > T || (equal && rank < need);
    const u64 tb = __ballot(take);
    if (tb) {
      unsigned base = 0;
      if (lane == 0) base = atomicAdd(len, (unsigned)__popcll(tb));
      base = __shfl(base, 0);
      const unsigned pos = base + (unsigned)__popcll(tb & below);
      if (take && pos < c.k) cand[pos] = composite(key, j);   // (pos < k always: k - need above T, need equal to it)
    }
  }
}

template <bool MAP>
__global__ __launch_bounds__(SEL_SORT_THREADS) void select_sort_kernel(const SelectArgs a) {
  __shared__ u64 keys[SEL_MAX_K];
  __shared__ int kept_s;
  const int tid = threadIdx.x, s = blockIdx.x;
  const int image = s / a.parts, part = s - image * a.parts;
  const int n = a.n[part], k = a.k[part];
  const long long off = a.off[part];
  const float* sc = a.scores + (long long)image * a.image_stride + off;
  int m = n;   // keys to load
  const u64* cand = nullptr;
  if (a.lp[part] >= 0) {
    const long long seg = (long long)image * a.longs + a.lp[part];
    const unsigned len = a.hdr[seg * SEL_HDR + 3 * SEL_BINS];
    m = (int)(len < (unsigned)k ? len : (unsigned)k);
    cand = a.cand + (long long)image * a.cand_image + a.cand_off[part];
  }
  int P = 1;
  while (P < m) P <<= 1;   // m <= SEL_MAX_K
  for (int j = tid; j < P; j += SEL_SORT_THREADS) {
    u64 key = 0ull;
    if (j < m) key = cand ? cand[j] : composite(orderable(sc[place<MAP>(a, (unsigned)j)], a.use_thresh, a.thresh), (unsigned)j);
    keys[j] = key;
  }
  if (tid == 0) kept_s = 0;
  __syncthreads();
  for (int kk = 2; kk <= P; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += SEL_SORT_THREADS) {
        const int i1 = ((t & ~(j - 1)) << 1) | (t & (j - 1)), i2 = i1 | j;
        const u64 x = keys[i1], y = keys[i2];
        const bool descending = (i1 & kk) == 0;
        if (descending ? x < y : x > y) keys[i1] = y, keys[i2] = x;
      }
      __syncthreads();
    }
  }
  for (int j = tid; j < P; j += SEL_SORT_THREADS)   // the last non-zero key
    if (keys[j] != 0ull && (j + 1 == P || keys[j + 1] == 0ull)) kept_s = j + 1;
  __syncthreads();
  const int kept = kept_s < k ? kept_s : k;
  const long long out0 = (long long)image * a.out_stride + a.kbase[part];
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int r = tid; r < k; r += SEL_SORT_THREADS) {
    int index = -1;
    float v = 0.f;
    f32x4 box = zero;
    const unsigned local = r < kept ? 0xffffffffu - (unsigned)keys[r] : 0xffffffffu;
    if (local < (unsigned)n) {   // (always so below kept; a key that names no element would be written as padding, not followed)
      index = (int)(off + local);
      v = sc[place<MAP>(a, local)];
      if (a.boxes_in) box = a.boxes_in[(long long)image * a.boxes_image_stride + off + local];
    }
    a.idx[out0 + r] = index;
    if (a.vals) a.vals[out0 + r] = v;
    if (a.boxes_out) a.boxes_out[out0 + r] = box;
  }
  if (tid == 0) a.count[s] = kept;
}

size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }

// The workspace's three regions for one call (the header states the formula, Python's select_workspace_bytes mirrors
// it) and each part's place in them; false: an argument outside the limits
struct SelectLayout {
  int longs;
  long long eq_image, cand_image, max_chunks;
  size_t hdr_bytes, eq_bytes, cand_bytes, total;
};
bool select_layout(int N, int parts, const int* n, const int* k, SelectArgs* a, SelectLayout* L) {
  if (N < 0 || parts < 1 || parts > SEL_MAX_PARTS) return false;
  L->longs = 0, L->eq_image = 0, L->cand_image = 0, L->max_chunks = 0;
  for (int p = 0; p < parts; p++) {
    if (n[p] < 0 || k[p] < 1 || k[p] > SEL_MAX_K) return false;
    const bool is_long = n[p] > SEL_MAX_K;
    const long long chunks = is_long ? ((long long)n[p] + SEL_CHUNK - 1) / SEL_CHUNK : 0;
    a->lp[p] = is_long ? L->longs : -1, a->eq_off[p] = L->eq_image, a->cand_off[p] = L->cand_image;
    if (is_long) {
      L->longs++;
      L->eq_image += chunks;
      L->cand_image += k[p];
      if (chunks > L->max_chunks) L->max_chunks = chunks;
    }
  }
  L->hdr_bytes = round16((size_t)N * L->longs * SEL_HDR * sizeof(unsigned));
  L->eq_bytes = round16((size_t)N * L->eq_image * sizeof(unsigned));
  L->cand_bytes = round16((size_t)N * L->cand_image * sizeof(u64));
  L->total = L->hdr_bytes + L->eq_bytes + L->cand_bytes;
  return true;
}

// The launch sequence of both entry points: one sort launch, with the six launches of the radix select before it when
// a part is longer than SEL_MAX_K
template <bool MAP>
int launch_select(const SelectArgs& a, const SelectLayout& L, unsigned S, hipStream_t st) {
  if (L.longs) {
    const unsigned words = (unsigned)(L.hdr_bytes / sizeof(unsigned));   // N longs <= 65535 segments of SEL_HDR words
    hipLaunchKernelGGL(select_zero_kernel, dim3((words + SEL_THREADS - 1) / SEL_THREADS), dim3(SEL_THREADS), 0, st, a.hdr,
                       words);
    if (int rc = launch_status("select_zero_kernel")) return rc;
    const dim3 grid((unsigned)L.max_chunks, S);
    for (int pass = 0; pass < 3; pass++) {
      hipLaunchKernelGGL(select_hist_kernel<MAP>, grid, dim3(SEL_THREADS), 0, st, a, pass);
      if (int rc = launch_status("select_hist_kernel")) return rc;
    }
    hipLaunchKernelGGL(select_count_kernel<MAP>, grid, dim3(SEL_THREADS), 0, st, a);
    if (int rc = launch_status("select_count_kernel")) return rc;
    hipLaunchKernelGGL(select_gather_kernel<MAP>, grid, dim3(SEL_THREADS), 0, st, a);
    if (int rc = launch_status("select_gather_kernel")) return rc;
  }
  hipLaunchKernelGGL(select_sort_kernel<MAP>, dim3(S), dim3(SEL_SORT_THREADS), 0, st, a);
  return launch_status("select_sort_kernel");
}

}  // namespace
}  // namespace wino
