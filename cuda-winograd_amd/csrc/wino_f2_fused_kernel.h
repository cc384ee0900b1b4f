// The fused Winograd F(2x2,3x3) kernel, as a header so that the library
// (wino_f2_fused.hip) and the ablation tool (tools/ablate_fused.hip) compile the same source.
//
// ABLATE is a developer knob (PROBE_OFF = the product kernel): its bits (PROBE_*) and the stamp buffers the
// diagnostic builds write (prm.dbg) are listed in wino_probe.h.
//
// Work decomposition: the launch's work is a set of "chunk iterations"
//   (item, chunk),  item = (tile block, k block),  chunk = 8 input channels,
// nTB * K/64 * C/8 of them, all of equal cost.  G logical workgroups (at most one per CU) share
// them in two phases:
//   * whole-item rounds: ndp = items / G rounds in which workgroup l owns item r*G + l outright.
//     All workgroups then walk the same chunk index at the same time, so the K/64 k-blocks that
//     share a tile block's patches and the tile blocks that share a filter chunk hit each other's
//     lines in the XCD's L2 (about 80 % hit rate over the whole launch, profiles/);
//   * a stream-K tail for the remaining items % G items: their chunk iterations, in item-major
//     order, are cut into G equal contiguous ranges.  At 256 channels and N = 128: 392 items on
//     256 CUs = one whole item (32 iterations) + 17 tail iterations each = 49 per CU, instead of
//     the 64 a second whole-item round would cost.  (All 392 items as one stream-K range were
//     measured too: the scattered channel phases halve the L2 hit rate and quadruple HBM traffic.)
// A tail range cuts an item into at most two partial SEGMENTS per workgroup (the head and the tail
// of its range).  A partial segment applies A^T m A to its partial sums (the inverse transform is
// linear), publishes the 64 KB pre-BN result as a write-through slab and draws a ticket on the
// item's counter; the wave that draws the last ticket adds the other segments' slabs (in segment
// order, whoever is last: the result is bitwise reproducible), applies BN + ReLU and stores.
// Nobody ever waits on another workgroup, so there is no residency assumption and no deadlock; the
// hand-off follows the write-through recipe (sc1 stores, the storing wave drains vmcnt, one relaxed
// agent-scope ticket add, sc1 loads by the reducer).
// Order of a range: a range that crosses an item boundary (a "straddler", two partial segments) runs its tail
// FIRST: its hand-offs complete in the middle of the launch and it ends with a whole item.  A range that lies
// inside ONE item (one partial segment) runs its whole items first and that segment LAST: by then the item's other
// segments were published a whole item ago, so this workgroup is the item's natural last arriver.
// The peek: a partial segment that would draw its ticket at once first LOOKS at the counter (one relaxed load per
// wave, in flight under A^T m A).  At nseg - 1 every other segment has drained and drawn and nobody else will look
// at the item again: the wave finishes it from its registers -- it never publishes its own part, draws no ticket
// and reads only the OTHER segments' slabs, its own part taking its place in the segment order (same operands,
// same order, same bits).  At anything less it takes the ticket path above, unchanged.  A shortcut, never a wait.
// And a ticket that comes back 0 was the item's first of at least two: its drawer skips the walk over the item's
// segments, which had nothing to tell it.
#pragma once
#include "wino_common.h"

#include <type_traits>

namespace wino {
namespace fused {

constexpr int TB = 64;                       // tiles per workgroup
constexpr int KB = 64;                       // out-channels per workgroup
constexpr int BC = 8;                        // in-channels per pipeline stage
constexpr int NTHREADS = 512;
constexpr int RAW_BYTES = TB * 16 * BC * 4;  // 32768: one raw-patch stage
constexpr int U_BYTES = 16 * KB * BC * 4;    // 32768: one filter stage
constexpr int N_RSTAGE = 2, N_USTAGE = 3;
constexpr int LDS_BYTES = N_RSTAGE * RAW_BYTES + N_USTAGE * U_BYTES;  // 163840 = all 160 KiB of the CU
constexpr int U_CHUNK_FLOATS = 16 * KB * BC; // 8192 floats per (c-chunk, k-block)
constexpr int PF = 2;                        // filter-fragment prefetch distance (points); 2..6 measured equal
constexpr int SLAB_BYTES = TB * 4 * KB * 4;  // 65536: pre-BN output of one item (64 tiles x 2x2 px x 64 k)
// First point-step that issues an LDS-DMA piece.  tools/ablate_fused 256 256 q with the iteration's barrier behind step 1
// (SYNC_STEP): 2 / 4 / 6 / 7 / 8 give 39.5 / 39.2 / 38.8 / 38.8 / 38.9-39.1 cycles per MFMA (the barrier at the top of the
// body: 4 / 6 gave 39.2 / 39.3) -- the pieces' barrier moved two steps back, and so did the best start.  The
// any-feature-map build keeps 4: at 7x7x512 (whole 64-iteration items, all 256 workgroups asking for the same filter
// chunk in the same step) 6 measured +0.4 % and 4 equal to the barrier at the top (profiles/loop_barrier/).
constexpr int dma0_for(bool gen) { return gen ? 4 : 6; }

// s_waitcnt lgkmcnt(n) alone (vmcnt/expcnt fields at "no wait"); n folds to a literal once the
// point loop is unrolled.
__device__ __forceinline__ void wait_lds(int n) {
  switch (n) {
    case 0: __builtin_amdgcn_s_waitcnt(0xC07F); break;
    case 1: __builtin_amdgcn_s_waitcnt(0xC17F); break;
    case 2: __builtin_amdgcn_s_waitcnt(0xC27F); break;
    case 3: __builtin_amdgcn_s_waitcnt(0xC37F); break;
    case 4: __builtin_amdgcn_s_waitcnt(0xC47F); break;
    case 5: __builtin_amdgcn_s_waitcnt(0xC57F); break;
    case 6: __builtin_amdgcn_s_waitcnt(0xC67F); break;
    case 7: __builtin_amdgcn_s_waitcnt(0xC77F); break;
    case 8: __builtin_amdgcn_s_waitcnt(0xC87F); break;
    case 9: __builtin_amdgcn_s_waitcnt(0xC97F); break;
    case 10: __builtin_amdgcn_s_waitcnt(0xCA7F); break;
    case 11: __builtin_amdgcn_s_waitcnt(0xCB7F); break;
    case 12: __builtin_amdgcn_s_waitcnt(0xCC7F); break;
    default: __builtin_amdgcn_s_waitcnt(0xCF7F); break;
  }
}
// The iteration's vmcnt(0) + barrier sits BEHIND the MFMAs of step SYNC_STEP - 1, not at the top of the body: steps
// 0 .. SYNC_STEP - 1 (point 0: 8 MFMAs) consume only what the wave already holds -- V_it, the fragments requested at
// steps 14, 15 of the iteration before -- and read only U_it, visible since the barrier before.  A wave goes from its
// transform burst and loop tail straight into those MFMAs and arrives at the barrier while the last of them executes
// (it cannot arrive before it has issued all eight; measured, DESIGN.md section 3.1 "Where the time goes").  Everything
// that needs the barrier comes behind it: the patch reads of raw_{it+1}, the reads of U_{it+1} (steps 14, 15) and the
// LDS-DMA refills.
constexpr int SYNC_STEP = 2;
static_assert(SYNC_STEP >= 1 && SYNC_STEP + 6 <= 16, "the twelve patch reads lie between the barrier and the burst");
static_assert(dma0_for(false) >= SYNC_STEP && dma0_for(false) + 8 <= 16 && dma0_for(true) >= SYNC_STEP && dma0_for(true) + 8 <= 16,
              "no LDS-DMA piece in front of the iteration's barrier");
static_assert(16 - PF >= SYNC_STEP, "the reads of U_{it+1} lie behind the iteration's barrier");
// LDS requests issued at the top of pinned step q of the point loop (see the kernel): always 2
// filter-fragment reads (step q+2 of this chunk, or step q-14 of the NEXT chunk on steps
// 14, 15), then 2 patch reads on the six steps from SYNC_STEP on (a wave reads 12 of its tiles' 16 patch pixels).
constexpr int lds_nr(int q) { return q >= SYNC_STEP && q < SYNC_STEP + 6 ? 2 : 0; }
constexpr int lds_n(int q) { return 2 + lds_nr(q); }
// How many LDS requests are younger than the last one step e's MFMAs need: the filter fragments of step e, requested
// PF steps earlier (for e < PF at steps 14, 15 of the iteration before: the count runs round the loop, and nothing
// between two bodies issues an LDS request that is still in flight at the next body's top; an extra one would only
// make the wait stricter).  The patch pixels are consumed by the burst behind step 15, which drains.
constexpr int lds_wait_count(int e) {
  // the fragments of step e were requested at step e-PF, before that step's patch reads
  int after = lds_nr((e - PF + 16) % 16);
  for (int q = e - PF + 1; q <= e; q++) after += lds_n((q + 16) % 16);
  return after > 15 ? 15 : after;
}
static_assert(lds_wait_count(0) == 4 && lds_wait_count(1) == 4, "steps 0, 1: two steps' fragment reads are younger");

// 8-byte LDS read at an absolute LDS byte address held in a register.  (`smem + offset` leaves a
// `v_add_u32 v, 0, v` per read in the loop -- the dynamic-LDS base is a symbol the optimizer does not
// fold -- so the fragment address registers carry the base themselves and are used as pointers.)
__device__ __forceinline__ f32x2 lds_read2(int addr) {
  return *(const __attribute__((address_space(3))) f32x2*)(size_t)(unsigned)addr;   // (size_t: the host pass parses this with 64-bit pointers)
}
struct TileCoord {
  int n, ty, tx;
};
__device__ __forceinline__ TileCoord decode_tile(int g) {
  TileCoord t;
  t.n = g / WINO_TILES;
  const int rem = g - t.n * WINO_TILES;
  t.ty = rem / 7;
  t.tx = rem - t.ty * 7;
  return t;
}

// Feature-map geometry of a launch: H x W outputs = ceil(H/2) x ceil(W/2) tiles per image, inside
// padded (H+2) x (W+2) tensors.  The reference's 14x14 stage is a compile-time specialisation
// (GEN = false: the divisions by 49 and 7 fold into multiplies); other sizes (ResNet's 56x56 and
// 28x28 stages) carry the numbers in the kernel arguments, with the two
// divisors as Granlund-Montgomery multipliers (FastDiv, wino_common.h).
struct Geo {
  int Hp, Wp;              // padded extents
  unsigned tiles, tiles_x;  // tiles per image, per tile row
  FastDiv d_tiles, d_tx;
};
template <bool GEN>
__device__ __forceinline__ TileCoord decode_tile_g(int g, const Geo& geo) {
  if (!GEN) return decode_tile(g);
  TileCoord t;
  t.n = (int)fastdiv((unsigned)g, geo.d_tiles);
  const unsigned rem = (unsigned)g - (unsigned)t.n * geo.tiles;
  t.ty = (int)fastdiv(rem, geo.d_tx);
  t.tx = (int)(rem - (unsigned)t.ty * geo.tiles_x);
  return t;
}

// Stream-K bookkeeping shared by the kernel and the host (T < 2^31, G <= 65535): logical
// workgroup l of G owns the iterations [sk_start(l), sk_start(l+1)) of T = q*G + rem, i.e.
// floor(l*T/G) = l*q + floor(l*rem/G) in 32-bit arithmetic.
__host__ __device__ inline unsigned sk_start(unsigned l, unsigned q, unsigned rem, unsigned G) {
  return l * q + l * rem / G;
}

// Which of a k-group's Gp tail ranges the workgroup at position j (consecutive positions share an XCD) runs.  Ranges
// of equal length q start at channel phase (q * range) mod nchunks, which repeats with period P = nchunks / gcd(q,
// nchunks); ranked by phase, rank r belongs to the ranges a + P * b with a = inv * r mod P.  Position j = r * copies +
// b, so that the workgroups of one XCD hold ranges of CONSECUTIVE phases: a filter chunk (k-block, channel chunk) one
// of them has fetched is what its neighbours ask for one iteration later -- an L2 hit instead of a fetch per
// workgroup.  P = 1, inv = 0, copies = Gp is the identity (unequal ranges, or a period that does not divide Gp).
__host__ __device__ inline int tail_range_of(int j, int P, int inv, int copies) {
  const int r = j / copies, b = j - r * copies;
  return (inv * r) % P + P * b;
}
__device__ __forceinline__ int tail_range_of_fast(int j, int P, int inv, int copies, FastDiv d_P, FastDiv d_copies) {
  const int r = (int)fastdiv((unsigned)j, d_copies), b = j - r * copies;
  const int ir = inv * r;
  return ir - (int)fastdiv((unsigned)ir, d_P) * P + P * b;
}

// The kernel's only argument.  The fields below the line are used by the epilogue alone: it
// re-reads them from the kernarg segment each time instead of keeping ~20 scalar registers
// (pointers + two buffer descriptors) alive across the main loop, which is out of SGPRs.
struct FusedParams {
  const float* in;
  const float* Uq;
  int N, C, K, relu, nTB;
  int ndp;                     // whole-item rounds: items / gridDim.x
  unsigned sk_q, sk_rem;       // tail, per k-group: (items % gridDim.x) / kp * C/8 = sk_q * (gridDim.x / kp) + sk_rem iterations
  int kp;                      // k-groups of the tail: K/64 (gridDim.x a multiple of it) or 1
  int Gp;                      // gridDim.x / kp: ranges (= positions) per k-group
  int ph_P, ph_inv, ph_copies; // which tail range the j-th position of a group runs (tail_range_of below)
  FastDiv d_kp, d_P, d_copies; // the three divisors as multipliers: a runtime integer division is ~40 instructions on
                               // this machine, and the first cut of the k-groups paid five of them in the prologue and
                               // five in every epilogue (+0.7 us on a 40 us launch)
  Geo geo;                     // feature-map geometry (read by the GEN = true build only)
  // ---- epilogue only ----
  const float* bnBias;
  const float* bnScale;
  float* out;
  float* slabs;
  unsigned* tickets;
  unsigned* err;               // host-visible word, set when a ticket is drawn on a counter that was not zero at launch
  unsigned long long* dbg;     // diagnostic builds only (PROBE_CLOCK, PROBE_PHASES, PROBE_TIMELINE): where the stamps go
};
// The arguments of the RES = true kernels: the plain ones, then the residual (padded like `out`; its ring is not read).
// The residual goes behind every existing field in a struct of its own rather than into FusedParams, so that the plain
// kernels' argument segment -- and the offsets of the implicit arguments the runtime places behind it -- stay as they
// were: their code is byte-identical with or without this form.
struct FusedResParams : FusedParams {
  const float* res;
};
template <bool RES>
using FusedArgs = std::conditional_t<RES, FusedResParams, FusedParams>;
// the epilogue forms of the two 3x3 kernels (their last template argument)
constexpr int EPI_PLAIN = 0, EPI_RES = 1, EPI_POOL = 2;

// Host side: the work layout fields above (ndp ... d_copies) of `items` items of p.C / BC chunk iterations on a grid
// of G logical workgroups: items / G whole-item rounds, the rest a stream-K tail.
// k-groups of the tail: K/64 when the grid is a multiple of it -- the items are K/64 per tile block, so the tail's
// item count is then a multiple too -- else 1 (one item-major list).
// Phase order of a k-group's tail ranges (tail_range_of): for Gp equal ranges of q iterations the period P = nchunks /
// gcd(q, nchunks) of their channel phases, the inverse of q / gcd modulo P, and Gp / P; the identity otherwise.
inline void fused_work_layout(FusedParams& p, long long items, int G) {
  const int nchunks = p.C / BC, kblk = p.K / KB;
  const int kp = kblk <= 1 || (G % kblk) != 0 ? 1 : kblk;
  const long long Tg = (items % G) * nchunks / kp, Gp = G / kp, q = Tg / Gp, rem = Tg % Gp;
  p.ndp = (int)(items / G);
  p.sk_q = (unsigned)q;
  p.sk_rem = (unsigned)rem;
  p.kp = kp;
  p.Gp = (int)Gp;
  p.ph_P = 1, p.ph_inv = 0, p.ph_copies = (int)Gp;
  if (rem == 0 && q > 0) {
    long long a = q % nchunks, b = nchunks;
    while (a) { const long long t = b % a; b = a; a = t; }
    const long long g = b, P = nchunks / g;
    if (P > 1 && Gp % P == 0) {
      const long long qq = (q / g) % P;
      for (long long x = 1; x < P; x++)
        if ((qq * x) % P == 1) { p.ph_P = (int)P; p.ph_inv = (int)x; p.ph_copies = (int)(Gp / P); break; }
    }
  }
  p.d_kp = make_fastdiv((unsigned)kp);
  p.d_P = make_fastdiv((unsigned)p.ph_P);
  p.d_copies = make_fastdiv((unsigned)p.ph_copies);
}

// The clock the chip holds inside the product kernel: workgroup 0 of every launch stores {s_memtime,
// s_memrealtime} here at its entry and at its exit (four 8-byte stores per launch from one lane; nothing
// reads them on the device).  wino_diag_last_clock() copies them out: bench.py takes the clock OF its timed
// launches from the last one of the burst instead of from a separate stamped build run afterwards.
__device__ unsigned long long wino_clk_slot_3x3[4];

// TAIL = the launch has a stream-K tail (any partial segment at all).  Launches of whole items only -- every
// shape whose items fit or divide the grid -- compile the hand-off out of the epilogue: 128 channels N = 128
// 40.1 -> 39.6 us, 256 channels N = 64 71.7 -> 71.0.  (Tried for the launches WITH a tail in the same step: the
// gather with two slabs in flight and the accumulators re-zeroed at the end of the epilogue to make room -- no
// gain at small batches, where an item has up to 8 segments, +0.8..1.2 % at 256 channels N = 96 / 256.)
//
// RES = the residual epilogue (the second 3x3 of a ResNet basic block): out = act(scale*conv + bias + res), res padded
// like out.  BN is applied before the LDS transpose as in the plain form; the ReLU waits until the residual's 16 bytes,
// loaded at the store's own offset, have been added.  Each residual element is read only by the lane that stores that
// offset, before its store, so out may be res (in place).  RES = false compiles exactly the plain kernel.
//
// POOL = the pooled epilogue (a VGG layer that is followed by MaxPool2d(2, 2)): out = maxpool2x2_s2(act(scale*conv +
// bias)), [N][H/2+2][W/2+2][K] with its zero ring.  An F(2x2) tile IS a pooling window: after the gather, BN and the
// ReLU its four outputs sit in one lane (y[r][cb][0..3]), so the max is taken in-lane and one value per (tile,
// out-channel) goes through the LDS transpose -- 2 KB per wave and two 16-byte store rounds where the plain form has
// 8 KB and eight.  Everything up to the finalize, the launch plan included, is the plain layer's; only the ring pass
// and the store addressing use the pooled geometry.  Tiles of a clipped last tile row / column (odd H or W) are
// dropped whole: floor, as torch pools.
//
// The epilogue is one template argument, EPI = EPI_PLAIN / EPI_RES / EPI_POOL (0 / 1 / 2: `false` and `true` still name
// the plain and the residual form).  EPI_PLAIN and EPI_RES compile exactly what RES = false / true compiled.
template <int ABLATE, bool GEN = false, bool TAIL = true, int EPI = EPI_PLAIN>
__global__ void __launch_bounds__(NTHREADS, 2)
wino_f2_fused_kernel(const FusedArgs<EPI == EPI_RES> prm) {
  static_assert(EPI == EPI_PLAIN || EPI == EPI_RES || EPI == EPI_POOL, "epilogue form");
  constexpr bool RES = EPI == EPI_RES, POOL = EPI == EPI_POOL;
  constexpr int DMA0 = dma0_for(GEN);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const float* in = prm.in;
  const float* Uq = prm.Uq;
  asm volatile("" : "+s"(in), "+s"(Uq));
  const int N = prm.N, C = prm.C, K = prm.K;
  const unsigned sk_q = prm.sk_q, sk_rem = prm.sk_rem;
  const int ndp = prm.ndp;

  // XCD-aware block -> logical workgroup: blocks b and b+8 share an XCD (its L2), so consecutive
  // logical workgroups -- which walk consecutive items, i.e. the K/64 k-blocks that read the same
  // input tiles -- are placed on the same XCD: XCD x = blockIdx % 8 gets the logical range that
  // starts at x*(G/8) + min(x, G%8).
  const int KBLK = K >> 6;
  const int nchunks = C / BC;
  const int G = gridDim.x;
  const int lg = (int)(blockIdx.x & 7) * (G >> 3) + ((int)(blockIdx.x & 7) < (G & 7) ? (int)(blockIdx.x & 7) : (G & 7)) +
                 (int)(blockIdx.x >> 3);
  if (ABLATE & PROBE_TIMELINE) {
    if (threadIdx.x == 0) {
      prm.dbg[(size_t)lg * TL_WORDS + TL_ENTRY] = __builtin_amdgcn_s_memrealtime();
      prm.dbg[(size_t)lg * TL_WORDS + TL3_ENTRY_CYC] = __builtin_amdgcn_s_memtime();
    }
  }
  if (ABLATE == PROBE_OFF && blockIdx.x == 0 && threadIdx.x == 0) {
    wino_clk_slot_3x3[0] = __builtin_amdgcn_s_memtime();
    wino_clk_slot_3x3[1] = __builtin_amdgcn_s_memrealtime();
  }
  auto clk_exit = [&]() {
    if (ABLATE == PROBE_OFF && blockIdx.x == 0 && threadIdx.x == 0) {
      wino_clk_slot_3x3[2] = __builtin_amdgcn_s_memtime();
      wino_clk_slot_3x3[3] = __builtin_amdgcn_s_memrealtime();
    }
  };
  // tail: items ndp*G .. ; then the rounds.  The tail is cut PER OUT-CHANNEL BLOCK (kp = K/64 groups when the grid
  // is a multiple of it): group k = lg % kp owns the tail items of k-block k (one per tile block, walked in
  // tile-block order: item tail_item0 + kp*j + k), (sk_q * Gp + sk_rem) chunk iterations cut into Gp = G / kp equal
  // ranges, range lp = lg / kp.  The kp workgroups with the same lp -- neighbours on one XCD -- then walk the SAME
  // tile blocks and channel chunks at the same time and share every patch line in the XCD's L2, exactly as the
  // whole-item rounds do.  (Round 2 cut one item-major list into G ranges: the k-blocks of a tile block sat at
  // different channel phases, every one of them fetched the patches for itself: HBM-side fetch 164 MB per launch
  // at the reference's 256 channels, N = 128, against 38 MB compulsory.)  kp = 1 is that old scheme.
  const int tail_item0 = ndp * G;
  const int kpg = prm.kp, Gp = prm.Gp;
  const int lpos = __builtin_amdgcn_readfirstlane((int)fastdiv((unsigned)lg, prm.d_kp)), grp = lg - lpos * kpg;
  const int lp = __builtin_amdgcn_readfirstlane(tail_range_of_fast(lpos, prm.ph_P, prm.ph_inv, prm.ph_copies, prm.d_P, prm.d_copies));   // the group's tail range this workgroup runs
  const unsigned t_begin = __builtin_amdgcn_readfirstlane(sk_start(lp, sk_q, sk_rem, Gp));
  const int Lt = (int)(__builtin_amdgcn_readfirstlane(sk_start(lp + 1, sk_q, sk_rem, Gp)) - t_begin);   // tail iterations of this workgroup
  const int L = Lt + ndp * nchunks;                                     // all its chunk iterations

  // ---- ring pass: the output's zero ring (the next 3x3 layer's padding, Kernel128_winograd.cu:
  // 163,243) is written here, once per launch, as a flat list of 16-byte units -- N images x 60
  // ring pixels x K/4 units -- split evenly over the workgroups; the stores are fully coalesced
  // and drain while the first LDS-DMA pieces are in flight.  (Per tile in the epilogue, the ring
  // cost more than the tiles' own stores: sparse predicated stores and their address arithmetic.)
  auto ring_pass = [&]() {
    if (ABLATE & PROBE_NO_STORE) return;
    // (POOL: the ring of the pooled output, (H/2 + 2) x (W/2 + 2))
    const unsigned Hi = GEN ? (unsigned)prm.geo.Hp : (unsigned)WINO_HW, Wi = GEN ? (unsigned)prm.geo.Wp : (unsigned)WINO_HW;
    const unsigned Hp = POOL ? (Hi - 2u) / 2u + 2u : Hi, Wp = POOL ? (Wi - 2u) / 2u + 2u : Wi;
    const unsigned rpx = 2u * Wp + 2u * (Hp - 2u);               // ring pixels per image (60 at 16 x 16)
    const unsigned upp = (unsigned)K >> 2;                       // units per ring pixel
    const unsigned long long U = (unsigned long long)N * rpx * upp;
    const unsigned u_begin = (unsigned)(U * (unsigned)lg / (unsigned)G);
    const unsigned u_end = (unsigned)(U * ((unsigned)lg + 1u) / (unsigned)G);
    const auto rsrc_ring = make_rsrc(prm.out, (unsigned)((size_t)N * Hp * Wp * K * sizeof(float)));
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    for (unsigned u = u_begin + threadIdx.x; u < u_end; u += NTHREADS) {
      const unsigned pid = u / upp, unit = u - pid * upp;
      const unsigned n = pid / rpx, q = pid - n * rpx;
      // q: [0, Wp) row 0, [Wp, 2Wp) the last row, then column 0 and the last column of rows 1..Hp-2
      const unsigned y = q < Wp ? 0u : q < 2 * Wp ? Hp - 1 : q < 2 * Wp + Hp - 2 ? q - 2 * Wp + 1 : q - 2 * Wp - (Hp - 2) + 1;
      const unsigned x = q < Wp ? q : q < 2 * Wp ? q - Wp : q < 2 * Wp + Hp - 2 ? 0u : Wp - 1;
      buf_store16(zero4, rsrc_ring, (((n * Hp + y) * Wp + x) * (unsigned)K + unit * 4u) * (unsigned)sizeof(float), 0);
    }
  };
  if (L <= 0) {   // more workgroups than iterations: this one only has its share of the ring
    ring_pass();
    clk_exit();
    return;
  }

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  // Point split: wave (wt, ph) owns 16 tiles x ALL 64 out-channels x 8 of the 16 Winograd points -- rows
  // i = 2 ph, 2 ph + 1 of the 4 x 4 point grid.  The two waves of a tile block then share no B^T d B
  // work (with 16 points per wave both computed the same V): a wave needs 3 of the 4 patch rows (12
  // reads) and 16 packed adds per iteration instead of 16 reads and 32 adds.  Timing-only ablation of
  // exactly that (half the adds, 12 reads): 124.3 -> 116.7 us at 256 channels, 41.9 -> 39.3 at 128.
  // The price is an exchange of partial A^T m A sums between the pair in the epilogue, after which
  // wave (wt, ph) owns out-channels [32 ph, 32 ph + 32) of its 16 tiles exactly as wave (wt, wk) did.
  const int wt = w >> 1;  // which 16-tile block of the 64
  const int ph = w & 1;   // which half of the point rows; after the epilogue exchange: which 32-channel half

  const unsigned u_off = lane * 16;
  const unsigned u_chunk_stride = (unsigned)(KBLK * U_CHUNK_FLOATS * sizeof(float));
  // buffer descriptors (wave-uniform): everything loop-variant goes into the scalar offset
  const auto rsrc_in = make_rsrc(in, (unsigned)((size_t)N * (GEN ? prm.geo.Hp * prm.geo.Wp : WINO_HW * WINO_HW) * C * sizeof(float)));
  const auto rsrc_u = make_rsrc(Uq, (unsigned)((size_t)16 * C * K * sizeof(float)));

  // ---- fragment read addresses (launch invariant) -------------------------------
  const int t16 = lane & 15, h = lane >> 4;
  // A: tile row tl = wt*16 + t16; 8-byte quarter h holds channels 2h, 2h+1 of the chunk
  const int lds0 = (int)(unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;   // absolute LDS address of smem[0]
  const int a_base = lds0 + (wt * 16 + t16) * 512 + ((h ^ (((t16 >> 3) & 1) << 1)) << 3);
  const int a_sw = t16 & 7;
  // Fragment reads must stay plain ds_read_b64: that form banks on 64 dwords, for which the
  // XOR layouts are conflict-free.  hipcc would fuse two reads off one base register into
  // ds_read2_b64 / ds_read2st64_b64, which bank on 32 dwords (2-way conflicts here, half the
  // bytes per clock).  Hiding how the bases relate (empty asm) prevents the fusion; pixels px
  // and px+8 share a base register but are never read in the same pinned step.
  // The three patch rows R0, R1, R2 this wave reads are (d0, d2, d1) for ph = 0 and (d2, d1, d3) for
  // ph = 1: then B^T d, rows 2 ph and 2 ph + 1, is  R0 - R1  and  R1 + s2 * R2  with s2 = +1 / -1 for
  // both halves (one code path).  One address register per pixel (12; they point into R0, and the raw stage is a
  // compile-time offset of each read: see body()).
  int a_adr[3][4];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int row = ph ? (k == 0 ? 2 : k == 1 ? 1 : 3) : (k == 0 ? 0 : k == 1 ? 2 : 1);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int px = 4 * row + j;
      a_adr[k][j] = a_base + (((px & 7) ^ a_sw) << 5) + ((px >> 3) << 8);
    }
  }
  // B: logical column block cb' of this wave is out-channel block cb' ^ 2 ph of the item (k_local =
  // (cb' ^ 2 ph) * 16 + t16): cb' = 0, 1 are the two blocks the wave keeps after the epilogue exchange,
  // cb' = 2, 3 the two it hands to its partner -- compile-time indices either way.  The byte offset of
  // the wave's first point (8 ph) inside a filter stage is folded in.
  int b_base[4];
#pragma unroll
  for (int cb = 0; cb < 4; cb++) {
    const int kl = (cb ^ (2 * ph)) * 16 + t16;
    b_base[cb] = lds0 + N_RSTAGE * RAW_BYTES + ph * (8 * 2048) + kl * 32 + ((h ^ (((kl >> 3) & 1) << 1)) << 3);
  }
  asm volatile("" : "+v"(b_base[1]), "+v"(b_base[2]), "+v"(b_base[3]));

  // B^T d B pieces (d, tmp, v are [row i][col j] = index 4i + j; Winograd point e = 4i + j), on
  // channel pairs (v_pk_add_f32)
  typedef f32x2 P2;
  auto sub2 = [](const P2& a, const P2& b) { return a - b; };
  auto add2 = [](const P2& a, const P2& b) { return a + b; };
  const float s2f = ph ? -1.f : 1.f;
  const P2 s2 = {s2f, s2f};
  // d[k*4 + j] = patch row R_k, column j;  tmp[i'*4 + j] = (B^T d) row 2 ph + i', column j;
  // v[p], p = 4 i' + j = the wave's point p (Winograd point e = 8 ph + p)
  auto tmp_col = [&](P2* tmp, const P2* d, int j) {  // B^T d, column j, the wave's two rows
    tmp[0 * 4 + j] = sub2(d[0 * 4 + j], d[1 * 4 + j]);
    tmp[1 * 4 + j] = d[1 * 4 + j] + s2 * d[2 * 4 + j];
  };
  auto v_point = [&](P2* v, const P2* tmp, int e) {  // (B^T d) B, point e (0..7)
    const int i = e >> 2, j = e & 3;
    if (j == 0) v[e] = sub2(tmp[i * 4 + 0], tmp[i * 4 + 2]);
    if (j == 1) v[e] = add2(tmp[i * 4 + 1], tmp[i * 4 + 2]);
    if (j == 2) v[e] = sub2(tmp[i * 4 + 2], tmp[i * 4 + 1]);
    if (j == 3) v[e] = sub2(tmp[i * 4 + 1], tmp[i * 4 + 3]);
  };

  unsigned long long st_wait = 0, st_comp = 0, st_epi = 0, st_prev = 0, st_span = 0, st_restart = 0;   // ABLATE & PROBE_PHASES: phase stamps
  unsigned long long st_ph[4] = {0, 0, 0, 0};   // epilogue phases: barrier, A^T m A, slab+ticket, gather+finalize
  unsigned long long st_sub[PH_NSUB] = {0, 0, 0, 0, 0, 0};   // ... and the parts of A^T m A and of gather+finalize (PH_SUB0 + PHS_*)
  auto stamp = [&]() -> unsigned long long {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
  };

  // Opaque pointer to the kernel's own arguments (constant address space: scalar loads).  The rare
  // paths below (tile-block switch of the DMA stream, epilogue) re-read what they need through it
  // instead of keeping those scalars alive across the main loop, which is out of SGPRs.
  typedef const __attribute__((address_space(4))) FusedParams* KernargPtr;
  auto kernarg = []() {
    KernargPtr kp = (KernargPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kp));
    return kp;
  };
  auto load_geo = [](KernargPtr kp) {   // member-wise: the struct lives in the constant address space
    Geo g;
    g.Hp = kp->geo.Hp; g.Wp = kp->geo.Wp; g.tiles = kp->geo.tiles; g.tiles_x = kp->geo.tiles_x;
    g.d_tiles.m = kp->geo.d_tiles.m; g.d_tiles.l = kp->geo.d_tiles.l;
    g.d_tx.m = kp->geo.d_tx.m; g.d_tx.l = kp->geo.d_tx.l;
    return g;
  };

  // ---- the DMA stream: walks (item, chunk) linearly, two iterations ahead of the MFMAs ------
  // raw stage layout: [tile 0..63][unit' 0..31] of 16 B; unit' = px'*2 + half'.
  // LDS unit (t, px', half') holds pixel px = px' ^ (t&7), channel half = half' ^ bit3(t).
  // wave-instruction q = 8*j + w (j = 0..3) covers tiles 2q, 2q+1.
  // (byte offsets from `in`, 32-bit: the DMA then uses the scalar-base + vector-offset address
  //  form and advancing to the next chunk is a scalar add instead of a 64-bit VALU add per piece)
  unsigned raw_off[4];        // per-lane source offsets of the DMA stream's tile block
  unsigned d_soff_raw = 0;    // + chunk * 32 B
  unsigned d_soff_u = 0;      // filter chunk of (k block, chunk), this wave's 1-KiB column
  // The stream is EVENT DRIVEN.  An advance is normally two scalar adds (the next chunk of the same item); every
  // d_run-th one is an event instead: the stream changes item (dma_set_item: new offsets, and new per-lane offsets when
  // the tile block changes) or it has issued the whole range and stands on its last chunk from there on -- the two
  // steps become 0, so the advance stays unconditional.  The main loop runs to the next event without asking; what an
  // event needs (item, tail iterations, advances left, tile block) waits in the lanes of ONE VGPR (ws_vg: a scalar per
  // lane, v_writelane / v_readlane in the event code), as it will be AT the event: none of it costs the loop a scalar
  // register or an instruction, and the epilogues, which are at the register budget, one VGPR.
  unsigned d_step_raw = (unsigned)(BC * sizeof(float)), d_step_u = u_chunk_stride;   // what an advance adds
  int d_run = 0;              // advances up to and including the next event
  int ws_vg = 0;
  // lanes of ws_vg
  typedef std::integral_constant<int, 0> WS_D_ITEM; typedef std::integral_constant<int, 1> WS_D_TAIL;
  typedef std::integral_constant<int, 2> WS_D_LEFT; typedef std::integral_constant<int, 3> WS_D_TB;
  typedef std::integral_constant<int, 4> WS_D_RUN;  typedef std::integral_constant<int, 5> WS_C_RUN;
  typedef std::integral_constant<int, 6> WS_C_LEFT;
  // a whole-first range (below): its tail segment's item, first chunk and length (WS_WF_LT = -1: not such a range)
  typedef std::integral_constant<int, 7> WS_T_ITEM; typedef std::integral_constant<int, 8> WS_T_CHUNK;
  typedef std::integral_constant<int, 9> WS_WF_LT;
  // (v_writelane_b32 has no builtin; volatile asm also keeps the scalars in their lanes: the compiler cannot look through it)
  auto ws_put = [&ws_vg](auto slot, int val) { asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(ws_vg) : "s"(val), "n"(decltype(slot)::value)); };
  auto ws_get = [&ws_vg](auto slot) { return __builtin_amdgcn_readlane(ws_vg, decltype(slot)::value); };
  ws_put(WS_D_TB{}, -1);
  constexpr int D_NEVER = 0x7fffffff;
  auto dma_set_item = [&](int item, int chunk) {   // wave-uniform; the per-lane part only when the tile block changes
    const int tb = item / KBLK, kb = item - tb * KBLK;
    if (tb != ws_get(WS_D_TB{})) {
      ws_put(WS_D_TB{}, tb);
      KernargPtr kp = kernarg();
      const Geo geo = load_geo(kp);
      const int Wp = GEN ? geo.Wp : WINO_HW, Hp = GEN ? geo.Hp : WINO_HW;
      const int C = kp->C, totalTiles = kp->N * (GEN ? (int)geo.tiles : WINO_TILES);
      const int up = lane & 31;
      const int pxp = up >> 1, halfp = up & 1;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int tl = 16 * j + 2 * w + (lane >> 5);
        const int px = pxp ^ (tl & 7);
        const int half = halfp ^ ((tl >> 3) & 1);
        int g = tb * TB + tl;
        g = g < totalTiles ? g : totalTiles - 1;  // clamp: padded rows read a valid tile
        const TileCoord tc = decode_tile_g<GEN>(g, geo);
        const int y = 2 * tc.ty + (px >> 2), x = 2 * tc.tx + (px & 3);
        raw_off[j] = (unsigned)((((size_t)(tc.n * Hp + y) * Wp + x) * C + half * 4) * sizeof(float));
      }
    }
    // (opaque: the loop carries these four registers as they are, no copy of them goes round it)
    asm volatile("" : "+v"(raw_off[0]), "+v"(raw_off[1]), "+v"(raw_off[2]), "+v"(raw_off[3]));
    d_soff_raw = __builtin_amdgcn_readfirstlane((unsigned)(chunk * (BC * sizeof(float))));
    d_soff_u = __builtin_amdgcn_readfirstlane((unsigned)((kb * U_CHUNK_FLOATS + w * 256) * sizeof(float)) + chunk * u_chunk_stride);
  };
  // ("+s": pins the loop-carried scalars to SGPRs.  Short of SGPRs, the compiler otherwise keeps
  //  one of them in a VGPR and wraps every LDS-DMA that uses it in a waterfall loop.)
  auto pin_dma_state = [&]() {
    d_run = __builtin_amdgcn_readfirstlane(d_run);
    asm volatile("" : "+s"(d_soff_raw), "+s"(d_soff_u), "+s"(d_step_raw), "+s"(d_step_u), "+s"(d_run));
  };
  auto dma_stand = [&]() {   // the range is issued: every later advance adds nothing
    d_step_raw = 0;
    d_step_u = 0;
    d_run = D_NEVER;
  };
  // The stream stands on (item, chunk) with `tail` tail iterations (this one included) and `left` advances still to
  // make: how far it runs on plain advances, and its state at the event that ends the run.
  auto dma_plan = [&](int item, int chunk, int tail, int left) {
    const int nch = kernarg()->C / BC;
    const int in_item = nch - 1 - chunk;
    const int plain = tail > 0 && tail - 1 < in_item ? tail - 1 : in_item;   // ... before the item or the tail ends
    if (left <= plain) {   // the range ends first
      if (left == 0) dma_stand();
      else d_run = left;
      left = -1;
    } else {               // the advance after them changes item
      d_run = plain + 1;
      left -= plain + 1;
      if (tail > 0) tail -= plain;
    }
    ws_put(WS_D_ITEM{}, item), ws_put(WS_D_TAIL{}, tail), ws_put(WS_D_LEFT{}, left);
  };
  auto dma_event = [&]() {   // d_run has run out
    int item = ws_get(WS_D_ITEM{}), tail = ws_get(WS_D_TAIL{});
    const int left = ws_get(WS_D_LEFT{});
    if (left < 0) {
      dma_stand();
    } else {
      int chunk = 0;
      if (TAIL && left + 1 == ws_get(WS_WF_LT{})) {      // whole-first range, rounds issued: its tail segment is what is left
        item = ws_get(WS_T_ITEM{}), chunk = ws_get(WS_T_CHUNK{}), tail = left + 1;
      } else if (tail > 0 && --tail == 0) item = lg;     // the tail range is issued: on to the whole items
      else item += tail > 0 ? kernarg()->kp : G;         // the next tail item of this k-group / round
      dma_set_item(item, chunk);                         // (it overwrites the two offsets the plain advance has just stepped)
      dma_plan(item, chunk, tail, left);
    }
    pin_dma_state();
  };
  auto dma_advance = [&]() {   // one advance outside the main loop (prologue)
    d_soff_raw += d_step_raw;
    d_soff_u += d_step_u;
    if (--d_run == 0) dma_event();
    pin_dma_state();
  };
  // LDS map: [R0 32K][R1 32K][U0 32K][U1 32K][U2 32K]; R = raw 4x4 patches, U = filter chunk.
  // Both DMA streams run TWO iterations ahead of the MFMAs, across item boundaries:
  //  * raw_{i+1} is consumed one iteration early: while the MFMAs of iteration i run (operands:
  //    V_i in registers, U_i in LDS) the wave reads raw_{i+1} from LDS and transforms it into
  //    V_{i+1}, in place over the V registers of points that have already retired, so the
  //    matrix pipe never waits for the input transform (2 raw stages suffice);
  //  * U_{i+1} is already visible during iteration i (3 filter stages), so the first filter
  //    fragments of iteration i+1 are requested at steps 14, 15 of iteration i, and iteration i+1 runs
  //    point 0 (steps 0, 1: 8 MFMAs) straight from them and from V_{i+1}, IN FRONT of its vmcnt(0) + barrier
  //    (SYNC_STEP): only what follows needs raw_{i+2} / U_{i+2} landed and the refilled stages free.
  auto issue_raw1 = [&](int rstage, int j) {  // one 1-KiB piece
    if (ABLATE & PROBE_NO_DMA_A) return;
    dma16_buf(rsrc_in, raw_off[j], d_soff_raw, smem + rstage * RAW_BYTES + (8 * j + w) * 1024);
  };
  auto issue_u1 = [&](int ustage, int j) {
    if (ABLATE & PROBE_NO_DMA_B) return;
    dma16_buf(rsrc_u, u_off, d_soff_u + j * 8192,
              smem + N_RSTAGE * RAW_BYTES + ustage * U_BYTES + (8 * j + w) * 1024);
  };

  // ---- the compute stream's position --------------------------------------------
  // (readfirstlane: the divisions run on the vector unit; without it the walkers' scalar state --
  //  and with it the LDS-DMA scalar offsets -- would be treated as divergent)
  // Order of the range.  A tail range that lies inside ONE item (one tail segment) runs its whole-item rounds first and
  // that segment last ("whole-first"); every other range runs its tail first.  The one-segment workgroup is then its tail
  // item's natural last arriver -- the other segments' slabs and tickets are a whole item old when it gets there -- and
  // finishes the item from its registers (epilogue(), "the peek").  Wave-uniform, settled here once; both walkers find
  // the tail segment's start in three lanes of ws_vg when the rounds run out.
  // (TAIL = false spells the start of the range as it always did: those builds keep their code byte for byte)
  int t_item = 0, t_chunk = 0;
  bool whole_first = false;
  if (TAIL) {
    t_item = __builtin_amdgcn_readfirstlane(tail_item0 + (int)(t_begin / (unsigned)nchunks) * kpg + grp);
    t_chunk = __builtin_amdgcn_readfirstlane((int)(t_begin % (unsigned)nchunks));
    whole_first = ndp > 0 && Lt > 0 && t_chunk + Lt <= nchunks;
    ws_put(WS_T_ITEM{}, t_item), ws_put(WS_T_CHUNK{}, t_chunk), ws_put(WS_WF_LT{}, whole_first ? Lt : -1);
  }
  const bool tail_first = Lt > 0 && !whole_first;
  const int tail0 = TAIL ? (tail_first ? Lt : 0) : Lt;
  int c_tail_vg = tail0;           // tail iterations still to compute (whole-first: none until the rounds are done)
  // (The current item and the kind of the current segment are looked at by the epilogue and the segment switch
  //  only: they ride through the main loop in VGPRs, like pend_vg below, and are read back with readfirstlane
  //  where they are needed.  The loop has no SGPR to spare.)
  int c_item_vg = TAIL ? __builtin_amdgcn_readfirstlane(tail_first ? t_item : lg)
                       : __builtin_amdgcn_readfirstlane(Lt > 0 ? tail_item0 + (int)(t_begin / (unsigned)nchunks) * kpg + grp : lg);
  int c_chunk = TAIL ? __builtin_amdgcn_readfirstlane(tail_first ? t_chunk : 0)
                     : __builtin_amdgcn_readfirstlane(Lt > 0 ? (int)(t_begin % (unsigned)nchunks) : 0);
  int seg_kind_vg = 0;             // bit 1: the current segment starts its item, bit 0: it is the whole item
  // a partial segment whose ticket is drawn in the next epilogue (-1: none).  Parked in a VGPR across the
  // main loop ("+v"; read back with readfirstlane in the epilogue): the loop has no SGPR to spare -- as a
  // scalar it pushed a buffer descriptor into VGPR lanes, four v_readlane per iteration.
  int pend_vg = -1;
  asm volatile("" : "+v"(pend_vg));

  f32x4 acc[8][4];   // [the wave's point p][logical column block cb']
#pragma unroll
  for (int e = 0; e < 8; e++)
#pragma unroll
    for (int cb = 0; cb < 4; cb++) acc[e][cb] = (f32x4){0.f, 0.f, 0.f, 0.f};
  P2 v[8];           // V_it (the wave's 8 points) at the top of iteration `it`; rewritten in place with V_{it+1}
  // A pinned step s = 0..15 of an iteration is (point p = s >> 1, column-block pair s & 1): 4 MFMAs.
  f32x2 bfn[PF][2];  // filter fragments of steps 0..PF-1 of the next iteration (requested at steps 14, 15; consumed in front of its barrier)

  // ---- prologue: iterations 0 and 1 in flight; V_0 and the first fragments un-pipelined -----
  dma_set_item(c_item_vg, c_chunk);
  dma_plan(c_item_vg, c_chunk, tail0, L - 1);   // L - 1 advances take the stream to the range's last chunk
  pin_dma_state();
  asm volatile("" : "+v"(c_item_vg));
#pragma unroll
  for (int j = 0; j < 4; j++) issue_raw1(0, j);
#pragma unroll
  for (int j = 0; j < 4; j++) issue_u1(0, j);
  // The DMA walker never leaves this workgroup's range: it stops on the last chunk (an advance past it adds
  // nothing), and the last two iterations of the range fetch that chunk again into stages nobody reads (see body()).
  if ((ABLATE & PROBE_TIMELINE) && tid == 0) prm.dbg[(size_t)lg * TL_WORDS + TL3_STAGE_REQ] = __builtin_amdgcn_s_memrealtime();   // first stage requested
  dma_advance();
  ring_pass();   // in the shadow of the first pieces' flight
  if (!(ABLATE & PROBE_NO_SYNC)) {
    wait_vmem_all();
    __syncthreads();
  }
  if ((ABLATE & PROBE_TIMELINE) && tid == 0) prm.dbg[(size_t)lg * TL_WORDS + TL3_STAGE_IN] = __builtin_amdgcn_s_memrealtime();   // ... and landed
  if (L > 1) {
#pragma unroll
    for (int j = 0; j < 4; j++) issue_raw1(1, j);
#pragma unroll
    for (int j = 0; j < 4; j++) issue_u1(1, j);
    dma_advance();
  }
  {
    P2 d[12];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int j = 0; j < 4; j++) d[k * 4 + j] = lds_read2(a_adr[k][j]);
    P2 tmp[8];
#pragma unroll
    for (int j = 0; j < 4; j++) tmp_col(tmp, d, j);
#pragma unroll
    for (int e = 0; e < 8; e++) v_point(v, tmp, e);
#pragma unroll
    for (int e = 0; e < PF; e++) {   // steps 0, 1: point 0, column-block pairs 0 and 1
      bfn[e][0] = lds_read2(b_base[2 * (e & 1) + 0] + (e >> 1) * 2048);
      bfn[e][1] = lds_read2(b_base[2 * (e & 1) + 1] + (e >> 1) * 2048);
    }
  }
  if (ABLATE & PROBE_TIMELINE) {
    if (tid == 0) prm.dbg[(size_t)lg * TL_WORDS + TL_FIRST] = __builtin_amdgcn_s_memrealtime();
  }
  if (ABLATE & PROBE_CLOCK) {  // diagnostic build only: in-kernel clock = d(s_memtime) / d(s_memrealtime)
    // The start stamps go to memory at once: kept in SGPRs across the main loop (which has none to
    // spare) they pushed loop-carried scalars into VGPRs and the build ran 15 % slower than the
    // product kernel -- not a faithful probe of its clock.
    if (tid == 0) {
      prm.dbg[(size_t)lg * CLK_WORDS + CLK_BEGIN_CYC] = __builtin_amdgcn_s_memtime();
      prm.dbg[(size_t)lg * CLK_WORDS + CLK_BEGIN_RT] = __builtin_amdgcn_s_memrealtime();
    }
  }

  // One pipeline step = iteration `it`.  The body exists twice, once per parity of `it` (par_c): iteration `it`
  // reads raw_{it+1} from R[(it + 1) & 1], which is then a compile-time offset (ROFF) of the patch reads -- the
  // twelve address registers a_adr[][] stay on R0 (flipping bit 15 of each after every iteration instead cost
  // twelve v_xor per iteration).  The filter stage (it % 3) is a run-time offset added to the fragment base
  // registers, the DMA destinations are scalar.
  // The schedule inside is pinned with sched_barrier(0): left alone, hipcc sinks every
  // ds_read to just before its first use and the wave eats one LDS latency per point.
  int ub_cur[4], ub_nxt[4];   // b_base[] + the byte offset of filter stage it % 3 / (it + 1) % 3
#pragma unroll
  for (int cb = 0; cb < 4; cb++) {
    ub_cur[cb] = b_base[cb];
    ub_nxt[cb] = b_base[cb] + U_BYTES;
  }
  auto body = [&](auto par_c, int rs_dma, int us_dma) {
    constexpr int ROFF = decltype(par_c)::value ? 0 : RAW_BYTES;
    // The iteration's synchronisation point, behind the MFMAs of step SYNC_STEP - 1 (see SYNC_STEP).  A bare barrier
    // behind the wave's own vmcnt(0): __syncthreads() would also drain lgkmcnt, and with it the fragment requests
    // steps 0 and 1 have just made.  What it orders: the LDS-DMA writes of raw_{it+1} / U_{it+1} (every wave's have
    // landed) before the reads below it, and every wave's reads of raw_it (iteration it - 1) and U_{it-1} before the
    // refills of R[it & 1] and U[(it + 2) % 3] from step DMA0 on.
    auto sync_point = [&]() {
      if (ABLATE & PROBE_PHASES) { const unsigned long long t = stamp(); if (st_prev) st_comp += t - st_prev; st_prev = t; }
      if (!(ABLATE & PROBE_NO_SYNC)) {
        wait_vmem_all();   // my DMA pieces of raw_{it+1} and U_{it+1} have landed
        __builtin_amdgcn_s_barrier();   // everyone's have; everyone is done with the stages refilled below
        asm volatile("" ::: "memory");
      }
      if (ABLATE & PROBE_PHASES) { const unsigned long long t = stamp(); st_wait += t - st_prev; st_prev = t; }
    };
    // The 8 LDS-DMA pieces this wave contributes per iteration (4 of raw_{it+2} into R[it&1], 4 of
    // U_{it+2} into U[(it+2)%3]) are issued one per step in steps DMA0..DMA0+7 instead of in a
    // burst behind the barrier: an LDS-DMA instruction holds the wave's issue port for >100 cycles, and
    // spread out the SIMD's other wave covers that with its MFMAs; starting at step DMA0 = 6 (the 14x14 builds) leaves the
    // last pieces steps 14, 15 and the burst of flight time before the wave's next vmcnt(0) -- the compiler, which cannot
    // tell the LDS stages apart, puts one of its own in front of the next body's first ds_read -- and point 0 more
    // before the barrier.
    // They are issued unconditionally: a branch per piece (the compiler routes half of the
    // conditions through a VALU compare) cost ~30 of the ~210 instructions between an iteration's
    // first and last MFMA.  In the last two iterations of the range, where nothing is left to
    // fetch, the walker stands on the range's last chunk (valid addresses) and the pieces land in
    // R[it&1] / U[(it+2)%3] like any others: free stages, disjoint from the ones an epilogue
    // stages its stores in, and drained by the next iteration's vmcnt(0) or by the one before exit.
    // raw_{it+1}: the stage is ROFF
    // fragment base addresses of U_it and U_{it+1}: ub_cur[] / ub_nxt[], loop-carried registers that are
    // rotated in the iteration's tail -- formed here, at
    // the top, their eight adds sit in front of the iteration's first MFMAs; left inside the reads,
    // hipcc re-adds the stage offset before every one.
    // (the two copies of the body use the two register sets in swapped roles, so the rotation
    //  is four adds into the set that has just gone dead instead of four moves and four adds)
    const int (&ucur)[4] = decltype(par_c)::value ? ub_nxt : ub_cur;
    const int (&unxt)[4] = decltype(par_c)::value ? ub_cur : ub_nxt;
    // filter fragment of step s (point s >> 1, column blocks 2 (s & 1) + c)
    auto bread = [&](const int (&base)[4], int s2_, int c) {
      return lds_read2(base[2 * (s2_ & 1) + c] + (s2_ >> 1) * 2048);
    };

    f32x2 bf[16][2];
#pragma unroll
    for (int e = 0; e < PF; e++) { bf[e][0] = bfn[e][0]; bf[e][1] = bfn[e][1]; }
    P2 d[12], tmp[8];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int e = 0; e < 16; e++) {
      const int pt = e >> 1, cbp = e & 1;
      // -- top of the step: every LDS request of this step, before any MFMA.  Consumers sit
      //    at least one step later, so their waits are counted (lgkmcnt(N)), not drains.
      if (ABLATE & PROBE_NO_B_READS) {
        const f32x2 fake = {v[(e + 3) & 7].x, v[(e + 5) & 7].y};
        if (e + PF < 16) { bf[e + PF][0] = fake; bf[e + PF][1] = fake; }
        else { bfn[e + PF - 16][0] = fake; bfn[e + PF - 16][1] = fake; }
      } else if (e + PF < 16) {  // filter fragments of step e+PF
        bf[e + PF][0] = bread(ucur, e + PF, 0);
        bf[e + PF][1] = bread(ucur, e + PF, 1);
      } else {                   // ... and of steps 0, 1 of the next iteration
        bfn[e + PF - 16][0] = bread(unxt, e + PF - 16, 0);
        bfn[e + PF - 16][1] = bread(unxt, e + PF - 16, 1);
      }
      if (e >= DMA0 && e < DMA0 + 4) {
        issue_raw1(rs_dma, e - DMA0);
      } else if (e >= DMA0 + 4 && e < DMA0 + 8) {
        issue_u1(us_dma, e - DMA0 - 4);
      }
      // next iteration's A operand rides along: the six steps behind the barrier (2-7) read its 12 patch pixels (two per step, in
      // the order R0[j], R1[j], R2[j] column by column); B^T d B itself is written behind the last
      // step, after the iteration's last MFMA, where it runs as one burst of packed adds while the
      // SIMD's other wave still has MFMAs to issue.  (It used to be written inside the steps and left
      // unpinned: the optimizer sank it out of the body's block into the walker's blocks behind it.
      // The loop is one block per body now, nothing sinks, and written in the steps the adds stay
      // between the MFMAs.)  Measured alternatives (with 16 points per wave), all slower:
      // pinned to steps 2-15 (scalar or packed, +3..+8 %: arithmetic between a wave's MFMAs delays its
      // own next MFMA, and when it waits on a patch read the whole wave stalls behind it, in-order
      // issue); B^T d as the loop-carried state with every point formed one step ahead of its use
      // (+8 %); the two waves of a SIMD phase-shifted (+6 %).
      // (After the last iteration this works on stale LDS; the result is never used -- cheaper
      // than a branch.)
      if (e >= SYNC_STEP && e < SYNC_STEP + 6 && !(ABLATE & PROBE_NO_A_PATH)) {
        const int q0 = 2 * (e - SYNC_STEP), q1 = q0 + 1;   // read index q -> (row k = q % 3, column j = q / 3)
        d[(q0 % 3) * 4 + q0 / 3] = lds_read2(a_adr[q0 % 3][q0 / 3] + ROFF);
        d[(q1 % 3) * 4 + q1 / 3] = lds_read2(a_adr[q1 % 3][q1 / 3] + ROFF);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (!(ABLATE & (PROBE_NO_A_PATH | PROBE_NO_B_READS))) wait_lds(lds_wait_count(e));
      __builtin_amdgcn_sched_barrier(0);
      const P2 a = v[pt];
      const f32x2 b0 = bf[e][0], b1 = bf[e][1];
      if (ABLATE & PROBE_NO_MFMA) {  // keep the operands live, skip the matrix pipe
        asm volatile("" ::"v"(a.x), "v"(a.y), "v"(b0.x), "v"(b0.y), "v"(b1.x), "v"(b1.y));
      } else {
        // Tied destination: the accumulate chain stays in place (same vDst as SrcC is the
        // back-to-back form the matrix pipe forwards without wait states).  Left to the register
        // allocator, the builtin form ping-pongs every accumulator through a temporary tuple
        // (dst != SrcC), which costs the dependent MFMA several passes.  The compiler does not
        // see MFMA hazards of inline asm: the only VALU access to acc[] is in the epilogue, behind
        // explicit s_nops.
        asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc[pt][2 * cbp + 0]) : "v"(a.x), "v"(b0.x));
        if ((ABLATE & PROBE_PHASES) && e == SYNC_STEP) st_restart += stamp() - st_prev;   // the first MFMA behind the barrier is issued (since its release)
        asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc[pt][2 * cbp + 1]) : "v"(a.x), "v"(b1.x));
        asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc[pt][2 * cbp + 0]) : "v"(a.y), "v"(b0.y));
        asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc[pt][2 * cbp + 1]) : "v"(a.y), "v"(b1.y));
      }
      if (ABLATE & PROBE_PHASES) {
        if (e == 15) st_span += stamp() - st_prev;   // the iteration's last MFMA is issued (since the barrier's release)
      }
      __builtin_amdgcn_sched_barrier(0);
      if (e == SYNC_STEP - 1) {
        sync_point();
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // B^T d B of the next iteration, in place over V: every point has retired, all patch reads are in (step 9)
    if (!(ABLATE & PROBE_NO_A_PATH)) {
      if (ABLATE & PROBE_NO_BTDB) {
#pragma unroll
        for (int i = 0; i < 12; i++) asm volatile("" :: "v"(d[i]));
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) tmp_col(tmp, d, j);
        if (ABLATE & PROBE_NO_VPOINT) {
#pragma unroll
          for (int i = 0; i < 8; i++) asm volatile("" :: "v"(tmp[i]));
        } else {
#pragma unroll
          for (int e = 0; e < 8; e++) v_point(v, tmp, e);
        }
      }
    }
  };

  // ---- per-wave epilogue (the DMA pipeline keeps running underneath) -------------------------
  // Slab image of one partial segment: [wave 0..7][q = 4cb+p][lane] of 16 B (output pixel p of the
  // tile rows 4h .. 4h+3, out-channel cb*16+t16, pre-BN).  Waves hand their 8 KiB parts over
  // independently: wave w of every segment of an item draws on tickets[8*item + w].
  //
  // A segment ends with the item's last chunk or with the range.  Whole segments are finalized
  // from registers.  A partial segment publishes its slab part; if more work follows (it is the
  // head of the range) its ticket is drawn one segment later, when the stores have long drained;
  // the range's last segment draws at once.  Whoever draws an item's last ticket gathers all
  // parts (in segment order: bitwise reproducible whoever reduces) and finalizes.
  //
  // Everything the epilogue needs beyond the accumulators is re-derived here from an OPAQUE copy
  // of the lane / wave id and from the kernarg segment, so that nothing epilogue-only is hoisted
  // out of the segment loop and kept in registers across the main loop (which has none to spare).
  // rfree / ufree = byte offsets of the two LDS stages nobody needs at a segment boundary
  // (raw_{it+1} is already in registers, U_it is spent); each wave takes 8 KiB of them.
  auto epilogue = [&](bool last_of_range, int rfree, int ufree) {
    unsigned long long ph_t = 0;
    auto phase = [&](int k) { if (ABLATE & PROBE_PHASES) { const unsigned long long t = stamp(); if (k >= 0) st_ph[k] += t - ph_t; ph_t = t; } };
    // the finer stamps (PHS_*): sub(-1) starts a stretch, sub(k) books the time since the last stamp on part k
    unsigned long long sub_t = 0;
    auto sub = [&](int k) { if (ABLATE & PROBE_PHASES) { const unsigned long long t = stamp(); if (k >= 0) st_sub[k] += t - sub_t; sub_t = t; } };
    phase(-1);
    // every wave is done reading those two stages (a bare barrier: no memory counter needs to
    // drain here, and __syncthreads() would wait for the LDS-DMA pieces in flight)
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // the last MFMAs' results must have landed before VALU code reads / rewrites the accumulators
    // (the hazard recognizer cannot see through the inline-asm MFMAs)
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    phase(0);
    int ln = lane, wv = w;
    asm volatile("" : "+v"(ln));
    asm volatile("" : "+s"(wv));
    const int e_t16 = ln & 15, e_h = ln >> 4, e_wt = wv >> 1, e_wk = wv & 1;
    char* wreg = smem + (wv < 4 ? rfree + wv * 8192 : ufree + (wv - 4) * 8192);
    KernargPtr kp = kernarg();
    const Geo geo = load_geo(kp);
    const int Wp = GEN ? geo.Wp : WINO_HW, Hp = GEN ? geo.Hp : WINO_HW;
    const int N = kp->N, K = kp->K, relu = kp->relu, KBLK = K >> 6, totalTiles = N * (GEN ? (int)geo.tiles : WINO_TILES);
    const unsigned sk_q = kp->sk_q, sk_rem = kp->sk_rem;
    const int tail_item0 = kp->ndp * G;
    // k-groups of the tail: this workgroup is range lp_e of group grp_e (slab slots are numbered by (tail range,
    // group)); worked out only by the partial-segment paths below, with multipliers instead of divisions
    struct TailPos { int kpg, Gp, lp, grp; FastDiv d_kp; };
    auto tail_pos = [&]() {
      TailPos t;
      t.kpg = kp->kp; t.Gp = kp->Gp;
      t.d_kp.m = kp->d_kp.m; t.d_kp.l = kp->d_kp.l;
      FastDiv dP, dC;
      dP.m = kp->d_P.m; dP.l = kp->d_P.l; dC.m = kp->d_copies.m; dC.l = kp->d_copies.l;
      const int lpos_e = (int)fastdiv((unsigned)lg, t.d_kp);
      t.grp = lg - lpos_e * t.kpg;
      t.lp = tail_range_of_fast(lpos_e, kp->ph_P, kp->ph_inv, kp->ph_copies, dP, dC);
      return t;
    };
    const float* bnBias = kp->bnBias;
    const float* bnScale = kp->bnScale;
    unsigned* tickets = kp->tickets;
    // (POOL: the output is the pooled map, Hq x Wq padded)
    const int Hq = POOL ? (Hp - 2) / 2 + 2 : Hp, Wq = POOL ? (Wp - 2) / 2 + 2 : Wp;
    const auto rsrc_out = make_rsrc(kp->out, (unsigned)((size_t)N * Hq * Wq * K * sizeof(float)));
    const auto rsrc_slab = make_rsrc(kp->slabs, (unsigned)((size_t)2 * G * SLAB_BYTES));
    const unsigned slab_voff = (unsigned)((wv * 8 * 64 + ln) * 16);

    auto load_bn = [&](int item, float (&sc)[2], float (&bi)[2]) {
      const int kb = item % KBLK;
#pragma unroll
      for (int cb = 0; cb < 2; cb++) {
        const int kc = kb * KB + e_wk * 32 + cb * 16 + e_t16;
        sc[cb] = bnScale[kc];
        bi[cb] = bnBias[kc];
      }
    };
    auto draw_ticket = [&](int item) -> unsigned {   // one returning agent-scope add per wave
      unsigned old = 0;
      if (ln == 0)
        old = __hip_atomic_fetch_add(tickets + (size_t)item * 8 + wv, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return old;   // meaningful in lane 0; readfirstlane at the use
    };

    // folded BN of this segment's item (this lane's two out-channels); in flight during A^T m A
    const int c_item = __builtin_amdgcn_readfirstlane(c_item_vg), seg_kind = __builtin_amdgcn_readfirstlane(seg_kind_vg);
    float bn_sc[2], bn_bi[2];
    load_bn(c_item, bn_sc, bn_bi);
    // The previous segment's deferred ticket is drawn now.
    int pend_item = __builtin_amdgcn_readfirstlane(pend_vg);
    unsigned pend_old = 0;
    if (TAIL && pend_item >= 0) pend_old = draw_ticket(pend_item);   // in flight while A^T m A runs
    // The peek.  A partial segment that ends its range looks at its item's counter before it publishes anything: one
    // relaxed agent-scope load per wave, in flight while A^T m A runs.  If every other segment has already drawn, this
    // wave finishes the item from its registers (below); if not, nothing is lost -- it takes the ticket path.
    // (sk_q = 0, ranges of at most one iteration on a grid beyond the tail's iterations, keeps the ticket path: some
    //  ranges own nothing there, and the gather from registers does not look for them.)
    // Every partial segment that would draw at once peeks (`now`, below: the range's last segment, and a straddler's
    // second one -- where the item lies between two straddlers, nseg = 2, the later of them finishes it this way).
    const bool draws_now = last_of_range || ((seg_kind & 2) && pend_item >= 0);
    const bool peeking = TAIL && draws_now && !(seg_kind & 1) && sk_q > 0 && !(ABLATE & PROBE_NO_HANDOFF);
    unsigned peek = 0;
    if (peeking && ln == 0)
      peek = __hip_atomic_load(tickets + (size_t)c_item * 8 + wv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // A^T m A (C/D layout: col = lane&15, row = 4*(lane>>4)+r).  The wave holds point rows i = 2 ph and
    // 2 ph + 1 (local rows 0, 1) for all four column blocks.  Per (tile row r, column block cb):
    //   column transform inside each point row:  c0(i) = m_i0 + m_i1 + m_i2,  c1(i) = m_i1 - m_i2 - m_i3
    //   row transform:  Y[0][b] = c_b(0) + c_b(1) + c_b(2),  Y[1][b] = c_b(1) - c_b(2) - c_b(3)
    // of which this wave can form the part of its two rows:
    //   ph = 0:  P[0][b] = c_b(0) + c_b(1),  P[1][b] = c_b(1)      ph = 1:  P[0][b] = c_b(2),  P[1][b] = -(c_b(2) + c_b(3))
    // (no multiplies by 0 / +-1: exact, and an Inf in one part cannot turn the other into NaN).  Pixel index p = 2a + b.
    // The parts of logical column blocks 2, 3 go to the partner wave (w ^ 1, the same tiles) through
    // this wave's 8 KB of the free LDS stages; the partner's parts of MY blocks 0, 1 come back the same
    // way.  y[cb][p][r] = output pixel p of tile row 4h+r, out-channel (32 ph) + cb*16 + t16 --
    // from here on exactly what the wave held when it owned 16 points of 32 out-channels.
    // The two halves differ only in which of {c(0), c(0) + c(1), c(1)} they form, so the code exists once per ph behind
    // ONE wave-uniform branch (outside the MFMA loop it is free) and each side computes only what it stores -- as
    // selects on ph this was four v_cndmask per part() on top of both candidates.  The minus of P[1][b], ph = 1, is
    // folded into the add that consumes the part: that wave keeps and sends the plain sum S = c_b(2) + c_b(3), and
    //   ph = 0 (receives S from its partner):  Y[1][b] = P[1][b] - S      ph = 1 (holds S itself):  Y[1][b] = X - S
    // -- x + (-s) and x - s are the same IEEE operation, so every output keeps its bits.
    // Everything below is written on PAIRS of tile rows (r, r + 1): they sit in adjacent registers of every
    // accumulator, so each add of the transform is one v_pk_add_f32 on register pairs as they lie -- per (r, cb) and
    // scalar, the compiler packed across the points instead and paid a v_mov_b32 per operand to line them up.  The
    // price is the layout of the result: y[cb][p] holds pixel p of the four tile rows r (not the four pixels of one
    // row); the exchange, the slab and BN + ReLU are elementwise and do not care, the transpose below picks its scalars
    // by index.
    f32x4 y[2][4];
    auto atma = [&](auto ph_c) {
      constexpr bool PH1 = decltype(ph_c)::value;
      auto parts = [&](int cb, f32x4 (&o)[4]) {   // of column block cb: o[p = 2a + b], over the four tile rows
#pragma unroll
        for (int rp = 0; rp < 2; rp++) {
          P2 c[2][2];
#pragma unroll
          for (int i = 0; i < 2; i++) {
            const f32x4 &q0 = acc[i * 4 + 0][cb], &q1 = acc[i * 4 + 1][cb], &q2 = acc[i * 4 + 2][cb], &q3 = acc[i * 4 + 3][cb];
            const P2 m0 = rp ? q0.zw : q0.xy, m1 = rp ? q1.zw : q1.xy, m2 = rp ? q2.zw : q2.xy, m3 = rp ? q3.zw : q3.xy;
            c[i][0] = m0 + m1 + m2;
            c[i][1] = m1 - m2 - m3;
          }
#pragma unroll
          for (int bb = 0; bb < 2; bb++) {
            const P2 a0 = PH1 ? c[0][bb] : c[0][bb] + c[1][bb];   // a = 0
            const P2 a1 = PH1 ? c[0][bb] + c[1][bb] : c[1][bb];   // a = 1 (ph = 1: S, its minus is in the consumer)
            if (rp) o[bb].zw = a0, o[2 + bb].zw = a1;
            else o[bb].xy = a0, o[2 + bb].xy = a1;
          }
        }
      };
      char* const xmine = wreg + ln * 16;
      const char* const xpart = smem + ((wv ^ 1) < 4 ? rfree + (wv ^ 1) * 8192 : ufree + ((wv ^ 1) - 4) * 8192) + ln * 16;
#pragma unroll
      for (int cb = 0; cb < 2; cb++) {
        f32x4 o[4];
        parts(2 + cb, o);
#pragma unroll
        for (int pp = 0; pp < 4; pp++) *(f32x4*)(xmine + (4 * cb + pp) * 1024) = o[pp];
      }
#pragma unroll
      for (int cb = 0; cb < 2; cb++) parts(cb, y[cb]);
      sub(PHS_PARTS);
      // every wave's outgoing parts are in LDS (its own ds_writes drained) before anyone reads them
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
#pragma unroll
      for (int cb = 0; cb < 2; cb++)
#pragma unroll
        for (int pp = 0; pp < 4; pp++) {
          const f32x4 x = *(const f32x4*)(xpart + (4 * cb + pp) * 1024);
          if (pp < 2) y[cb][pp] += x;
          else y[cb][pp] = PH1 ? x - y[cb][pp] : y[cb][pp] - x;
        }
      // ... and read, before the finalize below stages output rows through the same LDS
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    };
    sub(-1);
    if (wv & 1) atma(std::true_type{});
    else atma(std::false_type{});
    sub(PHS_EXCHANGE);
#pragma unroll
    for (int e = 0; e < 8; e++)
#pragma unroll
      for (int cb = 0; cb < 4; cb++) acc[e][cb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (ABLATE & PROBE_PHASES) {   // (the stamp must not be overtaken by the moves: they have no other reader before the next body)
#pragma unroll
      for (int e = 0; e < 8; e++)
#pragma unroll
        for (int cb = 0; cb < 4; cb++) asm volatile("" : "+v"(acc[e][cb]));
    }
    sub(PHS_ZERO);
    phase(1);
    const bool whole = !TAIL || (seg_kind & 1) != 0;
    // up to two items to look at: [0] this segment's, [1] the deferred head segment's
    // (job1 is taken BEFORE this segment may re-arm pend_item with its own deferred ticket -- the second
    //  partial segment of a range that goes on to whole items.  Round 1 tested pend_item != c_item after the
    //  re-arm and lost the drawn item in exactly that case: harmless while the range's neighbour, whose
    //  ticket on that item waits behind a whole item, draws last; an item never finalized when this
    //  workgroup starts late -- a grid beyond the CU count, or CUs shared with another stream's kernel.)
    int job0 = -1, job1 = TAIL ? pend_item : -1;
    pend_item = -1;
    unsigned old0 = 0;
    if (whole) {
      job0 = c_item;
    } else if (!(ABLATE & PROBE_NO_HANDOFF)) {
      // slab slot: 2l for the segment that continues an item (head of l's range), 2l+1 for the
      // one that starts an item
      // (a peeking segment publishes only if its peek fails: in the gather loop below, once the item's segment count
      //  is known)
      if (!peeking) {
        const TailPos tp = tail_pos();
        const unsigned my_slot = 2u * (unsigned)(tp.lp * tp.kpg + tp.grp) + ((seg_kind & 2) ? 1u : 0u);
#pragma unroll
        for (int q = 0; q < 8; q++)
          slab_store16(y[q >> 2][q & 3], rsrc_slab, slab_voff + q * 1024, my_slot * SLAB_BYTES);
      }
      // When is this segment's ticket drawn?  Whoever draws an item's last ticket gathers it, and a gather is
      // 3-5 us of work that only an epilogue can do:
      //  * the range's last segment: now (there is no later epilogue);
      //  * a segment that STARTS its item in a range that already had a partial segment (a "straddler": its
      //    range crosses an item boundary, so it pays one epilogue more than its neighbours): now.  Deferred to
      //    the final epilogue it was always its item's last arriver: the workgroups that are the slowest anyway
      //    gathered at the very end of the launch (round 1: exits spread over 106 .. 117.6 us at 256 channels,
      //    N = 128; tools/ablate_fused 256 256 t).  The wait costs little: the next iteration's vmcnt(0)
      //    would have waited for the same stores;
      //  * any other partial segment (the head of a straddling range): at the next epilogue, when its stores have
      //    long drained.
      // 256 channels: N = 128 118.7 -> 117.7 us, N = 96 98.5 -> 94.8; elsewhere within +-0.7 %.  (On top of this, the
      // gather's slabs requested all at once, the deferred item's before this segment's own finalize, with the
      // accumulators re-zeroed at the end of the epilogue to make room: 0.1-0.6 % slower everywhere.)
      // Both kinds of "now" peek first (above) and publish and draw, in the gather loop below, only when the peek finds
      // a segment still out.  The only tail segment of a range that lies inside one item is such a last segment: it
      // runs after the range's whole items, finds the others long done and finishes the (usual) 3-segment item from
      // its registers -- these workgroups have the slack (no second partial epilogue).  The straddler's second segment
      // must keep its "now": deferred, its ticket would be drawn in the straddler's final epilogue, AFTER the
      // one-segment workgroup has peeked, whose peek would then always fail (measured: +3.5 us at 256 channels,
      // N = 128).  Its peek pays where the item has no later finisher -- a 2-segment item between two straddlers, or
      // a grid without whole-item rounds: the later of the two finishes it with one slab read instead of a round trip
      // of its own part.
      const bool now = draws_now;
      if (peeking) {
        job0 = c_item;
      } else if (!now) {
        pend_item = c_item;        // ticket deferred to the next segment's epilogue
      } else {
        wait_vmem_all();           // this wave's write-through stores have left ...
        old0 = draw_ticket(c_item);   // ... before its ticket
        job0 = c_item;
      }
    }
    pend_vg = pend_item;
    asm volatile("" : "+v"(pend_vg));
    phase(2);
#pragma unroll 1
    for (int j = 0; j < (TAIL ? 2 : 1); j++) {
      const int item = j == 0 ? job0 : job1;
      if (item < 0) continue;
      if (!(j == 0 && whole)) {
        const TailPos tp = tail_pos();
        const int kpg = tp.kpg, Gp = tp.Gp, grp_e = tp.grp;
        unsigned old = __builtin_amdgcn_readfirstlane(j == 0 ? old0 : pend_old);
        bool cand = j == 0 && peeking;   // this wave may still finish the item from its registers
        const unsigned pk = __builtin_amdgcn_readfirstlane(peek);
        auto publish_and_draw = [&]() {   // a peek that failed: the ticket path
          const unsigned my_slot = 2u * (unsigned)(tp.lp * kpg + grp_e) + ((seg_kind & 2) ? 1u : 0u);
#pragma unroll
          for (int q = 0; q < 8; q++)
            slab_store16(y[q >> 2][q & 3], rsrc_slab, slab_voff + q * 1024, my_slot * SLAB_BYTES);
          wait_vmem_all();
          old = __builtin_amdgcn_readfirstlane(draw_ticket(item));
          cand = false;
        };
        // (a partial segment's item has at least two segments: a counter at 0 cannot be at nseg - 1)
        if (cand && pk == 0u) publish_and_draw();
        // A drawn ticket that came back 0 was the item's first: somebody else will finish the item, and the walk below
        // (a dozen range starts per wave) has nothing to find out.
        if (!cand && old == 0u) continue;
        // which logical workgroups share `item`: walk outwards from lg.  With more workgroups
        // than iterations some own nothing; they are not segments.
        const unsigned x0 = fastdiv((unsigned)(item - tail_item0), tp.d_kp) * (unsigned)nchunks, x1 = x0 + nchunks - 1;   // the group's tail space
        int gA = tp.lp, gB = tp.lp;
        while (sk_start(gA, sk_q, sk_rem, Gp) > x0) gA--;
        while (gB + 1 < Gp && sk_start(gB + 1, sk_q, sk_rem, Gp) <= x1) gB++;
        int nseg = 0;
        for (int g = gA; g <= gB; g++)
          nseg += sk_start(g + 1, sk_q, sk_rem, Gp) != sk_start(g, sk_q, sk_rem, Gp);
        // A peeking segment: a counter at nseg - 1 means that every other segment has drained its slab and drawn its
        // ticket and that nobody else will look at the item again -- this wave is its last arriver without drawing, and
        // its own part never leaves its registers.  Anything less: the ticket path -- publish, drain, draw.  Nobody waits.
        const bool mine = cand && pk == (unsigned)(nseg - 1);
        if (cand && !mine) {
          if (pk >= (unsigned)nseg && ln == 0)   // (as below: the counter was not zero at launch)
            __hip_atomic_store(kp->err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          publish_and_draw();
        }
        if (!mine && old != (unsigned)(nseg - 1)) {   // another workgroup's wave w will finish the item
          // ... unless the counter was not zero when the launch began (a launch that died mid-way before this
          // one): say so on the host-visible word; the library then refuses the stream until it is reset
          if (old >= (unsigned)nseg && ln == 0) __hip_atomic_store(kp->err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          continue;
        }
        if (ln == 0)   // self-cleaning counter: the next launch finds 0 again.  (Subtracted, not stored: a counter
                       // that was NOT zero at launch then stays off by the same amount, and the item's last
                       // drawer is certain to see a value >= nseg -- the report above cannot be missed.)
          __hip_atomic_fetch_sub(tickets + (size_t)item * 8 + wv, (unsigned)(mine ? nseg - 1 : nseg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // gather: all segments' parts, summed in segment order
        sub(-1);
        bool first = true;
        int g0 = gA;
        if (mine) {
          // This wave's own part takes its place in that order from y: the segments before it are summed in t and y
          // joins them as t + y (the same IEEE operation as y + t); the ones behind it are added to y as ever.  Same
          // operands, same order, same bits.  (sk_q > 0: every range in gA .. gB owns something.)
          if (gA < tp.lp) {
            f32x4 t[8];
#pragma unroll
            for (int q = 0; q < 8; q++)
              t[q] = slab_load16(rsrc_slab, slab_voff + q * 1024, (2u * (unsigned)(gA * kpg + grp_e) + 1u) * SLAB_BYTES);
#pragma unroll 1
            for (int g = gA + 1; g < tp.lp; g++) {   // (piecewise: y and t are all the registers the gather may hold)
#pragma unroll
              for (int q = 0; q < 8; q++)
                t[q] = t[q] + slab_load16(rsrc_slab, slab_voff + q * 1024, 2u * (unsigned)(g * kpg + grp_e) * SLAB_BYTES);
            }
#pragma unroll
            for (int q = 0; q < 8; q++) y[q >> 2][q & 3] = t[q] + y[q >> 2][q & 3];
          }
          first = false;
          g0 = tp.lp + 1;
        }
#pragma unroll 1
        for (int g = g0; g <= gB; g++) {
          if (sk_start(g + 1, sk_q, sk_rem, Gp) == sk_start(g, sk_q, sk_rem, Gp)) continue;   // owns nothing
          const unsigned slot = 2u * (unsigned)(g * kpg + grp_e) + (first ? 1u : 0u);   // (tail range g, this group)
          f32x4 t[8];
#pragma unroll
          for (int q = 0; q < 8; q++) t[q] = slab_load16(rsrc_slab, slab_voff + q * 1024, slot * SLAB_BYTES);
#pragma unroll
          for (int q = 0; q < 8; q++) y[q >> 2][q & 3] = first ? t[q] : y[q >> 2][q & 3] + t[q];
          first = false;
        }
        sub(PHS_GATHER);
      }
      float sc2[2] = {bn_sc[0], bn_sc[1]}, bi2[2] = {bn_bi[0], bn_bi[1]};
      // relu_nan() with the run-time `relu` folded into its threshold (nothing is below -Inf, and a NaN compares false
      // either way): one compare and one select per element, where testing `relu` per element cost a second select
      const float relu_thr = relu ? 0.f : -__builtin_inff();
      auto relu_if = [&](float v) { return v < relu_thr ? 0.f : v; };
      if (item != c_item) load_bn(item, sc2, bi2);   // the deferred head item
      if (ABLATE & PROBE_NO_STORE) continue;  // price the store tail

      // ---- finalize: BN + ReLU, then the wave's 16 tiles x 2x2 px x 32 out-channels go through
      // its private 8 KiB of LDS so that they leave as whole 128-byte runs of the padded NHWC
      // output (16 B per lane, 8 runs per store).  (The zero ring is written by the ring pass at
      // the start of the kernel.)
      // Image: [tile 0..15][px 0..3][k 0..31] floats; the 16-float group index (2*px + cb) is
      // XORed with (tile>>2)&3 = the MFMA row group h, which makes the ds_write_b32 of the 4 row
      // groups and the ds_read_b128 of every 16 lanes hit 64 distinct banks.
      const int tb = item / KBLK, kb = item - tb * KBLK;
      sub(-1);
      // RES: the eight residual runs this lane stores are requested before the transpose, so that their latency hides
      // under it; each only where its store is kept (the residual's ring is never read)
      f32x4 rv[RES ? 8 : 1];
      if constexpr (RES) {
        typedef const __attribute__((address_space(4))) FusedResParams* ResKernargPtr;
        const auto rsrc_res = make_rsrc(((ResKernargPtr)kp)->res, (unsigned)((size_t)N * Hp * Wp * K * sizeof(float)));
        const int px = (ln >> 3) & 3, pa = px >> 1, pb = px & 1;
        const unsigned kbyte = (unsigned)((kb * KB + e_wk * 32 + (ln & 7) * 4) * sizeof(float));
#pragma unroll
        for (int i = 0; i < 8; i++) {   // (the addressing of the store loop below)
          const int g = tb * TB + e_wt * 16 + 2 * i + (ln >> 5);
          const bool live = g < totalTiles;
          const TileCoord tc = decode_tile_g<GEN>(live ? g : 0, geo);
          const int py = 1 + 2 * tc.ty + pa, pxx = 1 + 2 * tc.tx + pb;
          const unsigned img = (unsigned)(tc.n * Hp * Wp);
          rv[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
          if (live && (!GEN || (py <= Hp - 2 && pxx <= Wp - 2)))
            rv[i] = buf_load16(rsrc_res, (unsigned)((img + py * Wp + pxx) * K * sizeof(float)) + kbyte, 0);
        }
      }
      if constexpr (POOL) {
        // Pooled finalize.  Image: [row P = 4 r + h][k 0..31] floats, 2 KB: tile 4 h + r of the wave's 16 sits in row
        // 4 r + h, and its 16-float group cb is XORed with h >> 1 -- the four row groups h of a ds_write_b32 then
        // hit the four 16-bank quarters, and the two rows a 16-lane ds_read_b128 group reads are consecutive (the
        // two 32-bank halves).
#pragma unroll
        for (int cb = 0; cb < 2; cb++) {
          f32x4 m = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int pp = 0; pp < 4; pp++) {
            f32x4 v1 = __builtin_elementwise_fma((f32x4){sc2[cb], sc2[cb], sc2[cb], sc2[cb]}, y[cb][pp], (f32x4){bi2[cb], bi2[cb], bi2[cb], bi2[cb]});   // (two v_pk_fma_f32)
#pragma unroll
            for (int r = 0; r < 4; r++) {
              v1[r] = relu_if(v1[r]);
              m[r] = pp == 0 ? v1[r] : max_nan(m[r], v1[r]);
            }
          }
#pragma unroll
          for (int r = 0; r < 4; r++) *(float*)(wreg + (4 * r + e_h) * 128 + ((cb ^ (e_h >> 1)) << 6) + e_t16 * 4) = m[r];
        }
        sub(PHS_BN);
        // lane -> row P = 8 i + (lane >> 3) = tile 4 (P & 3) + (P >> 2), 16-byte chunk lane & 7: two rounds of eight
        // whole 128-byte runs
        const unsigned kbyte = (unsigned)((kb * KB + e_wk * 32 + (ln & 7) * 4) * sizeof(float));
#pragma unroll
        for (int i = 0; i < 2; i++) {
          const int P = 8 * i + (ln >> 3), ph_t = P & 3, tl = 4 * ph_t + (P >> 2);
          const f32x4 val = *(const f32x4*)(wreg + P * 128 + (((((ln & 7) >> 2) ^ (ph_t >> 1))) << 6) + (ln & 3) * 16);
          const int g = tb * TB + e_wt * 16 + tl;
          const bool live = g < totalTiles;
          const TileCoord tc = decode_tile_g<GEN>(live ? g : 0, geo);
          const int py = 1 + tc.ty, pxx = 1 + tc.tx;
          const unsigned img = (unsigned)(tc.n * Hq * Wq);
          // (odd H or W: the clipped last tile row / column has no pooled output)
          const bool keep = live && (!GEN || (py <= Hq - 2 && pxx <= Wq - 2));
          if (keep) buf_store16_nt(val, rsrc_out, (unsigned)((img + py * Wq + pxx) * K * sizeof(float)) + kbyte, 0);
        }
        sub(PHS_STORE);
        continue;
      }
      int ep_wbase[4], ep_rbase[4];
#pragma unroll
      for (int jj = 0; jj < 4; jj++) {
        ep_wbase[jj] = e_h * 2048 + ((jj ^ e_h) << 6) + e_t16 * 4;                       // + r*512 + (g>>2)*256
        const int px = (ln >> 3) & 3, c = ln & 7;
        ep_rbase[jj] = (ln >> 5) * 512 + (((px * 2 + (c >> 2)) ^ jj) << 6) + (c & 3) * 16;   // + 2i*512
      }
#pragma unroll
      for (int cb = 0; cb < 2; cb++) {
#pragma unroll
        for (int pp = 0; pp < 4; pp++) {
          f32x4 v1 = __builtin_elementwise_fma((f32x4){sc2[cb], sc2[cb], sc2[cb], sc2[cb]}, y[cb][pp], (f32x4){bi2[cb], bi2[cb], bi2[cb], bi2[cb]});   // (two v_pk_fma_f32)
          const int g = pp * 2 + cb;
#pragma unroll
          for (int r = 0; r < 4; r++) {
            if (!RES) v1[r] = relu_if(v1[r]);   // (RES: after the residual's add, below)
            *(float*)(wreg + ep_wbase[g & 3] + r * 512 + (g >> 2) * 256) = v1[r];
          }
        }
      }
      sub(PHS_BN);
      // lane -> run (lane>>3) = (tile 2i + (lane>>5), px (lane>>3)&3), 16-byte chunk lane&7
      // (tried: the tile arithmetic on the scalar unit, one tile per half-wave -- 40 % slower)
      const int px = (ln >> 3) & 3, pa = px >> 1, pb = px & 1;
      const unsigned kbyte = (unsigned)((kb * KB + e_wk * 32 + (ln & 7) * 4) * sizeof(float));
#pragma unroll
      for (int i = 0; i < 8; i++) {
        f32x4 val = *(const f32x4*)(wreg + ep_rbase[i >> 1] + i * 1024);
        if constexpr (RES) {
          val += rv[i];
          if (relu) {
#pragma unroll
            for (int q = 0; q < 4; q++) val[q] = relu_nan(val[q]);
          }
        }
        const int g = tb * TB + e_wt * 16 + 2 * i + (ln >> 5);
        const bool live = g < totalTiles;
        const TileCoord tc = decode_tile_g<GEN>(live ? g : 0, geo);
        const int py = 1 + 2 * tc.ty + pa, pxx = 1 + 2 * tc.tx + pb;
        const unsigned img = (unsigned)(tc.n * Hp * Wp);
        // (odd H or W: the last tile row / column computes one output row / column too many, from
        //  patch rows that belong to the next image row or lie past the tensor -- the descriptor's
        //  range check returns 0 there; a Winograd output only depends on its own 3x3 window, so
        //  the kept outputs are unaffected, and the surplus ones must not reach the ring)
        const bool keep = live && (!GEN || (py <= Hp - 2 && pxx <= Wp - 2));
        // Non-temporal: the output is written once and, at 33 MB for the reference layer, exceeds the
        // 32 MB of L2 anyway.  Old and new libraries interleaved: 256ch 125.4 -> 123.9 us, 128ch
        // 43.5 -> 41.95, the other feature maps -0.4..-1.8 %; HBM bytes and L2 hit rate unchanged;
        // the bottleneck blocks, whose last launch reads this output at once, within +-0.3 %.
        // (A run-time choice between the two store forms cost more than it saved: its extra live
        // scalar pushed SGPR spill code into the MFMA loop.)
        if (keep) buf_store16_nt(val, rsrc_out, (unsigned)((img + py * Wp + pxx) * K * sizeof(float)) + kbyte, 0);
      }
      sub(PHS_STORE);
    }
    phase(3);
  };

  // ================================ main loop =====================================
  // The tight loop runs to the next EVENT: the end of the compute segment (then the one epilogue site) or the DMA
  // stream's next item switch / end, two iterations ahead of it (dma_event), whichever is due first, or both.  Between
  // events an iteration's tail is the common path alone: the stream's two scalar adds, the four fragment-base
  // rotations, the filter-stage counter, the count-down and its branch.  The two copies of the body alternate
  // statically; which one an entry starts with, and the parity it leaves, are settled once per entry.
  {
    int us = 0;    // filter stage of iteration `it` (= it % 3)
    int par = 0;   // it & 1
    auto next = [](int s) { return s == 2 ? 0 : s + 1; };
    int c_run = 0;       // iterations this segment still has to run
    ws_put(WS_C_LEFT{}, L);   // ... and the range after this segment
    // iterations of the next segment: to the end of the item, or of the tail range
    auto segment = [&]() {
      int c_tail = __builtin_amdgcn_readfirstlane(c_tail_vg);
      const int n = c_tail > 0 && c_tail < nchunks - c_chunk ? c_tail : nchunks - c_chunk;
      seg_kind_vg = c_chunk == 0 ? (n == nchunks ? 3 : 2) : 0;
      asm volatile("" : "+v"(seg_kind_vg));
      // the walker's state after this segment, settled now so that neither n nor c_chunk lives across the loop:
      // c_tail < 0 = "the tail ends with this segment"
      if (c_tail > 0 && (c_tail -= n) == 0) c_tail = -1;
      c_tail_vg = c_tail;
      ws_put(WS_C_LEFT{}, ws_get(WS_C_LEFT{}) - n);
      asm volatile("" : "+v"(c_tail_vg));
      c_chunk = 0;   // every later segment starts its item
      c_run = n;
    };
    auto tail = [&](auto par_c) {   // everything between two bodies
      d_soff_raw += d_step_raw;
      d_soff_u += d_step_u;
      asm volatile("" : "+s"(d_soff_raw), "+s"(d_soff_u));
      us = next(us);
      {   // rotate the filter-fragment bases: U_{it} was U_{it+1}; the new U_{it+1} is stage next(us)
        const int off = next(us) * U_BYTES;
#pragma unroll
        for (int cb = 0; cb < 4; cb++) {
          // the set the body just used as "current" is dead: it becomes the next body's "next"
          if (decltype(par_c)::value) ub_nxt[cb] = b_base[cb] + off;
          else ub_cur[cb] = b_base[cb] + off;
        }
      }
    };
    segment();
#pragma unroll 1
    for (;;) {
      {
        int k = d_run < c_run ? d_run : c_run;
        // both counts as they will be after the k iterations, parked: the loop keeps k alone
        ws_put(WS_D_RUN{}, d_run - k), ws_put(WS_C_RUN{}, c_run - k);
        // One trip = (body 0, tail 0, body 1, tail 1): an if for an entry on odd `it`, which skips body 0 once, an
        // if for a count that runs out after body 0, and the back edge -- three branches, one of them taken.  The
        // empty asm statements keep the compiler from threading those tests into a loop that is entered in its
        // middle, which it then repairs with a dispatch block and a flag test after every body.
        int skip0 = par;
        par ^= k & 1;   // the parity the k iterations leave
#pragma unroll 1
        do {
          asm volatile("" : "+s"(skip0));
          if (!skip0) {
            body(std::integral_constant<int, 0>{}, 0, next(next(us)));
            tail(std::integral_constant<int, 0>{});
            --k;
          }
          skip0 = 0;
          asm volatile("" : "+s"(k));
          if (k != 0) {
            body(std::integral_constant<int, 1>{}, 1, next(next(us)));
            tail(std::integral_constant<int, 1>{});
            --k;
          }
          asm volatile("" : "+s"(k));
        } while (k != 0);
        d_run = ws_get(WS_D_RUN{});
        c_run = ws_get(WS_C_RUN{});
      }
      if (d_run == 0) dma_event();
      if (c_run != 0) continue;
      // the segment's last iteration was it-1: raw stage R[it & 1] and the filter stage before U[us] are free
      const int us_last = us == 0 ? 2 : us - 1;
      const bool last_of_range = ws_get(WS_C_LEFT{}) == 0;
      if (ABLATE & PROBE_PHASES) { const unsigned long long t = stamp(); st_comp += t - st_prev; st_prev = t; }
      if ((ABLATE & PROBE_TIMELINE) && last_of_range && tid == 0) {
        KernargPtr kp = kernarg();
        kp->dbg[(size_t)lg * TL_WORDS + TL_LAST_EPI] = __builtin_amdgcn_s_memrealtime();
      }
      epilogue(last_of_range, par * RAW_BYTES, N_RSTAGE * RAW_BYTES + us_last * U_BYTES);
      if (ABLATE & PROBE_PHASES) { const unsigned long long t = stamp(); st_epi += t - st_prev; st_prev = t; }
      if (last_of_range) break;
      const int c_tail = __builtin_amdgcn_readfirstlane(c_tail_vg);
      if (TAIL && ws_get(WS_C_LEFT{}) == ws_get(WS_WF_LT{})) {   // whole-first range, rounds done: its tail segment
        c_item_vg = ws_get(WS_T_ITEM{});
        c_chunk = ws_get(WS_T_CHUNK{});
        c_tail_vg = ws_get(WS_WF_LT{});
      } else if (c_tail < 0) {   // tail done: first whole item
        c_item_vg = lg;
        c_tail_vg = 0;
      } else {
        c_item_vg += c_tail > 0 ? kernarg()->kp : G;
      }
      asm volatile("" : "+v"(c_item_vg), "+v"(c_tail_vg));
      segment();
    }
  }
  wait_vmem_all();   // no LDS-DMA of this wave may land after the workgroup's LDS has been given away
  clk_exit();

  // diagnostic builds: the stamps go to a buffer of their own (prm.dbg), never into an output
  if (ABLATE & PROBE_PHASES) {
    if (lane == 0) {
      unsigned long long* dbg = prm.dbg + ((size_t)lg * PH_WAVES + w) * PH_WORDS;
      dbg[PH_WAIT] = st_wait;
      dbg[PH_COMPUTE] = st_comp;
      dbg[PH_EPILOGUE] = st_epi;
      dbg[PH_EPI0 + 0] = st_ph[0];
      dbg[PH_EPI0 + 1] = st_ph[1];
      dbg[PH_EPI0 + 2] = st_ph[2];
      dbg[PH_EPI0 + 3] = st_ph[3];
      dbg[PH_SPAN] = st_span;
      dbg[PH_RESTART] = st_restart;
#pragma unroll
      for (int k = 0; k < PH_NSUB; k++) dbg[PH_SUB0 + k] = st_sub[k];
    }
  }
  if (ABLATE & PROBE_TIMELINE) {
    if (tid == 0) {
      KernargPtr kp = kernarg();
      kp->dbg[(size_t)lg * TL_WORDS + TL_EXIT] = __builtin_amdgcn_s_memrealtime();
      kp->dbg[(size_t)lg * TL_WORDS + TL3_EXIT_CYC] = __builtin_amdgcn_s_memtime();
    }
  }
  if (ABLATE & PROBE_CLOCK) {
    if (tid == 0) {
      KernargPtr kp = kernarg();
      unsigned long long* dbg = kp->dbg + (size_t)lg * CLK_WORDS;
      dbg[CLK_END_CYC] = __builtin_amdgcn_s_memtime();
      dbg[CLK_END_RT] = __builtin_amdgcn_s_memrealtime();
    }
  }
}

}  // namespace fused
}  // namespace wino
