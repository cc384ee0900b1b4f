// The launch planner of the 3x3 F(2x2,3x3) layers and the wino_conv3x3_*plan* queries that report its answers.
// Host code only: this file instantiates no kernel.  Every launch (wino_f2_launch.h), prepare and the clock probe
// (wino_f2_fused.hip) and the plan queries below read the one plan that plan_3x3 makes: the throughput kernel's grid
// (sk_cost, sk_grid_for) and whether the latency kernel runs instead, and in which form (small_form, small_plan).
#include "wino_f2_launch.h"

using namespace wino;

// Launch geometry of the throughput kernel (see the header of wino_f2_fused_kernel.h): G logical
// workgroups run items / G whole-item rounds and share the remaining items % G items as a
// stream-K tail.  Two candidates are priced with a small cost model, in units of one chunk
// iteration (~2.2 us at 2.3 GHz):
//   * G = items when that fits the CUs: whole items only, no tail, no hand-off;
//   * G = CUs (capped so that a workgroup keeps >= SK_MIN_ITERS iterations);
//   * when all items fit the CUs at once: item-aligned ranges, G = T / s for the shortest divisor
//     s >= 4 of the chunk count whose grid fits -- every workgroup then holds one segment instead
//     of straddling two items (one epilogue, not two).
// Measured on MI355X (N = 128): 256 channels 392 items -> G = 256 (1 round + 17-iteration tail)
// 125 us vs 151 us for two whole-item rounds; 128 channels 196 items -> G = 196, 43 us vs 51 us
// for G = 256 (all tail).  An epilogue costs ~2.3 iterations, the tail's hand-off ~3.2.
constexpr int SK_MIN_ITERS = 8, SK_ALIGNED_MIN_ITERS = 4;
// (hand-off refitted after the loop changes of this round: whole items vs the all-tail grid at 128 / 192 /
//  256 / 384 channels, N = 46..100, solve to 2.7-3.6 iterations; it was 4.8)
constexpr double SK_EPILOGUE_ITERS = 2.3, SK_HANDOFF_ITERS = 3.2, SK_HANDOFF_ALLTAIL_ITERS = 5.0;
static double sk_cost(long long items, int nchunks, long long G) {
  const long long ndp = items / G, tail_items = items % G;
  double c = (double)ndp * (nchunks + SK_EPILOGUE_ITERS);
  if (tail_items) {
    const long long tail_T = tail_items * nchunks, per = (tail_T + G - 1) / G;
    // A range usually straddles two items (two segments, two epilogues).  When the range length
    // divides an item's chunk count and the ranges are all equal, every workgroup holds exactly one
    // segment: one epilogue.  Measured (N = 12..40, 128 channels): 20.6-23.1 us with 4-iteration
    // aligned ranges against 27.3-28.1 with 8-iteration unaligned ones.
    const bool aligned = tail_T % G == 0 && per < nchunks && nchunks % per == 0;
    const double segments = aligned ? 1.0 : (double)((per + nchunks - 1) / nchunks) + 1.0;
    // (an all-tail grid whose ranges straddle items gathers everything at the very end of the launch, on every
    //  workgroup's critical path: re-measured after the ticket rule of round 2 -- 256 channels N = 24 / 32 / 48 / 64
    //  and 128 channels N = 96 solve to 4.1-6.2 iterations, against 2.7-3.2 for aligned ranges and 1.5-3 behind
    //  whole-item rounds; with 5.0 the policy takes the aligned halves at 256 channels N = 32 (45.1 against 48.0 us)
    //  and whole items at N = 64 (72.7 against 75.2) and at 128 channels N = 96 (39.8 against 40.8))
    const double handoff = (!aligned && ndp == 0) ? SK_HANDOFF_ALLTAIL_ITERS : SK_HANDOFF_ITERS;
    c += (double)per + segments * SK_EPILOGUE_ITERS + handoff;
    // (Not modelled: ranges of one or two iterations cut an item into many segments, and whoever gathers it reads
    //  their slabs one after the other.  192 channels, N = 112 -- 258 items on 256 CUs, a 48-iteration tail, 24
    //  segments per item -- takes 119.6 us against 107.1 for two even rounds on 129 workgroups; a per-segment term
    //  that catches this case (0.9-1.0 iterations per segment) mis-prices 128 channels N = 176 and 384 channels
    //  N = 112, where the same kind of tail costs 0.4 per segment and the even rounds lose 16-17 %.  Left as is.)
  }
  return c;
}
static int sk_grid_for(int cus, long long items, int nchunks, const Knobs& kn) {
  const int min_iters = kn.sk_min_iters > 0 ? kn.sk_min_iters : SK_MIN_ITERS;
  const long long T = items * nchunks;
  long long g = cus;
  if (g > T / min_iters) g = T / min_iters;
  if (g < 1) g = 1;
  if (items <= cus && sk_cost(items, nchunks, items) <= sk_cost(items, nchunks, g)) g = items;
  if (items < cus) {
    // item-aligned ranges: the shortest divisor of the chunk count (at least SK_ALIGNED_MIN_ITERS:
    // below that the serial gather of an item's segments outweighs the shorter ranges -- 256 channels
    // N = 5: 2-iteration ranges 29.7 us, 4-iteration ranges 24.5) whose grid fits the CUs
    for (int sl = SK_ALIGNED_MIN_ITERS; sl < nchunks; sl++) {
      if (nchunks % sl) continue;
      const long long ga = T / sl;
      if (ga > cus) continue;
      if (sk_cost(items, nchunks, ga) < sk_cost(items, nchunks, g)) g = ga;
      break;
    }
  }
  if (items > cus) {
    // several rounds: a grid a little below the CU count can make the rounds come out even -- items = r * G
    // exactly: whole items only, no tail, no hand-off (256 channels, N = 160: 492 items = 2 x 246: 138.6 us
    // against 144.2 for G = 256 with a 236-item tail).  Priced with the same model, exact divisions only.
    for (long long gg = cus - 1; gg >= cus - cus / 4 && gg >= 1; gg--)
      if (items % gg == 0 && sk_cost(items, nchunks, gg) < sk_cost(items, nchunks, g)) g = gg;
  }
  if (kn.sk_grid >= 1) g = kn.sk_grid;
  if (g > 16384) g = 16384;   // 2 * G slabs of 64 KB must stay below the 4 GiB a buffer descriptor spans
  return (int)g;
}

// Two kernels, same arithmetic: the throughput kernel (64-tile x 64-out-channel items, 8-wave
// workgroups, whole-item rounds + stream-K tail) and the one-wave-per-SIMD latency kernel (blocks of 16 tiles
// x 16 CT out-channels, CT = 1, 2 or 4; any feature map; wino_f2_small_kernel.h), which wins while its blocks fit
// ONE round of the CUs (a second round of blocks doubles the latency kernel's time at once).
// While the blocks leave CUs idle the latency kernel also splits a block's contraction over S workgroups
// (C-split): S as large as the idle CUs allow (at most 8, and every wave of the S workgroups gets a task in the
// first round: 4 S <= 2 C / 16).
// Among the block widths that fit, the one with the shortest modelled time (small_form below; least squares over the
// forms measured by tools/latency_cases.py explore3, profiles/r3/), and only while that beats the throughput kernel's
// fitted time in this regime, 18.8 us + 0.0174 us x C + 1.94 us x (chunk iterations per CU) (54 points at 64 ... 512
// channels, within 3 us): the latency kernel's price per task grows with C, and from 384 channels on a full round of
// its blocks is the slower launch.
// WINO_3X3_ALGO=big|small, WINO_SMALL_SPLIT, WINO_SMALL_CT override.
// T = 5.70 us + rounds x (0.487 + (0.509 + 0.229 fill) CT) us + split cost: a round is 8 whole-line pixel loads per wave
// (the workgroup's 32, shared through LDS) and 8 CT filter-fragment loads; fill = workgroups / CUs; the split cost (slab
// round trip, growing with the block) 0.4 / 1.2 / 4.5 us at CT = 1 / 2 / 4.  148 measured forms, rms 0.85 us.
constexpr double SMALL_T0 = 5.70, SMALL_ROUND = 0.487, SMALL_FLT = 0.509, SMALL_FLT_FILL = 0.2285;
// The block width ct on `cus` CUs: its blocks and the C-split.  false if its blocks do not fit one round.
static bool small_form(int N, int tiles, int C, int K, int cus, int ct, SmallPlan* pl) {
  if ((K % (16 * ct)) != 0) return false;
  pl->ct = ct;
  pl->nT16 = (int)(((long long)N * tiles + 15) / 16);
  const long long blocks = (long long)pl->nT16 * (K / (16 * ct));
  pl->blocks = (size_t)blocks;
  pl->split = 1;
  pl->t_us = 0;
  if (blocks > cus) return false;
  const int ntask = (C / 16) * 2;
  int sp = (int)(cus / blocks);
  if (sp > SMALL_MAX_SPLIT) sp = SMALL_MAX_SPLIT;
  while (sp > 1 && SMALL_WAVES * sp > ntask) sp--;
  pl->split = sp;
  const int waves = SMALL_WAVES * sp;
  const double fill = (double)(blocks * sp) / cus;
  const double split_us = sp > 1 ? (ct == 1 ? 0.38 : ct == 2 ? 1.21 : 4.45) : 0.0;
  pl->t_us = SMALL_T0 + (double)((ntask + waves - 1) / waves) * (SMALL_ROUND + (SMALL_FLT + SMALL_FLT_FILL * fill) * ct) + split_us;
  return true;
}
static SmallPlan small_plan(int N, int H, int W, int C, int K, int cus, const Knobs& kn) {
  SmallPlan pl = {false, 1, 0, 0, 1, 0.0};
  if ((C % 16) != 0 || H < 1 || W < 1) return pl;
  const long long tiles_ll = (long long)((H + 1) / 2) * ((W + 1) / 2);
  if (tiles_ll * N > (1ll << 30)) return pl;
  const int tiles = (int)tiles_ll;
  if (kn.small3_ct == 1 || kn.small3_ct == 2 || kn.small3_ct == 4) {
    pl.use = small_form(N, tiles, C, K, cus, kn.small3_ct, &pl);
  } else {
    SmallPlan best = pl;
    for (int ct = 1; ct <= 4; ct *= 2) {
      SmallPlan f = pl;
      if (small_form(N, tiles, C, K, cus, ct, &f) && (!best.use || f.t_us < best.t_us)) { best = f; best.use = true; }
    }
    const double items = (double)(((long long)N * tiles + TB - 1) / TB) * (K / KB);
    const double t_big = 18.8 + 0.0174 * C + 1.94 * items * (C / BC) / cus;
    if (best.use && 1.08 * best.t_us < t_big) pl = best;   // (the margin: the model is 2-3 us short on a full round of wide blocks)
    else small_form(N, tiles, C, K, cus, 1, &pl), pl.use = false;   // (the counts a forced launch would use)
  }
  if (kn.algo_3x3 == 1) pl.use = false;
  if (kn.algo_3x3 == 2) pl.use = pl.nT16 <= 65535 && (K % (16 * pl.ct)) == 0;
  if (!pl.use) return pl;
  if (kn.small_split >= 1 && kn.small_split <= SMALL_MAX_SPLIT) pl.split = kn.small_split;
  return pl;
}

Plan3x3 wino::plan_3x3(int N, int H, int W, int C, int K, int cus, const Knobs& kn, bool throughput) {
  Plan3x3 p{};
  const unsigned tiles_x = (unsigned)((W + 1) / 2), tiles = (unsigned)((H + 1) / 2) * tiles_x;
  p.geo = {H + 2, W + 2, tiles, tiles_x, make_fastdiv(tiles), make_fastdiv(tiles_x)};
  p.small = small_plan(N, H, W, C, K, cus, kn);
  if (p.small.use && !throughput) return p;
  const int nTB = (int)(((long long)N * tiles + TB - 1) / TB);
  p.items = (long long)nTB * (K / KB);
  p.G = sk_grid_for(cus, p.items, C / BC, kn);
  p.fp.N = N, p.fp.C = C, p.fp.K = K, p.fp.nTB = nTB, p.fp.geo = p.geo;
  fused_work_layout(p.fp, p.items, p.G);
  return p;
}

int wino::check_conv3x3_dims(int H, int W, int C, int K) {
  if (int rc = check_ck(C, K)) return rc;
  if (H < 1 || W < 1 || H > 4094 || W > 4094) {
    set_error("unsupported feature map %dx%d", H, W);
    return WINO_E_SHAPE;
  }
  // U [16][C][K] goes through one buffer descriptor in the throughput kernel (32-bit size and offsets); the latency
  // kernel could address more, but both take the same shapes (one plan per shape)
  const unsigned long long u_bytes = (unsigned long long)16 * C * K * sizeof(float);
  if (u_bytes >= FOUR_GIB) {
    set_error("C=%d K=%d: the filter matrix U (16 x C x K floats, %llu bytes) must stay below 4 GiB (C * K < 2^26)", C,
              K, u_bytes);
    return WINO_E_SHAPE;
  }
  if (conv3x3_batch_limit(H, W, C, K) < 1) {
    set_error("%dx%d C=%d K=%d: one image does not fit a launch (tensors must stay below 4 GiB)", H, W, C, K);
    return WINO_E_SHAPE;
  }
  return WINO_OK;
}

int wino::plan_3x3_here(int N, int H, int W, int C, int K, bool throughput, int* dev, Plan3x3* p) {
  int cus = 0;
  if (int rc = current_device(dev, &cus)) return rc;
  *p = plan_3x3(N, H, W, C, K, cus, knobs(), throughput);
  return WINO_OK;
}

// the plan of a wino_conv3x3_*plan* query
static int plan_query(int N, int H, int W, int C, int K, int cus, Plan3x3* p) {
  if (int rc = check_conv3x3(N, H, W, C, K)) return rc;
  *p = plan_3x3(N, H, W, C, K, cus, knobs(), true);
  return WINO_OK;
}

extern "C" {

int wino_conv3x3_plan(int N, int H, int W, int C, int K, int cus, int* grid, int* rounds, long* tail_iters,
                      int* iters_per_item) {
  if (!grid || !rounds || !tail_iters || !iters_per_item || cus < 1) { set_error("bad argument"); return WINO_E_ARG; }
  Plan3x3 p;
  if (int rc = plan_query(N, H, W, C, K, cus, &p)) return rc;
  *grid = p.G;
  *rounds = p.fp.ndp;
  *tail_iters = (long)((p.items % p.G) * (C / BC));
  *iters_per_item = C / BC;
  return WINO_OK;
}

// Host-side only: does this shape take the latency kernel on a device with `cus` CUs, and in which form.
int wino_conv3x3_small_plan2(int N, int H, int W, int C, int K, int cus, int* use, int* point_rows, int* split,
                             int* col_tiles, int* workgroups) {
  if (!use || !point_rows || !split || !col_tiles || !workgroups || cus < 1) { set_error("bad argument"); return WINO_E_ARG; }
  Plan3x3 p;
  if (int rc = plan_query(N, H, W, C, K, cus, &p)) return rc;
  *use = p.small.use;
  *point_rows = 2;
  *split = p.small.split;
  *col_tiles = p.small.ct;
  *workgroups = p.small.use ? (int)(p.small.blocks * p.small.split) : 0;
  return WINO_OK;
}

int wino_conv3x3_small_plan(int N, int H, int W, int C, int K, int cus, int* use, int* point_rows, int* split,
                            int* workgroups) {
  int ct = 0;
  return wino_conv3x3_small_plan2(N, H, W, C, K, cus, use, point_rows, split, &ct, workgroups);
}

// Host-side only: into how many k-groups the launch wino_conv3x3_plan describes cuts its tail (1 = one item-major
// list).  Group k owns the tail items of out-channel block k, item rounds*grid + groups*j + k for j = 0, 1, ...;
// its tail_iters / groups iterations are cut into Gp = grid / groups equal ranges [r*T/Gp, (r+1)*T/Gp), and the
// workgroup l = groups*j + k at position j runs range r = (phase_inv * (j / phase_copies)) % phase_period +
// phase_period * (j % phase_copies) -- the ranges of one XCD's workgroups start at consecutive channel phases.
int wino_conv3x3_plan_groups(int N, int H, int W, int C, int K, int cus, int* groups, int* phase_period, int* phase_inv,
                             int* phase_copies) {
  if (!groups || !phase_period || !phase_inv || !phase_copies || cus < 1) { set_error("bad argument"); return WINO_E_ARG; }
  Plan3x3 p;
  if (int rc = plan_query(N, H, W, C, K, cus, &p)) return rc;
  *groups = p.fp.kp;
  *phase_period = p.fp.ph_P;
  *phase_inv = p.fp.ph_inv;
  *phase_copies = p.fp.ph_copies;
  return WINO_OK;
}

}  // extern "C"
