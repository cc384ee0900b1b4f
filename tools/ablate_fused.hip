// Developer tool: prices the parts of the fused Winograd kernel by timing ablated variants
// (ABLATE; the probe bits and stamp layouts are csrc/wino_probe.h).  Not part of the library.
//   hipcc --offload-arch=gfx950 -O3 -Iinclude -Icuda-winograd_amd/csrc tools/ablate_fused.hip -o tools/ablate_fused
#include "wino_f2_fused_kernel.h"

#include <cstdlib>
#include <algorithm>
#include <vector>

namespace wino { void set_error(const char*, ...) {} int hip_fail(hipError_t, const char*) { return -1; } }
using namespace wino;
using namespace wino::fused;

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

static float* g_slabs;
static unsigned* g_tickets;
static unsigned long long* g_dbg;   // stamps of the diagnostic builds
static unsigned* g_err;              // the library's dirty-counter word (device memory here)
// the table's combinations
constexpr int NO_DMA = PROBE_NO_DMA_A | PROBE_NO_DMA_B, NO_AB = PROBE_NO_A_PATH | PROBE_NO_B_READS, NO_OUT = PROBE_NO_STORE | PROBE_NO_HANDOFF;
static int g_grid = 256;   // logical workgroups (argv[2]); 0 = one whole item per workgroup

static int grid_for(int N, int K) {
  const int nTB = (N * 49 + TB - 1) / TB;
  if (g_grid) return g_grid;
  return nTB * (K / KB);   // one whole item per workgroup
}

template <int AB>
float run(const float* in, const float* U, const float* b, const float* s, float* out, int N, int C, int K, int reps) {
  CK(hipFuncSetAttribute((const void*)(wino_f2_fused_kernel<AB>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
  const int nTB = (N * 49 + TB - 1) / TB;
  const int grid = grid_for(N, K);
  CK(hipMemset(g_tickets, 0, 65536 * 4));   // ablated variants may leave tickets behind
  FusedParams prm{};
  prm.in = in, prm.Uq = U, prm.N = N, prm.C = C, prm.K = K, prm.relu = 1, prm.nTB = nTB;
  prm.bnBias = b, prm.bnScale = s, prm.out = out, prm.slabs = g_slabs, prm.tickets = g_tickets, prm.err = g_err, prm.dbg = g_dbg;
  fused_work_layout(prm, (long long)nTB * (K / KB), grid);   // the library's rounds and tail placement
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  for (int i = 0; i < 5; i++)
    hipLaunchKernelGGL((wino_f2_fused_kernel<AB>), dim3(grid), dim3(NTHREADS), LDS_BYTES, 0, prm);
  CK(hipDeviceSynchronize());
  CK(hipEventRecord(e0));
  for (int i = 0; i < reps; i++)
    hipLaunchKernelGGL((wino_f2_fused_kernel<AB>), dim3(grid), dim3(NTHREADS), LDS_BYTES, 0, prm);
  CK(hipEventRecord(e1));
  CK(hipEventSynchronize(e1));
  float ms;
  CK(hipEventElapsedTime(&ms, e0, e1));
  return ms * 1000.f / reps;
}

int main(int argc, char** argv) {
  const int C = argc > 1 ? atoi(argv[1]) : 256, K = C;
  if (argc > 2) g_grid = atoi(argv[2]);
  CK(hipMalloc(&g_slabs, (size_t)2 * 4096 * SLAB_BYTES));
  CK(hipMalloc(&g_tickets, 65536 * 4));
  CK(hipMalloc(&g_dbg, (size_t)4096 * 64 * 8));
  CK(hipMalloc(&g_err, 64));
  CK(hipMemset(g_err, 0, 64));
  std::vector<int> Ns = {1, 83, 128};
  const size_t maxN = 256;
  float *in, *U, *b, *s, *out;
  CK(hipMalloc(&in, maxN * 256 * C * 4)); CK(hipMalloc(&out, maxN * 256 * K * 4));
  CK(hipMalloc(&U, (size_t)16 * C * K * 4)); CK(hipMalloc(&b, K * 4)); CK(hipMalloc(&s, K * 4));
  std::vector<float> h(maxN * 256 * C);
  for (auto& x : h) x = (float)rand() / RAND_MAX - 0.5f;
  CK(hipMemcpy(in, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(U, h.data(), (size_t)16 * C * K * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(b, h.data(), K * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(s, h.data() + K, K * 4, hipMemcpyHostToDevice));
  if (argc > 3 && argv[3][0] == 'w') {  // per-workgroup pass times of the stamped build, with each range's shape
    const int N = 128;
    run<PROBE_OFF>(in, U, b, s, out, N, C, K, 3000);
    const int nTB = (N * 49 + TB - 1) / TB, wgs = grid_for(N, K), nch = C / 8;
    const unsigned items = (unsigned)nTB * (K / KB), ndp = items / wgs, Tt = (items % wgs) * nch, q = Tt / wgs, rem = Tt % wgs;
    run<PROBE_CLOCK>(in, U, b, s, out, N, C, K, 20);
    std::vector<unsigned long long> st((size_t)wgs * CLK_WORDS);
    CK(hipMemcpy(st.data(), g_dbg, st.size() * 8, hipMemcpyDeviceToHost));
    printf("lg cycles tail_begin tail_len segments(tail) straddles\n");
    for (int l = 0; l < wgs; l++) {
      const unsigned t0 = sk_start(l, q, rem, wgs), t1 = sk_start(l + 1, q, rem, wgs);
      const int segs = t1 > t0 ? (int)((t1 - 1) / nch - t0 / nch + 1) : 0;
      printf("%d %llu %u %u %d %d ndp=%u\n", l, st[CLK_WORDS * l + CLK_END_CYC] - st[CLK_WORDS * l + CLK_BEGIN_CYC], t0, t1 - t0, segs, (int)(t0 % nch != 0) + (int)(t1 % nch != 0), ndp);
    }
    return 0;
  }
  if (argc > 3 && argv[3][0] == 't') {   // timeline: where a launch's wall time goes (chip-wide 100 MHz stamps)
    const int N = argc > 4 ? atoi(argv[4]) : 128;
    run<PROBE_OFF>(in, U, b, s, out, N, C, K, 3000);
    const float us_prod = run<PROBE_OFF>(in, U, b, s, out, N, C, K, 200);
    const float us_tl = run<PROBE_TIMELINE>(in, U, b, s, out, N, C, K, 200);   // the stamps of the LAST of 200 back-to-back launches stay
    const int wgs = grid_for(N, K);
    std::vector<unsigned long long> st((size_t)wgs * TL_WORDS);
    auto tl = [&](int l, int slot) { return st[(size_t)TL_WORDS * l + slot]; };
    CK(hipMemcpy(st.data(), g_dbg, st.size() * 8, hipMemcpyDeviceToHost));
    unsigned long long t0 = ~0ull, tend = 0;
    std::vector<double> entry, first, lastep, exitt, pro, epi;
    for (int l = 0; l < wgs; l++) { t0 = std::min(t0, tl(l, TL_ENTRY)); tend = std::max(tend, tl(l, TL_EXIT)); }
    for (int l = 0; l < wgs; l++) {
      entry.push_back((tl(l, TL_ENTRY) - t0) * 0.01); first.push_back((tl(l, TL_FIRST) - t0) * 0.01);
      lastep.push_back((tl(l, TL_LAST_EPI) - t0) * 0.01); exitt.push_back((tl(l, TL_EXIT) - t0) * 0.01);
      pro.push_back((tl(l, TL_FIRST) - tl(l, TL_ENTRY)) * 0.01); epi.push_back((tl(l, TL_EXIT) - tl(l, TL_LAST_EPI)) * 0.01);
    }
    auto pr = [&](const char* name, std::vector<double> v) {
      std::sort(v.begin(), v.end());
      printf("  %-34s min %7.2f  p10 %7.2f  median %7.2f  p90 %7.2f  max %7.2f us\n", name, v[0], v[v.size() / 10], v[v.size() / 2], v[v.size() * 9 / 10], v.back());
    };
    printf("%s C=%d N=%d grid=%d: product %.2f us per launch, timeline build %.2f; first entry -> last exit %.2f us (10 ns ticks)\n", argv[0], C, N, wgs, us_prod, us_tl, (tend - t0) * 0.01);
    pr("entry (after the first entry)", entry); pr("first MFMA", first); pr("start of the last epilogue", lastep); pr("exit", exitt);
    pr("entry -> first MFMA", pro); pr("last epilogue -> exit", epi);
    {
      std::vector<double> req, land;
      for (int l = 0; l < wgs; l++) { req.push_back((tl(l, TL3_STAGE_REQ) - tl(l, TL_ENTRY)) * 0.01); land.push_back((tl(l, TL3_STAGE_IN) - tl(l, TL_ENTRY)) * 0.01); }
      pr("entry -> first stage requested", req); pr("entry -> first stage landed", land);
    }
    if (argc > 5) {   // per workgroup, with the shape of its tail range: the launch's real cut (k-groups, phase order)
      const int nTB = (N * 49 + TB - 1) / TB, nch = C / 8;
      FusedParams lay{};
      lay.C = C, lay.K = K;
      fused_work_layout(lay, (long long)nTB * (K / KB), wgs);
      std::vector<double> cls[2][3];   // [one-segment range / straddler][last epilogue start, its length, exit]
      printf("lg range first_chunk len segs | first_mfma last_epi_start exit epi_len\n");
      for (int l = 0; l < wgs; l++) {
        const int lp = tail_range_of(l / lay.kp, lay.ph_P, lay.ph_inv, lay.ph_copies);
        const unsigned a = sk_start(lp, lay.sk_q, lay.sk_rem, lay.Gp), b2 = sk_start(lp + 1, lay.sk_q, lay.sk_rem, lay.Gp);
        const int segs = b2 > a ? (int)((b2 - 1) / nch - a / nch + 1) : 0;
        printf("%3d %3d %2u %2u %d | %6.2f %7.2f %7.2f %5.2f\n", l, lp, a % nch, b2 - a, segs, first[l], lastep[l], exitt[l], epi[l]);
        if (segs == 1 || segs == 2) { cls[segs - 1][0].push_back(lastep[l]); cls[segs - 1][1].push_back(epi[l]); cls[segs - 1][2].push_back(exitt[l]); }
      }
      for (int c = 0; c < 2; c++) {
        if (cls[c][0].empty()) continue;
        printf("%s (%zu workgroups):\n", c ? "straddlers (two tail segments)" : "one-segment ranges", cls[c][0].size());
        pr("start of the last epilogue", cls[c][0]); pr("last epilogue -> exit", cls[c][1]); pr("exit", cls[c][2]);
      }
    }
    return 0;
  }
  if (argc > 3 && argv[3][0] == 'h') {   // timing only: what the parts of the A path cost
    run<PROBE_OFF>(in, U, b, s, out, 128, C, K, 3000);
    for (int i = 0; i < 3; i++)
      printf("full %.1f   no v_point %.1f   no tmp_col + v_point (reads only) %.1f   no A path %.1f us\n", run<PROBE_OFF>(in, U, b, s, out, 128, C, K, 200),
             run<PROBE_NO_VPOINT>(in, U, b, s, out, 128, C, K, 200), run<PROBE_NO_BTDB>(in, U, b, s, out, 128, C, K, 200), run<PROBE_NO_A_PATH>(in, U, b, s, out, 128, C, K, 200));
    return 0;
  }
  if (argc > 3 && argv[3][0] == 'q') {  // quick mode: just the product kernel at N = 128, three trials of 50 launches
    run<PROBE_OFF>(in, U, b, s, out, 128, C, K, 3000);   // clock ramp: ~0.4 s of the same kernel (see bench.py, preheat)
    float t[3];
    for (int i = 0; i < 3; i++) t[i] = run<PROBE_OFF>(in, U, b, s, out, 128, C, K, 200);
    std::sort(t, t + 3);
    const int nTB = (128 * 49 + TB - 1) / TB, wgs = grid_for(128, K);
    const double iters = (double)nTB * (K / KB) * (C / 8) / wgs;
    run<PROBE_CLOCK>(in, U, b, s, out, 128, C, K, 3);
    std::vector<unsigned long long> st((size_t)wgs * CLK_WORDS);
    CK(hipMemcpy(st.data(), g_dbg, st.size() * 8, hipMemcpyDeviceToHost));
    double cyc = 0, rt = 0, cmax = 0;
    auto ck = [&](int i, int slot) { return st[(size_t)CLK_WORDS * i + slot]; };
    for (int i = 0; i < wgs; i++) { const double c = (double)(ck(i, CLK_END_CYC) - ck(i, CLK_BEGIN_CYC)); cyc += c; rt += (double)(ck(i, CLK_END_RT) - ck(i, CLK_BEGIN_RT)); cmax = std::max(cmax, c); }
    printf("%s C=%d grid=%d: %.1f / %.1f / %.1f us   loop+epilogues: %.1f cycles per MFMA per SIMD (slowest workgroup %.1f) at %.3f GHz\n",
           argv[0], C, wgs, t[0], t[1], t[2], cyc / wgs / iters / 128.0, cmax / iters / 128.0, cyc / rt * 0.1);
    return 0;
  }
  printf("C=K=%d   us per launch; items = K/64 * ceil(N*49/64); grid = %d logical workgroups (0: one item each)\n", C, g_grid);
  printf("%6s %6s %6s | %8s %8s %8s %8s %8s %8s %8s %8s %8s %8s\n", "N", "items", "grid", "full", "noRawDMA", "noUDMA", "noDMA", "noMFMA",
         "noBarr", "noStore", "noSlab", "noA", "noB");
  for (int N : Ns) {
    const int items = (K / 64) * ((N * 49 + 63) / 64);
    printf("%6d %6d %6d | %8.1f %8.1f %8.1f %8.1f %8.1f %8.1f %8.1f %8.1f %8.1f %8.1f\n", N, items, grid_for(N, K),
           run<PROBE_OFF>(in, U, b, s, out, N, C, K, 20), run<PROBE_NO_DMA_A>(in, U, b, s, out, N, C, K, 20),
           run<PROBE_NO_DMA_B>(in, U, b, s, out, N, C, K, 20), run<NO_DMA>(in, U, b, s, out, N, C, K, 20),
           run<PROBE_NO_MFMA>(in, U, b, s, out, N, C, K, 20), run<PROBE_NO_SYNC>(in, U, b, s, out, N, C, K, 20),
           run<PROBE_NO_STORE>(in, U, b, s, out, N, C, K, 20), run<PROBE_NO_HANDOFF>(in, U, b, s, out, N, C, K, 20),
           run<PROBE_NO_A_PATH>(in, U, b, s, out, N, C, K, 20), run<PROBE_NO_B_READS>(in, U, b, s, out, N, C, K, 20));
  }
  {  // what the non-MFMA side costs on its own (N = 128): everything below skips the MFMAs
    const int N = 128;
    printf("noMFMA and ... : alone %.1f  noDMA %.1f  noBarr %.1f  noA %.1f  noB %.1f  noA+noB %.1f  noDMA+noA+noB %.1f  noDMA+noBarr+noA+noB %.1f  +noStore+noSlab %.1f\n",
           run<PROBE_NO_MFMA>(in, U, b, s, out, N, C, K, 20), run<PROBE_NO_MFMA | NO_DMA>(in, U, b, s, out, N, C, K, 20), run<PROBE_NO_MFMA | PROBE_NO_SYNC>(in, U, b, s, out, N, C, K, 20),
           run<PROBE_NO_MFMA | PROBE_NO_A_PATH>(in, U, b, s, out, N, C, K, 20), run<PROBE_NO_MFMA | PROBE_NO_B_READS>(in, U, b, s, out, N, C, K, 20), run<PROBE_NO_MFMA | NO_AB>(in, U, b, s, out, N, C, K, 20),
           run<PROBE_NO_MFMA | NO_AB | NO_DMA>(in, U, b, s, out, N, C, K, 20), run<PROBE_NO_MFMA | NO_AB | NO_DMA | PROBE_NO_SYNC>(in, U, b, s, out, N, C, K, 20),
           run<PROBE_NO_MFMA | NO_AB | NO_DMA | PROBE_NO_SYNC | NO_OUT>(in, U, b, s, out, N, C, K, 20));
    printf("MFMA and ...   : noDMA+noBarr %.1f  noDMA+noBarr+noA+noB %.1f  +noStore+noSlab %.1f\n",
           run<NO_DMA | PROBE_NO_SYNC>(in, U, b, s, out, N, C, K, 20), run<NO_DMA | PROBE_NO_SYNC | NO_AB>(in, U, b, s, out, N, C, K, 20),
           run<NO_DMA | PROBE_NO_SYNC | NO_AB | NO_OUT>(in, U, b, s, out, N, C, K, 20));
  }
  {  // in-kernel clock of the main loop (diagnostic build, PROBE_CLOCK)
    const int N = 128;
    const int nTB = (N * 49 + TB - 1) / TB, wgs = grid_for(N, K);
    const double iters = (double)nTB * (K / KB) * (C / 8) / wgs;   // chunk iterations per workgroup
    run<PROBE_CLOCK>(in, U, b, s, out, N, C, K, 3);
    std::vector<unsigned long long> st((size_t)wgs * CLK_WORDS);
    CK(hipMemcpy(st.data(), g_dbg, st.size() * 8, hipMemcpyDeviceToHost));
    double cyc = 0, rt = 0, cmin = 1e30, cmax = 0;
    auto ck = [&](int i, int slot) { return st[(size_t)CLK_WORDS * i + slot]; };
    for (int i = 0; i < wgs; i++) { const double c = (double)(ck(i, CLK_END_CYC) - ck(i, CLK_BEGIN_CYC)); cyc += c; rt += (double)(ck(i, CLK_END_RT) - ck(i, CLK_BEGIN_RT)); cmin = std::min(cmin, c); cmax = std::max(cmax, c); }
    printf("main loop, N=128: in-kernel clock %.3f GHz; cycles per WG pass mean %.0f min %.0f max %.0f (= %.1f cycles per MFMA per SIMD)\n",
           cyc / rt * 0.1, cyc / wgs, cmin, cmax, cyc / wgs / iters / 128.0);
  }
  {  // per-wave phase stamps (PROBE_PHASES): barrier+DMA wait vs compute, in shader cycles
    const int N = 128;
    const int nTB = (N * 49 + TB - 1) / TB, wgs = grid_for(N, K);
    const double iters = (double)nTB * (K / KB) * (C / 8) / wgs;
    run<PROBE_PHASES>(in, U, b, s, out, N, C, K, 2);
    std::vector<unsigned long long> st((size_t)wgs * PH_WAVES * PH_WORDS);
    CK(hipMemcpy(st.data(), g_dbg, st.size() * 8, hipMemcpyDeviceToHost));
    double sum[PH_WAVES][PH_USED] = {{0}};
    for (int i = 0; i < wgs; i++) for (int w = 0; w < PH_WAVES; w++) for (int k = 0; k < PH_USED; k++) sum[w][k] += st[((size_t)i * PH_WAVES + w) * PH_WORDS + k];
    printf("per chunk iteration (%.2f per workgroup), mean over %d workgroups; stamps add overhead, read the SHARES:\n", iters, wgs);
    for (int w = 0; w < PH_WAVES; w++)
      printf("  wave %d: wait(vmcnt+barrier) %6.0f  compute %6.0f cycles per iteration (wait share %4.1f%%) | epilogues per workgroup %7.0f cycles = barrier %6.0f + AtmA %6.0f + slab/ticket %6.0f + gather/finalize %6.0f\n", w,
             sum[w][PH_WAIT] / wgs / iters, sum[w][PH_COMPUTE] / wgs / iters, 100.0 * sum[w][PH_WAIT] / (sum[w][PH_WAIT] + sum[w][PH_COMPUTE]), sum[w][PH_EPILOGUE] / wgs,
             sum[w][PH_EPI0 + 0] / wgs, sum[w][PH_EPI0 + 1] / wgs, sum[w][PH_EPI0 + 2] / wgs, sum[w][PH_EPI0 + 3] / wgs);
    // the finer epilogue stamps (PHS_*), per wave class: the parts of A^T m A and of gather + finalize, cycles per workgroup
    for (int c = 0; c < 2; c++) {
      double sub[PH_NSUB] = {0}, atma = 0, fin = 0;
      for (int w = 4 * c; w < 4 * c + 4; w++) {
        for (int k = 0; k < PH_NSUB; k++) sub[k] += sum[w][PH_SUB0 + k] / (4.0 * wgs);
        atma += sum[w][PH_EPI0 + 1] / (4.0 * wgs); fin += sum[w][PH_EPI0 + 3] / (4.0 * wgs);
      }
      printf("  waves %d-%d: AtmA %6.0f = parts %6.0f + exchange (2 barriers) %6.0f + re-zeroing %6.0f | gather/finalize %6.0f = slab loads+adds %6.0f + BN/ReLU/LDS writes %6.0f"
             " + LDS read/decode/store %6.0f + bookkeeping, ticket wait %6.0f cycles per workgroup\n",
             4 * c, 4 * c + 3, atma, sub[PHS_PARTS], sub[PHS_EXCHANGE], sub[PHS_ZERO], fin, sub[PHS_GATHER], sub[PHS_BN], sub[PHS_STORE],
             fin - sub[PHS_GATHER] - sub[PHS_BN] - sub[PHS_STORE]);
    }
    // where an iteration's compute part ends: barrier release -> last MFMA of step 15 (the MFMA span), from there to the
    // arrival at the next barrier (transform burst, DMA walker, loop control and the 8 MFMAs of point 0, which run in
    // front of the barrier), arrival -> release, release -> first MFMA behind it; per wave class (waves 0-3 / 4-7)
    for (int c = 0; c < 2; c++) {
      double span = 0, comp = 0, wait = 0, restart = 0;
      for (int w = 4 * c; w < 4 * c + 4; w++) { span += sum[w][PH_SPAN]; comp += sum[w][PH_COMPUTE]; wait += sum[w][PH_WAIT]; restart += sum[w][PH_RESTART]; }
      const double d = 4.0 * wgs * iters;
      printf("  waves %d-%d: MFMA span %6.0f  step 15's last MFMA -> barrier arrival %6.0f  arrival -> release %6.0f  release -> first MFMA %6.0f cycles per iteration\n",
             4 * c, 4 * c + 3, span / d, (comp - span) / d, wait / d, restart / d);
    }
  }
  return 0;
}
