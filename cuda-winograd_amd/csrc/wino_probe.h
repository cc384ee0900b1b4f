// The probe vocabulary of the hand-scheduled kernels: the bits of their ABLATE template argument and the layouts of
// the stamp buffers their diagnostic builds write.  Kernel and reader (tools/ablate_fused.hip, tools/ablate_1x1.hip,
// tools/small_timeline.hip, conv3x3_clock_probe in wino_f2_fused.hip) take every bit and every slot from here.
//
// ABLATE = PROBE_OFF is the product kernel.  Any other value is a developer build that prices one part of the kernel
// by leaving it out ("wrong": the outputs are garbage, timing only) or stamps the kernel's progress into a buffer of
// its own (prm.dbg / sk.dbg, never an output; "valid": the outputs are the product's).  3x3 = wino_f2_fused_kernel,
// 1x1 = conv1x1_bn_kernel; the tool modes are the tools' argv letters, "table" the run without one.
//   bit    name              kernels  what it does                                                results  tool mode
//   1      PROBE_NO_DMA_A    3x3 1x1  skip the pixel operand's LDS-DMA (raw patches / A)          wrong    both tables
//   2      PROBE_NO_DMA_B    3x3 1x1  skip the filter operand's LDS-DMA (U / B)                   wrong    both tables
//   4      PROBE_NO_MFMA     3x3 1x1  operands kept live, matrix pipe skipped                     wrong    both tables
//   8      PROBE_NO_SYNC     3x3 1x1  skip the per-stage vmcnt wait + barrier                     wrong    both tables
//   16     PROBE_CLOCK       3x3      s_memtime + s_memrealtime around the main loop (CLK_*)      valid    ablate_fused table, q, w; wino_diag_conv3x3_clock
//   32     PROBE_NO_A_PATH   3x3      skip the patch reads and B^T d B                            wrong    ablate_fused table, h
//   64     PROBE_NO_B_READS  3x3      skip the filter-fragment LDS reads                          wrong    ablate_fused table
//   512    PROBE_NO_STORE    3x3 1x1  skip the output stores and the ring pass                    wrong    both tables
//   1024   PROBE_NO_HANDOFF  3x3      skip the stream-K slab hand-off (partial segments dropped)  wrong    ablate_fused table
//   2048   PROBE_PHASES      3x3      per-wave s_memtime sums of wait / compute / epilogue (PH_*) valid    ablate_fused table
//   4096   PROBE_NO_VPOINT   3x3      B^T d B without its second half (v_point)                   wrong    ablate_fused h
//   8192   PROBE_NO_BTDB     3x3      patch reads only: neither tmp_col nor v_point               wrong    ablate_fused h
//   32768  PROBE_TIMELINE    3x3 1x1  s_memrealtime (100 MHz, chip-wide) at entry, first MFMA,    valid    ablate_fused t, ablate_1x1 t
//                                     start of the last epilogue and exit (TL_*)
// The 3x3 latency kernel (wino_f2_small_kernel) has one probe, its DIAG template argument: the timeline build of
// tools/small_timeline (SM_*, results valid).
#pragma once

namespace wino {

constexpr int PROBE_OFF = 0, PROBE_NO_DMA_A = 1, PROBE_NO_DMA_B = 2, PROBE_NO_MFMA = 4, PROBE_NO_SYNC = 8,
              PROBE_CLOCK = 16, PROBE_NO_A_PATH = 32, PROBE_NO_B_READS = 64, PROBE_NO_STORE = 512,
              PROBE_NO_HANDOFF = 1024, PROBE_PHASES = 2048, PROBE_NO_VPOINT = 4096, PROBE_NO_BTDB = 8192,
              PROBE_TIMELINE = 32768;

// ---- stamp buffers: 64-bit words, [workgroup][slot] ----
// PROBE_TIMELINE: TL_WORDS per workgroup (3x3: logical workgroup lg; 1x1: blockIdx.x).  s_memrealtime at entry, when
// the main loop is about to start (3x3: first MFMA; 1x1: first stage about to be waited for), at the start of the
// last epilogue and at exit; the slots from 4 on differ between the two kernels.
constexpr int TL_WORDS = 8, TL_ENTRY = 0, TL_FIRST = 1, TL_LAST_EPI = 2, TL_EXIT = 3;
constexpr int TL3_ENTRY_CYC = 4, TL3_EXIT_CYC = 5, TL3_STAGE_REQ = 6, TL3_STAGE_IN = 7;   // 3x3: s_memtime at entry / exit; s_memrealtime, first stage requested / landed
constexpr int TL1_HW_ID = 4, TL1_ENTRY_CYC = 5, TL1_EXIT_CYC = 6;   // 1x1: HW_REG_XCC_ID << 32 | HW_REG_HW_ID; s_memtime at entry / exit
// PROBE_CLOCK: CLK_WORDS per logical workgroup, s_memtime (CYC) and s_memrealtime (RT) around its main loop.
constexpr int CLK_WORDS = 4, CLK_BEGIN_CYC = 0, CLK_BEGIN_RT = 1, CLK_END_CYC = 2, CLK_END_RT = 3;
// PROBE_PHASES: PH_WORDS per wave (PH_USED of them written), PH_WAVES waves per logical workgroup; sums of s_memtime
// differences: vmcnt wait + barrier, the rest of the iterations, the epilogues, and of those (PH_EPI0 + 0..3) the
// barrier, A^T m A, slab + ticket, gather + finalize.  The iteration's barrier sits behind the MFMAs of point 0 (steps 0, 1):
// PH_SPAN is the part of PH_COMPUTE from the barrier's release to the last MFMA of step 15, PH_COMPUTE - PH_SPAN what a
// wave runs from there to its arrival at the next barrier (the burst, the loop tail and point 0's 8 MFMAs), PH_RESTART
// the time from a release to the issue of the first MFMA behind it.
// PH_SUB0 + PHS_*: finer stamps inside two of the epilogue phases.  A^T m A = the 16 part() evaluations with their LDS
// writes (PARTS), the pair exchange with its two barriers (EXCHANGE), the accumulators' re-zeroing (ZERO).  Of gather +
// finalize: a gather's slab loads and adds (GATHER), BN + ReLU + the LDS writes of the transpose (BN), the LDS read /
// tile decode / store loop (STORE); what is left of that phase is the hand-off bookkeeping and the ticket's round
// trip.  Each stamp costs an s_memtime and an lgkmcnt(0) wait, so the three parts of A^T m A add up to a little less
// than the (now longer) phase around them: read shares.
constexpr int PH_WORDS = 16, PH_WAVES = 8, PH_USED = 15, PH_WAIT = 0, PH_COMPUTE = 1, PH_EPILOGUE = 2, PH_EPI0 = 3, PH_SPAN = 7,
              PH_SUB0 = 8, PH_NSUB = 6, PH_RESTART = 14;
constexpr int PHS_PARTS = 0, PHS_EXCHANGE = 1, PHS_ZERO = 2, PHS_GATHER = 3, PHS_BN = 4, PHS_STORE = 5;
// DIAG build of the 3x3 latency kernel: SM_WORDS per workgroup, s_memrealtime, in time order (phase i of
// tools/small_timeline is slot i + 1 minus slot i).  A workgroup that does not finish its block stops at SM_TICKET;
// without a C-split (S = 1) SM_SLAB_OUT .. SM_GATHERED are not stamped.
constexpr int SM_WORDS = 8, SM_ENTRY = 0, SM_STAGED = 1, SM_MFMA_DONE = 2, SM_LDS_LEVEL = 3, SM_SLAB_OUT = 4,
              SM_TICKET = 5, SM_GATHERED = 6, SM_EXIT = 7;

}  // namespace wino
