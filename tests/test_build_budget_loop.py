"""What the compiler emits for the main loop of the fused 3x3 throughput kernel, checked at build time (no GPU needed).

The loop's common path is two copies of the body (169 instructions between the first and the last MFMA, plus the 24
packed operations of the next iteration's input transform) and, after each, a tail that only advances the DMA stream's
two scalar offsets, rotates the four filter-fragment bases, steps the filter-stage counter and counts the iteration
down.  Everything rarer -- an item switch of the DMA stream with its per-lane tile decode, the stream's end, the end of
a compute segment -- is an event handled outside that loop.  A wave runs the tail after its
last MFMA of the iteration, when the SIMD's other wave is already waiting at the barrier, so every instruction there is
serial time of the matrix pipe.  This test keeps the walker's state machine from growing back into the loop."""
import pytest

from build_report import compile_report
from isa_analysis import innermost_mfma_loop, loop_counts


@pytest.fixture(scope="module")
def fused_isa():
    return {n: v["body"] for n, v in compile_report("wino_f2_fused.hip").items() if "wino_f2_fused_kernel" in n}


def test_main_loop_holds_only_the_common_path(fused_isa):
    assert len(fused_isa) == 5, sorted(fused_isa)   # as test_fused_kernel_keeps_two_waves_per_simd counts them
    for name, body in fused_isa.items():
        c = loop_counts(innermost_mfma_loop(body))
        print(name, c)
        assert c["readlane"] == 0, (name, c)        # no walker scalar fetched back from a VGPR
        assert c["s_load"] == 0, (name, c)          # no kernel argument re-read
        assert c["tile_decode"] == 0, (name, c)     # the per-lane tile decode of an item switch has left the loop
        assert c["branches"] <= 4, (name, c)        # two exit tests + the back edge (+ one for block layout)
        assert c["instructions"] <= 450, (name, c)  # 2 x (169 + 24) + two tails of at most 30
        assert c["mfma"] == 128 and c["lds_dma"] == 16, (name, c)
