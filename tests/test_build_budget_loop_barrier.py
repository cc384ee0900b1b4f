"""Where the iteration's barrier sits in the main loop of the fused 3x3 throughput kernel, checked at build time (no GPU
needed).

An iteration's vmcnt(0) + barrier lies behind the MFMAs of point 0 (pinned steps 0 and 1, 8 MFMAs per wave), not at the
top of the body: a wave goes from its transform burst and loop tail straight into those MFMAs and reaches the barrier
while they execute.  That is correct only while nothing in front of the barrier needs it: no
LDS-DMA refill may be issued there.  The loop holds two copies of the body; a body's head is the loop's first instruction
or the instruction behind the previous body's last (64th) MFMA.  From the gfx950 disassembly of wino_f2_fused.hip."""
import re

import pytest

from build_report import compile_report
from isa_analysis import bodies, innermost_mfma_loop, instructions

LDS_DMA = re.compile(r"buffer_load_dword\S*\b.*\blds\b")
MFMA_PER_BODY = 64


@pytest.fixture(scope="module")
def fused_loops():
    out = {n: instructions(innermost_mfma_loop(v["body"]))
           for n, v in compile_report("wino_f2_fused.hip").items() if "wino_f2_fused_kernel" in n}
    assert len(out) == 5, sorted(out)
    return out


def test_the_loop_holds_one_barrier_per_body(fused_loops):
    for name, ins in fused_loops.items():
        n = sum(x.startswith("s_barrier") for x in ins)
        assert n == 2, (name, n)
        per_body = [sum(x.startswith("s_barrier") for x in b) for b in bodies(ins, MFMA_PER_BODY)]
        assert per_body == [1, 1], (name, per_body)


def test_point_0_runs_in_front_of_the_barrier(fused_loops):
    for name, ins in fused_loops.items():
        for k, b in enumerate(bodies(ins, MFMA_PER_BODY)):
            at = next(i for i, x in enumerate(b) if x.startswith("s_barrier"))
            front = b[:at]
            n = sum(x.startswith("v_mfma") for x in front)
            print(name, "body", k, ":", n, "MFMAs and", len(front), "instructions in front of the barrier")
            assert n == 8, (name, k, n)


def test_no_lds_dma_in_front_of_the_barrier(fused_loops):
    for name, ins in fused_loops.items():
        total = 0
        for k, b in enumerate(bodies(ins, MFMA_PER_BODY)):
            at = next(i for i, x in enumerate(b) if x.startswith("s_barrier"))
            assert not [x for x in b[:at] if LDS_DMA.match(x)], (name, k)
            total += sum(bool(LDS_DMA.match(x)) for x in b[at:])
        assert total == 16, (name, total)   # ... and all of them behind it


def test_the_barrier_drains_the_vector_memory_counter_only(fused_loops):
    """The wave's own vmcnt(0) stands directly in front of the barrier, and no wait that drains lgkmcnt lies between
    the body's head and the barrier: the fragment requests of steps 0 and 1 stay in flight across it."""
    for name, ins in fused_loops.items():
        for k, b in enumerate(bodies(ins, MFMA_PER_BODY)):
            at = next(i for i, x in enumerate(b) if x.startswith("s_barrier"))
            assert re.match(r"s_waitcnt vmcnt\(0\)$", b[at - 1]), (name, k, b[at - 1])
            drains = [x for x in b[:at] if re.match(r"s_waitcnt\b.*lgkmcnt\(0\)", x)]
            assert not drains, (name, k, drains)
