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

BRANCH = re.compile(r"^\s+s_c?branch\S*\s+(\.LBB\d+_\d+)")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
LDS_DMA = re.compile(r"buffer_load_dword\S*\b.*\blds\b")
MFMA_PER_BODY = 64


def _is_instruction(line):
    s = line.strip()
    return bool(s) and line[0] in " \t" and not s.startswith((".", ";")) and not s.endswith(":")


def _blocks(body):
    """Basic blocks of one kernel's lines and their successor lists."""
    blocks, cur = [], []
    for line in body:
        if LABEL.match(line) and cur:
            blocks.append(cur)
            cur = []
        cur.append(line)
        if _is_instruction(line) and re.match(r"s_c?branch|s_endpgm|s_setpc", line.strip()):
            blocks.append(cur)
            cur = []
    if cur:
        blocks.append(cur)
    where = {LABEL.match(b[0]).group(1): i for i, b in enumerate(blocks) if LABEL.match(b[0])}
    succ = []
    for i, b in enumerate(blocks):
        last = next((x.strip() for x in reversed(b) if _is_instruction(x)), "")
        m = BRANCH.match("\t" + last)
        out = [where[m.group(1)]] if m else []
        if not re.match(r"s_branch|s_endpgm|s_setpc", last) and i + 1 < len(blocks):
            out.append(i + 1)
        succ.append(out)
    return blocks, succ


def _reach(start, succ, nodes):
    seen, todo = set(), [start]
    while todo:
        v = todo.pop()
        for w in succ[v]:
            if w in nodes and w not in seen:
                seen.add(w)
                todo.append(w)
    return seen


def innermost_mfma_loop(body):
    """The instructions, in layout order, of the innermost loop that holds MFMAs: the smallest set of blocks that is
    strongly connected and holds an MFMA block, found by shrinking from the whole kernel -- a loop's inner loops are what
    stays strongly connected once the edges into its entry blocks are cut."""
    blocks, succ = _blocks(body)
    hot = {i for i, b in enumerate(blocks) if any("v_mfma" in x for x in b)}
    nodes, loop = set(range(len(blocks))), None
    while True:
        comps = []
        for h in sorted(hot & nodes):
            if any(h in c for c in comps):
                continue
            fwd = _reach(h, succ, nodes)
            if h not in fwd:
                continue   # on no cycle
            comps.append({v for v in fwd if h in _reach(v, succ, nodes)})
        if not comps:
            break
        assert len(comps) == 1, [sorted(c) for c in comps]
        loop = comps[0]
        pred_outside = {j for i, out in enumerate(succ) if i not in loop for j in out}
        entries = (loop & pred_outside) or {min(loop)}
        succ = [[j for j in out if not (i in loop and j in entries)] for i, out in enumerate(succ)]
        nodes = loop
    assert loop is not None
    return [x.strip() for i in sorted(loop) for x in blocks[i] if _is_instruction(x)]


def bodies(ins):
    """The loop's instructions cut into bodies: each ends with its 64th MFMA (what follows the last one -- the second
    tail -- is dropped)."""
    out, cur, n = [], [], 0
    for x in ins:
        cur.append(x)
        if x.startswith("v_mfma"):
            n += 1
            if n == MFMA_PER_BODY:
                out.append(cur)
                cur, n = [], 0
    return out


@pytest.fixture(scope="module")
def fused_loops(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fused_loop_barrier")
    kernels = [n for n in compile_report("wino_f2_fused.hip", tmp) if "wino_f2_fused_kernel" in n]
    isa = [f for f in tmp.iterdir() if f.name.endswith(".s") and "gfx950" in f.name]
    assert len(isa) == 1, isa
    text = isa[0].read_text()
    out = {}
    for name in kernels:
        i = text.index(name + ":")
        out[name] = innermost_mfma_loop(text[i:text.index(".Lfunc_end", i)].splitlines())
    assert len(out) == 5, sorted(out)
    return out


def test_the_loop_holds_one_barrier_per_body(fused_loops):
    for name, ins in fused_loops.items():
        n = sum(x.startswith("s_barrier") for x in ins)
        assert n == 2, (name, n)
        per_body = [sum(x.startswith("s_barrier") for x in b) for b in bodies(ins)]
        assert per_body == [1, 1], (name, per_body)


def test_point_0_runs_in_front_of_the_barrier(fused_loops):
    for name, ins in fused_loops.items():
        for k, b in enumerate(bodies(ins)):
            at = next(i for i, x in enumerate(b) if x.startswith("s_barrier"))
            front = b[:at]
            n = sum(x.startswith("v_mfma") for x in front)
            print(name, "body", k, ":", n, "MFMAs and", len(front), "instructions in front of the barrier")
            assert n == 8, (name, k, n)


def test_no_lds_dma_in_front_of_the_barrier(fused_loops):
    for name, ins in fused_loops.items():
        total = 0
        for k, b in enumerate(bodies(ins)):
            at = next(i for i, x in enumerate(b) if x.startswith("s_barrier"))
            assert not [x for x in b[:at] if LDS_DMA.match(x)], (name, k)
            total += sum(bool(LDS_DMA.match(x)) for x in b[at:])
        assert total == 16, (name, total)   # ... and all of them behind it


def test_the_barrier_drains_the_vector_memory_counter_only(fused_loops):
    """The wave's own vmcnt(0) stands directly in front of the barrier, and no wait that drains lgkmcnt lies between
    the body's head and the barrier: the fragment requests of steps 0 and 1 stay in flight across it."""
    for name, ins in fused_loops.items():
        for k, b in enumerate(bodies(ins)):
            at = next(i for i, x in enumerate(b) if x.startswith("s_barrier"))
            assert re.match(r"s_waitcnt vmcnt\(0\)$", b[at - 1]), (name, k, b[at - 1])
            drains = [x for x in b[:at] if re.match(r"s_waitcnt\b.*lgkmcnt\(0\)", x)]
            assert not drains, (name, k, drains)
