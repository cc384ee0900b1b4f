"""What the compiler emits for the main loop of the fused 3x3 throughput kernel, checked at build time (no GPU needed).

The loop's common path is two copies of the body (169 instructions between the first and the last MFMA, plus the 24
packed operations of the next iteration's input transform) and, after each, a tail that only advances the DMA stream's
two scalar offsets, rotates the four filter-fragment bases, steps the filter-stage counter and counts the iteration
down.  Everything rarer -- an item switch of the DMA stream with its per-lane tile decode, the stream's end, the end of
a compute segment -- is an event handled outside that loop.  A wave runs the tail after its
last MFMA of the iteration, when the SIMD's other wave is already waiting at the barrier, so every instruction there is
serial time of the matrix pipe.  This test keeps the walker's state machine from growing back into the loop."""
import re

import pytest

from build_report import CSRC, compile_report  # noqa: F401  (compile_report: the same cross-compile the other budgets use)

BRANCH = re.compile(r"^\s+s_c?branch\S*\s+(\.LBB\d+_\d+)")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")


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


def _sccs(nodes, succ):
    """Strongly connected components (Tarjan, iterative) of the graph restricted to `nodes`; only those with a cycle."""
    nodes = set(nodes)
    index, low, on, stack, out, n = {}, {}, set(), [], [], 0
    for root in sorted(nodes):
        if root in index:
            continue
        work = [(root, iter(succ[root]))]
        index[root] = low[root] = n
        n += 1
        stack.append(root)
        on.add(root)
        while work:
            v, it = work[-1]
            for w in it:
                if w not in nodes:
                    continue
                if w not in index:
                    index[w] = low[w] = n
                    n += 1
                    stack.append(w)
                    on.add(w)
                    work.append((w, iter(succ[w])))
                    break
                if w in on:
                    low[v] = min(low[v], index[w])
            else:
                work.pop()
                if work:
                    low[work[-1][0]] = min(low[work[-1][0]], low[v])
                if low[v] == index[v]:
                    comp = []
                    while True:
                        w = stack.pop()
                        on.discard(w)
                        comp.append(w)
                        if w == v:
                            break
                    if len(comp) > 1 or v in succ[v]:
                        out.append(comp)
    return out


def innermost_mfma_loop(body):
    """`body`: the lines of one kernel.  Returns the lines of the blocks of the innermost loop of its control-flow
    graph that holds MFMAs (exactly one must exist).  A loop is a strongly connected set of blocks; its inner loops are
    what stays strongly connected once the edges into its entry blocks are cut."""
    blocks, succ = _blocks(body)
    hot = {i for i, b in enumerate(blocks) if any("v_mfma" in x for x in b)}
    pred = [[] for _ in blocks]
    for i, out in enumerate(succ):
        for j in out:
            pred[j].append(i)
    nodes, loop = set(range(len(blocks))), None
    while True:
        inner = [c for c in _sccs(nodes, succ) if hot & set(c)]
        if not inner:
            break
        assert len(inner) == 1, [sorted(c) for c in inner]
        loop = set(inner[0])
        entries = {i for i in loop if any(p not in loop for p in pred[i])} or {min(loop)}
        succ = [[j for j in out if not (i in loop and j in entries)] for i, out in enumerate(succ)]
        nodes = loop
    assert loop is not None
    return [line for i in sorted(loop) for line in blocks[i]]


def loop_counts(lines):
    ins = [x.strip() for x in lines if _is_instruction(x)]

    def n(pat):
        return sum(bool(re.match(pat, x)) for x in ins)
    return {"instructions": len(ins), "branches": n(r"s_c?branch"), "readlane": n(r"v_readfirstlane|v_readlane"),
            "s_load": n(r"s_load|s_buffer_load"), "tile_decode": n(r"v_mul_hi_i32|v_mad_u64_u32"), "mfma": n(r"v_mfma"),
            "lds_dma": sum(bool(re.match(r"buffer_load_dwordx4\b.*\blds\b", x)) for x in ins)}


@pytest.fixture(scope="module")
def fused_isa(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fused_loop")
    kernels = {n: v for n, v in compile_report("wino_f2_fused.hip", tmp).items() if "wino_f2_fused_kernel" in n}
    isa = [f for f in tmp.iterdir() if f.name.endswith(".s") and "gfx950" in f.name]
    assert len(isa) == 1, isa
    text = isa[0].read_text()
    out = {}
    for name in kernels:
        i = text.index(name + ":")
        out[name] = text[i:text.index(".Lfunc_end", i)].splitlines()
    return out


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
