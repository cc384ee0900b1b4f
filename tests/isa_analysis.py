"""What the build tests of the fused 3x3 kernel read out of a kernel's ISA (the `body` of build_report.py's report): its
basic blocks and their successors, the innermost loop that holds MFMAs -- "the main loop" of DESIGN.md section 3.1, one
definition for every budget stated against it -- and the instruction counts inside and outside that loop.  No GPU
needed."""
import re

BRANCH = re.compile(r"^\s+s_c?branch\S*\s+(\.LBB\d+_\d+)")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")


def _is_instruction(line):
    s = line.strip()
    return bool(s) and line[0] in " \t" and not s.startswith((".", ";")) and not s.endswith(":")


def instructions(lines):
    """The instructions among `lines`, stripped, in layout order."""
    return [x.strip() for x in lines if _is_instruction(x)]


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


def _main_loop(body):
    """The blocks of one kernel and the indices of those in the innermost loop that holds MFMAs (exactly one must
    exist): the smallest set of blocks that is strongly connected and holds an MFMA block, found by shrinking from the
    whole kernel -- a loop's inner loops are what stays strongly connected once the edges into its entry blocks are
    cut."""
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
    return blocks, loop


def innermost_mfma_loop(body):
    """`body`: the lines of one kernel.  The lines of the blocks of its main loop, in layout order."""
    blocks, loop = _main_loop(body)
    return [line for i in sorted(loop) for line in blocks[i]]


def outside_innermost_mfma_loop(body):
    """`body`: the lines of one kernel.  The lines of every block that is NOT in its main loop."""
    blocks, loop = _main_loop(body)
    return [line for i, b in enumerate(blocks) if i not in loop for line in b]


def loop_counts(lines):
    """What the main loop is budgeted by: its instructions, and those of them that belong to the loop alone (MFMAs,
    LDS-DMA loads, branches) or to the events kept out of it (lane reads, argument loads, the tile decode)."""
    ins = instructions(lines)

    def n(pat):
        return sum(bool(re.match(pat, x)) for x in ins)
    return {"instructions": len(ins), "branches": n(r"s_c?branch"), "readlane": n(r"v_readfirstlane|v_readlane"),
            "s_load": n(r"s_load|s_buffer_load"), "tile_decode": n(r"v_mul_hi_i32|v_mad_u64_u32"), "mfma": n(r"v_mfma"),
            "lds_dma": sum(bool(re.match(r"buffer_load_dwordx4\b.*\blds\b", x)) for x in ins)}


def class_counts(lines, classes):
    """`classes`: {name: pattern an instruction starts with}.  How many of `lines`' instructions fall in each."""
    ins = instructions(lines)
    return {k: sum(bool(re.match(pat, x)) for x in ins) for k, pat in classes.items()}


def bodies(ins, mfma_per_body):
    """The loop's instructions cut into bodies: each ends with its last MFMA (what follows the last body's -- the
    second tail -- is dropped)."""
    out, cur, n = [], [], 0
    for x in ins:
        cur.append(x)
        if x.startswith("v_mfma"):
            n += 1
            if n == mfma_per_body:
                out.append(cur)
                cur, n = [], 0
    return out
