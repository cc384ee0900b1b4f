"""What the compiler emits OUTSIDE the main loop of the fused 3x3 throughput kernel, checked at build time (no GPU needed).

Outside the loop the kernel is its prologue, the DMA stream's event code and, most of it, the epilogue: A^T m A with the
pair exchange, the stream-K hand-off and the finalize ("Epilogue").  Both waves of a SIMD run the
epilogue at the same time and share one vector issue port, with the matrix pipe idle, so there an instruction removed is
time won and an instruction that creeps back is time lost without any other symptom.  Four classes are counted per
instantiation: selects (v_cndmask: A^T m A used to choose its sums with 64 of them, on a wave-uniform value), 64-bit
moves (v_mov_b64: the accumulators' zeroing, 64 at the kernel's start and 64 per epilogue), the per-lane tile decodes'
multiplies (v_mul_hi_i32 + v_mad_u64_u32) and the scalar multiplies of the hand-off's bookkeeping (s_mul_i32 +
s_mul_hi_u32).  The bounds are what this source emits plus 5 % for compiler drift; the counts before the epilogue's
diet are beside them.  The counts are printed (pytest -s) so that DESIGN.md can be checked against them."""
import re

import pytest

from build_report import compile_report, template_args

BRANCH = re.compile(r"^\s+s_c?branch\S*\s+(\.LBB\d+_\d+)")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")

CLASSES = {
    "cndmask": r"v_cndmask",
    "mov_b64": r"v_mov_b64",
    "tile_decode": r"v_mul_hi_i32|v_mad_u64_u32",
    "s_mul": r"s_mul_i32|s_mul_hi_u32",
}

# (ABLATE, GEN, TAIL, EPI) -> what the finished source emits outside the loop                  # before the diet
EMITTED = {
    (16, 0, 1, 0): {"cndmask": 75, "mov_b64": 132, "tile_decode": 74, "s_mul": 290},   # 138, 132, 74, 290
    (0, 0, 0, 0): {"cndmask": 42, "mov_b64": 132, "tile_decode": 74, "s_mul": 222},    # 105, 132, 74, 222
    (0, 1, 0, 0): {"cndmask": 66, "mov_b64": 132, "tile_decode": 20, "s_mul": 229},    # 129, 132, 20, 229
    (0, 0, 1, 0): {"cndmask": 75, "mov_b64": 132, "tile_decode": 74, "s_mul": 290},    # 138, 132, 74, 290
    (0, 1, 1, 0): {"cndmask": 99, "mov_b64": 132, "tile_decode": 20, "s_mul": 297},    # 162, 132, 20, 297
}
# (Only the selects moved: the stepped tile decode, the LDS re-zeroing and the multiplier form of the hand-off's range
#  starts were built, measured equal or slower and taken out again -- DESIGN_NOTEBOOK.md, "The epilogue's diet".  Their
#  classes are bounded where they stand so that they do not grow.)


# ---- the innermost MFMA loop of a kernel's control-flow graph, found as test_build_budget_loop.py finds it ----
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


def outside_innermost_mfma_loop(body):
    """`body`: the lines of one kernel.  Returns the lines of every block that is NOT in the innermost loop of its
    control-flow graph that holds MFMAs (exactly one such loop must exist)."""
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
    return [line for i, b in enumerate(blocks) if i not in loop for line in b]


def class_counts(lines):
    ins = [x.strip() for x in lines if _is_instruction(x)]
    return {k: sum(bool(re.match(pat, x)) for x in ins) for k, pat in CLASSES.items()}


@pytest.fixture(scope="module")
def fused_isa(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fused_epilogue")
    kernels = [n for n in compile_report("wino_f2_fused.hip", tmp) if "wino_f2_fused_kernel" in n]
    isa = [f for f in tmp.iterdir() if f.name.endswith(".s") and "gfx950" in f.name]
    assert len(isa) == 1, isa
    text = isa[0].read_text()
    out = {}
    for name in kernels:
        i = text.index(name + ":")
        out[name] = text[i:text.index(".Lfunc_end", i)].splitlines()
    return out


def test_epilogue_instruction_classes_stay_on_their_diet(fused_isa):
    assert len(fused_isa) == 5, sorted(fused_isa)
    seen = set()
    for name, body in fused_isa.items():
        key = tuple(template_args(name, "wino_f2_fused_kernel"))
        c = class_counts(outside_innermost_mfma_loop(body))
        print(key, c)
        assert key in EMITTED, name
        seen.add(key)
        for k, n in EMITTED[key].items():
            assert c[k] <= n + n // 20, (name, k, c[k], "bound", n + n // 20)
    assert seen == set(EMITTED)
