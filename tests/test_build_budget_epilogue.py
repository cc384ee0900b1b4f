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
import pytest

from build_report import compile_report, template_args
from isa_analysis import class_counts, outside_innermost_mfma_loop

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


@pytest.fixture(scope="module")
def fused_isa():
    return {n: v["body"] for n, v in compile_report("wino_f2_fused.hip").items() if "wino_f2_fused_kernel" in n}


def test_epilogue_instruction_classes_stay_on_their_diet(fused_isa):
    assert len(fused_isa) == 5, sorted(fused_isa)
    seen = set()
    for name, body in fused_isa.items():
        key = tuple(template_args(name, "wino_f2_fused_kernel"))
        c = class_counts(outside_innermost_mfma_loop(body), CLASSES)
        print(key, c)
        assert key in EMITTED, name
        seen.add(key)
        for k, n in EMITTED[key].items():
            assert c[k] <= n + n // 20, (name, k, c[k], "bound", n + n // 20)
    assert seen == set(EMITTED)
