"""Host-side checks of the projection bottleneck block (no GPU needed): the new C-ABI symbols, argument and shape
rejections (including the 32-bit limits of the strided / two-source addressing), the plan query's routing, and the
build budget of proj_block.hip -- whose kernels are the 1x1 kernels in their new operand forms -- beside the kernel
set of conv1x1.hip, which must not change."""
import ctypes
import os

import pytest

from build_report import compile_report, template_args
from conftest import ROOT

STAGES = {   # (Hin, Cin, Cm, C4, stride): ResNet-50's stage-entry blocks
    "conv2": (56, 64, 64, 256, 1),
    "conv3": (56, 256, 128, 512, 2),
    "conv4": (28, 512, 256, 1024, 2),
    "conv5": (14, 1024, 512, 2048, 2),
}
NEW = ["wino_proj_tail_elems", "wino_proj_tail_pack", "wino_proj_block_workspace_bytes_hw", "wino_proj_block_prepare_hw",
       "wino_proj_block_hw", "wino_proj_tail_plan"]


def test_new_symbols_exported_and_declared(pkg):
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "winograd_mi355x.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name + "(" in hdr, name
        assert name in pkg.ABI_SYMBOLS, name
    assert L.wino_abi_version() == 1


def test_sizes(pkg):
    L = pkg.lib()
    assert L.wino_proj_tail_elems(64, 64, 256) == (64 + 64 + 2) * 256
    assert L.wino_proj_tail_elems(0, 64, 256) == 0
    assert L.wino_proj_block_workspace_bytes_hw(2, 28, 28, 128) == 2 * 2 * 30 * 30 * 128 * 4


def _plan(pkg, *shape, cus=256):
    f, t = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = pkg.lib().wino_proj_tail_plan(*shape, cus, ctypes.byref(f), ctypes.byref(t))
    return rc, (f.value, t.value)


def test_shape_and_argument_rejections(pkg):
    L = pkg.lib()
    E_SHAPE, E_ARG = -2, -3
    ok = (2, 28, 28, 256, 128, 512, 2)
    assert _plan(pkg, *ok)[0] == 0
    assert _plan(pkg, 2, 28, 28, 256, 128, 512, 3)[0] == E_ARG      # stride 3
    assert _plan(pkg, 2, 28, 28, 256, 128, 512, 0)[0] == E_ARG
    assert _plan(pkg, 2, 28, 28, 48, 128, 512, 2)[0] == E_SHAPE     # Cin % 32
    assert _plan(pkg, 2, 28, 28, 256, 96, 512, 2)[0] == E_SHAPE     # Cm % 64
    assert _plan(pkg, 2, 28, 28, 256, 128, 480, 2)[0] == E_SHAPE    # C4 % 64
    assert _plan(pkg, 0, 28, 28, 256, 128, 512, 2)[0] == E_SHAPE    # no image
    assert _plan(pkg, *ok, cus=0)[0] == E_ARG
    # the 32-bit limits: M = N*H*W < 2^31, a tile's window over the strided x (111 rows * s * Win * Cin * 4 bytes)
    # and over the padded t2, the ring pass's 16-byte units, B's descriptor
    assert _plan(pkg, 1 << 20, 56, 56, 64, 64, 256, 1)[0] == E_SHAPE          # M = 3.3e9
    assert _plan(pkg, 1, 2, 4096 * 2, 4096, 64, 64, 2)[0] == E_SHAPE          # strided window: 111 * 2 * 8192 * 4096 * 4
    assert _plan(pkg, 1, 2, 4000, 64, 8192, 64, 1)[0] == E_SHAPE              # padded t2 window
    assert _plan(pkg, 1, 2, 9000, 64, 64, 64, 2)[0] == E_SHAPE                # output 4500 wide: more than 4094
    assert _plan(pkg, 1, 7, 7, 32768, 32768, 64, 2)[0] == E_SHAPE             # (Cm + Cin) * C4 * 4 >= 4 GiB
    # the entry point refuses bad arguments before it touches the GPU
    w = ctypes.c_void_p(256)
    bad = ctypes.c_void_p(260)
    args = [w] * 9
    assert L.wino_proj_block_hw(*args, 1, 14, 14, 64, 64, 128, 3, w, 1 << 30, None) == E_ARG     # stride 3
    assert L.wino_proj_block_hw(*args, 1, 14, 14, 48, 64, 128, 2, w, 1 << 30, None) == E_SHAPE   # Cin % 32
    assert L.wino_proj_block_hw(bad, *args[1:], 1, 14, 14, 64, 64, 128, 2, w, 1 << 30, None) == E_ARG   # misaligned x
    assert L.wino_proj_block_hw(*args[:7], bad, w, 1, 14, 14, 64, 64, 128, 2, w, 1 << 30, None) == E_ARG  # tail
    assert L.wino_proj_block_hw(*args, 1, 14, 14, 64, 64, 128, 2, bad, 1 << 30, None) == E_ARG   # workspace
    assert L.wino_proj_block_hw(*args, 1, 14, 14, 64, 64, 128, 2, w, 100, None) == E_ARG         # workspace too small
    assert L.wino_proj_block_hw(None, *args[1:], 1, 14, 14, 64, 64, 128, 2, w, 1 << 30, None) == E_ARG
    assert L.wino_proj_tail_pack(*[w] * 6, bad, 64, 64, 128, None) == E_ARG
    assert L.wino_proj_tail_pack(*[w] * 7, 64, 48, 128, None) == E_SHAPE
    assert L.wino_proj_block_prepare_hw(1, 14, 14, 64, 64, 128, 3, None) == E_ARG
    assert "stride" in L.wino_last_error_string().decode()


def _form_1x1(pkg, M, K, Kout):
    use = pkg.small_plan_1x1(M, K, Kout, cus=256)[0]
    if use:
        return pkg.FORM_LATENCY
    v = [ctypes.c_int() for _ in range(5)]
    assert pkg.lib().wino_conv1x1_plan(M, K, Kout, 256, *[ctypes.byref(x) for x in v]) == 0
    return pkg.FORM_STREAM_K if v[4].value else pkg.FORM_TILED


def test_plan_routing_at_the_stage_shapes(pkg, knobs):
    """The block's 1x1 launches are planned as the plain 1x1 layers of their GEMM shapes -- the tail as ONE GEMM of
    K = Cm + Cin -- so the latency form carries the reference's own one-image regime and the tiled kernel the big
    batches."""
    for k in ("WINO_1X1_ALGO", "WINO_1X1_SMALL_KS", "WINO_1X1_SK", "WINO_1X1_SK_GRID"):
        knobs.unset(k)
    for stage, (Hin, Cin, Cm, C4, s) in STAGES.items():
        H = (Hin - 1) // s + 1
        for N in (1, 2, 8, 16, 32, 128):
            rc, (first, tail) = _plan(pkg, N, Hin, Hin, Cin, Cm, C4, s)
            assert rc == 0
            M = N * H * H
            assert first == _form_1x1(pkg, M, Cin, Cm), (stage, N)
            assert tail == _form_1x1(pkg, M, Cm + Cin, C4), (stage, N)
        # one image: both 1x1 launches take the latency form at every stage
        assert _plan(pkg, 1, Hin, Hin, Cin, Cm, C4, s)[1] == (pkg.FORM_LATENCY,) * 2, stage
    # 128 images: the tiled kernel; conv5's tail (1536 -> 2048, 49 tiles per ... 6272 rows) in stream-K form
    assert _plan(pkg, 128, 28, 28, 512, 256, 1024, 2)[1] == (pkg.FORM_TILED, pkg.FORM_TILED)
    assert _plan(pkg, 128, 14, 14, 1024, 512, 2048, 2)[1] == (pkg.FORM_TILED, pkg.FORM_STREAM_K)
    # forced forms are reported as such
    knobs.set("WINO_1X1_ALGO", "big")
    knobs.set("WINO_1X1_SK", 1)
    assert _plan(pkg, 2, 28, 28, 256, 128, 512, 2)[1] == (pkg.FORM_STREAM_K,) * 2
    knobs.set("WINO_1X1_SK", 0)
    assert _plan(pkg, 2, 28, 28, 256, 128, 512, 2)[1] == (pkg.FORM_TILED,) * 2


def test_proj_form_kernels_build_budget(tmp_path):
    """proj_block.hip instantiates the 1x1 kernel templates in the projection forms only (the form is the templates'
    last argument, AF), and those keep the budgets of the plain forms (tests/test_build_budget.py): the tiled kernel
    128 VGPRs / 4 waves (8-wave) or 168 / 3 (4-wave), a few spills outside the loops at most; the latency kernel no
    spill at all; neither any spill code beside MFMAs."""
    k = compile_report("proj_block.hip", tmp_path)
    tiled = {n: v for n, v in k.items() if "conv1x1_bn_kernel" in n}
    small = {n: v for n, v in k.items() if "conv1x1_small_kernel" in n}
    assert len(tiled) == 8, sorted(tiled)     # {4, 8 waves} x {plain, stream-K} x {strided, two sources}
    assert len(small) == 36, sorted(small)    # KS {1, 2, 4} x RT {1, 2} x CT {1, 2, 4} x {strided, two sources}
    # half in each projection form (AF = A_STRIDED 1 / A_TWO 2), none in the plain form
    forms = [template_args(n, "conv1x1_bn_kernel")[-1] for n in tiled]
    assert sorted(forms) == [1] * 4 + [2] * 4, sorted(tiled)
    forms = [template_args(n, "conv1x1_small_kernel")[-1] for n in small]
    assert sorted(forms) == [1] * 18 + [2] * 18, sorted(small)
    for name, v in tiled.items():
        eight = "ILi32ELi8E" in name
        assert eight or "ILi32ELi4E" in name, name
        budget, waves = (128, 4) if eight else (168, 3)
        assert v["vgprs"] <= budget and v["occupancy"] >= waves and v["spill"] <= 8, (name, v)
        assert v["mfma"] >= 56 and v["spill_code_in_mfma_blocks"] == 0 and v["sgpr_spill"] <= 40, (name, v)
    for name, v in small.items():
        assert v["spill"] == 0 and v["sgpr_spill"] == 0 and v["spill_code_in_mfma_blocks"] == 0, (name, v)


def test_conv1x1_kernel_set_unchanged(tmp_path):
    """conv1x1.hip instantiates exactly the kernels it did before the projection forms existed: all in the plain
    operand form (AF = A_PLAIN = 0), none in the new ones."""
    k = compile_report("conv1x1.hip", tmp_path)
    tiled = [n for n in k if "conv1x1_bn_kernel" in n]
    small = [n for n in k if "conv1x1_small_kernel" in n]
    assert len(tiled) == 8 and len(small) == 18, sorted(k)
    assert all(template_args(n, "conv1x1_bn_kernel")[-1] == 0 for n in tiled), tiled
    assert all(template_args(n, "conv1x1_small_kernel")[-1] == 0 for n in small), small
    assert not [n for n in k if "proj" in n]
