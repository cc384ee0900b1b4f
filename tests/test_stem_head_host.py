"""Host-side checks of the ResNet stem (wino_stem_*) and head (wino_head_*, wino_avgpool_fc_hw) -- no GPU needed: the
new C-ABI symbols, the packed and workspace sizes, the form plan, every argument, shape and overlap rejection (each
fires before the GPU is touched; the addresses are fake), the Python argument errors, and the stem kernel's register
budget (no spill code)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

E_SHAPE, E_ARG = -2, -3
NEW = ["wino_stem_filter_elems", "wino_stem_filter_pack", "wino_stem_hw", "wino_stem_plan", "wino_head_elems",
       "wino_head_pack", "wino_head_workspace_bytes", "wino_head_prepare", "wino_avgpool_fc_hw"]
GIB = 1 << 30


def _p(addr):
    return ctypes.c_void_p(addr)


def test_new_symbols_exported_and_declared(pkg):
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "winograd_mi355x.h")).read()
    added = hdr[:hdr.index("#define WINO_ABI_VERSION")]
    for name in NEW:
        assert hasattr(L, name), name
        assert name + "(" in hdr, name
        assert name in pkg.ABI_SYMBOLS, name
        assert name in added, name   # in the "Added since" list
    assert L.wino_abi_version() == 1
    for name in ("stem_filter_pack", "stem", "stem_plan", "head_pack", "head_prepare", "avgpool_fc", "ResNet"):
        assert callable(getattr(pkg, name)), name


def test_packed_and_workspace_sizes(pkg):
    L = pkg.lib()
    assert L.wino_stem_filter_elems(64) == 64 * 148 + 2 * 64     # 37 k-steps of 4 per channel, then bias and scale
    assert L.wino_stem_filter_elems(128) == 128 * 150
    for bad in (0, -64, 32, 96):
        assert L.wino_stem_filter_elems(bad) == 0
    assert L.wino_head_elems(512, 1000) == (512 + 2) * 1024       # classes padded to a multiple of 64
    assert L.wino_head_elems(2048, 10) == 2050 * 64
    assert L.wino_head_elems(512, 64) == 514 * 64
    assert L.wino_head_elems(48, 10) == 0 and L.wino_head_elems(512, 0) == 0
    # pooled [N][C] rounded up to 256 bytes, then the GEMM's [N][Kp]
    assert L.wino_head_workspace_bytes(2, 512, 1000) == 4096 + 2 * 1024 * 4
    assert L.wino_head_workspace_bytes(3, 32, 1) == 512 + 3 * 64 * 4
    assert L.wino_head_workspace_bytes(0, 512, 10) == 0


def test_stem_plan(pkg, knobs):
    assert pkg.stem_plan(1, 224, 224) == pkg.STEM_FORM_SMALL
    assert pkg.stem_plan(2, 224, 224) == pkg.STEM_FORM_SMALL
    assert pkg.stem_plan(32, 224, 224) == pkg.STEM_FORM_BIG
    assert pkg.stem_plan(128, 224, 224) == pkg.STEM_FORM_BIG
    assert pkg.stem_plan(128, 224, 224, cus=1 << 20) == pkg.STEM_FORM_SMALL
    knobs.set("WINO_STEM_FORM", 1)
    assert pkg.stem_plan(1, 224, 224) == pkg.STEM_FORM_BIG
    knobs.set("WINO_STEM_FORM", 2)
    assert pkg.stem_plan(128, 224, 224) == pkg.STEM_FORM_SMALL
    knobs.unset("WINO_STEM_FORM")
    assert pkg.stem_plan(1, 224, 224) == pkg.STEM_FORM_SMALL
    L = pkg.lib()
    f = ctypes.c_int(-1)
    assert L.wino_stem_plan(1, 224, 224, 96, 256, ctypes.byref(f)) == E_SHAPE
    assert L.wino_stem_plan(1, 224, 224, 64, 256, None) == E_ARG


def test_stem_rejections(pkg):
    L = pkg.lib()
    x, packed, out = _p(GIB), _p(3 * GIB), _p(5 * GIB)
    assert L.wino_stem_filter_pack(None, _p(64), _p(128), packed, 64, None) == E_ARG
    assert L.wino_stem_filter_pack(_p(16), _p(64), _p(128), _p(3 * GIB + 4), 64, None) == E_ARG
    assert L.wino_stem_filter_pack(_p(16), _p(64), _p(128), packed, 96, None) == E_SHAPE

    def run(x=x, packed=packed, out=out, N=2, H=224, W=224, K=64, padded=0):
        return L.wino_stem_hw(x, packed, out, N, H, W, K, padded, None)

    assert run(x=None) == E_ARG
    assert run(out=None) == E_ARG
    assert run(x=_p(GIB + 4)) == E_ARG                  # misaligned base
    assert run(out=_p(5 * GIB + 8)) == E_ARG
    assert run(K=96) == E_SHAPE and run(K=0) == E_SHAPE
    assert run(N=0) == E_SHAPE and run(H=0) == E_SHAPE and run(W=-1) == E_SHAPE
    assert run(padded=2) == E_SHAPE
    assert run(H=30000, W=30000) == E_SHAPE             # one image past 2^31 elements
    assert run(out=_p(GIB + 1024)) == E_ARG             # out overlaps x
    assert run(packed=_p(GIB + 4096)) == E_ARG          # packed overlaps x
    # the padded output is larger: [2][58][58][64] floats from out reach into x placed just behind [2][56][56][64]
    assert run(out=_p(GIB - 2 * 56 * 56 * 64 * 4 - 16), padded=1) == E_ARG


def test_head_rejections(pkg):
    L = pkg.lib()
    feat, packed, out, ws = _p(GIB), _p(2 * GIB), _p(3 * GIB), _p(4 * GIB)
    need = L.wino_head_workspace_bytes(2, 512, 1000)

    def run(feat=feat, packed=packed, out=out, ws=ws, N=2, H=7, W=7, C=512, classes=1000, padded=1, ws_bytes=need):
        return L.wino_avgpool_fc_hw(feat, packed, out, N, H, W, C, classes, padded, ws, ws_bytes, None)

    assert run(feat=None) == E_ARG and run(ws=None) == E_ARG and run(out=None) == E_ARG
    assert run(out=_p(3 * GIB + 4)) == E_ARG
    assert run(C=48) == E_SHAPE and run(classes=0) == E_SHAPE and run(N=0) == E_SHAPE and run(H=0) == E_SHAPE
    assert run(padded=3) == E_SHAPE
    assert run(ws_bytes=need - 1) == E_ARG
    assert run(out=_p(GIB + 512)) == E_ARG                 # out overlaps feat
    assert run(ws=_p(2 * GIB + 1024)) == E_ARG             # workspace overlaps packed
    assert L.wino_head_pack(None, _p(64), packed, 512, 1000, None) == E_ARG
    assert L.wino_head_pack(_p(64), _p(64), _p(2 * GIB + 8), 512, 1000, None) == E_ARG
    assert L.wino_head_pack(_p(64), _p(64), packed, 500, 1000, None) == E_SHAPE
    assert L.wino_head_prepare(2, 500, 10, None) == E_SHAPE


def test_python_argument_errors(pkg):
    import torch
    with pytest.raises(pkg.WinoError):
        pkg.stem(torch.zeros(1, 3, 8, 8), torch.zeros(9600))             # a CPU tensor: no CPU path
    with pytest.raises(pkg.WinoError):
        pkg.stem_filter_pack(torch.zeros(64, 3, 7, 7), (torch.zeros(64), torch.zeros(64)))
    with pytest.raises(pkg.WinoError):
        pkg.avgpool_fc(torch.zeros(1, 7, 7, 512), torch.zeros(10), 10)
    with pytest.raises(pkg.WinoError):
        pkg.head_pack(torch.zeros(10, 512), torch.zeros(10))
    assert pkg.stem_out_hw(224, 224) == (56, 56)
    assert pkg.stem_out_hw(1, 1) == (1, 1)
    assert pkg.stem_out_hw(97, 131) == (25, 33)


def test_stem_kernels_do_not_spill(tmp_path):
    """Both stem forms fit their registers: no scratch, no spill code (the MFMA loop keeps 37 filter values and the
    accumulators of up to 19 row tiles per lane)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "cuda-winograd_amd", "csrc", "stem_head.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "cuda-winograd_amd", "csrc"), "-c", src, "-o",
                        str(tmp_path / "s.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)
    stem = [b for b in blocks if b.startswith("_ZN4wino") and "stem_kernel" in b.split()[0]]
    assert len(stem) == 2, [b.split()[0] for b in blocks[1:]]
    for b in stem:
        assert re.search(r"VGPRs Spill: 0\b", b) and re.search(r"SGPRs Spill: 0\b", b), b
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", b), b
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        assert lds <= 80 * 1024, lds     # two workgroups of the big form share a CU's 160 KiB
