"""Host-side checks of the downsampling basic block (wino_s2_proj_*, wino_conv3x3_s2_proj_bn_relu_hw,
wino_basic_block_s2_*) -- no GPU needed: the new C-ABI symbols, the packed size and the workspace size, every argument,
shape and overlap rejection (each fires before the GPU is touched; no call here gets past the checks, whose addresses
are fake), and the build of basic_block_s2.hip, which instantiates the 1x1 kernel templates in operand form A_TAPS_PROJ
only, within the budgets of the tap form (test_conv3x3_s2_host.py)."""
import os
import re
import shutil
import subprocess

import pytest

from build_report import CSRC, compile_report, template_args
from conftest import ROOT

E_SHAPE, E_ARG = -2, -3
A_TAPS_PROJ = 4
NEW = ["wino_s2_proj_elems", "wino_s2_proj_pack", "wino_conv3x3_s2_proj_bn_relu_hw",
       "wino_basic_block_s2_workspace_bytes_hw", "wino_basic_block_s2_hw", "wino_basic_block_s2_prepare_hw"]
GIB = 1 << 30


def _p(addr):
    import ctypes
    return ctypes.c_void_p(addr)


def test_new_symbols_exported_and_declared(pkg):
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "winograd_mi355x.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name + "(" in hdr, name
        assert name in pkg.ABI_SYMBOLS, name
        assert hdr.index(name) < hdr.index("#define WINO_ABI_VERSION"), name   # in the "Added since" list
    assert L.wino_abi_version() == 1
    assert "has no entry point yet" not in " ".join(open(os.path.join(ROOT, "INTEGRATION.md")).read().split())
    for name in ("s2_proj_pack", "conv3x3_s2_proj", "basic_block_s2", "basic_block_s2_prepare"):
        assert callable(getattr(pkg, name)), name


def test_packed_and_workspace_sizes(pkg):
    L = pkg.lib()
    # [10 C][K] filters (nine taps, then the shortcut) and four BN vectors of K
    assert L.wino_s2_proj_elems(64, 128) == (10 * 64 + 4) * 128
    assert L.wino_s2_proj_elems(512, 512) == (10 * 512 + 4) * 512
    assert L.wino_s2_proj_elems(0, 128) == 0
    # t1, padded, at the output grid: H = (Hin - 1) // 2 + 1
    assert L.wino_basic_block_s2_workspace_bytes_hw(2, 56, 56, 128) == 2 * 30 * 30 * 128 * 4
    assert L.wino_basic_block_s2_workspace_bytes_hw(3, 15, 7, 64) == 3 * 10 * 6 * 64 * 4
    assert L.wino_basic_block_s2_workspace_bytes_hw(1, 1, 1, 64) == 1 * 3 * 3 * 64 * 4
    assert L.wino_basic_block_s2_workspace_bytes_hw(0, 56, 56, 128) == 0


def test_pack_rejections(pkg):
    L = pkg.lib()
    args = [_p(k * GIB) for k in range(1, 8)]
    for i in range(7):
        a = list(args)
        a[i] = None
        assert L.wino_s2_proj_pack(*a, 64, 128, None) == E_ARG, i
    a = list(args)
    a[6] = _p(7 * GIB + 4)
    assert L.wino_s2_proj_pack(*a, 64, 128, None) == E_ARG             # packed: 16 bytes per lane
    assert L.wino_s2_proj_pack(*args, 48, 128, None) == E_SHAPE        # C % 32
    assert L.wino_s2_proj_pack(*args, 64, 96, None) == E_SHAPE         # K % 64


def _layer(L, x, packed, t1, sc, N=2, Hin=28, Win=28, C=64, K=128):
    return L.wino_conv3x3_s2_proj_bn_relu_hw(x, packed, t1, sc, N, Hin, Win, C, K, None)


def test_layer_rejections(pkg):
    L = pkg.lib()
    x, packed, t1, sc = _p(1 * GIB), _p(2 * GIB), _p(3 * GIB), _p(4 * GIB)
    args = [x, packed, t1, sc]
    for i in range(4):
        a = list(args)
        a[i] = None
        assert _layer(L, *a) == E_ARG, i
        a = list(args)
        a[i] = _p(a[i].value + 4)
        assert _layer(L, *a) == E_ARG, i
    assert _layer(L, *args, C=48) == E_SHAPE
    assert _layer(L, *args, K=96) == E_SHAPE
    assert _layer(L, *args, N=0) == E_SHAPE
    assert _layer(L, *args, N=1 << 22, Hin=56, Win=56) == E_SHAPE        # M = N*H*W >= 2^31
    assert _layer(L, *args, N=1, Hin=1, Win=8186, C=512, K=64) == E_SHAPE   # a tile's window over x (check_s2)
    # overlaps: x is 2 * 30 * 30 * 64 * 4 bytes, t1 and sc 2 * 16 * 16 * 128 * 4
    X, T = 2 * 30 * 30 * 64 * 4, 2 * 16 * 16 * 128 * 4
    assert _layer(L, x, packed, t1, t1) == E_ARG                          # t1 IS sc
    assert _layer(L, x, packed, t1, _p(3 * GIB + T - 16)) == E_ARG        # sc starts inside t1
    assert _layer(L, x, packed, _p(1 * GIB + X - 16), sc) == E_ARG        # t1 starts inside x
    assert _layer(L, x, _p(4 * GIB + T - 16), t1, sc) == E_ARG            # packed starts inside sc


def _block(L, x, packed, out, ws, ws_bytes=None, N=2, Hin=28, Win=28, C=64, K=128, U2=_p(6 * GIB), b2=_p(64),
           s2=_p(128)):
    need = N * ((Hin - 1) // 2 + 3) * ((Win - 1) // 2 + 3) * K * 4 if ws_bytes is None else ws_bytes
    return L.wino_basic_block_s2_hw(x, packed, U2, b2, s2, out, N, Hin, Win, C, K, ws, need, None)


def test_block_rejections(pkg):
    L = pkg.lib()
    x, packed, out, ws = _p(1 * GIB), _p(2 * GIB), _p(3 * GIB), _p(4 * GIB)
    T = 2 * 16 * 16 * 128 * 4          # out and the workspace at N = 2, 28 -> 14, K = 128
    X = 2 * 30 * 30 * 64 * 4
    P = (10 * 64 + 4) * 128 * 4
    for key in ("U2", "b2", "s2"):
        assert _block(L, x, packed, out, ws, **{key: None}) == E_ARG, key
    assert _block(L, None, packed, out, ws) == E_ARG
    assert _block(L, x, None, out, ws) == E_ARG
    assert _block(L, x, packed, None, ws) == E_ARG
    assert _block(L, x, packed, out, None) == E_ARG
    # 16-byte alignment of x, packed, U2, out, workspace
    assert _block(L, _p(1 * GIB + 4), packed, out, ws) == E_ARG
    assert _block(L, x, _p(2 * GIB + 8), out, ws) == E_ARG
    assert _block(L, x, packed, _p(3 * GIB + 4), ws) == E_ARG
    assert _block(L, x, packed, out, _p(4 * GIB + 12)) == E_ARG
    assert _block(L, x, packed, out, ws, U2=_p(6 * GIB + 4)) == E_ARG
    # shapes: C % 32, K % 64, the batch, the stride-2 layer's 32-bit windows, the second 3x3's feature map
    assert _block(L, x, packed, out, ws, C=48) == E_SHAPE
    assert _block(L, x, packed, out, ws, K=96) == E_SHAPE
    assert _block(L, x, packed, out, ws, N=0) == E_SHAPE
    assert _block(L, x, packed, out, ws, N=1 << 22, Hin=56, Win=56) == E_SHAPE
    assert _block(L, x, packed, out, ws, N=1, Hin=1, Win=8186, C=512, K=64) == E_SHAPE
    assert _block(L, x, packed, out, ws, N=1, Hin=3, Win=8200) == E_SHAPE   # a 4100-wide output
    # workspace too small by one float
    assert _block(L, x, packed, out, ws, ws_bytes=T - 4) == E_ARG
    assert "workspace" in L.wino_last_error_string().decode()
    # every overlap among x, out, the workspace and packed
    assert _block(L, x, packed, out, _p(3 * GIB + T - 16)) == E_ARG       # workspace inside out
    assert _block(L, x, packed, out, _p(1 * GIB + X - 16)) == E_ARG       # workspace inside x
    assert _block(L, x, packed, out, _p(2 * GIB + P - 16)) == E_ARG       # workspace inside packed
    assert _block(L, x, packed, _p(1 * GIB + 256), ws) == E_ARG           # out inside x
    assert _block(L, x, packed, _p(2 * GIB - T + 16), ws) == E_ARG        # out ends inside packed
    assert _block(L, x, _p(1 * GIB + 512), out, ws) == E_ARG              # packed inside x
    assert _block(L, x, packed, x, ws) == E_ARG                           # out IS x (the block changes the shape)
    assert "overlap" in L.wino_last_error_string().decode()
    assert L.wino_basic_block_s2_prepare_hw(1, 28, 28, 48, 128, None) == E_SHAPE
    assert L.wino_basic_block_s2_prepare_hw(1, 28, 28, 64, 96, None) == E_SHAPE
    assert L.wino_basic_block_s2_prepare_hw(0, 28, 28, 64, 128, None) == E_SHAPE


def test_python_argument_errors(pkg):
    """Shape errors are refused before any device check (these are CPU tensors)."""
    import torch
    x = torch.zeros(1, 30, 30, 64)
    bn = (torch.zeros(128), torch.ones(128))
    packed = torch.zeros((10 * 64 + 4) * 128)
    U2 = torch.zeros(16 * 128 * 128)
    with pytest.raises(pkg.WinoError, match="packed does not match"):
        pkg.basic_block_s2(x, torch.zeros(1000), U2, bn)
    with pytest.raises(pkg.WinoError, match="U2 must be"):
        pkg.basic_block_s2(x, packed, torch.zeros(16 * 64 * 128), bn)
    with pytest.raises(pkg.WinoError, match="x must be"):
        pkg.basic_block_s2(torch.zeros(30, 30, 64), packed, U2, bn)
    with pytest.raises(pkg.WinoError, match="x must be"):
        pkg.conv3x3_s2_proj(torch.zeros(1, 2, 30, 64), packed)
    with pytest.raises(pkg.WinoError, match="CUDA"):   # the right sizes get as far as the device check
        pkg.basic_block_s2(x, packed, U2, bn)


def test_proj_file_compiles_the_proj_form_only_within_budget(tmp_path):
    """basic_block_s2.hip instantiates the 1x1 kernel templates in form A_TAPS_PROJ (4) only -- 4 tiled kernels
    ({4, 8 waves} x {plain, stream-K}) and 18 latency kernels (KS x RT x CT) -- and its pack kernel, within the tap form's
    budgets: the tiled kernel 128 VGPRs / 4 waves (8-wave) or 168 / 3 (4-wave), the latency kernels no spill at all, no
    spill code beside MFMAs.  (The stream-K kernels hold a few more SGPRs than A_TAPS's -- the shortcut's flag and
    pointers -- spilled to VGPR lanes outside the MFMA blocks.)"""
    k = compile_report("basic_block_s2.hip", tmp_path)
    tiled = {n: v for n, v in k.items() if "conv1x1_bn_kernel" in n}
    small = {n: v for n, v in k.items() if "conv1x1_small_kernel" in n}
    pack = {n: v for n, v in k.items() if "s2_proj_pack_kernel" in n}
    assert len(tiled) == 4, sorted(tiled)
    assert len(small) == 18, sorted(small)
    assert len(pack) == 1, sorted(k)
    assert set(k) == set(tiled) | set(small) | set(pack), sorted(k)
    assert all(template_args(n, "conv1x1_bn_kernel")[-1] == A_TAPS_PROJ for n in tiled), sorted(tiled)
    assert all(template_args(n, "conv1x1_small_kernel")[-1] == A_TAPS_PROJ for n in small), sorted(small)
    for name, v in tiled.items():
        eight = "ILi32ELi8E" in name
        assert eight or "ILi32ELi4E" in name, name
        budget, waves = (128, 4) if eight else (168, 3)
        assert v["vgprs"] <= budget and v["occupancy"] >= waves and v["spill"] <= 8, (name, v)
        assert v["mfma"] >= 56 and v["spill_code_in_mfma_blocks"] == 0 and v["sgpr_spill"] <= 48, (name, v)
    for name, v in small.items():
        assert v["spill"] == 0 and v["sgpr_spill"] == 0 and v["spill_code_in_mfma_blocks"] == 0, (name, v)


def test_proj_form_k_loop_has_no_per_lane_offsets(tmp_path):
    """As in the tap form (test_conv3x3_s2_host.py): no readfirstlane loop and no per-lane multiply in a basic block with
    MFMAs of the A_TAPS_PROJ tiled kernels -- the shortcut tiles reuse the tap form's scalar k offsets."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    asm = tmp_path / "bb_s2.s"
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                          "-I" + CSRC, "--cuda-device-only", "-S", os.path.join(CSRC, "basic_block_s2.hip"), "-o",
                          str(asm)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    text = asm.read_text()
    names = re.findall(r"^(_ZN4wino7gemm1x117conv1x1_bn_kernel\w+):", text, re.M)
    assert len(names) == 4, names
    for name in names:
        i = text.index("\n" + name + ":") + 1
        body = text[i:text.index(".Lfunc_end", i)]
        hot = [b for b in re.split(r"\n(?=\.LBB\d+_\d+:)", body) if "v_mfma" in b]
        assert hot, name
        for op in ("v_readfirstlane", "s_and_saveexec", "v_mul_lo_u32"):
            assert sum(b.count(op) for b in hot) == 0, (name, op)
