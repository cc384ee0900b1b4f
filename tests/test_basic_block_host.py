"""Host-side checks of the residual 3x3 layer (wino_conv3x3_bn_add_relu_hw) and the ResNet basic block
(wino_basic_block_*) -- no GPU needed: the new C-ABI symbols, the workspace size, every argument, shape and overlap
rejection (each fires before the GPU is touched; no call here gets past the checks, whose addresses are fake), and
the build of conv3x3_res.hip, which instantiates the two 3x3 kernel templates with RES = true only, within the budgets
of the plain instantiations (test_build_budget.py)."""
import ctypes
import os

import pytest

from build_report import compile_report, template_args
from conftest import ROOT

E_SHAPE, E_ARG = -2, -3
NEW = ["wino_conv3x3_bn_add_relu_hw", "wino_basic_block_workspace_bytes_hw", "wino_basic_block_hw",
       "wino_basic_block_prepare_hw"]


def test_new_symbols_exported_and_declared(pkg):
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "winograd_mi355x.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name + "(" in hdr, name
        assert name in pkg.ABI_SYMBOLS, name
        assert hdr.index(name) < hdr.index("#define WINO_ABI_VERSION"), name   # in the "Added since" list
    assert L.wino_abi_version() == 1
    for name in ("conv3x3_bn_add_relu", "basic_block", "basic_block_prepare"):
        assert callable(getattr(pkg, name)), name


def test_workspace_size(pkg):
    L = pkg.lib()
    assert L.wino_basic_block_workspace_bytes_hw(2, 56, 56, 64) == 2 * 58 * 58 * 64 * 4   # t1, padded
    assert L.wino_basic_block_workspace_bytes_hw(3, 7, 9, 512) == 3 * 9 * 11 * 512 * 4
    assert L.wino_basic_block_workspace_bytes_hw(0, 56, 56, 64) == 0


# fake, well-aligned device addresses, far apart: the checks compare addresses and never dereference them
GIB = 1 << 30


def _p(addr):
    return ctypes.c_void_p(addr)


def _layer(L, inp, U, res, out, N=2, H=14, W=14, C=64, K=64, relu=1, bias=_p(64), scale=_p(128)):
    return L.wino_conv3x3_bn_add_relu_hw(inp, U, bias, scale, res, out, N, H, W, C, K, relu, None)


def test_layer_rejections(pkg):
    L = pkg.lib()
    inp, U, res, out = _p(1 * GIB), _p(2 * GIB), _p(3 * GIB), _p(4 * GIB)
    # NULL anywhere
    args = [inp, U, _p(64), _p(128), res, out]
    for i in range(6):
        a = list(args)
        a[i] = None
        assert L.wino_conv3x3_bn_add_relu_hw(*a, 2, 14, 14, 64, 64, 1, None) == E_ARG, i
    # 16-byte alignment of in, U, residual, out
    for i in (0, 1, 4, 5):
        a = list(args)
        a[i] = _p(a[i].value + 4)
        assert L.wino_conv3x3_bn_add_relu_hw(*a, 2, 14, 14, 64, 64, 1, None) == E_ARG, i
    # shapes: K % 64, C % 8, the feature map, the batch
    assert _layer(L, inp, U, res, out, K=96) == E_SHAPE
    assert _layer(L, inp, U, res, out, C=60) == E_SHAPE
    assert _layer(L, inp, U, res, out, H=0) == E_SHAPE
    assert _layer(L, inp, U, res, out, W=4095) == E_SHAPE
    assert _layer(L, inp, U, res, out, N=0) == E_SHAPE
    # overlaps: a padded 14x14x64 image is 16*16*64*4 = 64 KiB; N = 2 -> 128 KiB per tensor
    T = 2 * 16 * 16 * 64 * 4
    assert _layer(L, inp, U, _p(1 * GIB + T - 16), out) == E_ARG         # residual starts inside in
    assert _layer(L, inp, U, res, _p(1 * GIB - T + 16)) == E_ARG         # out ends inside in
    assert _layer(L, inp, U, inp, out) == E_ARG                          # residual IS in
    assert _layer(L, inp, U, res, inp) == E_ARG                          # out IS in
    assert _layer(L, inp, U, res, _p(3 * GIB + 256)) == E_ARG            # out partially over the residual
    assert _layer(L, inp, U, res, _p(3 * GIB - 256)) == E_ARG
    # the input's extent is its own C: C = 128 makes it 256 KiB
    assert _layer(L, inp, U, _p(1 * GIB + T + 16 * 16 * 64 * 4), out, C=128) == E_ARG
    # (that out == residual, and tensors that merely touch, pass these checks is covered on a GPU: past the checks the
    # entry point launches, and these addresses are fake)


def _block(L, x, out, ws, ws_bytes=None, N=2, H=14, W=14, C=64, **kw):
    a = dict(U1=_p(5 * GIB), b1=_p(64), s1=_p(128), U2=_p(6 * GIB), b2=_p(192), s2=_p(256))
    a.update(kw)
    need = 2 * 16 * 16 * 64 * 4 if ws_bytes is None else ws_bytes
    return L.wino_basic_block_hw(x, a["U1"], a["b1"], a["s1"], a["U2"], a["b2"], a["s2"], out, N, H, W, C, ws,
                                 need, None)


def test_block_rejections(pkg):
    L = pkg.lib()
    x, out, ws = _p(1 * GIB), _p(2 * GIB), _p(3 * GIB)
    T = 2 * 16 * 16 * 64 * 4
    for key in ("U1", "b1", "s1", "U2", "b2", "s2"):
        assert _block(L, x, out, ws, **{key: None}) == E_ARG, key
    assert _block(L, None, out, ws) == E_ARG
    assert _block(L, x, None, ws) == E_ARG
    assert _block(L, x, out, None) == E_ARG
    for key in ("U1", "U2"):
        assert _block(L, x, out, ws, **{key: _p(5 * GIB + 8)}) == E_ARG, key
    assert _block(L, _p(1 * GIB + 4), out, ws) == E_ARG
    assert _block(L, x, _p(2 * GIB + 4), ws) == E_ARG
    assert _block(L, x, out, _p(3 * GIB + 4)) == E_ARG
    # K = C: C % 64 (the layer's K % 64)
    assert _block(L, x, out, ws, C=96, ws_bytes=2 * 16 * 16 * 96 * 4) == E_SHAPE
    assert _block(L, x, out, ws, C=32, ws_bytes=2 * 16 * 16 * 32 * 4) == E_SHAPE
    assert _block(L, x, out, ws, N=0) == E_SHAPE
    assert _block(L, x, out, ws, H=4095) == E_SHAPE
    # workspace: too small by one float
    assert _block(L, x, out, ws, ws_bytes=T - 4) == E_ARG
    # overlaps: the workspace with x or out, and x with out unless they are the same tensor
    assert _block(L, x, out, _p(1 * GIB + T - 16)) == E_ARG
    assert _block(L, x, out, _p(2 * GIB - T + 16)) == E_ARG
    assert _block(L, x, out, x) == E_ARG
    assert _block(L, x, _p(1 * GIB + 256), ws) == E_ARG
    assert _block(L, x, _p(1 * GIB - 256), ws) == E_ARG
    assert L.wino_basic_block_prepare_hw(1, 14, 14, 96, None) == E_SHAPE
    assert L.wino_basic_block_prepare_hw(0, 14, 14, 64, None) == E_SHAPE


def test_python_block_refuses_a_channel_change(pkg):
    """The block keeps its channel count: a C -> K filter with K != C is refused from its size alone, before any
    device check (these are CPU tensors)."""
    import torch
    x = torch.zeros(1, 16, 16, 64)
    good = torch.zeros(16 * 64 * 64)
    wide = torch.zeros(16 * 64 * 128)
    bn = (torch.zeros(64), torch.ones(64))
    with pytest.raises(pkg.WinoError, match="keeps its channel count"):
        pkg.basic_block(x, wide, bn, good, bn)
    with pytest.raises(pkg.WinoError, match="keeps its channel count"):
        pkg.basic_block(x, good, bn, wide, bn)
    with pytest.raises(pkg.WinoError, match="CUDA"):   # the right sizes get as far as the device check
        pkg.basic_block(x, good, bn, good, bn)


def _res_kernels(kernels, family):
    return {n: template_args(n, family) for n in kernels if template_args(n, family) is not None}


def test_res_file_compiles_the_res_kernels_only_within_budget(tmp_path):
    k = compile_report("conv3x3_res.hip", tmp_path)
    fused = _res_kernels(k, "wino_f2_fused_kernel")
    small = _res_kernels(k, "wino_f2_small_kernel")
    assert len(k) == len(fused) + len(small), sorted(k)        # nothing else
    # fused: <ABLATE = 0, GEN, TAIL, RES = 1>, GEN x TAIL
    assert sorted(tuple(a) for a in fused.values()) == [(0, g, t, 1) for g in (0, 1) for t in (0, 1)], fused
    # latency: <CT, GEN, DIAG = 0, RES = 1>, CT {1, 2, 4} x GEN
    assert sorted(tuple(a) for a in small.values()) == [(ct, g, 0, 1) for ct in (1, 2, 4) for g in (0, 1)], small
    for name in fused:
        v = k[name]
        assert v["vgprs"] <= 256 and v["occupancy"] >= 2 and v["spill"] == 0, (name, v)
        assert v["mfma"] == 128 and v["spill_code_in_mfma_blocks"] == 0 and v["sgpr_spill"] <= 80, (name, v)
    for name in small:
        v = k[name]
        assert v["spill"] == 0 and v["sgpr_spill"] == 0 and v["spill_code_in_mfma_blocks"] == 0, (name, v)
        assert v["mfma"] >= 32, (name, v)


def test_plain_file_has_no_res_instantiation(tmp_path):
    k = compile_report("wino_f2_fused.hip", tmp_path)
    for family in ("wino_f2_fused_kernel", "wino_f2_small_kernel"):
        args = _res_kernels(k, family)
        assert args, family
        for name, a in args.items():
            assert len(a) == 4 and a[3] == 0, (name, a)   # RES = false everywhere
