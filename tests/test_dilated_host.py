"""Host-side checks of the dilated 3x3 layer (wino_conv3x3_dilated_*), the dilated bottleneck blocks
(wino_dilated_*_block_*) and the dilated ResNet stages -- no GPU needed: the C-ABI symbols, every shape and argument
refusal (each fires before the GPU is touched), the plan (tiled or stream-K, never the latency form), the tests' own
fp64 reference and NaN footprint proven against torch's conv2d(padding=d, dilation=d), and the block kinds of a ResNet
with replace_stride_with_dilation against torchvision's rule, written out."""
import ctypes
import importlib
import os

import numpy as np
import pytest

from conftest import ROOT
from dilated_cases import dilated_reference, footprint

E_SHAPE, E_ARG = -2, -3
NEW = ["wino_conv3x3_dilated_bn_relu_hw", "wino_conv3x3_dilated_prepare_hw", "wino_conv3x3_dilated_plan",
       "wino_dilated_residual_block_hw", "wino_dilated_residual_block_prepare_hw", "wino_dilated_proj_block_hw",
       "wino_dilated_proj_block_prepare_hw"]


def test_new_symbols_exported_and_declared(pkg):
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "winograd_mi355x.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name + "(" in hdr, name
        assert name in pkg.SIGNATURES, name
    assert L.wino_abi_version() == 1
    for name in ("conv3x3_dilated_bn_relu", "conv3x3_dilated_prepare", "conv3x3_dilated_plan", "dilated_residual_block",
                 "dilated_residual_block_prepare", "dilated_proj_block", "dilated_proj_block_prepare", "FCN"):
        assert hasattr(pkg, name), name


def _plan(pkg, N, H, W, C, K, d, cus=256):
    f = ctypes.c_int(-1)
    rc = pkg.lib().wino_conv3x3_dilated_plan(N, H, W, C, K, d, cus, ctypes.byref(f))
    return rc, f.value


def test_plan_refusals(pkg):
    L = pkg.lib()
    assert _plan(pkg, 2, 28, 28, 256, 256, 2)[0] == 0
    assert _plan(pkg, 2, 28, 28, 48, 256, 2)[0] == E_SHAPE            # C % 32
    assert _plan(pkg, 2, 28, 28, 256, 96, 2)[0] == E_SHAPE            # K % 64
    assert _plan(pkg, 2, 28, 28, 256, 256, 0)[0] == E_SHAPE           # dilation < 1
    assert _plan(pkg, 2, 28, 28, 256, 256, -3)[0] == E_SHAPE
    assert "dilation" in L.wino_last_error_string().decode()
    assert _plan(pkg, 0, 28, 28, 256, 256, 2)[0] == E_SHAPE
    assert _plan(pkg, 2, 28, 0, 256, 256, 2)[0] == E_SHAPE
    assert _plan(pkg, 2, 28, 28, 256, 256, 2, cus=0)[0] == E_ARG
    assert L.wino_conv3x3_dilated_plan(2, 28, 28, 256, 256, 2, 256, None) == E_ARG
    # the 32-bit limits.  M = N*H*W < 2^31
    assert _plan(pkg, 1 << 22, 28, 28, 64, 64, 2)[0] == E_SHAPE
    # a tile's window: (111 (2 (W+2) + 3) + 2 d (W+3) + 1) C 4 bytes.  W = 65, C = 512: 15208 + 136 d pixels of 2 KiB,
    # 2^32 from d = 15309 on
    assert _plan(pkg, 1, 65, 65, 512, 512, 15308)[0] == 0
    assert _plan(pkg, 1, 65, 65, 512, 512, 15309)[0] == E_SHAPE
    assert "window" in L.wino_last_error_string().decode()
    assert _plan(pkg, 1, 65, 65, 512, 512, (1 << 31) - 1)[0] == E_SHAPE
    assert _plan(pkg, 1, 2, 4094, 2560, 64, 1)[0] == E_SHAPE            # the window with no dilation to speak of
    assert _plan(pkg, 1, 7, 7, 4096, 32768, 2)[0] == E_SHAPE           # B: 9 * 4096 * 32768 * 4 bytes
    assert _plan(pkg, 1 << 20, 1, 1, 32, 4096, 2)[0] == E_SHAPE        # ring: 2^20 images * 8 pixels * 1024 units
    assert _plan(pkg, 1 << 18, 1, 1, 32, 4096, 2)[0] == 0
    assert _plan(pkg, 1, 3, 4100, 32, 64, 2)[0] == E_SHAPE             # more than 4094 wide
    # a dilation larger than the map is legal (DeepLabV3's ASPP rates on a small map included)
    for d in (12, 24, 36):
        assert _plan(pkg, 1, 3, 3, 32, 64, d)[0] == 0


def test_plan_is_never_the_latency_form(pkg, knobs):
    """Tiled or stream-K whatever the size -- the shapes the stride-2 tap layer gives to its latency form included --
    and whatever WINO_1X1_ALGO asks for."""
    shapes = [(1, 7, 7, 512, 512, 2), (1, 14, 14, 256, 256, 2), (2, 28, 28, 128, 128, 4), (1, 1, 1, 32, 64, 1),
              (1, 65, 65, 256, 256, 2), (8, 65, 65, 512, 512, 4), (128, 14, 14, 256, 256, 2)]
    for k in ("WINO_1X1_ALGO", "WINO_1X1_SMALL_KS", "WINO_1X1_SK", "WINO_1X1_SK_GRID"):
        knobs.unset(k)
    forms = {s: pkg.conv3x3_dilated_plan(*s) for s in shapes}
    assert set(forms.values()) <= {pkg.FORM_TILED, pkg.FORM_STREAM_K}, forms
    knobs.set("WINO_1X1_ALGO", "small")
    for s in shapes:
        assert pkg.conv3x3_dilated_plan(*s) in (pkg.FORM_TILED, pkg.FORM_STREAM_K), s
    knobs.set("WINO_1X1_ALGO", "big")
    knobs.set("WINO_1X1_SK", 0)
    assert pkg.conv3x3_dilated_plan(2, 28, 28, 64, 256, 2) == pkg.FORM_TILED
    knobs.set("WINO_1X1_SK", 1)
    assert pkg.conv3x3_dilated_plan(2, 28, 28, 64, 256, 2) == pkg.FORM_STREAM_K


def test_layer_refusals(pkg):
    L = pkg.lib()
    w, bad = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4)
    far = ctypes.c_void_p(1 << 30)
    args = [w, far, far, far, ctypes.c_void_p(1 << 31)]
    run = lambda a, *shape: L.wino_conv3x3_dilated_bn_relu_hw(*a, *shape, 1, None)
    for i in range(5):
        a = list(args)
        a[i] = None
        assert run(a, 1, 14, 14, 64, 64, 2) == E_ARG, i
    for i in (0, 1, 4):   # in, w_taps, out move 16 bytes per lane
        a = list(args)
        a[i] = bad
        assert run(a, 1, 14, 14, 64, 64, 2) == E_ARG, i
    assert run(args, 1, 14, 14, 48, 64, 2) == E_SHAPE
    assert run(args, 1, 14, 14, 64, 96, 2) == E_SHAPE
    assert run(args, 1, 14, 14, 64, 64, 0) == E_SHAPE
    assert run(args, 1, 65, 65, 512, 512, 15309) == E_SHAPE
    # in [1][16][16][64] is 65536 bytes: an out that starts inside it, or that it starts inside
    for out in ((1 << 20) + 65536 - 16, (1 << 20) - 65536 + 16, 1 << 20):
        a = list(args)
        a[4] = ctypes.c_void_p(out)
        assert run(a, 1, 14, 14, 64, 64, 2) == E_ARG, out
        assert "overlap" in L.wino_last_error_string().decode()
    assert L.wino_conv3x3_dilated_prepare_hw(1, 14, 14, 48, 64, 2, None) == E_SHAPE
    assert L.wino_conv3x3_dilated_prepare_hw(1, 14, 14, 64, 64, 0, None) == E_SHAPE


@pytest.mark.parametrize("proj", [False, True])
def test_block_refusals(pkg, proj):
    """Every refusal before the first launch, in the composer's order: NULL, alignment, shape, workspace size, overlap."""
    L = pkg.lib()
    base = 1 << 32
    ptrs = [ctypes.c_void_p(base + (i << 28)) for i in range(12)]
    bad = ctypes.c_void_p(base + 4)
    nt = 9 if proj else 11   # tensor pointers, out last
    args = ptrs[:nt]
    ws = ptrs[11]
    if proj:
        entry, ok = L.wino_dilated_proj_block_hw, (1, 14, 14, 64, 64, 128, 2)
        need = L.wino_proj_block_workspace_bytes_hw(1, 14, 14, 64)
        big = (1, 14, 14, 64, 64, 128)
    else:
        entry, ok = L.wino_dilated_residual_block_hw, (1, 14, 14, 128, 64, 2)
        need = L.wino_residual_block_workspace_bytes_hw(1, 14, 14, 64)
        big = (1, 14, 14, 128, 64)
    run = lambda a, *shape, ws_ptr=ws, ws_bytes=1 << 27: entry(*a, *shape, ws_ptr, ws_bytes, None)
    for i in range(nt):
        a = list(args)
        a[i] = None
        assert run(a, *ok) == E_ARG, i
    for i in ((0, 1, 4, 7, 8) if proj else (0, 1, 4, 7, 10)):   # x, w1, w2_taps, w3 / tail, out
        a = list(args)
        a[i] = bad
        assert run(a, *ok) == E_ARG, i
    assert run(args, *big, 0) == E_SHAPE                                  # dilation < 1
    assert run(args, *big, 1 << 30) == E_SHAPE                            # the 3x3's window over t1
    assert run(args, *((1, 14, 14, 64, 96, 128, 2) if proj else (1, 14, 14, 128, 96, 2))) == E_SHAPE   # Cm % 64
    assert run(args, *ok, ws_ptr=None) == E_ARG
    assert run(args, *ok, ws_ptr=bad) == E_ARG                            # misaligned workspace
    assert run(args, *ok, ws_bytes=need - 4) == E_ARG                     # short
    assert "workspace" in L.wino_last_error_string().decode()
    x_bytes = 14 * 14 * (64 if proj else 128) * 4
    for p in (args[0].value + x_bytes - 16, args[0].value - need + 16, args[-1].value):   # over x's end / start, at out
        assert run(args, *ok, ws_ptr=ctypes.c_void_p(p), ws_bytes=need) == E_ARG, p
        assert "overlaps" in L.wino_last_error_string().decode()
    prepare = L.wino_dilated_proj_block_prepare_hw if proj else L.wino_dilated_residual_block_prepare_hw
    assert prepare(*big, 0, None) == E_SHAPE


# ---- the tests' own reference, proven against torch ---------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(7, 7), (5, 9)])
@pytest.mark.parametrize("d", [1, 2, 3, 4, 12])
def test_reference_equals_torch(H, W, d):
    import torch
    rng = np.random.RandomState(10 * d + H)
    N, C, K = 2, 5, 3
    xp = np.zeros((N, H + 2, W + 2, C))
    xp[:, 1:-1, 1:-1, :] = rng.rand(N, H, W, C) - 0.5
    w, scale, bias = rng.rand(K, C, 3, 3) - 0.5, rng.rand(K) + 0.5, rng.rand(K) - 0.5
    for relu in (True, False):
        got = dilated_reference(xp, w, scale, bias, d, relu)
        x = torch.from_numpy(xp[:, 1:-1, 1:-1, :]).permute(0, 3, 1, 2)
        y = torch.nn.functional.conv2d(x, torch.from_numpy(w), padding=d, dilation=d)
        y = y * torch.from_numpy(scale)[None, :, None, None] + torch.from_numpy(bias)[None, :, None, None]
        want = (torch.relu(y) if relu else y).permute(0, 2, 3, 1).numpy()
        assert got.shape == want.shape == (N, H, W, K)
        assert np.abs(got - want).max() < 1e-13


@pytest.mark.parametrize("H,W", [(7, 7), (5, 9)])
@pytest.mark.parametrize("d", [1, 2, 3, 4, 12])
def test_footprint_equals_torch(H, W, d):
    """A NaN at one input pixel reaches exactly footprint() in torch's dilated convolution."""
    import torch
    w = torch.ones(1, 1, 3, 3, dtype=torch.float64)
    for y, x in ((0, 0), (H - 1, W - 1), (0, W // 2), (H // 2, W // 2), (H - 1, 0)):
        t = torch.zeros(1, 1, H, W, dtype=torch.float64)
        t[0, 0, y, x] = float("nan")
        out = torch.nn.functional.conv2d(t, w, padding=d, dilation=d)
        m = footprint(H, W, y, x, d)
        assert np.array_equal(torch.isnan(out)[0, 0].numpy(), m), (y, x)
        assert m[y, x] and 1 <= m.sum() <= 9


# ---- the networks' block kinds --------------------------------------------------------------------------------------
def test_resnet_block_kinds_follow_torchvision(pkg):
    R = importlib.import_module("cuda_winograd_amd.resnet")
    blocks = R.ARCHS["resnet50"][1]
    assert blocks == (3, 4, 6, 3)
    # torchvision: a dilated stage keeps stride 1; its first block runs at the previous dilation, the rest at the new
    want_ftt = [
        [("proj", 1)] + [("residual", 1)] * 2,
        [("proj_v15", 1)] + [("residual", 1)] * 3,
        [("proj", 1)] + [("dilated_residual", 2)] * 5,
        [("dilated_proj", 2)] + [("dilated_residual", 4)] * 2,
    ]
    assert R.dilated_block_plan((False, True, True), blocks) == want_ftt
    want_fft = [
        [("proj", 1)] + [("residual", 1)] * 2,
        [("proj_v15", 1)] + [("residual", 1)] * 3,
        [("proj_v15", 1)] + [("residual", 1)] * 5,
        [("proj", 1)] + [("dilated_residual", 2)] * 2,
    ]
    assert R.dilated_block_plan((False, False, True), blocks) == want_fft
    # no dilation: the plan is block_kind's
    plain = R.dilated_block_plan((False, False, False), blocks)
    for L, stage in enumerate(plain, 1):
        assert stage == [(R.block_kind(True, False, L, b == 0), 1) for b in range(len(stage))]
    # ResNet-101: 29 of its 33 blocks are dilated with (False, True, True)
    p101 = R.dilated_block_plan((False, True, True), R.ARCHS["resnet101"][1])
    assert sum(k.startswith("dilated") for st in p101 for k, _ in st) == 22 + 3
    assert sum(len(st) for st in p101[2:]) == 26
    for kind in ("dilated_residual", "dilated_proj"):
        assert kind in R.KINDS and R.KINDS[kind].stride == 1
    with pytest.raises(pkg.WinoError):
        R.dilated_block_plan((True, False, False), blocks)   # a stride-2 3x3 behind a dilated stage


def test_stage_shapes_and_refusals(pkg):
    R = importlib.import_module("cuda_winograd_amd.resnet")
    assert R.stage_shapes("resnet50", 224, 224) == R.stage_shapes("resnet50", 224, 224, (False, False, False))
    s = R.stage_shapes("resnet50", 520, 520, (False, True, True))
    assert [(c, h, w) for _, c, h, w in s[1:]] == [(256, 130, 130), (512, 65, 65), (1024, 65, 65), (2048, 65, 65)]
    s = R.stage_shapes("resnet50", 49, 81, (False, False, True))
    assert [(h, w) for _, _, h, w in s[1:]] == [(13, 21), (7, 11), (4, 6), (4, 6)]
    for arch in ("resnet18", "resnet34", "resnext50_32x4d", "resnext101_64x4d"):
        with pytest.raises(pkg.WinoError):
            R.stage_shapes(arch, 224, 224, (False, True, True))
        with pytest.raises(pkg.WinoError):
            R.ResNet(arch, 10, "cpu", (False, False, True))
        R.stage_shapes(arch, 224, 224, (False, False, False))
    with pytest.raises(pkg.WinoError):
        R.stage_shapes("resnet50", 224, 224, (True, True))
    assert R.ResNet("wide_resnet50_2", 10, "cpu", (False, True, True)).dilate == (False, True, True)
    assert R.ResNet("resnet50", 10, "cpu").dilate == (False, False, False)


def test_fcn_state_dict_keys(pkg):
    import torch
    S = importlib.import_module("cuda_winograd_amd.segmentation")
    exp = S.expected_fcn_keys("resnet50", 21)
    assert exp["classifier.0.weight"] == (512, 2048, 3, 3) and exp["classifier.4.weight"] == (21, 512, 1, 1)
    assert "backbone.layer4.2.conv3.weight" in exp and not any(k.startswith("backbone.fc") for k in exp)
    sd = {k: torch.empty(v) for k, v in exp.items()}
    sd["aux_classifier.0.weight"] = torch.empty(256, 1024, 3, 3)   # accepted and ignored
    assert S.validate_fcn_state_dict(sd, "resnet50") == 21
    bad = dict(sd)
    del bad["classifier.1.running_var"]
    with pytest.raises(pkg.WinoError, match="missing"):
        S.validate_fcn_state_dict(bad, "resnet50")
    bad = dict(sd, **{"backbone.fc.weight": torch.empty(1000, 2048)})
    with pytest.raises(pkg.WinoError, match="unexpected"):
        S.validate_fcn_state_dict(bad, "resnet50")
    with pytest.raises(pkg.WinoError):
        S.validate_fcn_state_dict(sd, "resnet18")
