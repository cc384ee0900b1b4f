"""Host-side checks of the concat projection (wino_conv1x1_cat_*), the ASPP module (wino_aspp_*) and DeepLabV3's state
dict -- no GPU needed: the C-ABI symbols, the plan (the GEMM's, never the latency form), every shape and argument
refusal (each fires before the GPU is touched), the workspace formula, and the tests' own fp64 ASPP reference proven
against a float64 torch composition."""
import ctypes
import importlib
import os

import numpy as np
import pytest

from aspp_cases import A_PADDED, C_PADDED, RELU, AsppCase, aspp_reference
from conftest import ROOT

E_SHAPE, E_ARG = -2, -3
NEW = ["wino_conv1x1_cat_bn_hw", "wino_conv1x1_cat_prepare_hw", "wino_conv1x1_cat_plan", "wino_aspp_hw",
       "wino_aspp_prepare_hw"]


def test_new_symbols_exported_and_declared(pkg):
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "winograd_mi355x.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name + "(" in hdr, name
        assert name in pkg.SIGNATURES, name
    assert L.wino_abi_version() == 1
    for name in ("conv1x1_cat_bn", "conv1x1_cat_prepare", "conv1x1_cat_plan", "aspp", "aspp_prepare",
                 "aspp_workspace_bytes", "DeepLabV3"):
        assert hasattr(pkg, name), name


# ---- the tests' own reference, proven against torch ---------------------------------------------------------------------
def test_aspp_reference_equals_torch():
    """conv2d with dilation, adaptive_avg_pool2d, bilinear interpolate of the 1x1 map, cat and conv2d, in float64."""
    import torch
    F = torch.nn.functional
    N, H, W, Cin, Cb, Kout, rates = 2, 5, 7, 32, 64, 64, (1, 2, 6)
    c = AsppCase(None, (torch, "cpu"), N, H, W, Cin, Cb, Kout, rates, seed=1)
    d = lambda a: a.double()
    nchw = lambda a: d(a).permute(0, 3, 1, 2)
    mat = lambda w: d(w).t()[:, :, None, None]                       # [Cin][K] -> [K][Cin][1][1]
    act = lambda t, bn: torch.relu(t * d(bn[1])[None, :, None, None] + d(bn[0])[None, :, None, None])
    x = nchw(c.x[:, 1:-1, 1:-1, :])
    branches = [act(F.conv2d(x, mat(c.w0)), c.bn[0])]
    for w, bn, r in zip(c.ws, c.bn[1:4], rates):
        branches.append(act(F.conv2d(x, d(w), padding=r, dilation=r), bn))
    p = act(F.conv2d(F.adaptive_avg_pool2d(x, 1), mat(c.w_pool)), c.bn[4])
    branches.append(F.interpolate(p, size=(H, W), mode="bilinear", align_corners=False))
    want = act(F.conv2d(torch.cat(branches, dim=1), mat(c.w_proj)), c.bn[5]).permute(0, 2, 3, 1).numpy()
    got = c.reference()
    assert got.shape == want.shape == (N, H, W, Kout)
    assert np.abs(got - want).max() < 1e-12
    # the images' means differ and the pooled branch carries weight in every image
    assert min(c.pooled_share()) > 1e-2
    n = lambda a: a.numpy()
    bn = [(n(b), n(s)) for b, s in c.bn]
    again = aspp_reference(n(c.x), n(c.w0), bn[0], [n(w) for w in c.ws], bn[1:4], rates, n(c.w_pool), bn[4],
                           n(c.w_proj), bn[5])
    assert np.array_equal(again, got)


# ---- the plan -------------------------------------------------------------------------------------------------------------
def _plan(pkg, N, H, W, S, Cs, Kout, cus=256):
    f = ctypes.c_int(-1)
    rc = pkg.lib().wino_conv1x1_cat_plan(N, H, W, S, Cs, Kout, cus, ctypes.byref(f))
    return rc, f.value


def _gemm_plan(pkg, M, Cin, Kout, cus=256):
    v = [ctypes.c_int(0) for _ in range(5)]
    assert pkg.lib().wino_conv1x1_plan(M, Cin, Kout, cus, *[ctypes.byref(x) for x in v]) == 0
    grid, row_tiles, col_blocks, k_steps, stream_k = (x.value for x in v)
    return {"grid": grid, "row_tiles": row_tiles, "waves": Kout // col_blocks // 16, "k_steps": k_steps,
            "stream_k": stream_k}


SHAPES = [(1, 65, 65, 4, 256, 256), (8, 65, 65, 4, 256, 256), (2, 28, 28, 4, 64, 256), (3, 15, 13, 5, 96, 128),
          (1, 1, 1, 2, 32, 64), (8, 1, 1, 4, 64, 128), (1, 14, 14, 8, 32, 64), (64, 14, 14, 2, 512, 512)]


def test_plan_is_the_gemms_and_never_the_latency_form(pkg, knobs):
    for k in ("WINO_1X1_ALGO", "WINO_1X1_SMALL_KS", "WINO_1X1_SK", "WINO_1X1_SK_GRID"):
        knobs.unset(k)
    for cus in (256, 64):
        for s in SHAPES:
            N, H, W, S, Cs, Kout = s
            rc, form = _plan(pkg, *s, cus=cus)
            assert rc == 0, s
            want = pkg.FORM_STREAM_K if _gemm_plan(pkg, N * H * W, S * Cs, Kout, cus)["stream_k"] else pkg.FORM_TILED
            assert form == want, (s, cus)
    knobs.set("WINO_1X1_ALGO", "small")
    for s in SHAPES:
        assert pkg.conv1x1_cat_plan(*s) in (pkg.FORM_TILED, pkg.FORM_STREAM_K), s
    knobs.set("WINO_1X1_ALGO", "big")
    knobs.set("WINO_1X1_SK", 0)
    assert pkg.conv1x1_cat_plan(2, 28, 28, 4, 64, 256) == pkg.FORM_TILED
    knobs.set("WINO_1X1_SK", 1)
    assert pkg.conv1x1_cat_plan(2, 28, 28, 4, 64, 256) == pkg.FORM_STREAM_K
    # the forced-form shapes of tests/test_gpu_aspp.py: one plans 8-wave tiles, the other 4-wave tiles
    assert _gemm_plan(pkg, 2 * 28 * 28, 4 * 64, 256)["waves"] == 8
    assert _gemm_plan(pkg, 3 * 15 * 13, 5 * 96, 128)["waves"] == 4


def test_plan_and_prepare_refusals(pkg):
    L = pkg.lib()
    err = lambda: L.wino_last_error_string().decode()
    assert _plan(pkg, 2, 9, 9, 4, 64, 64)[0] == 0
    assert _plan(pkg, 2, 9, 9, 4, 48, 64)[0] == E_SHAPE and "Cs" in err()           # Cs % 32
    assert _plan(pkg, 2, 9, 9, 4, 64, 96)[0] == E_SHAPE and "Kout" in err()         # Kout % 64
    for s in (1, 0, -1, 9):
        assert _plan(pkg, 2, 9, 9, s, 64, 64)[0] == E_SHAPE and "sources" in err(), s
    for s in (2, 8):
        assert _plan(pkg, 2, 9, 9, s, 64, 64)[0] == 0, s
    assert _plan(pkg, 0, 9, 9, 4, 64, 64)[0] == E_SHAPE
    assert _plan(pkg, 2, 9, 0, 4, 64, 64)[0] == E_SHAPE
    assert _plan(pkg, 1 << 22, 28, 28, 2, 32, 64)[0] == E_SHAPE                     # M = N*H*W < 2^31
    assert _plan(pkg, 2, 9, 9, 4, 64, 64, cus=0)[0] == E_ARG
    assert L.wino_conv1x1_cat_plan(2, 9, 9, 4, 64, 64, 256, None) == E_ARG
    assert L.wino_conv1x1_cat_prepare_hw(2, 9, 9, 4, 48, 64, None) == E_SHAPE
    assert L.wino_conv1x1_cat_prepare_hw(2, 9, 9, 1, 64, 64, None) == E_SHAPE
    assert L.wino_aspp_prepare_hw(1, 9, 9, 64, 64, 64, 1, 0, 3, None) == E_SHAPE and "dilation" in err()
    assert L.wino_aspp_prepare_hw(1, 9, 9, 48, 64, 64, 1, 2, 3, None) == E_SHAPE    # Cin % 32
    assert L.wino_aspp_prepare_hw(1, 9, 9, 64, 96, 64, 1, 2, 3, None) == E_SHAPE    # Cb % 64
    assert L.wino_aspp_prepare_hw(1, 9, 9, 64, 64, 96, 1, 2, 3, None) == E_SHAPE    # Kout % 64


# ---- the concat layer's refusals ---------------------------------------------------------------------------------------
P = lambda v: ctypes.c_void_p(v)
SRC, W_, BIAS, SCALE, OUT = 1 << 32, 2 << 32, 3 << 32, 4 << 32, 5 << 32   # far apart: nothing overlaps by accident


def _cat(pkg, ptrs=None, stride=None, shape=(2, 9, 9, 4, 64, 64), flags=RELU):
    N, H, W, S, Cs, Kout = shape
    ptrs = ptrs or [P(SRC), P(W_), P(BIAS), P(SCALE), P(OUT)]
    if stride is None:
        stride = N * H * W * Cs
    src, w, bias, scale, out = ptrs
    return pkg.lib().wino_conv1x1_cat_bn_hw(src, stride, w, bias, scale, out, N, H, W, S, Cs, Kout, flags, None)


def test_cat_layer_refusals(pkg):
    L = pkg.lib()
    err = lambda: L.wino_last_error_string().decode()
    ok = [P(SRC), P(W_), P(BIAS), P(SCALE), P(OUT)]
    for i in range(5):
        a = list(ok)
        a[i] = None
        assert _cat(pkg, a) == E_ARG and "NULL" in err(), i
    for i in (0, 1, 2, 4):   # src, w, bias_per_image (read 16 bytes per lane), out
        a = list(ok)
        a[i] = P(a[i].value + 4)
        assert _cat(pkg, a) == E_ARG and "aligned" in err(), i
    for flags in (8, 16, 1 << 16, RELU | 32, -1):   # ADD_RESIDUAL, RESIDUAL_UP2, the internal no-BN bit, ...
        assert _cat(pkg, flags=flags) == E_ARG and "flag" in err(), flags
    assert _cat(pkg, shape=(2, 9, 9, 4, 48, 64)) == E_SHAPE and "Cs" in err()
    assert _cat(pkg, shape=(2, 9, 9, 4, 64, 96)) == E_SHAPE
    for s in (1, 9):
        assert _cat(pkg, shape=(2, 9, 9, s, 64, 64)) == E_SHAPE and "sources" in err()
    n = 2 * 9 * 9 * 64                                                        # an unpadded source, in floats
    for stride in (n + 2, n + 1, -4):
        assert _cat(pkg, stride=stride) == E_SHAPE and "multiple of 4" in err(), stride
    assert _cat(pkg, stride=n - 4) == E_SHAPE and "smaller than a source" in err()
    npad = 2 * 11 * 11 * 64                                                   # a padded source is larger
    assert _cat(pkg, stride=npad - 4, flags=A_PADDED) == E_SHAPE and "smaller than a source" in err()
    # The window: (rows * Cs + (S-1) * src_stride) * 4 bytes < 2^32, rows = 112 or, padded, 111 (2 (W+2) + 3) + 1.
    # A call that passes it is recognised without a launch: out placed on src is refused as an overlap, the next check.
    on_src = [P(SRC), P(W_), P(BIAS), P(SCALE), P(SRC)]
    lim = ((1 << 30) - 112 * 64 - 1) // 3                                     # S = 4, Cs = 64, unpadded
    lim -= lim % 4
    assert ((112 * 64 + 3 * lim) * 4 < 1 << 32) and ((112 * 64 + 3 * (lim + 4)) * 4 >= 1 << 32)
    assert _cat(pkg, stride=lim + 4) == E_SHAPE and "window" in err()
    assert _cat(pkg, on_src, stride=lim) == E_ARG and "overlap" in err()
    rows = 111 * (2 * 11 + 3) + 1
    lim = ((1 << 30) - rows * 64 - 1) // 3
    lim -= lim % 4
    assert ((rows * 64 + 3 * lim) * 4 < 1 << 32) and ((rows * 64 + 3 * (lim + 4)) * 4 >= 1 << 32)
    assert _cat(pkg, stride=lim + 4, flags=A_PADDED) == E_SHAPE and "window" in err()
    assert _cat(pkg, on_src, stride=lim, flags=A_PADDED) == E_ARG and "overlap" in err()
    assert _cat(pkg, stride=1 << 40) == E_SHAPE and "window" in err()
    # overlaps: the sources' span is (S-1) * stride + one source; out [2][9][9][64]
    span, out_b = (3 * n + n) * 4, n * 4
    for out in (SRC, SRC + span - 16, SRC - out_b + 16):
        assert _cat(pkg, [P(SRC), P(W_), P(BIAS), P(SCALE), P(out)]) == E_ARG and "overlap" in err(), out
    for bias in (OUT, OUT + out_b - 16, SRC + span - 16):                       # bias_per_image on out, on the sources
        assert _cat(pkg, [P(SRC), P(W_), P(bias), P(SCALE), P(OUT)]) == E_ARG and "overlap" in err(), bias
    # the padded output is larger: an out whose ring reaches the bias
    assert _cat(pkg, [P(SRC), P(W_), P(OUT + out_b), P(SCALE), P(OUT)], flags=C_PADDED) == E_ARG and "overlap" in err()


# ---- the module's refusals ---------------------------------------------------------------------------------------------
def _aspp(pkg, ptrs=None, shape=(1, 9, 9, 64, 64, 64), rates=(1, 2, 3), ws=None, ws_bytes=None):
    ptrs = ptrs or [P((i + 1) << 32) for i in range(20)]
    need = pkg.aspp_workspace_bytes(*shape)
    ws = P(30 << 32) if ws is None else ws
    return pkg.lib().wino_aspp_hw(*ptrs, *shape, *rates, ws, need if ws_bytes is None else ws_bytes, None)


def test_aspp_refusals(pkg):
    """Every refusal before the first launch, in the blocks' order: NULL, alignment, shape, workspace size, overlap."""
    L = pkg.lib()
    err = lambda: L.wino_last_error_string().decode()
    ok = [P((i + 1) << 32) for i in range(20)]
    for i in range(20):
        a = list(ok)
        a[i] = None
        assert _aspp(pkg, a) == E_ARG and "NULL" in err(), i
    for i in (0, 1, 4, 7, 10, 13, 16, 19):   # in, w0, the three tap matrices, w_pool, w_proj, out
        a = list(ok)
        a[i] = P(a[i].value + 4)
        assert _aspp(pkg, a) == E_ARG and "aligned" in err(), i
    assert _aspp(pkg, ws=P((30 << 32) + 4)) == E_ARG and "aligned" in err()
    for rates in ((0, 2, 3), (1, -2, 3), (1, 2, 0)):
        assert _aspp(pkg, rates=rates) == E_SHAPE and "dilation" in err(), rates
    assert _aspp(pkg, rates=(1, 2, 1 << 30)) == E_SHAPE and "window" in err()
    assert _aspp(pkg, shape=(1, 9, 9, 48, 64, 64)) == E_SHAPE
    assert _aspp(pkg, shape=(1, 9, 9, 64, 96, 64)) == E_SHAPE
    assert _aspp(pkg, shape=(1, 9, 9, 64, 64, 96)) == E_SHAPE
    assert _aspp(pkg, shape=(0, 9, 9, 64, 64, 64), ws_bytes=1 << 20) == E_SHAPE
    need = pkg.aspp_workspace_bytes(1, 9, 9, 64, 64, 64)
    assert L.wino_aspp_hw(*ok, 1, 9, 9, 64, 64, 64, 1, 2, 3, None, need, None) == E_ARG
    assert _aspp(pkg, ws_bytes=need - 4) == E_ARG and "workspace" in err() and str(need) in err()
    # exactly `need` bytes pass the size check: placed on `in`, such a workspace is refused as an overlap, the next check
    in_b, out_b = 11 * 11 * 64 * 4, 11 * 11 * 64 * 4
    for p in (ok[0].value, ok[0].value + in_b - 16, ok[0].value - need + 16, ok[19].value + out_b - 16):
        assert _aspp(pkg, ws=P(p)) == E_ARG and "overlap" in err(), p
    a = list(ok)
    a[19] = P(ok[0].value + in_b - 16)                                       # out on in
    assert _aspp(pkg, a) == E_ARG and "overlap" in err()


def test_workspace_formula(pkg):
    """The pooled vector [N][Cin], its branch [N][Cb], the bias [N][Kout], each rounded up to 256 bytes, then four
    unpadded [N][H][W][Cb] slots; 0 for a dimension below 1."""
    r256 = lambda b: -(-b // 256) * 256
    for N, H, W, Cin, Cb, Kout in [(1, 9, 9, 64, 64, 64), (3, 5, 5, 96, 128, 64), (1, 65, 65, 2048, 256, 256),
                                   (8, 65, 65, 2048, 256, 256), (5, 1, 1, 32, 64, 192)]:
        want = r256(4 * N * Cin) + r256(4 * N * Cb) + r256(4 * N * Kout) + 4 * 4 * N * H * W * Cb
        assert pkg.aspp_workspace_bytes(N, H, W, Cin, Cb, Kout) == want
        assert want % 16 == 0
    assert pkg.aspp_workspace_bytes(3, 5, 5, 96, 128, 64) == 1280 + 1536 + 768 + 4 * 38400
    for bad in [(0, 9, 9, 64, 64, 64), (1, 9, 0, 64, 64, 64), (1, 9, 9, 64, 64, -64)]:
        assert pkg.aspp_workspace_bytes(*bad) == 0


# ---- DeepLabV3's state dict ----------------------------------------------------------------------------------------------
def test_deeplabv3_state_dict_keys(pkg):
    import torch
    S = importlib.import_module("cuda_winograd_amd.segmentation")
    exp = S.expected_deeplabv3_keys("resnet50", 21)
    assert exp["classifier.0.convs.0.0.weight"] == (256, 2048, 1, 1)
    assert exp["classifier.0.convs.2.0.weight"] == (256, 2048, 3, 3) and exp["classifier.0.convs.3.1.running_var"] == (256,)
    assert exp["classifier.0.convs.4.1.weight"] == (256, 2048, 1, 1) and exp["classifier.0.convs.4.2.bias"] == (256,)
    assert exp["classifier.0.project.0.weight"] == (256, 1280, 1, 1) and exp["classifier.0.project.1.weight"] == (256,)
    assert exp["classifier.1.weight"] == (256, 256, 3, 3) and exp["classifier.2.running_mean"] == (256,)
    assert exp["classifier.4.weight"] == (21, 256, 1, 1) and exp["classifier.4.bias"] == (21,)
    assert "backbone.layer4.2.conv3.weight" in exp and not any(k.startswith("backbone.fc") for k in exp)
    assert len(S.expected_deeplabv3_keys("resnet101", 21)) > len(exp)
    sd = {k: torch.empty(v) for k, v in exp.items()}
    sd["aux_classifier.0.weight"] = torch.empty(256, 1024, 3, 3)   # accepted and ignored
    sd["classifier.0.project.1.num_batches_tracked"] = torch.tensor(1)
    assert S.validate_deeplabv3_state_dict(sd, "resnet50") == 21
    bad = dict(sd)
    del bad["classifier.0.convs.4.2.running_var"]
    with pytest.raises(pkg.WinoError, match="missing key 'classifier.0.convs.4.2.running_var'"):
        S.validate_deeplabv3_state_dict(bad, "resnet50")
    bad = dict(sd, **{"classifier.0.convs.5.0.weight": torch.empty(256, 2048, 3, 3)})
    with pytest.raises(pkg.WinoError, match="unexpected key 'classifier.0.convs.5.0.weight'"):
        S.validate_deeplabv3_state_dict(bad, "resnet50")
    bad = dict(sd, **{"classifier.0.project.0.weight": torch.empty(256, 1024, 1, 1)})
    with pytest.raises(pkg.WinoError, match="'classifier.0.project.0.weight' has shape"):
        S.validate_deeplabv3_state_dict(bad, "resnet50")
    bad = dict(sd)
    del bad["classifier.4.weight"]
    with pytest.raises(pkg.WinoError, match="missing"):
        S.validate_deeplabv3_state_dict(bad, "resnet50")
    with pytest.raises(pkg.WinoError):
        S.validate_deeplabv3_state_dict(sd, "resnet18")
    # an FCN state dict is not a DeepLabV3 one
    F = S.expected_fcn_keys("resnet50", 21)
    with pytest.raises(pkg.WinoError):
        S.validate_deeplabv3_state_dict({k: torch.empty(v) for k, v in F.items()}, "resnet50")
