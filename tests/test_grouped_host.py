"""Host-side checks of the grouped 3x3 layer (wino_conv3x3_grouped_*), the two ResNeXt blocks (wino_grouped_*_block_*)
and the five archs they open (resnext50_32x4d, resnext101_32x8d, resnext101_64x4d, wide_resnet50_2, wide_resnet101_2)
-- no GPU needed: the filter size query, every argument and shape rejection (each fires before the GPU is touched: on a
machine without one, anything later fails with WINO_E_HIP instead), the state-dict shapes, and flops() against a count
made here from those shapes."""
import ctypes
import importlib
import os

import pytest

from conftest import ROOT

E_SHAPE, E_ARG = -2, -3
NEW = ["wino_conv3x3_grouped_filter_elems", "wino_conv3x3_grouped_filter_pack", "wino_conv3x3_grouped_bn_relu_hw",
       "wino_conv3x3_grouped_plan", "wino_grouped_residual_block_hw", "wino_grouped_residual_block_prepare_hw", "wino_grouped_proj_block_hw",
       "wino_grouped_proj_block_prepare_hw"]
NEW_ARCHS = ["resnext50_32x4d", "resnext101_32x8d", "resnext101_64x4d", "wide_resnet50_2", "wide_resnet101_2"]
LEGAL_CG = (4, 8, 16, 32, 64)


@pytest.fixture(scope="module")
def R(pkg):
    return importlib.import_module("cuda_winograd_amd.resnet")


def test_new_symbols_exported_and_declared(pkg):
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "winograd_mi355x.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name + "(" in hdr, name
        assert name in pkg.ABI_SYMBOLS, name
    assert L.wino_abi_version() == 1
    # no size query of their own: the grouped blocks' workspaces are the dense blocks'
    assert not [s for s in pkg.ABI_SYMBOLS if "grouped" in s and "workspace_bytes" in s]


def test_filter_elems(pkg):
    L = pkg.lib()
    for C in (64, 128, 192, 1024, 2048):
        for Cg in LEGAL_CG:
            assert L.wino_conv3x3_grouped_filter_elems(C, C // Cg) > 0, (C, Cg)
            assert L.wino_conv3x3_grouped_filter_elems(C, C // Cg) >= 9 * C * Cg      # room for every weight
    for C, groups in ((96, 3), (96, 6), (128, 64), (128, 3), (128, 1), (256, 2), (64, 0), (64, -1), (0, 1), (-64, 1),
                      (64, 64), (64, 128), (100, 25)):
        assert L.wino_conv3x3_grouped_filter_elems(C, groups) == 0, (C, groups)
    assert L.wino_conv3x3_grouped_filter_elems(64, 1) > 0            # groups = 1 is legal at C = 64 only
    w, bad = ctypes.c_void_p(256), ctypes.c_void_p(264)
    assert L.wino_conv3x3_grouped_filter_pack(None, w, 128, 32, None) == E_ARG
    assert L.wino_conv3x3_grouped_filter_pack(w, None, 128, 32, None) == E_ARG
    assert L.wino_conv3x3_grouped_filter_pack(w, bad, 128, 32, None) == E_ARG
    assert L.wino_conv3x3_grouped_filter_pack(w, w, 96, 3, None) == E_SHAPE
    assert L.wino_conv3x3_grouped_filter_pack(w, w, 128, 64, None) == E_SHAPE


# (C, groups) the layer refuses with WINO_E_SHAPE: C = 96, Cg = 2, a `groups` that does not divide C, groups = 1 at
# C > 64
BAD_CHANNELS = ((96, 3), (128, 64), (128, 3), (128, 1))
# one padded image of exactly 2^31 elements, (Hin + 2) * (Win + 2) * C, and one above: (Hin, Win, C, groups)
AT_2_31 = (4094, 4094, 128, 32)
HUGE = (5791, 5791, 64, 16)      # 5793^2 * 64 = 2^31 + 6e5


def test_layer_rejections(pkg):
    L = pkg.lib()
    a, b, bad = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 40), ctypes.c_void_p((1 << 20) + 8)
    args = [a, a, a, a, b]   # in, packed, bnBias, bnScale, out

    def run(p, N=1, Hin=14, Win=14, C=128, groups=32, stride=1):
        return L.wino_conv3x3_grouped_bn_relu_hw(*p, N, Hin, Win, C, groups, stride, 1, None)

    for C, groups in BAD_CHANNELS:
        assert run(args, C=C, groups=groups) == E_SHAPE, (C, groups)
        assert "groups" in L.wino_last_error_string().decode()
    assert run(args, stride=3) == E_ARG
    assert run(args, stride=0) == E_ARG
    assert run(args, N=0) == E_SHAPE
    assert run(args, Hin=0) == E_SHAPE
    assert (AT_2_31[0] + 2) * (AT_2_31[1] + 2) * AT_2_31[2] == 1 << 31
    for Hin, Win, C, groups in (AT_2_31, HUGE):
        for stride in (1, 2):
            assert run(args, Hin=Hin, Win=Win, C=C, groups=groups, stride=stride) == E_SHAPE
            assert "2^31" in L.wino_last_error_string().decode()
    assert run(args, N=1 << 26, Hin=56, Win=56, C=64, groups=16) == E_SHAPE      # 2^26 * 7 * 7 workgroups
    for i in range(5):
        p = list(args)
        p[i] = None
        assert run(p) == E_ARG, i
    for i in (0, 1, 4):   # in, packed, out move 16 bytes per lane
        p = list(args)
        p[i] = bad
        assert run(p) == E_ARG, i
    # in and out overlap: the same tensor, and out starting inside in
    assert run([a, a, a, a, a]) == E_ARG
    assert "overlap" in L.wino_last_error_string().decode()
    inside = ctypes.c_void_p((1 << 20) + 16 * 16 * 128 * 4 - 16)
    assert run([a, b, b, b, inside]) == E_ARG


def test_plan_query(pkg):
    """wino_conv3x3_grouped_plan answers from the launcher's own geometry: the 8- or 16-wide tile that pads the output
    row by less, KC = max(Cg, 16), the tiles of one image; and it refuses what the layer refuses, with the same code."""
    L = pkg.lib()
    v = [ctypes.c_int(-1) for _ in range(4)]
    refs = [ctypes.byref(x) for x in v]
    for stride in (1, 2):
        for W in list(range(1, 70)) + [2895]:
            Win = 2 * W - 1 if stride == 2 else W
            for Cg in LEGAL_CG:
                tw, kc, ty, tx = pkg.conv3x3_grouped_plan(2, 11, Win, 128 if Cg < 64 else 64, (128 if Cg < 64 else 64) // Cg, stride)
                pad8, pad16 = -W % 8, -W % 16
                assert tw == (8 if pad8 < pad16 else 16), (stride, W, tw)
                assert kc == max(Cg, 16) and tx == -(-W // tw)
                H = 11 if stride == 1 else 6
                assert ty == -(-H // ((4 if stride == 1 else 2) * 16 // tw))
    assert [pkg.conv3x3_grouped_plan(1, 5, W, 64, 16)[0] for W in (8, 9, 16, 17, 24, 25, 32, 33)] == [8, 16, 16, 8, 8, 16, 16, 8]
    # ResNeXt at 224 x 224: 56 -> 8-wide, 28 and 14 -> 16-wide, 7 -> 8-wide
    assert [pkg.conv3x3_grouped_plan(1, h, h, 256, 32)[0] for h in (56, 28, 14, 7)] == [8, 16, 16, 8]
    for C, groups in BAD_CHANNELS:
        assert L.wino_conv3x3_grouped_plan(1, 14, 14, C, groups, 1, *refs) == E_SHAPE, (C, groups)
    assert L.wino_conv3x3_grouped_plan(1, 14, 14, 128, 32, 3, *refs) == E_ARG
    assert L.wino_conv3x3_grouped_plan(0, 14, 14, 128, 32, 1, *refs) == E_SHAPE
    Hin, Win, C, groups = HUGE
    assert L.wino_conv3x3_grouped_plan(1, Hin, Win, C, groups, 2, *refs) == E_SHAPE
    assert L.wino_conv3x3_grouped_plan(1, Hin - 1, Win - 1, C, groups, 2, *refs) == 0
    assert [x.value for x in v] == [16, 16, 1448, 181]
    for i in range(4):   # a NULL out-parameter
        p = list(refs)
        p[i] = None
        assert L.wino_conv3x3_grouped_plan(1, 14, 14, 128, 32, 1, *p) == E_ARG, i
    with pytest.raises(pkg.WinoError):
        pkg.conv3x3_grouped_plan(1, 14, 14, 96, 3)


def test_block_rejections(pkg):
    L = pkg.lib()
    w, bad = ctypes.c_void_p(256), ctypes.c_void_p(264)
    ws = 1 << 30

    def res(p, N=1, H=14, W=14, C4=256, Cm=128, groups=32, ws_ptr=w, ws_bytes=ws):
        return L.wino_grouped_residual_block_hw(*p, N, H, W, C4, Cm, groups, ws_ptr, ws_bytes, None)

    def proj(p, N=1, Hin=14, Win=14, Cin=64, Cm=128, C4=256, groups=32, stride=2, ws_ptr=w, ws_bytes=ws):
        return L.wino_grouped_proj_block_hw(*p, N, Hin, Win, Cin, Cm, C4, groups, stride, ws_ptr, ws_bytes, None)

    for run, nptr, tensors in ((res, 11, (0, 1, 4, 7, 10)), (proj, 9, (0, 1, 4, 7, 8))):
        args = [w] * nptr
        for Cm, groups in BAD_CHANNELS:
            assert run(args, Cm=Cm, groups=groups) == E_SHAPE, (run.__name__, Cm, groups)
        assert run(args, N=0) == E_SHAPE
        for i in range(nptr):
            p = list(args)
            p[i] = None
            assert run(p) == E_ARG, (run.__name__, i)
        for i in tensors:   # x, w1, wg, w3 / tail, out
            p = list(args)
            p[i] = bad
            assert run(p) == E_ARG, (run.__name__, i)
        assert run(args, ws_ptr=bad) == E_ARG
        assert run(args, ws_ptr=None) == E_ARG
    # an image at or above 2^31 elements in the middle layer
    H, W, Cm, groups = AT_2_31
    assert res([w] * 11, H=H, W=W, C4=64, Cm=Cm, groups=groups) == E_SHAPE
    assert "2^31" in L.wino_last_error_string().decode()
    assert proj([w] * 9, Hin=H, Win=W, Cin=32, Cm=Cm, C4=64, groups=groups, stride=1) == E_SHAPE
    assert "2^31" in L.wino_last_error_string().decode()
    assert proj([w] * 9, stride=3) == E_ARG
    assert proj([w] * 9, Cin=48) == E_SHAPE
    assert res([w] * 11, C4=96) == E_SHAPE
    # a workspace one byte short of the dense blocks' sizes
    need = L.wino_residual_block_workspace_bytes_hw(1, 14, 14, 128)
    assert res([w] * 11, ws_bytes=need - 1) == E_ARG
    assert "workspace" in L.wino_last_error_string().decode()
    need1 = L.wino_proj_block_workspace_bytes_hw(1, 14, 14, 128)
    assert proj([w] * 9, stride=1, ws_bytes=need1 - 1) == E_ARG
    need2 = L.wino_proj_block_v15_workspace_bytes_hw(1, 14, 14, 128)
    assert need2 < need1
    assert proj([w] * 9, stride=2, ws_bytes=need2 - 1) == E_ARG
    # the workspace overlaps x
    assert res([w] * 11, ws_ptr=w) == E_ARG
    assert "overlaps" in L.wino_last_error_string().decode()
    assert proj([w] * 9, ws_ptr=w) == E_ARG
    # the prepares check the same shapes
    assert L.wino_grouped_residual_block_prepare_hw(1, 14, 14, 256, 128, 64, None) == E_SHAPE
    assert L.wino_grouped_proj_block_prepare_hw(1, 14, 14, 64, 128, 256, 3, 2, None) == E_SHAPE
    assert L.wino_grouped_proj_block_prepare_hw(1, 14, 14, 64, 128, 256, 32, 3, None) == E_ARG


def test_expected_keys_of_the_new_archs(pkg, R):
    k = R.expected_keys("resnext50_32x4d", 1000)
    assert k["layer1.0.conv2.weight"] == (128, 4, 3, 3)
    assert k["layer4.2.conv2.weight"] == (1024, 32, 3, 3)
    assert R.expected_keys("resnext101_32x8d", 1000)["layer1.0.conv2.weight"] == (256, 8, 3, 3)
    assert R.expected_keys("resnext101_64x4d", 1000)["layer1.0.conv2.weight"] == (256, 4, 3, 3)
    k = R.expected_keys("wide_resnet50_2", 1000)
    assert k["layer1.0.conv2.weight"] == (128, 128, 3, 3)
    assert k["layer1.0.conv3.weight"] == (256, 128, 1, 1)
    assert k["fc.weight"] == (1000, 2048)
    for arch in NEW_ARCHS:
        assert len(R.ARCHS[arch]) == 2 and R.ARCHS[arch][0] is True
        # every grouped 3x3 is a shape the layer takes
        for key, shape in R.expected_keys(arch, 10).items():
            if key.endswith("conv2.weight") and shape[0] != shape[1]:
                assert pkg.lib().wino_conv3x3_grouped_filter_elems(shape[0], shape[0] // shape[1]) > 0, (arch, key)
    # the existing archs keep (1, 64): Cm = planes
    assert R.expected_keys("resnet50", 1000)["layer3.0.conv2.weight"] == (256, 256, 3, 3)
    assert R.mid_channels("resnet50", 256) == (1, 256)
    assert R.mid_channels("resnext101_64x4d", 512) == (64, 2048)


def _count_flops(R, arch, classes, H, W):
    """2 FLOPs per multiply-add of every convolution and of the FC, from the state-dict shapes and the stage maps."""
    keys = R.expected_keys(arch, classes)
    maps = {name: (h, w) for name, _, h, w in R.stage_shapes(arch, H, W)}
    hc, wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    total = 0.0
    for key, shape in keys.items():
        if len(shape) != 4:
            continue
        k, c, r, s = shape
        if key == "conv1.weight":
            px = hc * wc
        else:
            layer, block = key.split(".")[0], int(key.split(".")[1])
            h, w = maps[layer]
            if block == 0 and key.endswith("conv1.weight"):   # before the block's stride: the previous stage's map
                prev = "stem" if layer == "layer1" else f"layer{int(layer[-1]) - 1}"
                h, w = maps[prev]
            px = h * w
        total += 2.0 * px * k * c * r * s
    return total + 2.0 * keys["fc.weight"][0] * keys["fc.weight"][1]


@pytest.mark.parametrize("arch", NEW_ARCHS + ["resnet50"])
def test_flops_match_a_count_from_the_key_shapes(arch, pkg, R):
    m = R.ResNet.__new__(R.ResNet)      # flops() reads the block list only: build it from the shapes, no device
    m.arch, m.classes = arch, 1000
    m.bottleneck, m.blocks = R.ARCHS[arch]
    m.groups = R.WIDTHS.get(arch, (1, 64))[0]
    m.layers, cin = [], 64
    for L, (planes, nb) in enumerate(zip(R.PLANES, m.blocks), 1):
        cm, cout = R.mid_channels(arch, planes)[1], 4 * planes
        kinds = ["grouped_proj" if L == 1 else "grouped_proj_s2"] + ["grouped_residual"] * (nb - 1) if m.groups > 1 \
            else ["proj" if L == 1 else "proj_v15"] + ["residual"] * (nb - 1)
        m.layers.append([(kind, cin if i == 0 else cout, cm, cout, None) for i, kind in enumerate(kinds)])
        cin = cout
    m.feat_c = cin
    want = _count_flops(R, arch, 1000, 224, 224)
    assert m.flops(224, 224) == want, (arch, m.flops(224, 224), want)
    if arch == "resnext50_32x4d":
        assert 8.4e9 < want < 8.6e9     # torchvision quotes 4.23 GMACs
    if arch == "wide_resnet50_2":
        assert 22.6e9 < want < 23.0e9   # 11.4 GMACs


def test_wrong_state_dict_names_the_first_bad_key(pkg, R):
    import torch
    sd = {k: torch.zeros(s) for k, s in R.expected_keys("resnet50", 10).items()}
    with pytest.raises(pkg.WinoError, match=r"layer1\.0\.conv1\.weight"):
        R.validate_state_dict(sd, "resnext50_32x4d")
    sd = {k: torch.zeros(s) for k, s in R.expected_keys("resnext50_32x4d", 10).items()}
    assert R.validate_state_dict(sd, "resnext50_32x4d") == 10
    with pytest.raises(pkg.WinoError, match=r"layer1\.0\.conv2\.weight"):    # (conv1 is 64 -> 128 in both)
        R.validate_state_dict(sd, "wide_resnet50_2")
    with pytest.raises(pkg.WinoError, match="unknown arch"):
        R.expected_keys("resnext50_16x4d", 10)
