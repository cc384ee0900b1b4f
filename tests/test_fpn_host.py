"""Host-side checks of the FPN neck -- no GPU needed: the refusals of WINO_RESIDUAL_UP2, the argument checks of
wino_fpn_level_hw before its first launch (the way tests/test_block_checks_host.py does it: fake addresses that are
never dereferenced; a call that got past the checks would return WINO_E_HIP on a machine without a GPU), ResNetFPN's
state-dict validation, and the fact the kernel rests on: torch's nearest upsampling from ceil(H/2) to H picks source
index dst >> 1."""
import ctypes
import importlib

import pytest

E_SHAPE, E_ARG = -2, -3
GIB = 1 << 30
RELU, A_PADDED, C_PADDED, ADD_RESIDUAL, UP2 = 1, 2, 4, 8, 16


@pytest.fixture(scope="module")
def FPN(pkg):
    return importlib.import_module("cuda_winograd_amd.fpn")


# ---- the flag ------------------------------------------------------------------------------------------------------
def _p(i):
    return None if i is None else ctypes.c_void_p(i * GIB)


def _ex_hw(L, flags, residual=5, shape=(2, 7, 7, 64, 64)):
    return L.wino_conv1x1_bn_ex_hw(_p(1), _p(2), _p(3), _p(4), _p(residual), _p(6), *shape, flags, None)


def _ex(L, flags, residual=5):
    return L.wino_conv1x1_bn_ex(_p(1), _p(2), _p(3), _p(4), _p(residual), _p(6), 196, 64, 64, flags, None)


def test_the_flag_is_the_next_free_bit(pkg):
    assert pkg.RESIDUAL_UP2 == UP2 == 16
    assert (pkg.RELU, pkg.A_PADDED, pkg.C_PADDED, pkg.ADD_RESIDUAL) == (RELU, A_PADDED, C_PADDED, ADD_RESIDUAL)


def test_up2_is_refused_where_it_has_no_meaning(pkg):
    L = pkg.lib()
    err = lambda: L.wino_last_error_string().decode()
    # the 14x14 M-form has no feature map to halve
    for extra in (0, RELU, A_PADDED | C_PADDED):
        assert _ex(L, ADD_RESIDUAL | UP2 | extra) == E_ARG
        assert "WINO_RESIDUAL_UP2" in err()
    # without WINO_ADD_RESIDUAL, with or without a residual pointer
    for extra in (0, RELU, A_PADDED, C_PADDED):
        assert _ex_hw(L, UP2 | extra) == E_ARG
        assert "WINO_ADD_RESIDUAL" in err()
        assert _ex_hw(L, UP2 | extra, residual=None) == E_ARG
    # with a null residual
    assert _ex_hw(L, ADD_RESIDUAL | UP2, residual=None) == E_ARG
    assert "residual" in err()
    # the next bit is still unknown, in both forms
    assert _ex_hw(L, 32) == E_ARG and "unknown flag" in err()
    assert _ex(L, 32) == E_ARG and "unknown flag" in err()
    # the shared argument checks hold with the flag: a misaligned coarse map, a shape the GEMM refuses
    assert L.wino_conv1x1_bn_ex_hw(_p(1), _p(2), _p(3), _p(4), ctypes.c_void_p(5 * GIB + 4), _p(6), 2, 7, 7, 64, 64,
                                   ADD_RESIDUAL | UP2, None) == E_ARG
    assert "16-byte aligned" in err()
    assert _ex_hw(L, ADD_RESIDUAL | UP2, shape=(2, 7, 7, 64, 96)) == E_SHAPE      # Kout % 64
    assert _ex_hw(L, ADD_RESIDUAL | UP2, shape=(2, 7, 7, 48, 64)) == E_SHAPE      # Cin % 32
    assert _ex_hw(L, ADD_RESIDUAL | UP2, shape=(2, 5000, 7, 64, 64)) == E_SHAPE   # feature map past 4094
    assert _ex_hw(L, ADD_RESIDUAL | UP2, shape=(0, 7, 7, 64, 64)) == E_SHAPE


# ---- wino_fpn_level_hw --------------------------------------------------------------------------------------------
KINDS = {"c": "t", "wl": "t", "lBias": "v", "lScale": "v", "top": "t", "inner": "t", "U": "t", "oBias": "v",
         "oScale": "v", "P": "t"}
ADDR = {name: (i + 1) * GIB for i, name in enumerate(KINDS)}
SHAPE = (2, 7, 7, 64, 64, 0)   # N, H, W, Cin, Cf, c_padded


def _level(L, shape=SHAPE, **override):
    a = dict(ADDR, **override)
    return L.wino_fpn_level_hw(*[None if a[n] is None else ctypes.c_void_p(a[n]) for n in KINDS], *shape, None)


def test_fpn_level_refuses_before_its_first_launch(pkg):
    L = pkg.lib()
    err = lambda: L.wino_last_error_string().decode()
    for arg, kind in KINDS.items():
        if arg != "top":                                              # (a NULL top is the coarsest level)
            assert _level(L, **{arg: None}) == E_ARG, arg
            assert "NULL" in err(), arg
        if kind == "t":
            assert _level(L, **{arg: ADDR[arg] + 4}) == E_ARG, arg
            assert "16-byte aligned" in err(), arg
    N, H, W, Cin, Cf, _ = SHAPE
    lvl = N * (H + 2) * (W + 2) * Cf * 4
    assert lvl > 256
    # inner inside P, inner inside c, top inside inner, top inside P (top is N x 6 x 6 x Cf)
    for kw in ({"inner": ADDR["P"] + 256}, {"inner": ADDR["c"] + 256}, {"P": ADDR["c"] + 256},
               {"top": ADDR["inner"] + 256}, {"top": ADDR["P"] + lvl - 256}):
        assert _level(L, **kw) == E_ARG, kw
        assert "overlap" in err(), kw
    # the padded stage input is the larger one: an inner right behind where the unpadded c would end lies inside it
    assert _level(L, shape=(N, H, W, Cin, Cf, 1), inner=ADDR["c"] + N * H * W * Cin * 4) == E_ARG
    assert "overlap" in err()
    # every layer's shape, before anything is launched
    for shape in ((0, 7, 7, 64, 64, 0), (2, 0, 7, 64, 64, 0), (2, 7, 7, 48, 64, 0), (2, 7, 7, 64, 96, 0),
                  (2, 7, 7, 64, 32, 0), (2, 4095, 7, 64, 64, 0), (1, 7, 7, 64, 8192, 0)):   # the last: C * K = 2^26
        assert _level(L, shape=shape) == E_SHAPE, shape
        assert L.wino_fpn_level_prepare_hw(*shape[:5], None) == E_SHAPE, shape


# ---- ResNetFPN's state dict -----------------------------------------------------------------------------------------
def _sd(FPN, arch, out_channels=256):
    import torch
    sd = {k: torch.zeros(v) for k, v in FPN.expected_fpn_keys(arch, out_channels).items()}
    for k in list(sd):
        if k.endswith("running_var"):
            sd[k] += 1
    return sd


def test_expected_keys_follow_torchvision(FPN):
    k50 = FPN.expected_fpn_keys("resnet50", 256)
    assert k50["body.conv1.weight"] == (64, 3, 7, 7) and k50["body.layer4.2.conv3.weight"] == (2048, 512, 1, 1)
    assert not [k for k in k50 if "fc." in k]
    assert [k50[f"fpn.inner_blocks.{i}.0.weight"] for i in range(4)] == [(256, c, 1, 1) for c in (256, 512, 1024, 2048)]
    assert all(k50[f"fpn.layer_blocks.{i}.0.weight"] == (256, 256, 3, 3) for i in range(4))
    assert all(k50[f"fpn.inner_blocks.{i}.0.bias"] == k50[f"fpn.layer_blocks.{i}.0.bias"] == (256,) for i in range(4))
    k18 = FPN.expected_fpn_keys("resnet18", 128)
    assert [k18[f"fpn.inner_blocks.{i}.0.weight"] for i in range(4)] == [(128, c, 1, 1) for c in (64, 128, 256, 512)]
    assert len([k for k in k50 if k.startswith("fpn.")]) == 16


@pytest.mark.parametrize("arch", ["resnet18", "resnet50", "resnext50_32x4d"])
def test_state_dict_errors_name_the_key(arch, pkg, FPN):
    """Raised on the host, before any device work (this test runs without a GPU)."""
    import torch
    sd = _sd(FPN, arch)
    FPN.validate_fpn_state_dict(sd, arch)
    tracked = dict(sd)
    tracked["body.bn1.num_batches_tracked"] = torch.tensor(0)          # optional
    FPN.validate_fpn_state_dict(tracked, arch)

    for key in ("fpn.inner_blocks.2.0.bias", "fpn.layer_blocks.0.0.weight", "body.layer3.1.bn2.running_mean"):
        missing = dict(sd)
        del missing[key]
        with pytest.raises(pkg.WinoError, match="missing key '" + key.replace(".", r"\.") + "'"):
            pkg.ResNetFPN.from_state_dict(missing, arch)
    for key in ("fpn.inner_blocks.4.0.weight", "fc.weight", "body.fc.weight", "conv1.weight"):
        extra = dict(sd)
        extra[key] = torch.zeros(1)
        with pytest.raises(pkg.WinoError, match="unexpected key '" + key.replace(".", r"\.") + "'"):
            pkg.ResNetFPN.from_state_dict(extra, arch)
    wrong = dict(sd)
    wrong["fpn.inner_blocks.1.0.weight"] = torch.zeros(256, 7, 1, 1)
    with pytest.raises(pkg.WinoError, match=r"fpn\.inner_blocks\.1\.0\.weight.*shape \(256, 7, 1, 1\)"):
        pkg.ResNetFPN.from_state_dict(wrong, arch)
    wrong = dict(sd)
    wrong["fpn.layer_blocks.3.0.weight"] = torch.zeros(256, 256, 1, 1)
    with pytest.raises(pkg.WinoError, match=r"fpn\.layer_blocks\.3\.0\.weight.*shape"):
        pkg.ResNetFPN.from_state_dict(wrong, arch)
    # another width of the pyramid is another set of shapes
    with pytest.raises(pkg.WinoError, match=r"fpn\.inner_blocks\.0\.0\.weight.*shape"):
        pkg.ResNetFPN.from_state_dict(sd, arch, out_channels=128)
    FPN.validate_fpn_state_dict(_sd(FPN, arch, 128), arch, 128)
    with pytest.raises(pkg.WinoError, match="multiple of 64"):
        FPN.validate_fpn_state_dict(sd, arch, 96)
    with pytest.raises(pkg.WinoError, match="unknown arch"):
        FPN.validate_fpn_state_dict(sd, "resnet20")


def test_every_arch_has_an_fpn_key_set(pkg, FPN):
    R = importlib.import_module("cuda_winograd_amd.resnet")
    for arch in R.ARCHS:
        FPN.validate_fpn_state_dict(_sd(FPN, arch), arch)
        exp = FPN.expected_fpn_keys(arch, 256)
        for i in range(4):                                   # every lateral fits the 1x1 kernels' Cin % 32
            assert exp[f"fpn.inner_blocks.{i}.0.weight"][1] % 32 == 0


def test_resnet_from_state_dict_still_needs_its_head(pkg):
    R = importlib.import_module("cuda_winograd_amd.resnet")
    assert "fc.weight" in R.expected_keys("resnet18", 10) and "fc.weight" not in R.expected_keys("resnet18", None)
    import torch
    sd = {k: torch.zeros(v) for k, v in R.expected_keys("resnet18", None).items()}
    with pytest.raises(pkg.WinoError, match=r"fc\.weight"):
        pkg.ResNet.from_state_dict(sd, "resnet18")


# ---- the fact the kernel rests on -------------------------------------------------------------------------------------
def test_torch_nearest_picks_dst_shift_1():
    """F.interpolate(size=H, mode="nearest") from Hc = (H+1)//2 reads source index dst >> 1, for every H in 1..4096
    (the kernel's (y >> 1, x >> 1)); checked along each axis of a 2-D interpolate as well, where both sizes differ."""
    import torch
    F = torch.nn.functional
    for H in range(1, 4097):
        Hc = (H + 1) // 2
        src = torch.arange(Hc, dtype=torch.float64).view(1, 1, Hc)
        got = F.interpolate(src, size=H, mode="nearest").view(-1).long()
        assert torch.equal(got, torch.arange(H) >> 1), H
    for H, W in ((7, 4), (5, 9), (1, 1), (2, 3), (13, 18), (200, 333)):
        Hc, Wc = (H + 1) // 2, (W + 1) // 2
        src = (torch.arange(Hc).view(Hc, 1) * 1000 + torch.arange(Wc).view(1, Wc)).double().view(1, 1, Hc, Wc)
        got = F.interpolate(src, size=(H, W), mode="nearest").view(H, W).long()
        want = (torch.arange(H).view(H, 1) >> 1) * 1000 + (torch.arange(W).view(1, W) >> 1)
        assert torch.equal(got, want), (H, W)
