"""Host-side checks of the whole-network module (cuda_winograd_amd.resnet) -- no GPU needed: the stage shapes it
computes equal torch's (small fp64 F.conv2d / F.max_pool2d shape runs on the CPU), the torchvision key layout it
expects, and state-dict validation errors that name the key, raised before any device work."""
import importlib

import pytest

ARCHS = ["resnet18", "resnet34", "resnet50", "resnet101", "resnet152"]
SIZES = [(224, 224), (97, 131), (299, 299), (1, 1)]


@pytest.fixture(scope="module")
def R(pkg):
    return importlib.import_module("cuda_winograd_amd.resnet")


def _torch_stage_shapes(arch, H, W, R):
    """The spatial sizes of torchvision's stem and four stages, by running one-channel fp64 convolutions with the
    same kernels, strides and paddings as the real network (both branches of every downsampling block)."""
    import torch
    import torch.nn.functional as F
    bottleneck, _ = R.ARCHS[arch]
    t = torch.zeros(1, 1, H, W, dtype=torch.float64)
    t = F.max_pool2d(F.conv2d(t, torch.zeros(1, 1, 7, 7, dtype=torch.float64), stride=2, padding=3), 3, 2, 1)
    shapes = [tuple(t.shape[2:])]
    k1 = torch.zeros(1, 1, 1, 1, dtype=torch.float64)
    k3 = torch.zeros(1, 1, 3, 3, dtype=torch.float64)
    for L in range(4):
        s = 1 if L == 0 else 2
        if bottleneck:
            y = F.conv2d(F.conv2d(F.conv2d(t, k1), k3, stride=s, padding=1), k1)
        else:
            y = F.conv2d(F.conv2d(t, k3, stride=s, padding=1), k3, padding=1)
        sc = F.conv2d(t, k1, stride=s)
        assert y.shape == sc.shape
        t = y
        shapes.append(tuple(t.shape[2:]))
    return shapes


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_stage_shapes_match_torch(arch, H, W, R):
    got = R.stage_shapes(arch, H, W)
    assert [(h, w) for _, _, h, w in got] == _torch_stage_shapes(arch, H, W, R)
    assert [name for name, _, _, _ in got] == ["stem", "layer1", "layer2", "layer3", "layer4"]
    exp = 4 if arch == "resnet50" else 1
    assert [c for _, c, _, _ in got] == [64, 64 * exp, 128 * exp, 256 * exp, 512 * exp]


def test_expected_keys_follow_torchvision(R):
    k18 = R.expected_keys("resnet18", 1000)
    assert k18["conv1.weight"] == (64, 3, 7, 7) and k18["fc.weight"] == (1000, 512)
    assert "layer1.0.downsample.0.weight" not in k18
    assert k18["layer2.0.downsample.0.weight"] == (128, 64, 1, 1)
    assert k18["layer2.0.conv1.weight"] == (128, 64, 3, 3)
    k50 = R.expected_keys("resnet50", 10)
    assert k50["layer1.0.downsample.0.weight"] == (256, 64, 1, 1)       # stride 1, 64 -> 256
    assert k50["layer2.0.conv2.weight"] == (128, 128, 3, 3)              # v1.5: the stride sits on the 3x3
    assert k50["layer4.2.conv3.weight"] == (2048, 512, 1, 1)
    assert k50["fc.weight"] == (10, 2048)
    # conv + BN tensors per arch: 2 + 5 * blocks (+ 5 per downsample) for basic nets, 2 + 15 * blocks (+5) otherwise
    n_weights = {a: sum(1 for k in R.expected_keys(a, 1000) if k.endswith("conv1.weight") or k.endswith("conv2.weight")
                        or k.endswith("conv3.weight") or k.endswith("downsample.0.weight")) for a in ARCHS}
    assert n_weights == {"resnet18": 1 + 16 + 3, "resnet34": 1 + 32 + 3, "resnet50": 1 + 48 + 4,
                         "resnet101": 1 + 99 + 4, "resnet152": 1 + 150 + 4}


def _sd(R, arch, classes=1000):
    import torch
    sd = {k: torch.zeros(v) for k, v in R.expected_keys(arch, classes).items()}
    for k in list(sd):
        if k.endswith("running_var"):
            sd[k] += 1
            sd[k[: -len("running_var")] + "num_batches_tracked"] = torch.tensor(0)
    return sd


@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_state_dict_errors_name_the_key(arch, pkg, R):
    import torch
    sd = _sd(R, arch)
    assert R.validate_state_dict(sd, arch) == 1000
    nb = {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}   # optional
    assert R.validate_state_dict(nb, arch) == 1000

    missing = dict(sd)
    del missing["layer3.1.bn2.running_mean"]
    with pytest.raises(pkg.WinoError, match=r"missing key 'layer3\.1\.bn2\.running_mean'"):
        pkg.ResNet.from_state_dict(missing, arch)
    extra = dict(sd)
    extra["layer5.0.conv1.weight"] = torch.zeros(1)
    with pytest.raises(pkg.WinoError, match=r"unexpected key 'layer5\.0\.conv1\.weight'"):
        pkg.ResNet.from_state_dict(extra, arch)
    wrong = dict(sd)
    wrong["layer2.0.conv2.weight"] = torch.zeros(128, 128, 1, 1)
    with pytest.raises(pkg.WinoError, match=r"layer2\.0\.conv2\.weight.*shape"):
        pkg.ResNet.from_state_dict(wrong, arch)
    nofc = {k: v for k, v in sd.items() if k != "fc.weight"}
    with pytest.raises(pkg.WinoError, match=r"fc\.weight"):
        pkg.ResNet.from_state_dict(nofc, arch)
    # a state dict of the other family names its first foreign key
    other = "resnet50" if arch == "resnet18" else "resnet18"
    with pytest.raises(pkg.WinoError, match=r"key '"):
        R.validate_state_dict(_sd(R, other), arch)
    with pytest.raises(pkg.WinoError, match="unknown arch"):
        R.validate_state_dict(sd, "resnet20")


def test_any_class_count(R):
    assert R.validate_state_dict(_sd(R, "resnet34", classes=10), "resnet34") == 10
