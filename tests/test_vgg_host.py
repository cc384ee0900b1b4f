"""Host-side checks of the VGG runner (cuda_winograd_amd.vgg) -- no GPU needed: torchvision's key names and shapes for
all eight architectures against a table written out here from its published configurations (torchvision itself is not
imported), every state-dict rejection, and the arithmetic of the flatten: the weight permutation of the first FC plus
a numpy model of AdaptiveAvgPool2d(7)'s bin rule against torch in fp64."""
import importlib

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def V(pkg):
    return importlib.import_module("cuda_winograd_amd.vgg")


# torchvision.models.vgg: the index of every Conv2d inside `features` and its output channels
CH = {
    "A": [64, 128, 256, 256, 512, 512, 512, 512],
    "B": [64, 64, 128, 128, 256, 256, 512, 512, 512, 512],
    "D": [64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512],
    "E": [64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512, 512, 512, 512],
}
TABLE = {
    "vgg11": ("A", [0, 3, 6, 8, 11, 13, 16, 18]),
    "vgg11_bn": ("A", [0, 4, 8, 11, 15, 18, 22, 25]),
    "vgg13": ("B", [0, 2, 5, 7, 10, 12, 15, 17, 20, 22]),
    "vgg13_bn": ("B", [0, 3, 7, 10, 14, 17, 21, 24, 28, 31]),
    "vgg16": ("D", [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]),
    "vgg16_bn": ("D", [0, 3, 7, 10, 14, 17, 20, 24, 27, 30, 34, 37, 40]),
    "vgg19": ("E", [0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28, 30, 32, 34]),
    "vgg19_bn": ("E", [0, 3, 7, 10, 14, 17, 20, 23, 27, 30, 33, 36, 40, 43, 46, 49]),
}
# the convolutions that are followed by MaxPool2d(2, 2), by position
POOLED = {"A": [0, 1, 3, 5, 7], "B": [1, 3, 5, 7, 9], "D": [1, 3, 6, 9, 12], "E": [1, 3, 7, 11, 15]}


def table_keys(arch, classes, hidden):
    cfg, idx = TABLE[arch]
    exp, cin = {}, 3
    for i, c in zip(idx, CH[cfg]):
        exp[f"features.{i}.weight"] = (c, cin, 3, 3)
        exp[f"features.{i}.bias"] = (c,)
        if arch.endswith("_bn"):
            for k in ("weight", "bias", "running_mean", "running_var"):
                exp[f"features.{i + 1}.{k}"] = (c,)
        cin = c
    exp.update({"classifier.0.weight": (hidden, 25088), "classifier.0.bias": (hidden,),
                "classifier.3.weight": (hidden, hidden), "classifier.3.bias": (hidden,),
                "classifier.6.weight": (classes, hidden), "classifier.6.bias": (classes,)})
    return exp


@pytest.mark.parametrize("arch", sorted(TABLE))
def test_expected_keys_match_torchvision(arch, V):
    assert V.expected_keys(arch, 1000, 4096) == table_keys(arch, 1000, 4096)
    assert V.expected_keys(arch, 10, 256) == table_keys(arch, 10, 256)
    assert set(V.ARCHS) == set(TABLE)
    cfg, idx = TABLE[arch]
    layers = V.conv_layers(arch)
    assert [l[0] for l in layers] == idx and [l[2] for l in layers] == CH[cfg]
    assert [j for j, l in enumerate(layers) if l[3]] == POOLED[cfg]


def _sd(arch, classes=10, hidden=128):
    sd = {k: torch.zeros(s) for k, s in table_keys(arch, classes, hidden).items()}
    if arch.endswith("_bn"):
        for k in list(sd):
            if k.endswith("running_var"):
                sd[k[: -len("running_var")] + "num_batches_tracked"] = torch.tensor(3)
    return sd


@pytest.mark.parametrize("arch", ["vgg11", "vgg16_bn"])
def test_validate_state_dict(arch, V, pkg):
    sd = _sd(arch)
    assert V.validate_state_dict(sd, arch) == (10, 128)    # num_batches_tracked tolerated
    for key in ("features.0.weight", "classifier.3.bias", "classifier.0.weight", "classifier.6.weight"):
        bad = dict(sd)
        del bad[key]
        with pytest.raises(pkg.WinoError, match=key.replace(".", r"\.")):
            V.validate_state_dict(bad, arch)
    bad = dict(sd)
    bad["features.1.weight" if arch == "vgg11" else "features.2.weight"] = torch.zeros(64)
    with pytest.raises(pkg.WinoError, match=r"unexpected key 'features\.[12]\.weight'"):
        V.validate_state_dict(bad, arch)
    bad = dict(sd)
    bad["features.0.weight"] = torch.zeros(64, 3, 5, 5)
    with pytest.raises(pkg.WinoError, match=r"'features\.0\.weight' has shape \(64, 3, 5, 5\)"):
        V.validate_state_dict(bad, arch)
    bad = dict(sd)
    bad["classifier.3.weight"] = torch.zeros(128, 64)
    with pytest.raises(pkg.WinoError, match=r"classifier\.3\.weight"):
        V.validate_state_dict(bad, arch)
    with pytest.raises(pkg.WinoError, match=r"classifier\.0\.weight.*100.*multiple of 64"):
        V.validate_state_dict(_sd(arch, hidden=100), arch)
    with pytest.raises(pkg.WinoError, match="unknown arch"):
        V.validate_state_dict(sd, "vgg12")
    with pytest.raises(pkg.WinoError, match="unknown arch"):
        V.expected_keys("resnet18", 10)


def test_vgg_is_exported_and_refuses_small_inputs(V, pkg):
    assert pkg.VGG is V.VGG
    m = V.VGG("vgg11", 10, 128, "cpu")
    for shape in ((1, 31, 64), (1, 64, 31), (0, 64, 64)):
        with pytest.raises(pkg.WinoError, match="32"):
            m.prepare(*shape)
    with pytest.raises(pkg.WinoError, match="CUDA"):
        V.VGG.from_state_dict(_sd("vgg11"), "vgg11", device="cpu")
    # flops: VGG-16 at 224x224 is 15.47 GMACs of convolutions and FCs
    m16 = V.VGG("vgg16", 1000, 4096, "cpu")
    m16.feat_c = 512
    assert abs(m16.flops() / 2 - 15.47e9) < 0.02e9
    shapes = V.layer_shapes("vgg16", 97, 131)
    assert [(h, w) for _, _, h, w, p in shapes if p] == [(97, 131), (48, 65), (24, 32), (12, 16), (6, 8)]


def _bins(H):
    """AdaptiveAvgPool2d(7) along one axis: bin i covers floor(i*H/7) .. ceil((i+1)*H/7) - 1."""
    return [(i * H // 7, -(-(i + 1) * H // 7)) for i in range(7)]


@pytest.mark.parametrize("H,W", [(7, 7), (1, 1), (8, 10), (13, 7)])
def test_flatten_arithmetic(H, W, V):
    """flatten_hwc(numpy bins) @ fc1_columns_hwc(W)^T == adaptive_avg_pool2d(x).flatten(1) @ W^T, fp64."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(H * 31 + W)
    N, C, hidden = 3, 8, 64
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(hidden, C * 49, generator=g, dtype=torch.float64)
    want = F.adaptive_avg_pool2d(x, (7, 7)).flatten(1) @ w.t()
    xn = x.permute(0, 2, 3, 1).numpy()                       # NHWC, what the kernel reads
    flat = np.empty((N, 7, 7, C))
    for i, (y0, y1) in enumerate(_bins(H)):
        for j, (x0, x1) in enumerate(_bins(W)):
            assert y1 > y0 and x1 > x0
            flat[:, i, j, :] = xn[:, y0:y1, x0:x1, :].mean(axis=(1, 2))
    got = flat.reshape(N, 49 * C) @ V.fc1_columns_hwc(w, C).numpy().T
    assert np.abs(got - want.numpy()).max() <= 1e-12 * np.abs(want.numpy()).max()
