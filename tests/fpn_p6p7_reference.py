"""fp64 CPU reference of torchvision's RetinaNet backbone for tests/test_gpu_fpn_p6p7.py and the RetinaNet tests:
BackboneWithFPN(returned_layers=[2, 3, 4], extra_blocks=LastLevelP6P7(256, 256)) read off a state dict, and random
weights in its key names (the recipe of fpn_reference.fpn_random_state_dict with the three levels' indices and the two
extra convolutions)."""
from reference_nets import random_state_dict, reference_forward

RETURNED = (2, 3, 4)


def p6p7_random_state_dict(torch, R, arch, out_channels=256, seed=0):
    """(sd, body): sd under body.* / fpn.inner_blocks.0..2 / fpn.layer_blocks.0..2 / fpn.extra_blocks.p6|p7, and the plain
    ResNet state dict `body` (with an fc) the fp64 reference forward reads."""
    body = random_state_dict(torch, R, arch, classes=8, seed=seed)
    sd = {"body." + k: v for k, v in body.items() if not k.startswith("fc.")}
    g = torch.Generator().manual_seed(seed + 777)
    stage_c = [c for _, c, _, _ in R.stage_shapes(arch, 64, 64)[1:]]
    conv3 = lambda: torch.randn(out_channels, out_channels, 3, 3, generator=g) * (1.0 / (9 * out_channels)) ** 0.5
    bias = lambda: (torch.rand(out_channels, generator=g) - 0.5) * 0.2
    for i, layer in enumerate(RETURNED):
        c = stage_c[layer - 1]
        sd[f"fpn.inner_blocks.{i}.0.weight"] = torch.randn(out_channels, c, 1, 1, generator=g) * (1.0 / c) ** 0.5
        sd[f"fpn.inner_blocks.{i}.0.bias"] = bias()
        sd[f"fpn.layer_blocks.{i}.0.weight"] = conv3()
        sd[f"fpn.layer_blocks.{i}.0.bias"] = bias()
    for name in ("p6", "p7"):
        sd[f"fpn.extra_blocks.{name}.weight"] = conv3()
        sd[f"fpn.extra_blocks.{name}.bias"] = bias()
    return sd, body


def p6p7_reference_forward(torch, sd, body, x):
    """fp64 CPU forward in eval mode: {"0", "1", "2", "p6", "p7"}, NHWC.  LastLevelP6P7 with in_channels ==
    out_channels takes P5: p6 = conv(P5, stride 2, padding 1), p7 = conv(relu(p6), stride 2, padding 1)."""
    F = torch.nn.functional
    _, stages = reference_forward(torch, body, x)
    c = [stages[f"layer{i}"].permute(0, 3, 1, 2) for i in RETURNED]
    d = {k: v.double() for k, v in sd.items() if k.startswith("fpn.")}
    inner = lambda i, t: F.conv2d(t, d[f"fpn.inner_blocks.{i}.0.weight"], d[f"fpn.inner_blocks.{i}.0.bias"])
    layer = lambda i, t: F.conv2d(t, d[f"fpn.layer_blocks.{i}.0.weight"], d[f"fpn.layer_blocks.{i}.0.bias"], padding=1)
    last_inner = inner(2, c[2])
    results = [None, None, layer(2, last_inner)]
    for i in (1, 0):
        lateral = inner(i, c[i])
        last_inner = lateral + F.interpolate(last_inner, size=lateral.shape[-2:], mode="nearest")
        results[i] = layer(i, last_inner)
    p6 = F.conv2d(results[2], d["fpn.extra_blocks.p6.weight"], d["fpn.extra_blocks.p6.bias"], stride=2, padding=1)
    p7 = F.conv2d(F.relu(p6), d["fpn.extra_blocks.p7.weight"], d["fpn.extra_blocks.p7.bias"], stride=2, padding=1)
    out = {str(i): t.permute(0, 2, 3, 1) for i, t in enumerate(results)}
    out.update(p6=p6.permute(0, 2, 3, 1), p7=p7.permute(0, 2, 3, 1))
    return out
