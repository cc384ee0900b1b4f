"""Random weights in torchvision's fcn_resnet* state-dict format and fp64 CPU forwards for the segmentation tests: the
ResNet body with replace_stride_with_dilation (read off the state dict and the three flags alone, torchvision's
_make_layer rule) and the FCN head with the bilinear resize."""
from reference_nets import random_state_dict


def dilated_body_forward(torch, d, x, dilate, eps=1e-5, prefix=""):
    """fp64 CPU forward of a torchvision bottleneck ResNet body in eval mode with replace_stride_with_dilation =
    `dilate`; d: the state dict in float64.  Returns {stage: NCHW}."""
    F = torch.nn.functional

    def bn(t, p):
        p = prefix + p
        return F.batch_norm(t, d[p + ".running_mean"], d[p + ".running_var"], d[p + ".weight"], d[p + ".bias"],
                            False, 0.0, eps)

    w = lambda k: d[prefix + k]
    t = F.max_pool2d(torch.relu(bn(F.conv2d(x.double(), w("conv1.weight"), stride=2, padding=3), "bn1")), 3, 2, 1)
    stages = {"stem": t}
    dil = 1
    for L in range(1, 5):
        prev, stride = dil, (2 if L > 1 else 1)
        if L > 1 and dilate[L - 2]:
            dil *= stride
            stride = 1
        b = 0
        while prefix + f"layer{L}.{b}.conv1.weight" in d:
            p = f"layer{L}.{b}"
            s, dd = (stride, prev) if b == 0 else (1, dil)
            y = torch.relu(bn(F.conv2d(t, w(p + ".conv1.weight")), p + ".bn1"))
            y = torch.relu(bn(F.conv2d(y, w(p + ".conv2.weight"), stride=s, padding=dd, dilation=dd), p + ".bn2"))
            y = bn(F.conv2d(y, w(p + ".conv3.weight")), p + ".bn3")
            sc = t
            if prefix + p + ".downsample.0.weight" in d:
                sc = bn(F.conv2d(t, w(p + ".downsample.0.weight"), stride=s), p + ".downsample.1")
            t = torch.relu(y + sc)
            b += 1
        stages[f"layer{L}"] = t
    return stages


def fcn_random_state_dict(torch, R, arch, classes=21, seed=0, aux=True):
    """torchvision-format fcn_resnet* weights with O(1) activations; with `aux`, a few aux_classifier.* keys too (the
    loader ignores them)."""
    g = torch.Generator().manual_seed(seed + 1)
    body = random_state_dict(torch, R, arch, classes=1000, seed=seed)
    sd = {"backbone." + k: v for k, v in body.items() if not k.startswith("fc.")}
    sd["classifier.0.weight"] = torch.randn(512, 2048, 3, 3, generator=g) * (2.0 / (2048 * 9)) ** 0.5
    sd["classifier.1.weight"] = torch.rand(512, generator=g) + 0.5
    sd["classifier.1.bias"] = (torch.rand(512, generator=g) - 0.5) * 0.2
    sd["classifier.1.running_mean"] = (torch.rand(512, generator=g) - 0.5) * 0.2
    sd["classifier.1.running_var"] = torch.rand(512, generator=g) + 0.5
    sd["classifier.1.num_batches_tracked"] = torch.tensor(100)
    sd["classifier.4.weight"] = torch.randn(classes, 512, 1, 1, generator=g) * (1.0 / 512) ** 0.5
    sd["classifier.4.bias"] = torch.rand(classes, generator=g) - 0.5
    if aux:
        sd["aux_classifier.0.weight"] = torch.randn(256, 1024, 3, 3, generator=g) * 0.01
        sd["aux_classifier.4.bias"] = torch.rand(classes, generator=g)
    return sd


def fcn_reference_forward(torch, sd, x, eps=1e-5):
    """fp64 CPU forward of torchvision's fcn_resnet* in eval mode: [N][classes][H][W]."""
    F = torch.nn.functional
    d = {k: v.double() for k, v in sd.items()}
    t = dilated_body_forward(torch, d, x, (False, True, True), eps, "backbone.")["layer4"]
    p = "classifier.1"
    t = F.conv2d(t, d["classifier.0.weight"], padding=1)
    t = torch.relu(F.batch_norm(t, d[p + ".running_mean"], d[p + ".running_var"], d[p + ".weight"], d[p + ".bias"],
                                False, 0.0, eps))
    t = F.conv2d(t, d["classifier.4.weight"], d["classifier.4.bias"])
    return F.interpolate(t, size=x.shape[-2:], mode="bilinear", align_corners=False)
