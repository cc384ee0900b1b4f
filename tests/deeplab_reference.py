"""Random weights in torchvision's deeplabv3_resnet* state-dict format and the fp64 CPU forward for the DeepLabV3 tests:
the dilated body of tests/segmentation_reference.py, then ASPP (rates 12, 24, 36), the 3x3 head and the bilinear resize
as torchvision's DeepLabHead composes them in eval mode (both dropouts are the identity)."""
from segmentation_reference import dilated_body_forward, fcn_random_state_dict

RATES = (12, 24, 36)


def deeplab_random_state_dict(torch, R, arch, classes=21, seed=0, aux=True):
    """torchvision-format deeplabv3_resnet* weights with O(1) activations; with `aux`, a few aux_classifier.* keys too
    (the loader ignores them)."""
    g = torch.Generator().manual_seed(seed + 2)
    sd = {k: v for k, v in fcn_random_state_dict(torch, R, arch, classes, seed, aux).items()
          if not k.startswith("classifier.")}

    def conv_bn(conv, bn, shape):
        sd[conv + ".weight"] = torch.randn(shape, generator=g) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
        sd[bn + ".weight"] = torch.rand(shape[0], generator=g) + 0.5
        sd[bn + ".bias"] = (torch.rand(shape[0], generator=g) - 0.5) * 0.2
        sd[bn + ".running_mean"] = (torch.rand(shape[0], generator=g) - 0.5) * 0.2
        sd[bn + ".running_var"] = torch.rand(shape[0], generator=g) + 0.5
        sd[bn + ".num_batches_tracked"] = torch.tensor(100)

    a = "classifier.0."
    conv_bn(a + "convs.0.0", a + "convs.0.1", (256, 2048, 1, 1))
    for i in (1, 2, 3):
        conv_bn(a + f"convs.{i}.0", a + f"convs.{i}.1", (256, 2048, 3, 3))
    conv_bn(a + "convs.4.1", a + "convs.4.2", (256, 2048, 1, 1))
    conv_bn(a + "project.0", a + "project.1", (256, 1280, 1, 1))
    conv_bn("classifier.1", "classifier.2", (256, 256, 3, 3))
    sd["classifier.4.weight"] = torch.randn(classes, 256, 1, 1, generator=g) * (1.0 / 256) ** 0.5
    sd["classifier.4.bias"] = torch.rand(classes, generator=g) - 0.5
    return sd


def deeplab_reference_forward(torch, sd, x, eps=1e-5):
    """fp64 CPU forward of torchvision's deeplabv3_resnet* in eval mode: [N][classes][H][W]."""
    F = torch.nn.functional
    d = {k: v.double() for k, v in sd.items()}

    def bn_relu(t, p):
        return torch.relu(F.batch_norm(t, d[p + ".running_mean"], d[p + ".running_var"], d[p + ".weight"],
                                       d[p + ".bias"], False, 0.0, eps))

    t = dilated_body_forward(torch, d, x, (False, True, True), eps, "backbone.")["layer4"]
    a = "classifier.0."
    branches = [bn_relu(F.conv2d(t, d[a + "convs.0.0.weight"]), a + "convs.0.1")]
    for i, r in zip((1, 2, 3), RATES):
        branches.append(bn_relu(F.conv2d(t, d[a + f"convs.{i}.0.weight"], padding=r, dilation=r), a + f"convs.{i}.1"))
    p = bn_relu(F.conv2d(F.adaptive_avg_pool2d(t, 1), d[a + "convs.4.1.weight"]), a + "convs.4.2")
    branches.append(F.interpolate(p, size=t.shape[-2:], mode="bilinear", align_corners=False))
    t = bn_relu(F.conv2d(torch.cat(branches, dim=1), d[a + "project.0.weight"]), a + "project.1")
    t = bn_relu(F.conv2d(t, d["classifier.1.weight"], padding=1), "classifier.2")
    t = F.conv2d(t, d["classifier.4.weight"], d["classifier.4.bias"])
    return F.interpolate(t, size=x.shape[-2:], mode="bilinear", align_corners=False)
