"""Random torchvision-format state dicts with a complete aux_classifier (FCNHead(1024, classes)) and the fp64 CPU
forward that returns both heads, for the tests of the segmentation networks' output options: the dilated body once, the
main head of tests/segmentation_reference.py or tests/deeplab_reference.py, the aux head on layer3's output, and the
bilinear resize of each."""
from deeplab_reference import RATES, deeplab_random_state_dict
from segmentation_reference import dilated_body_forward, fcn_random_state_dict


def _aux_keys(torch, classes, seed):
    g = torch.Generator().manual_seed(seed + 3)
    sd = {"aux_classifier.0.weight": torch.randn(256, 1024, 3, 3, generator=g) * (2.0 / (1024 * 9)) ** 0.5,
          "aux_classifier.1.weight": torch.rand(256, generator=g) + 0.5,
          "aux_classifier.1.bias": (torch.rand(256, generator=g) - 0.5) * 0.2,
          "aux_classifier.1.running_mean": (torch.rand(256, generator=g) - 0.5) * 0.2,
          "aux_classifier.1.running_var": torch.rand(256, generator=g) + 0.5,
          "aux_classifier.1.num_batches_tracked": torch.tensor(100),
          "aux_classifier.4.weight": torch.randn(classes, 256, 1, 1, generator=g) * (1.0 / 256) ** 0.5,
          "aux_classifier.4.bias": torch.rand(classes, generator=g) - 0.5}
    return sd


def aux_state_dict(torch, R, net, arch, classes=21, seed=0):
    """`net`: "fcn" or "deeplabv3"."""
    make = fcn_random_state_dict if net == "fcn" else deeplab_random_state_dict
    sd = make(torch, R, arch, classes, seed, aux=False)
    sd.update(_aux_keys(torch, classes, seed))
    return sd


def reference_outputs(torch, net, sd, x, eps=1e-5):
    """fp64 CPU forward of torchvision's fcn_resnet* / deeplabv3_resnet* in eval mode: {"out", "aux"}, each
    [N][classes][H][W]."""
    F = torch.nn.functional
    d = {k: v.double() for k, v in sd.items()}

    def bn_relu(t, p):
        return torch.relu(F.batch_norm(t, d[p + ".running_mean"], d[p + ".running_var"], d[p + ".weight"],
                                       d[p + ".bias"], False, 0.0, eps))

    up = lambda t: F.interpolate(t, size=x.shape[-2:], mode="bilinear", align_corners=False)
    stages = dilated_body_forward(torch, d, x, (False, True, True), eps, "backbone.")
    t = stages["layer4"]
    if net == "fcn":
        t = bn_relu(F.conv2d(t, d["classifier.0.weight"], padding=1), "classifier.1")
    else:
        a = "classifier.0."
        branches = [bn_relu(F.conv2d(t, d[a + "convs.0.0.weight"]), a + "convs.0.1")]
        for i, r in zip((1, 2, 3), RATES):
            branches.append(bn_relu(F.conv2d(t, d[a + f"convs.{i}.0.weight"], padding=r, dilation=r), a + f"convs.{i}.1"))
        p = bn_relu(F.conv2d(F.adaptive_avg_pool2d(t, 1), d[a + "convs.4.1.weight"]), a + "convs.4.2")
        branches.append(F.interpolate(p, size=t.shape[-2:], mode="bilinear", align_corners=False))
        t = bn_relu(F.conv2d(torch.cat(branches, dim=1), d[a + "project.0.weight"]), a + "project.1")
        t = bn_relu(F.conv2d(t, d["classifier.1.weight"], padding=1), "classifier.2")
    out = up(F.conv2d(t, d["classifier.4.weight"], d["classifier.4.bias"]))
    t = bn_relu(F.conv2d(stages["layer3"], d["aux_classifier.0.weight"], padding=1), "aux_classifier.1")
    aux = up(F.conv2d(t, d["aux_classifier.4.weight"], d["aux_classifier.4.bias"]))
    return {"out": out, "aux": aux}
