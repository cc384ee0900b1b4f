"""Random weights in torchvision's state-dict format and fp64 CPU forwards for the whole-network tests: the ResNet
family (ResNet, ResNeXt, Wide ResNet; the forward is read off the state dict alone) and VGG, each with the check that
runs a model and compares every stage and the logits with its reference at NET_TOL."""
from gpu_support import rel

NET_TOL = 1e-3   # the project's network bar


# ---- the ResNet family -----------------------------------------------------------------------------------------------
def random_state_dict(torch, R, arch, classes=1000, seed=0):
    """torchvision-format weights with O(1) activations: He-scaled convs (fan-in of the group), BN near identity, and a
    small gamma on each block's last BN so that the residual sums stay O(1) over many blocks."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    last = "bn3" if R.ARCHS[arch][0] else "bn2"
    for k, shape in R.expected_keys(arch, classes).items():
        if k.endswith(".weight") and len(shape) == 4:
            sd[k] = torch.randn(shape, generator=g) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
        elif k.endswith("running_mean"):
            sd[k] = (torch.rand(shape, generator=g) - 0.5) * 0.2
        elif k.endswith("running_var"):
            sd[k] = torch.rand(shape, generator=g) + 0.5
            sd[k[: -len("running_var")] + "num_batches_tracked"] = torch.tensor(100)
        elif k.endswith(".weight") and len(shape) == 1:
            sd[k] = (torch.rand(shape, generator=g) + 0.5) * (0.2 if k.split(".")[-2] == last and k.startswith("layer") else 1.0)
        elif k == "fc.weight":
            sd[k] = torch.randn(shape, generator=g) * (1.0 / shape[1]) ** 0.5
        elif k == "fc.bias":
            sd[k] = torch.rand(shape, generator=g) - 0.5
        else:
            sd[k] = (torch.rand(shape, generator=g) - 0.5) * 0.2
    return sd


def reference_forward(torch, sd, x, eps=1e-5):
    """fp64 CPU forward of a torchvision ResNet / ResNeXt / Wide ResNet in eval mode, read off the state dict alone:
    a block is a bottleneck when it has a conv3, its groups are conv2's out / in channel ratio, the stride sits on the
    3x3 (or, in a basic block, on conv1).  Returns (logits, {stage: NHWC})."""
    F = torch.nn.functional
    d = {k: v.double() for k, v in sd.items()}

    def bn(t, p):
        return F.batch_norm(t, d[p + ".running_mean"], d[p + ".running_var"], d[p + ".weight"], d[p + ".bias"],
                            False, 0.0, eps)

    t = F.max_pool2d(torch.relu(bn(F.conv2d(x.double(), d["conv1.weight"], stride=2, padding=3), "bn1")), 3, 2, 1)
    stages = {"stem": t.permute(0, 2, 3, 1)}
    for L in range(1, 5):
        b = 0
        while f"layer{L}.{b}.conv1.weight" in d:
            p = f"layer{L}.{b}"
            s = 2 if (b == 0 and L > 1) else 1
            if p + ".conv3.weight" in d:
                w2 = d[p + ".conv2.weight"]
                y = torch.relu(bn(F.conv2d(t, d[p + ".conv1.weight"]), p + ".bn1"))
                y = torch.relu(bn(F.conv2d(y, w2, stride=s, padding=1, groups=w2.shape[0] // w2.shape[1]), p + ".bn2"))
                y = bn(F.conv2d(y, d[p + ".conv3.weight"]), p + ".bn3")
            else:
                y = torch.relu(bn(F.conv2d(t, d[p + ".conv1.weight"], stride=s, padding=1), p + ".bn1"))
                y = bn(F.conv2d(y, d[p + ".conv2.weight"], padding=1), p + ".bn2")
            sc = t
            if p + ".downsample.0.weight" in d:
                sc = bn(F.conv2d(t, d[p + ".downsample.0.weight"], stride=s), p + ".downsample.1")
            t = torch.relu(y + sc)
            b += 1
        stages[f"layer{L}"] = t.permute(0, 2, 3, 1)
    return t.mean(dim=(2, 3)) @ d["fc.weight"].t() + d["fc.bias"], stages


def check_net(torch, model, sd, arch, x):
    logits, stages = model.forward(x, return_stages=True)
    torch.cuda.synchronize()
    want_logits, want = reference_forward(torch, sd, x.cpu())
    errs = {name: rel(torch, stages[name], want[name]) for name in want}
    errs["logits"] = rel(torch, logits, want_logits)
    print(f"{arch} N={x.shape[0]} {x.shape[2]}x{x.shape[3]}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    bad = {k: v for k, v in errs.items() if not v < NET_TOL}
    assert not bad, errs
    return logits.clone()


# ---- VGG ---------------------------------------------------------------------------------------------------------------
def vgg_random_state_dict(torch, V, arch, classes=1000, hidden=4096, seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in V.expected_keys(arch, classes, hidden).items():
        if k.endswith(".weight") and len(shape) == 4:
            sd[k] = torch.randn(shape, generator=g) * (2.0 / (shape[1] * 9)) ** 0.5
        elif k.endswith(".weight") and len(shape) == 2:
            sd[k] = torch.randn(shape, generator=g) * (1.0 / shape[1]) ** 0.5
        elif k.endswith("running_mean"):
            sd[k] = (torch.rand(shape, generator=g) - 0.5) * 0.2
        elif k.endswith("running_var"):
            sd[k] = torch.rand(shape, generator=g) + 0.5
            sd[k[: -len("running_var")] + "num_batches_tracked"] = torch.tensor(100)
        elif k.endswith(".weight"):
            sd[k] = torch.rand(shape, generator=g) + 0.5       # BN gamma
        else:
            sd[k] = (torch.rand(shape, generator=g) - 0.5) * 0.2
    return sd


def vgg_reference_forward(torch, V, sd, arch, x, eps=1e-5):
    """fp64 CPU forward of torchvision's VGG in eval mode: (logits, {"pool1".."pool5": NHWC})."""
    import torch.nn.functional as F
    d = {k: v.double() for k, v in sd.items()}
    bn = V.ARCHS[arch][1]
    t, stages = x.double(), {}
    for i, _, _, pool in V.conv_layers(arch):
        t = F.conv2d(t, d[f"features.{i}.weight"], d[f"features.{i}.bias"], padding=1)
        if bn:
            p = f"features.{i + 1}"
            t = F.batch_norm(t, d[p + ".running_mean"], d[p + ".running_var"], d[p + ".weight"], d[p + ".bias"],
                             False, 0.0, eps)
        t = torch.relu(t)
        if pool:
            t = F.max_pool2d(t, 2, 2)
            stages[f"pool{len(stages) + 1}"] = t.permute(0, 2, 3, 1)
    t = F.adaptive_avg_pool2d(t, (7, 7)).flatten(1)
    t = torch.relu(F.linear(t, d["classifier.0.weight"], d["classifier.0.bias"]))
    t = torch.relu(F.linear(t, d["classifier.3.weight"], d["classifier.3.bias"]))
    return F.linear(t, d["classifier.6.weight"], d["classifier.6.bias"]), stages


def check_vgg(torch, V, model, sd, arch, x):
    shape = (int(x.shape[0]), int(x.shape[2]), int(x.shape[3]))
    if model._shape != shape:
        model.prepare(*shape)
    for t in (*model._act, model._logits, model._ws):
        t.fill_(float("nan"))
    logits, stages = model.forward(x, return_stages=True)
    torch.cuda.synchronize()
    want_logits, want = vgg_reference_forward(torch, V, sd, arch, x.cpu())
    assert sorted(stages) == sorted(want) == [f"pool{i}" for i in range(1, 6)]
    errs = {name: rel(torch, stages[name], want[name]) for name in want}
    errs["logits"] = rel(torch, logits, want_logits)
    print(f"{arch} N={x.shape[0]} {x.shape[2]}x{x.shape[3]}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    bad = {k: v for k, v in errs.items() if not v < NET_TOL}
    assert not bad, errs
    return logits.clone()
