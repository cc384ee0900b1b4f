"""Random weights in torchvision's mobilenet_v3 state-dict format and the fp64 CPU forward with the five stride-level
maps, for tests/test_gpu_mobilenet_v3.py.  `M` is cuda_winograd_amd.mobilenet_v3 (its block tables and key list)."""


def random_state_dict(torch, M, arch="large", classes=10, seed=0):
    """He-scaled convolutions (fan-in of the group), BN near identity, small biases: activations stay O(1)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in M.expected_keys(arch, classes).items():
        if k.endswith(".weight") and len(shape) == 4:
            sd[k] = torch.randn(shape, generator=g) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
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


def reference_forward(torch, M, sd, arch, x, eps=1e-3):
    """fp64 CPU forward of torchvision's mobilenet_v3_{arch} in eval mode: (logits, {"stride2".."stride32": NHWC})."""
    F = torch.nn.functional
    d = {k: v.double() for k, v in sd.items()}
    acts = {"RE": F.relu, "HS": F.hardswish, None: lambda t: t}

    def cba(t, p, act, **kw):
        t = F.batch_norm(F.conv2d(t, d[p + ".0.weight"], **kw), d[p + ".1.running_mean"], d[p + ".1.running_var"],
                         d[p + ".1.weight"], d[p + ".1.bias"], False, 0.0, eps)
        return acts[act](t)

    t = cba(x.double(), "features.0", "HS", stride=2, padding=1)
    stages, level = {M.STAGES[0]: t.permute(0, 2, 3, 1)}, 0
    rows = M.BLOCKS[arch]
    for i, (cin, k, hid, cout, se, act, s) in enumerate(rows, 1):
        p, j, y = f"features.{i}.block", 0, t
        if hid != cin:
            y, j = cba(y, f"{p}.0", act), 1
        y = cba(y, f"{p}.{j}", act, stride=s, padding=k // 2, groups=hid)
        j += 1
        if se:
            q = F.relu(F.conv2d(y.mean(dim=(2, 3), keepdim=True), d[f"{p}.{j}.fc1.weight"], d[f"{p}.{j}.fc1.bias"]))
            y = y * F.hardsigmoid(F.conv2d(q, d[f"{p}.{j}.fc2.weight"], d[f"{p}.{j}.fc2.bias"]))
            j += 1
        y = cba(y, f"{p}.{j}", None)
        t = t + y if s == 1 and cin == cout else y
        level += s == 2
        stages[M.STAGES[level]] = t.permute(0, 2, 3, 1)
    t = cba(t, f"features.{len(rows) + 1}", "HS").mean(dim=(2, 3))
    t = F.hardswish(t @ d["classifier.0.weight"].t() + d["classifier.0.bias"])
    return t @ d["classifier.3.weight"].t() + d["classifier.3.bias"], stages
