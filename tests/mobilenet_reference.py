"""Random weights in torchvision's mobilenet_v2 state-dict format and the fp64 CPU forward with the five stride-level
maps, for tests/test_gpu_mobilenet.py.  `M` is cuda_winograd_amd.mobilenet (its block table and key list)."""


def random_state_dict(torch, M, width_mult=1.0, classes=10, seed=0):
    """He-scaled convolutions (fan-in of the group), BN near identity: activations stay O(1) through 52 layers."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in M.expected_keys(width_mult, classes).items():
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


def reference_forward(torch, M, sd, width_mult, x, eps=1e-5):
    """fp64 CPU forward of torchvision's mobilenet_v2 in eval mode: (logits, {"stride2".."stride32": NHWC})."""
    F = torch.nn.functional
    d = {k: v.double() for k, v in sd.items()}

    def cbr(t, conv, bn, act=True, **kw):
        t = F.batch_norm(F.conv2d(t, d[conv + ".weight"], **kw), d[bn + ".running_mean"], d[bn + ".running_var"],
                         d[bn + ".weight"], d[bn + ".bias"], False, 0.0, eps)
        return F.relu6(t) if act else t

    t, stages, level = cbr(x.double(), "features.0.0", "features.0.1", stride=2, padding=1), {}, 0
    for i, cin, hid, cout, s, e in M.blocks(width_mult)[1]:
        p, j, y = f"features.{i}.conv", 0, t
        if e != 1:
            y, j = cbr(y, f"{p}.0.0", f"{p}.0.1"), 1
        y = cbr(y, f"{p}.{j}.0", f"{p}.{j}.1", stride=s, padding=1, groups=hid)
        y = cbr(y, f"{p}.{j + 1}", f"{p}.{j + 2}", act=False)
        t = t + y if s == 1 and cin == cout else y
        level += s == 2
        stages[M.STAGES[level]] = t.permute(0, 2, 3, 1)
    t = cbr(t, "features.18.0", "features.18.1")
    return t.mean(dim=(2, 3)) @ d["classifier.1.weight"].t() + d["classifier.1.bias"], stages
