"""Whole torchvision ResNets on the library (cuda_winograd_amd.resnet): random weights in torchvision's state-dict
format, built here; the stem, every stage and the logits against an fp64 CPU forward written here (F.conv2d,
eval-mode BN); one whole forward captured in a torch.cuda.graph replays bitwise equal to eager; a second prepare at
another input shape; inputs whose last stages are 1x1, a batch where the throughput and stream-K forms take over
inside the network, and ResNet-152; no stream-K ticket left held."""
import pytest

pytestmark = pytest.mark.gpu

NET_TOL = 1e-3


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch, torch.device("cuda:0")


@pytest.fixture(scope="module")
def R(pkg):
    import importlib
    return importlib.import_module("cuda_winograd_amd.resnet")


def random_state_dict(torch, R, arch, classes=1000, seed=0):
    """torchvision-format weights with O(1) activations: He-scaled convs, BN near identity, and a small gamma on each
    block's last BN so that the residual sums stay O(1) over 100+ blocks."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    last_bn = {f"layer{L}.{b}.bn{3 if ARCH_BOTTLENECK[arch] else 2}" for L in range(1, 5) for b in range(64)}
    for k, shape in R.expected_keys(arch, classes).items():
        if k.endswith(".weight") and len(shape) == 4:
            fan_in = shape[1] * shape[2] * shape[3]
            sd[k] = torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5
        elif k.endswith("running_mean"):
            sd[k] = (torch.rand(shape, generator=g) - 0.5) * 0.2
        elif k.endswith("running_var"):
            sd[k] = torch.rand(shape, generator=g) + 0.5
        elif k.endswith(".weight") and len(shape) == 1:
            gamma = torch.rand(shape, generator=g) + 0.5
            sd[k] = gamma * (0.2 if k[: -len(".weight")] in last_bn else 1.0)
        elif k.endswith(".bias") and not k.startswith("fc"):
            sd[k] = (torch.rand(shape, generator=g) - 0.5) * 0.2
        elif k == "fc.weight":
            sd[k] = torch.randn(shape, generator=g) * (1.0 / shape[1]) ** 0.5
        else:
            sd[k] = torch.rand(shape, generator=g) - 0.5
        if k.endswith("running_var"):
            sd[k[: -len("running_var")] + "num_batches_tracked"] = torch.tensor(100)
    return sd


ARCH_BOTTLENECK = {"resnet18": False, "resnet34": False, "resnet50": True, "resnet101": True, "resnet152": True}


def reference_forward(torch, R, sd, arch, x, eps=1e-5):
    """fp64 CPU forward of torchvision's ResNet (v1.5 placement) in eval mode: (logits, {stage: NHWC})."""
    import torch.nn.functional as F
    d = {k: v.double() for k, v in sd.items()}

    def bn(t, p):
        return F.batch_norm(t, d[p + ".running_mean"], d[p + ".running_var"], d[p + ".weight"], d[p + ".bias"],
                            False, 0.0, eps)

    bottleneck, blocks = R.ARCHS[arch]
    t = F.max_pool2d(torch.relu(bn(F.conv2d(x.double(), d["conv1.weight"], stride=2, padding=3), "bn1")), 3, 2, 1)
    stages = {"stem": t.permute(0, 2, 3, 1)}
    for L, nb in enumerate(blocks, 1):
        for b in range(nb):
            p = f"layer{L}.{b}"
            s = 2 if (b == 0 and L > 1) else 1
            if bottleneck:
                y = torch.relu(bn(F.conv2d(t, d[p + ".conv1.weight"]), p + ".bn1"))
                y = torch.relu(bn(F.conv2d(y, d[p + ".conv2.weight"], stride=s, padding=1), p + ".bn2"))
                y = bn(F.conv2d(y, d[p + ".conv3.weight"]), p + ".bn3")
            else:
                y = torch.relu(bn(F.conv2d(t, d[p + ".conv1.weight"], stride=s, padding=1), p + ".bn1"))
                y = bn(F.conv2d(y, d[p + ".conv2.weight"], padding=1), p + ".bn2")
            sc = t
            if p + ".downsample.0.weight" in d:
                sc = bn(F.conv2d(t, d[p + ".downsample.0.weight"], stride=s), p + ".downsample.1")
            t = torch.relu(y + sc)
        stages[f"layer{L}"] = t.permute(0, 2, 3, 1)
    logits = t.mean(dim=(2, 3)) @ d["fc.weight"].t() + d["fc.bias"]
    return logits, stages


def _rel(torch, got, want):
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert not torch.isnan(got).any()
    return float((got - want).abs().max() / want.abs().max())


def _check_net(torch, R, model, sd, arch, x):
    logits, stages = model.forward(x, return_stages=True)
    torch.cuda.synchronize()
    want_logits, want = reference_forward(torch, R, sd, arch, x.cpu())
    errs = {name: _rel(torch, stages[name], want[name]) for name in want}
    errs["logits"] = _rel(torch, logits, want_logits)
    print(f"{arch} N={x.shape[0]} {x.shape[2]}x{x.shape[3]}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    bad = {k: v for k, v in errs.items() if not v < NET_TOL}
    assert not bad, errs
    return logits.clone()


@pytest.mark.parametrize("arch,N,H,W", [("resnet18", 2, 224, 224), ("resnet50", 2, 224, 224),
                                        ("resnet34", 1, 97, 131), ("resnet101", 1, 97, 131)])
def test_network_matches_fp64(arch, N, H, W, pkg, R, torch_dev):
    torch, dev = torch_dev
    sd = random_state_dict(torch, R, arch, seed=len(arch) + N)
    model = pkg.ResNet.from_state_dict(sd, arch)
    x = (torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(N + H)) * 2 - 1).to(dev)
    _check_net(torch, R, model, sd, arch, x)
    assert pkg.tickets_in_use() == 0


@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_whole_network_graph_replay_and_reprepare(arch, pkg, R, torch_dev):
    torch, dev = torch_dev
    sd = random_state_dict(torch, R, arch, classes=10, seed=77)
    model = pkg.ResNet.from_state_dict(sd, arch)
    N, H, W = 2, 128, 96
    x = (torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(5)) * 2 - 1).to(dev)
    sg = torch.cuda.Stream()
    with torch.cuda.stream(sg):
        model.prepare(N, H, W)
        eager = model(x).clone()
    sg.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=sg):
        out = model(x)
    for _ in range(2):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    with torch.cuda.stream(sg):
        assert pkg.tickets_in_use() == 0
    want, _ = reference_forward(torch, R, sd, arch, x.cpu())
    assert _rel(torch, eager, want) < NET_TOL
    # a second prepare at another shape, eager
    x2 = (torch.rand(3, 3, 75, 61, generator=torch.Generator().manual_seed(6)) * 2 - 1).to(dev)
    model.prepare(3, 75, 61)
    _check_net(torch, R, model, sd, arch, x2)
    assert pkg.tickets_in_use() == 0
    del graph


@pytest.mark.parametrize("arch,H", [("resnet18", 32), ("resnet50", 32), ("resnet18", 8), ("resnet50", 8)])
def test_network_at_small_maps(arch, H, pkg, R, torch_dev):
    """Inputs whose last stages shrink to one pixel: 32x32 (layer1..layer4 maps 8/4/2/1) and 8x8 (2/1/1/1)."""
    torch, dev = torch_dev
    maps = {32: [8, 4, 2, 1], 8: [2, 1, 1, 1]}[H]
    assert [h for name, _, h, w in R.stage_shapes(arch, H, H) if name != "stem"] == maps
    sd = random_state_dict(torch, R, arch, seed=H + len(arch))
    model = pkg.ResNet.from_state_dict(sd, arch)
    x = (torch.rand(3, 3, H, H, generator=torch.Generator().manual_seed(H)) * 2 - 1).to(dev)
    _check_net(torch, R, model, sd, arch, x)
    assert pkg.tickets_in_use() == 0


def _layer_forms(pkg, R, arch, N, H, W):
    """{'3x3': the forms of the network's Winograd 3x3 layers, '1x1': those of its 1x1-kernel launches (the 1x1s, the
    stride-2 3x3s and the head's GEMM)}, as the plan queries name them."""
    import shape_sweeps as S
    bottleneck, blocks = R.ARCHS[arch]
    names = {pkg.FORM_TILED: "tiled", pkg.FORM_STREAM_K: "stream_k", pkg.FORM_LATENCY: "latency"}
    f3, f1 = set(), set()
    h, w = pkg.stem_out_hw(H, W)
    cin = 64
    for i, planes in enumerate(R.PLANES):
        c4 = planes * 4 if bottleneck else planes
        if bottleneck:
            if i == 0:
                f1.update(names[f] for f in pkg.proj_tail_plan(N, h, w, cin, planes, c4, 1))
            else:
                f1.add(S.form_1x1(pkg, N * h * w, cin, planes))
                f1.add(names[pkg.conv3x3_s2_plan(N, h, w, planes, planes)])
                f1.add(names[pkg.proj_tail_plan(N, h, w, cin, planes, c4, 2)[1]])
                h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            if blocks[i] > 1:
                f1.add(S.form_1x1(pkg, N * h * w, c4, planes))
                f1.add(S.form_1x1(pkg, N * h * w, planes, c4))
        elif i:
            f1.add(names[pkg.conv3x3_s2_plan(N, h, w, cin, planes)])
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        f3.add(S.plan_3x3(pkg, N, h, w, planes, planes)[0])
        cin = c4
    f1.add(S.form_1x1(pkg, N, cin, S.head_cols(1000)))
    return {"3x3": f3, "1x1": f1}


@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_network_where_the_throughput_forms_take_over(arch, pkg, R, torch_dev):
    """N = 32 at 96x96: the plan queries send at least one 3x3 layer to the throughput kernel and at least one
    1x1-kernel launch to stream-K, inside the network."""
    torch, dev = torch_dev
    N, H, W = 32, 96, 96
    forms = _layer_forms(pkg, R, arch, N, H, W)
    assert "throughput" in forms["3x3"] and "stream_k" in forms["1x1"], forms
    sd = random_state_dict(torch, R, arch, seed=N + len(arch))
    model = pkg.ResNet.from_state_dict(sd, arch)
    x = (torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(N)) * 2 - 1).to(dev)
    _check_net(torch, R, model, sd, arch, x)
    assert pkg.tickets_in_use() == 0


def test_resnet152_forward(pkg, R, torch_dev):
    torch, dev = torch_dev
    sd = random_state_dict(torch, R, "resnet152", seed=152)
    model = pkg.ResNet.from_state_dict(sd, "resnet152")
    x = (torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(152)) * 2 - 1).to(dev)
    _check_net(torch, R, model, sd, "resnet152", x)
    assert pkg.tickets_in_use() == 0
