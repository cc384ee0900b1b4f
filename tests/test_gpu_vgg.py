"""Whole torchvision VGGs on the library (cuda_winograd_amd.vgg): random weights in torchvision's state-dict format,
built here (He-scaled convs, FCs scaled by 1/sqrt(fan_in), so activations stay O(1) through 16-19 layers without BN);
the five pooled maps and the logits against an fp64 CPU forward written here; a batch in which the plan queries send a
pooled layer to the throughput kernel with a stream-K tail; one whole forward captured in a torch.cuda.graph replays
bitwise equal to eager, and a second prepare at another shape follows it; no stream-K ticket left held.

The network runs on its own ping-pong tensors, not in the guarded arena (the per-layer tests of test_gpu_pool.py run
every form between guard bands); before every checked forward both activation tensors and the logits are filled with
NaN, so a ring, a pad channel or an output that a launch leaves unwritten poisons the stages behind it."""
import importlib

import pytest

import shape_sweeps as S

pytestmark = pytest.mark.gpu

NET_TOL = 1e-3   # the project's network bar (test_gpu_resnet.py)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch, torch.device("cuda:0")


@pytest.fixture(scope="module")
def V(pkg):
    return importlib.import_module("cuda_winograd_amd.vgg")


def random_state_dict(torch, V, arch, classes=1000, hidden=4096, seed=0):
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


def reference_forward(torch, V, sd, arch, x, eps=1e-5):
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


def _rel(torch, got, want):
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert not torch.isnan(got).any()
    return float((got - want).abs().max() / want.abs().max())


def _check_net(torch, V, model, sd, arch, x):
    shape = (int(x.shape[0]), int(x.shape[2]), int(x.shape[3]))
    if model._shape != shape:
        model.prepare(*shape)
    for t in (*model._act, model._logits, model._ws):
        t.fill_(float("nan"))
    logits, stages = model.forward(x, return_stages=True)
    torch.cuda.synchronize()
    want_logits, want = reference_forward(torch, V, sd, arch, x.cpu())
    assert sorted(stages) == sorted(want) == [f"pool{i}" for i in range(1, 6)]
    errs = {name: _rel(torch, stages[name], want[name]) for name in want}
    errs["logits"] = _rel(torch, logits, want_logits)
    print(f"{arch} N={x.shape[0]} {x.shape[2]}x{x.shape[3]}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    bad = {k: v for k, v in errs.items() if not v < NET_TOL}
    assert not bad, errs
    return logits.clone()


def _input(torch, dev, N, H, W):
    return (torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(N + H)) * 2 - 1).to(dev)


@pytest.mark.parametrize("arch", ["vgg16", "vgg16_bn"])
def test_vgg16_matches_fp64(arch, pkg, V, torch_dev):
    torch, dev = torch_dev
    sd = random_state_dict(torch, V, arch, seed=len(arch))
    model = pkg.VGG.from_state_dict(sd, arch)
    assert (model.classes, model.hidden) == (1000, 4096)
    _check_net(torch, V, model, sd, arch, _input(torch, dev, 2, 224, 224))
    assert pkg.tickets_in_use() == 0


@pytest.mark.parametrize("N,H,W", [(1, 97, 131), (3, 32, 32)])
@pytest.mark.parametrize("arch", ["vgg11", "vgg13_bn", "vgg19"])
def test_network_matches_fp64(arch, N, H, W, pkg, V, torch_dev):
    torch, dev = torch_dev
    sd = random_state_dict(torch, V, arch, classes=10, hidden=256, seed=len(arch) + N)
    model = pkg.VGG.from_state_dict(sd, arch)
    _check_net(torch, V, model, sd, arch, _input(torch, dev, N, H, W))
    assert pkg.tickets_in_use() == 0


def _pooled_forms(pkg, V, arch, N, H, W):
    """(form, detail) of every pooled layer, as the plan queries name them."""
    return [S.plan_3x3(pkg, N, h, w, max(cin, V.CPAD), cout) for cin, cout, h, w, pool in V.layer_shapes(arch, H, W)
            if pool]


def test_network_where_a_pooled_layer_runs_stream_k(pkg, V, torch_dev):
    """N = 32 at 96x96: the plan queries send at least one pooled layer to the throughput kernel with a stream-K
    tail, inside the network."""
    torch, dev = torch_dev
    arch, N, H, W = "vgg11", 32, 96, 96
    forms = _pooled_forms(pkg, V, arch, N, H, W)
    assert any(f == "throughput" and d["tail"] > 0 for f, d in forms), forms
    sd = random_state_dict(torch, V, arch, classes=10, hidden=256, seed=N)
    model = pkg.VGG.from_state_dict(sd, arch)
    _check_net(torch, V, model, sd, arch, _input(torch, dev, N, H, W))
    assert pkg.tickets_in_use() == 0


def test_whole_network_graph_replay_and_reprepare(pkg, V, torch_dev):
    torch, dev = torch_dev
    arch = "vgg13_bn"
    sd = random_state_dict(torch, V, arch, classes=10, hidden=256, seed=77)
    model = pkg.VGG.from_state_dict(sd, arch)
    N, H, W = 2, 128, 96
    x = _input(torch, dev, N, H, W)
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
    want, _ = reference_forward(torch, V, sd, arch, x.cpu())
    assert _rel(torch, eager, want) < NET_TOL
    # a second prepare at another shape, eager
    model.prepare(3, 75, 61)
    _check_net(torch, V, model, sd, arch, _input(torch, dev, 3, 75, 61))
    assert pkg.tickets_in_use() == 0
    with pytest.raises(pkg.WinoError, match="32"):
        model(_input(torch, dev, 1, 31, 40))
    del graph
