"""Whole torchvision ResNets on the library (cuda_winograd_amd.resnet): random weights in torchvision's state-dict
format, built here; the stem, every stage and the logits against an fp64 CPU forward written here (F.conv2d,
eval-mode BN); one whole forward captured in a torch.cuda.graph replays bitwise equal to eager; a second prepare at
another input shape; inputs whose last stages are 1x1, a batch where the throughput and stream-K forms take over
inside the network, and ResNet-152; no stream-K ticket left held."""
import pytest

from gpu_support import R, network_graph_scenario, rel, torch_dev  # noqa: F401
from reference_nets import NET_TOL, check_net, random_state_dict, reference_forward

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("arch,N,H,W", [("resnet18", 2, 224, 224), ("resnet50", 2, 224, 224),
                                        ("resnet34", 1, 97, 131), ("resnet101", 1, 97, 131)])
def test_network_matches_fp64(arch, N, H, W, pkg, R, torch_dev):
    torch, dev = torch_dev
    sd = random_state_dict(torch, R, arch, seed=len(arch) + N)
    model = pkg.ResNet.from_state_dict(sd, arch)
    x = (torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(N + H)) * 2 - 1).to(dev)
    check_net(torch, model, sd, arch, x)
    assert pkg.tickets_in_use() == 0


@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_whole_network_graph_replay_and_reprepare(arch, pkg, R, torch_dev):
    torch, dev = torch_dev
    sd = random_state_dict(torch, R, arch, classes=10, seed=77)
    model = pkg.ResNet.from_state_dict(sd, arch)
    x = (torch.rand(2, 3, 128, 96, generator=torch.Generator().manual_seed(5)) * 2 - 1).to(dev)
    eager, graph = network_graph_scenario(pkg, torch, model, x)
    want, _ = reference_forward(torch, sd, x.cpu())
    assert rel(torch, eager, want) < NET_TOL
    # a second prepare at another shape, eager
    x2 = (torch.rand(3, 3, 75, 61, generator=torch.Generator().manual_seed(6)) * 2 - 1).to(dev)
    model.prepare(3, 75, 61)
    check_net(torch, model, sd, arch, x2)
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
    check_net(torch, model, sd, arch, x)
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
    check_net(torch, model, sd, arch, x)
    assert pkg.tickets_in_use() == 0


def test_resnet152_forward(pkg, R, torch_dev):
    torch, dev = torch_dev
    sd = random_state_dict(torch, R, "resnet152", seed=152)
    model = pkg.ResNet.from_state_dict(sd, "resnet152")
    x = (torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(152)) * 2 - 1).to(dev)
    check_net(torch, model, sd, "resnet152", x)
    assert pkg.tickets_in_use() == 0
