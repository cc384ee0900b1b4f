"""Whole torchvision VGGs on the library (cuda_winograd_amd.vgg): random weights in torchvision's state-dict format,
built here (He-scaled convs, FCs scaled by 1/sqrt(fan_in), so activations stay O(1) through 16-19 layers without BN);
the five pooled maps and the logits against an fp64 CPU forward written here; a batch in which the plan queries send a
pooled layer to the throughput kernel with a stream-K tail; one whole forward captured in a torch.cuda.graph replays
bitwise equal to eager, and a second prepare at another shape follows it; no stream-K ticket left held.

The network runs on its own ping-pong tensors, not in the guarded arena (the per-layer tests of test_gpu_pool.py run
every form between guard bands); before every checked forward both activation tensors and the logits are filled with
NaN, so a ring, a pad channel or an output that a launch leaves unwritten poisons the stages behind it."""
import pytest

import shape_sweeps as S
from gpu_support import V, network_graph_scenario, rel, torch_dev  # noqa: F401
from reference_nets import NET_TOL, check_vgg, vgg_random_state_dict, vgg_reference_forward

pytestmark = pytest.mark.gpu


def _input(torch, dev, N, H, W):
    return (torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(N + H)) * 2 - 1).to(dev)


@pytest.mark.parametrize("arch", ["vgg16", "vgg16_bn"])
def test_vgg16_matches_fp64(arch, pkg, V, torch_dev):
    torch, dev = torch_dev
    sd = vgg_random_state_dict(torch, V, arch, seed=len(arch))
    model = pkg.VGG.from_state_dict(sd, arch)
    assert (model.classes, model.hidden) == (1000, 4096)
    check_vgg(torch, V, model, sd, arch, _input(torch, dev, 2, 224, 224))
    assert pkg.tickets_in_use() == 0


@pytest.mark.parametrize("N,H,W", [(1, 97, 131), (3, 32, 32)])
@pytest.mark.parametrize("arch", ["vgg11", "vgg13_bn", "vgg19"])
def test_network_matches_fp64(arch, N, H, W, pkg, V, torch_dev):
    torch, dev = torch_dev
    sd = vgg_random_state_dict(torch, V, arch, classes=10, hidden=256, seed=len(arch) + N)
    model = pkg.VGG.from_state_dict(sd, arch)
    check_vgg(torch, V, model, sd, arch, _input(torch, dev, N, H, W))
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
    sd = vgg_random_state_dict(torch, V, arch, classes=10, hidden=256, seed=N)
    model = pkg.VGG.from_state_dict(sd, arch)
    check_vgg(torch, V, model, sd, arch, _input(torch, dev, N, H, W))
    assert pkg.tickets_in_use() == 0


def test_whole_network_graph_replay_and_reprepare(pkg, V, torch_dev):
    torch, dev = torch_dev
    arch = "vgg13_bn"
    sd = vgg_random_state_dict(torch, V, arch, classes=10, hidden=256, seed=77)
    model = pkg.VGG.from_state_dict(sd, arch)
    N, H, W = 2, 128, 96
    x = _input(torch, dev, N, H, W)
    eager, graph = network_graph_scenario(pkg, torch, model, x)
    want, _ = vgg_reference_forward(torch, V, sd, arch, x.cpu())
    assert rel(torch, eager, want) < NET_TOL
    # a second prepare at another shape, eager
    model.prepare(3, 75, 61)
    check_vgg(torch, V, model, sd, arch, _input(torch, dev, 3, 75, 61))
    assert pkg.tickets_in_use() == 0
    with pytest.raises(pkg.WinoError, match="32"):
        model(_input(torch, dev, 1, 31, 40))
    del graph
