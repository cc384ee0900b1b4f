"""GPU tests of DeepLabV3-ResNet50 (cuda_winograd_amd.segmentation.DeepLabV3) end to end, against the fp64 CPU forward
of tests/deeplab_reference.py driven by a random state dict, at the project's network bar; eager against one-graph
replay."""
import pytest

from deeplab_reference import deeplab_random_state_dict, deeplab_reference_forward
from gpu_support import R, rel, torch_dev  # noqa: F401
from reference_nets import NET_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def deeplab(pkg, R, torch_dev):
    """One DeepLabV3-ResNet50 and its state dict for the module (21 classes: the columns are padded to 64)."""
    torch, dev = torch_dev
    sd = deeplab_random_state_dict(torch, R, "resnet50", classes=21, seed=4)
    return pkg.DeepLabV3.from_state_dict(sd, "resnet50"), sd


@pytest.mark.parametrize("N,H,W", [(1, 65, 65), (2, 49, 81)])   # 9x9 maps; 7x11 maps: every rate overreaches them
def test_deeplabv3_resnet50(N, H, W, deeplab, pkg, torch_dev):
    torch, dev = torch_dev
    model, sd = deeplab
    x = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(N + H)) - 0.5
    out = model(x.to(dev))
    torch.cuda.synchronize()
    assert sorted(out) == ["out"] and tuple(out["out"].shape) == (N, 21, H, W)
    assert model._shape == (N, H, W)                       # (a new input shape re-prepared)
    err = rel(torch, out["out"], deeplab_reference_forward(torch, sd, x))
    print(f"deeplabv3_resnet50 N={N} {H}x{W}: out {err:.2e}")
    assert err < NET_TOL
    assert pkg.tickets_in_use() == 0


def test_deeplabv3_replays_from_one_graph(deeplab, pkg, torch_dev):
    torch, dev = torch_dev
    model, sd = deeplab
    x = (torch.rand(1, 3, 65, 65, generator=torch.Generator().manual_seed(9)) - 0.5).to(dev)
    sg = torch.cuda.Stream()
    with torch.cuda.stream(sg):
        model.prepare(1, 65, 65)
        eager = model(x)["out"].clone()
    sg.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=sg):
        out = model(x)["out"]
    for _ in range(2):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    with torch.cuda.stream(sg):
        assert pkg.tickets_in_use() == 0
    del graph
    # a new input shape re-prepares and still matches the reference
    x2 = torch.rand(1, 3, 33, 49, generator=torch.Generator().manual_seed(10)) - 0.5
    got = model(x2.to(dev))["out"]
    assert model._shape == (1, 33, 49)
    assert rel(torch, got, deeplab_reference_forward(torch, sd, x2)) < NET_TOL
    assert pkg.tickets_in_use() == 0
