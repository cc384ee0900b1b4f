"""GPU tests of the segmentation networks: a ResNet-50 body with replace_stride_with_dilation on its stage outputs, and
the FCN-ResNet50 (cuda_winograd_amd.segmentation.FCN) end to end, against the fp64 CPU forwards of
tests/segmentation_reference.py driven by a random state dict, at the project's network bar; eager against one-graph
replay."""
import importlib

import pytest

from gpu_support import R, rel, torch_dev  # noqa: F401
from reference_nets import NET_TOL, random_state_dict
from segmentation_reference import dilated_body_forward, fcn_random_state_dict, fcn_reference_forward

pytestmark = pytest.mark.gpu
DILATE = (False, True, True)


@pytest.fixture(scope="module")
def fcn(pkg, R, torch_dev):
    """One FCN-ResNet50 and its state dict for the module (21 classes: the columns are padded to 64)."""
    torch, dev = torch_dev
    sd = fcn_random_state_dict(torch, R, "resnet50", classes=21, seed=3)
    return pkg.FCN.from_state_dict(sd, "resnet50"), sd


def test_dilated_resnet50_stage_outputs(pkg, R, torch_dev):
    torch, dev = torch_dev
    sd = random_state_dict(torch, R, "resnet50", classes=64, seed=1)
    model = R.ResNet.from_state_dict(sd, "resnet50", replace_stride_with_dilation=DILATE)
    kinds = [[k for k, *_ in st] for st in model.layers]
    assert kinds[2] == ["proj"] + ["dilated_residual"] * 5 and kinds[3] == ["dilated_proj"] + ["dilated_residual"] * 2
    x = torch.rand(2, 3, 65, 65, generator=torch.Generator().manual_seed(2)) - 0.5
    logits, stages = model.forward(x.to(dev), return_stages=True)
    torch.cuda.synchronize()
    want = dilated_body_forward(torch, {k: v.double() for k, v in sd.items()}, x, DILATE)
    assert tuple(stages["layer4"].shape) == (2, 9, 9, 2048) == tuple(stages["layer2"].shape[:3]) + (2048,)
    errs = {n: rel(torch, stages[n], want[n].permute(0, 2, 3, 1)) for n in want}
    d = {k: v.double() for k, v in sd.items()}
    errs["logits"] = rel(torch, logits, want["layer4"].mean(dim=(2, 3)) @ d["fc.weight"].t() + d["fc.bias"])
    print("dilated resnet50: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < NET_TOL for v in errs.values()), errs
    assert pkg.tickets_in_use() == 0


@pytest.mark.parametrize("N,H,W", [(1, 65, 65), (2, 49, 81)])   # 9x9 maps; 7x11 maps, which dilation 4 overreaches
def test_fcn_resnet50(N, H, W, fcn, pkg, torch_dev):
    torch, dev = torch_dev
    model, sd = fcn
    x = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(N + H)) - 0.5
    out = model(x.to(dev))
    torch.cuda.synchronize()
    assert sorted(out) == ["out"] and tuple(out["out"].shape) == (N, 21, H, W)
    assert model._shape == (N, H, W)                       # (a new input shape re-prepared)
    err = rel(torch, out["out"], fcn_reference_forward(torch, sd, x))
    print(f"fcn_resnet50 N={N} {H}x{W}: out {err:.2e}")
    assert err < NET_TOL
    assert pkg.tickets_in_use() == 0


def test_fcn_replays_from_one_graph(fcn, pkg, torch_dev):
    torch, dev = torch_dev
    model, sd = fcn
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
    assert rel(torch, got, fcn_reference_forward(torch, sd, x2)) < NET_TOL
