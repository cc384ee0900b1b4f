"""Whole torchvision MobileNetV3s on the library (cuda_winograd_amd.mobilenet_v3): random weights in torchvision's
state-dict format and an fp64 CPU forward from tests/mobilenet_v3_reference.py; the five stride-level maps and the logits
at NET_TOL, the pad channels of every map exactly 0; one forward captured in a torch.cuda.graph replays bitwise equal to
eager, and a second prepare at another shape follows it; bad state dicts name their key before any launch."""
import importlib

import pytest

import mobilenet_v3_reference as ref
from gpu_support import network_graph_scenario, rel, torch_dev  # noqa: F401
from reference_nets import NET_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M(pkg):
    return importlib.import_module("cuda_winograd_amd.mobilenet_v3")


def _input(torch, dev, N, H, W):
    return (torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(N + H)) * 2 - 1).to(dev)


def _check(pkg, torch, M, model, sd, arch, x):
    logits, stages = model.forward(x, stages=True)
    torch.cuda.synchronize()
    want_logits, want = ref.reference_forward(torch, M, sd, arch, x.cpu())
    assert list(stages) == list(want) == list(M.STAGES)
    errs = {}
    for name, w in want.items():
        c = w.shape[3]
        assert stages[name].shape[3] % 64 == 0 and bool((stages[name][..., c:] == 0).all()), f"{name}: pad channels"
        errs[name] = rel(torch, stages[name][..., :c], w)
    errs["logits"] = rel(torch, logits, want_logits)
    print(f"{arch} N={x.shape[0]} {x.shape[2]}x{x.shape[3]}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < NET_TOL for v in errs.values()), errs
    assert pkg.tickets_in_use() == 0


@pytest.mark.parametrize("H,W", [(64, 64), (70, 45)])
@pytest.mark.parametrize("arch", ["large", "small"])
def test_network_matches_fp64(arch, H, W, pkg, M, torch_dev):
    torch, dev = torch_dev
    sd = ref.random_state_dict(torch, M, arch, classes=10, seed=H)
    model = pkg.MobileNetV3.from_state_dict(sd, arch)
    assert model.classes == 10
    _check(pkg, torch, M, model, sd, arch, _input(torch, dev, 2, H, W))


@pytest.mark.parametrize("arch", ["large", "small"])
def test_whole_network_graph_replay_and_reprepare(arch, pkg, M, torch_dev):
    torch, dev = torch_dev
    sd = ref.random_state_dict(torch, M, arch, classes=10, seed=77)
    model = pkg.MobileNetV3.from_state_dict(sd, arch)
    x = _input(torch, dev, 2, 64, 64)
    eager, graph = network_graph_scenario(pkg, torch, model, x)
    assert rel(torch, eager, ref.reference_forward(torch, M, sd, arch, x.cpu())[0]) < NET_TOL
    model.prepare(3, 45, 70)   # a second prepare at another shape, eager
    _check(pkg, torch, M, model, sd, arch, _input(torch, dev, 3, 45, 70))
    del graph


@pytest.mark.parametrize("bad", ["missing", "shape"])
def test_bad_state_dicts_name_the_key(bad, pkg, M, torch_dev):
    torch, _ = torch_dev
    sd = ref.random_state_dict(torch, M, "large", classes=10)
    key = "features.5.block.2.fc1.bias" if bad == "missing" else "features.4.block.1.0.weight"   # an SE key; a 5x5 weight
    if bad == "missing":
        del sd[key]
    else:
        assert tuple(sd[key].shape[2:]) == (5, 5)
        sd[key] = sd[key][:, :, :3, :3]
    with pytest.raises(pkg.WinoError, match=key.replace(".", r"\.")):
        pkg.MobileNetV3.from_state_dict(sd, "large")
