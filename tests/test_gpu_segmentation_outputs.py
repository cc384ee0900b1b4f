"""GPU tests of the segmentation networks' output options (cuda_winograd_amd.segmentation: resize="kernel", labels,
aux, out=False) on FCN-ResNet50 and DeepLabV3-ResNet50, against the fp64 CPU forward of
tests/segmentation_aux_reference.py driven by a random state dict with a complete aux_classifier: both heads at the
project's network bar, the label map under the gap rule, the default path bitwise what it was, and all three outputs
replayed from one graph."""
import pytest

from gpu_support import R, rel, torch_dev  # noqa: F401
from reference_nets import NET_TOL
from resize_cases import check_labels
from segmentation_aux_reference import aux_state_dict, reference_outputs

pytestmark = pytest.mark.gpu
NETS = {"fcn": ("FCN", 3), "deeplabv3": ("DeepLabV3", 4)}   # class, state-dict seed
SHAPES = [(1, 65, 65), (2, 49, 81)]


@pytest.fixture(scope="module", params=sorted(NETS))
def net(request, pkg, R, torch_dev):
    """One network loaded with its aux head, its state dict, and the fp64 references of the module's inputs (computed
    once per shape)."""
    torch, dev = torch_dev
    cls, seed = NETS[request.param]
    sd = aux_state_dict(torch, R, request.param, "resnet50", classes=21, seed=seed)
    model = getattr(pkg, cls).from_state_dict(sd, "resnet50", aux=True)
    assert model.has_aux
    cache = {}

    def case(N, H, W):
        if (N, H, W) not in cache:
            x = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(N + H)) - 0.5
            cache[N, H, W] = (x, reference_outputs(torch, request.param, sd, x))
        return cache[N, H, W]

    return request.param, model, case


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_kernel_outputs_against_the_fp64_forward(N, H, W, net, pkg, torch_dev):
    torch, dev = torch_dev
    name, model, case = net
    x, want = case(N, H, W)
    xd = x.to(dev)
    got = model(xd, resize="kernel", labels=True, aux=True)
    torch.cuda.synchronize()
    assert sorted(got) == ["aux", "labels", "out"]
    assert tuple(got["out"].shape) == tuple(got["aux"].shape) == (N, 21, H, W)
    assert tuple(got["labels"].shape) == (N, H, W) and got["labels"].dtype == torch.int32
    assert got["out"].data_ptr() == model._out.data_ptr()          # the model's own buffer, returned as it stands
    errs = {k: rel(torch, got[k], want[k]) for k in ("out", "aux")}
    print(f"{name} N={N} {H}x{W}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < NET_TOL for v in errs.values()), errs
    labels = got["labels"].cpu().numpy()
    check_labels(labels, want["out"].numpy(), NET_TOL, f"{name} N={N} {H}x{W}")
    assert pkg.tickets_in_use() == 0
    # the fused case: only the label map is written
    model._out.fill_(float("nan"))
    fused = model(xd, labels=True, out=False)
    torch.cuda.synchronize()
    assert sorted(fused) == ["labels"] and bool(torch.isnan(model._out).all())
    assert (fused["labels"].cpu().numpy() == labels).all()
    # the kernel's out without labels or aux
    only = model(xd, resize="kernel")
    assert sorted(only) == ["out"] and rel(torch, only["out"], want["out"]) == errs["out"]
    assert pkg.tickets_in_use() == 0


def test_default_is_the_torch_path_bitwise(net, pkg, torch_dev):
    torch, dev = torch_dev
    name, model, case = net
    x, want = case(1, 65, 65)
    xd = x.to(dev)
    a = model(xd)
    assert sorted(a) == ["out"]
    b = model(xd, resize="torch")
    assert sorted(b) == ["out"] and a["out"].data_ptr() != b["out"].data_ptr()   # new tensors of torch's
    assert torch.equal(a["out"], b["out"])
    assert rel(torch, a["out"], want["out"]) < NET_TOL
    c = model(xd, aux=True)                                          # the aux head through torch's resize
    assert sorted(c) == ["aux", "out"] and torch.equal(c["out"], a["out"])
    assert rel(torch, c["aux"], want["aux"]) < NET_TOL
    with pytest.raises(pkg.WinoError, match="labels=True"):
        model(xd, out=False)
    with pytest.raises(pkg.WinoError, match="resize"):
        model(xd, resize="nearest")
    assert pkg.tickets_in_use() == 0


def test_aux_needs_a_model_loaded_with_it(net, pkg, torch_dev):
    torch, dev = torch_dev
    name, model, case = net
    bare = type(model)("resnet50", 21, dev)                          # (unpacked: the option is refused before any launch)
    assert not bare.has_aux
    with pytest.raises(pkg.WinoError, match="aux=True"):
        bare(case(1, 65, 65)[0].to(dev), aux=True)


def test_all_outputs_replay_from_one_graph(net, pkg, torch_dev):
    torch, dev = torch_dev
    name, model, case = net
    x = case(1, 65, 65)[0].to(dev)
    sg = torch.cuda.Stream()
    with torch.cuda.stream(sg):
        model.prepare(1, 65, 65)
        eager = {k: v.clone() for k, v in model(x, resize="kernel", labels=True, aux=True).items()}
    sg.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=sg):
        out = model(x, resize="kernel", labels=True, aux=True)
    assert sorted(out) == ["aux", "labels", "out"]
    for _ in range(2):
        out["out"].fill_(float("nan"))
        out["aux"].fill_(float("nan"))
        out["labels"].fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        for k in out:
            assert torch.equal(out[k], eager[k]), k
    with torch.cuda.stream(sg):
        assert pkg.tickets_in_use() == 0
    del graph
    assert pkg.tickets_in_use() == 0
