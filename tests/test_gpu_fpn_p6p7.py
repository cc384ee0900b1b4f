"""GPU tests of ResNetFPN(returned_layers=(2, 3, 4), extra_blocks="p6p7"), RetinaNet's backbone: the five levels against
the fp64 CPU forward of tests/fpn_p6p7_reference.py at the bar tests/test_gpu_fpn.py holds whole backbones to
(reference_nets.NET_TOL), on inputs whose P5 and P6 are odd, so that P6 and P7 take (Hin - 1) // 2 + 1; padded outputs
with exact zero rings; one graph; and the default backbone beside it, unchanged."""
import pytest

from fpn_p6p7_reference import p6p7_random_state_dict, p6p7_reference_forward
from gpu_support import R, network_graph_scenario, rel, torch_dev  # noqa: F401
from layer_refs import ring_is
from reference_nets import NET_TOL

pytestmark = pytest.mark.gpu

# N = 1 at 136x200: P3 17x25, P4 9x13, P5 5x7, P6 3x4, P7 2x2 -- an odd size into every stride-2 step, rows and columns.
# N = 2 at 64x64: 8 / 4 / 2 / 1 / 1 -- a single pixel convolved down to a single pixel.
NET_INPUTS = [(1, 136, 200), (2, 64, 64)]
SIZES = {(1, 136, 200): [(17, 25), (9, 13), (5, 7), (3, 4), (2, 2)], (2, 64, 64): [(8, 8), (4, 4), (2, 2), (1, 1), (1, 1)]}
KEYS = ["0", "1", "2", "p6", "p7"]
_NETS = {}


def _net(pkg, R, torch, arch):
    if arch not in _NETS:
        sd, body = p6p7_random_state_dict(torch, R, arch, seed=len(arch) + 1)
        model = pkg.ResNetFPN.from_state_dict(sd, arch, returned_layers=(2, 3, 4), extra_blocks="p6p7")
        refs = {}
        for i, (N, H, W) in enumerate(NET_INPUTS):
            x = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(i + 17)) - 0.5
            refs[(N, H, W)] = (x, p6p7_reference_forward(torch, sd, body, x))
        _NETS[arch] = (model, refs)
    return _NETS[arch]


@pytest.mark.parametrize("shape", NET_INPUTS, ids=["1x136x200", "2x64x64"])
@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_backbone_with_p6p7(arch, shape, pkg, R, torch_dev):
    torch, dev = torch_dev
    model, refs = _net(pkg, R, torch, arch)
    x, want = refs[shape]
    model.prepare(*shape)
    assert len(model._p) == len(model._inner) == 3 and len(model._extra) == 3
    for t in (*model._inner, *model._p):
        t.fill_(float("nan"))
    for t in model._extra:                       # (their rings stay the zeros prepare() wrote: the layer's input contract)
        t[:, 1:-1, 1:-1, :].fill_(float("nan"))
    out = model(x.to(dev))
    torch.cuda.synchronize()
    assert sorted(out) == sorted(want) == sorted(KEYS)
    assert [tuple(out[k].shape[1:3]) for k in KEYS] == SIZES[shape]
    errs = {k: rel(torch, out[k], want[k]) for k in KEYS}
    print(f"{arch}-fpn-p6p7 {shape}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert not {k: v for k, v in errs.items() if not v < NET_TOL}, errs
    assert bool((want["p6"] < 0).any()), "P6 has no negative value: the ReLU in front of P7 is not exercised"
    padded = model(x.to(dev), padded=True)
    torch.cuda.synchronize()
    for k in KEYS:
        p = padded[k]
        assert tuple(p.shape[1:3]) == tuple(s + 2 for s in out[k].shape[1:3]) and ring_is(p.cpu().double(), 0.0), k
        assert torch.equal(p[:, 1:-1, 1:-1, :], out[k]), k
    assert pkg.tickets_in_use() == 0


class _Coarsest:
    """The backbone as network_graph_scenario takes a model: one output tensor, P7 (it depends on every launch but the
    two finer output convolutions); the full dictionary of the last forward stays in .last."""

    def __init__(self, model):
        self.model, self.prepare = model, model.prepare

    def __call__(self, x):
        self.last = self.model(x)
        return self.last["p7"]


def test_p6p7_backbone_in_one_graph(pkg, R, torch_dev):
    torch, dev = torch_dev
    model, refs = _net(pkg, R, torch, "resnet18")
    x, want = refs[NET_INPUTS[0]]
    wrapped = _Coarsest(model)
    eager, graph = network_graph_scenario(pkg, torch, wrapped, x.to(dev))
    assert rel(torch, eager, want["p7"]) < NET_TOL
    outs = wrapped.last
    for t in (*model._inner, *model._p):
        t.fill_(float("nan"))
    for t in model._extra:
        t[:, 1:-1, 1:-1, :].fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for k in KEYS:
        assert rel(torch, outs[k], want[k]) < NET_TOL, k
    del graph


def test_bad_layer_arguments_raise(pkg, R, torch_dev):
    torch, _ = torch_dev
    sd, _ = p6p7_random_state_dict(torch, R, "resnet18", seed=3)
    with pytest.raises(pkg.WinoError, match="unexpected key 'fpn.extra_blocks.p6.weight'"):
        pkg.ResNetFPN.from_state_dict(sd, "resnet18", returned_layers=(2, 3, 4))
    with pytest.raises(pkg.WinoError, match="missing key 'fpn.inner_blocks.3.0.weight'"):
        pkg.ResNetFPN.from_state_dict(sd, "resnet18", extra_blocks="p6p7")
    with pytest.raises(pkg.WinoError, match="returned_layers"):
        pkg.ResNetFPN.from_state_dict(sd, "resnet18", returned_layers=(2, 4), extra_blocks="p6p7")
    with pytest.raises(pkg.WinoError, match="extra_blocks"):
        pkg.ResNetFPN.from_state_dict(sd, "resnet18", returned_layers=(2, 3, 4), extra_blocks="p6")
