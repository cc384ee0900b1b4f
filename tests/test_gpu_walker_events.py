"""The 3x3 throughput kernel's main loop runs from event to event: the DMA stream (two iterations ahead of the MFMAs)
changes item or reaches the end of the workgroup's range, the compute segment ends, or both at once, and each entry
starts on an even or an odd iteration.  The shapes and forced grids (WINO_SK_GRID) below are
small enough to run in a blink and are chosen so that every event, every coincidence of events and both entry parities
occur; the comment on each says what it is there for.

Every launch writes into a NaN-filled output and is compared three ways: with the direct comparator at the suite's
TIGHT, with the automatic grid's result at 2e-6 x max|ref| (the bound test_conv3x3_streamk_decompositions_agree holds
the decompositions to: the cut points only move the order of the channel sum), and bit for bit with a second, identical
launch.  After every launch the output's ring is zero and no ticket counter is left set."""
import pytest

from cases import TIGHT
from gpu_support import torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu

PLAIN = [
    # 3 tile blocks, the last with clamped tiles; 3 chunks per item, so segments start on odd `it`; ranges of 9, 3 and 1
    # iterations: the prologue's two advances and the stream's end in the first iterations; 10: a workgroup without work
    ((3, 14, 14, 24, 64), (1, 2, 3, 4, 5, 7, 9, 10)),
    # two out-channel blocks: item switches that keep the tile block (the per-lane offsets must survive), and the
    # tail cut per k-group
    ((2, 14, 14, 16, 128), (1, 2, 3, 4, 5, 8)),
    # one chunk per item: an item switch and a segment end on every iteration, both events together
    ((3, 14, 14, 8, 64), (1, 2, 3, 5)),
    # three k-groups, 5 chunks: tail -> whole-item switch, several whole-item rounds, more workgroups than iterations
    ((5, 14, 14, 40, 192), (1, 5, 7, 11, 12, 13, 24, 60, 61)),
    # the any-feature-map build, odd H and W
    ((4, 5, 9, 24, 64), (1, 3, 7)),
]
CASES = [("plain", shape, g) for shape, grids in PLAIN for g in grids]
CASES += [(kind, (3, 14, 14, 24, 64), g) for kind in ("res", "pool") for g in (2, 5)]

_layers = {}


def _interior(t):
    return t[:, 1:-1, 1:-1, :]


def _ring_is_zero(torch, t):
    inner = torch.zeros_like(t, dtype=torch.bool)
    _interior(inner)[...] = True
    return bool((t[~inner] == 0).all())


def _layer(kind, shape, pkg, torch_dev, knobs):
    """Operands, launcher, the direct comparator's result and the automatic grid's, computed once per layer."""
    key = (kind, shape)
    if key in _layers:
        return _layers[key]
    torch, dev = torch_dev
    N, H, W, C, K = shape
    g = torch.Generator(device="cpu").manual_seed(sum(shape) + len(kind))
    mk = lambda *s: (torch.rand(*s, generator=g) - 0.5).to(dev)   # noqa: E731
    x, w, s, b = mk(N, H + 2, W + 2, C), mk(K, C, 3, 3), mk(K), mk(K)
    U = pkg.filter_transform_f2(w)
    if kind == "plain":
        out_shape = (N, H + 2, W + 2, K)
        run = lambda out: pkg.conv3x3_bn_relu(x, U, b, s, out=out)   # noqa: E731
        direct = _interior(pkg.conv3x3_direct(x, w, b, s))
    elif kind == "res":
        out_shape = (N, H + 2, W + 2, K)
        res = mk(*out_shape)
        run = lambda out: pkg.conv3x3_bn_add_relu(x, U, b, s, res, out=out)   # noqa: E731
        direct = torch.relu(_interior(pkg.conv3x3_direct(x, w, b, s, relu=False)) + _interior(res))
    else:
        out_shape = (N, H // 2 + 2, W // 2 + 2, K)
        run = lambda out: pkg.conv3x3_bn_relu_pool(x, U, b, s, out=out)   # noqa: E731
        full = _interior(pkg.conv3x3_direct(x, w, b, s)).permute(0, 3, 1, 2)
        direct = torch.nn.functional.max_pool2d(full, 2, 2).permute(0, 2, 3, 1)
    direct = direct.clone()
    knobs.unset("WINO_SK_GRID")
    auto = torch.full(out_shape, float("nan"), device=dev)
    run(auto)
    assert pkg.tickets_in_use() == 0
    _layers[key] = (run, out_shape, direct, auto, float(direct.abs().max()))
    return _layers[key]


@pytest.mark.parametrize("kind,shape,grid", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_every_walker_event_and_entry_parity(kind, shape, grid, pkg, torch_dev, knobs):
    torch, dev = torch_dev
    knobs.set("WINO_3X3_ALGO", "big")
    run, out_shape, direct, auto, scale = _layer(kind, shape, pkg, torch_dev, knobs)
    knobs.set("WINO_SK_GRID", str(grid))
    outs = []
    for rep in range(2):
        out = torch.full(out_shape, float("nan"), device=dev)
        run(out)
        assert pkg.tickets_in_use() == 0, f"launch {rep}: an item was left unfinished"
        assert _ring_is_zero(torch, out), f"launch {rep}: the ring is not zero"
        outs.append(out)
    a = outs[0]
    assert not bool(torch.isnan(a).any()), "outputs never written"
    assert torch.equal(a, outs[1]), "not reproducible"
    err_direct = float((_interior(a) - direct).abs().max())
    err_auto = float((a - auto).abs().max())
    print(f"{kind} {shape} grid {grid}: vs direct {err_direct / scale:.2e}, vs automatic grid {err_auto / scale:.2e}")
    assert err_direct < TIGHT * scale
    assert err_auto < 2e-6 * float(auto.abs().max())
