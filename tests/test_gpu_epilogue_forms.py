"""Every kind of epilogue of the 3x3 throughput kernel ("Epilogue"), on shapes small enough to
run in a blink.  The forced grids (WINO_SK_GRID) cut the work so that each kind occurs: a whole item finalized from
registers; partial segments at the head of a range, continuing an item and straddling two; a ticket deferred to the next
epilogue and one drawn at once; gathers of two and of three or more segments; a workgroup without work.  Both halves of
the A^T m A pair exchange (ph = 0 / 1) run in every launch.

Every launch writes into a NaN-filled output and is compared three ways: with the direct comparator at the suite's
TIGHT, with the automatic grid's result at 2e-6 x max|ref| (the cut points only move the order of the channel sum), and
bit for bit with a second, identical launch.  After every launch the output's ring is zero and no ticket counter is
left set.

Stale accumulators: the epilogue re-zeroes the 128 accumulator registers between segments.  With the first 64 tiles' input
(image 0 and 15 tiles of image 1: the first tile block) scaled by 1e4 and the rest by 1e-4 -- and the other way round --
a register that kept its value would show as an error of order 1e4 x the tolerance.

Signs: A^T m A folds the minus of its second row into the add that consumes the part.  One case negates every weight;
one sets a single input channel of one tile's patch to +Inf and requires every output outside that patch's receptive
field to keep the finite run's bits."""
import pytest

from cases import TIGHT
from gpu_support import torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu

S3 = (3, 14, 14, 24, 64)
PLAIN = [
    # 3 tile blocks (the last with clamped tiles), 3 chunks per item: 1 = whole items only, one after the other in one
    # workgroup; 2 .. 9 = ranges of 5 .. 1 iterations: heads, continuations, straddlers, deferred and immediate tickets,
    # gathers of 2 and of 3 segments; 10 = a workgroup without work
    (S3, (1, 2, 3, 4, 5, 7, 9, 10)),
    # two out-channel blocks: the tail cut per k-group, slab slots numbered by (range, group)
    ((2, 14, 14, 16, 128), (2, 3, 5, 8)),
    # three k-groups, 5 chunks: tail then whole-item rounds; 61 = more workgroups than iterations
    ((5, 14, 14, 40, 192), (5, 7, 13, 61)),
    # the any-feature-map build, clipped last tile row and column: the store loop's tile addressing and `keep`
    ((4, 5, 9, 24, 64), (1, 3, 7)),
]
CASES = [("plain", shape, g) for shape, grids in PLAIN for g in grids]
CASES += [(kind, S3, g) for kind in ("res", "pool") for g in (2, 5)]
# the first tile block loud and the rest quiet, and the other way round: grid 1 = whole items back to back in one
# workgroup, grid 4 = partial segments of neighbouring items back to back
CASES += [(kind, S3, g) for kind in ("loud-first", "quiet-first") for g in (1, 4)]
CASES += [("negated", S3, 5)]

_layers = {}


def _interior(t):
    return t[:, 1:-1, 1:-1, :]


def _ring_is_zero(torch, t):
    inner = torch.zeros_like(t, dtype=torch.bool)
    _interior(inner)[...] = True
    return bool((t[~inner] == 0).all())


def _same_bits(torch, a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _first_block_mask(torch, N, H, W):
    """[N][H+2][W+2] bool: the padded input pixels whose output pixel lies in the first 64 tiles (ring pixels go with
    their nearest output pixel)."""
    tx_n = (W + 1) // 2
    tiles = ((H + 1) // 2) * tx_n
    oy = (torch.arange(H + 2) - 1).clamp(0, H - 1) // 2
    ox = (torch.arange(W + 2) - 1).clamp(0, W - 1) // 2
    g = torch.arange(N)[:, None, None] * tiles + oy[None, :, None] * tx_n + ox[None, None, :]
    return g < 64


def _operands(kind, shape, torch, dev):
    N, H, W, C, K = shape
    g = torch.Generator(device="cpu").manual_seed(sum(shape) + len(kind))
    mk = lambda *s: torch.rand(*s, generator=g) - 0.5   # noqa: E731
    x, w, s, b = mk(N, H + 2, W + 2, C), mk(K, C, 3, 3), mk(K), mk(K)
    if kind in ("loud-first", "quiet-first"):
        first = _first_block_mask(torch, N, H, W)[..., None]
        loud, quiet = (1e4, 1e-4) if kind == "loud-first" else (1e-4, 1e4)
        x = x * torch.where(first, torch.tensor(loud), torch.tensor(quiet))
    if kind == "negated":
        w = -w
    return x.to(dev), w.to(dev), s.to(dev), b.to(dev), g


def _layer(kind, shape, pkg, torch_dev, knobs):
    """Operands, launcher, the direct comparator's result and the automatic grid's, computed once per layer."""
    key = (kind, shape)
    if key in _layers:
        return _layers[key]
    torch, dev = torch_dev
    N, H, W, C, K = shape
    x, w, s, b, g = _operands(kind, shape, torch, dev)
    U = pkg.filter_transform_f2(w)
    if kind == "res":
        out_shape = (N, H + 2, W + 2, K)
        res = (torch.rand(*out_shape, generator=g) - 0.5).to(dev)
        run = lambda out: pkg.conv3x3_bn_add_relu(x, U, b, s, res, out=out)   # noqa: E731
        direct = torch.relu(_interior(pkg.conv3x3_direct(x, w, b, s, relu=False)) + _interior(res))
    elif kind == "pool":
        out_shape = (N, H // 2 + 2, W // 2 + 2, K)
        run = lambda out: pkg.conv3x3_bn_relu_pool(x, U, b, s, out=out)   # noqa: E731
        full = _interior(pkg.conv3x3_direct(x, w, b, s)).permute(0, 3, 1, 2)
        direct = torch.nn.functional.max_pool2d(full, 2, 2).permute(0, 2, 3, 1)
    else:
        out_shape = (N, H + 2, W + 2, K)
        run = lambda out: pkg.conv3x3_bn_relu(x, U, b, s, out=out)   # noqa: E731
        direct = _interior(pkg.conv3x3_direct(x, w, b, s))
    direct = direct.clone()
    knobs.unset("WINO_SK_GRID")
    auto = torch.full(out_shape, float("nan"), device=dev)
    run(auto)
    assert pkg.tickets_in_use() == 0
    _layers[key] = (run, out_shape, direct, auto, float(direct.abs().max()))
    return _layers[key]


def _launch_twice(torch, dev, pkg, run, out_shape):
    outs = []
    for rep in range(2):
        out = torch.full(out_shape, float("nan"), device=dev)
        run(out)
        assert pkg.tickets_in_use() == 0, f"launch {rep}: an item was left unfinished"
        assert _ring_is_zero(torch, out), f"launch {rep}: the ring is not zero"
        outs.append(out)
    assert _same_bits(torch, outs[0], outs[1]), "not reproducible"
    return outs[0]


@pytest.mark.parametrize("kind,shape,grid", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_every_epilogue_kind(kind, shape, grid, pkg, torch_dev, knobs):
    torch, dev = torch_dev
    knobs.set("WINO_3X3_ALGO", "big")
    run, out_shape, direct, auto, scale = _layer(kind, shape, pkg, torch_dev, knobs)
    knobs.set("WINO_SK_GRID", str(grid))
    a = _launch_twice(torch, dev, pkg, run, out_shape)
    assert not bool(torch.isnan(a).any()), "outputs never written"
    err_direct = float((_interior(a) - direct).abs().max())
    err_auto = float((a - auto).abs().max())
    print(f"{kind} {shape} grid {grid}: vs direct {err_direct / scale:.2e}, vs automatic grid {err_auto / scale:.2e}")
    assert err_direct < TIGHT * scale
    assert err_auto < 2e-6 * float(auto.abs().max())


@pytest.mark.parametrize("grid", (1, 4))
def test_inf_in_one_tile_stays_in_its_receptive_field(grid, pkg, torch_dev, knobs):
    """One input channel of one tile's 4 x 4 patch is +Inf.  The outputs whose 3 x 3 window touches the patch (all
    out-channels) may be anything; every other element keeps the bits of the finite run on the same grid."""
    torch, dev = torch_dev
    N, H, W, C, K = S3
    knobs.set("WINO_3X3_ALGO", "big")
    knobs.set("WINO_SK_GRID", str(grid))
    x, w, s, b, _ = _operands("inf", S3, torch, dev)
    U = pkg.filter_transform_f2(w)
    out_shape = (N, H + 2, W + 2, K)
    finite = _launch_twice(torch, dev, pkg, lambda out: pkg.conv3x3_bn_relu(x, U, b, s, out=out), out_shape)
    assert bool(torch.isfinite(finite).all())
    n, ty, tx, c = 1, 3, 4, 5          # tile 25 of image 1: tile 74, in the second tile block; its patch starts at (6, 8)
    xi = x.clone()
    xi[n, 2 * ty:2 * ty + 4, 2 * tx:2 * tx + 4, c] = float("inf")
    got = _launch_twice(torch, dev, pkg, lambda out: pkg.conv3x3_bn_relu(xi, U, b, s, out=out), out_shape)
    # padded input rows Y .. Y+3 are read by the outputs at padded rows Y-1 .. Y+4 (window rows oy-1 .. oy+1)
    touched = torch.zeros(out_shape, dtype=torch.bool, device=dev)
    touched[n, max(2 * ty - 1, 0):2 * ty + 5, max(2 * tx - 1, 0):2 * tx + 5, :] = True
    assert not bool(torch.isfinite(got[touched]).all()), "the Inf never reached an output"
    assert _same_bits(torch, got[~touched], finite[~touched]), "the Inf left its receptive field"
