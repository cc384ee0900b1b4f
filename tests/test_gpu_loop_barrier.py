"""The iteration barrier of the fused 3x3 kernel behind point 0's MFMAs ("The barrier's place").

An iteration runs the 8 MFMAs of point 0 (steps 0 and 1) BEFORE its vmcnt(0) + barrier; the patch reads of the next
iteration's raw stage, the reads of the next filter stage and the LDS-DMA refills come behind it.  What can go wrong with
that order shows at the edges of the pipeline, so the shapes below are the smallest that hold them; the comment on each
says which.  Every launch goes into a NaN-filled output.  The result is compared with the shared fp64 reference of
layer_refs at the suite's TIGHT; its ring is zero; no ticket counter is left set; wino_stream_check is clean.  The cut of
every forced grid is asserted from the plan queries, so the comments cannot drift from the launches.

The race screen repeats three of the cases 200 times, idle and beside a competing stream's launches: the synchronisation
structure is what changed, and a stage refilled or read on the wrong side of the barrier shows as a result that is not bit
for bit the first."""
import ctypes

import numpy as np
import pytest

import layer_refs as LR
from cases import TIGHT
from gpu_support import torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu

# (kind, (N, H, W, C, K), forced grid, the cut the planner makes of it: (whole-item rounds, k-groups, sk_q, sk_rem))
CASES = [
    # C = 8: ONE chunk per item, 7 items.  Three whole-item rounds and a one-iteration tail: every iteration is followed
    # by an epilogue, every body is the first after one (its point 0 runs over the epilogue's stores in flight) and the
    # bodies alternate parity one by one ...
    ("plain", (8, 14, 14, 8, 64), 2, (3, 1, 0, 1)),
    # ... one item per workgroup: the range's only iteration, the prologue's stage 0 and nothing else ...
    ("plain", (8, 14, 14, 8, 64), 7, (1, 1, 0, 0)),
    # ... and two k-groups
    ("plain", (8, 14, 14, 8, 128), 4, (3, 2, 0, 1)),
    # C = 16: two chunks per item: the raw-stage parity wraps inside every item, every entry of the loop is on even
    # parity, and the three-stage filter rotation runs through all its phases across items; tail segments of ONE iteration
    ("plain", (8, 14, 14, 16, 64), 2, (3, 1, 1, 0)),
    ("plain", (8, 14, 14, 16, 64), 3, (2, 1, 0, 2)),
    # C = 24: three chunks per item: the filter rotation wraps inside every item, and the items start on even and odd
    # parity in turn (the loop's odd entry, after the event that ends a segment); tail ranges of one and two iterations
    ("plain", (8, 14, 14, 24, 64), 2, (3, 1, 1, 1)),
    # ... ranges [0, 2) [2, 4) [4, 6) [6, 9) over items of 3: a straddler (2 | 3), one-segment ranges at the start, in
    # the middle and a whole item at the end; the DMA stream's events fall on both parities
    ("plain", (8, 14, 14, 24, 64), 4, (1, 1, 2, 1)),
    # C = 64 on grids that leave tail segments of one iteration (the shapes of the tail-order suite): ranges of 7 over
    # items of 8 -- ranges 0 and 7 whole-first, the rest straddlers ...
    ("plain", (19, 14, 14, 64, 64), 8, (1, 1, 7, 0)),
    # ... and unequal ranges (5 or 6): 6 whole-first ranges, 3 straddlers
    ("plain", (19, 14, 14, 64, 64), 9, (1, 1, 5, 3)),
    # 16 chunks per item: straddling ranges and whole-first ranges behind one whole round ...
    ("plain", (8, 14, 14, 128, 128), 8, (1, 2, 12, 0)),
    # ... and an all-tail grid: no whole round, six straddlers per k-group
    ("plain", (8, 14, 14, 128, 128), 16, (0, 2, 14, 0)),
    # the any-feature-map build: 13 x 13, 7 x 7 tiles with a clipped last tile row and column; three one-segment ranges
    # (2, 3 and 3 iterations) inside one item behind a whole round
    ("plain", (5, 13, 13, 64, 64), 3, (1, 1, 2, 2)),
    # the residual and the pooled entry points, on the shapes whose items change parity and wrap the rotation
    ("res", (8, 14, 14, 24, 64), 2, (3, 1, 1, 1)),
    ("pool", (8, 14, 14, 16, 64), 2, (3, 1, 1, 0)),
]
# the race screen: C = 8, a straddling tail with segments of one iteration, the any-feature-map shape
RACE_CASES = [CASES[0], CASES[8], CASES[11]]
RACE_REPEATS = 200

_layers = {}


def _interior(t):
    return t[:, 1:-1, 1:-1, :]


def _ring_is_zero(torch, t):
    inner = torch.zeros_like(t, dtype=torch.bool)
    _interior(inner)[...] = True
    return bool((t[~inner] == 0).all())


def _cut(pkg, shape):
    """(whole-item rounds, k-groups, sk_q, sk_rem) of the launch the planner makes of `shape` under the knobs in force,
    and its grid: from wino_conv3x3_plan and wino_conv3x3_plan_groups."""
    N, H, W, C, K = shape
    i = [ctypes.c_int() for _ in range(7)]
    tail = ctypes.c_long()
    L = pkg.lib()
    assert L.wino_conv3x3_plan(N, H, W, C, K, 256, ctypes.byref(i[0]), ctypes.byref(i[1]), ctypes.byref(tail), ctypes.byref(i[2])) == 0
    assert L.wino_conv3x3_plan_groups(N, H, W, C, K, 256, *(ctypes.byref(v) for v in i[3:7])) == 0
    grid, rounds, kp = i[0].value, i[1].value, i[3].value
    Tg, Gp = tail.value // kp, grid // kp
    return grid, (rounds, kp, Tg // Gp, Tg % Gp)


def _layer(kind, shape, pkg, torch_dev):
    """Operands, launcher and the fp64 reference, computed once per layer and shared by the tests below."""
    key = (kind, shape)
    if key in _layers:
        return _layers[key]
    torch, dev = torch_dev
    N, H, W, C, K = shape
    g = torch.Generator(device="cpu").manual_seed(sum(shape) + len(kind))
    x = LR.ring(torch.rand(N, H, W, C, generator=g) - 0.5)
    w = (torch.rand(K, C, 3, 3, generator=g) - 0.5) / np.sqrt(9 * C) * 4
    b, s = torch.rand(K, generator=g) - 0.5, torch.rand(K, generator=g) + 0.5
    res = LR.ring(torch.rand(N, H, W, K, generator=g) - 0.5, float("nan"))   # the residual's ring is never read
    xt, bt, st, rt = (a.contiguous().to(dev) for a in (x, b, s, res))
    U = pkg.filter_transform_f2(w.to(dev))
    if kind == "plain":
        out_shape = (N, H + 2, W + 2, K)
        run = lambda out: pkg.conv3x3_bn_relu(xt, U, bt, st, out=out)   # noqa: E731
        want = LR.conv3x3(LR.interior(x), w, (b, s), True)
    elif kind == "res":
        out_shape = (N, H + 2, W + 2, K)
        run = lambda out: pkg.conv3x3_bn_add_relu(xt, U, bt, st, rt, out=out)   # noqa: E731
        want = LR.conv3x3(LR.interior(x), w, (b, s), True, residual=LR.interior(res))
    else:
        out_shape = (N, H // 2 + 2, W // 2 + 2, K)
        run = lambda out: pkg.conv3x3_bn_relu_pool(xt, U, bt, st, out=out)   # noqa: E731
        want = LR.conv3x3(LR.interior(x), w, (b, s), True, pool=True)
    _layers[key] = (run, out_shape, want)
    return _layers[key]


def _checked_launch(pkg, torch_dev, run, out_shape, want, tag):
    torch, dev = torch_dev
    out = torch.full(out_shape, float("nan"), device=dev)
    run(out)
    assert pkg.tickets_in_use() == 0, f"{tag}: an item was left unfinished"
    pkg.stream_check()
    assert not bool(torch.isnan(out).any()), f"{tag}: outputs never written"
    assert _ring_is_zero(torch, out), f"{tag}: the ring is not zero"
    err = LR.rel(_interior(out), want)
    print(f"{tag}: vs fp64 reference {err:.2e}")
    assert err < TIGHT
    return out


_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)   # noqa: E731


@pytest.mark.parametrize("kind,shape,grid,cut", CASES, ids=_ids)
def test_point_0_in_front_of_the_barrier(kind, shape, grid, cut, pkg, torch_dev, knobs):
    knobs.set("WINO_3X3_ALGO", "big")
    run, out_shape, want = _layer(kind, shape, pkg, torch_dev)
    knobs.set("WINO_SK_GRID", str(grid))
    assert _cut(pkg, shape) == (grid, cut)
    _checked_launch(pkg, torch_dev, run, out_shape, want, f"{kind} {shape} grid {grid}")


@pytest.mark.parametrize("kind,shape,grid,cut", RACE_CASES, ids=_ids)
def test_race_screen(kind, shape, grid, cut, pkg, torch_dev, knobs):
    """200 launches idle, then 200 beside a second stream's launches of the same kernel (they hold CUs, so the
    workgroups start apart and the waves of a workgroup meet the barrier in another order): every result is bit for bit
    the first, which is checked against the reference.  Stops at the first difference."""
    torch, dev = torch_dev
    knobs.set("WINO_3X3_ALGO", "big")
    run, out_shape, want = _layer(kind, shape, pkg, torch_dev)
    knobs.set("WINO_SK_GRID", str(grid))
    assert _cut(pkg, shape) == (grid, cut)
    tag = f"{kind} {shape} grid {grid}"
    first = _checked_launch(pkg, torch_dev, run, out_shape, want, tag)
    out = torch.empty_like(first)
    for rep in range(RACE_REPEATS):
        out.fill_(float("nan"))
        run(out)
        assert torch.equal(out, first), f"{tag}: idle, launch {rep} differs from the first"
    g = torch.Generator(device="cpu").manual_seed(29)
    mk = lambda *s: (torch.rand(*s, generator=g) - 0.5).to(dev)   # noqa: E731
    # (a 1x1 layer that fills the chip: the forced grid, which is a handful of workgroups, does not apply to it)
    A, B, vs = mk(64 * 196, 512), mk(512, 128), mk(128)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for rep in range(RACE_REPEATS):
        with torch.cuda.stream(side):
            for _ in range(2):
                pkg.conv1x1_bn(A, B, vs, vs, True)
        out.fill_(float("nan"))
        run(out)
        assert torch.equal(out, first), f"{tag}: beside a competing stream, launch {rep} differs from the first"
    torch.cuda.synchronize()
    assert pkg.tickets_in_use() == 0
    pkg.stream_check()
    with torch.cuda.stream(side):
        assert pkg.tickets_in_use() == 0
