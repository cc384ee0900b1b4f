"""GPU tests of the two squeeze-excite kernels (se.hip) against fp64 at the project's layer bar, on the guarded arena.
fc_act: a skinny FC over partial sums, with a row's bits independent of its batch.  act_scale_pool: in-place activation
and per-(image, channel) gate on a flat or padded map, a padded map's ring untouched, with the pooled mean."""
import pytest
import torch

import guarded
from gpu_support import same_bits, torch_dev  # noqa: F401
from layer_refs import rel

pytestmark = pytest.mark.gpu

LAYER_TOL = 2e-5
FLOOR = 1e-30   # a ReLU can leave a single output all zero: the error is then absolute, and only an exact 0 passes
MARK = 123.0


def _act(y, act):
    return {"none": y, "relu": y.clamp(min=0), "hardswish": y * (y + 3).clamp(0, 6) / 6, "hardsigmoid": (y + 3).clamp(0, 6) / 6}[act]


def _fc(pkg, dev, parts, W, b, act, scale):
    arena = guarded.Arena(torch, dev, 16)
    out = arena.output(parts.shape[0], W.shape[0], name="out")
    assert pkg.fc_act(arena.input(parts, name="parts"), arena.input(W, name="W"), arena.input(b, name="b"), act, scale, out=out) is out
    arena.check(f"fc_act {tuple(parts.shape)} -> {W.shape[0]}")
    return out.cpu()


@pytest.mark.parametrize("act", ["relu", "hardsigmoid", "hardswish"])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("C,J", [(4, 1), (24, 72), (132, 10), (1284, 70)])
def test_fc_act_matches_fp64_and_rows_do_not_depend_on_the_batch(C, J, P, act, pkg, torch_dev):
    g = torch.Generator().manual_seed(C + J + P)
    parts = torch.randn(9, P, C, generator=g) * 3
    W, b = torch.randn(J, C, generator=g) / C ** 0.5, torch.randn(J, generator=g)
    scale = 1.0 if P == 1 else 1.0 / 7
    want = _act((parts.double().sum(dim=1) * scale) @ W.double().t() + b.double(), act)
    got = _fc(pkg, torch_dev[1], parts, W, b, act, scale)
    err = rel(got, want, FLOOR)
    print(f"C={C} J={J} P={P} {act}: rel err {err:.2e}")
    assert err < LAYER_TOL
    for n in (0, 8):   # the first row of the first chunk, the only row of the second
        assert same_bits(_fc(pkg, torch_dev[1], parts[n:n + 1], W, b, act, scale), got[n:n + 1])


@pytest.mark.parametrize("act", ["hardswish", "none"])
@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("C", [4, 132])
@pytest.mark.parametrize("one_pixel", [True, False])
@pytest.mark.parametrize("padded", [False, True])
def test_act_scale_pool(padded, one_pixel, C, gated, act, pkg, torch_dev):
    _, dev = torch_dev
    chunk = pkg.act_scale_pool_plan(1, 8, 8, C)[0]
    N, (H, W) = 3, (1, 1) if one_pixel else (5, -(-(chunk + 1) // 5))   # H W = chunk + 1, rounded up to rows of 5
    assert one_pixel or chunk < H * W < chunk + 5
    g = torch.Generator().manual_seed(H * W + C)
    x, gate = torch.randn(N, H, W, C, generator=g) * 3, torch.rand(N, C, generator=g) if gated else None
    want = _act(x.double(), act) * (gate.double()[:, None, None, :] if gated else 1.0)
    arena = guarded.Arena(torch, dev, 16)
    xin = arena.input(torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1), value=MARK) if padded else x, name="x", in_place=True)
    parts = arena.output(N, pkg.act_scale_pool_plan(N, H, W, C, padded)[1], C, name="partials")
    got = pkg.act_scale_pool(xin, act, None if gate is None else arena.input(gate, name="gate"), padded, partials=parts)
    assert got[0] is xin and got[1] is parts
    arena.check(f"act_scale_pool {tuple(xin.shape)}")
    y = xin.cpu()
    if padded:
        assert all(bool((r == MARK).all()) for r in (y[:, 0], y[:, -1], y[:, :, 0], y[:, :, -1])), "the ring was written"
        y = y[:, 1:-1, 1:-1, :]
    mean = parts.cpu().double().sum(dim=1) / (H * W)
    assert rel(y, want, FLOOR) < LAYER_TOL
    assert float((mean - want.mean(dim=(1, 2))).abs().max() / want.abs().max()) < LAYER_TOL
