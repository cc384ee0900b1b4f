"""GPU tests of dwconv3x3_bn_act (wino_dwconv3x3_bn_act_hw) against torch CPU fp64 F.conv2d(groups=C) at the project's
layer bar.  Every run is on the guarded arena at both placements into a NaN-filled output, so an unwritten ring or
element shows; the ring of the output must read exactly 0.  The inputs have a standard deviation of 6 / 0.84, so about a
fifth of them exceed an in_cap of 6, and the taps and BN are drawn so that about a fifth of the pre-activation values
exceed 6: both clamps bite."""
import numpy as np
import pytest
import torch

import guarded
import layer_refs
from gpu_support import same_bits, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu

LAYER_TOL = 2e-5   # the project's layer bar
ACTS = (("none", None), ("relu", None), ("relu6", 6.0))
CUS = 256


def _case(N, Hin, Win, C, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * C + Hin)
    x = torch.randn(N, Hin, Win, C, generator=g) * (6 / 0.84)
    w = torch.randn(C, 1, 3, 3, generator=g) / 3
    bias, scale = torch.rand(C, generator=g) - 0.5, torch.rand(C, generator=g) + 0.5
    scale[::3] *= -1
    return x, w, (bias, scale)


def _want(x, w, bn, stride, act, cap):
    xc = layer_refs.f64(x) if cap is None else layer_refs.f64(x).clamp(max=cap)
    y = layer_refs.conv3x3(xc, w, bn, False, stride=stride, groups=int(x.shape[3]))
    return {"none": y, "relu": y.clamp(min=0), "relu6": y.clamp(min=0, max=6)}[act]   # (clamp propagates NaN)


def _run(pkg, dev, x, w, bn, stride, act, cap, aligns=guarded.ALIGNS):
    """The layer on the guarded arena at each placement; the ring is checked, the interior returned (CPU)."""
    N, Hin, Win, C = x.shape
    H, W = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    first = None
    for align in aligns:
        arena = guarded.Arena(torch, dev, align)
        xi = arena.input(layer_refs.ring(x), name="x")
        taps = arena.input(w[:, 0].permute(1, 2, 0).contiguous(), name="w_taps")
        b, s = arena.input(bn[0], name="bias"), arena.input(bn[1], name="scale")
        out = arena.output(N, H + 2, W + 2, C, name="out")
        assert pkg.dwconv3x3_bn_act(xi, taps, b, s, stride, act, cap, out=out) is out
        arena.check(f"dwconv3x3 {tuple(x.shape)} s={stride} {act} align={align}")
        got = out.cpu()
        assert layer_refs.ring_is(got, 0.0), "the output ring is not exactly 0"
        got = layer_refs.interior(got).contiguous()
        first = got if first is None else first
        assert same_bits(got, first), "the two placements differ"
    return first


def _sizes(pkg, stride, C):
    _, th, tw, _, _ = pkg.dwconv3x3_plan(1, 64, 64, C, stride, CUS)
    return [(1, 1), (2, 3), (7, 7), (th * stride, tw * stride), (th * stride + 1, tw * stride + 1)]


@pytest.mark.parametrize("C", [4, 20, 64, 132])
@pytest.mark.parametrize("size", range(5))
@pytest.mark.parametrize("stride", [1, 2])
def test_matches_fp64(stride, size, C, pkg, torch_dev):
    Hin, Win = _sizes(pkg, stride, C)[size]
    for N in (1, 3):
        x, w, bn = _case(N, Hin, Win, C)
        for act, cap in ACTS:
            want = _want(x, w, bn, stride, act, cap)
            err = layer_refs.rel(_run(pkg, torch_dev[1], x, w, bn, stride, act, cap), want)
            print(f"N={N} {Hin}x{Win} C={C} s={stride} {act}: rel err {err:.2e}, "
                  f"inputs over 6: {float((x > 6).float().mean()):.2f}")
            assert err < LAYER_TOL


@pytest.mark.parametrize("stride", [1, 2])
def test_every_instantiation_by_name_and_equal_bits(stride, pkg, torch_dev, knobs):
    N, Hin, Win, C = 2, 19, 21, 132
    x, w, bn = _case(N, Hin, Win, C)
    want, got = _want(x, w, bn, stride, "relu6", 6.0), {}
    assert float((want == 6).double().mean()) > 0.1 and float((x > 6).float().mean()) > 0.15, "the clamps do not bite"
    for cb in (64, 16):
        knobs.set("WINO_DW_CB", cb)
        assert pkg.dwconv3x3_plan(N, Hin, Win, C, stride, CUS)[0] == cb
        got[cb] = _run(pkg, torch_dev[1], x, w, bn, stride, "relu6", 6.0)
        assert layer_refs.rel(got[cb], want) < LAYER_TOL
    assert same_bits(got[64], got[16])


@pytest.mark.parametrize("stride", [1, 2])
def test_nan_footprint(stride, pkg, torch_dev):
    x, w, bn = _case(2, 9, 11, 20)
    clean = _run(pkg, torch_dev[1], x, w, bn, stride, "relu6", 6.0, aligns=(256,))
    hurt = x.clone()
    hurt[1, 3, 5, 7] = float("nan")   # odd row and column: two windows each way at stride 2
    hit = torch.isnan(_want(hurt, w, bn, stride, "relu6", 6.0))   # exactly the windows that hold it
    assert int(hit.sum()) == (9 if stride == 1 else 4) and bool(hit[1, :, :, 7].any())
    got = _run(pkg, torch_dev[1], hurt, w, bn, stride, "relu6", 6.0, aligns=(256,))
    assert torch.equal(torch.isnan(got), hit)
    assert same_bits(got[~hit], clean[~hit]), "another output changed"


@pytest.mark.parametrize("bad", ["overlap", "stride", "channels", "act", "cap", "misaligned"])
def test_refusals_touch_nothing(bad, pkg, torch_dev):
    _, dev = torch_dev
    N, H, W, C = 2, 7, 9, 8
    room = torch.zeros(N * (H + 2) * (W + 2) * C + 4, device=dev)
    x = room[:-4].view(N, H + 2, W + 2, C)
    w, b, s = torch.ones(3, 3, C, device=dev), torch.zeros(C, device=dev), torch.ones(C, device=dev)
    out = torch.full_like(x, float("nan"))
    a = dict(x=x, out=out, C=C, stride=1, act=2, cap=6.0)
    a.update({"overlap": dict(out=x), "stride": dict(stride=3), "channels": dict(C=6), "act": dict(act=7),
              "cap": dict(cap=float("nan")), "misaligned": dict(x=room[1:-3].view(x.shape))}[bad])
    with pytest.raises(pkg.WinoError, match="rc=-2" if bad == "channels" else "rc=-3"):
        pkg._check(pkg.lib().wino_dwconv3x3_bn_act_hw(a["x"].data_ptr(), w.data_ptr(), b.data_ptr(), s.data_ptr(),
                                                      a["out"].data_ptr(), N, H, W, a["C"], a["stride"], a["act"], a["cap"],
                                                      pkg._stream()), "wino_dwconv3x3_bn_act_hw")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool((room == 0).all())
