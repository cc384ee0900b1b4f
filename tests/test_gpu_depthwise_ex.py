"""GPU tests of dwconv_bn_act (wino_dwconv_bn_act_hw), the depthwise K x K layer for K = 3 and 5, against torch CPU fp64
F.conv2d(groups=C, padding=K // 2) at the project's layer bar.  Every run is on the guarded arena at both placements into
NaN-filled outputs; the output ring must read exactly 0.  The inputs have a standard deviation of 3, so about 16 % of
them lie below -3 and 16 % above 3: all three branches of the hardswish are taken.  On the 1 x 1 and 2 x 3 maps every tap
but the centre lands on the ring or beyond it: the zero-staged positions outside the padded input feed real outputs."""
import pytest
import torch

import guarded
import layer_refs
from gpu_support import same_bits, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu

LAYER_TOL = 2e-5   # the project's layer bar
FLOOR = 1e-30      # a ReLU can leave a 1 x 1 map all zero: the error is then absolute, and only an exact 0 passes
ACTS = ((None, "none"), (None, "relu"), ("hardswish", "hardswish"))
F = torch.nn.functional


def _act(y, act):
    return {None: y, "none": y, "relu": y.clamp(min=0), "hardswish": y * (y + 3).clamp(0, 6) / 6}[act]


def _case(N, Hin, Win, C, K, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * C + 10 * Hin + K)
    x = torch.randn(N, Hin, Win, C, generator=g) * 3
    w = torch.randn(C, 1, K, K, generator=g) / K
    bias, scale = torch.rand(C, generator=g) - 0.5, torch.rand(C, generator=g) + 0.5
    scale[::3] *= -1
    return x, w, (bias, scale)


def _want(x, w, bn, stride, in_act, act):
    K = int(w.shape[2])
    y = F.conv2d(layer_refs.nchw(_act(layer_refs.f64(x), in_act)), w.double(), stride=stride, padding=K // 2, groups=int(x.shape[3]))
    return _act(layer_refs.nhwc(layer_refs.affine(y, bn)), act)


def _run(pkg, dev, x, w, bn, stride, in_act, act, pool=False, aligns=guarded.ALIGNS):
    """The layer on the guarded arena at each placement; the ring is checked; (interior, partials or None) on the CPU."""
    N, Hin, Win, C = x.shape
    K, H, W = int(w.shape[2]), (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    first = None
    for align in aligns:
        arena = guarded.Arena(torch, dev, align)
        xi = arena.input(layer_refs.ring(x), name="x")
        taps = arena.input(w[:, 0].permute(1, 2, 0).contiguous(), name="w_taps")
        b, s = arena.input(bn[0], name="bias"), arena.input(bn[1], name="scale")
        out = arena.output(N, H + 2, W + 2, C, name="out")
        parts = None
        if pool:
            _, _, _, ty, tx = pkg.dwconv_plan(N, Hin, Win, C, K, stride, pkg._cus(dev))
            parts = arena.output(N, ty * tx, C, name="partials")
        got = pkg.dwconv_bn_act(xi, taps, b, s, stride, act, in_act, out=out, partials=parts)
        assert (got[0] is out and got[1] is parts) if pool else got is out
        arena.check(f"dwconv {tuple(x.shape)} K={K} s={stride} {in_act}/{act} align={align}")
        got = out.cpu()
        assert layer_refs.ring_is(got, 0.0), "the output ring is not exactly 0"
        cur = (layer_refs.interior(got).contiguous(), parts.cpu() if pool else None)
        first = cur if first is None else first
        assert same_bits(cur[0], first[0]) and (not pool or same_bits(cur[1], first[1])), "the two placements differ"
    return first


def _sizes(pkg, K, stride, C):
    _, th, tw, _, _ = pkg.dwconv_plan(1, 64, 64, C, K, stride, 256)
    return [(1, 1), (2, 3), (th * stride, tw * stride), (th * stride + 1, tw * stride + 1)]


@pytest.mark.parametrize("C", [4, 132])
@pytest.mark.parametrize("size", range(4))
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("K", [3, 5])
def test_matches_fp64_with_pool(K, stride, size, C, pkg, torch_dev):
    Hin, Win = _sizes(pkg, K, stride, C)[size]
    for N in (1, 3):
        x, w, bn = _case(N, Hin, Win, C, K)
        if x.numel() >= 4000:
            assert float((x < -3).float().mean()) > 0.1 and float((x > 3).float().mean()) > 0.1, "a hardswish branch is idle"
        for in_act, act in ACTS:
            want = _want(x, w, bn, stride, in_act, act)
            got, parts = _run(pkg, torch_dev[1], x, w, bn, stride, in_act, act, pool=True)
            err = layer_refs.rel(got, want, FLOOR)
            mean = parts.double().sum(dim=1) / (want.shape[1] * want.shape[2])
            perr = float((mean - want.mean(dim=(1, 2))).abs().max() / max(float(want.abs().max()), FLOOR))
            print(f"N={N} {Hin}x{Win} C={C} K={K} s={stride} {in_act}/{act}: rel err {err:.2e}, pooled {perr:.2e}")
            assert err < LAYER_TOL and perr < LAYER_TOL


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("K", [3, 5])
def test_channel_blocks_and_the_3x3_entry_give_equal_bits(K, stride, pkg, torch_dev, knobs):
    N, Hin, Win, C = 2, 19, 21, 132
    x, w, bn = _case(N, Hin, Win, C, K)
    got = {}
    for cb in (64, 16):
        knobs.set("WINO_DW_CB", cb)
        assert pkg.dwconv_plan(N, Hin, Win, C, K, stride, 256)[0] == cb
        got[cb] = _run(pkg, torch_dev[1], x, w, bn, stride, "hardswish", "hardswish", pool=True)
        assert layer_refs.rel(got[cb][0], _want(x, w, bn, stride, "hardswish", "hardswish")) < LAYER_TOL
    assert same_bits(got[64][0], got[16][0])
    if K == 3:
        knobs.unset("WINO_DW_CB")
        dev = torch_dev[1]
        new = _run(pkg, dev, x, w, bn, stride, None, "relu6")[0]
        old = pkg.dwconv3x3_bn_act(layer_refs.ring(x).to(dev), w[:, 0].permute(1, 2, 0).contiguous().to(dev), bn[0].to(dev),
                                   bn[1].to(dev), stride, "relu6")
        assert same_bits(new, layer_refs.interior(old.cpu()).contiguous())


@pytest.mark.parametrize("stride", [1, 2])
def test_nan_footprint_5x5(stride, pkg, torch_dev):
    x, w, bn = _case(2, 9, 11, 20, 5)
    clean = _run(pkg, torch_dev[1], x, w, bn, stride, "hardswish", "hardswish", aligns=(256,))[0]
    hurt = x.clone()
    hurt[1, 3, 5, 7] = float("nan")
    hit = torch.isnan(_want(hurt, w, bn, stride, "hardswish", "hardswish"))   # exactly the windows that hold it
    assert int(hit.sum()) == (25 if stride == 1 else 4) and bool(hit[1, :, :, 7].any())
    got = _run(pkg, torch_dev[1], hurt, w, bn, stride, "hardswish", "hardswish", aligns=(256,))[0]
    assert torch.equal(torch.isnan(got), hit)
    assert same_bits(got[~hit], clean[~hit]), "another output changed"


@pytest.mark.parametrize("bad", ["K", "act", "channels", "pool_tiles", "overlap"])
def test_refusals_touch_nothing(bad, pkg, torch_dev):
    _, dev = torch_dev
    N, H, W, C = 2, 7, 9, 8
    room = torch.zeros(N * (H + 2) * (W + 2) * C, device=dev)
    x = room.view(N, H + 2, W + 2, C)
    w, b, s = torch.ones(5, 5, C, device=dev), torch.zeros(C, device=dev), torch.ones(C, device=dev)
    out, parts = torch.full_like(x, float("nan")), torch.full((N, 2, C), float("nan"), device=dev)
    tiles = pkg.dwconv_plan(N, H, W, C, 5, 1, pkg._cus(dev))
    assert tiles[3] * tiles[4] == 2
    a = dict(out=out, C=C, K=5, act=3, tiles=2)
    a.update({"K": dict(K=4), "act": dict(act=9), "channels": dict(C=6), "pool_tiles": dict(tiles=3), "overlap": dict(out=x)}[bad])
    with pytest.raises(pkg.WinoError, match="rc=-2" if bad == "channels" else "rc=-3"):
        pkg._check(pkg.lib().wino_dwconv_bn_act_hw(x.data_ptr(), w.data_ptr(), b.data_ptr(), s.data_ptr(), a["out"].data_ptr(),
                                                   parts.data_ptr(), N, H, W, a["C"], a["K"], 1, a["act"], 0, a["tiles"],
                                                   pkg._stream()), "wino_dwconv_bn_act_hw")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(parts).all()) and bool((room == 0).all())
