"""GPU tests of the concat projection, wino_conv1x1_cat_bn_hw (the tiled 1x1 GEMM kernel in operand form A_CAT: K runs
through S sources, one bias row per image), and of the ASPP module built on it.  Against the fp64 references of
tests/aspp_cases.py, into NaN-filled outputs, at cases.TIGHT: parity, the forced forms, the guarded arena, the
non-finite footprint, and eager against graph replay."""
import ctypes

import pytest

from aspp_cases import ASPP_SHAPES, A_PADDED, CAT_FORM_SHAPES, CAT_SHAPES, C_PADDED, RELU, AsppCase, CatLayer
from dilated_cases import FORMS
from gpu_support import graph_replay_scenario, torch_dev  # noqa: F401
from guarded import ALIGNS, Arena

pytestmark = pytest.mark.gpu
ids = lambda s: "x".join(str(v) for v in s).replace("(", "").replace(")", "").replace(", ", "-") if isinstance(s, tuple) else str(s)


# ---- the concat layer ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CAT_SHAPES, ids=ids)
def test_cat_layer_parity(shape, pkg, O, torch_dev):
    """ReLU on and off, sources padded (NaN rings) and unpadded, output padded (ring exactly 0) and unpadded; once with
    the sources further apart than their size and NaN in the gaps."""
    layer = CatLayer(pkg, torch_dev, *shape, seed=sum(shape))
    for relu in (True, False):
        for a_padded in (False, True):
            for c_padded in (False, True):
                got = layer.run(relu, a_padded, c_padded)
                layer.check(O, got, relu, c_padded, f"a_padded={a_padded} c_padded={c_padded}")
    for a_padded, gap in ((False, 4), (True, 260)):
        layer.check(O, layer.run(True, a_padded, True, gap=gap), True, True, f"a_padded={a_padded} gap={gap}")
    assert pkg.tickets_in_use() == 0


def _gemm_waves(pkg, M, Cin, Kout):
    v = [ctypes.c_int(0) for _ in range(5)]
    assert pkg.lib().wino_conv1x1_plan(M, Cin, Kout, 256, *[ctypes.byref(x) for x in v]) == 0
    return Kout // v[2].value // 16   # columns per block / 16


@pytest.mark.parametrize("form,shape", [(f, s) for s in CAT_FORM_SHAPES for f in sorted(FORMS)])
def test_cat_forced_forms(form, shape, pkg, O, torch_dev, knobs):
    """Whole tiles and stream-K, with grids whose ranges start, end and cross source boundaries, on 8-wave and on
    4-wave tiles: against the reference, bitwise equal from launch to launch, no ticket left."""
    torch, _ = torch_dev
    N, H, W, S, Cs, Kout = shape
    for k, v in FORMS[form].items():
        knobs.set(k, v)
    assert pkg.conv1x1_cat_plan(*shape) == (pkg.FORM_TILED if form == "tiled" else pkg.FORM_STREAM_K)
    assert _gemm_waves(pkg, N * H * W, S * Cs, Kout) == (8 if shape == CAT_FORM_SHAPES[0] else 4)
    layer = CatLayer(pkg, torch_dev, *shape, seed=sum(shape))
    srcs = layer.sources(a_padded := (form != "tiled"))
    a = layer.run(True, a_padded, True, srcs=srcs).clone()
    layer.check(O, a, True, True, form)
    assert torch.equal(layer.run(True, a_padded, True, srcs=srcs), a)
    assert pkg.tickets_in_use() == 0


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("shape,flags", [((2, 5, 7, 3, 64, 64), RELU | C_PADDED), ((3, 4, 4, 2, 96, 128), RELU | A_PADDED),
                                         ((1, 9, 9, 8, 32, 64), A_PADDED | C_PADDED)], ids=ids)
def test_cat_layer_in_the_guarded_arena(shape, flags, align, pkg, O, torch_dev):
    """NaN directly before and behind every operand, sentinel guards around the output: no guard byte changes, and no
    NaN beside an operand reaches the result (the first and the last source's windows included)."""
    torch, dev = torch_dev
    N, H, W, S, Cs, Kout = shape
    layer = CatLayer(pkg, torch_dev, *shape, seed=7 + align)
    arena = Arena(torch, dev, align)
    stack = torch.stack([v.cpu() for v in layer.sources(bool(flags & A_PADDED))])   # [S][N][h][w][Cs], NaN rings kept
    srcs = arena.input(stack, name="src")
    w, b, s = arena.input(layer.w, name="w"), arena.input(layer.bias, name="bias_per_image"), arena.input(layer.scale, name="bnScale")
    p = 2 if flags & C_PADDED else 0
    out = arena.output(N, H + p, W + p, Kout, name="out")
    pkg.conv1x1_cat_bn(srcs, w, b, s, flags, out=out)
    arena.check(f"concat layer {shape} flags {flags} align {align}")
    layer.check(O, out, bool(flags & RELU), bool(flags & C_PADDED))


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
def test_a_nan_in_one_source_reaches_exactly_its_pixel(relu, pkg, torch_dev):
    """a NaN at one pixel of one source makes exactly that output pixel NaN, in every channel; every
    other bit is the clean run's."""
    torch, dev = torch_dev
    N, H, W, S, Cs, Kout = shape = (2, 9, 9, 4, 64, 64)
    layer = CatLayer(pkg, torch_dev, *shape, seed=5)
    srcs = layer.sources()
    clean = layer.run(relu, srcs=srcs).clone()
    assert bool(torch.isfinite(clean).all())
    for j, n, y, x in ((0, 0, 0, 0), (2, 1, 4, 7), (3, 1, 8, 8)):
        keep = srcs[j][n, y, x, Cs // 3].clone()
        srcs[j][n, y, x, Cs // 3] = float("nan")
        got = layer.run(relu, srcs=srcs)
        srcs[j][n, y, x, Cs // 3] = keep
        want_bad = torch.zeros_like(clean, dtype=torch.bool)
        want_bad[n, y, x, :] = True
        assert torch.equal(torch.isnan(got), want_bad), (j, n, y, x)
        assert torch.equal(got[~want_bad].view(torch.int32), clean[~want_bad].view(torch.int32))


def test_an_inf_in_one_images_bias_changes_only_that_image(pkg, torch_dev):
    torch, dev = torch_dev
    N, H, W, S, Cs, Kout = shape = (5, 5, 5, 2, 32, 64)   # one tile holds all five images
    layer = CatLayer(pkg, torch_dev, *shape, seed=6)
    srcs = layer.sources()
    clean = layer.run(True, srcs=srcs).clone()
    bias = layer.bt.clone()
    bias[3, 17] = float("inf")
    got = layer.run(True, srcs=srcs, bias=bias)
    want_bad = torch.zeros_like(clean, dtype=torch.bool)
    want_bad[3, :, :, 17] = True
    assert torch.equal(~torch.isfinite(got), want_bad)
    assert bool((got[want_bad] == float("inf")).all())
    assert torch.equal(got[~want_bad].view(torch.int32), clean[~want_bad].view(torch.int32))


def test_cat_bad_arguments_raise(pkg, torch_dev):
    torch, dev = torch_dev
    layer = CatLayer(pkg, torch_dev, 2, 5, 5, 2, 32, 64, seed=3)
    srcs = layer.sources()
    with pytest.raises(pkg.WinoError):
        pkg.conv1x1_cat_bn(srcs[:1], layer.wt, layer.bt, layer.st)                     # one source
    with pytest.raises(pkg.WinoError):
        pkg.conv1x1_cat_bn([srcs[1], srcs[0]], layer.wt, layer.bt, layer.st)           # descending addresses
    with pytest.raises(pkg.WinoError):
        pkg.conv1x1_cat_bn(srcs, layer.wt, layer.bt[:1], layer.st)                     # one bias row for two images
    with pytest.raises(pkg.WinoError, match="rc=-3"):
        pkg.conv1x1_cat_bn(srcs, layer.wt, layer.bt, layer.st, 8)                      # ADD_RESIDUAL


# ---- the module ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ASPP_SHAPES, ids=ids)
def test_aspp_parity(shape, pkg, O, torch_dev):
    """Into a NaN-filled output through a NaN-filled workspace.  The images' means differ, and on the CPU the reference
    without the pooled branch differs from the full one by more than 1e-2 in every image: a dropped pooled bias, or
    image 0's bias for every image, cannot pass."""
    case = AsppCase(pkg, torch_dev, *shape, seed=sum(shape[:6]))
    share = case.pooled_share()
    print("pooled branch's share per image:", " ".join(f"{v:.3f}" for v in share))
    assert min(share) > 1e-2
    case.check(O, case.run())


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("shape", [(2, 5, 7, 64, 64, 64, (2, 3, 12)), (1, 4, 4, 96, 128, 64, (1, 12, 36))], ids=ids)
def test_aspp_in_the_guarded_arena(shape, align, pkg, O, torch_dev):
    torch, dev = torch_dev
    N, H, W, Cin, Cb, Kout, rates = shape
    case = AsppCase(pkg, torch_dev, *shape, seed=13 + align)
    arena = Arena(torch, dev, align)
    inp = lambda t, n: arena.input(t, name=n)
    x, w0, w_pool, w_proj = inp(case.x, "in"), inp(case.w0, "w0"), inp(case.w_pool, "w_pool"), inp(case.w_proj, "w_proj")
    taps = [inp(t, f"w{i + 1}_taps") for i, t in enumerate(case.taps)]
    bn = [(inp(b, f"bn{i}Bias"), inp(s, f"bn{i}Scale")) for i, (b, s) in enumerate(case.bn)]
    out = arena.output(N, H + 2, W + 2, Kout, name="out")
    ws = arena.workspace(case.workspace_bytes(), name="workspace")
    pkg.aspp(x, w0, bn[0], taps, bn[1:4], rates, w_pool, bn[4], w_proj, bn[5], out=out, workspace=ws)
    arena.check(f"aspp {shape} align {align}")
    case.check(O, out)


def test_aspp_replays_from_a_graph(pkg, O, torch_dev):
    """prepare reserves exactly the launches' scratch: the module captures into one graph and two replays are bitwise
    the eager result."""
    N, H, W, Cin, Cb, Kout, rates = shape = ASPP_SHAPES[1]
    case = AsppCase(pkg, torch_dev, *shape, seed=23)
    eager = graph_replay_scenario(pkg, torch_dev, case.run, lambda: pkg.aspp_prepare(N, H, W, Cin, Cb, Kout, rates),
                                  case.workspace_bytes())
    case.check(O, eager)
