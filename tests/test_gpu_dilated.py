"""GPU tests of the dilated 3x3 layer, wino_conv3x3_dilated_bn_relu_hw (the tiled 1x1 GEMM kernel in operand form
A_DIL: K = 9C, per-lane and per-tap A offsets over a padded input with a ring of width one), and of the two dilated
bottleneck blocks.  Against the fp64 reference of tests/dilated_cases.py, into NaN-filled outputs, at cases.TIGHT:
parity, the forced forms with the stream-K fail-fast contract, the guarded arena, and the non-finite footprint."""
import pytest

from cases import TIGHT
from dilated_cases import (FORM_SHAPES, FORMS, LAYER_SHAPES, PROJ_BLOCK, RESIDUAL_BLOCK, DilBlock, DilLayer,
                           footprint)
from gpu_support import dirty_ticket_scenario, graph_replay_scenario, torch_dev  # noqa: F401
from guarded import ALIGNS, Arena

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", LAYER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layer_parity(shape, pkg, O, torch_dev):
    N, H, W, C, K, d = shape
    layer = DilLayer(pkg, torch_dev, *shape, seed=sum(shape))
    layer.check(O, layer.run())
    layer.check(O, layer.run(relu=False), relu=False)
    assert pkg.tickets_in_use() == 0
    if d == 1:   # the plain 3x3: also against the comparator kernel
        full = pkg.conv3x3_direct(layer.xt, layer.wt, layer.bt, layer.st, True)
        got = layer.run()
        assert O.rel_error(got[:, 1:-1, 1:-1, :].cpu().numpy(), full[:, 1:-1, 1:-1, :].cpu().numpy()) < TIGHT


@pytest.mark.parametrize("form,shape", [(f, s) for s in FORM_SHAPES for f in sorted(FORMS)])
def test_forced_forms(form, shape, pkg, O, torch_dev, knobs):
    """Whole tiles and stream-K, grids that cut segments mid-tap included: against the reference, bitwise equal from
    launch to launch, no ticket left."""
    torch, _ = torch_dev
    for k, v in FORMS[form].items():
        knobs.set(k, v)
    assert pkg.conv3x3_dilated_plan(*shape) == (pkg.FORM_TILED if form == "tiled" else pkg.FORM_STREAM_K)
    layer = DilLayer(pkg, torch_dev, *shape, seed=sum(shape))
    a = layer.run().clone()
    layer.check(O, a)
    assert torch.equal(layer.run(), a)
    assert pkg.tickets_in_use() == 0


def test_a_dirty_ticket_counter_is_reported_and_reset_recovers(pkg, O, torch_dev, knobs):
    torch, dev = torch_dev
    knobs.set("WINO_1X1_ALGO", "big")
    knobs.set("WINO_1X1_SK", 1)
    shape = FORM_SHAPES[0]
    N, H, W, C, K, d = shape
    layer = DilLayer(pkg, torch_dev, *shape, seed=99)
    assert pkg.conv3x3_dilated_plan(*shape) == pkg.FORM_STREAM_K
    n_tickets = ((N * H * W + 111) // 112) * (K // 128)   # row tiles x column blocks
    dirty_ticket_scenario(pkg, torch, layer.run, n_tickets, check=lambda ref: layer.check(O, ref))


# ---- the guarded arena -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("shape", [(2, 5, 7, 64, 64, 2), (1, 9, 9, 32, 128, 12), (3, 4, 4, 96, 64, 2)],
                         ids=lambda s: "x".join(map(str, s)))
def test_layer_in_the_guarded_arena(shape, align, pkg, O, torch_dev):
    """NaN directly before and behind every operand, sentinel guards around the output: no guard byte changes, and no
    NaN behind an input reaches the result (the first and the last tile's windows are clipped to the tensor)."""
    torch, dev = torch_dev
    N, H, W, C, K, d = shape
    layer = DilLayer(pkg, torch_dev, *shape, seed=7 + align)
    arena = Arena(torch, dev, align)
    x, taps = arena.input(layer.x, name="in"), arena.input(layer.taps, name="w_taps")
    b, s = arena.input(layer.bias, name="bnBias"), arena.input(layer.scale, name="bnScale")
    out = arena.output(N, H + 2, W + 2, K, name="out")
    pkg.conv3x3_dilated_bn_relu(x, taps, b, s, d, relu=True, out=out)
    arena.check(f"dilated layer {shape} align {align}")
    layer.check(O, out)


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("d", [2, 12])
@pytest.mark.parametrize("proj", [False, True], ids=["residual", "proj"])
def test_blocks_in_the_guarded_arena(proj, d, align, pkg, O, torch_dev):
    torch, dev = torch_dev
    N, H, W, Cin, Cm, C4 = (2, 5, 7, 64, 64, 128) if proj else (2, 5, 7, 128, 64, 128)
    blk = DilBlock(pkg, torch_dev, N, H, W, Cin, Cm, C4, d, proj, seed=11 * d + align)
    arena = Arena(torch, dev, align)
    inp = lambda t, n: arena.input(t, name=n)
    x, w1, taps = inp(blk.x, "x"), inp(blk.w1, "w1"), inp(blk.taps, "w2_taps")
    bn = [(inp(bb, f"bn{i + 1}Bias"), inp(ss, f"bn{i + 1}Scale")) for i, (bb, ss) in enumerate(blk.bn[:3])]
    out = arena.output(N, H, W, C4, name="out")
    if proj:
        ws = arena.workspace(blk.workspace_bytes(), name="workspace", query="wino_proj_block_workspace_bytes_hw")
        pkg.dilated_proj_block(x, w1, bn[0], taps, bn[1], inp(blk.tail, "tail"), d, out=out, workspace=ws)
    else:
        ws = arena.workspace(blk.workspace_bytes(), name="workspace", query="wino_residual_block_workspace_bytes_hw")
        pkg.dilated_residual_block(x, w1, bn[0], taps, bn[1], inp(blk.w3, "w3"), bn[2], d, out=out, workspace=ws)
    arena.check(f"dilated block proj={proj} d={d} align {align}")
    blk.check(O, out)


# ---- non-finite values -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value,relu", [(float("nan"), True), (float("nan"), False), (float("inf"), False)],
                         ids=["nan-relu", "nan", "inf"])
@pytest.mark.parametrize("shape", [(2, 9, 9, 64, 128, 2), (2, 7, 7, 64, 64, 4)], ids=lambda s: "x".join(map(str, s)))
def test_one_nonfinite_input_reaches_exactly_its_footprint(shape, value, relu, pkg, torch_dev):
    """a NaN (an Inf) at one input element reaches the at most nine output pixels at offsets
    d * {-1, 0, 1}^2, in every output channel; every other bit of the output is that of the clean run, the ring stays
    zero and the second image is untouched."""
    torch, dev = torch_dev
    N, H, W, C, K, d = shape
    layer = DilLayer(pkg, torch_dev, *shape, seed=5)
    clean = layer.run(relu=relu).clone()
    assert bool(torch.isfinite(clean).all())
    for y, x in ((H // 2, W // 2), (0, W // 2), (H - 1, 0)):   # interior, edge, corner
        xt = layer.xt.clone()
        xt[0, 1 + y, 1 + x, C // 3] = value
        got = layer.run(relu=relu, x=xt)
        m = torch.from_numpy(footprint(H, W, y, x, d)).to(dev)
        assert 1 <= int(m.sum()) <= 9
        bad = ~torch.isfinite(got)
        want_bad = torch.zeros_like(bad)
        want_bad[0, 1:-1, 1:-1, :] = m[:, :, None]
        assert torch.equal(bad, want_bad), (y, x)
        if value != value:
            assert bool(torch.isnan(got[bad]).all())
        assert torch.equal(got[~bad].view(torch.int32), clean[~bad].view(torch.int32))
        assert torch.equal(got[1].view(torch.int32), clean[1].view(torch.int32))


# ---- the blocks ----------------------------------------------------------------------------------------------------------
def test_dilated_residual_block(pkg, O, torch_dev):
    blk = DilBlock(pkg, torch_dev, *RESIDUAL_BLOCK, proj=False, seed=21)
    blk.check(O, blk.run())


def test_dilated_proj_block(pkg, O, torch_dev):
    blk = DilBlock(pkg, torch_dev, *PROJ_BLOCK, proj=True, seed=22)
    blk.check(O, blk.run())


@pytest.mark.parametrize("proj", [False, True], ids=["residual", "proj"])
def test_blocks_replay_from_a_graph(proj, pkg, O, torch_dev):
    """prepare reserves exactly the launches' scratch: the block captures into one graph and replays bitwise."""
    case = PROJ_BLOCK if proj else RESIDUAL_BLOCK
    blk = DilBlock(pkg, torch_dev, *case, proj=proj, seed=23)
    N, H, W, Cin, Cm, C4, d = case
    if proj:
        prepare = lambda: pkg.dilated_proj_block_prepare(N, H, W, Cin, Cm, C4, d)
    else:
        prepare = lambda: pkg.dilated_residual_block_prepare(N, H, W, C4, Cm, d)
    eager = graph_replay_scenario(pkg, torch_dev, blk.run, prepare, blk.workspace_bytes())
    blk.check(O, eager)


def test_bad_arguments_raise(pkg, torch_dev):
    torch, dev = torch_dev
    layer = DilLayer(pkg, torch_dev, 1, 7, 7, 64, 128, 2, seed=3)
    with pytest.raises(pkg.WinoError):
        pkg.conv3x3_dilated_bn_relu(layer.xt, layer.wt, layer.bt, layer.st, 2)               # [K][C][3][3], not packed
    with pytest.raises(pkg.WinoError):
        pkg.conv3x3_dilated_bn_relu(layer.x, layer.taps, layer.bt, layer.st, 2)              # CPU input
    with pytest.raises(pkg.WinoError, match="rc=-2"):
        pkg.conv3x3_dilated_bn_relu(layer.xt, layer.taps, layer.bt, layer.st, 0)
    with pytest.raises(pkg.WinoError, match="rc=-3"):                                        # in place
        pkg.conv3x3_dilated_bn_relu(layer.xt, pkg.filter_pack_s2(layer.wt[:64]), layer.bt[:64], layer.st[:64], 2,
                                    out=layer.xt)
