"""GPU tests of the residual 3x3 layer (wino_conv3x3_bn_add_relu_hw) and the ResNet basic block (wino_basic_block_hw):
the layer against an fp64 composition at ResNet-18/34's stage shapes and in every kernel form forced, bitwise against
the plain layer with a zero residual, in place against out of place, the block against fp64 and a BasicBlock written in
plain torch, chained in place, in a graph, the fail-fast contract of the stream-K forms, and one batch that needs two
launches."""
import ctypes

import numpy as np
import pytest

import layer_refs as LR
from cases import TIGHT, BasicBlock, ResLayer
from gpu_support import dirty_ticket_scenario, graph_replay_scenario, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu

# ResNet-18/34's stages: (H, C); every 3x3 of the basic blocks there is C -> C at stride 1
STAGES = {"conv2": (56, 64), "conv3": (28, 128), "conv4": (14, 256), "conv5": (7, 512)}


@pytest.mark.parametrize("N", [1, 8, 128])
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_layer_at_the_stage_shapes(stage, N, pkg, O, torch_dev):
    """14x14 takes the fixed-geometry kernels, the others the general path (7x7: odd)."""
    H, C = STAGES[stage]
    layer = ResLayer(pkg, torch_dev, N, H, H, C, C, seed=H * 1000 + N)
    layer.check(O, layer.run(), idx=None if N < 128 else [0, 61, 127])


@pytest.mark.parametrize("shape", [(3, 14, 14, 128, 64), (2, 9, 13, 64, 128)])
def test_layer_without_relu(shape, pkg, O, torch_dev):
    N, H, W, C, K = shape
    layer = ResLayer(pkg, torch_dev, N, H, W, C, K, seed=N + H + W)
    layer.check(O, layer.run(relu=False), relu=False)


def _items(N, H, W, K):
    tiles = ((H + 1) // 2) * ((W + 1) // 2)
    return ((N * tiles + 63) // 64) * (K // 64)


def _plan(pkg, N, H, W, C, K):
    grid, rounds, it = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    tail = ctypes.c_long()
    rc = pkg.lib().wino_conv3x3_plan(N, H, W, C, K, 256, ctypes.byref(grid), ctypes.byref(rounds), ctypes.byref(tail),
                                     ctypes.byref(it))
    assert rc == 0
    return grid.value, rounds.value, tail.value


# (N, H, W, C, K): the fixed 14x14 path and the general one (odd)
FORCED = [(8, 14, 14, 256, 256), (8, 28, 28, 128, 128), (4, 7, 7, 512, 512)]


@pytest.mark.parametrize("shape", FORCED)
def test_every_throughput_form(shape, pkg, O, torch_dev, knobs):
    """WINO_3X3_ALGO=big with grids that give whole items only and a stream-K tail: each equals the plain layer's
    result plus the residual (the same plan, the same accumulation order) and the fp64 composition."""
    torch, dev = torch_dev
    N, H, W, C, K = shape
    layer = ResLayer(pkg, torch_dev, N, H, W, C, K, seed=sum(shape))
    items = _items(N, H, W, K)
    knobs.set("WINO_3X3_ALGO", "big")
    seen = set()
    for G in (items, items // 2 if items % 2 == 0 else items, items - 3, 13):
        knobs.set("WINO_SK_GRID", G)
        grid, rounds, tail = _plan(pkg, N, H, W, C, K)
        assert grid == G
        seen.add(tail > 0)
        got = layer.run()
        layer.check(O, got)
        assert torch.equal(layer.run(), got)   # reproducible from launch to launch
    assert seen == {False, True}


@pytest.mark.parametrize("shape", [(1, 14, 14, 256, 256), (2, 7, 7, 512, 512), (1, 28, 28, 128, 128)])
@pytest.mark.parametrize("ct", [1, 2, 4])
def test_every_latency_form(shape, ct, pkg, O, torch_dev, knobs):
    """WINO_3X3_ALGO=small at every block width, without and with the split-C reduction (S > 1)."""
    torch, dev = torch_dev
    N, H, W, C, K = shape
    layer = ResLayer(pkg, torch_dev, N, H, W, C, K, seed=ct * 7 + sum(shape))
    knobs.set("WINO_3X3_ALGO", "small")
    knobs.set("WINO_SMALL_CT", ct)
    for split in (1, 2, 4):
        knobs.set("WINO_SMALL_SPLIT", split)
        use, _, sp, gct, _ = pkg.small_plan_3x3_full(N, C, K, H=H, W=W)
        assert (use, sp, gct) == (1, split, ct)
        got = layer.run()
        layer.check(O, got)
        assert torch.equal(layer.run(), got)


@pytest.mark.parametrize("algo", ["big", "small", None])
@pytest.mark.parametrize("shape", [(8, 14, 14, 256, 256), (2, 7, 7, 512, 512)])
def test_zero_residual_is_the_plain_layer_bitwise(shape, algo, pkg, torch_dev, knobs):
    torch, dev = torch_dev
    N, H, W, C, K = shape
    layer = ResLayer(pkg, torch_dev, N, H, W, C, K, seed=3 + N)
    if algo:
        knobs.set("WINO_3X3_ALGO", algo)
    if algo == "big":
        knobs.set("WINO_SK_GRID", _items(N, H, W, K) - 3)   # with a tail
    if algo == "small":
        knobs.set("WINO_SMALL_SPLIT", 2)
    zero = torch.zeros_like(layer.rt)
    for relu in (True, False):
        plain = pkg.conv3x3_bn_relu(layer.xt, layer.U, layer.bt, layer.st, relu=relu)
        assert torch.equal(layer.run(relu=relu, res=zero), plain)


@pytest.mark.parametrize("algo", ["big", "small", None])
@pytest.mark.parametrize("shape", [(8, 14, 14, 256, 256), (3, 7, 7, 512, 512), (2, 28, 28, 128, 128)])
def test_in_place_equals_out_of_place(shape, algo, pkg, O, torch_dev, knobs):
    torch, dev = torch_dev
    N, H, W, C, K = shape
    layer = ResLayer(pkg, torch_dev, N, H, W, C, K, seed=11 + N)
    if algo:
        knobs.set("WINO_3X3_ALGO", algo)
    if algo == "big":
        knobs.set("WINO_SK_GRID", _items(N, H, W, K) - 3)
    if algo == "small":
        knobs.set("WINO_SMALL_SPLIT", 2)
    ref = layer.run()
    buf = layer.rt.clone()
    got = layer.run(res=buf, out=buf)
    assert got.data_ptr() == buf.data_ptr()
    assert torch.equal(got, ref)
    layer.check(O, got)


@pytest.mark.parametrize("N", [1, 8])
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_block_at_the_stage_shapes(stage, N, pkg, O, torch_dev):
    H, C = STAGES[stage]
    blk = BasicBlock(pkg, torch_dev, N, H, H, C, seed=500 + H + N)
    blk.check(O, blk.run())


def _basic_block_module(torch, C):
    """torchvision's BasicBlock (identity shortcut), written out in plain torch."""
    nn = torch.nn

    class BasicBlock(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1 = nn.Conv2d(C, C, 3, padding=1, bias=False)
            self.bn1 = nn.BatchNorm2d(C)
            self.conv2 = nn.Conv2d(C, C, 3, padding=1, bias=False)
            self.bn2 = nn.BatchNorm2d(C)
            self.relu = nn.ReLU(inplace=True)

        def forward(self, x):
            out = self.relu(self.bn1(self.conv1(x)))
            out = self.bn2(self.conv2(out))
            return self.relu(out + x)

    return BasicBlock()


@pytest.mark.parametrize("stage,N", [("conv3", 2), ("conv5", 3)])
def test_torchvision_style_weights(stage, N, pkg, O, torch_dev):
    torch, dev = torch_dev
    H, C = STAGES[stage]
    torch.manual_seed(18 + N)
    m = _basic_block_module(torch, C)
    for bn in (m.bn1, m.bn2):
        bn.weight.data = torch.rand(C) + 0.5
        bn.bias.data = torch.rand(C) - 0.5
        bn.running_mean.data = (torch.rand(C) - 0.5) * 0.2
        bn.running_var.data = torch.rand(C) * 0.5 + 0.5
    m.eval()

    def fold(bn):
        scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        return (bn.bias - bn.running_mean * scale).detach(), scale.detach()

    with torch.no_grad():
        x = torch.rand(N, C, H, H) - 0.5
        want = m.double()(x.double()).permute(0, 2, 3, 1).numpy()
        m.float()
        to = lambda a: a.float().contiguous().to(dev)
        xp = torch.zeros(N, H + 2, H + 2, C)
        xp[:, 1:-1, 1:-1, :] = x.permute(0, 2, 3, 1)
        bn1, bn2 = ([to(v) for v in fold(b)] for b in (m.bn1, m.bn2))
        got = pkg.basic_block(to(xp), pkg.filter_transform_f2(to(m.conv1.weight)), bn1,
                              pkg.filter_transform_f2(to(m.conv2.weight)), bn2)
    g = got.cpu().numpy()[:, 1:-1, 1:-1, :]
    assert g.shape == want.shape
    assert O.rel_error(g, want) < TIGHT
    assert (want > 0).mean() > 0.2


@pytest.mark.parametrize("stage,N", [("conv4", 8), ("conv2", 1), ("conv5", 2)])
def test_two_blocks_chained_in_place(stage, N, pkg, O, torch_dev):
    """out fed forward as the next block's x, in place: one activation tensor and one workspace for the chain."""
    torch, dev = torch_dev
    H, C = STAGES[stage]
    blk = BasicBlock(pkg, torch_dev, N, H, H, C, seed=77 + N)
    x = blk.xt.clone()
    ws = torch.empty(pkg.lib().wino_basic_block_workspace_bytes_hw(N, H, H, C) // 4, device=dev)
    for _ in range(2):
        assert blk.run(x=x, out=x, workspace=ws).data_ptr() == x.data_ptr()
    blk.check(O, x, blocks=2)
    # the same chain out of place, bit for bit
    y1 = blk.run()
    assert torch.equal(blk.run(x=y1), x)


@pytest.mark.parametrize("stage,N", [("conv4", 32), ("conv3", 1)])
def test_block_in_a_graph(stage, N, pkg, O, torch_dev):
    """The two launches captured into one graph (one stream) after basic_block_prepare: the replay equals eager."""
    torch, dev = torch_dev
    H, C = STAGES[stage]
    blk = BasicBlock(pkg, torch_dev, N, H, H, C, seed=909 + N)
    eager = graph_replay_scenario(pkg, torch_dev, blk.run, lambda: pkg.basic_block_prepare(N, H, H, C),
                                  pkg.lib().wino_basic_block_workspace_bytes_hw(N, H, H, C))
    if N <= 8:
        blk.check(O, eager)


@pytest.mark.parametrize("form", ["tail", "split"])
def test_a_dirty_ticket_counter_is_reported_and_reset_recovers(form, pkg, O, torch_dev, knobs):
    """Both stream-K forms of the residual layer keep the fail-fast contract: a ticket counter left non-zero is
    reported, every launch on the stream then fails with WINO_E_STATE, and wino_stream_reset_scratch() recovers
    bitwise results."""
    torch, dev = torch_dev
    if form == "tail":
        N, H, W, C, K = 8, 14, 14, 256, 256
        knobs.set("WINO_3X3_ALGO", "big")
        knobs.set("WINO_SK_GRID", _items(N, H, W, K) - 3)
        assert _plan(pkg, N, H, W, C, K)[2] > 0
        n_tickets = _items(N, H, W, K) * 8
    else:
        N, H, W, C, K = 1, 14, 14, 256, 256
        knobs.set("WINO_3X3_ALGO", "small")
        knobs.set("WINO_SMALL_CT", 1)
        knobs.set("WINO_SMALL_SPLIT", 4)
        use, _, sp, ct, wgs = pkg.small_plan_3x3_full(N, C, K, H=H, W=W)
        assert use == 1 and sp == 4
        n_tickets = wgs // sp
    layer = ResLayer(pkg, torch_dev, N, H, W, C, K, seed=99)
    dirty_ticket_scenario(pkg, torch, layer.run, n_tickets, check=lambda ref: layer.check(O, ref))


def test_batch_split_across_two_launches(pkg, O, torch_dev):
    """56x56x64 at N = 5100: the padded tensors pass 4 GiB, so the batch goes out as two launches (the first of 4928
    images); the residual advances with out.  In place, to fit in less memory; checked on both sides of the cut."""
    torch, dev = torch_dev
    N, H, C = 5100, 56, 64
    if torch.cuda.mem_get_info()[0] < 12 * (1 << 30):
        pytest.skip("needs 12 GiB of free device memory")
    g = torch.Generator(device=dev).manual_seed(5100)
    x = torch.zeros(N, H + 2, H + 2, C, device=dev)
    x[:, 1:-1, 1:-1, :] = torch.rand(N, H, H, C, device=dev, generator=g) - 0.5
    res = torch.zeros_like(x)
    res[:, 1:-1, 1:-1, :] = torch.rand(N, H, H, C, device=dev, generator=g) - 0.5
    w = (torch.rand(C, C, 3, 3, device=dev, generator=g) - 0.5) / np.sqrt(9 * C) * 4
    b = torch.rand(C, device=dev, generator=g) - 0.5
    s = torch.rand(C, device=dev, generator=g) + 0.5
    idx = [0, 4927, 4928, 5099]
    xs, rs = x[idx].cpu(), res[idx].cpu()
    got = pkg.conv3x3_bn_add_relu(x, pkg.filter_transform_f2(w), b, s, res, out=res)
    assert got.data_ptr() == res.data_ptr()
    g_idx = got[idx].cpu().numpy()
    del x, res, got
    torch.cuda.empty_cache()
    want = LR.conv3x3(LR.interior(xs), w, (b, s), True, residual=LR.interior(rs)).numpy()
    assert O.rel_error(g_idx[:, 1:-1, 1:-1, :], want) < TIGHT
    assert (g_idx[:, 0, :, :] == 0).all() and (g_idx[:, -1, :, :] == 0).all()
    assert pkg.tickets_in_use() == 0


def test_bad_arguments_raise(pkg, torch_dev):
    torch, dev = torch_dev
    layer = ResLayer(pkg, torch_dev, 1, 14, 14, 64, 128, seed=5)
    with pytest.raises(pkg.WinoError):
        layer.run(res=torch.zeros(1, 16, 16, 64, device=dev))            # residual with C channels, not K
    square = ResLayer(pkg, torch_dev, 1, 14, 14, 128, 128, seed=7)
    with pytest.raises(pkg.WinoError, match="rc=-3"):
        square.run(res=square.xt)                                        # the residual is the input
    blk = BasicBlock(pkg, torch_dev, 1, 14, 14, 64, seed=6)
    with pytest.raises(pkg.WinoError):
        blk.run(workspace=torch.empty(16, device=dev))                   # workspace too small
    with pytest.raises(pkg.WinoError, match="rc=-3"):
        ws = torch.empty(pkg.lib().wino_basic_block_workspace_bytes_hw(1, 14, 14, 64) // 4, device=dev)
        blk.run(out=ws.view(1, 16, 16, 64), workspace=ws)                # out is the workspace
