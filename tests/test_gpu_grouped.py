"""GPU tests of the grouped 3x3 layer (wino_conv3x3_grouped_bn_relu_hw), the two ResNeXt blocks built on it and the
ResNeXt / Wide-ResNet networks.

The oracle is layer_refs.conv3x3(..., groups=G), fp64 on the CPU with BN and the ReLU applied in fp64; an fp32 CPU grouped
conv sits at 2-4e-7 from it at these shapes, and the bar is the project's layer bar, max |diff| / max |want| < 2e-5.
Every layer and block tensor lives on a guarded arena (tests/guarded.py) at both placements of guarded.ALIGNS, and
arena.check runs after every case: no guard word written, every input equal to its master bit for bit."""
import pytest

import guarded
import layer_refs as LR
from gpu_support import R, network_graph_scenario, rel, torch_dev  # noqa: F401
from reference_nets import NET_TOL, check_net, random_state_dict, reference_forward

pytestmark = pytest.mark.gpu

TIGHT = 2e-5
CGS = (4, 8, 16, 32, 64)
MAPS = ((1, 1), (2, 3), (7, 5), (9, 8))       # 9 x 8: stride 2 clips an odd and an even edge


# ---------------------------------------------------------------------------------------------------- the layer
def _layer_inputs(torch, N, Hin, Win, C, Cg, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(N, Hin + 2, Win + 2, C)
    x[:, 1:-1, 1:-1, :] = torch.rand(N, Hin, Win, C, generator=g) - 0.5
    w = (torch.rand(C, Cg, 3, 3, generator=g) - 0.5) * (4.0 / (9 * Cg) ** 0.5)
    bias = torch.rand(C, generator=g) - 0.5
    sign = (torch.rand(C, generator=g) < 0.5).float() * 2 - 1          # BN scales of both signs
    scale = (torch.rand(C, generator=g) + 0.5) * sign
    return x, w, bias, scale


def _run_layer(pkg, torch_dev, x, w, bias, scale, groups, stride, relu, align, tag):
    """The layer on a guarded arena: (out interior, on the CPU); the ring is checked to be exactly 0 here."""
    torch, dev = torch_dev
    N, Hin, Win, C = x.shape[0], x.shape[1] - 2, x.shape[2] - 2, x.shape[3]
    H, W = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    packed = pkg.filter_pack_grouped(w.to(dev), groups)
    assert packed.numel() == pkg.lib().wino_conv3x3_grouped_filter_elems(C, groups)
    arena = guarded.Arena(torch, dev, align)
    xin, pk = arena.input(x, name="in"), arena.input(packed, name="packed")
    b, s = arena.input(bias, name="bias"), arena.input(scale, name="scale")
    out = arena.output(N, H + 2, W + 2, C, name="out")
    got = pkg.conv3x3_grouped_bn_relu(xin, pk, b, s, groups, stride=stride, relu=relu, out=out)
    assert got.data_ptr() == out.data_ptr()
    arena.check(tag)
    o = out.cpu()
    ring = o.clone()
    ring[:, 1:-1, 1:-1, :] = 0
    assert torch.equal(ring, torch.zeros_like(ring)), f"{tag}: ring not 0"     # (a NaN left in the ring fails too)
    return o[:, 1:-1, 1:-1, :]


def _layer_case(pkg, torch_dev, N, Hin, Win, C, Cg, stride, relu, align):
    torch, _ = torch_dev
    tag = f"grouped N={N} {Hin}x{Win} C={C} Cg={Cg} s={stride} relu={relu} align={align}"
    x, w, bias, scale = _layer_inputs(torch, N, Hin, Win, C, Cg, seed=1000 * Hin + 10 * Win + Cg + stride)
    got = _run_layer(pkg, torch_dev, x, w, bias, scale, C // Cg, stride, relu, align, tag)
    want = LR.conv3x3(LR.interior(x), w, (bias, scale), relu, stride=stride, groups=C // Cg)
    err = rel(torch, got, want)
    assert err < TIGHT, (tag, err)
    return want


@pytest.mark.parametrize("C", [64, 128])      # two channel blocks catch a wrong block base
@pytest.mark.parametrize("Cg", CGS)
def test_layer_matches_fp64(Cg, C, pkg, torch_dev):
    saw_negative = False
    for align in guarded.ALIGNS:
        for stride in (1, 2):
            for Hin, Win in MAPS:
                for N, relu in ((1, True), (3, False), (1, False), (3, True)):
                    want = _layer_case(pkg, torch_dev, N, Hin, Win, C, Cg, stride, relu, align)
                    saw_negative |= bool((want < 0).any())
    assert saw_negative      # relu off really left negative outputs to compare


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("Cg", [4, 64])
def test_layer_past_one_tile_in_every_direction(Cg, stride, pkg, torch_dev):
    """N = 3, 29 x 23, C = 192: several tiles down and across (clipped last ones), three channel blocks, three images."""
    for align in guarded.ALIGNS:
        _layer_case(pkg, torch_dev, 3, 29, 23, 192, Cg, stride, True, align)


# the smallest maps with two tiles down and across and clipped last tiles, by (stride, tile width): (Hin, Win)
TWO_TILE_MAPS = {(1, 16): (5, 25), (1, 8): (9, 17), (2, 16): (5, 49), (2, 8): (9, 33)}


@pytest.mark.parametrize("KC", [16, 32, 64])
@pytest.mark.parametrize("TW", [8, 16])
@pytest.mark.parametrize("stride", [1, 2])
def test_every_instantiation_past_one_tile(stride, TW, KC, pkg, torch_dev):
    """Each conv3x3_grouped_kernel<stride, TW, KC> by name, N = 2, C = 128 (two channel blocks): the plan query says that
    the shape takes it, with at least two tiles down and across and both last tiles clipped.  KC = 16 serves Cg = 4, 8
    and 16, each with a select of its own."""
    Hin, Win = TWO_TILE_MAPS[(stride, TW)]
    H, W = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    tile_h = (4 if stride == 1 else 2) * 16 // TW
    for i, Cg in enumerate((4, 8, 16) if KC == 16 else (KC,)):
        tw, kc, tiles_y, tiles_x = pkg.conv3x3_grouped_plan(2, Hin, Win, 128, 128 // Cg, stride)
        assert (tw, kc) == (TW, KC) and tiles_y >= 2 and tiles_x >= 2, (tw, kc, tiles_y, tiles_x)
        assert tiles_y == -(-H // tile_h) and H % tile_h and W % TW
        for j, align in enumerate(guarded.ALIGNS):
            _layer_case(pkg, torch_dev, 2, Hin, Win, 128, Cg, stride, bool((i + j) % 2), align)


# (Hin, Win) by stride: 8-wide tiles at both strides, 16-wide tiles at both
ONE_HOT_MAPS = {8: {1: (7, 5), 2: (7, 5)}, 16: {1: (6, 12), 2: (5, 20)}}


@pytest.mark.parametrize("Cg", CGS)
def test_one_hot_weights_do_not_leak_across_groups(Cg, pkg, torch_dev):
    """One non-zero tap from one input channel of one group: every output channel outside that group is exactly
    act(bias) -- a filter value packed off the block diagonal, or a column tile contracting over a neighbour's
    channels, shows here, where random weights would hide it below the tolerance.  In the 8-wide and in the 16-wide
    instantiations of both strides."""
    for tw, maps in ONE_HOT_MAPS.items():
        _one_hot(pkg, torch_dev, Cg, tw, maps)


def _one_hot(pkg, torch_dev, Cg, tw, maps):
    torch, _ = torch_dev
    C, N = 128, 2
    groups = C // Cg
    inputs = {stride: _layer_inputs(torch, N, *maps[stride], C, Cg, seed=77 + Cg) for stride in (1, 2)}
    for i, (grp, cl, tap) in enumerate(((0, 0, 4), (groups - 1, Cg - 1, 0), (groups // 2, Cg // 2, 8), (1 % groups, 1, 5))):
        for stride, relu in ((1, False), (2, True)):
            x, _, bias, scale = inputs[stride]
            assert pkg.conv3x3_grouped_plan(N, *maps[stride], C, groups, stride)[0] == tw
            w = torch.zeros(C, Cg, 3, 3)
            w[grp * Cg:(grp + 1) * Cg, cl, tap // 3, tap % 3] = torch.arange(1, Cg + 1, dtype=torch.float32) / Cg
            tag = f"one-hot Cg={Cg} TW={tw} group={grp} channel={cl} tap={tap} s={stride}"
            got = _run_layer(pkg, torch_dev, x, w, bias, scale, groups, stride, relu, guarded.ALIGNS[i % 2], tag)
            want = LR.conv3x3(LR.interior(x), w, (bias, scale), relu, stride=stride, groups=groups)
            inside = torch.zeros(C, dtype=torch.bool)
            inside[grp * Cg:(grp + 1) * Cg] = True
            act = torch.relu(bias) if relu else bias
            assert torch.equal(got[..., ~inside], act[~inside].expand_as(got[..., ~inside])), tag
            assert rel(torch, got[..., inside], want[..., inside]) < TIGHT, tag
            assert float((want[..., inside] - act[inside].double()).abs().max()) > 0.05, tag   # the tap does something


def test_bad_arguments_raise(pkg, torch_dev):
    torch, dev = torch_dev
    x, w, bias, scale = (t.to(dev) for t in _layer_inputs(torch, 1, 7, 5, 128, 4, seed=3))
    packed = pkg.filter_pack_grouped(w, 32)
    # packed for another group count.  (Cg = 4, 8 and 16 all pack to 9 * C * 16 floats -- a column tile is 16 wide --
    # so the size tells those apart from Cg = 32 and 64 only: the buffer is opaque and carries no group count.)
    with pytest.raises(pkg.WinoError):
        pkg.conv3x3_grouped_bn_relu(x, packed, bias, scale, 4)
    with pytest.raises(pkg.WinoError):
        pkg.conv3x3_grouped_bn_relu(x, packed[:-4], bias, scale, 32)         # a short buffer
    with pytest.raises(pkg.WinoError):
        pkg.conv3x3_grouped_bn_relu(x, packed, bias, scale, 32, stride=3)
    with pytest.raises(pkg.WinoError):
        pkg.conv3x3_grouped_bn_relu(x, packed, bias, scale, 32, out=torch.empty(1, 9, 7, 64, device=dev))
    with pytest.raises(pkg.WinoError):
        pkg.filter_pack_grouped(torch.zeros(128, 2, 3, 3, device=dev), 64)    # Cg = 2
    with pytest.raises(pkg.WinoError, match="rc=-3"):
        pkg.conv3x3_grouped_bn_relu(x, packed, bias, scale, 32, out=x)        # in place
    # the blocks: one BN vector of the wrong length each (the kernels would read past its end)
    z = lambda *s: torch.zeros(*s, device=dev)
    bn, bn3 = (z(128), z(128)), (z(256), z(256))
    with pytest.raises(pkg.WinoError, match="bn1 / bn2 vectors must have Cm values, bn3's C4"):
        pkg.grouped_residual_block(z(1, 7, 5, 256), z(256, 128), bn, packed, bn, z(128, 256), (z(256), z(128)), 32)
    with pytest.raises(pkg.WinoError, match="bn1 / bn2 vectors must have Cm values"):
        pkg.grouped_proj_block(z(1, 7, 5, 64), z(64, 128), bn, packed, (z(64), z(128)), z((128 + 64 + 2) * 256), 32, 2)


# ---------------------------------------------------------------------------------------------------- the blocks
CIN, CM, C4, GROUPS = 64, 128, 256, 32


class _Blocks:
    """The tensors of one identity and one projection block (folded BN vectors, NHWC activations) and their fp64
    references."""

    def __init__(self, torch, N, Hin, Win, seed):
        g = torch.Generator().manual_seed(seed)
        r = lambda *s: torch.rand(*s, generator=g) - 0.5
        self.N, self.Hin, self.Win = N, Hin, Win
        self.x_res = r(N, Hin, Win, C4)
        self.x_proj = r(N, Hin, Win, CIN)
        self.w1_res = r(C4, CM) / C4 ** 0.5 * 4
        self.w1_proj = r(CIN, CM) / CIN ** 0.5 * 4
        self.wg = r(CM, CM // GROUPS, 3, 3) / (9 * CM // GROUPS) ** 0.5 * 4
        self.w3 = r(CM, C4) / CM ** 0.5 * 4
        self.wp = r(CIN, C4) / CIN ** 0.5 * 2
        self.bn = [(r(c), r(c) + 1.0) for c in (CM, CM, C4, C4)]     # (bias, scale): bn1, bn2, bn3, bnp

    def reference_residual(self):
        bn = self.bn
        return LR.bottleneck(self.x_res, self.w1_res, bn[0], self.wg, bn[1], self.w3, bn[2], groups=GROUPS)

    def reference_proj(self, stride):
        bn = self.bn
        return LR.bottleneck(self.x_proj, self.w1_proj, bn[0], self.wg, bn[1], self.w3, bn[2], self.wp, bn[3],
                             stride=stride, stride_on="3x3", groups=GROUPS)


def _run_blocks(pkg, torch_dev, blk, stride, align, tag):
    """Both blocks on one arena, the workspaces exactly the reported sizes between sentinel guards."""
    torch, dev = torch_dev
    L = pkg.lib()
    N, Hin, Win = blk.N, blk.Hin, blk.Win
    H, W = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    arena = guarded.Arena(torch, dev, align)
    a = lambda t, name: arena.input(t, name=name)
    bn = [(a(b, f"bn{i}b"), a(s, f"bn{i}s")) for i, (b, s) in enumerate(blk.bn)]
    wg = a(pkg.filter_pack_grouped(blk.wg.to(dev), GROUPS), "wg")
    out = {}
    # identity block (always stride 1, at Hin x Win)
    x, w1, w3 = a(blk.x_res, "x_res"), a(blk.w1_res, "w1_res"), a(blk.w3, "w3")
    need = L.wino_residual_block_workspace_bytes_hw(N, Hin, Win, CM)
    ws = arena.workspace(need, name="ws_res")
    assert ws.numel() * 4 == need
    o = arena.output(N, Hin, Win, C4, name="out_res")
    pkg.grouped_residual_block(x, w1, bn[0], wg, bn[1], w3, bn[2], GROUPS, out=o, workspace=ws)
    out["residual"] = o
    # projection block
    xp, w1p = a(blk.x_proj, "x_proj"), a(blk.w1_proj, "w1_proj")
    tail = a(pkg.proj_tail_pack(w3, bn[2], blk.wp.to(dev), bn[3]), "tail")
    need = (L.wino_proj_block_workspace_bytes_hw(N, H, W, CM) if stride == 1
            else L.wino_proj_block_v15_workspace_bytes_hw(N, Hin, Win, CM))
    assert need == pkg.grouped_proj_block_workspace_bytes(N, Hin, Win, CM, stride)
    wsp = arena.workspace(need, name="ws_proj")
    assert wsp.numel() * 4 == need
    op = arena.output(N, H, W, C4, name="out_proj")
    pkg.grouped_proj_block(xp, w1p, bn[0], wg, bn[1], tail, GROUPS, stride, out=op, workspace=wsp)
    out["proj"] = op
    arena.check(tag)
    assert pkg.tickets_in_use() == 0
    # a workspace one byte smaller is refused (WINO_E_ARG) before anything is launched
    for short, call in ((ws, "wino_grouped_residual_block_hw"), (wsp, "wino_grouped_proj_block_hw")):
        args = ((x, w1, bn[0][0], bn[0][1], wg, bn[1][0], bn[1][1], w3, bn[2][0], bn[2][1], o) if short is ws else
                (xp, w1p, bn[0][0], bn[0][1], wg, bn[1][0], bn[1][1], tail, op))
        dims = (N, Hin, Win, C4, CM, GROUPS) if short is ws else (N, Hin, Win, CIN, CM, C4, GROUPS, stride)
        rc = getattr(L, call)(*[t.data_ptr() for t in args], *dims, short.data_ptr(), short.numel() * 4 - 1,
                              torch.cuda.current_stream().cuda_stream)
        assert rc == -3, (call, rc)
    arena.check(tag + " (short workspace)")
    return {k: v.cpu() for k, v in out.items()}


BLOCK_CASES = [(7, 9, 1), (2, 3, 1), (9, 8, 2), (3, 2, 2)]   # (Hin, Win, the projection block's stride)


@pytest.mark.parametrize("forced", [False, True], ids=["planned", "stream_k"])
@pytest.mark.parametrize("Hin,Win,stride", BLOCK_CASES)
def test_blocks_match_fp64(Hin, Win, stride, forced, pkg, knobs, torch_dev):
    """Cin 64 -> Cm 128 -> C4 256, groups 32, N = 2; `forced`: the 1x1 launches in the tiled kernel's stream-K form."""
    torch, _ = torch_dev
    if forced:
        knobs.set("WINO_1X1_ALGO", "big")
        knobs.set("WINO_1X1_SK", 1)
    blk = _Blocks(torch, 2, Hin, Win, seed=100 * Hin + Win)
    want = {"residual": blk.reference_residual(), "proj": blk.reference_proj(stride)}
    for align in guarded.ALIGNS:
        got = _run_blocks(pkg, torch_dev, blk, stride, align, f"blocks {Hin}x{Win} s={stride} forced={forced} align={align}")
        for name in want:
            err = rel(torch, got[name], want[name])
            assert err < TIGHT, (name, Hin, Win, stride, align, err)
            assert 0.1 < float((want[name] > 0).double().mean()) < 1.0      # both sides of the final ReLU
    assert pkg.tickets_in_use() == 0



# ---------------------------------------------------------------------------------------------------- the networks
def _input(torch, dev, N, H, W, seed):
    return (torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(dev)


@pytest.mark.parametrize("arch,N,H", [("resnext50_32x4d", 2, 64), ("wide_resnet50_2", 2, 64), ("resnext101_64x4d", 1, 32)])
def test_network_matches_fp64(arch, N, H, pkg, R, torch_dev):
    torch, dev = torch_dev
    sd = random_state_dict(torch, R, arch, seed=len(arch) + N)
    model = pkg.ResNet.from_state_dict(sd, arch)
    kinds = {kind for blocks in model.layers for kind, *_ in blocks}
    if arch.startswith("resnext"):
        assert kinds == {"grouped_proj", "grouped_proj_s2", "grouped_residual"}, kinds
    else:
        assert kinds == {"proj", "proj_v15", "residual"}, kinds
    x = _input(torch, dev, N, H, H, seed=N + H)
    check_net(torch, model, sd, arch, x)
    assert pkg.tickets_in_use() == 0


def test_resnext50_graph_replay_is_bitwise_eager(pkg, R, torch_dev):
    torch, dev = torch_dev
    arch, N, H, W = "resnext50_32x4d", 2, 64, 48
    sd = random_state_dict(torch, R, arch, classes=10, seed=50)
    model = pkg.ResNet.from_state_dict(sd, arch)
    x = _input(torch, dev, N, H, W, seed=9)
    eager, graph = network_graph_scenario(pkg, torch, model, x, rounds=1)
    want, _ = reference_forward(torch, sd, x.cpu())
    assert rel(torch, eager, want) < NET_TOL
    del graph


@pytest.mark.parametrize("arch", ["resnet18", "resnet34", "resnet50", "resnet101", "resnet152"])
def test_existing_archs_have_not_moved(arch, pkg, R, torch_dev):
    """The default (groups, width_per_group) = (1, 64) path: the same block kinds and shapes as before, the logits within
    NET_TOL of the fp64 forward."""
    torch, dev = torch_dev
    sd = random_state_dict(torch, R, arch, seed=len(arch))
    model = pkg.ResNet.from_state_dict(sd, arch)
    assert model.groups == 1
    for planes, blocks in zip(R.PLANES, model.layers):
        assert all(cm == planes for _, _, cm, _, _ in blocks)
        assert not any(kind.startswith("grouped") for kind, *_ in blocks)
    x = _input(torch, dev, 1, 64, 64, seed=64)
    logits = model(x)
    torch.cuda.synchronize()
    want, _ = reference_forward(torch, sd, x.cpu())
    assert rel(torch, logits, want) < NET_TOL
    assert pkg.tickets_in_use() == 0
