"""GPU tests of the downsampling basic block: the fused stride-2 3x3 + 1x1 stride-2 shortcut layer
(wino_conv3x3_s2_proj_bn_relu_hw, the 1x1 kernels in operand form A_TAPS_PROJ) and the block on it
(wino_basic_block_s2_hw).  Outputs go into NaN-filled buffers and are compared with fp64 references built here (torch on
the CPU); t1 bitwise against the plain stride-2 layer in every forced form; the block against a torchvision-style
BasicBlock with `downsample`; odd and tiny maps; a ResNet-18 stage opening; graph replay; the stream-K fail-fast
contract; Python argument errors."""
import numpy as np
import pytest

import layer_refs as LR
from cases import S2_FORM_SHAPES, S2_FORMS, TIGHT, S2Block, ring_mask, s2_legal
from gpu_support import dirty_ticket_scenario, graph_replay_scenario, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu

# the downsampling blocks of ResNet-18 / -34: (Hin, C, K), stride 2 on the first 3x3 and on the 1x1 shortcut
STAGES = {"conv3": (56, 64, 128), "conv4": (28, 128, 256), "conv5": (14, 256, 512)}


LAYER_POINTS = [(s, n) for s in sorted(STAGES) for n in (1, 2, 8, 32)] + [("conv4", 128)]


@pytest.mark.parametrize("stage,N", LAYER_POINTS)
def test_fused_layer_at_stage_shapes(stage, N, pkg, O, torch_dev):
    """t1 and sc of the fused layer against fp64, and t1 bitwise the plain stride-2 layer's output."""
    torch, _ = torch_dev
    Hin, C, K = STAGES[stage]
    blk = S2Block(pkg, torch_dev, N, Hin, Hin, C, K, seed=Hin * 1000 + N)
    t1, sc = blk.layer()
    blk.check_layer(O, t1, sc, idx=None if N <= 32 else [0, 77, 127])
    assert torch.equal(t1, blk.plain())
    assert pkg.tickets_in_use() == 0


@pytest.mark.parametrize("form,shape", [(f, s) for s in S2_FORM_SHAPES for f in sorted(S2_FORMS) if s2_legal(f, s)])
def test_forced_forms(form, shape, pkg, O, torch_dev, knobs):
    """In every form: t1 bitwise the plain layer's, sc against fp64, both bitwise from launch to launch."""
    torch, _ = torch_dev
    for k, v in S2_FORMS[form].items():
        knobs.set(k, v)
    N, Hin, Win, C, K = shape
    want = {"latency": pkg.FORM_LATENCY, "tiled": pkg.FORM_TILED}.get(form.split("_")[0], pkg.FORM_STREAM_K)
    assert pkg.conv3x3_s2_plan(N, Hin, Win, C, K) == want
    blk = S2Block(pkg, torch_dev, N, Hin, Win, C, K, seed=N * Hin + C)
    t1, sc = blk.layer()
    blk.check_layer(O, t1, sc)
    assert torch.equal(t1, blk.plain())
    t1b, scb = blk.layer()
    assert torch.equal(t1b, t1)
    assert torch.equal(scb[:, 1:-1, 1:-1, :], sc[:, 1:-1, 1:-1, :])
    assert pkg.tickets_in_use() == 0


def _torch_basic_block(torch, blk, dev):
    """torchvision's BasicBlock with `downsample` in eval mode, written in plain torch.nn (fp32, channels-last, on
    `dev`): random running statistics, folded here into the library's (bias, scale) pairs."""
    nn = torch.nn
    C, K = blk.C, blk.K
    g = torch.Generator(device="cpu").manual_seed(C + K)

    def bn():
        m = nn.BatchNorm2d(K, eps=1e-5)
        m.weight.data = torch.rand(K, generator=g) + 0.5
        m.bias.data = torch.rand(K, generator=g) - 0.5
        m.running_mean.data = torch.rand(K, generator=g) - 0.5
        m.running_var.data = torch.rand(K, generator=g) + 0.5
        return m.eval()

    def fold(m):
        s = m.weight.data / torch.sqrt(m.running_var.data + m.eps)
        return m.bias.data - m.running_mean.data * s, s

    conv1 = nn.Conv2d(C, K, 3, stride=2, padding=1, bias=False)
    conv2 = nn.Conv2d(K, K, 3, stride=1, padding=1, bias=False)
    convd = nn.Conv2d(C, K, 1, stride=2, bias=False)
    conv1.weight.data, conv2.weight.data, convd.weight.data = blk.w1.clone(), blk.w2.clone(), blk.wd.clone()
    bn1, bn2, bnd = bn(), bn(), bn()
    (blk.b1, blk.s1), (blk.b2, blk.s2), (blk.bd, blk.sd) = fold(bn1), fold(bn2), fold(bnd)
    for m in (conv1, conv2, convd, bn1, bn2, bnd):
        m.to(dev).to(memory_format=torch.channels_last)

    def forward(x):
        out = torch.relu(bn1(conv1(x)))
        out = bn2(conv2(out))
        return torch.relu(out + bnd(convd(x)))

    return forward


@pytest.mark.parametrize("N", [1, 8, 32])
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_block_against_fp64_and_torch(stage, N, pkg, O, torch_dev):
    """The block against the fp64 composition, and against a torchvision-style BasicBlock with `downsample` (eval-mode
    BatchNorm with random running statistics, folded) run by torch on the GPU."""
    torch, dev = torch_dev
    Hin, C, K = STAGES[stage]
    blk = S2Block(pkg, torch_dev, N, Hin, Hin, C, K, seed=7 * Hin + N)
    fwd = _torch_basic_block(torch, blk, dev)
    t = lambda a: a.contiguous().to(dev)
    K_ = blk.K
    blk.packed = pkg.s2_proj_pack(blk.taps, (t(blk.b1), t(blk.s1)), t(blk.wd.view(K_, C).t()), (t(blk.bd), t(blk.sd)))
    blk.bn2 = (t(blk.b2), t(blk.s2))
    out = blk.block()
    blk.check_block(O, out)
    with torch.no_grad():
        xin = blk.x[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).to(dev).contiguous(memory_format=torch.channels_last)
        ref = fwd(xin)
    assert O.rel_error(out[:, 1:-1, 1:-1, :].cpu().numpy(), ref.permute(0, 2, 3, 1).cpu().numpy()) < 1e-4
    assert pkg.tickets_in_use() == 0


@pytest.mark.parametrize("N,Hin,Win,C,K", [
    (2, 15, 15, 64, 128),    # 15 -> 8: the last output's window reaches the far ring
    (3, 7, 7, 128, 64),      # 7 -> 4, K < C
    (4, 1, 1, 64, 128),      # 1 -> 1: only the centre tap sees data
    (1, 15, 7, 32, 64),      # 15 x 7 -> 8 x 4, C = 32: one k-step per tap
])
def test_odd_and_tiny_maps(N, Hin, Win, C, K, pkg, O, torch_dev):
    torch, _ = torch_dev
    blk = S2Block(pkg, torch_dev, N, Hin, Win, C, K, seed=N + Hin * Win + C)
    t1, sc = blk.layer()
    blk.check_layer(O, t1, sc)
    assert torch.equal(t1, blk.plain())
    blk.check_block(O, blk.block())


@pytest.mark.parametrize("N", [1, 8])
def test_resnet18_stage_opening(N, pkg, O, torch_dev):
    """conv4's opening: the downsampling block (28 -> 14, 128 -> 256), then an identity basic_block in place on its
    out -- the padded layout chains as it stands -- against fp64."""
    torch, dev = torch_dev
    Hin, C, K = STAGES["conv4"]
    blk = S2Block(pkg, torch_dev, N, Hin, Hin, C, K, seed=1804 + N)
    g = torch.Generator(device="cpu").manual_seed(N)
    w3 = (torch.rand(K, K, 3, 3, generator=g) - 0.5) / np.sqrt(9 * K) * 4
    w4 = (torch.rand(K, K, 3, 3, generator=g) - 0.5) / np.sqrt(9 * K) * 4
    b3, s3, b4, s4 = (torch.rand(K, generator=g) + lo for lo in (-0.5, 0.5, -0.5, 0.5))
    t = lambda a: a.contiguous().to(dev)
    y = blk.block()
    out = pkg.basic_block(y, pkg.filter_transform_f2(t(w3)), (t(b3), t(s3)), pkg.filter_transform_f2(t(w4)),
                          (t(b4), t(s4)), out=y)
    assert out.data_ptr() == y.data_ptr()
    want = LR.basic_block(blk.reference()[2], w3, (b3, s3), w4, (b4, s4)).numpy()
    g_ = out.cpu().numpy()
    assert (g_[:, ring_mask(blk.H, blk.W), :] == 0).all()
    assert O.rel_error(g_[:, 1:-1, 1:-1, :], want) < TIGHT


@pytest.mark.parametrize("stage,N", [("conv3", 1), ("conv4", 32)])
def test_block_in_a_graph(stage, N, pkg, O, torch_dev):
    """The two launches captured into one graph (one stream) after basic_block_s2_prepare: the replay is bitwise the
    eager result."""
    torch, dev = torch_dev
    Hin, C, K = STAGES[stage]
    blk = S2Block(pkg, torch_dev, N, Hin, Hin, C, K, seed=4242 + N)
    eager = graph_replay_scenario(pkg, torch_dev, blk.block, lambda: pkg.basic_block_s2_prepare(N, Hin, Hin, C, K),
                                  pkg.lib().wino_basic_block_s2_workspace_bytes_hw(N, Hin, Hin, K))
    blk.check_block(O, eager)


def test_a_dirty_ticket_counter_is_reported_and_reset_recovers(pkg, O, torch_dev, knobs):
    """The fused layer in the forced stream-K form keeps the fail-fast contract: a ticket counter left non-zero is
    reported, every launch on the stream then fails with WINO_E_STATE, and wino_stream_reset_scratch() recovers
    bitwise results.  The shortcut's appended tiles never touch the tickets."""
    torch, dev = torch_dev
    knobs.set("WINO_1X1_ALGO", "big")
    knobs.set("WINO_1X1_SK", 1)
    N, Hin, Win, C, K = S2_FORM_SHAPES[0]
    blk = S2Block(pkg, torch_dev, N, Hin, Win, C, K, seed=99)
    assert pkg.conv3x3_s2_plan(N, Hin, Win, C, K) == pkg.FORM_STREAM_K
    n_tickets = ((N * 14 * 14 + 111) // 112) * (K // 128)   # row tiles x column blocks
    inner = lambda sc: sc[:, 1:-1, 1:-1, :]   # sc's ring is never written
    dirty_ticket_scenario(pkg, torch, blk.layer, n_tickets,
                          same=lambda got, ref: torch.equal(got[0], ref[0]) and torch.equal(inner(got[1]), inner(ref[1])),
                          check=lambda ref: blk.check_layer(O, *ref), also_refused=[blk.block],
                          after=lambda: blk.check_block(O, blk.block()))


def test_bad_arguments_raise(pkg, torch_dev):
    torch, dev = torch_dev
    blk = S2Block(pkg, torch_dev, 1, 14, 14, 64, 128, seed=3)
    with pytest.raises(pkg.WinoError):
        pkg.s2_proj_pack(blk.taps, blk.bn1, blk.taps, blk.bn1)                        # wd not [C][K]
    with pytest.raises(pkg.WinoError):
        pkg.s2_proj_pack(blk.taps, blk.bn1, torch.zeros(64, 128, device=dev), (blk.bn2[0][:64], blk.bn2[1]))
    with pytest.raises(pkg.WinoError):
        pkg.conv3x3_s2_proj(blk.x, blk.packed)                                         # CPU input
    with pytest.raises(pkg.WinoError):
        pkg.conv3x3_s2_proj(blk.xt.double(), blk.packed)                               # float64
    with pytest.raises(pkg.WinoError):
        pkg.conv3x3_s2_proj(blk.xt, blk.packed[:-1])                                   # not a packed buffer
    with pytest.raises(pkg.WinoError):
        pkg.conv3x3_s2_proj(blk.xt, blk.packed, t1=torch.empty(1, 16, 16, 128, device=dev))   # wrong t1 shape
    with pytest.raises(pkg.WinoError):
        pkg.basic_block_s2(blk.xt, blk.packed, blk.U2, blk.bn2, out=torch.empty(1, 16, 16, 128, device=dev))
    with pytest.raises(pkg.WinoError):
        pkg.basic_block_s2(blk.xt, blk.packed, blk.U2, blk.bn2, workspace=torch.empty(10, device=dev))
    with pytest.raises(pkg.WinoError):
        pkg.basic_block_s2(blk.xt, blk.packed, blk.U2[:-1], blk.bn2)                    # U2 not K -> K
    with pytest.raises(pkg.WinoError):
        pkg.basic_block_s2(blk.xt, blk.packed, blk.U2, (blk.bn2[0][:64], blk.bn2[1]))   # bn2 not K long
    x48 = torch.zeros(1, 16, 16, 48, device=dev)
    with pytest.raises(pkg.WinoError, match="rc=-2"):
        pkg.conv3x3_s2_proj(x48, torch.zeros((10 * 48 + 4) * 128, device=dev))         # C % 32
