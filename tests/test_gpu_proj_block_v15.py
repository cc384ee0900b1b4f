"""GPU tests of the v1.5 projection block, wino_proj_block_v15_hw (torchvision's placement: the stride 2 on the 3x3).
Three launches -- the 1x1 at full input resolution, the stride-2 3x3 (conv3x3_s2.hip), the v1 block's fused tail at
stride 2 -- against an fp64 composition computed here, against a v1.5 Bottleneck module written in plain torch with
eval-mode BN, and captured in a graph."""
import pytest

from cases import TIGHT, V15Block
from gpu_support import graph_replay_scenario, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu

# ResNet-50's v1.5 downsampling blocks: (Hin, Cin, Cm, C4)
STAGES = {
    "conv3": (56, 256, 128, 512),
    "conv4": (28, 512, 256, 1024),
    "conv5": (14, 1024, 512, 2048),
}


@pytest.mark.parametrize("N", [1, 16])
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_stage_blocks(stage, N, pkg, O, torch_dev):
    Hin, Cin, Cm, C4 = STAGES[stage]
    blk = V15Block(pkg, torch_dev, N, Hin, Hin, Cin, Cm, C4, seed=Hin + N)
    blk.check(O, blk.run())


def test_conv4_block_at_128_images(pkg, O, torch_dev):
    Hin, Cin, Cm, C4 = STAGES["conv4"]
    blk = V15Block(pkg, torch_dev, 128, Hin, Hin, Cin, Cm, C4, seed=4128)
    blk.check(O, blk.run(), idx=[0, 77, 127])


def test_odd_input(pkg, O, torch_dev):
    """Hin = 15, Win = 13 (8 x 7 outputs), Cin = 96."""
    blk = V15Block(pkg, torch_dev, 3, 15, 13, 96, 128, 256, seed=1513)
    blk.check(O, blk.run())


def _bottleneck_v15(torch, Cin, Cm, C4):
    """torchvision's Bottleneck with a projection (v1.5: conv2 carries the stride), written out in plain torch."""
    nn = torch.nn

    class Bottleneck(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1 = nn.Conv2d(Cin, Cm, 1, bias=False)
            self.bn1 = nn.BatchNorm2d(Cm)
            self.conv2 = nn.Conv2d(Cm, Cm, 3, stride=2, padding=1, bias=False)
            self.bn2 = nn.BatchNorm2d(Cm)
            self.conv3 = nn.Conv2d(Cm, C4, 1, bias=False)
            self.bn3 = nn.BatchNorm2d(C4)
            self.relu = nn.ReLU(inplace=True)
            self.downsample = nn.Sequential(nn.Conv2d(Cin, C4, 1, stride=2, bias=False), nn.BatchNorm2d(C4))

        def forward(self, x):
            out = self.relu(self.bn1(self.conv1(x)))
            out = self.relu(self.bn2(self.conv2(out)))
            out = self.bn3(self.conv3(out))
            return self.relu(out + self.downsample(x))

    return Bottleneck()


@pytest.mark.parametrize("stage,N", [("conv4", 2), ("conv3", 1)])
def test_torchvision_style_weights(stage, N, pkg, O, torch_dev):
    """A v1.5 Bottleneck module with random eval-mode BN statistics: its folded weights through the library against
    the module's own float64 CPU forward."""
    torch, dev = torch_dev
    Hin, Cin, Cm, C4 = STAGES[stage]
    torch.manual_seed(15 + N)
    m = _bottleneck_v15(torch, Cin, Cm, C4)
    for bn in (m.bn1, m.bn2, m.bn3, m.downsample[1]):
        c = bn.num_features
        bn.weight.data = torch.rand(c) + 0.5
        bn.bias.data = torch.rand(c) - 0.5
        bn.running_mean.data = (torch.rand(c) - 0.5) * 0.2
        bn.running_var.data = torch.rand(c) * 0.5 + 0.5
    m.eval()

    def fold(bn):
        scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        return (bn.bias - bn.running_mean * scale).detach(), scale.detach()

    with torch.no_grad():
        x = torch.rand(N, Cin, Hin, Hin) - 0.5
        want = m.double()(x.double()).permute(0, 2, 3, 1).numpy()
        m.float()
        to = lambda a: a.float().contiguous().to(dev)
        w1 = to(m.conv1.weight[:, :, 0, 0].t())
        w3 = to(m.conv3.weight[:, :, 0, 0].t())
        wp = to(m.downsample[0].weight[:, :, 0, 0].t())
        bn1, bn2, bn3, bnp = ([to(v) for v in fold(b)] for b in (m.bn1, m.bn2, m.bn3, m.downsample[1]))
        taps = pkg.filter_pack_s2(to(m.conv2.weight))
        tail = pkg.proj_tail_pack(w3, bn3, wp, bnp)
        got = pkg.proj_block_v15(to(x.permute(0, 2, 3, 1)), w1, bn1, taps, bn2, tail)
    g = got.cpu().numpy()
    assert g.shape == want.shape
    assert O.rel_error(g, want) < TIGHT
    assert (want > 0).mean() > 0.2


@pytest.mark.parametrize("stage,N", [("conv4", 20), ("conv3", 1)])
def test_block_in_a_graph(stage, N, pkg, O, torch_dev):
    """The three launches captured into one HIP graph (one stream, no parallel branches) after proj_block_v15_prepare:
    the replay equals eager bit for bit."""
    torch, dev = torch_dev
    Hin, Cin, Cm, C4 = STAGES[stage]
    blk = V15Block(pkg, torch_dev, N, Hin, Hin, Cin, Cm, C4, seed=808 + N)
    eager = graph_replay_scenario(pkg, torch_dev, blk.run, lambda: pkg.proj_block_v15_prepare(N, Hin, Hin, Cin, Cm, C4),
                                  pkg.lib().wino_proj_block_v15_workspace_bytes_hw(N, Hin, Hin, Cm))
    blk.check(O, eager, idx=[0])


def test_bad_arguments_raise(pkg, torch_dev):
    torch, dev = torch_dev
    blk = V15Block(pkg, torch_dev, 1, 14, 14, 64, 64, 128, seed=5)
    with pytest.raises(pkg.WinoError):
        blk.run(workspace=torch.empty(16, device=dev))                                     # workspace too small
    with pytest.raises(pkg.WinoError):
        blk.run(out=torch.empty(1, 14, 14, 128, device=dev))                               # the stride-1 shape
    with pytest.raises(pkg.WinoError):
        pkg.proj_block_v15(blk.xt, blk.w1t, blk.bnt[0], blk.taps.permute(3, 2, 0, 1).contiguous(), blk.bnt[1],
                           blk.tail)                                                       # [K][C][3][3] taps
    with pytest.raises(pkg.WinoError):
        pkg.proj_block_v15(blk.x, blk.w1t, blk.bnt[0], blk.taps, blk.bnt[1], blk.tail)    # CPU input
    with pytest.raises(pkg.WinoError, match="bn1 / bn2 vectors must have Cm values"):
        pkg.proj_block_v15(blk.xt, blk.w1t, (blk.bnt[0][0][:-1], blk.bnt[0][1]), blk.taps, blk.bnt[1],
                           blk.tail)                                                       # bn1's bias one value short
    x48 = torch.zeros(1, 14, 14, 48, device=dev)
    with pytest.raises(pkg.WinoError, match="rc=-2"):
        pkg.proj_block_v15(x48, torch.zeros(48, 64, device=dev), blk.bnt[0], blk.taps, blk.bnt[1],
                           torch.zeros((64 + 48 + 2) * 128, device=dev))                   # Cin % 32
