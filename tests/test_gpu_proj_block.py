"""GPU tests of the projection (downsampling) bottleneck block, wino_proj_block_hw: the first block of every ResNet
stage, v1 placement (stride on the first 1x1 and on the projection).  Three launches -- strided 1x1, Winograd 3x3,
and the fused tail (last 1x1 + projection shortcut in one GEMM of K = Cm + Cin) -- against the fp64 composition of
the layer oracles, the comparator kernels, and the four-launch composition the library allowed before."""
import numpy as np
import pytest

import layer_refs as LR
from cases import PROJ_FORMS, TIGHT, proj_weights
from gpu_support import graph_replay_scenario, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu

# ResNet-50's four stage-entry blocks: (Hin, Cin, Cm, C4, stride)
STAGES = {
    "conv2": (56, 64, 64, 256, 1),
    "conv3": (56, 256, 128, 512, 2),
    "conv4": (28, 512, 256, 1024, 2),
    "conv5": (14, 1024, 512, 2048, 2),
}


class _Block:
    """One block's tensors on the GPU, and the library's three ways to run it."""

    def __init__(self, pkg, torch_dev, N, Hin, Win, Cin, Cm, C4, s, seed):
        self.torch, self.dev = torch_dev
        self.pkg, self.s = pkg, s
        rng = np.random.RandomState(seed)
        self.x = (rng.rand(N, Hin, Win, Cin) - 0.5).astype(np.float32)
        self.w1, self.w2, self.w3, self.wp, self.bn = proj_weights(rng, Cin, Cm, C4)
        t = lambda a: self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.xt, self.w1t, self.w2t, self.w3t, self.wpt = t(self.x), t(self.w1), t(self.w2), t(self.w3), t(self.wp)
        self.bnt = [(t(b), t(sc)) for b, sc in self.bn]
        self.U2 = pkg.filter_transform_f2(self.w2t)
        self.tail = pkg.proj_tail_pack(self.w3t, self.bnt[2], self.wpt, self.bnt[3])
        self.H, self.W = (Hin - 1) // s + 1, (Win - 1) // s + 1
        self.N, self.Cin, self.Cm, self.C4 = N, Cin, Cm, C4

    def run(self, out=None, workspace=None):
        """The fused block, into NaN-filled output and workspace unless given."""
        torch = self.torch
        if out is None:
            out = torch.full((self.N, self.H, self.W, self.C4), float("nan"), device=self.dev)
        if workspace is None:
            need = self.pkg.lib().wino_proj_block_workspace_bytes_hw(self.N, self.H, self.W, self.Cm)
            workspace = torch.full((need // 4,), float("nan"), device=self.dev)
        return self.pkg.proj_block(self.xt, self.w1t, self.bnt[0], self.U2, self.bnt[1], self.tail, self.s,
                                   out=out, workspace=workspace)

    def composed(self):
        """What the library allowed before: a torch strided copy of x, the projection 1x1 written to memory, then
        the identity block's three launches with the shortcut added as a residual."""
        pkg, torch = self.pkg, self.torch
        xs = self.xt[:, ::self.s, ::self.s, :].contiguous()
        short = pkg.conv1x1_bn_ex(xs, self.wpt, self.bnt[3][0], self.bnt[3][1], 0)
        t1p = pkg.conv1x1_bn_ex(xs, self.w1t, self.bnt[0][0], self.bnt[0][1], pkg.RELU | pkg.C_PADDED)
        t2p = pkg.conv3x3_bn_relu(t1p, self.U2, self.bnt[1][0], self.bnt[1][1])
        out = pkg.conv1x1_bn_ex(t2p, self.w3t, self.bnt[2][0], self.bnt[2][1],
                                pkg.RELU | pkg.A_PADDED | pkg.ADD_RESIDUAL, residual=short)
        return out.reshape(self.N, self.H, self.W, self.C4)

    def oracle(self, idx=None):
        x, bn = self.x if idx is None else self.x[idx], self.bn
        return LR.bottleneck(x, self.w1, bn[0], self.w2, bn[1], self.w3, bn[2], self.wp, bn[3], stride=self.s).numpy()


def _check_block(blk, O, got, idx=None):
    got = got.cpu().numpy()
    assert np.isfinite(got).all()
    want = blk.oracle(idx)
    g = got if idx is None else got[idx]
    assert g.shape == want.shape
    assert O.rel_error(g, want) < TIGHT
    assert (want > 0).mean() > 0.2   # both sides of the final ReLU
    assert blk.pkg.tickets_in_use() == 0


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_stage_entry_blocks(stage, N, pkg, O, torch_dev):
    """ResNet-50's four stage-entry blocks at one image (the latency forms) and a few."""
    Hin, Cin, Cm, C4, s = STAGES[stage]
    blk = _Block(pkg, torch_dev, N, Hin, Hin, Cin, Cm, C4, s, seed=Hin + N)
    _check_block(blk, O, blk.run())


@pytest.mark.parametrize("N,Cin,Cm,C4", [(1, 64, 64, 128), (4, 96, 128, 256)])
def test_odd_input_stride_two(N, Cin, Cm, C4, pkg, O, torch_dev):
    """Hin = 15, Win = 13 at stride 2: the (Hin-1)/2 + 1 edge (8 x 7 outputs); Cin = 96 is not a multiple of 64."""
    blk = _Block(pkg, torch_dev, N, 15, 13, Cin, Cm, C4, 2, seed=1513 + N)
    assert (blk.H, blk.W) == (8, 7)
    _check_block(blk, O, blk.run())


def test_conv4_block_at_128_images(pkg, O, torch_dev):
    """The conv4_x entry block at N = 128: sampled images against the fp64 oracle, every element against a chain of
    the comparator kernels (direct 1x1 on a strided copy, direct 3x3, direct 1x1 for the tail and the projection)."""
    torch, dev = torch_dev
    Hin, Cin, Cm, C4, s = STAGES["conv4"]
    N = 128
    blk = _Block(pkg, torch_dev, N, Hin, Hin, Cin, Cm, C4, s, seed=4128)
    got = blk.run()
    _check_block(blk, O, got, idx=[0, 77, 127])
    H, W = blk.H, blk.W
    xs = blk.xt[:, ::s, ::s, :].contiguous().reshape(-1, Cin)
    t1 = pkg.conv1x1_direct(xs, blk.w1t, blk.bnt[0][0], blk.bnt[0][1], True)
    t1p = torch.zeros((N, H + 2, W + 2, Cm), device=dev)
    t1p[:, 1:-1, 1:-1, :] = t1.reshape(N, H, W, Cm)
    t2 = pkg.conv3x3_direct(t1p, blk.w2t, blk.bnt[1][0], blk.bnt[1][1], True)[:, 1:-1, 1:-1, :].reshape(-1, Cm)
    t3 = pkg.conv1x1_direct(t2, blk.w3t, blk.bnt[2][0], blk.bnt[2][1], False)
    sc = pkg.conv1x1_direct(xs, blk.wpt, blk.bnt[3][0], blk.bnt[3][1], False)
    chain = torch.relu(t3 + sc).reshape(N, H, W, C4)
    assert O.rel_error(got.cpu().numpy(), chain.cpu().numpy()) < TIGHT


@pytest.mark.parametrize("form", sorted(PROJ_FORMS))
@pytest.mark.parametrize("N,Hin,Cin,Cm,C4,s", [(2, 28, 256, 128, 512, 2), (2, 14, 96, 64, 128, 1)])
def test_forced_forms(form, N, Hin, Cin, Cm, C4, s, pkg, O, torch_dev, knobs):
    """Every form of both kernel families, including stream-K / split-K segments that start, end or straddle the
    fused tail's phase boundary; each against the oracle, and all forms against each other to tolerance."""
    for k, v in PROJ_FORMS[form].items():
        knobs.set(k, v)
    blk = _Block(pkg, torch_dev, N, Hin, Hin, Cin, Cm, C4, s, seed=N * Hin + Cin)
    _check_block(blk, O, blk.run())


def test_plan_query_names_the_forced_forms(pkg, knobs):
    """The forms the forced-form test relies on are the ones the plan query reports."""
    shape = (2, 28, 28, 256, 128, 512, 2)
    knobs.set("WINO_1X1_ALGO", "small")
    assert pkg.proj_tail_plan(*shape) == (pkg.FORM_LATENCY, pkg.FORM_LATENCY)
    knobs.set("WINO_1X1_ALGO", "big")
    knobs.set("WINO_1X1_SK", 0)
    assert pkg.proj_tail_plan(*shape) == (pkg.FORM_TILED, pkg.FORM_TILED)
    knobs.set("WINO_1X1_SK", 1)
    assert pkg.proj_tail_plan(*shape) == (pkg.FORM_STREAM_K, pkg.FORM_STREAM_K)


@pytest.mark.parametrize("stage,N", [("conv3", 1), ("conv4", 8), ("conv5", 32), ("conv2", 2)])
def test_reproducible_and_equal_to_the_composition(stage, N, pkg, O, torch_dev):
    """Two calls give bitwise-equal outputs; the result agrees with the four-launch composition of the existing
    entry points (strided copy, projection 1x1, three launches with the shortcut as residual) to tolerance."""
    torch, _ = torch_dev
    Hin, Cin, Cm, C4, s = STAGES[stage]
    blk = _Block(pkg, torch_dev, N, Hin, Hin, Cin, Cm, C4, s, seed=77 + N)
    a = blk.run().clone()
    b = blk.run()
    assert torch.equal(a, b)
    comp = blk.composed()
    assert O.rel_error(a.cpu().numpy(), comp.cpu().numpy()) < TIGHT
    assert pkg.tickets_in_use() == 0


@pytest.mark.parametrize("stage,N", [("conv4", 20), ("conv3", 1)])
def test_block_in_a_graph(stage, N, pkg, O, torch_dev):
    """The three launches captured into one HIP graph after proj_block_prepare: the replay equals eager bit for bit."""
    torch, dev = torch_dev
    Hin, Cin, Cm, C4, s = STAGES[stage]
    blk = _Block(pkg, torch_dev, N, Hin, Hin, Cin, Cm, C4, s, seed=808 + N)
    eager = graph_replay_scenario(pkg, torch_dev, blk.run, lambda: pkg.proj_block_prepare(N, Hin, Hin, Cin, Cm, C4, s),
                                  pkg.lib().wino_proj_block_workspace_bytes_hw(N, blk.H, blk.W, Cm))
    _check_block(blk, O, eager, idx=[0])


def test_bad_arguments_raise(pkg, torch_dev):
    torch, dev = torch_dev
    blk = _Block(pkg, torch_dev, 1, 14, 14, 64, 64, 128, 2, seed=5)
    with pytest.raises(pkg.WinoError):
        pkg.proj_block(blk.xt, blk.w1t, blk.bnt[0], blk.U2, blk.bnt[1], blk.tail, 3)
    ws = torch.empty(16, device=dev)
    with pytest.raises(pkg.WinoError):
        blk.run(workspace=ws)
    short = (blk.bnt[1][0], blk.bnt[1][1][:-1])                                            # bn2's scale one value short
    with pytest.raises(pkg.WinoError, match="bn1 / bn2 vectors must have Cm values"):
        pkg.proj_block(blk.xt, blk.w1t, blk.bnt[0], blk.U2, short, blk.tail, 2)
