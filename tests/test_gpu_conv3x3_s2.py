"""GPU tests of the stride-2 3x3 layer, wino_conv3x3_s2_bn_relu_hw: the 1x1 GEMM kernels in operand form A_TAPS
(K = 9C, the nine taps as scalar k offsets into the padded input).  Against an fp64 reference computed here (torch on
the CPU: stride-2, pad-1 conv, BN, ReLU) into NaN-filled outputs; every form forced; the stream-K fail-fast contract."""
import pytest

from cases import S2_FORM_SHAPES, S2_FORMS, TIGHT, S2Layer, s2_legal
from gpu_support import dirty_ticket_scenario, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu

STAGES = {"conv3": (56, 56, 128, 128), "conv4": (28, 28, 256, 256), "conv5": (14, 14, 512, 512)}


@pytest.mark.parametrize("N", [1, 2, 8])
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_stage_shapes(stage, N, pkg, O, torch_dev):
    """The 3x3 of ResNet-50's v1.5 stage-entry blocks (56->28, 28->14, 14->7) at a few images."""
    Hin, Win, C, K = STAGES[stage]
    layer = S2Layer(pkg, torch_dev, N, Hin, Win, C, K, seed=Hin * 10 + N)
    layer.check(O, layer.run())
    assert pkg.tickets_in_use() == 0


@pytest.mark.parametrize("N,Hin,Win,C,K", [
    (2, 15, 15, 64, 128),    # 15 -> 8: the last output row / column's window reaches the far ring
    (2, 7, 7, 128, 64),      # 7 -> 4, C != K
    (8, 5, 9, 96, 192),      # 5 x 9 -> 3 x 5; C / 32 = 3 k-steps per tap, K % 128 != 0
    (2, 2, 2, 32, 64),       # 2 -> 1
    (8, 1, 1, 64, 128),      # 1 -> 1: only the centre tap sees data
    (1, 28, 28, 512, 128),   # C != K
])
def test_odd_and_small_maps(N, Hin, Win, C, K, pkg, O, torch_dev):
    layer = S2Layer(pkg, torch_dev, N, Hin, Win, C, K, seed=N + Hin * Win + C)
    layer.check(O, layer.run())
    layer.check(O, layer.run(relu=False), relu=False)


def test_conv4_at_128_images(pkg, O, torch_dev):
    """N = 128 (the tiled kernel), sampled images against the fp64 reference, all of it against the 3x3 comparator
    kernel applied at stride 1 and subsampled."""
    torch, dev = torch_dev
    Hin, Win, C, K = STAGES["conv4"]
    layer = S2Layer(pkg, torch_dev, 128, Hin, Win, C, K, seed=4128)
    got = layer.run()
    layer.check(O, got, idx=[0, 63, 127])
    full = pkg.conv3x3_direct(layer.xt, layer.wt, layer.bt, layer.st, True)   # stride 1, [N][Hin+2][Win+2][K]
    want = full[:, 1:-1:2, 1:-1:2, :]
    assert O.rel_error(got[:, 1:-1, 1:-1, :].cpu().numpy(), want.cpu().numpy()) < TIGHT
    assert pkg.tickets_in_use() == 0


@pytest.mark.parametrize("form,shape", [(f, s) for s in S2_FORM_SHAPES for f in sorted(S2_FORMS) if s2_legal(f, s)])
def test_forced_forms(form, shape, pkg, O, torch_dev, knobs):
    """Every form of both kernel families against the reference, and bitwise equal from launch to launch."""
    torch, _ = torch_dev
    for k, v in S2_FORMS[form].items():
        knobs.set(k, v)
    N, Hin, Win, C, K = shape
    want = {"latency": pkg.FORM_LATENCY, "tiled": pkg.FORM_TILED}.get(form.split("_")[0], pkg.FORM_STREAM_K)
    ks = S2_FORMS[form].get("WINO_1X1_SMALL_KS", 1)
    assert pkg.conv3x3_s2_plan(N, Hin, Win, C, K) == want
    if want == pkg.FORM_LATENCY:
        assert pkg.small_plan_1x1_full(N * ((Hin + 1) // 2) * ((Win + 1) // 2), 9 * C, K)[1:4] == (
            ks, S2_FORMS[form]["WINO_1X1_SMALL_RT"], S2_FORMS[form]["WINO_1X1_SMALL_CT"])
    layer = S2Layer(pkg, torch_dev, N, Hin, Win, C, K, seed=N * Hin + C)
    a = layer.run().clone()
    layer.check(O, a)
    assert torch.equal(layer.run(), a)
    assert pkg.tickets_in_use() == 0


def test_a_dirty_ticket_counter_is_reported_and_reset_recovers(pkg, O, torch_dev, knobs):
    """The fail-fast contract of the stream-K form (test_gpu_latency.py): a ticket counter left non-zero (as by a
    launch that died mid-way) is reported, every launch on the stream then fails with WINO_E_STATE, and
    wino_stream_reset_scratch() recovers bitwise results."""
    torch, dev = torch_dev
    knobs.set("WINO_1X1_ALGO", "big")
    knobs.set("WINO_1X1_SK", 1)
    N, Hin, Win, C, K = S2_FORM_SHAPES[0]
    layer = S2Layer(pkg, torch_dev, N, Hin, Win, C, K, seed=99)
    assert pkg.conv3x3_s2_plan(N, Hin, Win, C, K) == pkg.FORM_STREAM_K
    n_tickets = ((N * 14 * 14 + 111) // 112) * (K // 128)   # row tiles x column blocks
    dirty_ticket_scenario(pkg, torch, layer.run, n_tickets, check=lambda ref: layer.check(O, ref))


def test_bad_arguments_raise(pkg, torch_dev):
    torch, dev = torch_dev
    layer = S2Layer(pkg, torch_dev, 1, 14, 14, 64, 128, seed=3)
    with pytest.raises(pkg.WinoError):
        pkg.conv3x3_s2_bn_relu(layer.xt, layer.wt, layer.bt, layer.st)               # [K][C][3][3], not packed
    with pytest.raises(pkg.WinoError):
        pkg.conv3x3_s2_bn_relu(layer.x, layer.taps, layer.bt, layer.st)              # CPU input
    with pytest.raises(pkg.WinoError):
        pkg.conv3x3_s2_bn_relu(layer.xt.double(), layer.taps, layer.bt, layer.st)    # float64
    with pytest.raises(pkg.WinoError):
        pkg.conv3x3_s2_bn_relu(layer.xt, layer.taps, layer.bt, layer.st, out=torch.empty(1, 16, 16, 128, device=dev))
    x48 = torch.zeros(1, 16, 16, 48, device=dev)
    with pytest.raises(pkg.WinoError, match="rc=-2"):
        pkg.conv3x3_s2_bn_relu(x48, torch.zeros(3, 3, 48, 128, device=dev), layer.bt, layer.st)
