"""GPU tests of the stride-2 3x3 layer, wino_conv3x3_s2_bn_relu_hw: the 1x1 GEMM kernels in operand form A_TAPS
(K = 9C, the nine taps as scalar k offsets into the padded input).  Against an fp64 reference computed here (torch on
the CPU: stride-2, pad-1 conv, BN, ReLU) into NaN-filled outputs; every form forced; the stream-K fail-fast contract."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TIGHT = 2e-5


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch, torch.device("cuda:0")


class _Layer:
    """One layer's tensors: the padded input with a zero ring, [K][C][3][3] weights, folded BN vectors."""

    def __init__(self, pkg, torch_dev, N, Hin, Win, C, K, seed):
        self.torch, self.dev = torch_dev
        self.pkg = pkg
        torch = self.torch
        g = torch.Generator(device="cpu").manual_seed(seed)
        x = torch.zeros(N, Hin + 2, Win + 2, C)
        x[:, 1:-1, 1:-1, :] = torch.rand(N, Hin, Win, C, generator=g) - 0.5
        self.x = x
        self.w = (torch.rand(K, C, 3, 3, generator=g) - 0.5) / np.sqrt(9 * C) * 4
        self.bias = torch.rand(K, generator=g) - 0.5
        self.scale = torch.rand(K, generator=g) + 0.5
        self.xt, self.wt = x.to(self.dev), self.w.to(self.dev)
        self.bt, self.st = self.bias.to(self.dev), self.scale.to(self.dev)
        self.taps = pkg.filter_pack_s2(self.wt)
        self.N, self.Hin, self.Win, self.C, self.K = N, Hin, Win, C, K
        self.H, self.W = (Hin - 1) // 2 + 1, (Win - 1) // 2 + 1

    def run(self, relu=True):
        out = self.torch.full((self.N, self.H + 2, self.W + 2, self.K), float("nan"), device=self.dev)
        return self.pkg.conv3x3_s2_bn_relu(self.xt, self.taps, self.bt, self.st, relu=relu, out=out)

    def reference(self, idx=None, relu=True):
        """fp64 on the CPU: interior of the padded input -> conv2d(stride 2, padding 1) -> BN -> ReLU, [n][H][W][K]."""
        torch = self.torch
        x = self.x if idx is None else self.x[idx]
        xin = x[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).double()
        y = torch.nn.functional.conv2d(xin, self.w.double(), stride=2, padding=1)
        y = y * self.scale.double()[None, :, None, None] + self.bias.double()[None, :, None, None]
        if relu:
            y = torch.relu(y)
        return y.permute(0, 2, 3, 1).numpy()

    def check(self, O, got, idx=None, relu=True):
        g = got.cpu().numpy()
        if idx is not None:
            g = g[idx]
        assert np.isfinite(g).all()
        ring = np.ones((self.H + 2, self.W + 2), bool)
        ring[1:-1, 1:-1] = False
        assert (g[:, ring, :] == 0).all(), "output ring is not zero"
        want = self.reference(idx, relu)
        assert O.rel_error(g[:, 1:-1, 1:-1, :], want) < TIGHT
        if relu:
            assert (want > 0).mean() > 0.2   # both sides of the ReLU


STAGES = {"conv3": (56, 56, 128, 128), "conv4": (28, 28, 256, 256), "conv5": (14, 14, 512, 512)}


@pytest.mark.parametrize("N", [1, 2, 8])
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_stage_shapes(stage, N, pkg, O, torch_dev):
    """The 3x3 of ResNet-50's v1.5 stage-entry blocks (56->28, 28->14, 14->7) at a few images."""
    Hin, Win, C, K = STAGES[stage]
    layer = _Layer(pkg, torch_dev, N, Hin, Win, C, K, seed=Hin * 10 + N)
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
    layer = _Layer(pkg, torch_dev, N, Hin, Win, C, K, seed=N + Hin * Win + C)
    layer.check(O, layer.run())
    layer.check(O, layer.run(relu=False), relu=False)


def test_conv4_at_128_images(pkg, O, torch_dev):
    """N = 128 (the tiled kernel), sampled images against the fp64 reference, all of it against the 3x3 comparator
    kernel applied at stride 1 and subsampled."""
    torch, dev = torch_dev
    Hin, Win, C, K = STAGES["conv4"]
    layer = _Layer(pkg, torch_dev, 128, Hin, Win, C, K, seed=4128)
    got = layer.run()
    layer.check(O, got, idx=[0, 63, 127])
    full = pkg.conv3x3_direct(layer.xt, layer.wt, layer.bt, layer.st, True)   # stride 1, [N][Hin+2][Win+2][K]
    want = full[:, 1:-1:2, 1:-1:2, :]
    assert O.rel_error(got[:, 1:-1, 1:-1, :].cpu().numpy(), want.cpu().numpy()) < TIGHT
    assert pkg.tickets_in_use() == 0


# (knob settings) -> a forced form
FORMS = {f"latency_ks{ks}_rt{rt}_ct{ct}": {"WINO_1X1_ALGO": "small", "WINO_1X1_SMALL_KS": ks, "WINO_1X1_SMALL_RT": rt,
                                          "WINO_1X1_SMALL_CT": ct}
         for ks in (1, 2, 4) for rt in (1, 2) for ct in (1, 2, 4)}
FORMS.update({
    "tiled": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 0},
    "stream_k": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1},
    # ranges that start and end inside taps (C / 32 k-steps per tap)
    "split_24": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1, "WINO_1X1_SK_GRID": 24},
    "split_40": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1, "WINO_1X1_SK_GRID": 40},
    "split_104": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1, "WINO_1X1_SK_GRID": 104},
})
# (N, Hin, Win, C, K): 8-wave tiles (K = 256) with 2 k-steps per tap, 4-wave tiles (K = 128) with 3 per tap
FORM_SHAPES = [(2, 28, 28, 64, 256), (3, 15, 13, 96, 128)]


def _legal(form, shape):
    """The latency forms the planner accepts for this shape (conv1x1.hip small1_legal): K = 9C in 16-channel chunks per
    wave, the workgroup's columns a divisor of K."""
    kn = FORMS[form]
    if kn["WINO_1X1_ALGO"] != "small":
        return True
    C, K, ks, ct = shape[3], shape[4], kn["WINO_1X1_SMALL_KS"], kn["WINO_1X1_SMALL_CT"]
    return (9 * C) % (16 * ks) == 0 and K % ((4 // ks) * ct * 16) == 0


@pytest.mark.parametrize("form,shape", [(f, s) for s in FORM_SHAPES for f in sorted(FORMS) if _legal(f, s)])
def test_forced_forms(form, shape, pkg, O, torch_dev, knobs):
    """Every form of both kernel families against the reference, and bitwise equal from launch to launch."""
    torch, _ = torch_dev
    for k, v in FORMS[form].items():
        knobs.set(k, v)
    N, Hin, Win, C, K = shape
    want = {"latency": pkg.FORM_LATENCY, "tiled": pkg.FORM_TILED}.get(form.split("_")[0], pkg.FORM_STREAM_K)
    ks = FORMS[form].get("WINO_1X1_SMALL_KS", 1)
    assert pkg.conv3x3_s2_plan(N, Hin, Win, C, K) == want
    if want == pkg.FORM_LATENCY:
        assert pkg.small_plan_1x1_full(N * ((Hin + 1) // 2) * ((Win + 1) // 2), 9 * C, K)[1:4] == (
            ks, FORMS[form]["WINO_1X1_SMALL_RT"], FORMS[form]["WINO_1X1_SMALL_CT"])
    layer = _Layer(pkg, torch_dev, N, Hin, Win, C, K, seed=N * Hin + C)
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
    N, Hin, Win, C, K = FORM_SHAPES[0]
    layer = _Layer(pkg, torch_dev, N, Hin, Win, C, K, seed=99)
    assert pkg.conv3x3_s2_plan(N, Hin, Win, C, K) == pkg.FORM_STREAM_K
    n_tickets = ((N * 14 * 14 + 111) // 112) * (K // 128)   # row tiles x column blocks
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ref = layer.run().clone()
        layer.check(O, ref)
        assert pkg.tickets_in_use() == 0
        pkg.stream_check()
        for i in range(n_tickets):
            pkg.poison_ticket(i, 1)
        layer.run()   # computes with dirty counters: its result is not to be trusted, and it must say so
        with pytest.raises(pkg.WinoError, match="rc=-4"):
            pkg.stream_check()
        with pytest.raises(pkg.WinoError, match="rc=-4"):
            layer.run()
        pkg.stream_reset_scratch()
        pkg.stream_check()
        assert pkg.tickets_in_use() == 0
        for _ in range(2):
            assert torch.equal(layer.run(), ref)
        assert pkg.tickets_in_use() == 0
    torch.cuda.synchronize()


def test_bad_arguments_raise(pkg, torch_dev):
    torch, dev = torch_dev
    layer = _Layer(pkg, torch_dev, 1, 14, 14, 64, 128, seed=3)
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
