"""GPU tests of the downsampling basic block: the fused stride-2 3x3 + 1x1 stride-2 shortcut layer
(wino_conv3x3_s2_proj_bn_relu_hw, the 1x1 kernels in operand form A_TAPS_PROJ) and the block on it
(wino_basic_block_s2_hw).  Outputs go into NaN-filled buffers and are compared with fp64 references built here (torch on
the CPU); t1 bitwise against the plain stride-2 layer in every forced form; the block against a torchvision-style
BasicBlock with `downsample`; odd and tiny maps; a ResNet-18 stage opening; graph replay; the stream-K fail-fast
contract; Python argument errors."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TIGHT = 2e-5

# the downsampling blocks of ResNet-18 / -34: (Hin, C, K), stride 2 on the first 3x3 and on the 1x1 shortcut
STAGES = {"conv3": (56, 64, 128), "conv4": (28, 128, 256), "conv5": (14, 256, 512)}


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch, torch.device("cuda:0")


def _ring(H, W):
    ring = np.ones((H + 2, W + 2), bool)
    ring[1:-1, 1:-1] = False
    return ring


class _Block:
    """One downsampling block's parameters (CPU masters, device copies, the packed buffer) and its fp64 reference."""

    def __init__(self, pkg, torch_dev, N, Hin, Win, C, K, seed):
        self.torch, self.dev = torch_dev
        torch = self.torch
        self.pkg = pkg
        g = torch.Generator(device="cpu").manual_seed(seed)
        x = torch.zeros(N, Hin + 2, Win + 2, C)
        x[:, 1:-1, 1:-1, :] = torch.rand(N, Hin, Win, C, generator=g) - 0.5
        self.x = x
        self.w1 = (torch.rand(K, C, 3, 3, generator=g) - 0.5) / np.sqrt(9 * C) * 4
        self.wd = (torch.rand(K, C, 1, 1, generator=g) - 0.5) / np.sqrt(C) * 4
        self.w2 = (torch.rand(K, K, 3, 3, generator=g) - 0.5) / np.sqrt(9 * K) * 4
        vec = lambda lo: torch.rand(K, generator=g) + lo
        self.b1, self.s1 = vec(-0.5), vec(0.5)
        self.bd, self.sd = vec(-0.5), vec(0.5)
        self.b2, self.s2 = vec(-0.5), vec(0.5)
        t = lambda a: a.contiguous().to(self.dev)
        self.xt = t(x)
        self.taps = pkg.filter_pack_s2(t(self.w1))
        self.packed = pkg.s2_proj_pack(self.taps, (t(self.b1), t(self.s1)), t(self.wd.view(K, C).t()),
                                       (t(self.bd), t(self.sd)))
        self.U2 = pkg.filter_transform_f2(t(self.w2))
        self.bn1 = (t(self.b1), t(self.s1))
        self.bn2 = (t(self.b2), t(self.s2))
        self.N, self.Hin, self.Win, self.C, self.K = N, Hin, Win, C, K
        self.H, self.W = (Hin - 1) // 2 + 1, (Win - 1) // 2 + 1

    def nan(self):
        return self.torch.full((self.N, self.H + 2, self.W + 2, self.K), float("nan"), device=self.dev)

    def layer(self):
        return self.pkg.conv3x3_s2_proj(self.xt, self.packed, t1=self.nan(), sc=self.nan())

    def plain(self):
        return self.pkg.conv3x3_s2_bn_relu(self.xt, self.taps, *self.bn1, relu=True, out=self.nan())

    def block(self, out=None, workspace=None):
        return self.pkg.basic_block_s2(self.xt, self.packed, self.U2, self.bn2,
                                       out=self.nan() if out is None else out, workspace=workspace)

    def reference(self, idx=None, block=True):
        """fp64 on the CPU: (t1, sc, out), each [n][H][W][K] (out None unless `block`)."""
        torch = self.torch
        F = torch.nn.functional
        x = self.x if idx is None else self.x[idx]
        xin = x[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).double()
        bn = lambda y, s, b: y * s.double()[None, :, None, None] + b.double()[None, :, None, None]
        t1 = torch.relu(bn(F.conv2d(xin, self.w1.double(), stride=2, padding=1), self.s1, self.b1))
        sc = bn(F.conv2d(xin, self.wd.double(), stride=2), self.sd, self.bd)
        nhwc = lambda y: y.permute(0, 2, 3, 1).numpy()
        if not block:
            return nhwc(t1), nhwc(sc), None
        out = torch.relu(bn(F.conv2d(t1, self.w2.double(), padding=1), self.s2, self.b2) + sc)
        return nhwc(t1), nhwc(sc), nhwc(out)

    def check_layer(self, O, t1, sc, idx=None):
        a, b = t1.cpu().numpy(), sc.cpu().numpy()
        if idx is not None:
            a, b = a[idx], b[idx]
        ring = _ring(self.H, self.W)
        assert np.isfinite(a).all()
        assert (a[:, ring, :] == 0).all(), "t1's ring is not zero"
        assert np.isfinite(b[:, 1:-1, 1:-1, :]).all(), "sc's interior is not all written"
        assert np.isnan(b[:, ring, :]).all(), "sc's ring was written"
        want_t1, want_sc, _ = self.reference(idx, block=False)
        assert O.rel_error(a[:, 1:-1, 1:-1, :], want_t1) < TIGHT
        assert O.rel_error(b[:, 1:-1, 1:-1, :], want_sc) < TIGHT
        assert (want_t1 > 0).mean() > 0.2 and (want_sc < 0).mean() > 0.2   # both sides of t1's ReLU; sc has none

    def check_block(self, O, out, idx=None):
        g = out.cpu().numpy()
        if idx is not None:
            g = g[idx]
        assert np.isfinite(g).all()
        assert (g[:, _ring(self.H, self.W), :] == 0).all(), "out's ring is not zero"
        want = self.reference(idx)[2]
        assert O.rel_error(g[:, 1:-1, 1:-1, :], want) < TIGHT
        assert (want > 0).mean() > 0.2


LAYER_POINTS = [(s, n) for s in sorted(STAGES) for n in (1, 2, 8, 32)] + [("conv4", 128)]


@pytest.mark.parametrize("stage,N", LAYER_POINTS)
def test_fused_layer_at_stage_shapes(stage, N, pkg, O, torch_dev):
    """t1 and sc of the fused layer against fp64, and t1 bitwise the plain stride-2 layer's output."""
    torch, _ = torch_dev
    Hin, C, K = STAGES[stage]
    blk = _Block(pkg, torch_dev, N, Hin, Hin, C, K, seed=Hin * 1000 + N)
    t1, sc = blk.layer()
    blk.check_layer(O, t1, sc, idx=None if N <= 32 else [0, 77, 127])
    assert torch.equal(t1, blk.plain())
    assert pkg.tickets_in_use() == 0


# (knob settings) -> a forced form, as in test_gpu_conv3x3_s2.py
FORMS = {f"latency_ks{ks}_rt{rt}_ct{ct}": {"WINO_1X1_ALGO": "small", "WINO_1X1_SMALL_KS": ks, "WINO_1X1_SMALL_RT": rt,
                                          "WINO_1X1_SMALL_CT": ct}
         for ks in (1, 2, 4) for rt in (1, 2) for ct in (1, 2, 4)}
FORMS.update({
    "tiled": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 0},
    "stream_k": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1},
    # ranges that start and end inside taps, the centre tap's included
    "split_24": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1, "WINO_1X1_SK_GRID": 24},
    "split_40": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1, "WINO_1X1_SK_GRID": 40},
    "split_104": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1, "WINO_1X1_SK_GRID": 104},
})
# (N, Hin, Win, C, K): 8-wave tiles (K = 256) with 2 k-steps per tap, 4-wave tiles (K = 128) with 3 per tap
FORM_SHAPES = [(2, 28, 28, 64, 256), (3, 15, 13, 96, 128)]


def _legal(form, shape):
    """The latency forms the planner accepts for this shape (K = 9C in 16-channel chunks per wave, the workgroup's
    columns a divisor of K)."""
    kn = FORMS[form]
    if kn["WINO_1X1_ALGO"] != "small":
        return True
    C, K, ks, ct = shape[3], shape[4], kn["WINO_1X1_SMALL_KS"], kn["WINO_1X1_SMALL_CT"]
    return (9 * C) % (16 * ks) == 0 and K % ((4 // ks) * ct * 16) == 0


@pytest.mark.parametrize("form,shape", [(f, s) for s in FORM_SHAPES for f in sorted(FORMS) if _legal(f, s)])
def test_forced_forms(form, shape, pkg, O, torch_dev, knobs):
    """In every form: t1 bitwise the plain layer's, sc against fp64, both bitwise from launch to launch."""
    torch, _ = torch_dev
    for k, v in FORMS[form].items():
        knobs.set(k, v)
    N, Hin, Win, C, K = shape
    want = {"latency": pkg.FORM_LATENCY, "tiled": pkg.FORM_TILED}.get(form.split("_")[0], pkg.FORM_STREAM_K)
    assert pkg.conv3x3_s2_plan(N, Hin, Win, C, K) == want
    blk = _Block(pkg, torch_dev, N, Hin, Win, C, K, seed=N * Hin + C)
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
    blk = _Block(pkg, torch_dev, N, Hin, Hin, C, K, seed=7 * Hin + N)
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
    blk = _Block(pkg, torch_dev, N, Hin, Win, C, K, seed=N + Hin * Win + C)
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
    blk = _Block(pkg, torch_dev, N, Hin, Hin, C, K, seed=1804 + N)
    g = torch.Generator(device="cpu").manual_seed(N)
    w3 = (torch.rand(K, K, 3, 3, generator=g) - 0.5) / np.sqrt(9 * K) * 4
    w4 = (torch.rand(K, K, 3, 3, generator=g) - 0.5) / np.sqrt(9 * K) * 4
    b3, s3, b4, s4 = (torch.rand(K, generator=g) + lo for lo in (-0.5, 0.5, -0.5, 0.5))
    t = lambda a: a.contiguous().to(dev)
    y = blk.block()
    out = pkg.basic_block(y, pkg.filter_transform_f2(t(w3)), (t(b3), t(s3)), pkg.filter_transform_f2(t(w4)),
                          (t(b4), t(s4)), out=y)
    assert out.data_ptr() == y.data_ptr()
    F = torch.nn.functional
    bn = lambda v, s, b: v * s.double()[None, :, None, None] + b.double()[None, :, None, None]
    y0 = torch.from_numpy(blk.reference()[2]).permute(0, 3, 1, 2)
    u = torch.relu(bn(F.conv2d(y0, w3.double(), padding=1), s3, b3))
    want = torch.relu(bn(F.conv2d(u, w4.double(), padding=1), s4, b4) + y0).permute(0, 2, 3, 1).numpy()
    g_ = out.cpu().numpy()
    assert (g_[:, _ring(blk.H, blk.W), :] == 0).all()
    assert O.rel_error(g_[:, 1:-1, 1:-1, :], want) < TIGHT


@pytest.mark.parametrize("stage,N", [("conv3", 1), ("conv4", 32)])
def test_block_in_a_graph(stage, N, pkg, O, torch_dev):
    """The two launches captured into one graph (one stream) after basic_block_s2_prepare: the replay is bitwise the
    eager result."""
    torch, dev = torch_dev
    Hin, C, K = STAGES[stage]
    blk = _Block(pkg, torch_dev, N, Hin, Hin, C, K, seed=4242 + N)
    eager = blk.block().clone()
    out = torch.zeros_like(eager)
    ws = torch.empty(pkg.lib().wino_basic_block_s2_workspace_bytes_hw(N, Hin, Hin, K) // 4, device=dev)
    sg = torch.cuda.Stream()
    with torch.cuda.stream(sg):
        pkg.basic_block_s2_prepare(N, Hin, Hin, C, K)
    sg.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=sg):
        blk.block(out=out, workspace=ws)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    with torch.cuda.stream(sg):
        assert pkg.tickets_in_use() == 0
    blk.check_block(O, eager)


def test_a_dirty_ticket_counter_is_reported_and_reset_recovers(pkg, O, torch_dev, knobs):
    """The fused layer in the forced stream-K form keeps the fail-fast contract: a ticket counter left non-zero is
    reported, every launch on the stream then fails with WINO_E_STATE, and wino_stream_reset_scratch() recovers
    bitwise results.  The shortcut's appended tiles never touch the tickets."""
    torch, dev = torch_dev
    knobs.set("WINO_1X1_ALGO", "big")
    knobs.set("WINO_1X1_SK", 1)
    N, Hin, Win, C, K = FORM_SHAPES[0]
    blk = _Block(pkg, torch_dev, N, Hin, Win, C, K, seed=99)
    assert pkg.conv3x3_s2_plan(N, Hin, Win, C, K) == pkg.FORM_STREAM_K
    n_tickets = ((N * 14 * 14 + 111) // 112) * (K // 128)   # row tiles x column blocks
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t1, sc = blk.layer()
        t1, sc = t1.clone(), sc.clone()
        blk.check_layer(O, t1, sc)
        assert pkg.tickets_in_use() == 0
        pkg.stream_check()
        for i in range(n_tickets):
            pkg.poison_ticket(i, 1)
        blk.layer()   # computes with dirty counters: its result is not to be trusted, and it must say so
        with pytest.raises(pkg.WinoError, match="rc=-4"):
            pkg.stream_check()
        with pytest.raises(pkg.WinoError, match="rc=-4"):
            blk.layer()
        with pytest.raises(pkg.WinoError, match="rc=-4"):
            blk.block()
        pkg.stream_reset_scratch()
        pkg.stream_check()
        assert pkg.tickets_in_use() == 0
        for _ in range(2):
            a, b = blk.layer()
            assert torch.equal(a, t1)
            assert torch.equal(b[:, 1:-1, 1:-1, :], sc[:, 1:-1, 1:-1, :])
        blk.check_block(O, blk.block())
        assert pkg.tickets_in_use() == 0
    torch.cuda.synchronize()


def test_bad_arguments_raise(pkg, torch_dev):
    torch, dev = torch_dev
    blk = _Block(pkg, torch_dev, 1, 14, 14, 64, 128, seed=3)
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
