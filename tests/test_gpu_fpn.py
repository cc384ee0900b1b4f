"""GPU tests of the FPN neck: the 1x1 layer with the upsampled residual (WINO_RESIDUAL_UP2) in every launch form at
the smallest shapes that exercise each index path, against fp64 with F.interpolate(nearest) at 2e-5, the coarse map's
ring NaN; the same layer between guards; the stream-K form's hand-off state; one pyramid level; and whole ResNet-FPN
backbones against an fp64 CPU forward of torchvision's BackboneWithFPN."""
import pytest

import guarded as G
import shape_sweeps as S
from cases import TIGHT
from forms_1x1 import FORMS, knobs_set as _knobs, sk_plan as _sk_plan, takes as _takes
from fpn_reference import (LAYER_TOL, Up2Layer, fpn_random_state_dict, fpn_reference_forward, level_reference,
                           padded_nan, up_hw)
from gpu_support import (R, dirty_ticket_scenario, graph_replay_scenario, network_graph_scenario, rel,  # noqa: F401
                         torch_dev)
from layer_refs import ring_is
from reference_nets import NET_TOL

pytestmark = pytest.mark.gpu

# (N, H, W): 5 1/4 row tiles of 112 that cross image boundaries; odd, the last row and column read a coarse pixel
# alone; H != W; a single pixel; 2x3 over 1x2
SHAPES = [(3, 14, 14), (2, 7, 7), (2, 5, 9), (1, 1, 1), (2, 2, 3)]
CHANNELS = [(32, 64), (64, 128), (160, 256)]   # the last gives the 8-wave workgroups


def _pad_forms(pkg):
    return [a | c | r for a in (0, pkg.A_PADDED) for c in (0, pkg.C_PADDED) for r in (0, pkg.RELU)]


def test_every_form_runs_somewhere():
    """Host arithmetic over the cases below: each latency setting except KS = 4 is legal for one of the issue's channel
    pairs (Cin = 160 is no multiple of 64: KS = 4 runs in test_latency_ks4), the stream-K form is legal at several
    cases and one of its grids cuts tiles."""
    ran = set()
    for N, H, W in SHAPES:
        for Cin, Kout in CHANNELS:
            for g in (8, 24):
                legal, cuts = _sk_plan(N * H * W, Cin, Kout, g)
                if legal:
                    ran.add(("sk", cuts))
            for ks in (1, 2, 4):
                for rt in (1, 2):
                    for ct in (1, 2, 4):
                        if Cin % (16 * ks) == 0 and Kout % ((4 // ks) * ct * 16) == 0 and not (ks > 1 and Cin // ks < 64):
                            ran.add((ks, rt, ct))
    assert ("sk", True) in ran
    assert {k for k in ran if k[0] != "sk"} == {(ks, rt, ct) for ks in (1, 2) for rt in (1, 2) for ct in (1, 2, 4)}
    assert _sk_plan(3 * 14 * 14, 160, 256, 24) == (True, True)


@pytest.mark.parametrize("Cin,Kout", CHANNELS)
@pytest.mark.parametrize("N,H,W", SHAPES, ids=[f"{n}x{h}x{w}" for n, h, w in SHAPES])
def test_layer_parity_in_every_form(N, H, W, Cin, Kout, pkg, knobs, torch_dev):
    torch, dev = torch_dev
    layer = Up2Layer(torch, dev, N, H, W, Cin, Kout, seed=N * 1000 + H * 10 + W + Cin)
    M = N * H * W
    ran = []
    for form, kv in FORMS.items():
        with _knobs(knobs, kv):
            if not _takes(pkg, form, M, Cin, Kout):
                continue
            ran.append(form)
            for flags in _pad_forms(pkg):
                got = layer.run(pkg, flags).clone()
                layer.check(pkg, flags, got, f"[up2 {N}x{H}x{W} {Cin}->{Kout} {form} flags={flags}]")
                assert torch.equal(layer.run(pkg, flags), got), (form, flags)   # bitwise from launch to launch
            assert pkg.tickets_in_use() == 0, form
    assert {"auto", "tiled"} <= set(ran) and any(f.startswith("latency") for f in ran), ran
    if (N, H, W, Cin, Kout) == (3, 14, 14, 160, 256):
        assert "sk8" in ran and "sk24" in ran, ran


def test_latency_ks4(pkg, knobs, torch_dev):
    """The K split over all four waves needs Cin % 64 == 0, which none of the channel pairs above has with a legal
    width: 256 -> 64 at the odd shape."""
    torch, dev = torch_dev
    N, H, W, Cin, Kout = 2, 7, 7, 256, 64
    layer = Up2Layer(torch, dev, N, H, W, Cin, Kout, seed=44)
    for rt in (1, 2):
        with _knobs(knobs, {"WINO_1X1_ALGO": "small", "WINO_1X1_SMALL_KS": 4, "WINO_1X1_SMALL_RT": rt,
                            "WINO_1X1_SMALL_CT": 1}):
            assert pkg.small_plan_1x1_full(N * H * W, Cin, Kout, S.CUS)[:4] == (1, 4, rt, 1)
            for flags in _pad_forms(pkg):
                got = layer.run(pkg, flags).clone()
                layer.check(pkg, flags, got, f"[up2 ks4 rt{rt} flags={flags}]")
                assert torch.equal(layer.run(pkg, flags), got)


def test_bad_arguments_raise(pkg, torch_dev):
    torch, dev = torch_dev
    layer = Up2Layer(torch, dev, 2, 7, 7, 32, 64, seed=1)
    t = layer.dev
    UP = pkg.ADD_RESIDUAL | pkg.RESIDUAL_UP2
    with pytest.raises(pkg.WinoError, match="coarser map"):      # a same-size residual under the flag
        pkg.conv1x1_bn_ex(t["A"], t["B"], t["b"], t["s"], UP, residual=torch.zeros(2, 7, 7, 64, device=dev))
    with pytest.raises(pkg.WinoError, match="coarser map"):      # the coarse map without its ring
        pkg.conv1x1_bn_ex(t["A"], t["B"], t["b"], t["s"], UP, residual=torch.zeros(2, 4, 4, 64, device=dev))
    with pytest.raises(pkg.WinoError, match="ADD_RESIDUAL"):
        pkg.conv1x1_bn_ex(t["A"], t["B"], t["b"], t["s"], pkg.RESIDUAL_UP2, residual=t["top"])
    with pytest.raises(pkg.WinoError, match="rc=-3"):            # the library itself, through the 14x14 M-form
        pkg._check(pkg.lib().wino_conv1x1_bn_ex(t["A"].data_ptr(), t["B"].data_ptr(), t["b"].data_ptr(),
                                                t["s"].data_ptr(), t["top"].data_ptr(), t["A"].data_ptr(), 98, 32, 64,
                                                UP, None), "wino_conv1x1_bn_ex")


# ---- guard bands ------------------------------------------------------------------------------------------------------
GUARDED = [(3, 14, 14, 160, 256), (2, 7, 7, 32, 64), (2, 5, 9, 64, 128), (1, 1, 1, 160, 256)]
GUARDED_FORMS = ["auto", "tiled", "sk8", "sk24", "latency_ks1_rt1_ct1", "latency_ks2_rt2_ct4"]


@pytest.mark.parametrize("shape", GUARDED, ids=["x".join(map(str, s)) for s in GUARDED])
def test_layer_between_guards(shape, pkg, knobs, torch_dev):
    """Every operand on the guarded arena at the 256-byte and the 16-mod-256 placement (inputs between NaN guards,
    the output of exactly its size between sentinel guards): no byte next to a tensor changes, no input is written."""
    torch, dev = torch_dev
    N, H, W, Cin, Kout = shape
    layer = Up2Layer(torch, dev, N, H, W, Cin, Kout, seed=sum(shape))
    ran = []
    for form in GUARDED_FORMS:
        with _knobs(knobs, FORMS[form]):
            if not _takes(pkg, form, N * H * W, Cin, Kout):
                continue
            ran.append(form)
            for flags in (pkg.RELU, pkg.A_PADDED | pkg.C_PADDED, pkg.A_PADDED | pkg.RELU, pkg.C_PADDED | pkg.RELU):
                for align in G.ALIGNS:
                    arena = G.Arena(torch, dev, align=align)
                    t = {k: arena.input(v, name=k) for k, v in layer.cpu.items()
                         if k != ("A" if flags & pkg.A_PADDED else "Ap")}
                    out = arena.output(*layer.out_shape(pkg, flags), name="out")
                    tag = f"[up2 guarded {shape} {form} flags={flags} align={align}]"
                    layer.check(pkg, flags, layer.run(pkg, flags, t=t, out=out), tag)
                    assert pkg.tickets_in_use() == 0, tag
                    arena.check(tag)
    assert len(ran) >= 3, ran


# ---- the stream-K form's hand-off state ---------------------------------------------------------------------------------
def test_a_dirty_ticket_counter_is_reported_and_reset_recovers(pkg, knobs, torch_dev):
    """The upsampled-residual epilogue is a new instantiation of the ticket code: a counter left non-zero is reported,
    every launch on the stream then fails with WINO_E_STATE, and wino_stream_reset_scratch() recovers bitwise."""
    torch, dev = torch_dev
    N, H, W, Cin, Kout = 3, 14, 14, 160, 256
    layer = Up2Layer(torch, dev, N, H, W, Cin, Kout, seed=99)
    flags = pkg.C_PADDED | pkg.RELU
    with _knobs(knobs, FORMS["sk24"]):
        assert _takes(pkg, "sk24", N * H * W, Cin, Kout) and _sk_plan(N * H * W, Cin, Kout, 24)[1]
        n_tickets = ((N * H * W + 111) // 112) * (Kout // 128)   # row tiles x column blocks
        dirty_ticket_scenario(pkg, torch, lambda: layer.run(pkg, flags), n_tickets,
                              check=lambda ref: layer.check(pkg, flags, ref, "[up2 stream-K, clean]"))
        assert pkg.tickets_in_use() == 0


# ---- one level --------------------------------------------------------------------------------------------------------------
class Level:
    def __init__(self, pkg, torch, dev, with_top, c_padded, seed, N=2, H=7, W=7, Cin=64, Cf=64):
        self.pkg, self.torch, self.c_padded, self.shape = pkg, torch, c_padded, (N, H, W, Cin, Cf)
        g = torch.Generator().manual_seed(seed)
        r = lambda *sh: torch.rand(*sh, generator=g)
        Hc, Wc = up_hw(H, W)
        c = r(N, H, W, Cin) - 0.5
        wl = (r(Cf, Cin, 1, 1) - 0.5) / Cin ** 0.5 * 4
        wo = (r(Cf, Cf, 3, 3) - 0.5) / (9 * Cf) ** 0.5 * 4
        bl, bo = r(Cf) - 0.5, r(Cf) - 0.5
        top = r(N, Hc, Wc, Cf) - 0.5 if with_top else None
        self.want = level_reference(torch, c, wl, bl, wo, bo, top)
        d = lambda t: t.to(dev)
        self.c = d(padded_nan(torch, c) if c_padded else c)
        self.wl, self.bl, self.bo = d(wl.reshape(Cf, Cin).t().contiguous()), d(bl), d(bo)
        self.U = pkg.filter_transform_f2(d(wo))
        self.top = d(padded_nan(torch, top)) if with_top else None
        self.ones = torch.ones(Cf, device=dev)

    def run(self, inner=None, out=None):
        N, H, W, _, Cf = self.shape
        full = lambda: self.torch.full((N, H + 2, W + 2, Cf), float("nan"), device=self.c.device)
        return self.pkg.fpn_level(self.c, self.wl, self.bl, self.U, self.bo, top=self.top, c_padded=self.c_padded,
                                  ones=self.ones, inner=full() if inner is None else inner,
                                  out=full() if out is None else out)

    def check(self, inner, P):
        torch = self.torch
        for name, got, want in (("inner", inner, self.want[0]), ("P", P, self.want[1])):
            got = got.cpu()
            assert ring_is(got, 0.0), f"{name}: ring is not exactly 0"
            err = rel(torch, got[:, 1:-1, 1:-1, :], want)
            print(f"fpn_level {name}: rel err {err:.3e}")
            assert err < TIGHT, (name, err)


@pytest.mark.parametrize("c_padded", [False, True], ids=["unpadded", "padded"])
@pytest.mark.parametrize("with_top", [False, True], ids=["coarsest", "top"])
def test_one_level(with_top, c_padded, pkg, torch_dev):
    """7x7 <- 4x4, Cin = 64, Cf = 64: both launches against the fp64 chain at the two-launch blocks' tolerance, then
    the level captured into one graph."""
    torch, dev = torch_dev
    lvl = Level(pkg, torch, dev, with_top, c_padded, seed=10 + 2 * with_top + c_padded)
    N, H, W, Cin, Cf = lvl.shape
    inner, P = lvl.run()
    lvl.check(inner, P)
    inner2, P2 = lvl.run()
    assert torch.equal(inner2, inner) and torch.equal(P2, P)
    assert pkg.tickets_in_use() == 0
    nbytes = N * (H + 2) * (W + 2) * Cf * 4
    run = lambda out=None, workspace=None: lvl.run(
        inner=None if workspace is None else workspace.view(N, H + 2, W + 2, Cf), out=out)[1]
    eager = graph_replay_scenario(pkg, torch_dev, run, lambda: pkg.fpn_level_prepare(N, H, W, Cin, Cf), nbytes)
    assert torch.equal(eager, P)


def test_level_bad_arguments_raise(pkg, torch_dev):
    torch, dev = torch_dev
    lvl = Level(pkg, torch, dev, True, False, seed=3)
    N, H, W, Cin, Cf = lvl.shape
    with pytest.raises(pkg.WinoError, match="top must have shape"):
        pkg.fpn_level(lvl.c, lvl.wl, lvl.bl, lvl.U, lvl.bo, top=torch.zeros(N, H + 2, W + 2, Cf, device=dev))
    buf = torch.zeros(N, H + 2, W + 2, Cf, device=dev)
    with pytest.raises(pkg.WinoError, match="rc=-3"):            # inner is P
        pkg.fpn_level(lvl.c, lvl.wl, lvl.bl, lvl.U, lvl.bo, top=lvl.top, inner=buf, out=buf)
    with pytest.raises(pkg.WinoError, match="w_lat"):
        pkg.fpn_level(lvl.c, lvl.wl[:32].contiguous(), lvl.bl, lvl.U, lvl.bo)


# ---- whole backbones ----------------------------------------------------------------------------------------------------
# N = 2 at 64x64: pyramid 16 / 8 / 4 / 2, pool 1.  N = 1 at 72x104: 18x26 / 9x13 / 5x7 / 3x4, pool 2x2 -- an odd size at
# every top-down step.
NET_INPUTS = [(2, 64, 64), (1, 72, 104)]
_NETS = {}   # arch -> (sd, body, model, {input: (x, fp64 reference)}): built once, shared by the tests below


def _net(pkg, R, torch, dev, arch):
    if arch not in _NETS:
        sd, body = fpn_random_state_dict(torch, R, arch, seed=len(arch))
        model = pkg.ResNetFPN.from_state_dict(sd, arch)
        refs = {}
        for i, (N, H, W) in enumerate(NET_INPUTS):
            x = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(i + 7)) - 0.5
            refs[(N, H, W)] = (x, fpn_reference_forward(torch, sd, body, x))
        _NETS[arch] = (sd, body, model, refs)
    return _NETS[arch]


@pytest.mark.parametrize("shape", NET_INPUTS, ids=["2x64x64", "1x72x104"])
@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_backbone_with_fpn(arch, shape, pkg, R, torch_dev):
    """resnet18 (padded body) and resnet50 (unpadded body) with random weights: all five outputs against the fp64 CPU
    forward at NET_TOL."""
    torch, dev = torch_dev
    _, _, model, refs = _net(pkg, R, torch, dev, arch)
    x, want = refs[shape]
    model.prepare(*shape)
    for t in (*model._inner, *model._p):
        t.fill_(float("nan"))
    out = model(x.to(dev))
    torch.cuda.synchronize()
    assert sorted(out) == sorted(want) == ["0", "1", "2", "3", "pool"]
    sizes = [tuple(out[k].shape[1:3]) for k in ("0", "1", "2", "3", "pool")]
    assert sizes == ([(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)] if shape[1] == 64 else
                     [(18, 26), (9, 13), (5, 7), (3, 4), (2, 2)])
    errs = {k: rel(torch, out[k], want[k]) for k in want}
    print(f"{arch}-fpn {shape}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert not {k: v for k, v in errs.items() if not v < NET_TOL}, errs
    for p in model._p:                                   # the rings of the padded outputs are exactly 0
        assert bool((p[:, 0] == 0).all() and (p[:, -1] == 0).all() and (p[:, :, 0] == 0).all() and (p[:, :, -1] == 0).all())
    assert pkg.tickets_in_use() == 0


class _Finest:
    """The backbone as network_graph_scenario takes a model: one output tensor, the finest level (it depends on the
    whole body and on every lateral); the full dictionary of the last forward stays in .last."""

    def __init__(self, model):
        self.model, self.prepare = model, model.prepare

    def __call__(self, x):
        self.last = self.model(x)
        return self.last["0"]


def test_backbone_in_one_graph(pkg, R, torch_dev):
    torch, dev = torch_dev
    _, _, model, refs = _net(pkg, R, torch, dev, "resnet18")
    x, want = refs[NET_INPUTS[0]]
    wrapped = _Finest(model)
    eager0, graph = network_graph_scenario(pkg, torch, wrapped, x.to(dev))
    assert rel(torch, eager0, want["0"]) < NET_TOL
    # the other levels, replayed into NaN-filled tensors: the captured forward rewrites them all
    outs = wrapped.last
    for t in (*model._inner, *model._p):
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for k in want:
        assert rel(torch, outs[k], want[k]) < NET_TOL, k
    del graph
