"""NaN and Inf sent through the kernels' arithmetic ("Non-finite values"): one poisoned element per
launch, at the pixels next to an image boundary, at a corner, an edge and the centre, in the first and the last
channel, in a weight, a BN bias and a BN scale; every layer in every launch form of the existing form tables, at the
smallest shapes at which one work item holds several images.  tests/nonfinite.py holds the plan, the footprints and the
checker, and tests/test_nonfinite_host.py proves them against torch on the CPU.  Per launch: reference NaN -> NaN,
reference Inf -> that Inf (or NaN behind a Winograd transform); outside the footprint bit for bit the clean launch;
inside it non-finite or within the layer's tolerance; the stream's state check passes.

Blocks and whole networks: a poisoned pixel in image 1 leaves image 0 bitwise the clean run's and makes image 1
non-finite wherever the fp64 forward is, which for the classifiers is every logit."""
import pytest

import nonfinite as NF
import shape_sweeps as S
from cases import PROJ_FORMS, S2_FORMS, s2_legal
from forms_1x1 import FORMS, knobs_set, takes
from fpn_reference import fpn_random_state_dict, fpn_reference_forward
from gpu_support import R, V, torch_dev  # noqa: F401
from nonfinite import NAN, s2_out
from reference_nets import NET_TOL, random_state_dict, reference_forward, vgg_random_state_dict, vgg_reference_forward

pytestmark = pytest.mark.gpu


def _run(pkg, knobs, torch_dev, layer, forms, seed):
    """One layer under every form of `forms` ({name: (knobs, takes())}) that the plan takes; returns the forms run."""
    torch, dev = torch_dev
    plan = NF.Plan(layer, seed)
    ran = []
    for form, (kv, taken) in forms.items():
        with knobs_set(knobs, kv):
            if taken():
                ran.append(form)
                NF.run_plan(pkg, torch, dev, plan, form)
    return ran


# ---- the fused F(2x2) 3x3 -----------------------------------------------------------------------------------------------
def _takes_3x3(pkg, form, kv, N, H, W, C, K):
    """Does the plan, under the knobs set, take the forced form?  (As shape_sweeps.check_forced asks.)"""
    kind, d = S.plan_3x3(pkg, N, H, W, C, K)
    if form == "auto":
        return True
    if form.startswith("big"):
        return kind == "throughput" and d["grid"] == kv["WINO_SK_GRID"] and (d["tail"] > 0) == (form == "big_tail")
    return kind == "latency" and d == {"split": kv["WINO_SMALL_SPLIT"], "ct": kv["WINO_SMALL_CT"]}


@pytest.mark.parametrize("N,H,W", NF.SHAPES_3X3, ids=["3x7x5", "3x6x6"])
@pytest.mark.parametrize("mode", list(NF.MODES_3X3))
def test_fused_3x3(mode, N, H, W, pkg, knobs, torch_dev):
    torch, _ = torch_dev
    ran = set()
    for i, layer in enumerate(NF.layers_3x3(torch, mode, N, H, W)):
        C, K = layer.shape[3:]
        forms = {f: (kv, lambda f=f, kv=kv: _takes_3x3(pkg, f, kv, N, H, W, C, K))
                 for f, kv in NF.forms_3x3(N, H, W, K).items()}
        got = _run(pkg, knobs, torch_dev, layer, forms, seed=100 + i)
        assert {"auto", "big_tail", "big_whole"} <= set(got), (layer.tag, got)
        assert C % 16 or {"small_split1", "small_split2"} <= set(got), (layer.tag, got)
        ran |= set(got)
    assert ran == set(NF.forms_3x3(N, H, W, 64)), ran


# ---- the 1x1 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cin,Kout", NF.CHANNELS_1X1)
@pytest.mark.parametrize("N,H,W", NF.SHAPES_1X1, ids=["3x7x5", "3x14x14", "1x1x1"])
def test_1x1_in_every_form(N, H, W, Cin, Kout, pkg, knobs, torch_dev):
    torch, _ = torch_dev
    forms = {f: (kv, lambda f=f: takes(pkg, f, N * H * W, Cin, Kout)) for f, kv in FORMS.items()}
    for i, layer in enumerate(NF.layers_1x1(torch, N, H, W, Cin, Kout)):
        ran = _run(pkg, knobs, torch_dev, layer, forms, seed=200 + i)
        assert {"auto", "tiled"} <= set(ran) and any(f.startswith("latency") for f in ran), (layer.tag, ran)
        if (N, H, W, Cin, Kout) == (3, 14, 14, 160, 256):
            assert "sk8" in ran and "sk24" in ran, ran


# ---- the stride-2 3x3 and the fused shortcut ----------------------------------------------------------------------------
def test_stride2_3x3_and_fused_shortcut(pkg, knobs, torch_dev):
    torch, _ = torch_dev
    N, Hin, Win, C, K = NF.S2_SHAPE
    M = N * s2_out(Hin) * s2_out(Win)

    def taken(form):
        if not s2_legal(form, NF.S2_SHAPE):
            return False
        kv = S2_FORMS[form]
        planned = S.FORM_NAMES[pkg.conv3x3_s2_plan(N, Hin, Win, C, K)]
        if kv["WINO_1X1_ALGO"] == "small":
            want = (kv["WINO_1X1_SMALL_KS"], kv["WINO_1X1_SMALL_RT"], kv["WINO_1X1_SMALL_CT"])
            return planned == "latency" and tuple(pkg.small_plan_1x1_full(M, 9 * C, K, S.CUS)[1:4]) == want
        return planned == ("tiled" if form == "tiled" else "stream_k")

    forms = {"auto": ({}, lambda: True)}
    forms.update({f: (kv, lambda f=f: taken(f)) for f, kv in S2_FORMS.items()})
    for i, layer in enumerate(NF.layers_s2(torch)):
        ran = _run(pkg, knobs, torch_dev, layer, forms, seed=300 + i)
        assert "tiled" in ran and any(f.startswith("latency") for f in ran) and \
            any(f in ran for f in ("stream_k", "split_24", "split_40", "split_104")), (layer.tag, ran)


# ---- the grouped 3x3 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W", NF.SHAPES_GROUPED, ids=["3x7x5", "3x9x8", "3x6x12", "3x5x20"])
def test_grouped_3x3(N, H, W, pkg, knobs, torch_dev):
    """(A poisoned activation channel's footprint is its own group: every other group stays bitwise clean.)"""
    torch, _ = torch_dev
    for i, layer in enumerate(NF.layers_grouped(torch, N, H, W)):
        assert _run(pkg, knobs, torch_dev, layer, {"auto": ({}, lambda: True)}, seed=400 + i) == ["auto"]


# ---- the stem, the head, image_pack, avgpool7_flatten ---------------------------------------------------------------------
def test_stem(pkg, knobs, torch_dev):
    torch, _ = torch_dev
    for i, layer in enumerate(NF.layers_stem(torch)):
        N, H, W, K = layer.shape
        forms = {"auto": ({}, lambda: True)}
        forms.update({name: ({"WINO_STEM_FORM": f}, lambda f=f: pkg.stem_plan(N, H, W, K) == f)
                      for name, f in (("big", 1), ("small", 2))})
        assert _run(pkg, knobs, torch_dev, layer, forms, seed=500 + i) == ["auto", "big", "small"], layer.tag


def test_head(pkg, knobs, torch_dev):
    torch, _ = torch_dev
    ran = set()
    for i, layer in enumerate(NF.layers_head(torch)):
        N, H, W, C, classes = layer.shape
        forms = {"auto": ({}, lambda: True)}
        forms.update({f: (kv, lambda f=f: S.form_1x1(pkg, N, C, S.head_cols(classes)) == f)
                      for f, kv in S.HEAD_FORMS.items()})
        got = _run(pkg, knobs, torch_dev, layer, forms, seed=600 + i)
        assert {"auto", "latency", "tiled"} <= set(got), (layer.tag, got)
        ran |= set(got)
    assert "stream_k" in ran, ran


def test_image_pack_and_avgpool7(pkg, knobs, torch_dev):
    torch, _ = torch_dev
    for i, layer in enumerate(NF.layers_pack(torch)):
        _run(pkg, knobs, torch_dev, layer, {"auto": ({}, lambda: True)}, seed=700 + i)


# ---- blocks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(len(NF.BLOCKS)), ids=NF.BLOCKS)
def test_block_keeps_a_poisoned_image_to_itself(which, pkg, knobs, torch_dev):
    torch, _ = torch_dev
    layer = list(NF.blocks(torch))[which]
    assert layer.tag.startswith(NF.BLOCKS[which])
    forms = {"auto": ({}, lambda: True)}
    # the strided and the two-operand 1x1 launches in each of their forms, the plan asked that it takes them
    table = {"proj_block": {f: PROJ_FORMS[f] for f in ("tiled", "latency", "split_24")},
             "proj_block_v15": S.V15_FORMS}.get(NF.BLOCKS[which], {})
    for f, kv in table.items():
        case = S.Case(NF.BLOCKS[which], layer.case_shape, dict(kv), f)
        forms[f] = (kv, lambda case=case: S.check_forced(case, S.plan_form(pkg, case)) is None)
    ran = _run(pkg, knobs, torch_dev, layer, forms, seed=800 + which)
    assert ran == list(forms), (layer.tag, ran)


# ---- whole networks ---------------------------------------------------------------------------------------------------------
def _poisoned_input(torch, N, H, W, seed):
    x = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(seed)) * 2 - 1
    xp = x.clone()
    xp[1, 1, H // 2, W // 2] = NAN
    return x, xp


def _check_outputs(torch, clean, got, want, tag):
    """{name: NHWC or [N][classes]}: image 0 bitwise the clean run's, image 1 NaN wherever the fp64 forward's is."""
    for k in want:
        as4 = lambda t: t.reshape(t.shape[0], 1, 1, -1) if t.dim() == 2 else t
        c, g, w = as4(clean[k]), as4(got[k]), as4(want[k].contiguous())
        NF.check_poisoned(torch, c, g, w, NF.box(torch, tuple(w.shape), 1), NET_TOL, f"[{tag} {k}]")


def _forward(model, x, dev):
    out = model(x.to(dev))
    out = out if isinstance(out, dict) else {"logits": out}
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("arch", ["resnet18", "resnext50_32x4d"])
def test_resnet_keeps_a_nan_pixel_to_its_image(arch, pkg, R, torch_dev):
    torch, dev = torch_dev
    sd = random_state_dict(torch, R, arch, classes=10, seed=len(arch))
    model = pkg.ResNet.from_state_dict(sd, arch)
    x, xp = _poisoned_input(torch, 2, 64, 64, seed=9)
    clean, got = _forward(model, x, dev), _forward(model, xp, dev)
    pkg.stream_check()
    want = reference_forward(torch, sd, xp)[0]
    assert bool(torch.isnan(want[1]).all()) and bool(torch.isfinite(want[0]).all())
    _check_outputs(torch, clean, got, {"logits": want}, arch)
    assert pkg.tickets_in_use() == 0
    assert all(torch.equal(a, b) for a, b in zip(_forward(model, x, dev).values(), clean.values())), "a NaN left state behind"


def test_vgg_keeps_a_nan_pixel_to_its_image(pkg, V, torch_dev):
    torch, dev = torch_dev
    arch = "vgg11_bn"
    sd = vgg_random_state_dict(torch, V, arch, classes=10, hidden=256, seed=11)
    model = pkg.VGG.from_state_dict(sd, arch)
    x, xp = _poisoned_input(torch, 2, 32, 32, seed=10)
    clean, got = _forward(model, x, dev), _forward(model, xp, dev)
    pkg.stream_check()
    want = vgg_reference_forward(torch, V, sd, arch, xp)[0]
    assert bool(torch.isnan(want[1]).all()) and bool(torch.isfinite(want[0]).all())
    _check_outputs(torch, clean, got, {"logits": want}, arch)
    assert pkg.tickets_in_use() == 0


def test_resnet_fpn_keeps_a_nan_pixel_to_its_image(pkg, R, torch_dev):
    torch, dev = torch_dev
    sd, body = fpn_random_state_dict(torch, R, "resnet18", seed=8)
    model = pkg.ResNetFPN.from_state_dict(sd, "resnet18")
    x, xp = _poisoned_input(torch, 2, 64, 64, seed=12)
    clean, got = _forward(model, x, dev), _forward(model, xp, dev)
    pkg.stream_check()
    want = fpn_reference_forward(torch, sd, body, xp)
    assert sorted(want) == sorted(got) == ["0", "1", "2", "3", "pool"]
    assert all(bool(torch.isnan(w[1]).any()) for w in want.values())
    _check_outputs(torch, clean, got, want, "resnet18-fpn")
    assert pkg.tickets_in_use() == 0


def test_resnet18_graph_replay_keeps_a_nan_pixel_to_its_image(pkg, R, torch_dev):
    """One captured forward over a static input: replayed on the poisoned input it gives what the eager run gives, and
    replayed on the clean input again it is bitwise the clean logits (the NaN left nothing behind)."""
    torch, dev = torch_dev
    arch = "resnet18"
    sd = random_state_dict(torch, R, arch, classes=10, seed=21)
    model = pkg.ResNet.from_state_dict(sd, arch)
    x, xp = _poisoned_input(torch, 2, 64, 64, seed=13)
    xs = x.to(dev)
    sg = torch.cuda.Stream()
    with torch.cuda.stream(sg):
        model.prepare(2, 64, 64)
        clean = model(xs).clone()
    sg.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=sg):
        out = model(xs)
    xs.copy_(xp)
    graph.replay()
    torch.cuda.synchronize()
    got = out.clone()
    want = reference_forward(torch, sd, xp)[0]
    _check_outputs(torch, {"logits": clean}, {"logits": got}, {"logits": want}, "resnet18 graph")
    xs.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, clean)
    with torch.cuda.stream(sg):
        assert pkg.tickets_in_use() == 0
        pkg.stream_check()
    del graph
