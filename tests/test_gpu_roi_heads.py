"""GPU tests of the R-CNN box and mask heads (cuda_winograd_amd.detection) and of the second stage end to end:
ResNetFPN(padded=True) -> multiscale_roi_align -> BoxHead / MaskHead against the fp64 chain of tests/roi_cases.py and
tests/fpn_reference.py at the project's network bar, reference_nets.NET_TOL.  The two sweeps run the heads over
roi_cases.box_head_cases() / mask_head_cases() in the automatic form and with their GEMMs forced into the tiled, the
stream-K and the latency form, and count which form each GEMM took."""
import collections

import pytest
import torch

import roi_cases as rc
import shape_sweeps as S
from cases import PROJ_FORMS
from fpn_reference import fpn_random_state_dict, fpn_reference_forward
from gpu_support import R, rel, torch_dev  # noqa: F401
from reference_nets import NET_TOL

pytestmark = pytest.mark.gpu
C = 64
CANON = dict(canonical_scale=rc.CANONICAL_SCALE, canonical_level=rc.CANONICAL_LEVEL)


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("boxes", [1, 37])
@pytest.mark.parametrize("classes", [5, 91])
def test_box_head(classes, boxes, pkg, torch_dev):
    _, dev = torch_dev
    P, rep = 7, 128
    sd = rc.box_head_state_dict(C, P, rep, classes, seed=classes)
    head = pkg.BoxHead.from_state_dict(sd, in_channels=C, P=P)
    pooled = rc.reference(C, P, 2)[:boxes].float()             # the fp64 reference's pooled tensor, rounded to fp32
    want_cls, want_box = rc.box_head_reference(sd, pooled)
    head.prepare(boxes)
    for t in (head._h6, head._h7, head._scores):
        t.fill_(float("nan"))
    logits, regression = head(pooled.to(dev))
    torch.cuda.synchronize()
    assert tuple(logits.shape) == (boxes, classes) and tuple(regression.shape) == (boxes, 4 * classes)
    # views of one GEMM's output; its zero-padded columns lie behind them
    kp = (5 * classes + 63) // 64 * 64
    assert tuple(head._scores.shape) == (boxes, kp) and logits.data_ptr() == head._scores.data_ptr()
    assert regression.data_ptr() == head._scores.data_ptr() + 4 * classes
    assert bool((head._scores[:, 5 * classes:] == 0).all())
    errs = rel(torch, logits, want_cls), rel(torch, regression, want_box)
    print(f"box head classes={classes} R={boxes}: logits {errs[0]:.2e} regression {errs[1]:.2e}")
    assert max(errs) < NET_TOL
    assert pkg.tickets_in_use() == 0


@pytest.mark.parametrize("boxes", [1, 9])
@pytest.mark.parametrize("P,classes", [(14, 3), (14, 91), (6, 3), (6, 91)])
def test_mask_head(P, classes, boxes, pkg, torch_dev):
    _, dev = torch_dev
    bx = rc.boxes(0)
    sd = rc.mask_head_state_dict(C, classes, seed=classes + P)
    head = pkg.MaskHead.from_state_dict(sd, in_channels=C)
    maps = [t.to(dev) for t in rc.pyramid(C)]
    rois = bx.rois[bx.index("interior_l0")[0]:][:boxes].to(dev)
    pooled = pkg.roi_align(maps, rois, P, rc.SCALES, 2, out_padded=True, **CANON)      # the ring is the kernel's exact 0
    before = pooled.clone()
    head.prepare(boxes, P)
    for t in (head._a, head._b, head._up, head._scores, head._masks):
        t.fill_(float("nan"))
    masks = head(pooled)
    torch.cuda.synchronize()
    assert torch.equal(bits(pooled), bits(before))                                   # the input is not written
    assert tuple(masks.shape) == (boxes, classes, 2 * P, 2 * P)
    want = rc.mask_head_reference(sd, before[:, 1:-1, 1:-1, :].cpu())
    err = rel(torch, masks, want)
    print(f"mask head P={P} classes={classes} R={boxes}: {err:.2e}")
    assert err < NET_TOL
    assert pkg.tickets_in_use() == 0


def test_transposed_convolution_placement(pkg, torch_dev):
    """A single non-zero input pixel lights exactly its 2 x 2 output block, with the four weights in torch's order
    (w[ci][co][dy][dx] at output (2y + dy, 2x + dx)).  The 3x3 convolutions are identities, so the pixel arrives as it is."""
    _, dev = torch_dev
    P, classes, boxes, y0, x0, c0 = 6, 3, 2, 4, 1, 17
    sd = {k: torch.zeros_like(v) for k, v in rc.mask_head_state_dict(C, classes).items()}
    for i in range(4):
        sd[f"mask_head.{i}.0.weight"][:, :, 1, 1] = torch.eye(C)
    for k in range(classes):                        # class k reads channel k of the up-sampled map
        sd["mask_predictor.mask_fcn_logits.weight"][k, k, 0, 0] = 1.0
    w5 = sd["mask_predictor.conv5_mask.weight"]
    w5[c0, 0] = torch.tensor([[1.0, 2.0], [3.0, 4.0]])
    w5[c0, 2] = torch.tensor([[5.0, 6.0], [7.0, 8.0]])
    head = pkg.MaskHead.from_state_dict(sd, in_channels=C)
    pooled = torch.zeros(boxes, P + 2, P + 2, C)
    pooled[1, 1 + y0, 1 + x0, c0] = 1.0
    masks = head(pooled.to(dev)).cpu()
    want = torch.zeros(boxes, classes, 2 * P, 2 * P)
    want[1, 0, 2 * y0:2 * y0 + 2, 2 * x0:2 * x0 + 2] = w5[c0, 0]
    want[1, 2, 2 * y0:2 * y0 + 2, 2 * x0:2 * x0 + 2] = w5[c0, 2]
    assert float((masks - want).abs().max()) < 1e-5
    assert float((masks - rc.mask_head_reference(sd, pooled[:, 1:-1, 1:-1, :]).float()).abs().max()) < 1e-5


def test_both_heads_in_one_graph(pkg, torch_dev):
    """RoIAlign (no prepare) and both heads (after prepare(R)) captured into one graph: replays into NaN-filled tensors are
    bitwise the eager results, and no ticket stays held."""
    _, dev = torch_dev
    bx, boxes, classes = rc.boxes(0), 20, 5
    box = pkg.BoxHead.from_state_dict(rc.box_head_state_dict(C, 7, 128, classes), in_channels=C, P=7)
    mask = pkg.MaskHead.from_state_dict(rc.mask_head_state_dict(C, classes), in_channels=C)
    maps = [rc.padded_nan(t).to(dev) for t in rc.pyramid(C)]
    rois = bx.rois[:boxes].to(dev)
    p7 = torch.empty(boxes, 7, 7, C, device=dev)
    p14 = torch.empty(boxes, 16, 16, C, device=dev)

    def forward():
        pkg.multiscale_roi_align(maps, rois, rc.IMAGE, 7, in_padded=True, out=p7, **CANON)
        pkg.multiscale_roi_align(maps, rois, rc.IMAGE, 14, in_padded=True, out_padded=True, out=p14, **CANON)
        return (*box(p7), mask(p14))

    sg = torch.cuda.Stream()
    with torch.cuda.stream(sg):
        box.prepare(boxes)
        mask.prepare(boxes, 14)
        eager = [t.clone() for t in forward()]
    sg.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=sg):
        outs = forward()
    for _ in range(2):
        for t in (p7, p14, box._h6, box._h7, box._scores, mask._a, mask._b, mask._up, mask._scores, mask._masks):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs, eager):
            assert torch.equal(bits(got), bits(want))
    with torch.cuda.stream(sg):
        assert pkg.tickets_in_use() == 0
    assert pkg.tickets_in_use() == 0
    want_cls, _ = rc.box_head_reference(rc.box_head_state_dict(C, 7, 128, classes), rc.reference(C, 7, 2)[:boxes])
    assert rel(torch, eager[0], want_cls) < NET_TOL
    del graph


# ---- the sweeps ------------------------------------------------------------------------------------------------------------
FORCED = ("tiled", "stream_k", "latency")
KNOB_NAMES = sorted({k for f in FORCED for k in PROJ_FORMS[f]} | {"WINO_3X3_ALGO"})


def force(knobs, form, with_3x3=False):
    for k in KNOB_NAMES:
        knobs.unset(k)
    if form != "auto":
        for k, v in PROJ_FORMS[form].items():
            knobs.set(k, v)
        if with_3x3:
            knobs.set("WINO_3X3_ALGO", rc.HEAD_3X3_ALGO[form])


def test_box_head_sweep(pkg, knobs, torch_dev):
    """Every case of box_head_cases() on random pooled input, in the automatic form and under the tiled, stream-K and
    latency knob sets.  The plan queries say which form fc6, fc7 and the predictor take under each (a knob set the plan
    does not follow for a GEMM is recorded as what it took); over the sweep each of them runs in all three forms
    (tests/test_roi_host.py shows from the plan queries alone that the list allows it)."""
    _, dev = torch_dev
    ran, worst = collections.defaultdict(set), 0.0
    for c in rc.box_head_cases():
        sd = rc.box_head_state_dict(c.C, c.P, c.rep, c.classes, seed=c.seed)
        head = pkg.BoxHead.from_state_dict(sd, in_channels=c.C, P=c.P)
        pooled = torch.rand(c.R, c.P, c.P, c.C, generator=torch.Generator().manual_seed(c.seed)) - 0.5
        want_cls, want_box = rc.box_head_reference(sd, pooled)
        x, kp = pooled.to(dev), (5 * c.classes + 63) // 64 * 64
        for form in rc.HEAD_FORMS:
            force(knobs, form)
            took = {name: S.form_1x1(pkg, *g) for name, g in rc.box_head_gemms(c).items()}
            first = None
            for _ in range(2):
                head.prepare(c.R)
                for t in (head._h6, head._h7, head._scores):
                    t.fill_(float("nan"))
                logits, regression = head(x)
                torch.cuda.synchronize()
                assert tuple(head._scores.shape) == (c.R, kp) and bool((head._scores[:, 5 * c.classes:] == 0).all())
                first = head._scores.clone() if first is None else first
                assert torch.equal(bits(head._scores), bits(first)), (c, form)
            errs = rel(torch, logits, want_cls), rel(torch, regression, want_box)
            worst = max(worst, *errs)
            print(f"box head {tuple(c)[:5]} {form} {took}: logits {errs[0]:.2e} regression {errs[1]:.2e}")
            assert max(errs) < NET_TOL, (c, form)
            assert pkg.tickets_in_use() == 0
            for name, f in took.items():
                ran[name].add(f)
    force(knobs, "auto")
    print(f"box head sweep: worst rel err {worst:.2e}; forms {dict(ran)}")
    for name in ("fc6", "fc7", "predictor"):
        assert ran[name] >= set(FORCED), (name, ran[name])


def test_mask_head_sweep(pkg, knobs, torch_dev):
    """Every case of mask_head_cases() on a random pooled input with an exact-zero ring, which is not written: the
    automatic form and the three knob sets, WINO_3X3_ALGO beside them (big with tiled and stream-K, small with latency).
    Over the sweep the transposed convolution and the logits GEMM each run tiled, stream-K and latency, and the 3x3
    runs on the throughput and on the latency kernel."""
    _, dev = torch_dev
    ran, worst = collections.defaultdict(set), 0.0
    for c in rc.mask_head_cases():
        sd = rc.mask_head_state_dict(c.C, c.classes, seed=c.seed)
        head = pkg.MaskHead.from_state_dict(sd, in_channels=c.C)
        pooled = torch.zeros(c.R, c.P + 2, c.P + 2, c.C)
        pooled[:, 1:-1, 1:-1, :] = torch.rand(c.R, c.P, c.P, c.C, generator=torch.Generator().manual_seed(c.seed)) - 0.5
        want = rc.mask_head_reference(sd, pooled[:, 1:-1, 1:-1, :])
        x = pooled.to(dev)
        for form in rc.HEAD_FORMS:
            force(knobs, form, with_3x3=True)
            took = {name: S.form_1x1(pkg, *g) for name, g in rc.mask_head_gemms(c).items()}
            took["conv3x3"] = S.plan_3x3(pkg, c.R, c.P, c.P, c.C, c.C)[0]
            first = None
            for _ in range(2):
                head.prepare(c.R, c.P)
                for t in (head._a, head._b, head._up, head._scores, head._masks):
                    t.fill_(float("nan"))
                masks = head(x)
                torch.cuda.synchronize()
                assert tuple(masks.shape) == (c.R, c.classes, 2 * c.P, 2 * c.P)
                first = masks.clone() if first is None else first
                assert torch.equal(bits(masks), bits(first)), (c, form)
            assert torch.equal(bits(x.cpu()), bits(pooled)), "the input was written"
            err = rel(torch, masks, want)
            worst = max(worst, err)
            print(f"mask head {tuple(c)[:4]} {form} {took}: {err:.2e}")
            assert err < NET_TOL, (c, form)
            assert pkg.tickets_in_use() == 0
            for name, f in took.items():
                ran[name].add(f)
    force(knobs, "auto")
    print(f"mask head sweep: worst rel err {worst:.2e}; forms {dict(ran)}")
    for name in ("deconv", "logits"):
        assert ran[name] >= set(FORCED), (name, ran[name])
    assert ran["conv3x3"] == {"throughput", "latency"}


# ---- end to end ------------------------------------------------------------------------------------------------------------
E2E_HW = ((16, 16), (8, 8), (4, 4), (2, 2))      # the pyramid of a 64 x 64 input
E2E_BOXES = torch.tensor([   # table-style boxes in a 64 x 64 image: interior on each level, the four borders, thin, outside
    [0, 5.3, 7.1, 11.9, 12.7], [1, 10.2, 20.3, 21.4, 31.9], [0, 8.5, 12.5, 30.1, 35.3], [1, 2.2, 8.4, 31.7, 60.3],
    [0, -3.1, 20.3, 3.3, 26.1], [1, 30.6, -1.7, 36.2, 4.9], [0, 57.3, 10.2, 63.6, 16.5], [1, 22.2, 56.9, 28.7, 63.1],
    [1, -9.3, 8.2, -2.9, 14.3], [0, 10.3, 20.1, 10.9, 26.3], [1, 70.3, 80.1, 76.2, 86.7], [0, 1.3, 2.1, 62.7, 58.9]])


@pytest.fixture(scope="module")
def backbone(pkg, R, torch_dev):
    _, dev = torch_dev
    sd, body = fpn_random_state_dict(torch, R, "resnet18", out_channels=C, seed=5)
    model = pkg.ResNetFPN.from_state_dict(sd, "resnet18", out_channels=C)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(11)) - 0.5
    return model, x, fpn_reference_forward(torch, sd, body, x)


def test_default_forward_did_not_move(backbone, torch_dev):
    """ResNetFPN.forward without the keyword is bitwise what padded=True, sliced, gives: the same views of the same
    tensors.  (The one test here that does not need the new kernel.)"""
    _, dev = torch_dev
    model, x, want = backbone
    plain = {k: v.clone() for k, v in model(x.to(dev)).items()}
    views = model(x.to(dev))
    padded = model(x.to(dev), padded=True)
    torch.cuda.synchronize()
    assert sorted(padded) == sorted(plain) == ["0", "1", "2", "3", "pool"]
    for i in range(4):
        k = str(i)
        assert padded[k] is model._p[i] and tuple(padded[k].shape[1:3]) == tuple(s + 2 for s in E2E_HW[i])
        assert torch.equal(bits(padded[k][:, 1:-1, 1:-1, :]), bits(plain[k]))
        assert views[k].data_ptr() == padded[k][:, 1:-1, 1:-1, :].data_ptr() and views[k].stride() == padded[k].stride()
        assert rel(torch, plain[k], want[k]) < NET_TOL
    assert torch.equal(bits(padded["pool"]), bits(plain["pool"])) and tuple(plain["pool"].shape) == (2, 1, 1, C)
    assert views["pool"].data_ptr() == views["3"].data_ptr() and views["pool"].stride() == views["3"][:, ::2, ::2, :].stride()


def test_second_stage_end_to_end(backbone, pkg, torch_dev):
    _, dev = torch_dev
    model, x, feats64 = backbone
    classes, rois = 5, E2E_BOXES
    levels = rc.torchvision_levels(rois, rc.SCALES)
    assert set(levels.tolist()) == {0, 1, 2, 3} and torch.equal(levels, rc.threshold_levels(rois, rc.SCALES))
    combos = [(7, 2), (14, 2)]
    assert float(rc.min_sample_margin(rois, levels, combos, hw=E2E_HW).min()) >= rc.SAMPLE_MARGIN
    sd_box, sd_mask = rc.box_head_state_dict(C, 7, 128, classes, seed=1), rc.mask_head_state_dict(C, classes, seed=2)
    box = pkg.BoxHead.from_state_dict(sd_box, in_channels=C, P=7)
    mask = pkg.MaskHead.from_state_dict(sd_mask, in_channels=C)
    feats = model(x.to(dev), padded=True)
    p7 = pkg.multiscale_roi_align(feats, rois.to(dev), (64, 64), 7, in_padded=True, **CANON)
    per_image = [rois[rois[:, 0] == n][:, 1:].to(dev) for n in range(2)]       # the list form, for the mask branch
    order = torch.cat([torch.nonzero(rois[:, 0] == n).flatten() for n in range(2)])
    p14 = pkg.multiscale_roi_align(feats, per_image, (64, 64), 14, in_padded=True, out_padded=True, **CANON)
    logits, regression = box(p7)
    masks = mask(p14)
    torch.cuda.synchronize()
    maps64 = [feats64[str(i)] for i in range(4)]
    want7 = rc.roi_align_reference(maps64, rois, 7, rc.SCALES, 2, levels)
    want14 = rc.roi_align_reference(maps64, rois[order], 14, rc.SCALES, 2, levels[order])
    want_cls, want_box = rc.box_head_reference(sd_box, want7)
    want_masks = rc.mask_head_reference(sd_mask, want14)
    errs = {"pooled7": rel(torch, p7, want7), "pooled14": rel(torch, p14[:, 1:-1, 1:-1, :], want14),
            "logits": rel(torch, logits, want_cls), "regression": rel(torch, regression, want_box),
            "masks": rel(torch, masks, want_masks)}
    print("second stage: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert not {k: v for k, v in errs.items() if not v < NET_TOL}, errs
    assert pkg.tickets_in_use() == 0
