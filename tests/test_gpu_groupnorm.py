"""GPU tests of groupnorm_relu (wino_groupnorm_relu_hw) against the fp64 reference of tests/groupnorm_cases.py at
cases.TIGHT, in both forced forms.  Every run is on the guarded arena at both placements, twice with equal bits, into
NaN-filled outputs and workspace; the input's ring holds NaN and the ring of the output must keep its bits."""
import numpy as np
import pytest
import torch

import groupnorm_cases as gc
from cases import TIGHT
from gpu_support import torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu

CPG = sorted({(C, cpg) for C in gc.CHANNELS for cpg in gc.cpgs(C)})


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("form", gc.FORMS)
@pytest.mark.parametrize("C,cpg", CPG)
def test_groupnorm_cases_against_fp64(C, cpg, form, pkg, torch_dev, knobs):
    """Every map and case class at this (C, cpg) in this form; N, ReLU and in place rotate so that each value meets each
    map and each class."""
    knobs.set("WINO_GN_FORM", form)
    G, run = C // cpg, 0
    for mi, (h, w) in enumerate(gc.MAPS):
        for ki, kind in enumerate(gc.KINDS):
            N, relu, in_place = 1 + (mi + ki) % 3, (mi + ki // 3) % 2 == 0, (mi + ki) % 2 == 1
            assert pkg.groupnorm_plan(N, h, w, C, G, _cus())[0] == form
            x, gamma, beta = gc.case(kind, N, h, w, C, G)
            tag = f"{kind} N={N} {h}x{w} C={C} cpg={cpg} {form} relu={relu} in_place={in_place}"
            got = gc.run_groupnorm(pkg, torch_dev[1], x, gamma, beta, G, relu, in_place, tag=tag)
            want = gc.reference(x, gamma, beta, G, relu=relu)
            err = gc.rel_err(got, want)
            print(f"{tag}: rel err {err:.2e}")
            assert err < TIGHT, tag
            if kind == "constant":                 # variance exactly 0: the output is beta
                b = np.where(beta[:cpg] < 0, 0, beta[:cpg]) if relu else beta[:cpg]
                assert np.abs(got[..., :cpg] - b).max() < TIGHT * np.abs(want).max(), tag
            run += 1
    assert run == len(gc.MAPS) * len(gc.KINDS)


@pytest.mark.parametrize("h,w", gc.MAPS)
def test_the_two_forms_agree(h, w, pkg, torch_dev, knobs):
    N, C, G = 2, 256, 32
    x, gamma, beta = gc.case("offset", N, h, w, C, G)
    want = gc.reference(x, gamma, beta, G)
    got = {}
    for form in gc.FORMS:
        knobs.set("WINO_GN_FORM", form)
        name, chunks = pkg.groupnorm_plan(N, h, w, C, G, _cus())
        assert name == form and (chunks == 1 or form == "split")
        if form == "split" and (h, w) == (37, 29):
            assert chunks > 1 and (h * w) % chunks != 0, f"{chunks} chunks: the last one is not ragged"
        assert (pkg.groupnorm_workspace_bytes(N, h, w, C, G) == 0) == (form == "whole")
        got[form] = gc.run_groupnorm(pkg, torch_dev[1], x, gamma, beta, G, tag=f"{form} {h}x{w}")
        assert gc.rel_err(got[form], want) < TIGHT
    diff = np.abs(got["whole"].astype(np.float64) - got["split"]).max()
    print(f"{h}x{w}: whole - split {diff:.2e}")
    assert diff <= 2e-6 * np.abs(want).max()


@pytest.mark.parametrize("form", gc.FORMS)
def test_in_place_is_out_of_place_bit_for_bit(form, pkg, torch_dev, knobs):
    knobs.set("WINO_GN_FORM", form)
    for C, G, (h, w) in ((64, 32, (7, 11)), (256, 32, (13, 21)), (128, 1, (2, 3))):
        x, gamma, beta = gc.case("plain", 2, h, w, C, G)
        a = gc.run_groupnorm(pkg, torch_dev[1], x, gamma, beta, G, in_place=False, aligns=(256,))
        b = gc.run_groupnorm(pkg, torch_dev[1], x, gamma, beta, G, in_place=True, aligns=(256,))
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("form", gc.FORMS)
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_non_finite_element_stays_in_its_image_and_group(bad, form, pkg, torch_dev, knobs):
    knobs.set("WINO_GN_FORM", form)
    for C, cpg, (h, w) in ((64, 1, (7, 11)), (64, 2, (13, 21)), (256, 8, (13, 21)), (128, 128, (7, 11))):
        G, N = C // cpg, 3
        x, gamma, beta = gc.case("plain", N, h, w, C, G)
        clean = gc.run_groupnorm(pkg, torch_dev[1], x, gamma, beta, G, aligns=(256,))
        g = min(G - 1, 5)
        # anywhere in the group, and at the group's shift: its first channel at the image's first pixel, which every value
        # of the group is taken relative to and which the split form hands on through the workspace
        for n, y, xx, c in ((1, h // 2, w - 1, g * cpg + cpg // 2), (2, 0, 0, g * cpg)):
            hurt = x.copy()
            hurt[n, y, xx, c] = bad
            got = gc.run_groupnorm(pkg, torch_dev[1], hurt, gamma, beta, G, aligns=(256,), tag=f"{bad} {form} at {(n, y, xx, c)}")
            hit = np.zeros(x.shape, dtype=bool)
            hit[n, :, :, g * cpg:(g + 1) * cpg] = True
            assert np.isnan(got[hit]).all(), "its own (image, group) is not NaN throughout"
            assert np.array_equal(got.view(np.int32)[~hit], clean.view(np.int32)[~hit]), "another group or image changed"


@pytest.mark.parametrize("C,form", [(2048, "split"), (8192, "split"), (8192, "whole")])
def test_a_group_wider_than_the_workgroups_lanes(C, form, pkg, torch_dev, knobs):
    """One group of C channels: more channel quads than the workgroup has threads (256 in the split form, 1024 in the
    whole form), so a thread's quad changes from item to item, gamma and beta are loaded per item, and the statistics
    are reduced over every bit of the thread number."""
    knobs.set("WINO_GN_FORM", form)
    assert C // 4 > (256 if form == "split" else 1024)
    for kind, (h, w), N, relu, in_place in (("offset", (2, 3), 2, True, False), ("plain", (1, 1), 1, False, True),
                                            ("scales", (3, 2), 1, True, True)):
        x, gamma, beta = gc.case(kind, N, h, w, C, 1)
        got = gc.run_groupnorm(pkg, torch_dev[1], x, gamma, beta, 1, relu, in_place, tag=f"{kind} C={C} {form}")
        err = gc.rel_err(got, gc.reference(x, gamma, beta, 1, relu=relu))
        print(f"{kind} N={N} {h}x{w} C={C} one group {form}: rel err {err:.2e}")
        assert err < TIGHT
    x, gamma, beta = gc.case("plain", 2, 2, 3, C, 1)
    clean = gc.run_groupnorm(pkg, torch_dev[1], x, gamma, beta, 1, aligns=(256,))
    x = x.copy()
    x[1, 1, 2, C - 3] = float("nan")
    got = gc.run_groupnorm(pkg, torch_dev[1], x, gamma, beta, 1, aligns=(256,))
    assert np.isnan(got[1]).all() and np.array_equal(got[0].view(np.int32), clean[0].view(np.int32))


def test_refusals_touch_nothing(pkg, torch_dev, knobs):
    _, dev = torch_dev
    knobs.set("WINO_GN_FORM", "split")
    N, h, w, C, G = 2, 5, 7, 64, 32
    x = torch.randn(N, h + 2, w + 2, C, device=dev)
    gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    out = torch.full_like(x, 9.0)
    need = pkg.groupnorm_workspace_bytes(N, h, w, C, G)
    assert need == N * min(h * w, 128) * 4 * G * 4
    ws = torch.full((need // 4,), 9.0, device=dev)
    L, p = pkg.lib(), lambda t: t.data_ptr()

    def call(xp=None, gp=None, bp=None, op=None, dims=(N, h, w, C, G), eps=1e-5, wsp=None, wsb=need):
        return L.wino_groupnorm_relu_hw(p(x) if xp is None else xp, p(gamma) if gp is None else gp,
                                        p(beta) if bp is None else bp, p(out) if op is None else op, *dims, eps, 1,
                                        p(ws) if wsp is None else wsp, wsb, pkg._stream())

    SHAPE, ARG = -2, -3
    for dims in ((-1, h, w, C, G), (N, 0, w, C, G), (N, h, 0, C, G), (N, h, w, 32, 32), (N, h, w, 96, 32), (N, h, w, C, 0),
                 (N, h, w, C, 3), (N, h, w, 192, 1), (N, h, w, C, 128), (N, h, (1 << 26) - 2, C, G),
                 (N, (1 << 20), (1 << 14), C, G)):
        assert call(dims=dims) == SHAPE, dims
    assert call(dims=(0, h, w, C, G), xp=0) == 0                         # nothing to do, nothing looked at
    assert call(xp=0) == ARG and call(gp=0) == ARG and call(bp=0) == ARG and call(op=0) == ARG
    assert call(xp=p(x) + 4) == ARG and call(gp=p(gamma) + 4) == ARG and call(bp=p(beta) + 8) == ARG and call(op=p(out) + 4) == ARG
    for eps in (0.0, -1e-5, float("inf"), float("nan")):
        assert call(eps=eps) == ARG, eps
    assert call(wsb=need - 4) == ARG and call(wsp=0) == ARG and call(wsp=p(ws) + 4, wsb=need) == ARG
    assert call(op=p(x) + 16) == ARG                                     # overlap that is not in place
    assert call(wsp=p(x)) == ARG and call(gp=p(out)) == ARG and call(bp=p(out) + 64) == ARG
    torch.cuda.synchronize()
    assert bool((out == 9).all()) and bool((ws == 9).all())
    with pytest.raises(pkg.WinoError, match="x must be"):
        pkg.groupnorm_relu(x[:, :, :, ::2], gamma, beta, G)
    with pytest.raises(pkg.WinoError, match="gamma and beta"):
        pkg.groupnorm_relu(x, gamma[:32].contiguous(), beta, G)
    with pytest.raises(pkg.WinoError, match="workspace too small"):
        pkg.groupnorm_relu(x, gamma, beta, G, workspace=ws[:-1])
    with pytest.raises(pkg.WinoError, match="rc=-2"):
        pkg.groupnorm_relu(x, gamma, beta, 3)
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out[:, 0] == 9).all()) and not bool((out[:, 1:-1, 1:-1] == 9).any())


@pytest.mark.parametrize("form", gc.FORMS)
def test_graph_replay_is_eager_bit_for_bit(form, pkg, torch_dev, knobs):
    _, dev = torch_dev
    knobs.set("WINO_GN_FORM", form)
    N, h, w, C, G = 2, 13, 21, 256, 32
    x, gamma, beta = gc.case("offset", N, h, w, C, G)
    xt, gt, bt = (torch.from_numpy(a).to(dev) for a in (gc.padded(x, 0.0), gamma, beta))
    need = pkg.groupnorm_workspace_bytes(N, h, w, C, G)
    ws = torch.full((max(need, 4) // 4,), float("nan"), device=dev)
    eager = pkg.groupnorm_relu(xt, gt, bt, G, workspace=ws).clone()
    out = torch.zeros_like(eager)
    sg = torch.cuda.Stream()
    sg.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=sg):
        pkg.groupnorm_relu(xt, gt, bt, G, out=out, workspace=ws)
    for _ in range(2):
        out.fill_(float("nan"))
        ws.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[:, 1:-1, 1:-1], eager[:, 1:-1, 1:-1])
    assert gc.rel_err(eager[:, 1:-1, 1:-1].cpu().numpy(), gc.reference(x, gamma, beta, G)) < TIGHT


@pytest.mark.parametrize("index", range(gc.SWEEP_COUNT))
def test_random_legal_layouts(index, pkg, torch_dev, knobs):
    s = gc.sweep_specs()[index]
    if s["form"]:
        knobs.set("WINO_GN_FORM", s["form"])
    x, gamma, beta = gc.case(s["kind"], s["N"], s["h"], s["w"], s["C"], s["G"], seed=index)
    got = gc.run_groupnorm(pkg, torch_dev[1], x, gamma, beta, s["G"], s["relu"], s["in_place"], tag=str(s))
    err = gc.rel_err(got, gc.reference(x, gamma, beta, s["G"], relu=s["relu"]))
    print(s, f"rel err {err:.2e}")
    assert err < TIGHT
