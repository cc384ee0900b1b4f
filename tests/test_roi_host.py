"""Host-side checks of multi-scale RoIAlign (wino_roi_align_hw) and of the R-CNN heads -- no GPU needed: the C-ABI
symbol, every refusal (each fires before the GPU is touched), the box generator's properties, the thresholds level rule
against torchvision's formula, the fp32 restatement of the arithmetic against the fp64 reference (what entitles the GPU
tests to cases.TIGHT), the heads' state-dict validation and their pure packing functions against torch in fp64."""
import ctypes
import importlib
import math
import os

import pytest
import torch

import roi_cases as rc
import shape_sweeps as S
from cases import PROJ_FORMS, TIGHT
from conftest import ROOT

E_SHAPE, E_ARG = -2, -3
F0, F1, F2, F3, ROIS, OUT = (k << 40 for k in range(1, 7))   # far apart: nothing overlaps by accident
OK = dict(f0=F0, f1=F1, f2=F2, f3=F3, hw=[v for s in rc.LEVEL_HW for v in s], scales=list(rc.SCALES), levels=4, N=2, C=64,
          in_padded=0, rois=ROIS, R=10, P=7, sampling=2, canonical_scale=16.0, canonical_level=4, out=OUT, out_padded=0)


def _call(pkg, **kw):
    a = dict(OK, **kw)
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    hw = None if a["hw"] is None else (ctypes.c_int * len(a["hw"]))(*a["hw"])
    sc = None if a["scales"] is None else (ctypes.c_float * len(a["scales"]))(*a["scales"])
    return pkg.lib().wino_roi_align_hw(p(a["f0"]), p(a["f1"]), p(a["f2"]), p(a["f3"]), hw, sc, a["levels"], a["N"], a["C"],
                                       a["in_padded"], p(a["rois"]), a["R"], a["P"], a["sampling"], a["canonical_scale"],
                                       a["canonical_level"], p(a["out"]), a["out_padded"], None)


@pytest.fixture(scope="module")
def D(pkg):
    return importlib.import_module("cuda_winograd_amd.detection")


def test_new_symbol_exported_and_declared(pkg):
    hdr = open(os.path.join(ROOT, "include", "winograd_mi355x.h")).read()
    assert hasattr(pkg.lib(), "wino_roi_align_hw")
    assert "wino_roi_align_hw(" in hdr and "wino_roi_align_hw." in hdr       # the prototype, and the "added since" list
    assert "wino_roi_align_hw" in pkg.SIGNATURES
    for name in ("roi_align", "multiscale_roi_align", "boxes_to_rois", "BoxHead", "MaskHead"):
        assert hasattr(pkg, name), name
    assert not [s for s in pkg.SIGNATURES if "roi" in s and ("workspace" in s or "prepare" in s)]


def test_every_refusal_fires_without_a_gpu(pkg):
    err = lambda: pkg.lib().wino_last_error_string().decode()
    bad_shapes = dict(levels=(0, 5, -1), N=(0, -1), C=(0, -4, 6, 63), P=(0, 65, -1), R=(-1,), sampling=(0, 5, -1),
                      in_padded=(2, -1), out_padded=(2, -1))
    for k, values in bad_shapes.items():
        for v in values:
            assert _call(pkg, **{k: v}) == E_SHAPE and f"{k}={v}" in err(), (k, v, err())
    for i in range(8):   # every h and w of hw_host
        for v in (0, -3):
            hw = list(OK["hw"])
            hw[i] = v
            assert _call(pkg, hw=hw) == E_SHAPE and f"{'hw'[i % 2]}={v}" in err() and f"level {i // 2}" in err(), (i, v)
    # one image of a level map, and one box's output, below 2^31 elements
    assert _call(pkg, levels=1, hw=[32768, 16384], scales=[0.25], C=4) == E_SHAPE and "h=32768" in err()
    assert _call(pkg, levels=1, hw=[46340, 46340], scales=[0.25], C=4, in_padded=1) == E_SHAPE and "32-bit" in err()
    assert _call(pkg, P=64, C=1 << 19) == E_SHAPE and f"C={1 << 19}" in err() and "P=64" in err()
    assert _call(pkg, P=64, C=(1 << 19) - 4, out=ROIS) == E_ARG and "overlap" in err()   # (just below 2^31: the next check)
    # pointers
    for k in ("f0", "f1", "f2", "f3", "rois", "out", "hw", "scales"):
        assert _call(pkg, **{k: None}) == E_ARG and "NULL" in err(), k
    for k in ("f0", "f1", "f2", "f3", "rois", "out"):
        assert _call(pkg, **{k: OK[k] + 4}) == E_ARG and "aligned" in err(), k
    # pointers beyond `levels` are ignored: NULL or misaligned is fine (the call reaches the next check, the overlap)
    assert _call(pkg, levels=2, scales=[0.25, 0.125], f2=None, f3=F3 + 4, out=ROIS) == E_ARG and "overlap" in err()
    # the scale sequence
    for scales in ([0.25, 0.125, 0.0625, 0.0625], [0.25, 0.125, 0.0625, 0.015625], [0.3, 0.15, 0.075, 0.0375],
                   [0.25, 0.5, 1.0, 2.0], [0.25, 0.125, float("nan"), 0.03125], [0.0, 0.125, 0.0625, 0.03125],
                   [-0.25, 0.125, 0.0625, 0.03125], [float("inf"), 0.125, 0.0625, 0.03125]):
        assert _call(pkg, scales=scales) == E_ARG and "scale_host[" in err(), scales
    for s in (0.0, -1.0, float("nan"), float("inf")):
        assert _call(pkg, levels=1, scales=[s]) == E_ARG and "scale_host[0]" in err(), s
    assert _call(pkg, levels=1, scales=[0.3], out=ROIS) == E_ARG and "overlap" in err()   # one level: any positive scale
    assert _call(pkg, scales=[4.0, 2.0, 1.0, 0.5], out=ROIS) == E_ARG and "overlap" in err()   # k0 = -2 is an integer
    for cs in (0.0, -16.0, float("nan"), float("inf")):
        assert _call(pkg, canonical_scale=cs) == E_ARG and "canonical_scale" in err(), cs
    # out against every level map and against rois: first byte, last byte, and just clear of both
    out_b, rois_b = 10 * 49 * 64 * 4, 10 * 5 * 4
    maps_b = [2 * h * w * 64 * 4 for h, w in rc.LEVEL_HW]
    for base, nbytes in zip((F0, F1, F2, F3, ROIS), (*maps_b, rois_b)):
        last = base + (nbytes - 1) // 16 * 16
        for out in (base, last, base - out_b + 16):
            assert _call(pkg, out=out) == E_ARG and "overlap" in err(), (base, out)
    assert _call(pkg, out=F3 + maps_b[3], in_padded=1) == E_ARG and "overlap" in err()   # the padded map is larger
    with pytest.raises(pkg.WinoError, match="rc=-2"):
        pkg._check(_call(pkg, C=6), "wino_roi_align_hw")


def test_no_boxes_is_ok_and_launches_nothing(pkg):
    assert _call(pkg, R=0) == 0
    assert _call(pkg, R=0, rois=None, out=None) == 0      # an empty torch tensor has no address
    assert _call(pkg, R=0, C=6) == E_SHAPE                # ... but the shape is still checked


# ---- the generator ---------------------------------------------------------------------------------------------------------
def test_generator_properties():
    bx = rc.boxes(0)
    assert len(bx.names) == len(rc.TABLE) + rc.N_RANDOM and bx.rois.dtype == torch.float32
    props = rc.class_properties(bx)
    for name in rc.CLASSES[:-1]:
        assert len(props[name]) >= 2 and all(props[name]), (name, props[name])
    assert len(bx.index("random")) == rc.N_RANDOM
    print(f"drawn {bx.drawn}, redrawn {bx.redrawn}")
    assert bx.redrawn <= 0.10 * bx.drawn
    for name in rc.CLASSES:   # both images in every class, all four levels among the random boxes
        assert {0.0, 1.0} <= set(bx.rois[bx.index(name), 0].tolist()) or name in ("random",), name
    assert set(bx.levels[bx.index("random")].tolist()) == {0, 1, 2, 3}
    assert set(bx.rois[bx.index("random"), 0].tolist()) == {0.0, 1.0}
    # every sample margin holds, for the table as for the random boxes, at every (P, sampling) the GPU tests run
    m = rc.min_sample_margin(bx.rois, bx.levels, rc.PS_COMBOS)
    print(f"closest sample to a discontinuity: {float(m.min()):.2e}")
    assert float(m.min()) >= rc.SAMPLE_MARGIN
    ex = bx.index("exact")
    assert float(rc.min_sample_margin(bx.rois[ex], bx.levels[ex], rc.EXACT_COMBOS).min()) >= rc.SAMPLE_MARGIN
    on_threshold = [n.startswith("threshold_") for n in bx.names]
    lm = rc.level_margin(bx.rois)
    assert all(float(v) >= rc.LEVEL_MARGIN or t for v, t in zip(lm, on_threshold))
    assert all(float(v) == 0 for v, t in zip(lm, on_threshold) if t)
    assert rc.boxes(0) is bx and torch.equal(rc.Boxes(0).rois, bx.rois)          # seeded


def test_exact_subset_is_exact_in_fp32():
    bx = rc.boxes(0)
    ex = bx.index("exact")
    assert float(rc.min_sample_margin(bx.rois[ex], bx.levels[ex], rc.EXACT_COMBOS_S4).min()) >= rc.SAMPLE_MARGIN
    for P, S in rc.EXACT_COMBOS + rc.EXACT_COMBOS_S4:
        for l in range(4):
            sel = [r for r in ex if int(bx.levels[r]) == l]
            y64, x64 = rc.sample_coords(bx.rois[sel], rc.SCALES[l], P, S)
            y32, x32 = rc.sample_coords(bx.rois[sel], rc.SCALES[l], P, S, dtype=torch.float32)
            assert torch.equal(y32.double(), y64) and torch.equal(x32.double(), x64)


def test_thresholds_rule_agrees_with_torchvisions_formula():
    bx = rc.boxes(0)
    got = rc.threshold_levels(bx.rois, rc.SCALES)
    assert torch.equal(got, rc.torchvision_levels(bx.rois, rc.SCALES))
    assert torch.equal(got, rc.torchvision_levels(bx.rois, rc.SCALES, dtype=torch.float32))
    for name, level in (("threshold_8", 1), ("threshold_16", 2), ("threshold_32", 3)):   # the upper level, under all three
        idx = bx.index(name)
        assert got[idx].tolist() == [level] * len(idx)
        assert rc.torchvision_levels(bx.rois[idx], rc.SCALES, dtype=torch.float32).tolist() == [level] * len(idx)
        assert bx.levels[idx].tolist() == [level] * len(idx)
    flipped = bx.index("flipped")
    assert got[flipped].tolist().count(0) >= 3                       # area <= 0: level 0
    assert rc.threshold_levels(torch.tensor([[0, float("nan"), 0, 4, 4]]), rc.SCALES).tolist() == [0]
    assert rc.threshold_levels(bx.rois, rc.SCALES[:1]).tolist() == [0] * len(bx.names)
    # the thresholds, as floats, sit just below 8^2, 16^2, 32^2
    for t, edge in zip(rc.level_thresholds(rc.SCALES), (64.0, 256.0, 1024.0)):
        assert edge * (1 - 3e-6) < float(t) < edge


@pytest.mark.parametrize("P", [7, 14])
def test_fp32_restatement_holds_a_quarter_of_tight(P):
    """Measured: 1.3e-6 at P = 7 and 1.7e-6 at P = 14 (sampling 2, C = 8) against TIGHT = 2e-5."""
    bx = rc.boxes(0)
    for S in (1, 2, 3):
        want = rc.reference(8, P, S)
        got = rc.roi_align_reference(rc.pyramid(8), bx.rois, P, rc.SCALES, S, bx.levels, dtype=torch.float32)
        err = rc.rel_err(got, want)
        print(f"fp32 restatement P={P} sampling={S}: {err:.2e}")
        assert err < TIGHT / 4


def test_reference_rules_for_bad_boxes():
    maps = rc.pyramid(8)
    nan = float("nan")
    rois = torch.tensor([[0, 5.3, 7.1, 11.9, 12.7], [-1, 5.3, 7.1, 11.9, 12.7], [2, 5.3, 7.1, 11.9, 12.7],
                         [0.5, 5.3, 7.1, 11.9, 12.7], [nan, 5.3, 7.1, 11.9, 12.7], [1, nan, 7.1, 11.9, 12.7],
                         [1, 5.3, 7.1, float("inf"), 12.7], [nan, nan, 7.1, 11.9, 12.7]])
    out, touched = rc.roi_align_reference(maps, rois, 7, rc.SCALES, 2, rc.threshold_levels(rois, rc.SCALES), taps=True)
    assert bool(torch.isfinite(out[0]).all()) and float(out[0].abs().max()) > 0 and touched[0][:2] == (0, 0)
    for r in (1, 2, 3, 4, 7):
        assert bool((out[r] == 0).all()) and touched[r] is None
    for r in (5, 6):
        assert bool(torch.isnan(out[r]).all()) and touched[r] is None


def test_launch_split_knob(pkg, knobs):
    """WINO_ROI_LAUNCH_TASKS caps the output positions of one launch; unset, 0, negative or not a number it changes
    nothing (the other WINO_* numbers read the same way: 0 is "not given"), and below one box it means one box."""
    n = pkg.roi_align_launches
    big = (1 << 31) // (66 * 66)                                # the boxes of one launch at P = 64 padded: 493 k
    knobs.unset("WINO_ROI_LAUNCH_TASKS")
    assert big == 492994 and n(big, 64, True) == 1 and n(big + 1, 64, True) == 2 and n(2 * big + 1, 64, True) == 3
    assert n(0, 7) == 0 and n(89, 7) == 1 and n((1 << 31) - 1, 1) == 1
    for v in ("0", "-1", "-2147483648", "junk", ""):
        knobs.set("WINO_ROI_LAUNCH_TASKS", v)
        assert n(89, 7, True) == 1 and n(big + 1, 64, True) == 2, v
    knobs.set("WINO_ROI_LAUNCH_TASKS", 12 * 81 + 40)
    assert n(89, 7, True) == 8 and n(96, 7, True) == 8 and n(97, 7, True) == 9 and n(89, 7, False) == 5
    knobs.set("WINO_ROI_LAUNCH_TASKS", 5)                       # less than one box of 49 positions: a box per launch
    assert n(89, 7) == 89 and n(89, 1) == 18
    knobs.unset("WINO_ROI_LAUNCH_TASKS")
    assert n(89, 7, True) == 1
    L, out = pkg.lib(), ctypes.c_long(0)
    for R, P, padded in ((-1, 7, 0), (1, 0, 0), (1, 65, 0), (1, 7, 2)):
        assert L.wino_roi_align_launches(R, P, padded, ctypes.byref(out)) == E_SHAPE
    assert L.wino_roi_align_launches(1, 7, 0, None) == E_ARG
    assert "wino_roi_align_launches(" in open(os.path.join(ROOT, "include", "winograd_mi355x.h")).read()


# ---- the sweep: any geometry ---------------------------------------------------------------------------------------------
SWEEP = rc.roi_sweep_cases()


def test_sweep_cases_pass_the_argument_checks(pkg):
    """Every sweep case reaches the entry point's last check (out laid over rois), so every earlier one accepts it; the
    cases that go through multiscale_roi_align get their scales back from infer_roi_scales."""
    err = lambda: pkg.lib().wino_last_error_string().decode()
    assert 20 <= len(SWEEP) <= 28 and len({c.name for c in SWEEP}) == len(SWEEP)
    for c in SWEEP:
        geo, R = c.geo, len(rc.case_boxes(c).names)
        hw = [v for s in geo.hw for v in s]
        assert _call(pkg, hw=hw, scales=list(geo.scales), levels=geo.levels, N=geo.N, C=c.C, in_padded=int(c.in_padded), R=R,
                     P=c.P, sampling=c.S, out_padded=int(c.out_padded), out=ROIS, **geo.canon) == E_ARG, (c.name, err())
        assert "overlap" in err(), (c.name, err())
        if c.defaults:
            p = 2 if c.in_padded else 0
            maps = [torch.empty(1, h + p, w + p, 4) for h, w in geo.hw]
            assert tuple(pkg.infer_roi_scales(maps, geo.image, c.in_padded)) == geo.scales, c.name
            assert (geo.canonical_scale, geo.canonical_level) == rc.DEFAULT_CANON


def test_sweep_reaches_its_corners():
    got = lambda f: {f(c) for c in SWEEP}
    for S in (1, 2, 3, 4):
        Ps = {c.P for c in SWEEP if c.S == S}
        assert 1 in Ps and any(P % 2 and P > 1 for P in Ps) and any(P % 2 == 0 for P in Ps), (S, Ps)
    p64 = [c for c in SWEEP if c.P == 64]
    assert len(p64) == 1 and p64[0].C == 4
    assert got(lambda c: c.geo.levels) == {1, 2, 3, 4}
    assert got(lambda c: c.geo.k0) >= {0, 1, 2, 3, 4, 5}
    one = [c.geo.scales[0] for c in SWEEP if c.geo.levels == 1]
    assert any(math.log2(s) == round(math.log2(s)) for s in one) and any(math.log2(s) != round(math.log2(s)) for s in one)
    assert got(lambda c: c.geo.N) == {1, 2, 3, 4, 5}
    for c in SWEEP:   # boxes in the first and in the last image
        assert {0.0, float(c.geo.N - 1)} <= set(rc.case_boxes(c).rois[:, 0].tolist()), c.name
    coarse = lambda g: round(1 / g.scales[-1])
    odd = [c for c in SWEEP if c.geo.image[0] % coarse(c.geo) and c.geo.image[1] % coarse(c.geo)]
    assert len(odd) >= len(SWEEP) // 2
    for c in SWEEP:
        assert c.geo.hw == tuple((math.ceil(c.geo.image[0] * s), math.ceil(c.geo.image[1] * s)) for s in c.geo.scales)
    assert any(math.ceil(c.geo.image[0] * s) != c.geo.image[0] * s for c in odd for s in c.geo.scales)
    all_hw = [s for c in SWEEP for s in c.geo.hw]
    assert any(h == 1 for h, w in all_hw) and any(w == 1 for h, w in all_hw) and any(w >= 3 * h for h, w in all_hw)
    assert got(lambda c: c.C) == {4, 8, 252, 256, 260, 320, 516}
    assert got(lambda c: (c.in_padded, c.out_padded)) == {(False, False), (False, True), (True, False), (True, True)}
    multi = [c for c in SWEEP if c.geo.levels > 1]
    assert {c.geo.canonical_scale for c in multi} == {16.0, 24.0, 56.0, 224.0}
    assert {c.geo.canonical_level for c in multi} == {3, 4, 5}
    assert len([c for c in multi if c.defaults]) >= 2
    assert any(c.geo.k0 != 2 for c in multi)


def test_sweep_levels_agree_and_spread():
    """torchvision's formula in fp64 and the thresholds rule give every box of every case the same level, under the
    case's own canonical values; every case with several levels hits two at least, the list hits all four."""
    hit = set()
    for c in SWEEP:
        gb, geo = rc.case_boxes(c), c.geo
        want = rc.torchvision_levels(gb.rois, geo.scales, **geo.canon)
        assert torch.equal(gb.levels, want)
        assert torch.equal(rc.threshold_levels(gb.rois, geo.scales, **geo.canon), want), c.name
        good = [r for r, n in enumerate(gb.names) if n != "huge"]        # (a huge box's level is the top one, and unread)
        levels = set(want[good].tolist())
        assert len(levels) >= min(geo.levels, 2), (c.name, levels)
        assert levels <= set(range(geo.levels))
        hit |= levels
        for j in range(1, geo.levels):                                    # a box on a threshold takes the upper level
            assert want[gb.index(f"threshold_{j}")].tolist() == [j, j], (c.name, j)
    assert hit == {0, 1, 2, 3}


def test_sweep_redraw_cap_and_margins():
    """At most one third of the random draws are redrawn (a condition: a generator that throws most of its draws away
    would be one that shapes its inputs), and every kept box but those on a threshold keeps both margins."""
    for c in SWEEP:
        gb, geo = rc.case_boxes(c), c.geo
        assert len(gb.index("random")) == c.n == gb.drawn - gb.redrawn
        assert 3 * gb.redrawn <= gb.drawn, (c.name, gb.redrawn, gb.drawn)
        m = rc.min_sample_margin(gb.rois, gb.levels, [(c.P, c.S)], hw=geo.hw, scales=geo.scales)
        assert float(m.min()) >= rc.SAMPLE_MARGIN, c.name
        lm = rc.level_margin(gb.rois, geo.scales, **geo.canon)
        for v, n in zip(lm.tolist(), gb.names):
            assert v == 0 if n.startswith("threshold_") else v >= rc.LEVEL_MARGIN, (c.name, n, v)
        again = rc.GeoBoxes(geo, ((c.P, c.S),), c.seed, c.n)                  # seeded
        assert torch.equal(again.rois, gb.rois) and rc.case_boxes(c) is gb


def test_sweep_class_properties():
    """Every named class has its property in every geometry.  A class may be missing from a geometry only where there is
    no room for it: an interior box of level l needs sqrt(area) above that level's threshold inside the image."""
    assert all(all(v) for v in rc.geo_class_properties(rc.geometry_boxes(rc.BASE_GEOMETRY, rc.PS_COMBOS, 0, 4)).values())
    for c in SWEEP:
        gb, geo = rc.case_boxes(c), c.geo
        props = rc.geo_class_properties(gb)
        assert all(all(v) for v in props.values()), (c.name, {k: v for k, v in props.items() if not all(v)})
        edges = [0.0] + geo.edges()
        for name in rc.named_classes(geo):
            room = True
            if name.startswith("interior_l"):
                room = (1.02 * edges[int(name[-1])]) ** 2 < 0.98 * 0.98 * geo.image[0] * geo.image[1]
            assert len(props.get(name, [])) == ((4 if name == "flipped" else 2) if room else 0), (c.name, name)
        huge = gb.index("huge")
        assert len(huge) == 2 * len(rc.HUGE) and len(props["huge"]) == len(huge)
        assert bool((gb.rois[huge, 1:].abs().max(dim=1).values >= 1e30).all()) and bool(torch.isfinite(gb.rois).all())
        assert {1e30, 3e38} <= {float(f"{abs(v):.0e}") for v in gb.rois[huge, 1:].flatten().tolist()}


def test_sweep_fp32_restatement_holds_a_quarter_of_tight():
    """What entitles the GPU sweep to TIGHT: on every case the straight fp32 restatement is within TIGHT / 4 of the fp64
    reference, in which the good boxes are finite and the huge ones exact zeros.  Measured worst over the list: 3.9e-6
    (the defaults case with a 34 x 30 finest level; 2.9e-6 where the finest level's sides are at most 24).  Nothing
    is claimed for larger maps: the restatement's error grows with the coordinates (README, the RoIAlign paragraph)."""
    worst = 0.0
    for c in SWEEP:
        gb, want = rc.case_boxes(c), rc.case_reference(c)
        assert bool(torch.isfinite(want).all()) and bool((want[gb.index("huge")] == 0).all()), c.name
        assert float(want.abs().max()) > 0.05, c.name
        got = rc.roi_align_reference(rc.case_pyramid(c), gb.rois, c.P, c.geo.scales, c.S, gb.levels, dtype=torch.float32)
        err = rc.rel_err(got, want)
        print(f"{c.name} finest {c.geo.hw[0]} P={c.P} S={c.S} C={c.C}: fp32 restatement {err:.2e}")
        worst = max(worst, err)
        assert err < TIGHT / 4, c.name
    print(f"worst {worst:.2e}")


# ---- the heads ---------------------------------------------------------------------------------------------------------------
def _validation(pkg, validate, sd, exp, **kw):
    for k in exp:
        bad = dict(sd)
        del bad[k]
        with pytest.raises(pkg.WinoError, match=f"missing key '{k}'"):
            validate(bad, **kw)
        bad = dict(sd, **{k: torch.empty((3,) + tuple(exp[k]))})
        with pytest.raises(pkg.WinoError, match=f"'{k}'"):
            validate(bad, **kw)
    with pytest.raises(pkg.WinoError, match="unexpected key 'extra.weight'"):
        validate(dict(sd, **{"extra.weight": torch.empty(3)}), **kw)


def test_box_head_state_dict_validation(pkg, D):
    exp = D.expected_box_head_keys(64, 7, 128, 5)
    assert exp["box_head.fc6.weight"] == (128, 64 * 49) and exp["box_predictor.bbox_pred.weight"] == (20, 128)
    sd = {k: torch.empty(v) for k, v in exp.items()}
    assert D.validate_box_head_state_dict(sd, 64, 7) == (128, 5)
    _validation(pkg, D.validate_box_head_state_dict, sd, exp, in_channels=64, P=7)
    with pytest.raises(pkg.WinoError, match="'box_head.fc6.weight' has shape"):
        D.validate_box_head_state_dict(sd, 64, 14)
    sd96 = {k: torch.empty(v) for k, v in D.expected_box_head_keys(64, 7, 96, 5).items()}
    with pytest.raises(pkg.WinoError, match="rep=96"):
        D.validate_box_head_state_dict(sd96, 64, 7)
    sd_odd = {k: torch.empty(v) for k, v in D.expected_box_head_keys(12, 1, 128, 5).items()}
    with pytest.raises(pkg.WinoError, match=r"in_channels\*P\*P=12"):
        D.validate_box_head_state_dict(sd_odd, 12, 1)


def test_mask_head_state_dict_validation(pkg, D):
    exp = D.expected_mask_head_keys(64, 3)
    assert len(exp) == 12 and exp["mask_head.3.0.weight"] == (64, 64, 3, 3)
    assert exp["mask_predictor.conv5_mask.weight"] == (64, 64, 2, 2)
    assert exp["mask_predictor.mask_fcn_logits.weight"] == (3, 64, 1, 1)
    sd = {k: torch.empty(v) for k, v in exp.items()}
    assert D.validate_mask_head_state_dict(sd, 64) == 3
    _validation(pkg, D.validate_mask_head_state_dict, sd, exp, in_channels=64)
    with pytest.raises(pkg.WinoError, match="has shape"):
        D.validate_mask_head_state_dict(sd, 128)
    sd96 = {k: torch.empty(v) for k, v in D.expected_mask_head_keys(96, 3).items()}
    with pytest.raises(pkg.WinoError, match="in_channels=96"):
        D.validate_mask_head_state_dict(sd96, 96)


def test_fc6_permutation_and_predictor_packing(D):
    C, P, rep, classes, R = 8, 3, 16, 5, 6
    g = torch.Generator().manual_seed(3)
    sd = {k: v.double() for k, v in rc.box_head_state_dict(C, P, rep, classes, seed=3).items()}
    pooled = torch.rand(R, P, P, C, generator=g, dtype=torch.float64) - 0.5     # NHWC
    F = torch.nn.functional
    want = F.linear(pooled.permute(0, 3, 1, 2).flatten(1), sd["box_head.fc6.weight"])
    B = D.pack_fc6(sd["box_head.fc6.weight"], C, P)
    assert tuple(B.shape) == (P * P * C, rep)
    assert float((pooled.reshape(R, -1) @ B - want).abs().max()) < 1e-13
    wp, bp = D.pack_predictor(sd["box_predictor.cls_score.weight"], sd["box_predictor.cls_score.bias"],
                              sd["box_predictor.bbox_pred.weight"], sd["box_predictor.bbox_pred.bias"])
    assert tuple(wp.shape) == (rep, 64) and tuple(bp.shape) == (64,)
    x = torch.rand(R, rep, generator=g, dtype=torch.float64)
    y = x @ wp + bp
    assert float((y[:, :classes] - F.linear(x, sd["box_predictor.cls_score.weight"],
                                            sd["box_predictor.cls_score.bias"])).abs().max()) < 1e-13
    assert float((y[:, classes:5 * classes] - F.linear(x, sd["box_predictor.bbox_pred.weight"],
                                                       sd["box_predictor.bbox_pred.bias"])).abs().max()) < 1e-13
    assert bool((y[:, 5 * classes:] == 0).all())


def test_transposed_convolution_as_a_gemm(D):
    """B = w.permute(0, 2, 3, 1).reshape(C, 4C), bias tiled four times: rows (r, y, x) x columns (dy, dx, co) viewed as
    rows (r, y, x, dy, dx) feed the per-pixel logits GEMM, and the one permute at the end gives F.conv_transpose2d +
    F.conv2d."""
    C, classes, R, P = 8, 3, 2, 4
    g = torch.Generator().manual_seed(4)
    sd = {k: v.double() for k, v in rc.mask_head_state_dict(C, classes, seed=4).items()}
    x = torch.rand(R, P, P, C, generator=g, dtype=torch.float64) - 0.5          # NHWC
    F = torch.nn.functional
    up = F.conv_transpose2d(x.permute(0, 3, 1, 2), sd["mask_predictor.conv5_mask.weight"],
                            sd["mask_predictor.conv5_mask.bias"], stride=2)
    want = F.conv2d(torch.relu(up), sd["mask_predictor.mask_fcn_logits.weight"], sd["mask_predictor.mask_fcn_logits.bias"])
    B, b4 = D.pack_deconv(sd["mask_predictor.conv5_mask.weight"], sd["mask_predictor.conv5_mask.bias"])
    assert tuple(B.shape) == (C, 4 * C) and tuple(b4.shape) == (4 * C,)
    rows = x.reshape(R * P * P, C) @ B + b4                                     # [(r, y, x)][(dy, dx, co)]
    got_up = rows.view(R, P, P, 2, 2, C).permute(0, 5, 1, 3, 2, 4).reshape(R, C, 2 * P, 2 * P)
    assert float((got_up - up).abs().max()) < 1e-13
    wl, bl = D.pack_logits(sd["mask_predictor.mask_fcn_logits.weight"], sd["mask_predictor.mask_fcn_logits.bias"])
    assert tuple(wl.shape) == (C, 64)
    scores = torch.relu(rows).view(R * P * P * 4, C) @ wl + bl                  # [(r, y, x, dy, dx)][classes, padded]
    assert bool((scores[:, classes:] == 0).all())
    got = scores.view(R, P, P, 2, 2, 64)[..., :classes].permute(0, 5, 1, 3, 2, 4).reshape(R, classes, 2 * P, 2 * P)
    assert float((got - want).abs().max()) < 1e-13


def test_head_sweeps_reach_every_form(pkg, knobs, D):
    """The case lists have the shapes the issue names, every case passes the heads' own validation, and -- from the plan
    queries alone -- every GEMM of either head takes the tiled, the stream-K and the latency form under some knob set of
    some case, and the mask head's 3x3 both of its kernels."""
    box, mask = rc.box_head_cases(), rc.mask_head_cases()
    assert 8 <= len(box) <= 12 and 6 <= len(mask) <= 10
    assert {c.C for c in box} == {32, 64, 96, 160} and {c.P for c in box} == {2, 4, 7, 8}
    assert {c.rep for c in box} == {64, 192, 320} and {c.classes for c in box} == {1, 2, 12, 13, 91}
    assert {c.R for c in box} == {1, 2, 111, 112, 113, 300}
    assert any((c.C * c.P * c.P) % 64 for c in box) and all((c.C * c.P * c.P) % 32 == 0 for c in box)
    assert {5 * c.classes for c in box} >= {60, 65}
    assert {c.C for c in mask} == {64, 128} and {c.P for c in mask} == {2, 6, 14}
    assert {c.classes for c in mask} == {1, 3, 64, 65, 91} and {c.R for c in mask} == {1, 3, 9, 40}
    for c in box:
        sd = {k: torch.empty(v) for k, v in D.expected_box_head_keys(c.C, c.P, c.rep, c.classes).items()}
        assert D.validate_box_head_state_dict(sd, c.C, c.P) == (c.rep, c.classes)
    for c in mask:
        sd = {k: torch.empty(v) for k, v in D.expected_mask_head_keys(c.C, c.classes).items()}
        assert D.validate_mask_head_state_dict(sd, c.C) == c.classes
    ran = {}
    for form in rc.HEAD_FORMS:
        for k in ("WINO_1X1_ALGO", "WINO_1X1_SK", "WINO_3X3_ALGO"):
            knobs.unset(k)
        if form != "auto":
            for k, v in PROJ_FORMS[form].items():
                knobs.set(k, v)
            knobs.set("WINO_3X3_ALGO", rc.HEAD_3X3_ALGO[form])
        for c in box:
            for name, g in rc.box_head_gemms(c).items():
                ran.setdefault(name, set()).add(S.form_1x1(pkg, *g))
        for c in mask:
            for name, g in rc.mask_head_gemms(c).items():
                ran.setdefault(name, set()).add(S.form_1x1(pkg, *g))
            ran.setdefault("conv3x3", set()).add(S.plan_3x3(pkg, c.R, c.P, c.P, c.C, c.C)[0])
    for name in ("fc6", "fc7", "predictor", "deconv", "logits"):
        assert ran[name] == {"tiled", "stream_k", "latency"}, (name, ran[name])
    assert ran["conv3x3"] == {"throughput", "latency"}
