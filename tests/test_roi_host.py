"""Host-side checks of multi-scale RoIAlign (wino_roi_align_hw) and of the R-CNN heads -- no GPU needed: the C-ABI
symbol, every refusal (each fires before the GPU is touched), the box generator's properties, the thresholds level rule
against torchvision's formula, the fp32 restatement of the arithmetic against the fp64 reference (what entitles the GPU
tests to cases.TIGHT), the heads' state-dict validation and their pure packing functions against torch in fp64."""
import ctypes
import importlib
import os

import pytest
import torch

import roi_cases as rc
from cases import TIGHT
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
    for P, S in rc.EXACT_COMBOS:
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
