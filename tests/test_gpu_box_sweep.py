"""GPU sweeps of box decoding (wino_box_decode_hw) and batched NMS (wino_batched_nms_hw) over what the library accepts,
against the fp64 references of tests/box_cases.py.  tests/test_gpu_boxes.py runs the detectors' layouts and thresholds;
here are the rest: every NMS compare at equality, the thresholds' extremes with degenerate and infinite boxes, boxes off
the quarter-pixel lattice, and the decode over its legal column layouts, grids, weights, clamps and image sizes.
tests/test_boxes_host.py shows on the CPU what entitles these tests to exact NMS results and to cases.TIGHT.  Every run
is on the guarded arena at both alignments, into NaN-filled outputs and a NaN-filled workspace, twice, bitwise equal
(gpu_support.run_decode / run_nms).  The runs at the size limits and past 4 GiB are in tests/test_gpu_large_tensors.py."""
import numpy as np
import pytest

import box_cases as bc
from cases import TIGHT
from gpu_support import run_decode, run_nms, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu


def assert_nms(got, want, tag):
    """keep, count and rois exactly the reference's (rois bit for bit: they hold infinities), -1 after the count."""
    (keep, count, rois), (want_keep, want_count, want_rois) = got, want[:3]
    assert np.array_equal(count, want_count), (tag, count.tolist(), want_count.tolist())
    assert np.array_equal(keep, want_keep), tag
    assert np.array_equal(rois.view(np.int32), want_rois.view(np.int32)), tag
    for s in range(keep.shape[0]):
        assert (keep[s, count[s]:] == -1).all(), tag


# ---- A1: every compare at equality ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iou_thresh,min_size", bc.EqualityCase.runs())
def test_nms_compares_at_equality(iou_thresh, min_size, pkg, torch_dev):
    """iou > iou_thresh, side >= min_size, score >= score_thresh on operands that are exact in fp32: a pair whose IoU is
    the threshold keeps its second box, a side or a score equal to its threshold makes a candidate, and one fp32
    neighbour further the decision turns; the ties sit in diagonal and off-diagonal words of the bit matrix."""
    c = bc.equality_case()
    p = dict(iou_thresh=iou_thresh, min_size=min_size, score_thresh=c.SCORE_THRESH)
    for use_groups in (True, False):
        want = c.expected(iou_thresh, min_size, use_groups)
        got = run_nms(pkg, torch_dev[1], c.boxes, c.scores, c.groups if use_groups else None, c.R, p,
                      tag=f"equality groups={use_groups}")
        assert_nms(got, want, (iou_thresh, min_size, use_groups))
    full = int(c.expected(iou_thresh, min_size, True)[1].max())
    want = c.expected(iou_thresh, min_size, True, max(full // 2, 1))
    got = run_nms(pkg, torch_dev[1], c.boxes, c.scores, c.groups, max(full // 2, 1), p, aligns=(16,), tag="equality cut")
    assert_nms(got, want, (iou_thresh, min_size, "cut"))


# ---- A2: the thresholds' extremes, degenerate and infinite boxes, any group id ---------------------------------------------
@pytest.mark.parametrize("iou_thresh", bc.SWEEP_IOU)
@pytest.mark.parametrize("R", bc.SWEEP_R)
def test_nms_parameter_and_geometry_sweep(R, iou_thresh, pkg, torch_dev):
    c = bc.sweep_nms_case(R)
    combos = bc.sweep_combos(iou_thresh)
    assert len(combos) == 16
    for k, combo in enumerate(combos):
        _, min_size, score_thresh, use_groups = combo
        p = dict(iou_thresh=iou_thresh, min_size=min_size)
        if score_thresh is not None:
            p["score_thresh"] = score_thresh
        want = c.expected(combo)
        got = run_nms(pkg, torch_dev[1], c.boxes, None if score_thresh is None else c.scores,
                      c.groups if use_groups else None, R, p, aligns=((256, 16) if k % 4 == 0 else (16,)), tag=str(combo))
        assert_nms(got, want, combo)
    print(f"R={R} iou_thresh={iou_thresh}: kept {[c.expected(x)[1].tolist() for x in combos[:4]]} ...")


# ---- A3: boxes off the lattice -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", bc.OFF_LATTICE_R)
def test_nms_off_lattice_boxes(R, pkg, torch_dev):
    c = bc.off_lattice_case(R)
    for use_groups, use_scores in c.variants:
        p = dict(c.PARAMS)
        if not use_scores:
            p.pop("score_thresh")
        want = c.expected(use_groups, use_scores)
        got = run_nms(pkg, torch_dev[1], c.boxes, c.scores if use_scores else None, c.groups if use_groups else None, R, p,
                      aligns=((256, 16) if use_groups else (16,)), tag=f"off-lattice groups={use_groups}")
        assert_nms(got, want, (R, use_groups, use_scores))
    print(f"R={R}: kept {c.expected()[1].tolist()} of {R}")


# a grid-mode launch of the sweep with a score column and image sizes that cut through its boxes: 4 images of 480 boxes.
# On the fp32 restatement's boxes the reference's smallest margins are 1.4e-3 (IoU), 3.4e-3 (side) and 1.1e-3 (score)
DECODE_TO_NMS = 11
DECODE_NMS_PARAMS = dict(iou_thresh=0.5, min_size=1e-2, score_thresh=-0.5)


def test_nms_on_the_decodes_own_boxes(pkg, torch_dev):
    """The second off-lattice source: what the decode kernel itself wrote, sorted by its score column on the host (a
    stable sort, ties to the lower index), one segment per image, anchor index as group.  The reference is fed the same
    fp32 boxes, and the margins it met on them are asserted, so a fragile decision fails loudly rather than wrongly (a
    side's margin is capped at min_size: a box clipped to an edge has a side of exactly 0 in every precision)."""
    c = bc.decode_sweep_cases()[DECODE_TO_NMS]
    assert c.grid and c.score_col is not None and c.spec["hw"] in ("usual", "fractional") and c.N * c.rpi * c.A >= 1000
    boxes, scores = run_decode(pkg, torch_dev[1], c, aligns=(256,), tag="decode for nms")
    order = np.argsort(-scores, axis=1, kind="stable")
    boxes = np.ascontiguousarray(np.take_along_axis(boxes, order[:, :, None], axis=1))
    scores = np.ascontiguousarray(np.take_along_axis(scores, order, axis=1))
    groups = np.ascontiguousarray((order % c.A).astype(np.int32))
    assert (boxes != np.round(boxes * 4) / 4).mean() > 0.3
    p, R = DECODE_NMS_PARAMS, boxes.shape[1]
    want = bc.batched_nms_reference(boxes, scores, groups, **p)
    margin = dict(iou=min(r.iou_margin for r in want[3]), size=min(r.size_margin for r in want[3]),
                  score=min(r.score_margin for r in want[3]))
    print(f"decode -> NMS: N={c.N} R={R} kept {want[1].tolist()}, margins {margin}")
    assert margin["iou"] >= bc.IOU_MARGIN and margin["score"] >= bc.SCORE_MARGIN
    assert margin["size"] >= min(bc.size_margin(p["min_size"]), p["min_size"])
    assert (want[1] > 0).all() and (want[1] < R).all()
    assert_nms(run_nms(pkg, torch_dev[1], boxes, scores, groups, R, p, tag="decode -> nms"), want, "decode -> nms")


# ---- B: the decode over its legal launches --------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(bc.decode_sweep_specs())))
def test_decode_sweep(index, pkg, torch_dev):
    c = bc.decode_sweep_cases()[index]
    boxes, scores = run_decode(pkg, torch_dev[1], c, offset=c.offset, extra=c.extra, tag=f"sweep {index}")
    want = c.reference()
    err = bc.rel_err(boxes, want)
    print(f"sweep {index}: {c.spec}: {err:.2e}")
    assert err < TIGHT
    if c.spec["hw"] == "zero":
        assert not boxes.any(), "clipped to an image of 0 x 0: exactly zero"
    if c.score_col is None:
        assert scores is None                                  # (run_decode saw the scores buffer keep its NaN fill)
    else:
        assert np.array_equal(scores.view(np.int32), c.scores().view(np.int32)), "the score column is copied bit for bit"
