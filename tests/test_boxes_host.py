"""Host-side checks of box decoding (wino_box_decode_hw) and batched NMS (wino_batched_nms_hw) -- no GPU needed: the
C-ABI symbols, every refusal of both entry points (each fires before the GPU is touched), the workspace formula, and
what entitles the GPU tests to their bars: a straight torch fp32 restatement of the decode holds cases.TIGHT / 4 against
the fp64 reference of tests/box_cases.py, an fp32 restatement of the NMS walk makes the fp64 walk's decisions exactly,
every committed case keeps the generator's margins within its redraw cap, every case class has its property, and the
seeded detector's fp64 forward keeps ten times those margins."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import box_cases as bc
from cases import TIGHT
from conftest import ROOT

E_SHAPE, E_ARG = -2, -3
HEAD, ANC, HW, BOXES, SCORES, GROUPS, KEEP, COUNT, ROIS, WS = (k << 40 for k in range(1, 11))
DEC_OK = dict(head=HEAD, N=2, rpi=15, ld=64, A=3, delta_col=3, score_col=0, anchors=ANC, gh=3, gw=5, sy=8, sx=8, hw=HW,
              weights=(1.0, 1.0, 1.0, 1.0), clamp=bc.CLIP, boxes=BOXES, bstride=45, boff=0, scores=SCORES, sstride=45,
              soff=0)
NMS_OK = dict(boxes=BOXES, scores=SCORES, groups=GROUPS, S=2, R=100, iou=0.5, min_size=0.0, score_thresh=-math.inf,
              max_out=10, keep=KEEP, count=COUNT, rois=ROIS, ws=WS, ws_bytes=2 * 100 * 2 * 8)


def _p(v):
    return None if v is None else ctypes.c_void_p(v)


def _decode(pkg, **kw):
    a = dict(DEC_OK, **kw)
    return pkg.lib().wino_box_decode_hw(_p(a["head"]), a["N"], a["rpi"], a["ld"], a["A"], a["delta_col"], a["score_col"],
                                        _p(a["anchors"]), a["gh"], a["gw"], a["sy"], a["sx"], _p(a["hw"]), *a["weights"],
                                        a["clamp"], _p(a["boxes"]), a["bstride"], a["boff"], _p(a["scores"]), a["sstride"],
                                        a["soff"], None)


def _nms(pkg, **kw):
    a = dict(NMS_OK, **kw)
    return pkg.lib().wino_batched_nms_hw(_p(a["boxes"]), _p(a["scores"]), _p(a["groups"]), a["S"], a["R"], a["iou"],
                                         a["min_size"], a["score_thresh"], a["max_out"], _p(a["keep"]), _p(a["count"]),
                                         _p(a["rois"]), _p(a["ws"]), a["ws_bytes"], None)


def test_new_symbols_exported_and_declared(pkg):
    hdr = open(os.path.join(ROOT, "include", "winograd_mi355x.h")).read()
    for name in ("wino_box_decode_hw", "wino_batched_nms_hw"):
        assert hasattr(pkg.lib(), name) and name in pkg.ABI_SYMBOLS and name in pkg.SIGNATURES
        assert name + "(" in hdr and name + "," in hdr                      # the prototype, and the "added since" list
    for name in ("box_decode", "batched_nms", "nms_workspace_bytes"):
        assert callable(getattr(pkg, name)), name
    assert not [s for s in pkg.SIGNATURES if ("nms" in s or "box_decode" in s) and ("workspace" in s or "prepare" in s)]
    assert pkg.lib().wino_abi_version() == 1
    assert pkg.BBOX_XFORM_CLIP == bc.CLIP


def test_decode_refusals_fire_without_a_gpu(pkg):
    err = lambda: pkg.lib().wino_last_error_string().decode()
    bad = dict(N=(-1,), rpi=(-1, 14), ld=(0, -64), A=(0, -1, 16), delta_col=(-1, 53), score_col=(62,), gh=(2, 0, -3),
               gw=(4, 0), sy=(0, -8), sx=(0,))
    for k, values in bad.items():
        for v in values:
            assert _decode(pkg, **{k: v}) == E_SHAPE and "box_decode: unsupported shape" in err(), (k, v, err())
    name = dict(rpi="rows_per_image", gh="grid_h", gw="grid_w", sy="stride_y", sx="stride_x")
    assert _decode(pkg, sy=0) == E_SHAPE and "stride_y=0" in err()
    assert _decode(pkg, gh=2) == E_SHAPE and f"{name['gh']}=2" in err()
    # N rows_per_image A below 2^31
    assert _decode(pkg, N=1 << 16, rpi=1 << 15, gh=0, gw=0, A=1, bstride=1 << 15, sstride=1 << 15) == E_SHAPE
    assert "2^31" in err()
    big = (1 << 31) - 1                                                      # (a product that would pass 2^63)
    assert _decode(pkg, N=big, rpi=big, gh=0, gw=0, A=15, ld=128, delta_col=15, bstride=1 << 62, sstride=1 << 62) == E_SHAPE
    assert "2^31" in err()
    # an image's boxes between its offset and its stride
    for kw in (dict(bstride=44), dict(boff=-1), dict(boff=1), dict(sstride=44), dict(soff=-1), dict(bstride=50, boff=6),
               dict(sstride=50, soff=6)):
        assert _decode(pkg, **kw) == E_SHAPE and "must fit between the offset and the stride" in err(), kw
    assert _decode(pkg, sstride=0, soff=-5, score_col=-1, scores=None, boxes=HEAD) == E_ARG    # unused: not checked
    # nothing to do
    assert _decode(pkg, N=0, head=None, boxes=None, scores=None, anchors=None, hw=None) == 0
    assert _decode(pkg, rpi=0, gh=0, gw=0, bstride=0, sstride=0, head=None, boxes=None) == 0
    assert _decode(pkg, N=0, A=0) == E_SHAPE                                 # ... but the shape is still checked
    # pointers
    for k in ("head", "anchors", "hw", "boxes", "scores"):
        assert _decode(pkg, **{k: None}) == E_ARG and "NULL" in err(), k
        assert _decode(pkg, **{k: DEC_OK[k] + 4}) == E_ARG and "aligned" in err(), k
    assert _decode(pkg, scores=None, score_col=-1, boxes=HEAD) == E_ARG and "overlap" in err()
    # weights and clamp
    for w in (0.0, math.nan, math.inf, -math.inf):
        for i in range(4):
            ws = [1.0] * 4
            ws[i] = w
            assert _decode(pkg, weights=tuple(ws)) == E_ARG and "weights" in err(), (i, w)
    assert _decode(pkg, clamp=math.nan) == E_ARG and "clamp" in err()
    assert _decode(pkg, weights=(-10.0, 10.0, 5.0, 5.0), clamp=math.inf, boxes=HEAD) == E_ARG and "overlap" in err()
    # outputs against every input and each other: first byte, last byte, and just clear of both
    boxes_b, scores_b = (45 + 45) * 16, (45 + 45) * 4
    for base, nbytes in ((HEAD, 30 * 64 * 4), (ANC, 3 * 16), (HW, 16)):
        last = base + (nbytes - 1) // 16 * 16
        for out, out_b in (("boxes", boxes_b), ("scores", scores_b)):
            for at in (base, last, base - (out_b - 1) // 16 * 16):
                assert _decode(pkg, **{out: at}) == E_ARG and "overlap" in err(), (base, out, at)
    assert _decode(pkg, scores=BOXES + boxes_b - 16) == E_ARG and "overlap" in err()
    # the slice of a wider buffer is what counts: an offset moves it clear of, or onto, the head
    assert _decode(pkg, boxes=HEAD - 100 * 16, bstride=300, boff=100) == E_ARG and "overlap" in err()
    assert _decode(pkg, boxes=HEAD - 45 * 16, bstride=45, N=1, rpi=15, scores=HEAD) == E_ARG and "overlap" in err()
    # boxes mode: anchors is [rows][4]
    assert _decode(pkg, gh=0, gw=0, boxes=ANC + 29 * 16) == E_ARG and "overlap" in err()
    with pytest.raises(pkg.WinoError, match="rc=-2"):
        pkg._check(_decode(pkg, A=0), "wino_box_decode_hw")


def test_nms_refusals_fire_without_a_gpu(pkg):
    err = lambda: pkg.lib().wino_last_error_string().decode()
    for k, values in dict(S=(-1,), R=(-1, 32769), max_out=(0, -1)).items():
        for v in values:
            assert _nms(pkg, **{k: v}) == E_SHAPE and f"{k}={v}" in err(), (k, v, err())
    assert _nms(pkg, S=1 << 15, R=32768) == E_SHAPE and "2^24" in err()          # 2^24 workgroups of the mask kernel
    assert _nms(pkg, S=(1 << 15) - 1, R=32768, ws_bytes=0) == E_ARG and "workspace too small" in err()
    assert _nms(pkg, S=0, boxes=None, keep=None, count=None, ws=None, ws_bytes=0) == 0
    assert _nms(pkg, S=0, max_out=0) == E_SHAPE                              # ... but the shape is still checked
    assert _nms(pkg, R=0, count=None) == E_ARG and "NULL" in err()
    for k in ("boxes", "keep", "count"):
        assert _nms(pkg, **{k: None}) == E_ARG and "NULL" in err(), k
    assert _nms(pkg, ws=None) == E_ARG and "workspace too small" in err()
    for k in ("boxes", "scores", "groups", "keep", "count", "rois", "ws"):
        assert _nms(pkg, **{k: NMS_OK[k] + 4}) == E_ARG and "aligned" in err(), k
    for k in ("iou", "min_size", "score_thresh"):
        assert _nms(pkg, **{k: math.nan}) == E_ARG and "NaN" in err(), k
    assert _nms(pkg, ws_bytes=3199) == E_ARG and "need 3200 bytes" in err()
    # every output against every input and every other output
    sizes = dict(boxes=200 * 16, scores=800, groups=800, keep=80, count=8, rois=400, ws=3200)
    outs = ("keep", "count", "rois", "ws")
    for o in outs:
        for other in sizes:
            if other == o:
                continue
            last = NMS_OK[other] + (sizes[other] - 1) // 16 * 16
            for at in (NMS_OK[other], last, NMS_OK[other] - (sizes[o] - 1) // 16 * 16):
                assert _nms(pkg, **{o: at}) == E_ARG and "overlap" in err(), (o, other, at)
    # optional operands left out are not checked: the call reaches the overlap check
    assert _nms(pkg, scores=None, groups=None, rois=None, keep=BOXES) == E_ARG and "overlap" in err()
    with pytest.raises(pkg.WinoError, match="rc=-2"):
        pkg._check(_nms(pkg, max_out=0), "wino_batched_nms_hw")


def test_workspace_formula(pkg):
    hdr = open(os.path.join(ROOT, "include", "winograd_mi355x.h")).read()
    assert "S * R * ceil(R / 64) * 8 bytes" in hdr
    err = lambda: pkg.lib().wino_last_error_string().decode()
    for S, R in ((1, 1), (2, 64), (3, 65), (5, 2049), (1, 32768), (7, 700)):
        need = S * R * math.ceil(R / 64) * 8
        assert pkg.nms_workspace_bytes(S, R) == need
        assert _nms(pkg, S=S, R=R, ws_bytes=need - 1) == E_ARG and f"need {need} bytes" in err()
        assert _nms(pkg, S=S, R=R, ws_bytes=need, keep=BOXES) == E_ARG and "overlap" in err()
    assert pkg.nms_workspace_bytes(0, 5) == 0 and pkg.nms_workspace_bytes(5, 0) == 0


def test_python_ops_refuse_host_tensors(pkg):
    with pytest.raises(pkg.WinoError, match="no CPU path"):
        pkg.box_decode(torch.zeros(15, 64), torch.zeros(3, 4), torch.zeros(1, 2), 3, grid=(3, 5, 8, 8))
    with pytest.raises(pkg.WinoError, match="no CPU path"):
        pkg.batched_nms(torch.zeros(1, 8, 4))


# ---- decode: the references ------------------------------------------------------------------------------------------------
def torch_decode_fp32(c: bc.DecodeCase) -> np.ndarray:
    """BoxCoder.decode_single + clip_boxes_to_image as torchvision writes them, in torch float32."""
    head, hw, A = torch.from_numpy(c.head), torch.from_numpy(c.image_hw), c.A
    rows = head.shape[0]
    if c.grid:
        anc = torch.from_numpy(bc.grid_anchors(c.anchors, *c.grid, dtype=np.float32)).repeat(c.N, 1, 1)
    else:
        anc = torch.from_numpy(c.anchors)[:, None, :].expand(rows, A, 4)
    d = head[:, c.delta_col:c.delta_col + 4 * A].reshape(rows, A, 4)
    wx, wy, ww, wh = c.weights
    widths, heights = anc[..., 2] - anc[..., 0], anc[..., 3] - anc[..., 1]
    ctr_x, ctr_y = anc[..., 0] + 0.5 * widths, anc[..., 1] + 0.5 * heights
    dx, dy = d[..., 0] / wx, d[..., 1] / wy
    dw, dh = torch.clamp(d[..., 2] / ww, max=c.clamp), torch.clamp(d[..., 3] / wh, max=c.clamp)
    pcx, pcy = dx * widths + ctr_x, dy * heights + ctr_y
    pw, ph = torch.exp(dw) * widths, torch.exp(dh) * heights
    H = hw[:, 0].repeat_interleave(c.rpi)[:, None]
    W = hw[:, 1].repeat_interleave(c.rpi)[:, None]
    lo = torch.zeros(())
    out = torch.stack([torch.clamp(pcx - 0.5 * pw, min=lo, max=W), torch.clamp(pcy - 0.5 * ph, min=lo, max=H),
                       torch.clamp(pcx + 0.5 * pw, min=lo, max=W), torch.clamp(pcy + 0.5 * ph, min=lo, max=H)], dim=-1)
    assert out.dtype == torch.float32
    return out.reshape(c.N, c.rpi * A, 4).numpy()


def test_decode_case_lists():
    grid, box = bc.GRID_CASES, bc.BOX_MODE_CASES
    assert {c["grid"][:2] for c in grid} == set(bc.GRID_SHAPES) and {c["A"] for c in grid} == {1, 3, 12}
    assert {c["ld"] for c in grid} == {64, 128} and {c["N"] for c in grid} == {1, 3}
    assert {c["N"] * c["rows_per_image"] for c in box} == {1, 63, 65, 257} and {c["A"] for c in box} == {1, 2, 5, 91}
    assert all(c["weights"] == (10.0, 10.0, 5.0, 5.0) for c in box)
    for mode, cases in ((False, grid), (True, box)):
        for i in range(len(cases)):
            c = bc.decode_case(i, mode)
            if c.grid:   # image sizes that are no multiple of the stride
                assert all(h % c.grid[2] and w % c.grid[3] for h, w in c.image_hw.tolist()), c.image_hw
            want = c.reference()
            assert np.isfinite(want).all()
            assert (want[..., 0] <= want[..., 2]).all() and (want[..., 1] <= want[..., 3]).all()
    assert sum(bc.decode_case(i, m).above for m, cs in ((False, grid), (True, box)) for i in range(len(cs))) >= 50


def test_decode_fp32_restatement_holds_a_quarter_of_tight():
    """What entitles the GPU tests to TIGHT: torch's own arithmetic in fp32, and the reference's in fp32, are within
    TIGHT / 4 of the fp64 reference on every case.  Measured worst over the lists: 2.7e-7 (the outputs are clipped to
    images of at most 200 pixels, so an error is a few ulps of a coordinate)."""
    worst = 0.0
    for mode, cases in ((False, bc.GRID_CASES), (True, bc.BOX_MODE_CASES)):
        for i in range(len(cases)):
            c = bc.decode_case(i, mode)
            want = c.reference()
            for got in (torch_decode_fp32(c), c.reference(dtype=np.float32)):
                e = bc.rel_err(got, want)
                worst = max(worst, e)
                assert e < TIGHT / 4, (mode, i, e)
    print(f"worst fp32 restatement of the decode: {worst:.2e}")
    # the sweep over the legal launches: measured worst 4.3e-7
    worst = 0.0
    for i, c in enumerate(bc.decode_sweep_cases()):
        want = c.reference()
        for got in (torch_decode_fp32(c), c.reference(dtype=np.float32)):
            e = bc.rel_err(got, want)
            worst = max(worst, e)
            assert e < TIGHT / 4, (i, c.spec, e)
            if c.spec["hw"] == "zero":
                assert not got.any()
    print(f"worst fp32 restatement of the decode over the sweep: {worst:.2e}")


def test_decode_reference_propagates_nan_and_clamps_inf():
    c = bc.decode_case(4)   # 3 x 5, A = 3
    clean = c.reference()
    for k, coords in ((0, (0, 2)), (1, (1, 3)), (2, (0, 2)), (3, (1, 3))):
        head = c.head.copy()
        head[7, c.delta_col + 4 * 1 + k] = np.nan
        got = c.reference(head)
        hit = np.zeros(got.shape, dtype=bool)
        hit[0, 7 * 3 + 1, list(coords)] = True
        assert np.array_equal(np.isnan(got), hit) and np.array_equal(got[~hit], clean[~hit])
    head = c.head.copy()
    head[7, c.delta_col + 4 + 2] = np.inf           # dw = +Inf takes the clamp
    head[8, c.delta_col + 4 + 3] = -np.inf          # dh = -Inf: a box of height 0
    got = c.reference(head)
    assert np.isfinite(got).all() and got[0, 8 * 3 + 1, 1] == got[0, 8 * 3 + 1, 3]


# ---- NMS: the references and the generator ------------------------------------------------------------------------------
def torch_nms_fp32(boxes, scores, groups, iou_thresh, min_size, score_thresh=-math.inf, max_out=None):
    """Greedy NMS as torchvision's kernels compute it, in torch float32, one segment."""
    b = torch.from_numpy(boxes)
    R = b.shape[0]
    w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    dead = ~((w >= min_size) & (h >= min_size))
    if scores is not None:
        dead |= ~(torch.from_numpy(scores) >= score_thresh)
    g = None if groups is None else torch.from_numpy(groups)
    area, keep = w * h, []
    for i in range(R):
        if dead[i]:
            continue
        keep.append(i)
        if len(keep) >= (max_out or R):
            break
        lt, rb = torch.max(b[i, :2], b[i + 1:, :2]), torch.min(b[i, 2:], b[i + 1:, 2:])
        wh = (rb - lt).clamp(min=0)
        inter = wh[:, 0] * wh[:, 1]
        hit = inter / (area[i] + area[i + 1:] - inter) > iou_thresh
        if g is not None:
            hit &= g[i + 1:] == g[i]
        dead[i + 1:] |= hit
    return keep


def _all_cases():
    return [bc.nms_case(R, S) for R in bc.NMS_R for S in bc.NMS_S] + [bc.nms_case(R, 1) for R in bc.NMS_WIDE_R]


def test_nms_cases_keep_their_margins_within_the_redraw_cap():
    drawn = redrawn = 0
    for c in _all_cases():
        assert c.boxes.dtype == np.float32 and np.array_equal(c.boxes, np.round(c.boxes * 4) / 4)     # on the lattice
        assert (np.diff(c.scores, axis=1) <= 0).all()                                                  # priority order
        assert c.redrawn <= bc.REDRAW_CAP * c.drawn, (c.R, c.S, c.redrawn, c.drawn)
        drawn, redrawn = drawn + c.drawn, redrawn + c.redrawn
        for use_groups, use_scores in c.variants:
            keep, count, rois, results = c.expected(use_groups, use_scores)
            for r in results:
                assert not r.fragile
                assert r.iou_margin >= bc.IOU_MARGIN and r.score_margin >= bc.SCORE_MARGIN
                assert r.size_margin >= bc.size_margin(c.PARAMS["min_size"])
        if c.R >= 63:   # suppression happens, the thresholds bite, and groups matter
            keep, count, _, _ = c.expected()
            assert (count > 0).all() and (count < 0.9 * c.R).all(), (c.R, c.S, count)
            assert not np.array_equal(c.expected(False, False)[0], keep)
            if c.variants == bc.VARIANTS:
                assert not np.array_equal(c.expected(False, True)[0], keep)
                assert not np.array_equal(c.expected(True, False)[0], keep)
        assert bc.nms_case(c.R, c.S) is c
        again = bc.NmsCase(c.R, c.S, seed=7 * c.R + c.S) if c.R <= 129 else c
        assert np.array_equal(again.boxes, c.boxes)                                                    # seeded
    print(f"drawn {drawn}, redrawn {redrawn}")


def test_nms_fp32_restatement_makes_the_same_decisions():
    """The walk in fp32 -- torch's arithmetic for R <= 700, the reference's own for every case -- keeps exactly what the
    fp64 walk keeps, in every variant, and with groups and scores at max_out below, at and above the kept count."""
    for c in _all_cases():
        for use_groups, use_scores in c.variants:
            cut = (use_groups, use_scores) == bc.VARIANTS[0] and c.R <= 2049
            sc, g = (c.scores if use_scores else None), (c.groups if use_groups else None)
            p = dict(c.PARAMS)
            if not use_scores:
                p.pop("score_thresh")
            keep, count, _, _ = c.expected(use_groups, use_scores)
            full = int(count[0])
            for max_out in ((None, max(full // 2, 1), max(full, 1), full + 3) if cut else (None,)):
                want = c.expected(use_groups, use_scores, max_out)[0]
                got = bc.batched_nms_reference(c.boxes, sc, g, max_out=max_out, dtype=np.float32, **p)[0]
                assert np.array_equal(got, want), (c.R, c.S, use_groups, use_scores, max_out)
                if c.R <= 700 and max_out is None and (use_groups, use_scores) in ((True, True), (False, False)):
                    for s in range(c.S):
                        k = torch_nms_fp32(c.boxes[s], None if sc is None else sc[s], None if g is None else g[s],
                                           max_out=max_out, **p)
                        assert k == [v for v in want[s].tolist() if v >= 0], (c.R, s, max_out)


def test_every_case_class_has_its_property():
    cc = bc.class_case()
    assert len(cc.NAMES) == cc.boxes.shape[0] == 6
    keep, count, rois, results = cc.expected()
    for r in results:
        assert not r.fragile and r.iou_margin >= bc.IOU_MARGIN and r.size_margin >= bc.size_margin(cc.PARAMS["min_size"])
    by = dict(zip(cc.NAMES, range(6)))
    R, M = cc.R, cc.MAX_OUT
    assert count[by["nothing_kept"]] == 0 and (keep[by["nothing_kept"]] == -1).all()
    assert cc.expected(max_out=R)[1][by["all_kept"]] == R
    assert count[by["all_identical"]] == 1 and keep[by["all_identical"], 0] == 0
    assert count[by["more_than_max_out"]] == M and keep[by["more_than_max_out"]].tolist() == list(range(M))
    assert cc.expected(max_out=R)[1][by["more_than_max_out"]] > M
    apart, merged = cc.expected(max_out=R), cc.expected(use_groups=False, max_out=R)
    assert apart[1][by["groups_apart"]] == R and merged[1][by["groups_apart"]] == R // 2
    s = by["clusters"]
    assert 0 < count[s] < R
    # the fixed-size outputs: -1 after the count, rois = (segment, box) then (-1, 0, 0, 0, 0)
    for s in range(6):
        k = int(count[s])
        assert (keep[s, :k] >= 0).all() and (np.diff(keep[s, :k]) > 0).all() and (keep[s, k:] == -1).all()
        assert (rois[s, :k, 0] == s).all() and np.array_equal(rois[s, :k, 1:], cc.boxes[s][keep[s, :k]])
        assert (rois[s, k:, 0] == -1).all() and (rois[s, k:, 1:] == 0).all()


def test_reference_never_keeps_a_nan_box():
    c = bc.nms_case(65, 2)
    boxes = c.boxes.copy()
    boxes[0, ::7, 1] = np.nan
    keep, count, _, _ = bc.batched_nms_reference(boxes, c.scores, c.groups, **c.PARAMS)
    assert not set(range(0, 65, 7)) & set(keep[0].tolist()) and count[0] > 0
    assert np.array_equal(keep[1], c.expected()[0][1])
    boxes[0] = np.nan
    assert bc.batched_nms_reference(boxes, c.scores, c.groups, **c.PARAMS)[1].tolist() == [0, int(c.expected()[1][1])]


# ---- the sweeps: decode layouts, NMS at equality, parameters, off-lattice boxes, many segments ---------------------------
def test_decode_sweep_has_every_pin():
    specs = bc.decode_sweep_specs()
    cases = bc.decode_sweep_cases()
    assert len(specs) == 40 and [c.spec for c in cases] == specs
    grid = [s for s in specs if s["grid"]]
    box = [s for s in specs if not s["grid"]]
    assert {s["N"] for s in specs} == {1, 2, 3, 4} and {s["A"] for s in specs} == set(bc.SWEEP_A)
    for mode in (grid, box):
        assert {s["score_col"] is None for s in mode} == {True, False}
    # the leading dimension: 4A, 4A + 1, 5A, 5A + 3, odd ones and ones that are no multiple of 4
    for form in (lambda A: 4 * A, lambda A: 4 * A + 1, lambda A: 5 * A, lambda A: 5 * A + 3):
        assert any(s["ld"] == form(s["A"]) for s in specs)
    assert any(s["ld"] % 2 for s in specs) and any(s["ld"] % 4 for s in specs) and any(s["ld"] % 64 == 0 for s in specs)
    # the columns: deltas off a multiple of 4, deltas before the scores, the scores against the row's end, none
    assert any(s["delta_col"] % 4 for s in specs) and any(s["delta_col"] == 0 for s in specs)
    assert any(s["score_col"] is not None and s["delta_col"] < s["score_col"] for s in specs)
    assert any(s["score_col"] is not None and s["score_col"] + s["A"] == s["ld"] for s in specs)
    assert any(s["score_col"] == 0 for s in specs) and any(s["delta_col"] + 4 * s["A"] == s["ld"] for s in specs)
    # grid mode: single rows, columns and cells, unequal strides and a stride of 1
    shapes = {s["grid"][:2] for s in grid}
    assert (1, 1) in shapes and any(h == 1 and w > 1 for h, w in shapes) and any(w == 1 and h > 1 for h, w in shapes)
    assert max(h for h, _ in shapes) == 40 and max(w for _, w in shapes) == 40
    assert any(s["grid"][2] != s["grid"][3] for s in grid) and any(s["grid"][2:] == (1, 1) for s in grid)
    assert {s["grid"][2:] for s in grid} == set(bc.SWEEP_STRIDES)
    # boxes mode: total at the edge of a 256-thread block
    assert {s["rows_per_image"] for s in box if s["A"] == 1 and s["N"] == 1} == set(bc.SWEEP_BOX_ROWS)
    for key, values in (("weights", bc.SWEEP_WEIGHTS), ("clamp", bc.SWEEP_CLAMPS), ("hw", bc.SWEEP_HW),
                        ("slice", bc.SWEEP_SLICES)):
        assert {s[key] for s in specs} == set(values), key
    assert any(s["slice"][0] > 0 and s["slice"][1] > 0 for s in specs)
    for c in cases:
        want = c.reference()
        assert np.isfinite(want).all() and np.isfinite(c.head).all()
        d = c.head[:, c.delta_col:c.delta_col + 4 * c.A].reshape(-1, c.A, 4) / np.asarray(c.weights, dtype=np.float32)
        assert float(np.exp(d[..., 2:].max())) < 1e4                       # whatever the clamp
        if c.spec["hw"] == "zero":
            assert not want.any() and bc.rel_err(want, want) == 0.0 and bc.rel_err(want + 1e-30, want) == bc.INF
        if c.spec["hw"] == "nothing_clips":
            assert float(want.max()) < float(c.image_hw.min())
        if c.spec["hw"] == "fractional":
            assert (c.image_hw % 1 != 0).all()
    assert sum(c.above for c in cases) >= 50
    clipped = [c for c in cases if c.spec["hw"] in ("usual", "fractional")]
    at_edge = [bool((c.reference() == c.image_hw[:, None, [1, 0, 1, 0]]).any()) for c in clipped]
    assert sum(at_edge) >= 0.75 * len(clipped), at_edge                   # (a launch of one or two boxes may miss the edge)


def test_equality_family_is_exact_in_both_precisions():
    """Every run of the equality family: the fp32 restatement keeps what the fp64 reference keeps, with and without
    groups; the pair at equality is kept at its IoU and above, suppressed a neighbour below; a side or a score equal
    to its threshold makes a candidate, its neighbour below does not."""
    four = np.array([[0, 0, 8, 4], [0, 0, 4, 4], [100, 0, 104, 4], [100, 0, 103, 4]], dtype=np.float32)
    for dtype in (np.float64, np.float32):
        assert bc.nms_reference(four, iou_thresh=0.5, dtype=dtype).keep == [0, 1, 2]
        assert bc.nms_reference(four, iou_thresh=0.75, dtype=dtype).keep == [0, 1, 2, 3]
        assert bc.nms_reference(four, iou_thresh=bc.f32_below(0.5), dtype=dtype).keep == [0, 2]
    c = bc.equality_case()
    assert bc.equality_case() is c and c.boxes.shape == (c.S, c.R, 4) and c.R == 130
    assert {rows for rows in c.pair_rows} == {(0, 63), (63, 64), (0, 129), (64, 127)}
    thr = c.SCORE_THRESH
    for iou, ms in c.runs():
        for use_groups in (True, False):
            keep, count, rois, _ = c.expected(iou, ms, use_groups)
            got = c.expected(iou, ms, use_groups, dtype=np.float32)
            assert np.array_equal(got[0], keep) and np.array_equal(got[1], count) and np.array_equal(got[2], rois)
            for s in range(c.S):
                k = set(keep[s, :count[s]].tolist())
                w, h = c.boxes[s, :, 2] - c.boxes[s, :, 0], c.boxes[s, :, 3] - c.boxes[s, :, 1]
                cand = (w >= ms) & (h >= ms) & (c.scores[s] >= np.float32(thr))
                (i, j), (_, _, v) = c.pair_rows[s], c.PAIRS[s // 4]
                lone = np.ones(c.R, dtype=bool)
                lone[[i, j]] = False
                assert k - {i, j} == set(np.nonzero(cand & lone)[0].tolist())      # a box that overlaps nothing: kept iff candidate
                if cand[i] and cand[j]:
                    assert i in k and (j in k) == (not v > iou), (s, iou, ms)
        # the thresholds themselves are met: sides and scores equal to them, and the neighbours on both sides
        w, h = c.boxes[..., 2] - c.boxes[..., 0], c.boxes[..., 3] - c.boxes[..., 1]
        for side in (ms - 0.25, ms, ms + 0.25):
            assert (w == side).any() and (h == side).any()
    for r in (0, 63, 64, 129):                                            # lanes 0 and 63 of a block, and the next block's
        w, h = c.boxes[:, r, 2] - c.boxes[:, r, 0], c.boxes[:, r, 3] - c.boxes[:, r, 1]
        for v in (bc.f32_below(thr), thr, bc.f32_above(thr)):
            assert (c.scores[:, r] == np.float32(v)).any(), (v, r)
        for side in (2.0, 0.25):
            assert ((w == side) | (h == side)).any(), (side, r)
    # pairs that are both candidates exist at equality with a threshold score on the suppressor
    assert sum(c.scores[s, c.pair_rows[s][0]] == np.float32(thr) for s in range(c.S)) == c.S // 2


@pytest.mark.parametrize("R", bc.SWEEP_R)
def test_nms_sweep_keeps_its_margins_in_every_combination(R):
    """The parameter and geometry sweep: the redraw cap holds, every special kind is in every segment, every group id is
    used, and the fp32 walk equals the fp64 walk under each of the 96 combinations."""
    c = bc.sweep_nms_case(R)
    combos = bc.sweep_combos()
    assert len(combos) == 96 and len(set(combos)) == 96
    assert {x[0] for x in combos} == set(bc.SWEEP_IOU) and {x[1] for x in combos} == set(bc.SWEEP_MIN_SIZE)
    assert {x[2] for x in combos} == set(bc.SWEEP_SCORE_THRESH) and {x[3] for x in combos} == {True, False}
    assert c.S == 3 and c.redrawn <= bc.REDRAW_CAP * c.drawn, (c.redrawn, c.drawn)
    assert set(np.unique(c.groups).tolist()) == set(bc.SWEEP_GROUPS)
    finite = np.where(np.isfinite(c.boxes), c.boxes, 0)
    assert np.array_equal(finite, np.round(finite * 4) / 4) and float(np.abs(finite).max()) < 4096 and not np.isnan(c.boxes).any()
    for s in range(c.S):
        b = c.boxes[s]
        with np.errstate(invalid="ignore"):
            w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
        assert ((w == 0) & (h > 0)).any() and ((h == 0) & (w > 0)).any() and (w < 0).any() and (h < 0).any()
        assert ((w < 0) & (h < 0)).any()
        point = np.nonzero((w == 0) & (h == 0))[0]
        assert any(np.array_equal(b[i], b[j]) for i in point for j in point if i < j)          # an identical zero-area pair
        assert np.isinf(b).any(axis=1).sum() >= 5 and (np.isinf(b).sum(axis=1) == 4).any()
        assert (b == -bc.INF).any() and (b == bc.INF).any()
        touch = (b[:, None, 0] == b[None, :, 2]) & (b[:, None, 1] < b[None, :, 3]) & (b[None, :, 1] < b[:, None, 3])
        assert touch.any()                                                                      # shares an edge: intersection 0
    kept = set()
    for combo in combos:
        keep, count, rois, results = c.expected(combo)
        for r in results:
            assert r.iou_margin >= bc.IOU_MARGIN and r.score_margin >= bc.SCORE_MARGIN, combo
        got = c.expected(combo, dtype=np.float32)
        assert np.array_equal(got[0], keep) and np.array_equal(got[1], count), combo
        assert np.array_equal(got[2].view(np.int32), rois.view(np.int32)), combo
        kept.add(tuple(count.tolist()))
    assert len(kept) >= 20                                                  # the parameters bite
    print(f"R={R}: drawn {c.drawn}, redrawn {c.redrawn}, {len(kept)} distinct count vectors")


@pytest.mark.parametrize("R", bc.OFF_LATTICE_R)
def test_off_lattice_case_keeps_its_margins(R):
    c = bc.off_lattice_case(R)
    assert c.S == 2 and c.boxes.dtype == np.float32 and c.redrawn <= bc.REDRAW_CAP * c.drawn, (c.redrawn, c.drawn)
    assert (c.boxes != np.round(c.boxes * 4) / 4).mean() > 0.99             # off the lattice
    w, h = c.boxes[..., 2] - c.boxes[..., 0], c.boxes[..., 3] - c.boxes[..., 1]
    assert 2.5 < float(min(w.min(), h.min())) < 4.5 and 300 < float(max(w.max(), h.max())) < 400
    assert (np.diff(c.scores, axis=1) <= 0).all()
    for use_groups, use_scores in c.variants:
        p = dict(c.PARAMS)
        if not use_scores:
            p.pop("score_thresh")
        keep, count, rois, results = c.expected(use_groups, use_scores)
        for r in results:
            assert not r.fragile and r.iou_margin >= bc.IOU_MARGIN and r.score_margin >= bc.SCORE_MARGIN
            assert r.size_margin >= bc.size_margin(c.PARAMS["min_size"])
        got = bc.batched_nms_reference(c.boxes, c.scores if use_scores else None, c.groups if use_groups else None,
                                       dtype=np.float32, **p)
        assert np.array_equal(got[0], keep) and np.array_equal(got[1], count)
        assert (count > 0.15 * R).all() and (count < 0.6 * R).all(), count
    print(f"R={R}: kept {c.expected()[1].tolist()}, redrawn {c.redrawn}")


def test_limit_cases_keep_their_margins():
    """nb == W at three scan widths; the largest R is left to the GPU test (its walk takes seconds)."""
    for R in bc.NMS_LIMIT_R[:2]:
        c = bc.nms_case(R, 1)
        assert -(-R // 64) in (64, 256) and c.redrawn <= bc.REDRAW_CAP * c.drawn
        for use_groups, use_scores in c.variants:
            keep, count, _, results = c.expected(use_groups, use_scores)
            assert not results[0].fragile and 0 < count[0] < 0.9 * R
    assert bc.NMS_LIMIT_R[-1] == bc.NMS_MAX_R == 32768


def test_one_box_sources_and_tiling():
    boxes, scores, keep, count, rois = bc.one_box_sources()
    K = boxes.shape[0]
    assert K == 300 and boxes.shape == (K, 1, 4) and keep.shape == (K, 1) and rois.shape == (K, 1, 5)
    w, h = boxes[:, 0, 2] - boxes[:, 0, 0], boxes[:, 0, 3] - boxes[:, 0, 1]
    cand = (w >= 2.0) & (h >= 2.0) & (scores[:, 0] >= np.float32(0.25))
    assert np.array_equal(count, cand.astype(np.int32)) and np.array_equal(keep[:, 0], np.where(cand, 0, -1))
    for side in (1.75, 2.0, 2.25):
        assert (w == side).any() and (h == side).any()
    for v in (bc.f32_below(0.25), 0.25, bc.f32_above(0.25)):
        assert ((scores[:, 0] == np.float32(v)) & (w >= 2.0) & (h >= 2.0)).any()
    assert 0.2 < cand.mean() < 0.8
    got = bc.batched_nms_reference(boxes, scores, None, max_out=1, dtype=np.float32, **bc.ONE_BOX_PARAMS)
    assert np.array_equal(got[0], keep) and np.array_equal(got[2], rois)
    S = 2 * K + 7
    tk, tc, tr = bc.tile_segments(keep, count, rois, S)
    want = bc.batched_nms_reference(np.tile(boxes, (3, 1, 1))[:S], np.tile(scores, (3, 1))[:S], None, max_out=1,
                                    **bc.ONE_BOX_PARAMS)
    assert np.array_equal(tk, want[0]) and np.array_equal(tc, want[1]) and np.array_equal(tr.view(np.int32), want[2].view(np.int32))
    assert np.float32((1 << 24) - 1) == (1 << 24) - 1                       # float(s) is exact for every s the library takes


# ---- the detector's seed ---------------------------------------------------------------------------------------------------
def test_detector_seed_keeps_ten_times_the_margins(pkg):
    """The fp64 forward of box_cases.DETECTOR on the CPU: every NMS decision of both stages keeps ten times the generator's
    margins (the seed is chosen so that this holds), no two logits or scores that are ranked tie, both images end with
    detections, and the exported names exist."""
    import importlib
    R = importlib.import_module("cuda_winograd_amd.resnet")
    ref = bc.detector_reference_forward(R)
    print(ref["margins"], ref["filt"]["count"], ref["cand"]["count"])
    bc.assert_margins(ref["margins"], 10.0)
    assert int(ref["cand"]["count"].min()) > 0 and not bool(ref["cand"]["overflow"].any())
    assert int((ref["filt"]["rois"][:, :, 0] >= 0).sum()) == int(ref["filt"]["count"].sum())
    for name in ("RPN", "FasterRCNN"):
        assert hasattr(pkg, name)
    det = importlib.import_module("cuda_winograd_amd.detection")
    assert torch.equal(det.base_anchors((32,), (0.5, 1.0, 2.0)), bc.base_anchors((32,), (0.5, 1.0, 2.0)))
    assert det.base_anchors((32,), (0.5, 1.0, 2.0)).tolist() == [[-23, -11, 23, 11], [-16, -16, 16, 16], [-11, -23, 11, 23]]
    assert det.SCORE_THRESH_STRICT == bc.SCORE_THRESH
    sd = {k[4:]: v for k, v in ref["sd"].items() if k.startswith("rpn.")}
    with pytest.raises(pkg.WinoError, match="missing key 'head.bbox_pred.bias'"):
        det.RPN.from_state_dict({k: v for k, v in sd.items() if k != "head.bbox_pred.bias"}, 64)
    with pytest.raises(pkg.WinoError, match="unexpected key 'mask.weight'"):
        pkg.FasterRCNN.from_state_dict(dict(ref["sd"], **{"mask.weight": torch.zeros(1)}), "resnet18", out_channels=64)
    legacy = {k.replace("head.conv.0.0", "head.conv"): v for k, v in sd.items()}
    assert set(det.expected_rpn_keys(legacy, 64, 3)) == set(legacy)
