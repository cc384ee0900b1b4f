"""Host tests of the mask paste: the fp64 reference of tests/mask_cases.py against a literal transcription of
torchvision's paste_masks_in_image on torch-CPU fp64 F.interpolate, the box generator's classes and margins, the lattice
case, and what paste_masks and MaskRCNN refuse before the library or a device is touched."""
import importlib

import numpy as np
import pytest
import torch

import mask_cases as mc

SHAPES = ((40, 56), (37, 53), (5, 1), (130, 19))
MS = (2, 8, 28, 62)
N, D, NCLS = 2, 6, 5


# ---- torchvision, transcribed (roi_heads.py: maskrcnn_inference, expand_boxes, expand_masks, paste_mask_in_image) -----------
def tv_expand_boxes(boxes, scale):
    w_half = (boxes[:, 2] - boxes[:, 0]) * 0.5
    h_half = (boxes[:, 3] - boxes[:, 1]) * 0.5
    x_c = (boxes[:, 2] + boxes[:, 0]) * 0.5
    y_c = (boxes[:, 3] + boxes[:, 1]) * 0.5
    w_half *= scale
    h_half *= scale
    boxes_exp = torch.zeros_like(boxes)
    boxes_exp[:, 0] = x_c - w_half
    boxes_exp[:, 2] = x_c + w_half
    boxes_exp[:, 1] = y_c - h_half
    boxes_exp[:, 3] = y_c + h_half
    return boxes_exp


def tv_expand_masks(mask, padding):
    M = mask.shape[-1]
    scale = float(M + 2 * padding) / M
    return torch.nn.functional.pad(mask, (padding,) * 4), scale


def tv_paste_mask_in_image(mask, box, im_h, im_w):
    TO_REMOVE = 1
    w = int(box[2] - box[0] + TO_REMOVE)
    h = int(box[3] - box[1] + TO_REMOVE)
    w = max(w, 1)
    h = max(h, 1)
    mask = mask.expand((1, 1, -1, -1))
    mask = torch.nn.functional.interpolate(mask, size=(h, w), mode="bilinear", align_corners=False)
    mask = mask[0][0]
    im_mask = torch.zeros((im_h, im_w), dtype=mask.dtype)
    x_0 = max(int(box[0]), 0)
    x_1 = min(int(box[2]) + 1, im_w)
    y_0 = max(int(box[1]), 0)
    y_1 = min(int(box[3]) + 1, im_h)
    if x_0 >= x_1 or y_0 >= y_1:
        return im_mask   # (the header's rule: an empty window is a zero plane; torch's negative slice ends are not copied)
    im_mask[y_0:y_1, x_0:x_1] = mask[(y_0 - int(box[1])):(y_1 - int(box[1])), (x_0 - int(box[0])):(x_1 - int(box[0]))]
    return im_mask


def torchvision_paste(logits, labels, boxes, im_h, im_w):
    """One image: logits [D][classes][M][M] (fp64), labels [D], boxes [D][4] float32 -> [D][im_h][im_w] fp64."""
    prob = torch.sigmoid(logits)[torch.arange(logits.shape[0]), labels][:, None]
    masks, scale = tv_expand_masks(prob, 1)
    bx = tv_expand_boxes(boxes.clone(), scale).to(dtype=torch.int64)
    return torch.stack([tv_paste_mask_in_image(m[0], b, im_h, im_w) for m, b in zip(masks, bx)])


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_reference_is_torchvision(H, W, M):
    boxes, hw, _ = mc.paste_boxes(N, D, H, W, M)
    logits, labels = mc.paste_logits(N * D, NCLS, M), mc.paste_labels(N * D, NCLS)
    want, margin = mc.paste_reference(logits, labels, boxes, hw, H, W)
    assert margin >= mc.INT_MARGIN
    im_h, im_w = mc.image_ints(hw, H, W)
    worst = 0.0
    for n in range(N):
        sl = slice(n * D, (n + 1) * D)
        tv = torchvision_paste(torch.from_numpy(logits[sl]).double(), torch.from_numpy(labels[sl]).long(),
                               torch.from_numpy(boxes[sl]), int(im_h[n]), int(im_w[n])).numpy()
        worst = max(worst, float(np.abs(want[n, :, :im_h[n], :im_w[n]] - tv).max()))
        assert (want[n, :, im_h[n]:] == 0).all() and (want[n, :, :, im_w[n]:] == 0).all()
    print(f"H={H} W={W} M={M}: max |reference - torchvision| = {worst:.2e}, int_margin {margin:.2e}")
    assert worst < 1e-12


def test_generator_has_every_class_and_keeps_its_margins():
    seen = set()
    for H, W in SHAPES:
        for M in MS:
            boxes, hw, names = mc.paste_boxes(N, D, H, W, M)
            assert (mc.int_margin(boxes, M) >= mc.INT_MARGIN).all()
            b32, f32 = mc.box_integers(boxes, M, np.float32)
            b64, _ = mc.box_integers(boxes, M, np.float64)
            assert f32.all() and (b32 == b64).all()
            im_h, im_w = mc.image_ints(hw, H, W)
            for k, name in enumerate(names):
                if name != "random":
                    assert name in mc.properties(b32[k], int(im_h[k // D]), int(im_w[k // D]), H, W)
            if (H, W) in ((40, 56), (130, 19)):
                assert set(names) >= set(mc.CLASSES), (H, W, M, set(mc.CLASSES) - set(names))
            seen |= set(names)
    assert seen >= set(mc.CLASSES)


@pytest.mark.parametrize("M", mc.LATTICE_M)
def test_lattice_boxes_are_exact_and_truncate_toward_zero(M):
    H, W = 40, 56
    boxes, hw = mc.lattice_boxes(N, D, H, W, M)
    e = mc.expand(boxes, M, np.float64)
    bi, _ = mc.box_integers(boxes, M, np.float32)
    neg = (e < 0) & (e > -1)
    assert neg.any() and (bi[neg] == 0).all() and (np.floor(e[neg]) == -1).all()
    assert ((e == np.rint(e)) & (e > 0)).any()
    want, _ = mc.paste_reference(mc.paste_logits(N * D, NCLS, M), mc.paste_labels(N * D, NCLS), boxes, hw, H, W)
    assert all((want[n, d] != 0).any() for n in range(N) for d in range(D))


def test_to_gemm_rows_is_the_headers_index():
    M, P, ld = 4, 2, 8
    lg = mc.paste_logits(3, NCLS, M)
    rows = mc.to_gemm_rows(lg, ld)
    for r, c, Y, X in ((0, 0, 0, 0), (1, 4, 3, 2), (2, 2, 1, 3)):
        assert rows[(((r * P + (Y >> 1)) * P + (X >> 1)) * 4 + (Y & 1) * 2 + (X & 1)), c] == lg[r, c, Y, X]
    assert np.isnan(rows[:, NCLS:]).all()


def test_reference_special_planes():
    H, W, M = 20, 24, 4
    boxes, hw, _ = mc.paste_boxes(N, D, H, W, M)
    boxes = boxes.copy()
    labels = mc.paste_labels(N * D, NCLS).copy()
    labels[1], labels[2] = -1, NCLS
    boxes[3, 2] = np.nan
    boxes[7, 0] = np.inf
    want, _ = mc.paste_reference(mc.paste_logits(N * D, NCLS, M), labels, boxes, hw, H, W)
    im_h, im_w = mc.image_ints(hw, H, W)
    assert (want[0, 1] == 0).all() and (want[0, 2] == 0).all()
    assert np.isnan(want[0, 3, :im_h[0], :im_w[0]]).all()
    assert np.isnan(want[1, 1, :im_h[1], :im_w[1]]).all() and (want[1, 1, im_h[1]:] == 0).all() and (want[1, 1, :, im_w[1]:] == 0).all()
    assert int(np.isnan(want).any(axis=(2, 3)).sum()) == 2


# ---- what the wrapper and the model refuse before the library or a device is touched --------------------------------------
def test_paste_masks_refuses_bad_arguments(pkg):
    lg, lb = torch.zeros(2, 3, 4, 4), torch.zeros(2, dtype=torch.int32)
    bx, hw = torch.zeros(2, 4), torch.ones(1, 2)
    for kw, msg in ((dict(layout="nchw"), "layout"), (dict(H=0), "bad plane"), (dict(W=-1), "bad plane"),
                    (dict(H=1 << 16, W=1 << 15), "bad plane"), (dict(threshold=float("nan")), "NaN"),
                    (dict(want_out=False), "neither"), (dict(), "CUDA")):
        args = dict(H=8, W=8)
        args.update(kw)
        with pytest.raises(pkg.WinoError, match=msg):
            pkg.paste_masks(lg, lb, bx, hw, **args)


def test_mask_rcnn_splits_and_validates_the_state_dict(pkg):
    import roi_cases as rc
    det = importlib.import_module("cuda_winograd_amd.detection")
    mask = {"roi_heads." + k: v for k, v in rc.mask_head_state_dict(64, NCLS).items()}
    sd = dict(mask)
    sd.update({"backbone.body.conv1.weight": torch.zeros(1), "rpn.head.cls_logits.bias": torch.zeros(3),
               "roi_heads.box_head.fc6.bias": torch.zeros(1)})
    rest, got = det.split_mask_state_dict(sd)
    assert sorted(got) == sorted(k[len("roi_heads."):] for k in mask)
    assert sorted(rest) == ["backbone.body.conv1.weight", "roi_heads.box_head.fc6.bias", "rpn.head.cls_logits.bias"]
    assert all(got[k[len("roi_heads."):]] is v for k, v in mask.items())
    assert det.validate_mask_head_state_dict(got, 64) == NCLS
    make = lambda d, **kw: pkg.MaskRCNN.from_state_dict(d, "resnet18", out_channels=64, **kw)
    with pytest.raises(pkg.WinoError, match="masks must be one of"):
        make(sd, masks="logits")
    for P in (0, 7, 32):
        with pytest.raises(pkg.WinoError, match="mask_P"):
            make(sd, mask_P=P)
    with pytest.raises(pkg.WinoError, match="NaN"):
        make(sd, mask_threshold=float("nan"))
    missing = {k: v for k, v in sd.items() if k != "roi_heads.mask_predictor.conv5_mask.bias"}
    with pytest.raises(pkg.WinoError, match="missing key 'mask_predictor.conv5_mask.bias'"):
        make(missing)
    extra = dict(sd, **{"roi_heads.mask_head.4.0.weight": torch.zeros(64, 64, 3, 3)})
    with pytest.raises(pkg.WinoError, match="unexpected key 'mask_head.4.0.weight'"):
        make(extra)
    wrong = dict(sd, **{"roi_heads.mask_head.0.0.bias": torch.zeros(32)})
    with pytest.raises(pkg.WinoError, match="has shape"):
        make(wrong)
    with pytest.raises(pkg.WinoError, match="missing key 'mask_predictor.mask_fcn_logits.weight'"):
        make({k: v for k, v in sd.items() if not k.startswith("roi_heads.mask_")})
    # what is left is FasterRCNN's to judge, after the split
    with pytest.raises(pkg.WinoError, match="unexpected key 'mask_head.0.0.weight' for Faster R-CNN"):
        make(dict(sd, **{"mask_head.0.0.weight": torch.zeros(1)}))
