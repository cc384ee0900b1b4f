"""The fp64 reference of RetinaNet for tests/test_retinanet_host.py and tests/test_gpu_retinanet.py: a transcription of
torchvision's RetinaNetHead (RetinaNetClassificationHead / RetinaNetRegressionHead without a norm layer) and of
RetinaNet.postprocess_detections, stage by stage, each stage usable on the device's own input to it, and the seeded
detector the GPU test runs: resnet18, 64 channels, 5 classes, N = 2 at 64 x 96 (levels 8x12, 4x6, 2x3, 1x2, 1x1).

postprocess_detections per image and level: scores = sigmoid(logits).flatten(); keep = scores > score_thresh; the
topk_candidates best of those; anchor = index // K, label = index % K; decode_single + clip.  Then the levels are
concatenated, batched_nms(boxes, scores, labels, nms_thresh) keeps in descending score order, and the first
detections_per_img survive.  Every discrete stage reports the smallest margin of the decisions it made (the distance
of a score from the threshold, the gap between neighbouring scores, the NMS's IoU margin), and the test asserts the
margins of tests/box_cases.py on them."""
import math

import numpy as np
import torch

import box_cases as bc

RETINA = dict(arch="resnet18", out_channels=64, classes=5, N=2, H=64, W=96, topk=40, detections=10, seed=12,
              score_thresh=0.05, nms_thresh=0.5,
              sizes=((8, 10, 12), (16, 20, 25), (32, 40, 50), (64, 80, 101), (128, 161, 203)), ratios=(0.5, 1.0, 2.0))
LEVELS = ("0", "1", "2", "p6", "p7")
LEVEL_HW = [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)]
A = 9
CONVS = 4


def head_state_dict(C: int, A: int, classes: int, seed: int = 0, legacy: bool = False, g=None):
    """torchvision's RetinaNetHead keys below `head.`: He-scaled towers, a classification output whose logits straddle the
    0.05 threshold, small regression deltas.  legacy: the towers as conv.{2i} (a Sequential of Conv2d and ReLU)."""
    g = g or torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    stem = (lambda i: f"conv.{2 * i}") if legacy else (lambda i: f"conv.{i}.0")
    sd = {}
    # (the class biases spread around logit(0.05) = -2.94: about half the channels pass the threshold, so a level of 45
    # scores leaves padding rows and a level of thousands fills its top-k)
    for head, last, width, wscale, bscale, bias in (("classification_head", "cls_logits", A * classes, 2.0, 1.5, -3.0),
                                                    ("regression_head", "bbox_reg", 4 * A, 0.5, 0.1, 0.0)):
        for i in range(CONVS):
            sd[f"{head}.{stem(i)}.weight"] = rn(C, C, 3, 3) * (2.0 / (9 * C)) ** 0.5
            sd[f"{head}.{stem(i)}.bias"] = rn(C) * 0.1
        sd[f"{head}.{last}.weight"] = rn(width, C, 3, 3) * (wscale / (9 * C)) ** 0.5
        sd[f"{head}.{last}.bias"] = rn(width) * bscale + bias
    return sd


def detector_state_dict(resnet_module):
    """The seeded torchvision-named state dict of RETINA: backbone.* and head.* (float32), and the backbone's parts."""
    import fpn_p6p7_reference as fr
    d = RETINA
    fpn_sd, body = fr.p6p7_random_state_dict(torch, resnet_module, d["arch"], d["out_channels"], seed=d["seed"])
    sd = {"backbone." + k: v for k, v in fpn_sd.items()}
    sd.update({"head." + k: v for k, v in head_state_dict(d["out_channels"], A, d["classes"], seed=d["seed"] + 5).items()})
    return sd, fpn_sd, body


def detector_input():
    d = RETINA
    return torch.rand(d["N"], 3, d["H"], d["W"], generator=torch.Generator().manual_seed(d["seed"] + 1)) - 0.5


def head_reference(sd, feats):
    """fp64 RetinaNetHead on NHWC level maps {"0", "1", "2", "p6", "p7"} -> per level (class logits [N][h][w][A K] with
    channel a K + k, box regression [N][h][w][4 A]): torchvision's view(N, -1, K, H, W).permute(0, 3, 4, 1, 2).reshape(N,
    -1, K) is the NHWC flattening of exactly these channels."""
    F = torch.nn.functional
    w = {k[len("head."):]: v.double() for k, v in sd.items() if k.startswith("head.")}
    out = []
    for name in LEVELS:
        x = feats[name].double().permute(0, 3, 1, 2)
        maps = []
        for head, last in (("classification_head", "cls_logits"), ("regression_head", "bbox_reg")):
            t = x
            for i in range(CONVS):
                t = torch.relu(F.conv2d(t, w[f"{head}.conv.{i}.0.weight"], w[f"{head}.conv.{i}.0.bias"], padding=1))
            maps.append(F.conv2d(t, w[f"{head}.{last}.weight"], w[f"{head}.{last}.bias"], padding=1).permute(0, 2, 3, 1))
        out.append(tuple(maps))
    return out


def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))


def level_select_reference(logits, topk: int, score_thresh: float):
    """One level of postprocess_detections on class logits [N][n] (the flat (HWA, K) order): per image the indices of the
    min(topk, candidates) best scores among sigmoid(logit) > score_thresh, best first, in fp64.  Returns (idx [N][k] int32
    padded with -1, count [N], thresh_margin: the smallest |score - score_thresh|, tie_gap: the smallest gap between two
    neighbours among the kept scores and the first one left out -- the decisions the order and the cut rest on -- 0 for a
    tie)."""
    logits = np.asarray(logits)
    N, n = logits.shape
    k = min(topk, n)
    idx, count = np.full((N, k), -1, dtype=np.int32), np.zeros(N, dtype=np.int32)
    scores = sigmoid64(logits)
    thresh_margin, tie_gap = float(np.abs(scores - score_thresh).min()), bc.INF
    for i in range(N):
        cand = np.nonzero(scores[i] > score_thresh)[0]
        order = cand[np.argsort(-scores[i, cand], kind="stable")]
        c = min(k, len(order))
        idx[i, :c], count[i] = order[:c], c
        if len(order) > 1:   # (a tie below the first score left out decides nothing)
            tie_gap = min(tie_gap, float(np.abs(np.diff(scores[i, order[:k + 1]])).min()))
    return idx, count, thresh_margin, tie_gap


def decode_selected_reference(reg, idx, base, grid, image_hw, K: int):
    """reg [N][h][w][4 A] (any float dtype) -> (boxes [N][k][4] fp64, labels [N][k]) of idx: BoxCoder(weights (1, 1, 1, 1))
    on the whole level in fp64, gathered at idx // K; a zero box and label -1 where idx < 0."""
    reg = np.asarray(reg)
    N, h, w, c = reg.shape
    level = bc.decode_reference(reg.reshape(N * h * w, c), base, image_hw, c // 4, grid=grid)
    boxes = np.zeros(idx.shape + (4,), dtype=np.float64)
    labels = np.full(idx.shape, -1, dtype=np.int32)
    for i in range(N):
        live = idx[i] >= 0
        boxes[i, live] = level[i, idx[i, live] // K]
        labels[i, live] = idx[i, live] % K
    return boxes, labels


def detections_reference(boxes, scores, labels, valid, nms_thresh: float, detections: int):
    """The tail of postprocess_detections on the levels' concatenated candidates, boxes [N][M][4], scores [N][M], labels
    [N][M] and valid [N][M] (rows that hold a candidate): batched_nms in descending score order with groups = label (greedy,
    fp64), the first `detections` kept.  Returns the padded (boxes [N][D][4], scores [N][D], labels [N][D] int64, count
    [N]) in the inputs' dtypes, order (per image the valid rows, best first), and the margins (iou, tie)."""
    boxes, scores, labels, valid = (np.asarray(t) for t in (boxes, scores, labels, valid))
    N, D = boxes.shape[0], detections
    ob, os_ = np.zeros((N, D, 4), dtype=boxes.dtype), np.zeros((N, D), dtype=scores.dtype)
    ol, count = np.full((N, D), -1, dtype=np.int64), np.zeros(N, dtype=np.int32)
    orders, iou_margin, tie_gap = [], bc.INF, bc.INF
    for i in range(N):
        rows = np.nonzero(valid[i])[0]
        order = rows[np.argsort(-scores[i, rows].astype(np.float64), kind="stable")]
        orders.append(order)
        if len(rows) > 1:
            tie_gap = min(tie_gap, float(np.diff(np.sort(scores[i, rows].astype(np.float64))).min()))
        r = bc.nms_reference(boxes[i, order], None, labels[i, order], nms_thresh, 0.0, max_out=D, exact_sides=True)
        keep = order[r.keep]
        c = len(keep)
        ob[i, :c], os_[i, :c], ol[i, :c], count[i] = boxes[i, keep], scores[i, keep], labels[i, keep], c
        iou_margin = min(iou_margin, r.iou_margin)
    return dict(boxes=ob, scores=os_, labels=ol, count=count, orders=orders, iou_margin=iou_margin, tie_gap=tie_gap)


def assert_margins(thresh_margin: float, tie_gaps, iou_margin: float) -> None:
    """tests/box_cases.py's margins: a score's distance from the threshold, no tie among candidates, the NMS's IoU."""
    assert thresh_margin >= bc.SCORE_MARGIN, thresh_margin
    assert min(tie_gaps) > 0, tie_gaps
    assert iou_margin >= bc.IOU_MARGIN, iou_margin


def logit_threshold_bounds(t: float, s: float):
    """(sigmoid(t), sigmoid(pred(t))) in fp64 for the fp32 number t: the defining property of the logit threshold is
    sigmoid(t) > s >= sigmoid(pred(t))."""
    t32 = np.float32(t)
    assert float(t32) == t, "t is not an fp32 number"
    below = np.nextafter(t32, np.float32(-np.inf))
    sig = lambda v: 1.0 / (1.0 + math.exp(-float(v)))
    return sig(t32), sig(below)
