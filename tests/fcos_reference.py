"""The fp64 reference of FCOS for tests/test_fcos_host.py and tests/test_gpu_fcos.py: a transcription of torchvision's
FCOSHead (FCOSClassificationHead / FCOSRegressionHead: four times Conv2d, GroupNorm(32, C), ReLU, then cls_logits, and
relu(bbox_reg) beside bbox_ctrness) and of FCOS.postprocess_detections, stage by stage, each stage usable on the device's
own input to it, and the seeded detector the GPU test runs: resnet18, 64 channels (GroupNorm(32, 64), two channels per
group), 5 classes, N = 2 at 64 x 96 (levels 8x12, 4x6, 2x3, 1x2, 1x1), 40 candidates per level, 10 detections.

postprocess_detections per image and level: scores = sqrt(sigmoid(logits) * sigmoid(centerness)).flatten(); keep =
scores > score_thresh; the topk_candidates best of those; location = index // K, label = index % K;
BoxLinearCoder(normalize_by_size=True).decode + clip.  The tail (concatenate, batched_nms by label, the first
detections_per_img) is RetinaNet's: retinanet_reference.detections_reference.  Every discrete stage reports the smallest
margin of the decisions it made, and the test asserts the margins of tests/box_cases.py on them."""
import numpy as np
import torch

import box_cases as bc
from retinanet_reference import assert_margins, detections_reference  # noqa: F401  (the shared tail and margins)

FCOS = dict(arch="resnet18", out_channels=64, classes=5, N=2, H=64, W=96, topk=40, detections=10, seed=21,
            score_thresh=0.2, nms_thresh=0.6, sizes=((8,), (16,), (32,), (64,), (128,)))
LEVELS = ("0", "1", "2", "p6", "p7")
LEVEL_HW = [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)]
CONVS, GROUPS, EPS = 4, 32, 1e-5


def head_state_dict(C: int, classes: int, seed: int = 0):
    """torchvision's FCOSHead keys below `head.`: He-scaled towers with GroupNorm weights around 1, a classification
    output whose scores straddle the 0.2 threshold (with a centerness near 0, score > 0.2 is logit > -2.44: the class
    biases spread around it, so a level of 5 or 10 scores leaves padding rows and a level of 480 fills its top-k of 40),
    box distances of both signs (the ReLU cuts the negative ones to 0)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    sd = {}
    for head in ("classification_head", "regression_head"):
        for i in range(CONVS):
            sd[f"{head}.conv.{3 * i}.weight"] = rn(C, C, 3, 3) * (2.0 / (9 * C)) ** 0.5
            sd[f"{head}.conv.{3 * i}.bias"] = rn(C) * 0.1
            sd[f"{head}.conv.{3 * i + 1}.weight"] = 1.0 + rn(C) * 0.2
            sd[f"{head}.conv.{3 * i + 1}.bias"] = rn(C) * 0.2
    for key, width, wscale, bscale, bias in (("classification_head.cls_logits", classes, 2.0, 1.5, -2.5),
                                             ("regression_head.bbox_reg", 4, 1.0, 0.3, 0.8),
                                             ("regression_head.bbox_ctrness", 1, 1.0, 0.2, 0.0)):
        sd[f"{key}.weight"] = rn(width, C, 3, 3) * (wscale / (9 * C)) ** 0.5
        sd[f"{key}.bias"] = rn(width) * bscale + bias
    return sd


def detector_state_dict(resnet_module):
    """The seeded torchvision-named state dict of FCOS: backbone.* and head.* (float32), and the backbone's parts."""
    import fpn_p6p7_reference as fr
    d = FCOS
    fpn_sd, body = fr.p6p7_random_state_dict(torch, resnet_module, d["arch"], d["out_channels"], seed=d["seed"])
    sd = {"backbone." + k: v for k, v in fpn_sd.items()}
    sd.update({"head." + k: v for k, v in head_state_dict(d["out_channels"], d["classes"], seed=d["seed"] + 5).items()})
    return sd, fpn_sd, body


def detector_input():
    d = FCOS
    return torch.rand(d["N"], 3, d["H"], d["W"], generator=torch.Generator().manual_seed(d["seed"] + 1)) - 0.5


def head_reference(sd, feats):
    """fp64 FCOSHead on NHWC level maps {"0", "1", "2", "p6", "p7"} -> per level (class logits [N][h][w][K], bbox_reg
    BEFORE its ReLU [N][h][w][4], centerness [N][h][w]); sd: keys below `head.` or with the prefix.  The head as one
    stage is for the host tests: on a 1 x 1 level a group is two values, and GroupNorm turns the fp32 rounding of the
    convolution in front of it into up to 1 / sqrt(eps) = 316 times as much, so the GPU test checks the head layer by
    layer, each fed the device's own input (conv_reference, norm_reference)."""
    F = torch.nn.functional
    w = {(k[len("head."):] if k.startswith("head.") else k): v.double() for k, v in sd.items() if not k.startswith("backbone.")}
    out = []
    for name in LEVELS:
        x = feats[name].double().permute(0, 3, 1, 2)
        towers = {}
        for head in ("classification_head", "regression_head"):
            t = x
            for i in range(CONVS):
                t = F.conv2d(t, w[f"{head}.conv.{3 * i}.weight"], w[f"{head}.conv.{3 * i}.bias"], padding=1)
                t = torch.relu(F.group_norm(t, GROUPS, w[f"{head}.conv.{3 * i + 1}.weight"], w[f"{head}.conv.{3 * i + 1}.bias"], EPS))
            towers[head] = t
        last = lambda head, key: F.conv2d(towers[head], w[f"{head}.{key}.weight"], w[f"{head}.{key}.bias"],
                                          padding=1).permute(0, 2, 3, 1)
        out.append((last("classification_head", "cls_logits"), last("regression_head", "bbox_reg"),
                    last("regression_head", "bbox_ctrness")[..., 0]))
    return out


def _head_weights(sd):
    return {(k[len("head."):] if k.startswith("head.") else k): v.double() for k, v in sd.items() if not k.startswith("backbone.")}


def conv_reference(sd, key: str, x):
    """fp64 3x3 convolution `key` (with its bias) of the head on an NHWC map -> NHWC."""
    w = _head_weights(sd)
    y = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w[f"{key}.weight"], w[f"{key}.bias"], padding=1)
    return y.permute(0, 2, 3, 1)


def norm_reference(sd, key: str, y):
    """fp64 GroupNorm(32, C) `key` of the head, then ReLU, on an NHWC map -> NHWC."""
    w = _head_weights(sd)
    z = torch.nn.functional.group_norm(y.double().permute(0, 3, 1, 2), GROUPS, w[f"{key}.weight"], w[f"{key}.bias"], EPS)
    return torch.relu(z).permute(0, 2, 3, 1)


def score_reference(logits, ctr):
    """sqrt(sigmoid(logits) * sigmoid(centerness)) in fp64: [N][h][w][K]."""
    sig = lambda v: 1.0 / (1.0 + np.exp(-np.asarray(v, dtype=np.float64)))
    return np.sqrt(sig(logits) * sig(ctr)[..., None])


def level_select_reference(scores, topk: int, score_thresh: float):
    """One level of postprocess_detections on scores [N][n] (the flat (HW, K) order): per image the indices of the
    min(topk, candidates) best among score > score_thresh, best first, ties to the lower index.  Returns (idx [N][k] int32
    padded with -1, count [N], thresh_margin: the smallest |score - score_thresh|, tie_gap: the smallest gap between two
    neighbours among the kept scores and the first one left out, 0 for a tie)."""
    scores = np.asarray(scores, dtype=np.float64)
    N, n = scores.shape
    k = min(topk, n)
    idx, count = np.full((N, k), -1, dtype=np.int32), np.zeros(N, dtype=np.int32)
    thresh_margin, tie_gap = float(np.abs(scores - score_thresh).min()), bc.INF
    for i in range(N):
        cand = np.nonzero(scores[i] > score_thresh)[0]
        order = cand[np.argsort(-scores[i, cand], kind="stable")]
        c = min(k, len(order))
        idx[i, :c], count[i] = order[:c], c
        if len(order) > 1:
            tie_gap = min(tie_gap, float(np.abs(np.diff(scores[i, order[:k + 1]])).min()))
    return idx, count, thresh_margin, tie_gap


def decode_selected_reference(reg, idx, base, grid, image_hw, K: int):
    """reg [N][h][w][4] before its ReLU (any float dtype) -> (boxes [N][k][4] fp64, labels [N][k]) of idx:
    BoxLinearCoder(normalize_by_size=True).decode on relu(reg) at location idx // K of the level, clipped to the image, in
    fp64; a zero box and label -1 where idx < 0."""
    reg = np.maximum(np.asarray(reg, dtype=np.float64), 0.0)
    N, h, w, _ = reg.shape
    gh, gw, sy, sx = grid
    x1, y1, x2, y2 = (float(v) for v in np.asarray(base, dtype=np.float64).reshape(4))
    boxes = np.zeros(idx.shape + (4,), dtype=np.float64)
    labels = np.full(idx.shape, -1, dtype=np.int32)
    for i in range(N):
        H, W = (float(v) for v in image_hw[i])
        for j, id_ in enumerate(idx[i]):
            if id_ < 0:
                continue
            loc, labels[i, j] = divmod(int(id_), K)
            y, x = divmod(loc, w)
            ax1, ay1, ax2, ay2 = x1 + x * sx, y1 + y * sy, x2 + x * sx, y2 + y * sy
            cx, cy, aw, ah = 0.5 * (ax1 + ax2), 0.5 * (ay1 + ay2), ax2 - ax1, ay2 - ay1
            l, t, r, b = reg[i, y, x]
            box = (cx - l * aw, cy - t * ah, cx + r * aw, cy + b * ah)
            boxes[i, j] = [min(max(box[0], 0.0), W), min(max(box[1], 0.0), H), min(max(box[2], 0.0), W), min(max(box[3], 0.0), H)]
    return boxes, labels


def torch_head(C: int, classes: int):
    """torchvision's FCOSHead as a torch.nn module tree with its key names (torchvision itself is not a dependency): for
    load_state_dict(strict=True) of head_state_dict's keys."""
    nn = torch.nn

    def tower():
        layers = []
        for _ in range(CONVS):
            layers += [nn.Conv2d(C, C, 3, padding=1), nn.GroupNorm(GROUPS, C), nn.ReLU()]
        return nn.Sequential(*layers)

    class Cls(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv, self.cls_logits = tower(), nn.Conv2d(C, classes, 3, padding=1)

        def forward(self, x):
            return self.cls_logits(self.conv(x))

    class Reg(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv, self.bbox_reg, self.bbox_ctrness = tower(), nn.Conv2d(C, 4, 3, padding=1), nn.Conv2d(C, 1, 3, padding=1)

        def forward(self, x):
            t = self.conv(x)
            return self.bbox_reg(t), self.bbox_ctrness(t)

    class Head(nn.Module):
        def __init__(self):
            super().__init__()
            self.classification_head, self.regression_head = Cls(), Reg()

        def forward(self, x):
            return (self.classification_head(x), *self.regression_head(x))

    return Head()
