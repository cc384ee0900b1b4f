"""torchvision's Faster / Mask / Keypoint R-CNN on the library's kernels.  The second stage: what follows ``MultiScaleRoIAlign``
(``multiscale_roi_align``, the one new kernel) runs on layers the library already has.

``BoxHead.from_state_dict(sd)`` is ``TwoMLPHead`` + ``FastRCNNPredictor`` under the key names they have below
torchvision's ``roi_heads.``: ``box_head.fc6|fc7.weight|bias``, ``box_predictor.cls_score|bbox_pred.weight|bias``.
``head(pooled)`` takes the unpadded RoIAlign output ``[R][P][P][C]`` and returns ``(class_logits [R][classes],
box_regression [R][4*classes])``: three ``conv1x1_bn`` launches with scale = ones, the first two with ReLU.  ``fc6`` is
permuted at load from torchvision's ``(c, y, x)`` column order to ``(y, x, c)``, so the NHWC pooled tensor is its A matrix
``[R][P*P*C]`` without a copy; ``cls_score`` and ``bbox_pred`` are one GEMM whose ``5*classes`` columns are zero-padded to
a multiple of 64, and the two results are views of its output.

``MaskHead.from_state_dict(sd)`` is ``MaskRCNNHeads`` (state-dict version 2, no norm layer) + ``MaskRCNNPredictor``:
``mask_head.{0..3}.0.weight|bias`` (four 3x3 convolutions), ``mask_predictor.conv5_mask.weight|bias`` (the
``ConvTranspose2d(C, C, 2, 2)``) and ``mask_predictor.mask_fcn_logits.weight|bias`` (the 1x1 to the classes).
``head(pooled_padded)`` takes the padded RoIAlign output ``[R][P+2][P+2][C]`` (P even, zero ring) and returns the mask
logits ``[R][classes][2P][2P]``: four ``conv3x3_bn_relu`` launches at N = R on two ping-pong tensors, then two GEMMs.

The transposed convolution needs no depth-to-space kernel.  With stride = kernel = 2 no two input pixels meet in an
output pixel: ``out[co][2y+dy][2x+dx] = b[co] + sum_ci in[ci][y][x] w[ci][co][dy][dx]``.  That is the 1x1 GEMM of the
pixels ``[R*P*P][C]`` with ``B = w.permute(0, 2, 3, 1).reshape(C, 4C)`` (columns ordered ``(dy, dx, co)``) and the bias
tiled four times.  Its output ``[R*P*P][4C]`` is the same memory as ``[R*P*P*4][C]`` with the rows ordered
``(r, y, x, dy, dx)``: one row per OUTPUT pixel, all C channels contiguous.  The per-pixel 1x1 that follows does not care
in which order the pixels come, so that view is its A matrix as it stands; the order is undone once, on the small
``classes``-channel result, by a view + permute + copy in torch: ``[R][P][P][2][2][classes] -> [R][classes][P][2][P][2]``.

The first stage and the detector.  ``RPN.from_state_dict(sd)`` takes the keys below torchvision's ``rpn.``
(``head.conv.0.0.weight|bias``, or the legacy ``head.conv.weight|bias``; ``head.cls_logits`` [A][C][1][1]; ``head.bbox_pred``
[4A][C][1][1]), packs the two 1x1s like ``pack_predictor`` into one GEMM of 5A columns padded to 64 (objectness 0..A, deltas
A..5A) and runs per level ``conv3x3_bn_relu`` -> ``conv1x1_bn_ex(A_PADDED)`` -> ``box_decode`` in grid mode (base anchors
computed on the host in float32 as AnchorGenerator does; strides image // grid; "pool" copied once into a zero-ring
tensor), then ``filter_proposals`` with torch as plumbing: per-level ``topk`` on the logits, ``gather``, one stable
descending ``sort`` per image on the logit (the order of the probabilities wherever they differ, ties to the lower
index), ``sigmoid``, and ``batched_nms`` with groups = level.  ``select="kernel"`` (``RPN``, ``postprocess_detections``,
``FasterRCNN`` / ``MaskRCNN.from_state_dict``; the default ``"torch"`` is the code above, bit for bit) hands the
selecting and ordering to ``select_topk``: one call over the five levels (top k per level, logits and boxes gathered
into ``filter_proposals``' slots), one over the gathered logits (the stable sort, boxes written in order), and one in
``postprocess_detections`` (the candidates and their boxes).  Equal scores then go to the lower index everywhere, which
torch's ``topk`` does not promise; at most 8192 rows per call.  ``postprocess_detections`` is softmax, ``box_decode`` in
boxes mode straight on the box head's GEMM output, class 0 dropped, padding rows' scores 0, per image the ``topk`` of at
most ``max_candidates`` (default min(all, 8192)), ``batched_nms`` with groups = label and score_thresh =
nextafter(0.05) (torchvision's strict >).  Named deviation: the result is torchvision's whenever at most
``max_candidates`` scores of an image pass the threshold; ``overflow`` [N] says when more did.
``FasterRCNN.from_state_dict(sd, arch)`` (``backbone.body.*``, ``backbone.fpn.*``, ``rpn.*``, ``roi_heads.box_head.*``,
``roi_heads.box_predictor.*``) composes ResNetFPN(padded) -> RPN -> multiscale_roi_align -> BoxHead -> postprocess; after
``prepare(N, H, W)`` a forward reads no device data on the host and is captured into one graph.

``MaskRCNN.from_state_dict(sd, arch)`` adds ``roi_heads.mask_head.*`` / ``roi_heads.mask_predictor.*`` (split off before
``BoxHead``'s validator, which rejects keys it does not know).  ``postprocess_detections(rois_out=...)`` lets
``batched_nms`` write the detections as RoIAlign rows, ``(n, box)`` then ``(-1, 0, 0, 0, 0)``; on them run
``multiscale_roi_align(P = mask_P, in_padded, out_padded)`` -> ``MaskHead(raw=True)`` (the logits GEMM's output, no
permute copy) -> ``paste_masks(layout="gemm_rows")``: torchvision's ``maskrcnn_inference`` + ``paste_masks_in_image`` in
one launch, ``"masks"`` [N][D][H][W] float32 and / or ``"masks_binary"`` uint8, planes past ``count`` zero (label -1).
Like the rest, a forward after ``prepare`` reads no device data on the host and is captured into one graph.

``predict(images)`` is torchvision's whole call: a list of ``[3][h][w]`` images of different sizes (all float32 in
[0, 1] or all uint8) in, detections in each image's own pixels out.  ``prepare_images(shapes, ...)`` computes the resized
sizes (``transform_size``: torchvision's rule bit for bit) and the batch size, runs ``prepare`` and allocates the batch,
the resized sizes and the box ratios; ``predict`` then runs ``image_transform`` (one launch: normalise, resize, batch) ->
the detector -> ``torch.mul(boxes, ratio)`` (torchvision's ``resize_boxes``, ratio = fp32(original) / fp32(resized)), and
Mask R-CNN pastes its masks once, at original size: ``paste_masks`` with the rescaled boxes and ``image_hw`` = the original
sizes into ``[N][D][Hmax][Wmax]`` planes, zero beyond each image's own size (``to_image_lists`` crops them).  The mask
RoIAlign reads the un-rescaled detections, as in torchvision.  After ``prepare_images`` a ``predict`` reads no device data
on the host and is captured into one graph.  ``forward`` on a ready batch is unchanged.

``KeypointRCNN.from_state_dict(sd, arch)`` adds ``roi_heads.keypoint_head.{0,2,..,14}.weight|bias`` (eight 3x3
convolutions, the widths read off the state dict) and ``roi_heads.keypoint_predictor.kps_score_lowres.weight|bias`` (the
``ConvTranspose2d(C, K, 4, 2, 1)``), split off like the mask branch's keys.  On the detections' RoIAlign rows run
``multiscale_roi_align(P = keypoint_P, in_padded, out_padded)`` -> ``KeypointHead(raw=True)``: eight ``conv3x3_bn_relu``
launches at N = R and one GEMM with ``pack_kps_deconv``'s ``B [C][16K -> 64]`` (columns ``(ky, kx, k)``), which leaves
the transposed convolution's partial products, one row per input pixel.  With stride 2 and kernel 4 up to four of them
meet in an output pixel, so there is no view that undoes it; ``heatmaps_to_keypoints(layout="deconv_rows")`` gathers them
in LDS, adds the bias, upsamples x2 and then does torchvision's ``heatmaps_to_keypoints`` -- there a Python loop with a
host read and a ``[K][h][w]`` bicubic resize per detection -- in one launch: ``"keypoints"`` [N][D][K][3] = (x, y, 1) and
``"keypoints_scores"`` [N][D][K], rows past ``count`` zero.  ``predict`` computes them on the un-rescaled detections and
multiplies by ``(rw, rh, 1)`` (``resize_keypoints``).  ``KeypointHead(raw=False)`` composes torchvision's logits
[R][K][4P][4P] in torch (``fold``, bias, ``interpolate``) for callers who want them.

How a branch plugs in.  ``FasterRCNN`` holds the only ``prepare`` / ``forward`` / ``predict`` / ``to_lists``; a detector
differs by ``self.branches`` (``MaskBranch``, ``KeypointBranch``; none for Faster R-CNN), and all a detector keeps for
them is ``_det_rois`` [N][D][5], the detections as RoIAlign rows, allocated and handed to ``postprocess_detections`` only
when there is a branch.  A branch owns its head, P, RoIAlign output and output tensors and has five hooks:
``check(H, W)`` raises before anything is allocated; ``prepare(N, D, H, W, for_predict)`` allocates and prepares the head
at R = N * D; ``run(out, feats, det_rois, (H, W), stages)`` is everything that reads the un-rescaled detections;
``finish(out, image_hw, (H, W), tf)`` runs once the boxes are final (``tf`` is ``prepare_images``' dict in ``predict``,
None in ``forward``); ``predict_outputs(tf, Hmax, Wmax)`` adds the branch's entries to that dict.  One pass is
``_detect`` -> every ``run`` in list order -> ``predict``'s boxes x ratio -> every ``finish`` in list order, and ``_shape``
is set when the last branch has prepared.  ``to_lists`` slices whichever output keys the dict holds.  Both heads' 3x3
chains are ``_ConvTower``: the filter packing, the ``pooled_padded`` checks, the zero-ring buffers and the launch loop.

How a dense detector plugs in.  ``RetinaNet`` and ``FCOS`` (``from_state_dict(sd, arch)``: ``backbone.*`` with
``fpn.extra_blocks.p6|p7``, ``head.*``) are the one-stage detectors on the same plumbing (``_Detector``: ``prepare`` /
``forward`` / ``predict`` / ``prepare_images`` / ``to_lists`` are shared with ``FasterRCNN``).  ``_DenseDetector`` holds
their only ``_prepare`` and ``_detect``: ResNetFPN(returned_layers = (2, 3, 4), "p6p7") -> the head -> per level
``select_topk_map`` on the class map in place and the decode of the selected rows -> one ``select_topk`` by score with
the boxes as payload -> the label gather -> ``batched_nms`` by label -> the padded result and the ``stages`` dict; and
``_load_parts``, what the two ``from_state_dict`` share: the argument checks, the state-dict split, the class-count check
and the backbone and head.  ``_DenseHead`` holds the heads' only ``prepare`` and ``forward``: per level the ping-pong
pair, the two output maps and the level x tower loop, with ``groupnorm_relu`` in place after each tower convolution where
the tower has norms.  A head gives its name for messages, ``cols`` / ``ld_cls`` / ``ld_reg`` and a ``_pack`` that lists each
tower's keys.  A model gives its name, head class and validator, its threshold function (``logit_threshold`` /
``score_threshold``), its base anchors, the stage key of the selected values (``level_logits`` / ``level_scores``),
``ctr_col`` (FCOS: ``fcos_score_map`` runs on the class map before the select), ``_decode`` (``retina_decode`` /
``fcos_decode``) and ``_scores`` (the selected values to candidate scores: the sigmoid where a row is kept, or the values
themselves).  See the two classes' docstrings for the named deviations.

Not built: torchvision's ``fixed_size`` / ``_skip_resize`` options, training targets and the v2 heads.

The key names above are written from memory of torchvision's source and have not been checked against an installed
torchvision; the tests build their own state dicts under these names.
"""
from __future__ import annotations

import torch

from . import A_PADDED, IMAGENET_MEAN, IMAGENET_STD, IMAGE_DTYPES, RELU, WinoError, conv1x1_bn, conv1x1_bn_ex
from . import conv1x1_prepare, conv3x3_bn_relu, conv3x3_prepare
from . import filter_transform_f2
from ._net import Net, check_state_dict

MASK_CONVS = 4


def _pad64(n: int) -> int:
    return (int(n) + 63) // 64 * 64


# ---- pure packing functions (any device, any float dtype) -----------------------------------------------------------------
def pack_fc6(w: torch.Tensor, C: int, P: int) -> torch.Tensor:
    """fc6.weight [rep][C*P*P], columns in torchvision's flatten order (c, y, x) -> B [P*P*C][rep], rows ordered (y, x, c):
    the NHWC pooled tensor [R][P][P][C] viewed as [R][P*P*C] is then the GEMM's A."""
    rep = int(w.shape[0])
    return w.reshape(rep, C, P, P).permute(2, 3, 1, 0).reshape(P * P * C, rep).contiguous()


def pack_predictor(cls_w, cls_b, box_w, box_b):
    """cls_score [classes][rep] and bbox_pred [4*classes][rep] -> (B [rep][kp], bias [kp]) of one GEMM: columns 0..classes
    are the class logits, classes..5*classes the box regression, the rest (kp = 5*classes up to a multiple of 64) zero."""
    classes, rep = int(cls_w.shape[0]), int(cls_w.shape[1])
    kp = _pad64(5 * classes)
    B = cls_w.new_zeros((rep, kp))
    B[:, :classes] = cls_w.t()
    B[:, classes:5 * classes] = box_w.t()
    bias = cls_b.new_zeros(kp)
    bias[:classes] = cls_b
    bias[classes:5 * classes] = box_b
    return B, bias


def pack_deconv(w: torch.Tensor, b: torch.Tensor):
    """ConvTranspose2d(C, Co, 2, 2) weight [C][Co][2][2] and bias [Co] -> (B [C][4*Co] with columns (dy, dx, co), the bias
    tiled four times): the transposed convolution as a 1x1 GEMM, see the module docstring."""
    C, Co = int(w.shape[0]), int(w.shape[1])
    return w.permute(0, 2, 3, 1).reshape(C, 4 * Co).contiguous(), b.repeat(4)


def pack_logits(w: torch.Tensor, b: torch.Tensor):
    """mask_fcn_logits weight [classes][C][1][1] and bias -> (B [C][kp], bias [kp]), kp = classes up to a multiple of 64."""
    classes, C = int(w.shape[0]), int(w.shape[1])
    kp = _pad64(classes)
    B = w.new_zeros((C, kp))
    B[:, :classes] = w.reshape(classes, C).t()
    bias = b.new_zeros(kp)
    bias[:classes] = b
    return B, bias


# ---- state dicts ---------------------------------------------------------------------------------------------------------
def expected_box_head_keys(in_channels: int, P: int, rep: int, classes: int):
    """{key: shape} of TwoMLPHead(in_channels*P*P, rep) + FastRCNNPredictor(rep, classes)."""
    return {"box_head.fc6.weight": (rep, in_channels * P * P), "box_head.fc6.bias": (rep,),
            "box_head.fc7.weight": (rep, rep), "box_head.fc7.bias": (rep,),
            "box_predictor.cls_score.weight": (classes, rep), "box_predictor.cls_score.bias": (classes,),
            "box_predictor.bbox_pred.weight": (4 * classes, rep), "box_predictor.bbox_pred.bias": (4 * classes,)}


def _dim0(sd, key: str) -> int:
    if key not in sd:
        raise WinoError(f"state dict: missing key {key!r}")
    return int(sd[key].shape[0])


def validate_box_head_state_dict(sd, in_channels: int = 256, P: int = 7):
    """Checks every key and shape on the host; rep and classes are read off fc6 and cls_score.  Returns (rep, classes).
    Raises WinoError naming the first missing, unexpected or wrongly shaped key, or the figure a kernel cannot take."""
    in_channels, P = int(in_channels), int(P)
    rep = _dim0(sd, "box_head.fc6.weight")
    classes = _dim0(sd, "box_predictor.cls_score.weight")
    check_state_dict(sd, expected_box_head_keys(in_channels, P, rep, classes), "the box head", "weight")
    if rep < 64 or rep % 64:
        raise WinoError(f"box head: representation size rep={rep} must be a multiple of 64")
    if (in_channels * P * P) % 32:
        raise WinoError(f"box head: in_channels*P*P={in_channels * P * P} (in_channels={in_channels}, P={P}) must be a "
                        "multiple of 32")
    return rep, classes


def expected_mask_head_keys(in_channels: int, classes: int):
    """{key: shape} of MaskRCNNHeads(C, (C, C, C, C), 1) without a norm layer + MaskRCNNPredictor(C, C, classes)."""
    C = in_channels
    exp = {}
    for i in range(MASK_CONVS):
        exp[f"mask_head.{i}.0.weight"] = (C, C, 3, 3)
        exp[f"mask_head.{i}.0.bias"] = (C,)
    exp["mask_predictor.conv5_mask.weight"] = (C, C, 2, 2)
    exp["mask_predictor.conv5_mask.bias"] = (C,)
    exp["mask_predictor.mask_fcn_logits.weight"] = (classes, C, 1, 1)
    exp["mask_predictor.mask_fcn_logits.bias"] = (classes,)
    return exp


def validate_mask_head_state_dict(sd, in_channels: int = 256) -> int:
    """Checks every key and shape on the host; the class count is read off mask_fcn_logits.  Returns it."""
    in_channels = int(in_channels)
    classes = _dim0(sd, "mask_predictor.mask_fcn_logits.weight")
    check_state_dict(sd, expected_mask_head_keys(in_channels, classes), "the mask head", "weight")
    if in_channels < 64 or in_channels % 64:
        raise WinoError(f"mask head: in_channels={in_channels} must be a multiple of 64")
    return classes


# ---- the heads -------------------------------------------------------------------------------------------------------------
class BoxHead(Net):
    """TwoMLPHead + FastRCNNPredictor on the 1x1 GEMM kernel, inference only."""

    def __init__(self, in_channels: int, P: int, rep: int, classes: int, device):
        super().__init__(device)
        self.in_channels, self.P, self.rep, self.classes = int(in_channels), int(P), int(rep), int(classes)

    @classmethod
    def from_state_dict(cls, sd, in_channels: int = 256, P: int = 7, device=None) -> "BoxHead":
        rep, classes = validate_box_head_state_dict(sd, in_channels, P)
        return cls._load(sd, None, device, in_channels, P, rep, classes)

    def _pack(self, sd, eps):
        self.w6 = self._t(pack_fc6(sd["box_head.fc6.weight"], self.in_channels, self.P))
        self.b6 = self._t(sd["box_head.fc6.bias"])
        self.w7 = self._t(sd["box_head.fc7.weight"].t())
        self.b7 = self._t(sd["box_head.fc7.bias"])
        wp, bp = pack_predictor(sd["box_predictor.cls_score.weight"], sd["box_predictor.cls_score.bias"],
                                sd["box_predictor.bbox_pred.weight"], sd["box_predictor.bbox_pred.bias"])
        self.wp, self.bp = self._t(wp), self._t(bp)
        self._ones = torch.ones(max(self.rep, int(self.wp.shape[1])), dtype=torch.float32, device=self.device)
        torch.cuda.current_stream().synchronize()

    def prepare(self, R: int) -> None:
        """Allocate the three activations for R boxes and reserve the stream scratch of the three launches on the current
        stream.  Call it before capturing a forward into a graph."""
        R, kp, f32 = int(R), int(self.wp.shape[1]), torch.float32
        if R < 1:
            raise WinoError(f"box head: R={R} boxes")
        with torch.cuda.device(self.device):
            self._h6 = torch.empty((R, self.rep), dtype=f32, device=self.device)
            self._h7 = torch.empty((R, self.rep), dtype=f32, device=self.device)
            self._scores = torch.empty((R, kp), dtype=f32, device=self.device)
            conv1x1_prepare(R, self.in_channels * self.P * self.P, self.rep)
            conv1x1_prepare(R, self.rep, self.rep)
            conv1x1_prepare(R, self.rep, kp)
        self._shape = R

    def forward(self, pooled: torch.Tensor):
        """pooled [R][P][P][C] float32 (roi_align's unpadded output) -> (class_logits [R][classes], box_regression
        [R][4*classes]): views of one tensor of the head's, valid until the next forward.  A new R re-runs prepare()."""
        want = (self.P, self.P, self.in_channels)
        if not isinstance(pooled, torch.Tensor) or pooled.dim() != 4 or tuple(pooled.shape[1:]) != want:
            raise WinoError(f"pooled must be [R]{list(want)}")
        if pooled.device != self.device or pooled.dtype != torch.float32 or not pooled.is_contiguous():
            raise WinoError(f"pooled must be contiguous float32 on {self.device}")
        R = int(pooled.shape[0])
        if R != self._shape:
            self.prepare(R)
        kp, ones = int(self.wp.shape[1]), self._ones
        with torch.cuda.device(self.device):
            conv1x1_bn(pooled.view(R, -1), self.w6, self.b6, ones[: self.rep], True, out=self._h6)
            conv1x1_bn(self._h6, self.w7, self.b7, ones[: self.rep], True, out=self._h7)
            conv1x1_bn(self._h7, self.wp, self.bp, ones[:kp], False, out=self._scores)
        return self._scores[:, : self.classes], self._scores[:, self.classes: 5 * self.classes]


class _ConvTower(Net):
    """What MaskHead and KeypointHead share: a chain of conv3x3_bn_relu layers at N = R on the padded RoIAlign output.  A
    subclass gives `in_channels`, `widths` (one per layer) and `_ones` (at least max(widths) long)."""

    def _pack_tower(self, sd, stems) -> None:
        """convs = [(the F(2x2) filter transform, the bias)] of the layers at sd[stem.weight|bias]."""
        self.convs = [(filter_transform_f2(self._t(sd[f"{s}.weight"])), self._t(sd[f"{s}.bias"])) for s in stems]

    def _alloc_tower(self, R: int, P: int) -> None:
        """The layers' outputs [R][P+2][P+2][width] with zero rings.  Layer i writes buffer (its width, i mod 2): equal
        widths ping-pong on two tensors."""
        bufs, self._acts = {}, []
        for i, w in enumerate(self.widths):
            if (w, i % 2) not in bufs:
                bufs[(w, i % 2)] = torch.zeros((R, P + 2, P + 2, w), dtype=torch.float32, device=self.device)
            self._acts.append(bufs[(w, i % 2)])

    def _reserve_tower(self, R: int, P: int) -> None:
        """The stream scratch of the launches; a head calls it after all its allocations, as it always has."""
        for c, w in zip([self.in_channels] + self.widths, self.widths):
            conv3x3_prepare(R, c, w, P, P)

    def _begin_tower(self, x):
        """forward's opening: x is [R][P+2][P+2][in_channels] float32 on the head's device; a new (R, P) re-runs
        prepare().  Returns (R, P)."""
        C = self.in_channels
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or int(x.shape[3]) != C or x.shape[1] != x.shape[2]:
            raise WinoError(f"pooled_padded must be [R][P+2][P+2][{C}]")
        if x.device != self.device or x.dtype != torch.float32 or not x.is_contiguous():
            raise WinoError(f"pooled_padded must be contiguous float32 on {self.device}")
        R, P = int(x.shape[0]), int(x.shape[1]) - 2
        if (R, P) != self._shape:
            self.prepare(R, P)
        return R, P

    def _run_tower(self, x):
        """The launches; returns the last layer's output (it is not x's memory: x is not written)."""
        for (U, bias), dst, w in zip(self.convs, self._acts, self.widths):
            conv3x3_bn_relu(x, U, bias, self._ones[:w], relu=True, out=dst)
            x = dst
        return x


class MaskHead(_ConvTower):
    """MaskRCNNHeads + MaskRCNNPredictor on the Winograd 3x3 and the 1x1 GEMM kernels, inference only."""
    _a = property(lambda self: self._acts[0])   # the two ping-pong tensors under the names they had
    _b = property(lambda self: self._acts[1])

    def __init__(self, in_channels: int, classes: int, device):
        super().__init__(device)
        self.in_channels, self.classes = int(in_channels), int(classes)
        self.widths = [self.in_channels] * MASK_CONVS

    @classmethod
    def from_state_dict(cls, sd, in_channels: int = 256, device=None) -> "MaskHead":
        classes = validate_mask_head_state_dict(sd, in_channels)
        return cls._load(sd, None, device, in_channels, classes)

    def _pack(self, sd, eps):
        self._pack_tower(sd, [f"mask_head.{i}.0" for i in range(MASK_CONVS)])
        wd, bd = pack_deconv(sd["mask_predictor.conv5_mask.weight"], sd["mask_predictor.conv5_mask.bias"])
        self.wd, self.bd = self._t(wd), self._t(bd)
        wl, bl = pack_logits(sd["mask_predictor.mask_fcn_logits.weight"], sd["mask_predictor.mask_fcn_logits.bias"])
        self.wl, self.bl = self._t(wl), self._t(bl)
        self._ones = torch.ones(max(4 * self.in_channels, int(self.wl.shape[1])), dtype=torch.float32, device=self.device)
        torch.cuda.current_stream().synchronize()

    def prepare(self, R: int, P: int = 14) -> None:
        """Allocate the two ping-pong tensors, the transposed convolution's output, the padded-class scores and the
        result for R boxes of P x P, and reserve the stream scratch of the six launches on the current stream.  Call it
        before capturing a forward into a graph."""
        R, P, C, kp, f32 = int(R), int(P), self.in_channels, int(self.wl.shape[1]), torch.float32
        if R < 1 or P < 2 or P % 2:
            raise WinoError(f"mask head: R={R} boxes of P={P}: need R >= 1 and an even P >= 2")
        with torch.cuda.device(self.device):
            self._alloc_tower(R, P)
            self._up = torch.empty((R * P * P, 4 * C), dtype=f32, device=self.device)
            self._scores = torch.empty((R * P * P * 4, kp), dtype=f32, device=self.device)
            self._masks = torch.empty((R, self.classes, 2 * P, 2 * P), dtype=f32, device=self.device)
            self._reserve_tower(R, P)
            conv1x1_prepare(R * P * P, C, 4 * C)
            conv1x1_prepare(R * P * P * 4, C, kp)
        self._shape = (R, P)

    def forward(self, pooled_padded: torch.Tensor, raw: bool = False):
        """pooled_padded [R][P+2][P+2][C] float32 with a zero ring (roi_align's out_padded output; it is not written) ->
        mask logits [R][classes][2P][2P], a tensor of the head's, valid until the next forward.  A new (R, P) re-runs
        prepare().  raw=True: returns (the logits GEMM's output [R*P*P*4][ld] with rows ordered (r, y, x, dy, dx) and the
        classes in its first columns, ld) and skips the permute copy: paste_masks' "gemm_rows" layout."""
        R, P = self._begin_tower(pooled_padded)
        C, kp, ones = self.in_channels, int(self.wl.shape[1]), self._ones
        with torch.cuda.device(self.device):
            top = self._run_tower(pooled_padded)
            conv1x1_bn_ex(top, self.wd, self.bd, ones[: 4 * C], A_PADDED | RELU, out=self._up, hw=(P, P))
            # rows (r, y, x) x columns (dy, dx, c) are rows (r, y, x, dy, dx) x columns c: the logits GEMM's A as it stands
            conv1x1_bn(self._up.view(R * P * P * 4, C), self.wl, self.bl, ones[:kp], False, out=self._scores)
            if raw:
                return self._scores, kp
            scores = self._scores.view(R, P, P, 2, 2, kp)[..., : self.classes]
            self._masks.view(R, self.classes, P, 2, P, 2).copy_(scores.permute(0, 5, 1, 3, 2, 4))
        return self._masks


# ---- the first stage ---------------------------------------------------------------------------------------------------
ANCHOR_SIZES = ((32,), (64,), (128,), (256,), (512,))
ANCHOR_RATIOS = (0.5, 1.0, 2.0)
RPN_LEVELS = ("0", "1", "2", "3", "pool")
BOX_WEIGHTS = (10.0, 10.0, 5.0, 5.0)
SCORE_THRESH_STRICT = 0.05000000447034836   # nextafter(float32(0.05), inf): torchvision keeps score > 0.05
SELECTS = ("torch", "kernel")
SELECT_MAX_ROWS = 8192   # what one select_topk part can keep


def _check_select(select) -> str:
    if select not in SELECTS:
        raise WinoError(f"select must be one of {SELECTS}, got {select!r}")
    return select


def base_anchors(sizes, ratios) -> torch.Tensor:
    """torchvision's AnchorGenerator.generate_anchors on the host in float32: h_r = sqrt(ratio), w_r = 1 / h_r,
    round([-w, -h, w, h] / 2), ratio-major: [len(ratios) * len(sizes)][4]."""
    scales = torch.as_tensor(sizes, dtype=torch.float32)
    ar = torch.as_tensor(ratios, dtype=torch.float32)
    h_r = torch.sqrt(ar)
    w_r = 1 / h_r
    ws = (w_r[:, None] * scales[None, :]).view(-1)
    hs = (h_r[:, None] * scales[None, :]).view(-1)
    return (torch.stack([-ws, -hs, ws, hs], dim=1) / 2).round()


def pack_rpn_head(cls_w, cls_b, box_w, box_b):
    """cls_logits [A][C][1][1] and bbox_pred [4A][C][1][1] -> (B [C][kp], bias [kp]) of one GEMM, like pack_predictor:
    objectness at columns 0..A, deltas at A..5A, the rest (kp = 5A up to a multiple of 64) zero."""
    A, C = int(cls_w.shape[0]), int(cls_w.shape[1])
    return pack_predictor(cls_w.reshape(A, C), cls_b, box_w.reshape(4 * A, C), box_b)


def expected_rpn_keys(sd, in_channels: int, A: int):
    """{key: shape} of torchvision's RPNHead below `rpn.`; the legacy spelling head.conv.weight|bias is accepted."""
    conv = "head.conv" if "head.conv.weight" in sd else "head.conv.0.0"
    C = in_channels
    return {f"{conv}.weight": (C, C, 3, 3), f"{conv}.bias": (C,), "head.cls_logits.weight": (A, C, 1, 1),
            "head.cls_logits.bias": (A,), "head.bbox_pred.weight": (4 * A, C, 1, 1), "head.bbox_pred.bias": (4 * A,)}


class RPN(Net):
    """torchvision's RegionProposalNetwork at test time: RPNHead (one Winograd 3x3 and one 1x1 GEMM per level),
    box_decode in grid mode per level, and filter_proposals with torch as plumbing (topk, gather, sigmoid, sort) around
    batched_nms.  No host read of device data after prepare()."""

    def __init__(self, in_channels, sizes, ratios, pre_nms_top_n, post_nms_top_n, nms_thresh, score_thresh, min_size, device,
                 select="torch"):
        super().__init__(device)
        self.select = _check_select(select)
        self.in_channels, self.sizes, self.ratios = int(in_channels), tuple(tuple(s) for s in sizes), tuple(ratios)
        self.A = len(self.sizes[0]) * len(self.ratios)
        self.pre, self.post = int(pre_nms_top_n), int(post_nms_top_n)
        self.nms_thresh, self.score_thresh, self.min_size = float(nms_thresh), float(score_thresh), float(min_size)

    @classmethod
    def from_state_dict(cls, sd, in_channels: int = 256, sizes=ANCHOR_SIZES, ratios=ANCHOR_RATIOS, pre_nms_top_n: int = 1000,
                        post_nms_top_n: int = 1000, nms_thresh: float = 0.7, score_thresh: float = 0.0,
                        min_size: float = 1e-3, device=None, select: str = "torch") -> "RPN":
        """sd: the keys below torchvision's `rpn.` (head.conv.0.0, head.cls_logits, head.bbox_pred).  select: "torch"
        (topk / sort / gather) or "kernel" (select_topk), see the module docstring."""
        _check_select(select)
        if len(sizes) != len(RPN_LEVELS) or len({len(s) for s in sizes}) != 1:
            raise WinoError(f"rpn: {len(RPN_LEVELS)} levels need {len(RPN_LEVELS)} size tuples of one length")
        A = len(sizes[0]) * len(ratios)
        check_state_dict(sd, expected_rpn_keys(sd, int(in_channels), A), "the RPN head", "weight")
        if in_channels < 64 or in_channels % 64:
            raise WinoError(f"rpn: in_channels={in_channels} must be a multiple of 64")
        if min(int(pre_nms_top_n), int(post_nms_top_n)) < 1:
            raise WinoError("rpn: pre_nms_top_n and post_nms_top_n must be at least 1")
        return cls._load(sd, None, device, in_channels, sizes, ratios, pre_nms_top_n, post_nms_top_n, nms_thresh,
                         score_thresh, min_size, select=select)

    def _pack(self, sd, eps):
        conv = "head.conv" if "head.conv.weight" in sd else "head.conv.0.0"
        self.U = filter_transform_f2(self._t(sd[f"{conv}.weight"]))
        self.bc = self._t(sd[f"{conv}.bias"])
        wp, bp = pack_rpn_head(sd["head.cls_logits.weight"], sd["head.cls_logits.bias"], sd["head.bbox_pred.weight"],
                               sd["head.bbox_pred.bias"])
        self.wp, self.bp = self._t(wp), self._t(bp)
        self.base = [self._t(base_anchors(s, self.ratios)) for s in self.sizes]
        self._ones = torch.ones(max(self.in_channels, int(self.wp.shape[1])), dtype=torch.float32, device=self.device)
        torch.cuda.current_stream().synchronize()

    def prepare(self, N: int, level_hw, image_size) -> None:
        """Allocate every tensor of the first stage for N images whose five levels are `level_hw` [(h, w)] and reserve
        the launches' stream scratch on the current stream.  Call it before capturing a forward into a graph."""
        from . import nms_workspace_bytes, select_workspace_bytes
        N, C, kp, dev, f32 = int(N), self.in_channels, int(self.wp.shape[1]), self.device, torch.float32
        level_hw = [(int(h), int(w)) for h, w in level_hw]
        H, W = int(image_size[0]), int(image_size[1])
        if len(level_hw) != len(RPN_LEVELS):
            raise WinoError(f"rpn: {len(RPN_LEVELS)} levels, got {len(level_hw)}")
        with torch.cuda.device(dev):
            self._t3 = [torch.zeros((N, h + 2, w + 2, C), dtype=f32, device=dev) for h, w in level_hw]
            self._head = [torch.empty((N * h * w, kp), dtype=f32, device=dev) for h, w in level_hw]
            ph, pw = level_hw[-1]
            self._pool = torch.zeros((N, ph + 2, pw + 2, C), dtype=f32, device=dev)
            self._n = [h * w * self.A for h, w in level_hw]
            self._k = [min(self.pre, n) for n in self._n]
            total, K = sum(self._n), sum(self._k)
            if self.select == "kernel" and K > SELECT_MAX_ROWS:
                raise WinoError(f"rpn: select=\"kernel\" sorts at most {SELECT_MAX_ROWS} proposals per image, the levels "
                                f"keep {K}")
            self._boxes = torch.empty((N, total, 4), dtype=f32, device=dev)
            self._logits = torch.empty((N, total), dtype=f32, device=dev)
            self._level_of = torch.cat([torch.full((k,), l, dtype=torch.int32) for l, k in enumerate(self._k)]).to(dev)
            self._keep = torch.empty((N, self.post), dtype=torch.int32, device=dev)
            self._count = torch.empty((N,), dtype=torch.int32, device=dev)
            self._rois = torch.empty((N, self.post, 5), dtype=f32, device=dev)
            self._ws = torch.empty((nms_workspace_bytes(N, K) + 3) // 4, dtype=f32, device=dev)
            if self.select == "kernel":
                i32 = torch.int32
                self._sel = dict(
                    idx=torch.empty((N, K), dtype=i32, device=dev), logit=torch.empty((N, K), dtype=f32, device=dev),
                    count=torch.empty((N, len(self._k)), dtype=i32, device=dev),
                    boxes=torch.empty((N, K, 4), dtype=f32, device=dev),
                    ws=torch.empty((select_workspace_bytes(N, self._n, self._k) + 3) // 4, dtype=f32, device=dev),
                    order=torch.empty((N, K), dtype=i32, device=dev), slogit=torch.empty((N, K), dtype=f32, device=dev),
                    count2=torch.empty((N, 1), dtype=i32, device=dev), sboxes=torch.empty((N, K, 4), dtype=f32, device=dev),
                    ws2=torch.empty((select_workspace_bytes(N, K, K) + 3) // 4, dtype=f32, device=dev))
            for h, w in level_hw:
                conv3x3_prepare(N, C, C, h, w)
                conv1x1_prepare(N * h * w, C, kp)
        self._grid = [(h, w, H // h, W // w) for h, w in level_hw]
        self._shape = (N, tuple(level_hw), (H, W))

    def forward(self, features, image_hw: torch.Tensor, image_size, stages=None):
        """features: ResNetFPN(...)(x, padded=True); image_hw [N][2] float32 on the device (the clip sizes); image_size
        (H, W) of the batch.  Returns (rois [N * post][5] with padding rows of index -1, scores [N][post], count [N]):
        tensors of the module's, valid until the next forward.  `stages`: a dict that receives every intermediate."""
        from . import batched_nms, box_decode, select_topk
        maps = [features[k] for k in RPN_LEVELS]
        N, C, kp, A = int(maps[0].shape[0]), self.in_channels, int(self.wp.shape[1]), self.A
        level_hw = tuple((int(m.shape[1]) - 2, int(m.shape[2]) - 2) for m in maps[:-1]) + \
            ((int(maps[-1].shape[1]), int(maps[-1].shape[2])),)
        shape = (N, level_hw, (int(image_size[0]), int(image_size[1])))
        if shape != self._shape:
            self.prepare(N, level_hw, image_size)
        with torch.cuda.device(self.device):
            self._pool[:, 1:-1, 1:-1, :].copy_(maps[-1])   # "pool" is a strided view: once into a zero-ring tensor
            maps[-1] = self._pool
            off = 0
            for l, x in enumerate(maps):
                conv3x3_bn_relu(x, self.U, self.bc, self._ones[:C], relu=True, out=self._t3[l])
                conv1x1_bn_ex(self._t3[l], self.wp, self.bp, self._ones[:kp], A_PADDED, out=self._head[l])
                box_decode(self._head[l], self.base[l], image_hw, A, grid=self._grid[l], delta_col=A, score_col=0,
                           out_boxes=self._boxes, out_scores=self._logits, out_offset=off)
                off += self._n[l]
            if self.select == "kernel":
                # filter_proposals on select_topk: the levels' top k into the cat's slots, then the stable sort
                b, offs = self._sel, [sum(self._n[:l]) for l in range(len(self._n))]
                idx32, logit, _, lboxes = select_topk(self._logits, self._k, self._n, offs, boxes=self._boxes,
                                                      out_idx=b["idx"], out_vals=b["logit"], out_count=b["count"],
                                                      out_boxes=b["boxes"], workspace=b["ws"])
                order32, slogit, _, sboxes = select_topk(logit, sum(self._k), boxes=lboxes, out_idx=b["order"],
                                                         out_vals=b["slogit"], out_count=b["count2"],
                                                         out_boxes=b["sboxes"], workspace=b["ws2"])
                idx, order = idx32.long(), order32.long()
            else:
                # filter_proposals: torch as plumbing
                idx, off = [], 0
                for n, k in zip(self._n, self._k):
                    idx.append(self._logits[:, off:off + n].topk(k, dim=1, sorted=True).indices + off)
                    off += n
                idx = torch.cat(idx, dim=1)
                logit = self._logits.gather(1, idx)
                slogit, order = torch.sort(logit, dim=1, descending=True, stable=True)   # (by logit: the order of the probabilities)
                sidx = idx.gather(1, order)
                sboxes = self._boxes.gather(1, sidx[:, :, None].expand(-1, -1, 4)).contiguous()
            slevel = self._level_of[order].contiguous()
            prob = torch.sigmoid(slogit)
            batched_nms(sboxes, prob, slevel, self.nms_thresh, self.min_size, self.score_thresh, self.post, self._rois,
                        self._ws, self._keep, self._count)
            kept = self._keep >= 0
            scores = torch.where(kept, prob.gather(1, self._keep.clamp(min=0).long()), torch.zeros_like(prob[:, :1]))
        if stages is not None:
            stages.update(rpn_head=list(self._head), rpn_boxes=self._boxes, rpn_logits=self._logits, topk_idx=idx,
                          sorted_boxes=sboxes, sorted_logits=slogit, sorted_scores=prob, sorted_levels=slevel,
                          rpn_keep=self._keep, rpn_count=self._count, rois=self._rois, proposal_scores=scores)
        return self._rois.view(N * self.post, 5), scores, self._count


def postprocess_detections(head_out: torch.Tensor, rois: torch.Tensor, image_hw: torch.Tensor, classes: int,
                           score_thresh: float = SCORE_THRESH_STRICT, nms_thresh: float = 0.5, detections: int = 100,
                           min_size: float = 1e-2, max_candidates=None, stages=None, rois_out=None, select: str = "torch"):
    """torchvision's RoIHeads.postprocess_detections with fixed-size outputs and no host read.  head_out [R][kp]: BoxHead's
    one GEMM output (class logits at 0..classes, deltas at classes..5*classes), R = N * per rows; rois [R][5] with padding
    rows of index -1; image_hw [N][2].  softmax (torch), box_decode in boxes mode on head_out in place with weights
    (10, 10, 5, 5), class 0 dropped, padding rows' scores 0, per image the top max_candidates (default min(all, 8192))
    by score, batched_nms with groups = label.  score_thresh is >=: the default is nextafter(0.05), torchvision's strict >.
    Returns {"boxes" [N][D][4], "scores" [N][D], "labels" [N][D] int64 (-1 past count), "count" [N], "overflow" [N]}.
    Named deviation: the result equals torchvision's whenever at most max_candidates scores of an image pass the
    threshold; overflow[n] (computed on the device) says when more did.  rois_out: a tensor [N][D][5] that batched_nms
    fills with the detections as RoIAlign rows, (n, box) then (-1, 0, 0, 0, 0): the mask branch's input.
    select: "torch" (topk and gather) or "kernel" (one select_topk call; equal scores, the padding rows' zeros among
    them, then go to the lower index; max_candidates <= 8192)."""
    from . import batched_nms, box_decode, select_topk
    _check_select(select)
    N, R, classes = int(image_hw.shape[0]), int(rois.shape[0]), int(classes)
    if classes < 2 or R % N or head_out.dim() != 2 or int(head_out.shape[0]) != R or int(head_out.shape[1]) < 5 * classes:
        raise WinoError(f"postprocess_detections: head_out {tuple(head_out.shape)}, rois {tuple(rois.shape)}, N={N}, "
                        f"classes={classes}")
    per, fg = R // N, classes - 1
    M = per * fg
    kc = M if max_candidates is None else int(max_candidates)
    kc = max(1, min(kc, M, 8192 if max_candidates is None else M))
    if select == "kernel" and kc > SELECT_MAX_ROWS:
        raise WinoError(f"postprocess_detections: select=\"kernel\" keeps at most {SELECT_MAX_ROWS} candidates, "
                        f"max_candidates={kc}")
    prob = torch.softmax(head_out[:, :classes], dim=-1)
    boxes, _ = box_decode(head_out, rois[:, 1:5].contiguous(), image_hw, classes, BOX_WEIGHTS, None, classes)
    boxes = boxes.view(N, per, classes, 4)[:, :, 1:].reshape(N, M, 4)
    valid = (rois[:, 0] >= 0).view(N, per, 1)
    scores = (prob.view(N, per, classes)[:, :, 1:] * valid).reshape(N, M)
    if select == "kernel":
        cidx32, cscores, _, cboxes = select_topk(scores, kc, boxes=boxes)
        cidx = cidx32.long()
    else:
        top = scores.topk(kc, dim=1, sorted=True)
        cidx = top.indices
        cboxes = boxes.gather(1, cidx[:, :, None].expand(-1, -1, 4)).contiguous()
        cscores = top.values.contiguous()
    clabels = (cidx % fg + 1).to(torch.int32).contiguous()
    overflow = (scores >= score_thresh).sum(dim=1) > kc
    keep, count = batched_nms(cboxes, cscores, clabels, nms_thresh, min_size, score_thresh, int(detections),
                              rois_out=rois_out)[:2]
    kept = keep >= 0
    at = keep.clamp(min=0).long()
    out = {"boxes": cboxes.gather(1, at[:, :, None].expand(-1, -1, 4)) * kept[:, :, None],
           "scores": cscores.gather(1, at) * kept,
           "labels": torch.where(kept, clabels.gather(1, at).long(), torch.full_like(at, -1)),
           "count": count, "overflow": overflow}
    if stages is not None:
        stages.update(class_prob=prob, class_boxes=boxes, class_scores=scores, cand_idx=cidx, cand_boxes=cboxes,
                      cand_scores=cscores, cand_labels=clabels, det_keep=keep)
    return out


MASK_KEYS = ("masks", "masks_binary")
LIST_KEYS = ("boxes", "scores", "labels") + MASK_KEYS + ("keypoints", "keypoints_scores")   # what to_lists slices per image


class _Detector(Net):
    """What the detectors share: prepare, the one forward / predict path, prepare_images and the list views.  A subclass
    gives `_prepare(N, H, W, for_predict)` (which sets `_shape = (N, H, W)` last) and `_detect(x, image_sizes, st)` ->
    (the result dict, the pyramid, image_hw), and may fill `branches` (and then `_det_rois`)."""

    def __init__(self, device, detections: int):
        super().__init__(device)
        self.detections = int(detections)
        self.branches = []   # the RoI branches that run on the detections, in order: none for Faster R-CNN and RetinaNet
        self._det_rois = None
        self._tf, self._tf_params = None, None   # prepare_images' state, and the parameters of its last call

    def prepare(self, N: int, H: int, W: int) -> None:
        """Allocate everything for [N][3][H][W] inputs and reserve every launch's stream scratch on the current stream.
        After it a forward performs no host read of device data, so it can be captured into one graph."""
        self._prepare(N, H, W, for_predict=False)

    def _run(self, x, image_sizes, st, tf=None):
        """forward's and predict's one path: _detect, every branch on the un-rescaled detections, predict's boxes into
        each image's own pixels (`tf`: prepare_images' state, None in forward), then what the branches do once the boxes
        are final."""
        out, feats, hw = self._detect(x, image_sizes, st)
        size = self._shape[1:]
        with torch.cuda.device(self.device):
            for b in self.branches:
                b.run(out, feats, self._det_rois, size, st)
            if tf is not None:
                out["boxes"] = torch.mul(out["boxes"], tf["ratio"], out=tf["boxes"])
            for b in self.branches:
                b.finish(out, hw, size, tf)
        if tf is not None:
            out["original_sizes"] = list(tf["orig"])
        if st is not None:
            out.update(st)
        return out

    def forward(self, x: torch.Tensor, image_sizes=None, stages: bool = False):
        """x [N][3][H][W] float32, already normalised; image_sizes: None (every image fills the batch) or a float32
        device tensor [N][2] of (H_img, W_img).  Returns {"boxes" [N][D][4], "scores" [N][D], "labels" [N][D], "count" [N],
        "overflow" [N]}, rows past count zero with label -1, plus what each branch adds (tensors of the model's, valid
        until the next forward); with stages=True also every intermediate."""
        return self._run(x, image_sizes, {} if stages else None)

    def prepare_images(self, shapes, dtype=torch.float32, min_size: int = 800, max_size: int = 1333, mean=IMAGENET_MEAN,
                       std=IMAGENET_STD, size_divisible: int = 32) -> None:
        """Everything predict needs for a list of images of `shapes` [(h, w)] (or (3, h, w)) and `dtype` (float32 or
        uint8): the resized sizes (transform_size) and the batch size (batch_hw), prepare(N, Hb, Wb), the batch
        [N][3][Hb][Wb], the device image_hw [N][2] (the resized sizes: forward's image_sizes), the ratio tensor [N][1][4] =
        fp32(original) / fp32(resized) as (rw, rh, rw, rh) (torchvision's resize_boxes) and the rescaled boxes.  After it
        a predict on such a list performs no host read of device data, so it can be captured into one graph."""
        from . import batch_hw, transform_size
        if dtype not in IMAGE_DTYPES:
            raise WinoError(f"prepare_images: dtype must be torch.float32 or torch.uint8, got {dtype}")
        shapes = [tuple(s) for s in shapes]
        if not shapes or any(len(s) not in (2, 3) or (len(s) == 3 and int(s[0]) != 3) for s in shapes):
            raise WinoError("prepare_images: shapes must be a non-empty list of (h, w) or (3, h, w)")
        orig = [(int(s[-2]), int(s[-1])) for s in shapes]
        params = dict(min_size=int(min_size), max_size=int(max_size), mean=tuple(float(v) for v in mean),
                      std=tuple(float(v) for v in std), size_divisible=int(size_divisible))
        self._tf, self._tf_params = None, params   # (remembered for predict even if what follows raises)
        sizes = [transform_size(h, w, params["min_size"], params["max_size"]) for h, w in orig]
        Hb, Wb = batch_hw(sizes, params["size_divisible"])
        N, dev, f32 = len(orig), self.device, torch.float32
        self._prepare(N, Hb, Wb, for_predict=True)
        new, old = torch.tensor(orig, dtype=f32), torch.tensor(sizes, dtype=f32)
        ratio = (new / old)[:, [1, 0, 1, 0]].reshape(N, 1, 4)   # (a torch fp32 division of the two size tensors)
        with torch.cuda.device(dev):
            tf = dict(key=(tuple(orig), dtype), params=params, orig=orig, sizes=sizes, shape=(N, Hb, Wb),
                      batch=torch.empty((N, 3, Hb, Wb), dtype=f32, device=dev), image_hw=old.to(dev),
                      orig_hw=new.to(dev), ratio=ratio.contiguous().to(dev),
                      boxes=torch.empty((N, self.detections, 4), dtype=f32, device=dev))
            for b in self.branches:
                b.predict_outputs(tf, max(h for h, _ in orig), max(w for _, w in orig))
        torch.cuda.current_stream().synchronize()
        self._tf = tf

    def _ready(self, images):
        """predict's opening: the list checked, prepare_images re-run when its shapes or dtype are new (with the
        parameters of the last prepare_images, or the defaults)."""
        images = list(images)
        if not images or any(not isinstance(t, torch.Tensor) or t.dim() != 3 or int(t.shape[0]) != 3 for t in images):
            raise WinoError("images must be a non-empty list of [3][h][w] tensors")
        if any(t.device != self.device or t.dtype != images[0].dtype for t in images):
            raise WinoError(f"the images must be on {self.device} and of one dtype")
        key = (tuple((int(t.shape[1]), int(t.shape[2])) for t in images), images[0].dtype)
        if self._tf is None or self._tf["key"] != key or self._tf["shape"] != self._shape:
            self.prepare_images(key[0], key[1], **(self._tf_params or {}))
        return images, self._tf

    def _transform(self, images, tf):
        from . import image_transform
        p = tf["params"]
        with torch.cuda.device(self.device):
            return image_transform(images, tf["sizes"], tf["shape"][1], tf["shape"][2], p["mean"], p["std"], out=tf["batch"])

    def predict(self, images):
        """torchvision's detector call: images, a list of [3][h][w] tensors of different sizes (all float32 in [0, 1] or
        all uint8), through image_transform -> the detector -> the mapping back.  Returns forward's dict with "boxes"
        [N][D][4] in each image's own pixels (a tensor of the model's, valid until the next predict), what each branch
        adds, mapped back likewise, plus "original_sizes", the host list of (h, w).  A list of new shapes or dtype re-runs
        prepare_images."""
        images, tf = self._ready(images)
        return self._run(self._transform(images, tf), tf["image_hw"], None, tf)

    @staticmethod
    def to_lists(out):
        """torchvision's list of dicts per image: "boxes", "scores", "labels" and whichever of the branches' outputs `out`
        holds, "masks" / "masks_binary" [c][1][H][W], "keypoints" [c][K][3], "keypoints_scores" [c][K].  Synchronises (it
        reads count)."""
        keys = [k for k in LIST_KEYS if k in out]
        return [{k: (out[k][n, :c].unsqueeze(1) if k in MASK_KEYS else out[k][n, :c]).clone() for k in keys}
                for n, c in enumerate(out["count"].tolist())]

    @staticmethod
    def to_image_lists(out):
        """to_lists of a predict's result: boxes and keypoints are already in each image's own pixels, each image's
        masks are cropped to its own [h][w]."""
        res = _Detector.to_lists(out)
        for key in MASK_KEYS:
            if key in out:
                for d, (h, w) in zip(res, out["original_sizes"]):
                    d[key] = d[key][:, :, :h, :w].contiguous()
        return res


class FasterRCNN(_Detector):
    """torchvision's fasterrcnn_*_fpn at test time on the library's kernels: ResNetFPN(padded) -> RPN ->
    multiscale_roi_align -> BoxHead -> postprocess_detections.  forward takes the already normalised batch; predict
    takes a list of images of different sizes (GeneralizedRCNNTransform in one launch) and returns boxes in each image's
    own pixels."""

    def __init__(self, backbone, rpn, box_head, detections, score_thresh, nms_thresh, max_candidates, device,
                 select="torch"):
        super().__init__(device, detections)
        self.select = _check_select(select)
        self.backbone, self.rpn, self.box_head = backbone, rpn, box_head
        self.score_thresh, self.nms_thresh = float(score_thresh), float(nms_thresh)
        self.max_candidates = max_candidates

    @classmethod
    def from_state_dict(cls, sd, arch: str, num_classes=None, out_channels: int = 256, P: int = 7, eps: float = 1e-5,
                        rpn_pre_nms_top_n: int = 1000, rpn_post_nms_top_n: int = 1000, rpn_nms_thresh: float = 0.7,
                        rpn_score_thresh: float = 0.0, box_score_thresh: float = SCORE_THRESH_STRICT,
                        box_nms_thresh: float = 0.5, box_detections_per_img: int = 100, max_candidates=None, sizes=ANCHOR_SIZES,
                        ratios=ANCHOR_RATIOS, device=None, select: str = "torch") -> "FasterRCNN":
        """sd under torchvision's key names: backbone.body.*, backbone.fpn.*, rpn.*, roi_heads.box_head.*,
        roi_heads.box_predictor.*; each part is validated with check_state_dict.  select: "torch" or "kernel", for the
        RPN's filter_proposals and postprocess_detections alike (see the module docstring)."""
        from .fpn import ResNetFPN
        _check_select(select)
        parts = _split_by_prefix(sd, ("backbone.", "rpn.", "roi_heads."), "Faster R-CNN")
        backbone = ResNetFPN.from_state_dict(parts["backbone."], arch, out_channels, eps, device)
        rpn = RPN.from_state_dict(parts["rpn."], out_channels, sizes, ratios, rpn_pre_nms_top_n, rpn_post_nms_top_n,
                                  rpn_nms_thresh, rpn_score_thresh, 1e-3, backbone.device, select=select)
        box_head = BoxHead.from_state_dict(parts["roi_heads."], out_channels, P, backbone.device)
        if num_classes is not None and int(num_classes) != box_head.classes:
            raise WinoError(f"state dict has {box_head.classes} classes, num_classes={num_classes}")
        return cls(backbone, rpn, box_head, box_detections_per_img, box_score_thresh, box_nms_thresh, max_candidates,
                   backbone.device, select=select)

    def _prepare(self, N: int, H: int, W: int, for_predict: bool) -> None:
        """prepare(); for_predict: on behalf of prepare_images, so a branch may leave what only forward needs to the
        first forward.  The model counts as prepared (_shape) once the last branch is."""
        N, H, W, D, dev = int(N), int(H), int(W), self.detections, self.device
        if self.select == "kernel" and self.max_candidates is not None and int(self.max_candidates) > SELECT_MAX_ROWS:
            raise WinoError(f"select=\"kernel\" keeps at most {SELECT_MAX_ROWS} candidates, "
                            f"max_candidates={self.max_candidates}")
        for b in self.branches:
            b.check(H, W)
        self._shape = None   # (a prepare that raises from here on leaves the model unprepared, whatever it was before)
        with torch.cuda.device(dev):
            self.backbone.prepare(N, H, W)
            p = self.backbone._p
            level_hw = [(int(t.shape[1]) - 2, int(t.shape[2]) - 2) for t in p]
            level_hw.append(((level_hw[-1][0] + 1) // 2, (level_hw[-1][1] + 1) // 2))
            self.rpn.prepare(N, level_hw, (H, W))
            R, bh = N * self.rpn.post, self.box_head
            bh.prepare(R)
            self._pooled = torch.empty((R, bh.P, bh.P, bh.in_channels), dtype=torch.float32, device=dev)
            self._full_hw = torch.tensor([[float(H), float(W)]] * N, dtype=torch.float32, device=dev)
            # the detections as RoIAlign rows [N][D][5]: what every branch reads, so only written when there is one
            self._det_rois = torch.empty((N, D, 5), dtype=torch.float32, device=dev) if self.branches else None
            for b in self.branches:
                b.prepare(N, D, H, W, for_predict)
        self._shape = (N, H, W)

    def _detect(self, x, image_sizes, st):
        """Faster R-CNN's stages; returns (the result dict, the pyramid, image_hw)."""
        from . import multiscale_roi_align
        self._begin(x)
        N, H, W = self._shape
        hw = self._full_hw if image_sizes is None else image_sizes
        if tuple(hw.shape) != (N, 2) or hw.device != self.device or hw.dtype != torch.float32:
            raise WinoError(f"image_sizes must be a float32 tensor [{N}][2] on {self.device}")
        with torch.cuda.device(self.device):
            feats = self.backbone(x, padded=True)
            rois, _, _ = self.rpn(feats, hw, (H, W), stages=st)
            pooled = multiscale_roi_align(feats, rois, (H, W), self.box_head.P, 2, in_padded=True, out=self._pooled)
            self.box_head(pooled)
            out = postprocess_detections(self.box_head._scores, rois, hw, self.box_head.classes, self.score_thresh,
                                         self.nms_thresh, self.detections, 1e-2, self.max_candidates, stages=st,
                                         rois_out=self._det_rois, select=self.select)
        if st is not None:
            st.update(features=feats, pooled=pooled, head_out=self.box_head._scores)
        return out, feats, hw


def _split_state_dict(sd, prefixes):
    """(the keys that start with none of `prefixes`, as they are; those that do, below `roi_heads.`)."""
    rest, part = {}, {}
    for k, v in sd.items():
        if k.startswith(prefixes):
            part[k[len("roi_heads."):]] = v
        else:
            rest[k] = v
    return rest, part


def _split_by_prefix(sd, prefixes, name: str):
    """{prefix: the keys of `sd` below it} for each of `prefixes`; a key below none of them raises, naming the model."""
    parts = {prefix: {} for prefix in prefixes}
    for k, v in sd.items():
        for prefix, part in parts.items():
            if k.startswith(prefix):
                part[k[len(prefix):]] = v
                break
        else:
            raise WinoError(f"state dict: unexpected key {k!r} for {name}")
    return parts


class _RoIBranch:
    """What runs on a detector's detections beside the box head.  A branch owns its head, its P, its RoIAlign output and
    its outputs; FasterRCNN calls check, prepare, run, finish and predict_outputs (see the module docstring) and knows
    nothing else about it."""

    def __init__(self, head, P: int):
        self.head, self.P = head, int(P)

    def check(self, H: int, W: int) -> None:
        """Raises for a batch size the branch cannot take, before anything is allocated."""

    def _prepare_head(self, R: int) -> None:
        self.head.prepare(R, self.P)
        self.pooled = torch.empty((R, self.P + 2, self.P + 2, self.head.in_channels), dtype=torch.float32,
                                  device=self.head.device)

    def _head_on(self, feats, det_rois, size):
        """RoIAlign on the detections and the head: (the head's raw GEMM output, its leading dimension)."""
        from . import multiscale_roi_align
        pooled = multiscale_roi_align(feats, det_rois.view(-1, 5), size, self.P, 2, in_padded=True, out_padded=True,
                                      out=self.pooled)
        return self.head(pooled, raw=True)


MASK_PREFIXES = ("roi_heads.mask_head.", "roi_heads.mask_predictor.")
MASK_OUTPUTS = ("prob", "binary", "both")


def split_mask_state_dict(sd):
    """(the Faster R-CNN keys as they are, the mask branch's keys below `roi_heads.`): BoxHead's validator rejects keys
    it does not know, so the mask branch leaves before it sees the rest."""
    return _split_state_dict(sd, MASK_PREFIXES)


class MaskBranch(_RoIBranch):
    """multiscale_roi_align (padded, P) -> MaskHead (raw logits) -> paste_masks in the gemm_rows layout: adds "masks"
    float32 and / or "masks_binary" uint8 (`masks`: "prob", "binary" or "both"), planes past count zero.  forward's are
    [N][D][H][W] planes of the batch; predict's are pasted once, at original size, with the rescaled boxes into
    [N][D][Hmax][Wmax], zero beyond each image's own size.  stages: mask_rois, mask_pooled and mask_logits (the raw
    [N*D*P*P*4][ld] GEMM output)."""

    def __init__(self, head, P: int, masks: str, threshold: float):
        super().__init__(head, P)
        self.masks, self.threshold = masks, threshold

    def prepare(self, N: int, D: int, H: int, W: int, for_predict: bool) -> None:
        self._prepare_head(N * D)
        self._labels32 = torch.empty((N, D), dtype=torch.int32, device=self.head.device)
        self._masks = self._masks_bin = None
        if not for_predict:
            self._planes(N, D, H, W)

    def _planes(self, N: int, D: int, H: int, W: int) -> None:
        """forward's mask planes [N][D][H][W] (0.8 GB of fp32 at N = 2, D = 100, 800 x 1216), unless they are there:
        predict pastes into planes of its own, so after prepare_images the first forward allocates them."""
        dev = self.head.device
        if self.masks != "binary" and self._masks is None:
            self._masks = torch.empty((N, D, H, W), dtype=torch.float32, device=dev)
        if self.masks != "prob" and self._masks_bin is None:
            self._masks_bin = torch.empty((N, D, H, W), dtype=torch.uint8, device=dev)

    def predict_outputs(self, tf, Hmax: int, Wmax: int) -> None:
        shape, dev = (*tf["boxes"].shape[:2], Hmax, Wmax), self.head.device
        tf["mask_hw"] = (Hmax, Wmax)
        tf["masks"] = torch.empty(shape, dtype=torch.float32, device=dev) if self.masks != "binary" else None
        tf["masks_bin"] = torch.empty(shape, dtype=torch.uint8, device=dev) if self.masks != "prob" else None

    def run(self, out, feats, det_rois, size, st) -> None:
        self._logits = self._head_on(feats, det_rois, size)[0]
        if st is not None:
            st.update(mask_rois=det_rois, mask_pooled=self.pooled, mask_logits=self._logits)

    def finish(self, out, image_hw, size, tf) -> None:
        from . import paste_masks
        if tf is None:
            self._planes(*out["labels"].shape, *size)
            masks, masks_bin = self._masks, self._masks_bin
        else:
            image_hw, size, masks, masks_bin = tf["orig_hw"], tf["mask_hw"], tf["masks"], tf["masks_bin"]
        self._labels32.copy_(out["labels"])
        prob, binary = paste_masks(self._logits, self._labels32, out["boxes"], image_hw, *size, M=2 * self.P,
                                   classes=self.head.classes, layout="gemm_rows", out=masks, binary=masks_bin,
                                   want_out=False, threshold=self.threshold)
        if prob is not None:
            out["masks"] = prob
        if binary is not None:
            out["masks_binary"] = binary


class MaskRCNN(FasterRCNN):
    """torchvision's maskrcnn_resnet50_fpn at test time: FasterRCNN, then on its detections multiscale_roi_align
    (padded, P = mask_P) -> MaskHead (raw logits) -> paste_masks in the gemm_rows layout.  forward's masks are image-size
    planes [N][D][H][W] of the normalised batch; predict's are pasted once, at original size, into [N][D][Hmax][Wmax]."""
    # the mask branch's buffers under the names they had on the model: read-only, the branch owns them
    _mask_pooled = property(lambda self: self.branches[0].pooled)
    _masks = property(lambda self: self.branches[0]._masks)
    _masks_bin = property(lambda self: self.branches[0]._masks_bin)

    @classmethod
    def from_state_dict(cls, sd, arch: str, num_classes=None, out_channels: int = 256, mask_P: int = 14,
                        masks: str = "prob", mask_threshold: float = 0.5, **faster_rcnn) -> "MaskRCNN":
        """sd: FasterRCNN's keys plus roi_heads.mask_head.* and roi_heads.mask_predictor.*.  masks: which tensors a
        forward returns, "prob" ("masks", float32), "binary" ("masks_binary", uint8 = prob > mask_threshold) or "both".
        Every other argument is FasterRCNN.from_state_dict's."""
        mask_P, mask_threshold = int(mask_P), float(mask_threshold)
        _check_select(faster_rcnn.get("select", "torch"))
        if masks not in MASK_OUTPUTS:
            raise WinoError(f"masks must be one of {MASK_OUTPUTS}, got {masks!r}")
        if mask_P < 2 or mask_P % 2 or 2 * mask_P > 62:
            raise WinoError(f"mask_P={mask_P}: need an even mask_P with 2 <= mask_P <= 31")
        if mask_threshold != mask_threshold:
            raise WinoError("mask_threshold is NaN")
        rest, mask_sd = split_mask_state_dict(sd)
        mask_classes = validate_mask_head_state_dict(mask_sd, out_channels)
        m = super().from_state_dict(rest, arch, num_classes, out_channels, device=faster_rcnn.pop("device", None),
                                    **faster_rcnn)
        if mask_classes != m.box_head.classes:
            raise WinoError(f"state dict: the mask head has {mask_classes} classes, the box head {m.box_head.classes}")
        m.mask_head = MaskHead.from_state_dict(mask_sd, out_channels, m.device)
        m.mask_P, m.masks, m.mask_threshold = mask_P, masks, mask_threshold
        m.branches = [MaskBranch(m.mask_head, mask_P, masks, mask_threshold)]
        return m


# ---- Keypoint R-CNN ------------------------------------------------------------------------------------------------------
KEYPOINT_CONVS = 8
KEYPOINT_PREFIXES = ("roi_heads.keypoint_head.", "roi_heads.keypoint_predictor.")
KEYPOINT_MAX_P = 16      # heatmaps_to_keypoints takes M = 4 P <= 64
KEYPOINT_MAX_SIDE = 16384


def pack_kps_deconv(w: torch.Tensor, b: torch.Tensor):
    """kps_score_lowres, ConvTranspose2d(C, K, 4, stride 2, padding 1): weight [C][K][4][4] and bias [K] -> (B [C][ld] with
    columns (ky, kx, k), ld = 16 K up to a multiple of 64 and the rest zero, the bias [K] as it is).  The GEMM of the pixels
    [R*P*P][C] with B leaves the transposed convolution's partial products, one row per INPUT pixel; unlike MaskHead's
    stride = kernel = 2 deconvolution up to four of them meet in an output pixel, so the bias cannot ride in the GEMM:
    heatmaps_to_keypoints' "deconv_rows" layout gathers them and adds it."""
    C, K = int(w.shape[0]), int(w.shape[1])
    B = w.new_zeros((C, _pad64(16 * K)))
    B[:, : 16 * K] = w.permute(0, 2, 3, 1).reshape(C, 16 * K)
    return B, b.clone()


def _keypoint_widths(sd):
    return [_dim0(sd, f"keypoint_head.{2 * i}.weight") for i in range(KEYPOINT_CONVS)]


def expected_keypoint_head_keys(in_channels: int, widths, K: int):
    """{key: shape} of KeypointRCNNHeads(in_channels, widths) + KeypointRCNNPredictor(widths[-1], K): the convolutions sit
    at the even indices of a Sequential whose odd entries are ReLUs."""
    exp, c = {}, int(in_channels)
    for i, wd in enumerate(widths):
        exp[f"keypoint_head.{2 * i}.weight"] = (int(wd), c, 3, 3)
        exp[f"keypoint_head.{2 * i}.bias"] = (int(wd),)
        c = int(wd)
    exp["keypoint_predictor.kps_score_lowres.weight"] = (c, int(K), 4, 4)
    exp["keypoint_predictor.kps_score_lowres.bias"] = (int(K),)
    return exp


def validate_keypoint_head_state_dict(sd, in_channels: int = 256) -> int:
    """Checks every key and shape on the host; the eight widths are read off the convolutions and K off
    kps_score_lowres.  Returns K."""
    in_channels = int(in_channels)
    widths = _keypoint_widths(sd)
    w = sd.get("keypoint_predictor.kps_score_lowres.weight")
    if w is None:
        raise WinoError("state dict: missing key 'keypoint_predictor.kps_score_lowres.weight'")
    if w.dim() != 4:
        raise WinoError(f"state dict: key 'keypoint_predictor.kps_score_lowres.weight' has shape {tuple(w.shape)}, the "
                        "keypoint head needs [C][K][4][4]")
    K = int(w.shape[1])
    check_state_dict(sd, expected_keypoint_head_keys(in_channels, widths, K), "the keypoint head", "weight")
    for c in [in_channels] + widths:
        if c < 64 or c % 64:
            raise WinoError(f"keypoint head: every width must be a multiple of 64, got in_channels={in_channels}, "
                            f"widths={widths}")
    if K < 1:
        raise WinoError("keypoint head: K=0 keypoints")
    return K


class KeypointHead(_ConvTower):
    """KeypointRCNNHeads + KeypointRCNNPredictor on the Winograd 3x3 and the 1x1 GEMM kernels, inference only: eight
    conv3x3_bn_relu launches at N = R, then the transposed convolution's partial products as one GEMM."""

    def __init__(self, in_channels: int, widths, K: int, device):
        super().__init__(device)
        self.in_channels, self.widths, self.K = int(in_channels), [int(w) for w in widths], int(K)

    @classmethod
    def from_state_dict(cls, sd, in_channels: int = 256, device=None) -> "KeypointHead":
        K = validate_keypoint_head_state_dict(sd, in_channels)
        return cls._load(sd, None, device, in_channels, _keypoint_widths(sd), K)

    def _pack(self, sd, eps):
        self._pack_tower(sd, [f"keypoint_head.{2 * i}" for i in range(KEYPOINT_CONVS)])
        wd, bd = pack_kps_deconv(sd["keypoint_predictor.kps_score_lowres.weight"],
                                 sd["keypoint_predictor.kps_score_lowres.bias"])
        self.wd, self.bias = self._t(wd), self._t(bd)
        self.ld = int(self.wd.shape[1])
        n = max(self.widths + [self.ld])
        self._ones = torch.ones(n, dtype=torch.float32, device=self.device)
        self._zeros = torch.zeros(self.ld, dtype=torch.float32, device=self.device)
        torch.cuda.current_stream().synchronize()

    def prepare(self, R: int, P: int = 14) -> None:
        """Allocate the ping-pong tensors [R][P+2][P+2][width] (two when the widths agree, as torchvision's 512s do) and
        the rows tensor [R*P*P][ld], and reserve the stream scratch of the nine launches on the current stream.  Call it
        before capturing a forward into a graph."""
        R, P, f32, dev = int(R), int(P), torch.float32, self.device
        if R < 1 or not 1 <= P <= KEYPOINT_MAX_P:
            raise WinoError(f"keypoint head: R={R} boxes of P={P}: need R >= 1 and 1 <= P <= {KEYPOINT_MAX_P}")
        with torch.cuda.device(dev):
            self._alloc_tower(R, P)
            self._rows = torch.empty((R * P * P, self.ld), dtype=f32, device=dev)
            self._maps = torch.empty((R, self.K, 4 * P, 4 * P), dtype=f32, device=dev)
            self._reserve_tower(R, P)
            conv1x1_prepare(R * P * P, self.widths[-1], self.ld)
        self._shape = (R, P)

    def forward(self, pooled_padded: torch.Tensor, raw: bool = False):
        """pooled_padded [R][P+2][P+2][in_channels] float32 with a zero ring (roi_align's out_padded output; it is not
        written) -> torchvision's keypoint logits [R][K][4P][4P], a tensor of the head's, valid until the next forward.
        A new (R, P) re-runs prepare().  raw=True: returns (the GEMM's output [R*P*P][ld], rows (r, iy, ix) and columns
        (ky, kx, k), ld): heatmaps_to_keypoints' "deconv_rows" layout, to be passed with the head's `bias`.  raw=False
        composes the logits in torch (fold, bias, x2 bilinear upsample): plumbing for callers who want them, not on
        KeypointRCNN's path."""
        R, P = self._begin_tower(pooled_padded)
        K, ld = self.K, self.ld
        with torch.cuda.device(self.device):
            top = self._run_tower(pooled_padded)
            conv1x1_bn_ex(top, self.wd, self._zeros, self._ones[:ld], A_PADDED, out=self._rows)
            if raw:
                return self._rows, ld
            F = torch.nn.functional
            cols = self._rows[:, : 16 * K].view(R, P, P, 4, 4, K).permute(0, 5, 3, 4, 1, 2).reshape(R, 16 * K, P * P)
            low = F.fold(cols, (2 * P, 2 * P), kernel_size=4, stride=2, padding=1) + self.bias.view(1, K, 1, 1)
            self._maps.copy_(F.interpolate(low, scale_factor=2, mode="bilinear", align_corners=False))
        return self._maps


def split_keypoint_state_dict(sd):
    """(the Faster R-CNN keys as they are, the keypoint branch's keys below `roi_heads.`), like split_mask_state_dict."""
    return _split_state_dict(sd, KEYPOINT_PREFIXES)


class KeypointBranch(_RoIBranch):
    """multiscale_roi_align (padded, P) -> KeypointHead (raw rows) -> heatmaps_to_keypoints in the deconv_rows layout: adds
    "keypoints" [N][D][K][3] = (x, y, 1) and "keypoints_scores" [N][D][K], rows past count zero.  They are computed on the
    un-rescaled detections; predict multiplies the keypoints by (rw, rh, 1) (torchvision's resize_keypoints).  stages:
    keypoint_rois, keypoint_pooled and keypoint_rows (the raw [N*D*P*P][ld] GEMM output)."""

    def check(self, H: int, W: int) -> None:
        if max(int(H), int(W)) > KEYPOINT_MAX_SIDE:
            raise WinoError(f"Keypoint R-CNN: a batch of {H} x {W} exceeds {KEYPOINT_MAX_SIDE} pixels a side")

    def prepare(self, N: int, D: int, H: int, W: int, for_predict: bool) -> None:
        K, dev = self.head.K, self.head.device
        self._prepare_head(N * D)
        self._keypoints = torch.empty((N, D, K, 3), dtype=torch.float32, device=dev)
        self._kp_scores = torch.empty((N, D, K), dtype=torch.float32, device=dev)

    def predict_outputs(self, tf, Hmax: int, Wmax: int) -> None:
        (N, D), K, dev = tf["boxes"].shape[:2], self.head.K, self.head.device
        ones = torch.ones((N, 1, 1), dtype=torch.float32, device=dev)
        tf["kp_ratio"] = torch.cat([tf["ratio"][:, :, :2], ones], dim=2).reshape(N, 1, 1, 3).contiguous()   # (rw, rh, 1)
        tf["keypoints"] = torch.empty((N, D, K, 3), dtype=torch.float32, device=dev)

    def run(self, out, feats, det_rois, size, st) -> None:
        from . import heatmaps_to_keypoints
        rows, ld = self._head_on(feats, det_rois, size)
        heatmaps_to_keypoints(rows, det_rois, K=self.head.K, M=4 * self.P, layout="deconv_rows", bias=self.head.bias, ld=ld,
                              max_side=max(size), out=self._keypoints, scores_out=self._kp_scores)
        out["keypoints"], out["keypoints_scores"] = self._keypoints, self._kp_scores
        if st is not None:
            st.update(keypoint_rois=det_rois, keypoint_pooled=self.pooled, keypoint_rows=rows)

    def finish(self, out, image_hw, size, tf) -> None:
        if tf is not None:
            out["keypoints"] = torch.mul(out["keypoints"], tf["kp_ratio"], out=tf["keypoints"])


class KeypointRCNN(FasterRCNN):
    """torchvision's keypointrcnn_resnet50_fpn at test time: FasterRCNN, then on its detections multiscale_roi_align
    (padded, P = keypoint_P) -> KeypointHead (raw rows) -> heatmaps_to_keypoints in the deconv_rows layout.  Adds
    "keypoints" [N][D][K][3] = (x, y, 1) and "keypoints_scores" [N][D][K], rows past count zero."""
    _kp_pooled = property(lambda self: self.branches[0].pooled)   # (the name it had on the model; the branch owns it)

    @classmethod
    def from_state_dict(cls, sd, arch: str, num_classes=None, out_channels: int = 256, keypoint_P: int = 14,
                        **faster_rcnn) -> "KeypointRCNN":
        """sd: FasterRCNN's keys plus roi_heads.keypoint_head.* and roi_heads.keypoint_predictor.*.  Every other argument
        is FasterRCNN.from_state_dict's."""
        keypoint_P = int(keypoint_P)
        _check_select(faster_rcnn.get("select", "torch"))
        if not 1 <= keypoint_P <= KEYPOINT_MAX_P:
            raise WinoError(f"keypoint_P={keypoint_P}: need 1 <= keypoint_P <= {KEYPOINT_MAX_P}")
        rest, kp_sd = split_keypoint_state_dict(sd)
        validate_keypoint_head_state_dict(kp_sd, out_channels)
        m = super().from_state_dict(rest, arch, num_classes, out_channels, device=faster_rcnn.pop("device", None),
                                    **faster_rcnn)
        m.keypoint_head = KeypointHead.from_state_dict(kp_sd, out_channels, m.device)
        m.keypoint_P = keypoint_P
        m.branches = [KeypointBranch(m.keypoint_head, keypoint_P)]
        return m


# ---- the dense detectors: what RetinaNet and FCOS share -------------------------------------------------------------------------
RETINA_LEVELS = ("0", "1", "2", "p6", "p7")
RETINA_CONVS = 4
RETINA_NMS_SCORE_MIN = 1.1754943508222875e-38   # FLT_MIN: what a padding row's score 0.0 fails in batched_nms
FCOS_GROUPS = 32     # torchvision's GroupNorm(32, in_channels) between FCOS's tower convolutions


class _DenseHead(_ConvTower):
    """What RetinaNetHead and FCOSHead share: a classification and a regression tower of RETINA_CONVS 3x3 convolutions and
    a last 3x3 without ReLU, run per level with the same packed weights on every level, into padded maps of the head's.
    A tower without norms runs its convolutions with ReLU; one with norms runs them without and follows each with
    groupnorm_relu in place.  A subclass gives `name` (for messages), `cols`, `ld_cls`, `ld_reg` and a `_pack(sd, eps)`
    that hands `_pack_towers` the keys of its two towers."""

    def __init__(self, in_channels: int, classes: int, device):
        super().__init__(device)
        self.in_channels, self.classes = int(in_channels), int(classes)
        self.widths = [self.in_channels] * RETINA_CONVS

    def _pack_towers(self, sd, towers) -> None:
        """towers: per tower (the stems of its convolutions, the stems of their GroupNorms or None, the stems of the last
        convolutions, concatenated along K).  Sets `towers` = [(convs [(U, bias)], norms [(gamma, beta)] or None, U and
        bias of the last convolution, its padded width)]."""
        self.towers = []
        for stems, norm_stems, last in towers:
            self._pack_tower(sd, stems)
            norms = norm_stems and [(self._t(sd[f"{s}.weight"]), self._t(sd[f"{s}.bias"])) for s in norm_stems]
            wl, bl = pack_retina_last(torch.cat([sd[f"{s}.weight"] for s in last]), torch.cat([sd[f"{s}.bias"] for s in last]))
            self.towers.append((self.convs, norms, filter_transform_f2(self._t(wl)), self._t(bl), int(wl.shape[0])))
        del self.convs
        self._ones = torch.ones(max(self.in_channels, self.ld_cls, self.ld_reg), dtype=torch.float32, device=self.device)
        torch.cuda.current_stream().synchronize()

    def prepare(self, N: int, level_hw) -> None:
        """Allocate, per level of `level_hw` [(h, w)], the two ping-pong tensors both towers share, the two output maps
        and, for a head with norms, the GroupNorm workspace, and reserve the stream scratch of every convolution on the
        current stream.  Call it before capturing a forward into a graph."""
        N, C, dev, f32 = int(N), self.in_channels, self.device, torch.float32
        level_hw = tuple((int(h), int(w)) for h, w in level_hw)
        if N < 1 or not level_hw or min(min(hw) for hw in level_hw) < 1:
            raise WinoError(f"{self.name}: N={N} images, levels {level_hw}")
        with torch.cuda.device(dev):
            zeros = lambda h, w, c: torch.zeros((N, h + 2, w + 2, c), dtype=f32, device=dev)
            self._pp = [(zeros(h, w, C), zeros(h, w, C)) for h, w in level_hw]
            self._cls = [zeros(h, w, self.ld_cls) for h, w in level_hw]
            self._reg = [zeros(h, w, self.ld_reg) for h, w in level_hw]
            if self.towers[0][1] is not None:
                # the split form's size whatever the plan says now: a WINO_GN_FORM set after prepare finds room
                self._gn_ws = [torch.empty((N * min(h * w, 128) * 4 * FCOS_GROUPS,), dtype=f32, device=dev) for h, w in level_hw]
            for h, w in level_hw:
                for k in (C, self.ld_cls, self.ld_reg):
                    conv3x3_prepare(N, C, k, h, w)
        self._shape = (N, level_hw)

    def forward(self, maps):
        """maps: the levels' padded features [N][h+2][w+2][in_channels] (zero rings; they are not written).  Returns
        (class maps, regression maps), one per level: tensors of the head's, valid until the next forward.  New shapes
        re-run prepare()."""
        from . import groupnorm_relu   # looked up per call: a tool that times the convolutions alone replaces it
        maps, C = list(maps), self.in_channels
        for x in maps:
            if not isinstance(x, torch.Tensor) or x.dim() != 4 or int(x.shape[3]) != C or min(x.shape[1:3]) < 3:
                raise WinoError(f"{self.name}: every level must be [N][h+2][w+2][{C}]")
            if x.device != self.device or x.dtype != torch.float32 or not x.is_contiguous():
                raise WinoError(f"{self.name}: every level must be contiguous float32 on {self.device}")
        shape = (int(maps[0].shape[0]), tuple((int(x.shape[1]) - 2, int(x.shape[2]) - 2) for x in maps))
        if any(int(x.shape[0]) != shape[0] for x in maps):
            raise WinoError(f"{self.name}: the levels differ in N")
        if shape != self._shape:
            self.prepare(*shape)
        with torch.cuda.device(self.device):
            for l, x0 in enumerate(maps):
                for (convs, norms, U, bias, kp), outs in zip(self.towers, (self._cls, self._reg)):
                    x = x0
                    for i, (Ui, bi) in enumerate(convs):
                        x = conv3x3_bn_relu(x, Ui, bi, self._ones[:C], relu=norms is None, out=self._pp[l][i % 2])
                        if norms is not None:
                            groupnorm_relu(x, *norms[i], FCOS_GROUPS, out=x, workspace=self._gn_ws[l])
                    conv3x3_bn_relu(x, U, bias, self._ones[:kp], relu=False, out=outs[l])
        return self._cls, self._reg


class _DenseDetector(_Detector):
    """What RetinaNet and FCOS share: ResNetFPN(returned_layers = (2, 3, 4), extra_blocks = "p6p7", padded) -> the head ->
    per level select_topk_map on the class map in place and the model's decode of the selected rows -> one select_topk over
    the levels' candidates by score with the boxes as payload -> batched_nms with groups = label -> the padded result.
    A model gives `name`, `head_cls` and `validate_head`, `threshold` (score_thresh -> what select_topk_map compares
    with, kept as `thresh`), `values_key` (the stage key of the selected values), `ctr_col` (the regression map's
    centerness column where fcos_score_map runs before the select, else None), `_decode` and `_scores`."""
    ctr_col = None

    def __init__(self, backbone, head, base, detections, score_thresh, nms_thresh, topk_candidates, device):
        """base: the base anchors [A][4] of each level, host tensors."""
        super().__init__(device, detections)
        self.backbone, self.head = backbone, head
        self.score_thresh, self.nms_thresh, self.topk = float(score_thresh), float(nms_thresh), int(topk_candidates)
        self.thresh = self.threshold(self.score_thresh)
        with torch.cuda.device(self.device):
            self.base = [self._t(b) for b in base]
            torch.cuda.current_stream().synchronize()

    @classmethod
    def _load_parts(cls, sd, arch, num_classes, sizes_ok: bool, sizes_need: str, score_thresh, topk_candidates,
                    detections_per_img, device, out_channels, eps, *head_args):
        """from_state_dict's shared part: the argument checks, the state dict split into `backbone.` and `head.` and
        validated, and (the backbone, the head) loaded; `head_args` go between out_channels and the device."""
        from .fpn import ResNetFPN
        levels = len(RETINA_LEVELS)
        if not sizes_ok:
            raise WinoError(f"{cls.name}: {levels} levels need {levels} {sizes_need}")
        cls.threshold(score_thresh)
        if not 1 <= int(topk_candidates) <= SELECT_MAX_ROWS // levels or int(detections_per_img) < 1:
            raise WinoError(f"{cls.name}: topk_candidates={topk_candidates} (the levels' candidates are sorted by one "
                            f"select_topk of at most {SELECT_MAX_ROWS} rows), detections_per_img={detections_per_img}")
        parts = _split_by_prefix(sd, ("backbone.", "head."), cls.name)
        classes = cls.validate_head(parts["head."], out_channels, *head_args)
        if num_classes is not None and int(num_classes) != classes:
            raise WinoError(f"state dict has {classes} classes, num_classes={num_classes}")
        backbone = ResNetFPN.from_state_dict(parts["backbone."], arch, out_channels, eps, device, returned_layers=(2, 3, 4),
                                             extra_blocks="p6p7")
        return backbone, cls.head_cls.from_state_dict(parts["head."], out_channels, *head_args, backbone.device)

    def _prepare(self, N: int, H: int, W: int, for_predict: bool) -> None:
        from . import nms_workspace_bytes, select_map_workspace_bytes, select_workspace_bytes
        N, H, W, D, dev, f32, i32 = int(N), int(H), int(W), self.detections, self.device, torch.float32, torch.int32
        self._shape = None
        with torch.cuda.device(dev):
            self.backbone.prepare(N, H, W)
            level_hw = [(int(t.shape[1]) - 2, int(t.shape[2]) - 2) for t in (*self.backbone._p, *self.backbone._extra[::2])]
            self.head.prepare(N, level_hw)
            cols = self.head.cols
            self._grid = [(h, w, H // h, W // w) for h, w in level_hw]
            if min(min(g[2:]) for g in self._grid) < 1:
                raise WinoError(f"{self.name}: a batch of {H} x {W} is smaller than its pyramid levels {level_hw}")
            self._k = [min(self.topk, h * w * cols) for h, w in level_hw]
            self._off = [sum(self._k[:l]) for l in range(len(self._k))]
            K = sum(self._k)
            empty = lambda shape, dtype=f32: torch.empty(shape, dtype=dtype, device=dev)
            self._b = dict(
                idx=empty((N, K), i32), vals=empty((N, K)), count=[empty((N,), i32) for _ in level_hw], boxes=empty((N, K, 4)),
                labels=empty((N, K), i32), order=empty((N, K), i32), sscores=empty((N, K)), count2=empty((N, 1), i32),
                sboxes=empty((N, K, 4)), keep=empty((N, D), i32), det_count=empty((N,), i32),
                ws=[empty(((select_map_workspace_bytes(N, h, w, cols, k) + 3) // 4,)) for (h, w), k in zip(level_hw, self._k)],
                ws2=empty(((select_workspace_bytes(N, K, K) + 3) // 4,)), nms=empty(((nms_workspace_bytes(N, K) + 3) // 4,)))
            self._full_hw = torch.tensor([[float(H), float(W)]] * N, dtype=f32, device=dev)
        self._shape = (N, H, W)

    def _detect(self, x, image_sizes, st):
        """The dense detector's stages; returns (the result dict, the pyramid, image_hw)."""
        from . import batched_nms, fcos_score_map, select_topk, select_topk_map
        self._begin(x)
        N, H, W = self._shape
        hw = self._full_hw if image_sizes is None else image_sizes
        if tuple(hw.shape) != (N, 2) or hw.device != self.device or hw.dtype != torch.float32:
            raise WinoError(f"image_sizes must be a float32 tensor [{N}][2] on {self.device}")
        b, K, cols = self._b, self.head.classes, self.head.cols
        with torch.cuda.device(self.device):
            feats = self.backbone(x, padded=True)
            cls, reg = self.head([feats[name] for name in RETINA_LEVELS])
            for l, (k, off) in enumerate(zip(self._k, self._off)):
                if self.ctr_col is not None:
                    fcos_score_map(cls[l], reg[l], K, self.ctr_col)
                select_topk_map(cls[l], cols, k, self.thresh, b["idx"], b["vals"], b["count"][l], off, b["ws"][l])
                self._decode(b["idx"], reg[l], self.base[l], hw, self._grid[l], K, k, b["boxes"], b["labels"], off)
            scores = self._scores(b["idx"], b["vals"])
            order, sscores, _, sboxes = select_topk(scores, sum(self._k), boxes=b["boxes"], out_idx=b["order"],
                                                    out_vals=b["sscores"], out_count=b["count2"], out_boxes=b["sboxes"],
                                                    workspace=b["ws2"])
            slabels = b["labels"].gather(1, order.long())
            keep, count = batched_nms(sboxes, sscores, slabels, self.nms_thresh, 0.0, RETINA_NMS_SCORE_MIN, self.detections,
                                      workspace=b["nms"], keep=b["keep"], count=b["det_count"])
            kept = keep >= 0
            at = keep.clamp(min=0).long()
            out = {"boxes": sboxes.gather(1, at[:, :, None].expand(-1, -1, 4)) * kept[:, :, None],
                   "scores": sscores.gather(1, at) * kept,
                   "labels": torch.where(kept, slabels.gather(1, at).long(), torch.full_like(at, -1)), "count": count}
        if st is not None:
            st.update({self.values_key: b["vals"]}, features=feats, cls_maps=list(cls), reg_maps=list(reg), level_idx=b["idx"],
                      level_count=torch.stack(b["count"]), cand_boxes=b["boxes"], cand_labels=b["labels"], cand_scores=scores,
                      order=order, sorted_boxes=sboxes, sorted_scores=sscores, sorted_labels=slabels, det_keep=keep)
        return out, feats, hw


# ---- RetinaNet --------------------------------------------------------------------------------------------------------------
RETINA_SIZES = tuple((x, int(x * 2 ** (1.0 / 3)), int(x * 2 ** (2.0 / 3))) for x in (32, 64, 128, 256, 512))


def logit_threshold(score_thresh: float) -> float:
    """The fp32 logit t with sigmoid(t) > score_thresh >= sigmoid(pred(t)), sigmoid evaluated in fp64: the fp32 successor
    of log(s / (1 - s)).  `logit >= t` is then `sigmoid(logit) > s` on exact arithmetic: torchvision's strict compare,
    moved in front of the sigmoid."""
    import math
    s = float(score_thresh)
    if not 0.0 < s < 1.0:
        raise WinoError(f"score_thresh={score_thresh}: RetinaNet thresholds the logit and needs 0 < score_thresh < 1")
    # sigmoid in fp64 is monotone over the fp32 numbers: bisect their order (the bit patterns, negatives mirrored) for the
    # first one whose sigmoid exceeds s.  No stepping from log(s / (1 - s)): at s = 0.5 the first fp32 number whose fp64
    # sigmoid exceeds 0.5 lies 2^29 numbers above 0.
    import struct
    sig = lambda v: 0.0 if v < -700.0 else 1.0 / (1.0 + math.exp(-v))
    value = lambda key: struct.unpack("<f", struct.pack("<I", key if key >= 0 else 0x80000000 - key - 1))[0]   # -1 is -0.0
    lo, hi = -0x7f800001, 0x7f800000   # -Inf (sigmoid 0 <= s) and +Inf (sigmoid 1 > s)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if sig(value(mid)) > s:
            hi = mid
        else:
            lo = mid
    return value(hi)


def _retina_conv(sd, head: str, i: int) -> str:
    """The stem of tower convolution i of `head`: conv.{i}.0 (Conv2dNormActivation), or the legacy Sequential's
    conv.{2i} (its odd entries are ReLUs)."""
    return f"{head}.conv.{2 * i}" if f"{head}.conv.0.weight" in sd else f"{head}.conv.{i}.0"


def expected_retinanet_head_keys(sd, in_channels: int, A: int, classes: int):
    """{key: shape} of torchvision's RetinaNetHead below `head.`; the legacy spelling conv.{2i} is accepted per tower."""
    C, exp = int(in_channels), {}
    for head, last, width in (("classification_head", "cls_logits", A * classes), ("regression_head", "bbox_reg", 4 * A)):
        for i in range(RETINA_CONVS):
            exp[f"{_retina_conv(sd, head, i)}.weight"] = (C, C, 3, 3)
            exp[f"{_retina_conv(sd, head, i)}.bias"] = (C,)
        exp[f"{head}.{last}.weight"] = (width, C, 3, 3)
        exp[f"{head}.{last}.bias"] = (width,)
    return exp


def validate_retinanet_head_state_dict(sd, in_channels: int = 256, A: int = 9) -> int:
    """Checks every key and shape on the host; the class count is read off cls_logits.  Returns it."""
    in_channels, A = int(in_channels), int(A)
    width = _dim0(sd, "classification_head.cls_logits.weight")
    if A < 1 or width < A or width % A:
        raise WinoError(f"state dict: key 'classification_head.cls_logits.weight' has {width} channels for A={A} anchors")
    check_state_dict(sd, expected_retinanet_head_keys(sd, in_channels, A, width // A), "the RetinaNet head", "weight")
    if in_channels < 64 or in_channels % 64:
        raise WinoError(f"RetinaNet head: in_channels={in_channels} must be a multiple of 64")
    return width // A


def pack_retina_last(w: torch.Tensor, b: torch.Tensor):
    """A tower's last 3x3, weight [K][C][3][3] and bias [K] -> the same with K zero-padded to a multiple of 64 (819 -> 832,
    36 -> 64): the pad columns of the map are then exactly 0."""
    K, kp = int(w.shape[0]), _pad64(int(w.shape[0]))
    wp, bp = w.new_zeros((kp,) + tuple(w.shape[1:])), b.new_zeros(kp)
    wp[:K], bp[:K] = w, b
    return wp, bp


class RetinaNetHead(_DenseHead):
    """torchvision's RetinaNetHead (classification and regression towers, no norm layer) on the Winograd 3x3, inference
    only: per level four conv3x3 + ReLU and one conv3x3 without, per tower, with the same packed weights on every level.
    The outputs stay the padded maps the kernels write: class logits [N][h+2][w+2][pad64(A classes)] with channel
    a * classes + k, box regression [N][h+2][w+2][pad64(4 A)] with anchor a's deltas at 4a .. 4a + 3 -- what
    select_topk_map and retina_decode read in place."""

    name = "RetinaNet head"

    def __init__(self, in_channels: int, A: int, classes: int, device):
        super().__init__(in_channels, classes, device)
        self.A = int(A)
        self.cols, self.ld_cls, self.ld_reg = self.A * self.classes, _pad64(self.A * self.classes), _pad64(4 * self.A)

    @classmethod
    def from_state_dict(cls, sd, in_channels: int = 256, A: int = 9, device=None) -> "RetinaNetHead":
        """sd: the keys below torchvision's `head.`."""
        classes = validate_retinanet_head_state_dict(sd, in_channels, A)
        return cls._load(sd, None, device, in_channels, A, classes)

    def _pack(self, sd, eps):
        self._pack_towers(sd, [([_retina_conv(sd, head, i) for i in range(RETINA_CONVS)], None, [f"{head}.{last}"])
                               for head, last in (("classification_head", "cls_logits"), ("regression_head", "bbox_reg"))])


class RetinaNet(_DenseDetector):
    """torchvision's retinanet_resnet50_fpn at test time on the library's kernels: ResNetFPN(returned_layers = (2, 3, 4),
    extra_blocks = "p6p7", padded) -> RetinaNetHead -> per level select_topk_map on the class logit map in place and
    retina_decode of the selected anchors -> one select_topk over the levels' candidates by score with the boxes as
    payload -> batched_nms with groups = label.  Scores are torch plumbing, as in RPN: sigmoid(logit) where a row is
    kept, else 0; the labels follow the sort by a torch gather.  forward takes the normalised batch, predict a list of
    images (the shared detector path).  After prepare a forward reads no device data on the host and is captured into
    one graph, bit-identical to the eager run.

    Named deviations from torchvision's postprocess_detections:
      * the threshold is applied to the logit, `logit >= t` with t = logit_threshold(score_thresh), the fp32 successor of
        log(s / (1 - s)) evaluated in fp64, not to the fp32 sigmoid (`sigmoid(logit) > s`): the two differ only where
        the fp32 sigmoid rounds across s;
      * the per-level top-k orders by logit with ties to the lower index (torchvision's order among equal scores is
        unspecified), and so does the order in which equal scores enter the NMS.
    Not built: the v2 heads (they need P6 from C5 beside the GroupNorm kernel FCOSHead runs), SSD."""

    name, head_cls, values_key = "RetinaNet", RetinaNetHead, "level_logits"
    validate_head, threshold = staticmethod(validate_retinanet_head_state_dict), staticmethod(logit_threshold)

    def __init__(self, backbone, head, sizes, ratios, detections, score_thresh, nms_thresh, topk_candidates, device):
        self.sizes, self.ratios = tuple(tuple(s) for s in sizes), tuple(ratios)
        super().__init__(backbone, head, [base_anchors(s, self.ratios) for s in self.sizes], detections, score_thresh,
                         nms_thresh, topk_candidates, device)

    @classmethod
    def from_state_dict(cls, sd, arch: str, num_classes=None, score_thresh: float = 0.05, nms_thresh: float = 0.5,
                        detections_per_img: int = 300, topk_candidates: int = 1000, sizes=RETINA_SIZES, ratios=ANCHOR_RATIOS,
                        device=None, out_channels: int = 256, eps: float = 1e-5) -> "RetinaNet":
        """sd under torchvision's key names: backbone.body.*, backbone.fpn.* (inner_blocks / layer_blocks 0..2 and
        extra_blocks.p6|p7) and head.*; each part is validated with check_state_dict."""
        ok = len(sizes) == len(RETINA_LEVELS) and len({len(s) for s in sizes}) == 1
        backbone, head = cls._load_parts(sd, arch, num_classes, ok, "size tuples of one length", score_thresh,
                                         topk_candidates, detections_per_img, device, out_channels, eps,
                                         len(sizes[0]) * len(ratios) if ok else 0)
        return cls(backbone, head, sizes, ratios, detections_per_img, score_thresh, nms_thresh, topk_candidates,
                   backbone.device)

    def _decode(self, *operands):
        from . import retina_decode
        retina_decode(*operands)

    def _scores(self, idx, logit):
        return torch.where(idx >= 0, torch.sigmoid(logit), torch.zeros_like(logit))


# ---- FCOS ------------------------------------------------------------------------------------------------------------------
FCOS_SIZES = ((8,), (16,), (32,), (64,), (128,))
FCOS_CTR_COL = 4     # bbox_ctrness rides in column 4 of the regression map, beside bbox_reg's 0 .. 3


def score_threshold(score_thresh: float) -> float:
    """The fp32 successor of score_thresh: `score >= t` on fp32 scores is torchvision's strict `score > score_thresh`."""
    import numpy as np
    s = np.float32(score_thresh)
    if not 0.0 <= float(s) < 1.0:
        raise WinoError(f"score_thresh={score_thresh}: FCOS needs 0 <= score_thresh < 1")
    return float(np.nextafter(s, np.float32(np.inf)))


def expected_fcos_head_keys(in_channels: int, classes: int):
    """{key: shape} of torchvision's FCOSHead below `head.`: per tower conv.{0,3,6,9} (3x3 with bias) and their
    GroupNorms conv.{1,4,7,10}, then cls_logits, bbox_reg and bbox_ctrness."""
    C, exp = int(in_channels), {}
    for head in ("classification_head", "regression_head"):
        for i in range(RETINA_CONVS):
            exp[f"{head}.conv.{3 * i}.weight"], exp[f"{head}.conv.{3 * i}.bias"] = (C, C, 3, 3), (C,)
            exp[f"{head}.conv.{3 * i + 1}.weight"], exp[f"{head}.conv.{3 * i + 1}.bias"] = (C,), (C,)
    for key, width in (("classification_head.cls_logits", int(classes)), ("regression_head.bbox_reg", 4),
                       ("regression_head.bbox_ctrness", 1)):
        exp[f"{key}.weight"], exp[f"{key}.bias"] = (width, C, 3, 3), (width,)
    return exp


def validate_fcos_head_state_dict(sd, in_channels: int = 256) -> int:
    """Checks every key and shape on the host (the GroupNorm keys included); the class count is read off cls_logits.
    Returns it."""
    in_channels = int(in_channels)
    classes = _dim0(sd, "classification_head.cls_logits.weight")
    check_state_dict(sd, expected_fcos_head_keys(in_channels, classes), "the FCOS head", "weight")
    if in_channels < 64 or in_channels % 64 or (in_channels // FCOS_GROUPS) & (in_channels // FCOS_GROUPS - 1):
        raise WinoError(f"FCOS head: in_channels={in_channels} must be a multiple of 64 with in_channels / {FCOS_GROUPS} a "
                        "power of two")
    return classes


class FCOSHead(_DenseHead):
    """torchvision's FCOSHead (classification and regression towers with GroupNorm(32, C) + ReLU) on the Winograd 3x3 and
    the GroupNorm kernel, inference only: per level and tower four times conv3x3 (bias, no ReLU) -> groupnorm_relu in
    place, then the last 3x3 without ReLU, with the same packed weights on every level.  The outputs stay the padded maps
    the kernels write: class logits [N][h+2][w+2][pad64(classes)], and one regression map [N][h+2][w+2][64] with bbox_reg
    in columns 0 .. 3 (before its ReLU: fcos_decode applies it) and bbox_ctrness in column 4 -- what fcos_score_map,
    select_topk_map and fcos_decode read in place."""

    name = "FCOS head"

    def __init__(self, in_channels: int, classes: int, device):
        super().__init__(in_channels, classes, device)
        self.cols, self.ld_cls, self.ld_reg = self.classes, _pad64(self.classes), 64

    @classmethod
    def from_state_dict(cls, sd, in_channels: int = 256, device=None) -> "FCOSHead":
        """sd: the keys below torchvision's `head.`."""
        classes = validate_fcos_head_state_dict(sd, in_channels)
        return cls._load(sd, None, device, in_channels, classes)

    def _pack(self, sd, eps):
        self._pack_towers(sd, [([f"{head}.conv.{3 * i}" for i in range(RETINA_CONVS)],
                                [f"{head}.conv.{3 * i + 1}" for i in range(RETINA_CONVS)], [f"{head}.{k}" for k in last])
                               for head, last in (("classification_head", ("cls_logits",)),
                                                  ("regression_head", ("bbox_reg", "bbox_ctrness")))])


class FCOS(_DenseDetector):
    """torchvision's fcos_resnet50_fpn at test time on the library's kernels: ResNetFPN(returned_layers = (2, 3, 4),
    extra_blocks = "p6p7", padded) -> FCOSHead -> per level fcos_score_map in place on the class logit map,
    select_topk_map on the score map and fcos_decode of the selected locations -> one select_topk over the levels'
    candidates by score with the boxes as payload -> batched_nms with groups = label.  forward takes the normalised
    batch, predict a list of images (the shared detector path).  After prepare a forward reads no device data on the
    host and is captured into one graph, bit-identical to the eager run.

    Named deviations from torchvision's postprocess_detections:
      * equal scores go to the lower index, in the per-level top-k and in the order in which they enter the NMS
        (torchvision's order among equal scores is unspecified);
      * the score is the kernel's fp32 value of sqrt(sigmoid(logit) * sigmoid(centerness)); the threshold `score >
        score_thresh` is applied to it as `score >= score_threshold(score_thresh)`, its fp32 successor;
      * stages=True exposes the score maps ("cls_maps") where RetinaNet exposes logit maps: the logits are overwritten
        in place."""

    name, head_cls, values_key, ctr_col = "FCOS", FCOSHead, "level_scores", FCOS_CTR_COL
    validate_head, threshold = staticmethod(validate_fcos_head_state_dict), staticmethod(score_threshold)

    def __init__(self, backbone, head, sizes, detections, score_thresh, nms_thresh, topk_candidates, device):
        self.sizes = tuple(tuple(s) for s in sizes)
        super().__init__(backbone, head, [base_anchors(s, (1.0,)) for s in self.sizes], detections, score_thresh, nms_thresh,
                         topk_candidates, device)

    @classmethod
    def from_state_dict(cls, sd, arch: str, num_classes=None, score_thresh: float = 0.2, nms_thresh: float = 0.6,
                        detections_per_img: int = 100, topk_candidates: int = 1000, sizes=FCOS_SIZES, device=None,
                        out_channels: int = 256, eps: float = 1e-5) -> "FCOS":
        """sd under torchvision's key names: backbone.body.*, backbone.fpn.* (inner_blocks / layer_blocks 0..2 and
        extra_blocks.p6|p7) and head.*; each part is validated with check_state_dict."""
        ok = len(sizes) == len(RETINA_LEVELS) and all(len(s) == 1 for s in sizes)
        backbone, head = cls._load_parts(sd, arch, num_classes, ok, "tuples of one anchor size", score_thresh,
                                         topk_candidates, detections_per_img, device, out_channels, eps)
        return cls(backbone, head, sizes, detections_per_img, score_thresh, nms_thresh, topk_candidates, backbone.device)

    def _decode(self, *operands):
        from . import fcos_decode
        fcos_decode(*operands)

    def _scores(self, idx, score):
        return score                                     # (the select writes 0.0 past a level's kept count)


__all__ = ["BoxHead", "MaskHead", "KeypointHead", "RPN", "FasterRCNN", "MaskRCNN", "KeypointRCNN", "RetinaNetHead",
           "FCOSHead", "FCOS", "score_threshold", "expected_fcos_head_keys", "validate_fcos_head_state_dict",
           "RetinaNet", "logit_threshold", "expected_retinanet_head_keys", "validate_retinanet_head_state_dict",
           "pack_retina_last", "split_mask_state_dict",
           "split_keypoint_state_dict", "postprocess_detections", "base_anchors", "pack_rpn_head",
           "expected_rpn_keys", "expected_box_head_keys", "expected_mask_head_keys", "expected_keypoint_head_keys",
           "validate_box_head_state_dict", "validate_mask_head_state_dict", "validate_keypoint_head_state_dict", "pack_fc6",
           "pack_predictor", "pack_deconv", "pack_logits", "pack_kps_deconv"]
