"""The second stage of torchvision's Faster / Mask R-CNN on the library's kernels: what follows ``MultiScaleRoIAlign``
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

Not built: the RPN, box decoding, NMS, the post-processing (softmax / sigmoid, the selection of the predicted class's
mask, the paste into the image) and the BN variants of the v2 heads.  Boxes come from the caller.

The key names above are written from memory of torchvision's source and have not been checked against an installed
torchvision; the tests build their own state dicts under these names.
"""
from __future__ import annotations

import torch

from . import A_PADDED, RELU, WinoError, conv1x1_bn, conv1x1_bn_ex, conv1x1_prepare, conv3x3_bn_relu, conv3x3_prepare
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


class MaskHead(Net):
    """MaskRCNNHeads + MaskRCNNPredictor on the Winograd 3x3 and the 1x1 GEMM kernels, inference only."""

    def __init__(self, in_channels: int, classes: int, device):
        super().__init__(device)
        self.in_channels, self.classes = int(in_channels), int(classes)

    @classmethod
    def from_state_dict(cls, sd, in_channels: int = 256, device=None) -> "MaskHead":
        classes = validate_mask_head_state_dict(sd, in_channels)
        return cls._load(sd, None, device, in_channels, classes)

    def _pack(self, sd, eps):
        self.convs = [(filter_transform_f2(self._t(sd[f"mask_head.{i}.0.weight"])), self._t(sd[f"mask_head.{i}.0.bias"]))
                      for i in range(MASK_CONVS)]
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
            self._a = torch.zeros((R, P + 2, P + 2, C), dtype=f32, device=self.device)
            self._b = torch.zeros((R, P + 2, P + 2, C), dtype=f32, device=self.device)
            self._up = torch.empty((R * P * P, 4 * C), dtype=f32, device=self.device)
            self._scores = torch.empty((R * P * P * 4, kp), dtype=f32, device=self.device)
            self._masks = torch.empty((R, self.classes, 2 * P, 2 * P), dtype=f32, device=self.device)
            conv3x3_prepare(R, C, C, P, P)
            conv1x1_prepare(R * P * P, C, 4 * C)
            conv1x1_prepare(R * P * P * 4, C, kp)
        self._shape = (R, P)

    def forward(self, pooled_padded: torch.Tensor) -> torch.Tensor:
        """pooled_padded [R][P+2][P+2][C] float32 with a zero ring (roi_align's out_padded output; it is not written) ->
        mask logits [R][classes][2P][2P], a tensor of the head's, valid until the next forward.  A new (R, P) re-runs
        prepare()."""
        x, C = pooled_padded, self.in_channels
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or int(x.shape[3]) != C or x.shape[1] != x.shape[2]:
            raise WinoError(f"pooled_padded must be [R][P+2][P+2][{C}]")
        if x.device != self.device or x.dtype != torch.float32 or not x.is_contiguous():
            raise WinoError(f"pooled_padded must be contiguous float32 on {self.device}")
        R, P = int(x.shape[0]), int(x.shape[1]) - 2
        if (R, P) != self._shape:
            self.prepare(R, P)
        kp, ones = int(self.wl.shape[1]), self._ones
        with torch.cuda.device(self.device):
            src, dst = x, self._a
            for U, bias in self.convs:   # pooled -> a -> b -> a -> b
                conv3x3_bn_relu(src, U, bias, ones[:C], relu=True, out=dst)
                src, dst = dst, (self._b if dst is self._a else self._a)
            conv1x1_bn_ex(src, self.wd, self.bd, ones[: 4 * C], A_PADDED | RELU, out=self._up, hw=(P, P))
            # rows (r, y, x) x columns (dy, dx, c) are rows (r, y, x, dy, dx) x columns c: the logits GEMM's A as it stands
            conv1x1_bn(self._up.view(R * P * P * 4, C), self.wl, self.bl, ones[:kp], False, out=self._scores)
            scores = self._scores.view(R, P, P, 2, 2, kp)[..., : self.classes]
            self._masks.view(R, self.classes, P, 2, P, 2).copy_(scores.permute(0, 5, 1, 3, 2, 4))
        return self._masks


__all__ = ["BoxHead", "MaskHead", "expected_box_head_keys", "expected_mask_head_keys", "validate_box_head_state_dict",
           "validate_mask_head_state_dict", "pack_fc6", "pack_predictor", "pack_deconv", "pack_logits"]
