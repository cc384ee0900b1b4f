"""torchvision's FCN-ResNet50 / -101 and DeepLabV3-ResNet50 / -101 (``torchvision.models.segmentation.fcn_resnet*``,
``deeplabv3_resnet*``) on the library's kernels.

``FCN.from_state_dict(sd, arch)`` takes the segmentation model's state dict (its key names): ``backbone.*`` is the
ResNet body without ``fc``, built with ``replace_stride_with_dilation=(False, True, True)`` -- layer3 and layer4 run at
layer2's resolution with dilations 2 and 4 (``dilated_residual_block`` / ``dilated_proj_block``) -- and
``classifier.*`` is the FCN head: a 3x3 2048 -> 512 with BN and ReLU (the Winograd layer), dropout (identity at
inference) and a 1x1 512 -> classes with bias.  ``aux_classifier.*`` keys are accepted and ignored.

``model(x_nchw)`` returns ``{"out": [N][classes][H][W]}``.  The forward is the body's chain of launches, a torch
``copy_`` of layer4's output into a pre-zeroed padded tensor, the two head layers, and torch's bilinear
``F.interpolate`` back to the input size (the resize is torch plumbing, not a kernel of this library).  After
``prepare(N, H, W)`` a whole forward can be captured in one ``torch.cuda.graph``.

``DeepLabV3.from_state_dict(sd, arch)`` is the same body with the DeepLabV3 head: ASPP with rates 12, 24, 36 (``aspp``:
the concatenation and the broadcast pooled branch never exist), a 3x3 256 -> 256 with BN and ReLU (the Winograd layer)
and the 1x1 to the classes; both dropouts are the identity at inference.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import (A_PADDED, WinoError, aspp, aspp_prepare, aspp_workspace_bytes, conv1x1_bn_ex, conv1x1_prepare,
               conv3x3_bn_relu, conv3x3_prepare, filter_pack_s2, filter_transform_f2)
from ._net import BN_KEYS, Net, check_state_dict
from .resnet import ResNet, expected_keys, stage_shapes

ARCHS = ("resnet50", "resnet101")
DILATE = (False, True, True)
HEAD_C = 512   # FCNHead: in_channels // 4


def expected_fcn_keys(arch: str, classes: int):
    """{key: shape} of a torchvision fcn_resnet* state dict without its aux_classifier (num_batches_tracked aside)."""
    if arch not in ARCHS:
        raise WinoError(f"unknown arch {arch!r}: one of {sorted(ARCHS)}")
    exp = {f"backbone.{k}": v for k, v in expected_keys(arch, None).items()}
    exp["classifier.0.weight"] = (HEAD_C, 2048, 3, 3)
    for k in BN_KEYS:
        exp[f"classifier.1.{k}"] = (HEAD_C,)
    exp["classifier.4.weight"] = (classes, HEAD_C, 1, 1)
    exp["classifier.4.bias"] = (classes,)
    return exp


def validate_fcn_state_dict(sd, arch: str) -> int:
    """Checks every key and shape of `sd` against `arch` on the host (aux_classifier.* keys are skipped); returns the
    class count.  Raises WinoError naming the first missing, unexpected or wrongly shaped key."""
    if "classifier.4.weight" not in sd:
        raise WinoError("state dict: missing key 'classifier.4.weight'")
    classes = int(sd["classifier.4.weight"].shape[0])
    main = {k: v for k, v in sd.items() if not k.startswith("aux_classifier.")}
    check_state_dict(main, expected_fcn_keys(arch, classes), f"fcn_{arch}", "weight")
    return classes


class FCN(Net):
    """A torchvision FCN-ResNet on the library's kernels, inference only (BN folded at load)."""

    def __init__(self, arch: str, classes: int, device):
        super().__init__(device)
        self.arch, self.classes = arch, int(classes)
        self.body = ResNet(arch, 0, device, DILATE)   # headless: only its _pack_body / _prepare_body / _run_body are used

    @classmethod
    def from_state_dict(cls, sd, arch: str, eps: float = 1e-5, device=None) -> "FCN":
        """Validate `sd` (torchvision's fcn_resnet* key names) for `arch`, fold every BN and pack every filter on
        `device` (default: the current CUDA device)."""
        return cls._load(sd, eps, device, arch, validate_fcn_state_dict(sd, arch))

    def _pack(self, sd, eps):
        self.body._pack_body(sd, eps, "backbone.")
        self.head_U = filter_transform_f2(self._t(sd["classifier.0.weight"]))
        self.head_bn = self._fold_bn(sd, "classifier.1", eps)
        # the 1x1 512 -> classes: [Cin][Kout] with the columns padded to a multiple of 64 (zero weights and biases)
        kp = (self.classes + 63) // 64 * 64
        w = sd["classifier.4.weight"]
        self.cls_w = torch.zeros((HEAD_C, kp), dtype=torch.float32, device=self.device)
        self.cls_w[:, : self.classes] = self._t(w.reshape(w.shape[0], w.shape[1]).t())
        self.cls_bias = torch.zeros(kp, dtype=torch.float32, device=self.device)
        self.cls_bias[: self.classes] = self._t(sd["classifier.4.bias"])
        self.cls_ones = torch.ones(kp, dtype=torch.float32, device=self.device)
        torch.cuda.current_stream().synchronize()

    def prepare(self, N: int, H: int, W: int) -> None:
        """Allocate the body's activations and the head's tensors for [N][3][H][W] inputs and reserve the stream
        scratch of every launch on the current stream.  Call it before capturing a forward into a graph."""
        N, H, W = int(N), int(H), int(W)
        dev, f32, body = self.device, torch.float32, self.body
        with torch.cuda.device(dev):
            ws = body._prepare_body(N, H, W)
            body._ws = torch.empty((ws + 3) // 4, dtype=f32, device=dev)
            _, c, h, w = stage_shapes(self.arch, H, W, DILATE)[-1]
            kp = int(self.cls_w.shape[1])
            self._feat = torch.zeros((N, h + 2, w + 2, c), dtype=f32, device=dev)   # layer4's output, padded; the ring stays 0
            self._mid = torch.zeros((N, h + 2, w + 2, HEAD_C), dtype=f32, device=dev)
            self._scores = torch.zeros((N, h, w, kp), dtype=f32, device=dev)
            conv3x3_prepare(N, c, HEAD_C, h, w)
            conv1x1_prepare(N * h * w, HEAD_C, kp)
        self._shape = (N, H, W)

    def forward(self, x: torch.Tensor):
        """x [N][3][H][W] float32 on the model's device -> {"out": [N][classes][H][W]} (a new tensor of torch's).  A
        new input shape re-runs prepare()."""
        self._begin(x)
        with torch.cuda.device(self.device):
            top = self.body._run_body(x.contiguous())[-1]
            self._feat[:, 1:-1, 1:-1, :].copy_(top)
            conv3x3_bn_relu(self._feat, self.head_U, *self.head_bn, relu=True, out=self._mid)
            conv1x1_bn_ex(self._mid, self.cls_w, self.cls_bias, self.cls_ones, A_PADDED, out=self._scores)
            scores = self._scores[..., : self.classes].permute(0, 3, 1, 2)
            out = F.interpolate(scores, size=(int(x.shape[2]), int(x.shape[3])), mode="bilinear", align_corners=False)
        return {"out": out}


ASPP_RATES = (12, 24, 36)
ASPP_C = 256   # torchvision's ASPP: every branch, the projection and the head's 3x3


def expected_deeplabv3_keys(arch: str, classes: int):
    """{key: shape} of a torchvision deeplabv3_resnet* state dict without its aux_classifier (num_batches_tracked
    aside)."""
    if arch not in ARCHS:
        raise WinoError(f"unknown arch {arch!r}: one of {sorted(ARCHS)}")
    exp = {f"backbone.{k}": v for k, v in expected_keys(arch, None).items()}

    def conv_bn(conv, bn, shape):
        exp[f"{conv}.weight"] = shape
        for k in BN_KEYS:
            exp[f"{bn}.{k}"] = (shape[0],)

    conv_bn("classifier.0.convs.0.0", "classifier.0.convs.0.1", (ASPP_C, 2048, 1, 1))
    for i in (1, 2, 3):
        conv_bn(f"classifier.0.convs.{i}.0", f"classifier.0.convs.{i}.1", (ASPP_C, 2048, 3, 3))
    conv_bn("classifier.0.convs.4.1", "classifier.0.convs.4.2", (ASPP_C, 2048, 1, 1))
    conv_bn("classifier.0.project.0", "classifier.0.project.1", (ASPP_C, 5 * ASPP_C, 1, 1))
    conv_bn("classifier.1", "classifier.2", (ASPP_C, ASPP_C, 3, 3))
    exp["classifier.4.weight"] = (classes, ASPP_C, 1, 1)
    exp["classifier.4.bias"] = (classes,)
    return exp


def validate_deeplabv3_state_dict(sd, arch: str) -> int:
    """Checks every key and shape of `sd` against `arch` on the host (aux_classifier.* keys are skipped); returns the
    class count.  Raises WinoError naming the first missing, unexpected or wrongly shaped key."""
    if "classifier.4.weight" not in sd:
        raise WinoError("state dict: missing key 'classifier.4.weight'")
    classes = int(sd["classifier.4.weight"].shape[0])
    main = {k: v for k, v in sd.items() if not k.startswith("aux_classifier.")}
    check_state_dict(main, expected_deeplabv3_keys(arch, classes), f"deeplabv3_{arch}", "weight")
    return classes


class DeepLabV3(Net):
    """A torchvision DeepLabV3-ResNet on the library's kernels, inference only (BN folded at load)."""

    def __init__(self, arch: str, classes: int, device):
        super().__init__(device)
        self.arch, self.classes = arch, int(classes)
        self.body = ResNet(arch, 0, device, DILATE)   # headless, as FCN's

    @classmethod
    def from_state_dict(cls, sd, arch: str, eps: float = 1e-5, device=None) -> "DeepLabV3":
        """Validate `sd` (torchvision's deeplabv3_resnet* key names) for `arch`, fold every BN and pack every filter on
        `device` (default: the current CUDA device)."""
        return cls._load(sd, eps, device, arch, validate_deeplabv3_state_dict(sd, arch))

    def _pack(self, sd, eps):
        self.body._pack_body(sd, eps, "backbone.")
        mat = lambda k: self._t(sd[k].reshape(sd[k].shape[0], sd[k].shape[1]).t())   # [K][C][1][1] -> [C][K]
        a = "classifier.0."
        self.w0, self.bn0 = mat(a + "convs.0.0.weight"), self._fold_bn(sd, a + "convs.0.1", eps)
        self.taps = [filter_pack_s2(self._t(sd[a + f"convs.{i}.0.weight"])) for i in (1, 2, 3)]
        self.bn_taps = [self._fold_bn(sd, a + f"convs.{i}.1", eps) for i in (1, 2, 3)]
        self.w_pool, self.bn_pool = mat(a + "convs.4.1.weight"), self._fold_bn(sd, a + "convs.4.2", eps)
        self.w_proj, self.bn_proj = mat(a + "project.0.weight"), self._fold_bn(sd, a + "project.1", eps)
        self.head_U = filter_transform_f2(self._t(sd["classifier.1.weight"]))
        self.head_bn = self._fold_bn(sd, "classifier.2", eps)
        # the 1x1 256 -> classes: [Cin][Kout] with the columns padded to a multiple of 64 (zero weights and biases)
        kp = (self.classes + 63) // 64 * 64
        w = sd["classifier.4.weight"]
        self.cls_w = torch.zeros((ASPP_C, kp), dtype=torch.float32, device=self.device)
        self.cls_w[:, : self.classes] = self._t(w.reshape(w.shape[0], w.shape[1]).t())
        self.cls_bias = torch.zeros(kp, dtype=torch.float32, device=self.device)
        self.cls_bias[: self.classes] = self._t(sd["classifier.4.bias"])
        self.cls_ones = torch.ones(kp, dtype=torch.float32, device=self.device)
        torch.cuda.current_stream().synchronize()

    def prepare(self, N: int, H: int, W: int) -> None:
        """Allocate the body's activations and the head's tensors for [N][3][H][W] inputs and reserve the stream
        scratch of every launch on the current stream.  Call it before capturing a forward into a graph."""
        N, H, W = int(N), int(H), int(W)
        dev, f32, body = self.device, torch.float32, self.body
        with torch.cuda.device(dev):
            ws = body._prepare_body(N, H, W)
            body._ws = torch.empty((ws + 3) // 4, dtype=f32, device=dev)
            _, c, h, w = stage_shapes(self.arch, H, W, DILATE)[-1]
            kp = int(self.cls_w.shape[1])
            self._feat = torch.zeros((N, h + 2, w + 2, c), dtype=f32, device=dev)   # layer4's output, padded; the ring stays 0
            self._aspp_ws = torch.empty((aspp_workspace_bytes(N, h, w, c, ASPP_C, ASPP_C) + 3) // 4, dtype=f32, device=dev)
            self._pyr = torch.zeros((N, h + 2, w + 2, ASPP_C), dtype=f32, device=dev)
            self._mid = torch.zeros((N, h + 2, w + 2, ASPP_C), dtype=f32, device=dev)
            self._scores = torch.zeros((N, h, w, kp), dtype=f32, device=dev)
            aspp_prepare(N, h, w, c, ASPP_C, ASPP_C, ASPP_RATES)
            conv3x3_prepare(N, ASPP_C, ASPP_C, h, w)
            conv1x1_prepare(N * h * w, ASPP_C, kp)
        self._shape = (N, H, W)

    def forward(self, x: torch.Tensor):
        """x [N][3][H][W] float32 on the model's device -> {"out": [N][classes][H][W]} (a new tensor of torch's).  A
        new input shape re-runs prepare()."""
        self._begin(x)
        with torch.cuda.device(self.device):
            top = self.body._run_body(x.contiguous())[-1]
            self._feat[:, 1:-1, 1:-1, :].copy_(top)
            aspp(self._feat, self.w0, self.bn0, self.taps, self.bn_taps, ASPP_RATES, self.w_pool, self.bn_pool,
                 self.w_proj, self.bn_proj, out=self._pyr, workspace=self._aspp_ws)
            conv3x3_bn_relu(self._pyr, self.head_U, *self.head_bn, relu=True, out=self._mid)
            conv1x1_bn_ex(self._mid, self.cls_w, self.cls_bias, self.cls_ones, A_PADDED, out=self._scores)
            scores = self._scores[..., : self.classes].permute(0, 3, 1, 2)
            out = F.interpolate(scores, size=(int(x.shape[2]), int(x.shape[3])), mode="bilinear", align_corners=False)
        return {"out": out}


__all__ = ["FCN", "DeepLabV3", "expected_fcn_keys", "validate_fcn_state_dict", "expected_deeplabv3_keys",
           "validate_deeplabv3_state_dict"]
