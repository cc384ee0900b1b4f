"""torchvision's FCN-ResNet50 / -101 (``torchvision.models.segmentation.fcn_resnet*``) on the library's kernels.

``FCN.from_state_dict(sd, arch)`` takes the segmentation model's state dict (its key names): ``backbone.*`` is the
ResNet body without ``fc``, built with ``replace_stride_with_dilation=(False, True, True)`` -- layer3 and layer4 run at
layer2's resolution with dilations 2 and 4 (``dilated_residual_block`` / ``dilated_proj_block``) -- and
``classifier.*`` is the FCN head: a 3x3 2048 -> 512 with BN and ReLU (the Winograd layer), dropout (identity at
inference) and a 1x1 512 -> classes with bias.  ``aux_classifier.*`` keys are accepted and ignored.

``model(x_nchw)`` returns ``{"out": [N][classes][H][W]}``.  The forward is the body's chain of launches, a torch
``copy_`` of layer4's output into a pre-zeroed padded tensor, the two head layers, and torch's bilinear
``F.interpolate`` back to the input size (the resize is torch plumbing, not a kernel of this library).  After
``prepare(N, H, W)`` a whole forward can be captured in one ``torch.cuda.graph``.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import (A_PADDED, WinoError, conv1x1_bn_ex, conv1x1_prepare, conv3x3_bn_relu, conv3x3_prepare,
               filter_transform_f2)
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


__all__ = ["FCN", "expected_fcn_keys", "validate_fcn_state_dict"]
