"""torchvision's FCN-ResNet50 / -101 and DeepLabV3-ResNet50 / -101 (``torchvision.models.segmentation.fcn_resnet*``,
``deeplabv3_resnet*``) on the library's kernels.

``FCN.from_state_dict(sd, arch)`` takes the segmentation model's state dict (its key names): ``backbone.*`` is the
ResNet body without ``fc``, built with ``replace_stride_with_dilation=(False, True, True)`` -- layer3 and layer4 run at
layer2's resolution with dilations 2 and 4 (``dilated_residual_block`` / ``dilated_proj_block``) -- and
``classifier.*`` is the FCN head: a 3x3 2048 -> 512 with BN and ReLU (the Winograd layer), dropout (identity at
inference) and a 1x1 512 -> classes with bias.  ``aux_classifier.*`` keys are accepted and ignored unless the model is
loaded with ``aux=True``: then they are validated and packed as torchvision's ``FCNHead(1024, classes)`` on layer3's
output (a 3x3 1024 -> 256 with BN and ReLU, the 1x1 to the classes).

``model(x_nchw)`` returns ``{"out": [N][classes][H][W]}``.  The forward is the body's chain of launches, a torch
``copy_`` of layer4's output into a pre-zeroed padded tensor, the two head layers, and the bilinear resize back to the
input size: by default torch's ``F.interpolate`` (a new tensor), with ``resize="kernel"`` the library's
``resize_bilinear`` into a buffer of the model's that the next forward overwrites.  ``labels=True`` adds ``"labels"``
(int32 ``[N][H][W]``, the argmax over the classes, from the same launch) and implies the kernel; with it ``out=False``
skips the score tensor, so that only the label map is written.  ``aux=True`` adds ``"aux"``.  After ``prepare(N, H, W)``
a whole forward, with any of these options, can be captured in one ``torch.cuda.graph``.

``DeepLabV3.from_state_dict(sd, arch)`` is the same body with the DeepLabV3 head: ASPP with rates 12, 24, 36 (``aspp``:
the concatenation and the broadcast pooled branch never exist), a 3x3 256 -> 256 with BN and ReLU (the Winograd layer)
and the 1x1 to the classes; both dropouts are the identity at inference.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import (A_PADDED, WinoError, aspp, aspp_prepare, aspp_workspace_bytes, conv1x1_bn_ex, conv1x1_prepare,
               conv3x3_bn_relu, conv3x3_prepare, filter_pack_s2, filter_transform_f2, resize_bilinear)
from ._net import BN_KEYS, Net, check_state_dict
from .resnet import ResNet, expected_keys, stage_shapes

ARCHS = ("resnet50", "resnet101")
DILATE = (False, True, True)
HEAD_C = 512   # FCNHead: in_channels // 4
AUX_IN, AUX_C = 1024, 256   # the aux head: FCNHead(1024, classes) on layer3's output


def _aux_keys(classes: int):
    """{key: shape} of torchvision's aux_classifier, FCNHead(1024, classes)."""
    exp = {"aux_classifier.0.weight": (AUX_C, AUX_IN, 3, 3)}
    for k in BN_KEYS:
        exp[f"aux_classifier.1.{k}"] = (AUX_C,)
    exp["aux_classifier.4.weight"] = (classes, AUX_C, 1, 1)
    exp["aux_classifier.4.bias"] = (classes,)
    return exp


def _validate(sd, exp_keys, arch: str, name: str, aux: bool) -> int:
    """The two validators' body: the class count read off classifier.4.weight, then every key and shape."""
    if "classifier.4.weight" not in sd:
        raise WinoError("state dict: missing key 'classifier.4.weight'")
    classes = int(sd["classifier.4.weight"].shape[0])
    main = sd if aux else {k: v for k, v in sd.items() if not k.startswith("aux_classifier.")}
    check_state_dict(main, exp_keys(arch, classes, aux=aux), f"{name}_{arch}", "weight")
    return classes


class _SegNet(Net):
    """What FCN and DeepLabV3 share: the dilated body, the 1x1 to the classes, the aux head and the output stage."""

    def __init__(self, arch: str, classes: int, device, aux: bool = False):
        super().__init__(device)
        self.arch, self.classes, self.has_aux = arch, int(classes), bool(aux)
        self.body = ResNet(arch, 0, device, DILATE)   # headless: only its _pack_body / _prepare_body / _run_body are used

    def _pack_cls(self, sd, prefix: str, cin: int):
        """The 1x1 cin -> classes at sd[prefix.*]: [Cin][Kout] with the columns padded to a multiple of 64 (zero weights
        and biases); returns (w, bias)."""
        kp = (self.classes + 63) // 64 * 64
        w = sd[f"{prefix}.weight"]
        cw = torch.zeros((cin, kp), dtype=torch.float32, device=self.device)
        cw[:, : self.classes] = self._t(w.reshape(w.shape[0], w.shape[1]).t())
        bias = torch.zeros(kp, dtype=torch.float32, device=self.device)
        bias[: self.classes] = self._t(sd[f"{prefix}.bias"])
        return cw, bias

    def _pack_aux(self, sd, eps):
        if not self.has_aux:
            return
        self.aux_U = filter_transform_f2(self._t(sd["aux_classifier.0.weight"]))
        self.aux_bn = self._fold_bn(sd, "aux_classifier.1", eps)
        self.aux_w, self.aux_bias = self._pack_cls(sd, "aux_classifier.4", AUX_C)

    def _prepare_outputs(self, N: int, H: int, W: int) -> None:
        """The kernel path's output tensors and the aux head's activations (inside prepare's device context)."""
        dev, f32 = self.device, torch.float32
        kp = int(self.cls_w.shape[1])
        self._out = torch.empty((N, self.classes, H, W), dtype=f32, device=dev)
        self._labels = torch.empty((N, H, W), dtype=torch.int32, device=dev)
        if self.has_aux:
            _, c, h, w = stage_shapes(self.arch, H, W, DILATE)[-2]
            self._aux_feat = torch.zeros((N, h + 2, w + 2, c), dtype=f32, device=dev)   # layer3's output, padded; the ring stays 0
            self._aux_mid = torch.zeros((N, h + 2, w + 2, AUX_C), dtype=f32, device=dev)
            self._aux_scores = torch.zeros((N, h, w, kp), dtype=f32, device=dev)
            self._aux_out = torch.empty((N, self.classes, H, W), dtype=f32, device=dev)
            conv3x3_prepare(N, c, AUX_C, h, w)
            conv1x1_prepare(N * h * w, AUX_C, kp)

    def _options(self, resize, labels, aux, out):
        """forward's keyword options checked; returns whether the resize is the library's."""
        if resize not in ("torch", "kernel"):
            raise WinoError(f"resize must be 'torch' or 'kernel', got {resize!r}")
        if not out and not labels:
            raise WinoError("out=False needs labels=True")
        if aux and not self.has_aux:
            raise WinoError("forward(aux=True) needs a model loaded with from_state_dict(..., aux=True)")
        return resize == "kernel" or bool(labels)

    def _finish(self, x, stages, kernel: bool, labels: bool, aux: bool, out: bool):
        """The output stage: self._scores (and, with aux, the aux head on layer3's output) resized to x's size."""
        size = (int(x.shape[2]), int(x.shape[3]))
        res = {}
        if kernel:
            o, lab = resize_bilinear(self._scores, *size, C=self.classes, out=self._out if out else None,
                                     labels=self._labels if labels else None, want_out=False)
            if out:
                res["out"] = o
            if labels:
                res["labels"] = lab
        else:
            scores = self._scores[..., : self.classes].permute(0, 3, 1, 2)
            res["out"] = F.interpolate(scores, size=size, mode="bilinear", align_corners=False)
        if aux:
            self._aux_feat[:, 1:-1, 1:-1, :].copy_(stages[-2])
            conv3x3_bn_relu(self._aux_feat, self.aux_U, *self.aux_bn, relu=True, out=self._aux_mid)
            conv1x1_bn_ex(self._aux_mid, self.aux_w, self.aux_bias, self.cls_ones, A_PADDED, out=self._aux_scores)
            if kernel:
                res["aux"] = resize_bilinear(self._aux_scores, *size, C=self.classes, out=self._aux_out)[0]
            else:
                scores = self._aux_scores[..., : self.classes].permute(0, 3, 1, 2)
                res["aux"] = F.interpolate(scores, size=size, mode="bilinear", align_corners=False)
        return res


def expected_fcn_keys(arch: str, classes: int, aux: bool = False):
    """{key: shape} of a torchvision fcn_resnet* state dict (num_batches_tracked aside), without its aux_classifier
    unless `aux`."""
    if arch not in ARCHS:
        raise WinoError(f"unknown arch {arch!r}: one of {sorted(ARCHS)}")
    exp = {f"backbone.{k}": v for k, v in expected_keys(arch, None).items()}
    exp["classifier.0.weight"] = (HEAD_C, 2048, 3, 3)
    for k in BN_KEYS:
        exp[f"classifier.1.{k}"] = (HEAD_C,)
    exp["classifier.4.weight"] = (classes, HEAD_C, 1, 1)
    exp["classifier.4.bias"] = (classes,)
    if aux:
        exp.update(_aux_keys(classes))
    return exp


def validate_fcn_state_dict(sd, arch: str, aux: bool = False) -> int:
    """Checks every key and shape of `sd` against `arch` on the host (aux_classifier.* keys are skipped unless `aux`:
    then they are checked like the rest); returns the class count.  Raises WinoError naming the first missing,
    unexpected or wrongly shaped key."""
    return _validate(sd, expected_fcn_keys, arch, "fcn", aux)


class FCN(_SegNet):
    """A torchvision FCN-ResNet on the library's kernels, inference only (BN folded at load)."""

    @classmethod
    def from_state_dict(cls, sd, arch: str, eps: float = 1e-5, device=None, aux: bool = False) -> "FCN":
        """Validate `sd` (torchvision's fcn_resnet* key names) for `arch`, fold every BN and pack every filter on
        `device` (default: the current CUDA device).  With `aux` the aux_classifier is validated and packed too."""
        return cls._load(sd, eps, device, arch, validate_fcn_state_dict(sd, arch, aux), aux=aux)

    def _pack(self, sd, eps):
        self.body._pack_body(sd, eps, "backbone.")
        self.head_U = filter_transform_f2(self._t(sd["classifier.0.weight"]))
        self.head_bn = self._fold_bn(sd, "classifier.1", eps)
        self.cls_w, self.cls_bias = self._pack_cls(sd, "classifier.4", HEAD_C)
        self.cls_ones = torch.ones(int(self.cls_w.shape[1]), dtype=torch.float32, device=self.device)
        self._pack_aux(sd, eps)
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
            self._prepare_outputs(N, H, W)
        self._shape = (N, H, W)

    def forward(self, x: torch.Tensor, *, resize: str = "torch", labels: bool = False, aux: bool = False,
                out: bool = True):
        """x [N][3][H][W] float32 on the model's device -> {"out": [N][classes][H][W]}: a new tensor of torch's, or with
        resize="kernel" the model's own buffer, overwritten by the next forward.  labels=True adds "labels" (int32
        [N][H][W]) and implies the kernel; out=False (with labels) leaves "out" unwritten and out of the result;
        aux=True adds "aux" (a model loaded with aux=True).  A new input shape re-runs prepare()."""
        kernel = self._options(resize, labels, aux, out)
        self._begin(x)
        with torch.cuda.device(self.device):
            stages = self.body._run_body(x.contiguous())
            self._feat[:, 1:-1, 1:-1, :].copy_(stages[-1])
            conv3x3_bn_relu(self._feat, self.head_U, *self.head_bn, relu=True, out=self._mid)
            conv1x1_bn_ex(self._mid, self.cls_w, self.cls_bias, self.cls_ones, A_PADDED, out=self._scores)
            return self._finish(x, stages, kernel, bool(labels), bool(aux), bool(out))


ASPP_RATES = (12, 24, 36)
ASPP_C = 256   # torchvision's ASPP: every branch, the projection and the head's 3x3


def expected_deeplabv3_keys(arch: str, classes: int, aux: bool = False):
    """{key: shape} of a torchvision deeplabv3_resnet* state dict (num_batches_tracked aside), without its
    aux_classifier unless `aux`."""
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
    if aux:
        exp.update(_aux_keys(classes))
    return exp


def validate_deeplabv3_state_dict(sd, arch: str, aux: bool = False) -> int:
    """Checks every key and shape of `sd` against `arch` on the host (aux_classifier.* keys are skipped unless `aux`:
    then they are checked like the rest); returns the class count.  Raises WinoError naming the first missing,
    unexpected or wrongly shaped key."""
    return _validate(sd, expected_deeplabv3_keys, arch, "deeplabv3", aux)


class DeepLabV3(_SegNet):
    """A torchvision DeepLabV3-ResNet on the library's kernels, inference only (BN folded at load)."""

    @classmethod
    def from_state_dict(cls, sd, arch: str, eps: float = 1e-5, device=None, aux: bool = False) -> "DeepLabV3":
        """Validate `sd` (torchvision's deeplabv3_resnet* key names) for `arch`, fold every BN and pack every filter on
        `device` (default: the current CUDA device).  With `aux` the aux_classifier is validated and packed too."""
        return cls._load(sd, eps, device, arch, validate_deeplabv3_state_dict(sd, arch, aux), aux=aux)

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
        self.cls_w, self.cls_bias = self._pack_cls(sd, "classifier.4", ASPP_C)
        self.cls_ones = torch.ones(int(self.cls_w.shape[1]), dtype=torch.float32, device=self.device)
        self._pack_aux(sd, eps)
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
            self._prepare_outputs(N, H, W)
        self._shape = (N, H, W)

    def forward(self, x: torch.Tensor, *, resize: str = "torch", labels: bool = False, aux: bool = False,
                out: bool = True):
        """x [N][3][H][W] float32 on the model's device -> {"out": [N][classes][H][W]}: a new tensor of torch's, or with
        resize="kernel" the model's own buffer, overwritten by the next forward.  labels=True adds "labels" (int32
        [N][H][W]) and implies the kernel; out=False (with labels) leaves "out" unwritten and out of the result;
        aux=True adds "aux" (a model loaded with aux=True).  A new input shape re-runs prepare()."""
        kernel = self._options(resize, labels, aux, out)
        self._begin(x)
        with torch.cuda.device(self.device):
            stages = self.body._run_body(x.contiguous())
            self._feat[:, 1:-1, 1:-1, :].copy_(stages[-1])
            aspp(self._feat, self.w0, self.bn0, self.taps, self.bn_taps, ASPP_RATES, self.w_pool, self.bn_pool,
                 self.w_proj, self.bn_proj, out=self._pyr, workspace=self._aspp_ws)
            conv3x3_bn_relu(self._pyr, self.head_U, *self.head_bn, relu=True, out=self._mid)
            conv1x1_bn_ex(self._mid, self.cls_w, self.cls_bias, self.cls_ones, A_PADDED, out=self._scores)
            return self._finish(x, stages, kernel, bool(labels), bool(aux), bool(out))


__all__ = ["FCN", "DeepLabV3", "expected_fcn_keys", "validate_fcn_state_dict", "expected_deeplabv3_keys",
           "validate_deeplabv3_state_dict"]
