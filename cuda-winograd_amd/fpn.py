"""torchvision's ResNet-FPN backbones (``BackboneWithFPN`` / ``resnet_fpn_backbone``: the backbones of Faster / Mask /
Keypoint R-CNN and RetinaNet) on the library's kernels: a headless ResNet body and a Feature Pyramid Network on its
four stage outputs.

``ResNetFPN.from_state_dict(sd, arch)`` takes the backbone's state dict under torchvision's key names --
``body.<resnet keys>`` without ``fc``, ``fpn.inner_blocks.{i}.0.weight|bias`` (the 1x1 laterals) and
``fpn.layer_blocks.{i}.0.weight|bias`` (the 3x3 output convolutions), i = 0..3 -- for every arch of ``resnet.ARCHS``.
``model(x_nchw)`` returns {"0", "1", "2", "3", "pool"}.

``returned_layers`` and ``extra_blocks`` are torchvision's: the ResNet stages (1..4, ascending and consecutive) whose
outputs feed the pyramid, numbered "0".. in that order, and what follows the coarsest level: ``"pool"``
(``LastLevelMaxPool``) or ``"p6p7"`` (``LastLevelP6P7(out_channels, out_channels)``: keys
``fpn.extra_blocks.p6|p7.weight|bias``, P6 = conv3x3 stride 2 of P5, P7 = conv3x3 stride 2 of relu(P6), returned as
"p6" and "p7").  ``returned_layers=(2, 3, 4), extra_blocks="p6p7"`` is ``retinanet_resnet50_fpn``'s backbone; the
defaults are the R-CNNs'.  P6 from C5 (``LastLevelP6P7(2048, 256)``, the v2 model) is not built.

The pyramid runs from the coarsest level down, one ``fpn_level`` (two launches) per level: the lateral 1x1 adds the
coarser level's ``inner`` in its epilogue, read at (y >> 1, x >> 1) -- ``F.interpolate(mode="nearest")`` for the size
pairs a stride-2 stage makes -- so no upsampled tensor is ever written; the 3x3 is the Winograd layer.  ``"pool"`` is
torchvision's ``LastLevelMaxPool``, ``max_pool2d(kernel 1, stride 2)``: the view ``P3[:, ::2, ::2, :]``, no kernel.
"""
from __future__ import annotations

import torch

from . import WinoError, conv3x3_s2_bn_relu, conv3x3_s2_prepare, filter_pack_s2, filter_transform_f2, fpn_level
from . import fpn_level_prepare
from ._net import Net, check_state_dict
from .resnet import ARCHS, ResNet, expected_keys, stage_shapes

LEVELS = 4
RETURNED_LAYERS = (1, 2, 3, 4)
EXTRA_BLOCKS = ("pool", "p6p7")


def _check_layers(returned_layers, extra_blocks):
    """returned_layers as a tuple of ints: ascending, consecutive stages of 1..4; extra_blocks one of EXTRA_BLOCKS."""
    layers = tuple(int(v) for v in returned_layers)
    if not layers or layers != tuple(range(layers[0], layers[0] + len(layers))) or layers[0] < 1 or layers[-1] > LEVELS:
        raise WinoError(f"returned_layers={returned_layers!r}: consecutive ResNet stages out of 1..{LEVELS}, ascending")
    if extra_blocks not in EXTRA_BLOCKS:
        raise WinoError(f"extra_blocks must be one of {EXTRA_BLOCKS}, got {extra_blocks!r}")
    return layers


def expected_fpn_keys(arch: str, out_channels: int, returned_layers=RETURNED_LAYERS, extra_blocks: str = "pool"):
    """{key: shape} of a torchvision BackboneWithFPN state dict of `arch` (num_batches_tracked aside)."""
    layers = _check_layers(returned_layers, extra_blocks)
    exp = {f"body.{k}": v for k, v in expected_keys(arch, None).items()}
    stage_c = [c for _, c, _, _ in stage_shapes(arch, 64, 64)[1:]]
    for i, layer in enumerate(layers):
        exp[f"fpn.inner_blocks.{i}.0.weight"] = (out_channels, stage_c[layer - 1], 1, 1)
        exp[f"fpn.inner_blocks.{i}.0.bias"] = (out_channels,)
        exp[f"fpn.layer_blocks.{i}.0.weight"] = (out_channels, out_channels, 3, 3)
        exp[f"fpn.layer_blocks.{i}.0.bias"] = (out_channels,)
    if extra_blocks == "p6p7":
        for name in ("p6", "p7"):
            exp[f"fpn.extra_blocks.{name}.weight"] = (out_channels, out_channels, 3, 3)
            exp[f"fpn.extra_blocks.{name}.bias"] = (out_channels,)
    return exp


def validate_fpn_state_dict(sd, arch: str, out_channels: int = 256, returned_layers=RETURNED_LAYERS,
                            extra_blocks: str = "pool") -> None:
    """Checks every key and shape of `sd` against `arch` with an FPN of `out_channels` on the host.  Raises WinoError
    naming the first missing, unexpected or wrongly shaped key."""
    if arch not in ARCHS:
        raise WinoError(f"unknown arch {arch!r}: one of {sorted(ARCHS)}")
    out_channels = int(out_channels)
    if out_channels < 64 or out_channels % 64:
        raise WinoError(f"out_channels={out_channels}: the FPN's layers need a multiple of 64")
    check_state_dict(sd, expected_fpn_keys(arch, out_channels, returned_layers, extra_blocks), f"{arch} + FPN", "weight")


class ResNetFPN(Net):
    """A torchvision ResNet-FPN backbone on the library's kernels, inference only (BN folded at load)."""

    def __init__(self, arch: str, out_channels: int, device, returned_layers=RETURNED_LAYERS, extra_blocks: str = "pool"):
        super().__init__(device)
        self.arch, self.out_channels = arch, int(out_channels)
        self.layers, self.extra_blocks = _check_layers(returned_layers, extra_blocks), extra_blocks
        self.body = ResNet(arch, 0, device)   # headless: only its _pack_body / _prepare_body / _run_body are used

    @classmethod
    def from_state_dict(cls, sd, arch: str, out_channels: int = 256, eps: float = 1e-5, device=None,
                        returned_layers=RETURNED_LAYERS, extra_blocks: str = "pool") -> "ResNetFPN":
        """Validate `sd` (torchvision's BackboneWithFPN key names) for `arch`, fold every BN and pack every filter on
        `device` (default: the current CUDA device).  returned_layers, extra_blocks: see the module docstring."""
        validate_fpn_state_dict(sd, arch, out_channels, returned_layers, extra_blocks)
        return cls._load(sd, eps, device, arch, out_channels, returned_layers=returned_layers, extra_blocks=extra_blocks)

    def _pack(self, sd, eps):
        self.body._pack_body(sd, eps, "body.")
        self.levels = []   # per level, finest first: (lateral [Cin][Cf], its bias, U of the 3x3, its bias)
        for i in range(len(self.layers)):
            wl = sd[f"fpn.inner_blocks.{i}.0.weight"]
            self.levels.append((self._t(wl.reshape(wl.shape[0], wl.shape[1]).t()),
                                self._t(sd[f"fpn.inner_blocks.{i}.0.bias"]),
                                filter_transform_f2(self._t(sd[f"fpn.layer_blocks.{i}.0.weight"])),
                                self._t(sd[f"fpn.layer_blocks.{i}.0.bias"])))
        # LastLevelP6P7: the stride-2 3x3 layer's filters and the biases, P6 then P7
        self.extra = [(filter_pack_s2(self._t(sd[f"fpn.extra_blocks.{name}.weight"])),
                       self._t(sd[f"fpn.extra_blocks.{name}.bias"])) for name in ("p6", "p7")] \
            if self.extra_blocks == "p6p7" else []
        self._ones = torch.ones(self.out_channels, dtype=torch.float32, device=self.device)
        torch.cuda.current_stream().synchronize()

    def prepare(self, N: int, H: int, W: int) -> None:
        """Allocate the body's activations, the levels' `inner` and `P` tensors (and P6, relu(P6) and P7) for
        [N][3][H][W] inputs and reserve the stream scratch of every launch on the current stream.  Call it before
        capturing a forward into a graph."""
        N, H, W = int(N), int(H), int(W)
        dev, f32, body = self.device, torch.float32, self.body
        with torch.cuda.device(dev):
            ws = body._prepare_body(N, H, W)
            body._ws = torch.empty((ws + 3) // 4, dtype=f32, device=dev)
            self._inner, self._p = [], []
            for _, c, h, w in [stage_shapes(self.arch, H, W)[layer] for layer in self.layers]:
                self._inner.append(torch.zeros((N, h + 2, w + 2, self.out_channels), dtype=f32, device=dev))
                self._p.append(torch.zeros((N, h + 2, w + 2, self.out_channels), dtype=f32, device=dev))
                fpn_level_prepare(N, h, w, c, self.out_channels)
            self._extra = []   # P6, relu(P6), P7: zero rings
            if self.extra:
                Cf = self.out_channels
                h6, w6 = (h - 1) // 2 + 1, (w - 1) // 2 + 1   # (h, w: the coarsest level's)
                h7, w7 = (h6 - 1) // 2 + 1, (w6 - 1) // 2 + 1
                self._extra = [torch.zeros((N, a + 2, b + 2, Cf), dtype=f32, device=dev)
                               for a, b in ((h6, w6), (h6, w6), (h7, w7))]
                conv3x3_s2_prepare(N, h, w, Cf, Cf)
                conv3x3_s2_prepare(N, h6, w6, Cf, Cf)
        self._shape = (N, H, W)

    def forward(self, x: torch.Tensor, padded: bool = False):
        """x [N][3][H][W] float32 on the model's device -> {"0", "1", "2", "3", "pool"}: the pyramid levels P2..P5 at
        strides 4..32 and the pooled P5, each an NHWC view [N][h][w][out_channels] of the model's own tensors, valid
        until the next forward.  A new input shape re-runs prepare().  padded=True returns "0".."3" as the padded
        tensors [N][h+2][w+2][out_channels] themselves (zero ring), what multiscale_roi_align(in_padded=True) reads
        without a copy; "pool" stays the strided view of P5's interior.  With returned_layers / extra_blocks="p6p7" the
        keys are "0".. for the returned stages, then "p6" and "p7" in place of "pool", padded or not like the others.
        P6 is the convolution's output without a ReLU; P7's input relu(P6) is a second launch of the same stride-2
        layer with relu=True into a zero-ring tensor of its own (the layer is small, and the ReLU is then the
        library's NaN-propagating one on every path)."""
        self._begin(x)
        with torch.cuda.device(self.device):
            stages = self.body._run_body(x.contiguous())
            stages, L = [stages[layer - 1] for layer in self.layers], len(self.layers)
            for i in reversed(range(L)):   # top-down: the coarsest level has no `top`
                wl, bl, U, bo = self.levels[i]
                fpn_level(stages[i], wl, bl, U, bo, top=self._inner[i + 1] if i + 1 < L else None,
                          c_padded=not self.body.bottleneck, ones=self._ones, inner=self._inner[i], out=self._p[i])
            if self.extra:
                (w6, b6), (w7, b7) = self.extra
                p6, p6r, p7 = self._extra
                conv3x3_s2_bn_relu(self._p[-1], w6, b6, self._ones, relu=False, out=p6)
                conv3x3_s2_bn_relu(self._p[-1], w6, b6, self._ones, relu=True, out=p6r)
                conv3x3_s2_bn_relu(p6r, w7, b7, self._ones, relu=False, out=p7)
        out = {str(i): p if padded else p[:, 1:-1, 1:-1, :] for i, p in enumerate(self._p)}
        if self.extra:
            out.update(p6=p6 if padded else p6[:, 1:-1, 1:-1, :], p7=p7 if padded else p7[:, 1:-1, 1:-1, :])
        else:
            out["pool"] = self._p[-1][:, 1:-1:2, 1:-1:2, :]
        return out


__all__ = ["ResNetFPN", "expected_fpn_keys", "validate_fpn_state_dict"]
