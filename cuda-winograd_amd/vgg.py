"""Whole torchvision VGGs (11, 13, 16, 19, with and without BN) on the library's kernels.

``VGG.from_state_dict(sd, arch)`` takes a torchvision state dict (its key names), folds every conv bias / BN into a
(bias, scale) pair and packs every filter once; ``model(x_nchw)`` returns the logits.  The forward is a straight chain
of launches on the current stream:

- ``image_pack`` turns the NCHW images into the padded NHWC input of the first 3x3 layer, its 3 channels zero-padded
  to ``CPAD`` = 16 (the first filter is padded the same way before its transform).  16, not 8: the latency kernel
  needs C % 16, so small batches keep their latency form; at large batches the first layer's contraction is two chunk
  iterations instead of one, on a layer that is a few percent of the network.
- every convolution is ``conv3x3_bn_relu`` or, where the configuration has ``'M'`` behind it, ``conv3x3_bn_relu_pool``
  (the max-pool in the Winograd epilogue: the un-pooled activation never exists).  The activations ping-pong between
  two tensors sized for the largest layer.
- ``avgpool7_flatten`` (AdaptiveAvgPool2d(7) + flatten in (h, w, c) order), two ``conv1x1_bn`` GEMMs with M = N for
  the hidden FC layers (scale 1, the FC bias as BN bias, ReLU) and ``avgpool_fc`` at H = W = 1 for the last one.
  ``classifier.0.weight`` is permuted from torch's (c, h, w) column order to (h, w, c) once, at pack time.  Dropout is
  the identity at inference.

``prepare(N, H, W)`` allocates the activations, one workspace and the logits for an input shape and reserves every
launch's stream scratch, so that a whole forward can then be captured in one ``torch.cuda.graph``.
"""
from __future__ import annotations

import torch

from . import (WinoError, avgpool7_flatten, avgpool_fc, conv1x1_bn, conv1x1_prepare, conv3x3_bn_relu,
               conv3x3_bn_relu_pool, conv3x3_prepare, filter_transform_f2, head_pack, head_prepare, image_pack, lib)
from ._net import BN_KEYS, Net, check_state_dict

# torchvision's configurations A, B, D, E
_CFGS = {
    "A": (64, "M", 128, "M", 256, 256, "M", 512, 512, "M", 512, 512, "M"),
    "B": (64, 64, "M", 128, 128, "M", 256, 256, "M", 512, 512, "M", 512, 512, "M"),
    "D": (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"),
    "E": (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M"),
}
# arch -> (configuration, batch norm?)
ARCHS = {
    "vgg11": ("A", False), "vgg13": ("B", False), "vgg16": ("D", False), "vgg19": ("E", False),
    "vgg11_bn": ("A", True), "vgg13_bn": ("B", True), "vgg16_bn": ("D", True), "vgg19_bn": ("E", True),
}
CPAD = 16        # channels of the packed image (see the module docstring)
MIN_HW = 32      # five floors of H/2 must leave a pixel


def _arch(arch: str):
    if arch not in ARCHS:
        raise WinoError(f"unknown arch {arch!r}: one of {sorted(ARCHS)}")
    cfg, bn = ARCHS[arch]
    return _CFGS[cfg], bn


def conv_layers(arch: str):
    """[(features index, Cin, Cout, pooled?)] of the convolutions of `arch`, in order (torchvision's make_layers: a
    conv takes an index, its BN the next one in the _bn forms, then the ReLU; an 'M' takes one)."""
    cfg, bn = _arch(arch)
    layers, i, cin = [], 0, 3
    for j, v in enumerate(cfg):
        if v == "M":
            i += 1
            continue
        layers.append((i, cin, v, j + 1 < len(cfg) and cfg[j + 1] == "M"))
        i += 3 if bn else 2
        cin = v
    return layers


def expected_keys(arch: str, classes: int, hidden: int = 4096):
    """{key: shape} of a torchvision state dict of `arch` (num_batches_tracked aside)."""
    _, bn = _arch(arch)
    exp = {}
    cout = 3
    for i, cin, cout, _ in conv_layers(arch):
        exp[f"features.{i}.weight"] = (cout, cin, 3, 3)
        exp[f"features.{i}.bias"] = (cout,)
        if bn:
            for k in BN_KEYS:
                exp[f"features.{i + 1}.{k}"] = (cout,)
    for idx, (o, c) in zip((0, 3, 6), ((hidden, cout * 49), (hidden, hidden), (classes, hidden))):
        exp[f"classifier.{idx}.weight"] = (o, c)
        exp[f"classifier.{idx}.bias"] = (o,)
    return exp


def validate_state_dict(sd, arch: str):
    """Checks every key and shape of `sd` against `arch` on the host; returns (classes, hidden), both read from the
    state dict.  Raises WinoError naming the first missing, unexpected or wrongly shaped key, or the first FC's
    weight when the hidden width is not a multiple of 64."""
    _arch(arch)
    for k in ("classifier.0.weight", "classifier.6.weight"):
        if k not in sd:
            raise WinoError(f"state dict: missing key {k!r} for {arch}")
        if sd[k].dim() != 2:
            raise WinoError(f"state dict: key {k!r} has shape {tuple(sd[k].shape)}, {arch} needs a matrix")
    hidden, classes = int(sd["classifier.0.weight"].shape[0]), int(sd["classifier.6.weight"].shape[0])
    if hidden < 64 or hidden % 64:
        raise WinoError(f"state dict: key 'classifier.0.weight' gives the hidden width {hidden}: it must be a "
                        "multiple of 64")
    check_state_dict(sd, expected_keys(arch, classes, hidden), arch, "running_mean")
    return classes, hidden


def fc1_columns_hwc(w: torch.Tensor, C: int) -> torch.Tensor:
    """classifier.0.weight [hidden][C*49], columns in torch's flatten order (c, h, w) -> the same matrix with its
    columns in (h, w, c) order, the order avgpool7_flatten writes."""
    hidden = int(w.shape[0])
    return w.reshape(hidden, C, 7, 7).permute(0, 2, 3, 1).reshape(hidden, 49 * C)


def layer_shapes(arch: str, H: int, W: int):
    """[(Cin, Cout, h, w, pooled?)] per convolution for an H x W input: h x w is the layer's INPUT (= conv output) map;
    a pooled layer writes h//2 x w//2."""
    out, h, w = [], H, W
    for _, cin, cout, pool in conv_layers(arch):
        out.append((cin, cout, h, w, pool))
        if pool:
            h, w = h // 2, w // 2
    return out


class VGG(Net):
    """A torchvision VGG on the library's kernels, inference only (conv bias and BN folded at load)."""

    def __init__(self, arch: str, classes: int, hidden: int, device):
        super().__init__(device)
        self.arch, self.classes, self.hidden = arch, classes, hidden
        _, self.bn = _arch(arch)

    # ------------------------------------------------------------------ loading
    @classmethod
    def from_state_dict(cls, sd, arch: str, eps: float = 1e-5, device=None) -> "VGG":
        """Validate `sd` (torchvision key names) for `arch`, fold every conv bias and BN (scale = gamma / sqrt(var +
        eps), bias = beta + (b - mean) * scale; without BN scale = 1, bias = b) and pack every filter on `device`
        (default: the current CUDA device)."""
        return cls._load(sd, eps, device, arch, *validate_state_dict(sd, arch))

    def _pack(self, sd, eps):
        self.convs = []   # (Cin as run, Cout, pooled?, U, bias, scale)
        for i, cin, cout, pool in conv_layers(self.arch):
            w = sd[f"features.{i}.weight"].detach().float()
            if cin < CPAD and cin % 8:   # the first layer: zero channels up to the packed image's
                w = torch.cat([w, w.new_zeros(cout, CPAD - cin, 3, 3)], dim=1)
                cin = CPAD
            b = sd[f"features.{i}.bias"]   # without BN: scale = 1, bias = b
            bias, scale = (self._fold_bn(sd, f"features.{i + 1}", eps, conv_bias=b) if self.bn
                           else (self._t(b), self._t(torch.ones_like(b))))
            self.convs.append((cin, cout, pool, filter_transform_f2(self._t(w)), bias, scale))
        self.feat_c = self.convs[-1][1]
        ones = torch.ones(self.hidden, dtype=torch.float32, device=self.device)
        w0 = fc1_columns_hwc(sd["classifier.0.weight"].detach().float(), self.feat_c)
        self.fc = [(self._t(w0.t()), self._t(sd["classifier.0.bias"]), ones),            # B = W^T [Cin][hidden]
                   (self._t(sd["classifier.3.weight"].detach().float().t()), self._t(sd["classifier.3.bias"]), ones)]
        self.head_packed = head_pack(self._t(sd["classifier.6.weight"]), self._t(sd["classifier.6.bias"]))
        torch.cuda.current_stream().synchronize()

    # ------------------------------------------------------------------ per input shape
    def prepare(self, N: int, H: int, W: int) -> None:
        """Allocate the two ping-pong activation tensors (sized for the largest layer), the workspace and the logits
        for [N][3][H][W] inputs and reserve the stream scratch of every launch on the current stream.  Call it before
        capturing a forward into a graph."""
        N, H, W = int(N), int(H), int(W)
        if N < 1 or H < MIN_HW or W < MIN_HW:
            raise WinoError(f"bad input shape N={N} H={H} W={W}: VGG needs N >= 1 and H, W >= {MIN_HW} "
                            "(five 2x2 pools must leave a pixel)")
        dev, f32 = self.device, torch.float32
        shapes = layer_shapes(self.arch, H, W)
        elems = N * (H + 2) * (W + 2) * CPAD
        with torch.cuda.device(dev):
            for (_, _, h, w, pool), (cin, cout, _, _, _, _) in zip(shapes, self.convs):
                ho, wo = (h // 2, w // 2) if pool else (h, w)
                elems = max(elems, N * (ho + 2) * (wo + 2) * cout)
                conv3x3_prepare(N, cin, cout, h, w)    # the pooled layer takes the plain layer's plan
            elems = max(elems, N * 49 * self.feat_c, N * self.hidden)
            conv1x1_prepare(N, 49 * self.feat_c, self.hidden)
            conv1x1_prepare(N, self.hidden, self.hidden)
            head_prepare(N, self.hidden, self.classes)
            self._act = [torch.zeros(elems, dtype=f32, device=dev) for _ in range(2)]
            ws = lib().wino_head_workspace_bytes(N, self.hidden, self.classes)
            self._ws = torch.empty((ws + 3) // 4, dtype=f32, device=dev)
            self._logits = torch.empty((N, self.classes), dtype=f32, device=dev)
        self._shape = (N, H, W)

    def _view(self, i, *shape):
        n = 1
        for v in shape:
            n *= v
        return self._act[i][:n].view(*shape)

    def _run(self, x, stages):
        N, H, W = self._shape
        cur = 0
        a = image_pack(x, CPAD, out=self._view(cur, N, H + 2, W + 2, CPAD))
        h, w, npool = H, W, 0
        for cin, cout, pool, U, bias, scale in self.convs:
            if pool:
                h, w = h // 2, w // 2
                a = conv3x3_bn_relu_pool(a, U, bias, scale, True, out=self._view(cur ^ 1, N, h + 2, w + 2, cout))
                npool += 1
                if stages is not None:   # (a copy: the ping-pong tensors are rewritten two layers on)
                    stages[f"pool{npool}"] = a[:, 1:-1, 1:-1, :].clone()
            else:
                a = conv3x3_bn_relu(a, U, bias, scale, True, out=self._view(cur ^ 1, N, h + 2, w + 2, cout))
            cur ^= 1
        a = avgpool7_flatten(a, in_padded=True, out=self._view(cur ^ 1, N, 49 * self.feat_c))
        cur ^= 1
        for B, bias, ones in self.fc:
            a = conv1x1_bn(a, B, bias, ones, True, out=self._view(cur ^ 1, N, self.hidden))
            cur ^= 1
        avgpool_fc(a.view(N, 1, 1, self.hidden), self.head_packed, self.classes, in_padded=False, out=self._logits,
                   workspace=self._ws)

    def forward(self, x: torch.Tensor, return_stages: bool = False):
        """x [N][3][H][W] float32 on the model's device -> logits [N][classes] (the model's own output tensor,
        rewritten by the next forward).  With return_stages, also {"pool1".."pool5"}: copies of the five pooled maps
        (NHWC interiors).  A new input shape re-runs prepare()."""
        self._begin(x)
        stages = {} if return_stages else None
        with torch.cuda.device(self.device):
            self._run(x.contiguous(), stages)
        if not return_stages:
            return self._logits
        return self._logits, stages

    def flops(self, H: int = 224, W: int = 224) -> float:
        """Algorithmic multiply-add FLOPs of one image (2 per MAC; convolutions on their true input channels, FCs)."""
        f = 0.0
        for cin, cout, h, w, _ in layer_shapes(self.arch, H, W):
            f += 2.0 * h * w * 9 * cin * cout
        return f + 2.0 * (49 * self.feat_c * self.hidden + self.hidden * self.hidden + self.hidden * self.classes)


__all__ = ["ARCHS", "VGG", "conv_layers", "layer_shapes", "expected_keys", "validate_state_dict", "fc1_columns_hwc"]
