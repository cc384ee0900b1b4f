"""What the whole-network classes (``ResNet``, ``VGG``) share: loading a torchvision state dict onto a device, the BN
fold, the key / shape check of a state dict, and the opening of ``forward``."""
from __future__ import annotations

import torch

from ._abi import WinoError

BN_KEYS = ("weight", "bias", "running_mean", "running_var")


def check_state_dict(sd, exp, arch: str, tracked_beside: str) -> None:
    """Every key of `exp` ({key: shape}) is in `sd` with that shape, and `sd` holds nothing else -- except a BN's
    num_batches_tracked, ignored where its `tracked_beside` key ("weight" or "running_mean") is expected.  Raises
    WinoError naming the first missing, unexpected or wrongly shaped key."""
    for k in exp:
        if k not in sd:
            raise WinoError(f"state dict: missing key {k!r} for {arch}")
    for k, v in sd.items():
        if k.endswith(".num_batches_tracked") and k[: -len("num_batches_tracked")] + tracked_beside in exp:
            continue
        if k not in exp:
            raise WinoError(f"state dict: unexpected key {k!r} for {arch}")
        if tuple(v.shape) != exp[k]:
            raise WinoError(f"state dict: key {k!r} has shape {tuple(v.shape)}, {arch} needs {exp[k]}")


class Net:
    """An inference-only network on the library's kernels.  A subclass gives _pack(sd, eps), prepare(N, H, W) and
    forward(x, ...); its constructor takes the device last."""

    def __init__(self, device):
        self.device = torch.device(device)
        self._shape = None

    @classmethod
    def _load(cls, sd, eps, device, *args, **kwargs):
        """cls(*args, device, **kwargs) with `sd` packed on `device` (default: the current CUDA device)."""
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise WinoError(f"{cls.__name__} runs on a CUDA(HIP) device only -- there is no CPU path")
        m = cls(*args, dev, **kwargs)
        with torch.cuda.device(dev):
            m._pack(sd, eps)
        return m

    def _t(self, v):
        return v.detach().to(device=self.device, dtype=torch.float32).contiguous()

    def _fold_bn(self, sd, prefix: str, eps: float, conv_bias=None):
        """The BN at sd[prefix.*] behind a convolution with `conv_bias` (or none), folded in fp64: scale = gamma /
        sqrt(var + eps), bias = beta - (mean - conv_bias) * scale.  Returns (bias, scale), the library's order."""
        g, beta = sd[f"{prefix}.weight"].double(), sd[f"{prefix}.bias"].double()
        mean, var = sd[f"{prefix}.running_mean"].double(), sd[f"{prefix}.running_var"].double()
        scale = g / torch.sqrt(var + eps)
        if conv_bias is not None:
            mean = mean - conv_bias.double()
        return self._t(beta - mean * scale), self._t(scale)

    def _begin(self, x) -> None:
        """forward's opening: x is [N][3][H][W] float32 on the model's device; a new input shape re-runs prepare()."""
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or int(x.shape[1]) != 3:
            raise WinoError("x must be [N][3][H][W]")
        if x.device != self.device or x.dtype != torch.float32:
            raise WinoError(f"x must be float32 on {self.device}")
        shape = (int(x.shape[0]), int(x.shape[2]), int(x.shape[3]))
        if shape != self._shape:
            self.prepare(*shape)

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)
