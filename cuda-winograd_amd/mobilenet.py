"""torchvision's MobileNetV2 on the library's kernels.

``MobileNetV2.from_state_dict(sd, width_mult)`` takes a torchvision state dict (its key names), folds every BN into a
(bias, scale) pair and packs every filter once; ``model(x_nchw)`` returns the logits.  Every channel count is
zero-padded up to a multiple of 64 at pack time (``CPAD``), the rule the dense heads use for their last filters: it
satisfies the 1x1 kernel's Cin % 32, Kout % 64.  Pad channels carry zero weights, zero scale and zero bias, so they are
exactly 0 through every activation and residual; the price is that the early layers compute 64 channels where the network
has 16 to 32.  The forward is a straight chain of launches on the current stream:

- stem: ``image_pack`` to 32 channels, then ``conv3x3_s2_bn_relu`` (ReLU) into a padded map;
- an inverted residual: expand, ``conv1x1_bn_ex`` with RELU | C_PADDED (flat in, padded out); depthwise,
  ``dwconv3x3_bn_act(act="relu6", in_cap=6)`` (padded in and out: the cap on its input turns the ReLU of the layer before
  it, the expand or the stem, into ReLU6); project, ``conv1x1_bn_ex`` with A_PADDED and no activation, plus ADD_RESIDUAL
  where the stride is 1 and the channels match (padded in, flat [N H W][C] out).  The t = 1 block has no expand;
- ``features.18``: a flat 1x1 with ReLU, then ``clamp_(max=6)`` -- torch plumbing, the one place a GEMM's ReLU6 has no
  depthwise behind it -- and ``avgpool_fc``.  Dropout is the identity at inference.

``prepare(N, H, W)`` allocates the activations, the workspace and the logits for an input shape and reserves the scratch
of every 1x1 launch, the stem and the head, so that a whole forward can be captured in one ``torch.cuda.graph``; the
depthwise layer has no scratch.  ``forward`` reads nothing on the host.
"""
from __future__ import annotations

import torch

from . import (A_PADDED, ADD_RESIDUAL, C_PADDED, RELU, WinoError, _out_hw, avgpool_fc, conv1x1_bn, conv1x1_bn_ex,
               conv1x1_prepare, conv3x3_s2_bn_relu, conv3x3_s2_prepare, dwconv3x3_bn_act, filter_pack_s2, head_pack,
               head_prepare, image_pack, lib)
from ._net import BN_KEYS, Net, check_state_dict

# torchvision's inverted-residual setting: (expansion t, channels c, repeats n, stride s)
SETTING = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))
STEM_C, LAST_C = 32, 1280
CPAD = 64        # every channel count is padded up to a multiple of this
IMG_C = 32       # channels of the packed image: the stride-2 3x3 needs C % 32
MIN_HW = 32      # five halvings must leave a pixel
STAGES = ("stride2", "stride4", "stride8", "stride16", "stride32")


def _make_divisible(v: float, divisor: int = 8) -> int:
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    return new_v + divisor if new_v < 0.9 * v else new_v


def _pad(c: int) -> int:
    return -(-c // CPAD) * CPAD


def blocks(width_mult: float = 1.0):
    """(stem channels, [(features index, Cin, hidden, Cout, stride, t)], last channels) of mobilenet_v2(width_mult)."""
    cin = _make_divisible(STEM_C * width_mult)
    stem, out, i = cin, [], 1
    for t, c, n, s in SETTING:
        cout = _make_divisible(c * width_mult)
        for j in range(n):
            out.append((i, cin, int(round(cin * t)), cout, s if j == 0 else 1, t))
            cin, i = cout, i + 1
    return stem, out, _make_divisible(LAST_C * max(1.0, width_mult))


def expected_keys(width_mult: float, classes: int):
    """{key: shape} of a torchvision mobilenet_v2 state dict (num_batches_tracked aside)."""
    stem, blks, last = blocks(width_mult)
    exp = {}

    def conv_bn(conv, bn, shape):
        exp[f"{conv}.weight"] = shape
        for k in BN_KEYS:
            exp[f"{bn}.{k}"] = (shape[0],)

    conv_bn("features.0.0", "features.0.1", (stem, 3, 3, 3))
    for i, cin, hid, cout, _, t in blks:
        p, j = f"features.{i}.conv", 0
        if t != 1:
            conv_bn(f"{p}.0.0", f"{p}.0.1", (hid, cin, 1, 1))
            j = 1
        conv_bn(f"{p}.{j}.0", f"{p}.{j}.1", (hid, 1, 3, 3))
        conv_bn(f"{p}.{j + 1}", f"{p}.{j + 2}", (cout, hid, 1, 1))
    conv_bn("features.18.0", "features.18.1", (last, blks[-1][3], 1, 1))
    exp["classifier.1.weight"], exp["classifier.1.bias"] = (classes, last), (classes,)
    return exp


def layer_shapes(width_mult: float, H: int, W: int):
    """[(Cin, hidden, Cout, stride, t, (hin, win), (h, w))] per inverted residual for an H x W input, channels as run
    (padded); hin x win is the block's input map, h x w its output."""
    _, blks, _ = blocks(width_mult)
    h, w = _out_hw(H, W, 2)
    out = []
    for _, cin, hid, cout, s, t in blks:
        ho, wo = _out_hw(h, w, s)
        out.append((_pad(cin), _pad(hid), _pad(cout), s, t, (h, w), (ho, wo)))
        h, w = ho, wo
    return out


class MobileNetV2(Net):
    """torchvision's mobilenet_v2 on the library's kernels, inference only (BN folded at load)."""

    def __init__(self, width_mult: float, classes: int, device):
        super().__init__(device)
        self.width_mult, self.classes = float(width_mult), classes

    @classmethod
    def from_state_dict(cls, sd, width_mult: float = 1.0, eps: float = 1e-5, device=None) -> "MobileNetV2":
        """Validate `sd` (torchvision key names) for mobilenet_v2(width_mult=width_mult), fold every BN, zero-pad every
        channel count to a multiple of 64 and pack every filter on `device` (default: the current CUDA device).  The
        number of classes is read from classifier.1.weight."""
        arch = f"mobilenet_v2(width_mult={width_mult})"
        k = "classifier.1.weight"
        if k not in sd:
            raise WinoError(f"state dict: missing key {k!r} for {arch}")
        if sd[k].dim() != 2:
            raise WinoError(f"state dict: key {k!r} has shape {tuple(sd[k].shape)}, {arch} needs a matrix")
        classes = int(sd[k].shape[0])
        check_state_dict(sd, expected_keys(width_mult, classes), arch, "running_mean")
        return cls._load(sd, eps, device, width_mult, classes)

    # ------------------------------------------------------------------ loading
    def _bn(self, sd, prefix, eps, cp):
        """The folded BN, zero-padded to `cp` channels: a pad channel's output is fma(0, acc, 0) = 0."""
        bias, scale = self._fold_bn(sd, prefix, eps)
        z = bias.new_zeros(cp - bias.numel())
        return torch.cat([bias, z]), torch.cat([scale, z])

    def _pw(self, sd, conv, bn, eps):
        """A 1x1 conv + BN as (B [Cin padded][Cout padded], bias, scale)."""
        w = sd[f"{conv}.weight"].detach().float()[:, :, 0, 0]
        o, i = int(w.shape[0]), int(w.shape[1])
        B = torch.zeros(_pad(i), _pad(o))
        B[:i, :o] = w.t()
        return (self._t(B), *self._bn(sd, bn, eps, _pad(o)))

    def _pack(self, sd, eps):
        stem, blks, last = blocks(self.width_mult)
        w = sd["features.0.0.weight"].detach().float()
        ws = torch.zeros(_pad(stem), IMG_C, 3, 3)
        ws[:stem, :3] = w
        self.stem = (filter_pack_s2(self._t(ws)), *self._bn(sd, "features.0.1", eps, _pad(stem)))
        self.blocks = []   # (expand or None, (taps, bias, scale), project, stride, residual?)
        for i, cin, hid, cout, s, t in blks:
            p, j = f"features.{i}.conv", 0
            expand = None
            if t != 1:
                expand, j = self._pw(sd, f"{p}.0.0", f"{p}.0.1", eps), 1
            taps = torch.zeros(3, 3, _pad(hid))
            taps[:, :, :hid] = sd[f"{p}.{j}.0.weight"].detach().float()[:, 0].permute(1, 2, 0)
            dw = (self._t(taps), *self._bn(sd, f"{p}.{j}.1", eps, _pad(hid)))
            self.blocks.append((expand, dw, self._pw(sd, f"{p}.{j + 1}", f"{p}.{j + 2}", eps), s, s == 1 and cin == cout))
        self.last = self._pw(sd, "features.18.0", "features.18.1", eps)
        self.feat_c = _pad(last)
        wfc = torch.zeros(self.classes, self.feat_c)
        wfc[:, :last] = sd["classifier.1.weight"].detach().float()
        self.head_packed = head_pack(self._t(wfc), self._t(sd["classifier.1.bias"]))
        torch.cuda.current_stream().synchronize()

    # ------------------------------------------------------------------ per input shape
    def prepare(self, N: int, H: int, W: int) -> None:
        """Allocate the activations (the packed image, two flat ping-pong tensors for the blocks' inputs and outputs, one
        padded tensor each for the expanded map and the depthwise output, each sized for its largest layer), the head's
        workspace and the logits for [N][3][H][W] inputs, and reserve the stream scratch of every 1x1 launch, the stem
        and the head on the current stream.  Call it before capturing a forward into a graph."""
        N, H, W = int(N), int(H), int(W)
        if N < 1 or H < MIN_HW or W < MIN_HW:
            raise WinoError(f"bad input shape N={N} H={H} W={W}: MobileNetV2 needs N >= 1 and H, W >= {MIN_HW}")
        dev, f32 = self.device, torch.float32
        shapes = layer_shapes(self.width_mult, H, W)
        h1, w1 = _out_hw(H, W, 2)
        stem_k = int(self.stem[1].numel())
        flat, wide, deep = 0, N * (h1 + 2) * (w1 + 2) * stem_k, 0
        with torch.cuda.device(dev):
            conv3x3_s2_prepare(N, H, W, IMG_C, stem_k)
            for cin, hid, cout, _, t, (h, w), (ho, wo) in shapes:
                if t != 1:
                    conv1x1_prepare(N * h * w, cin, hid)
                    wide = max(wide, N * (h + 2) * (w + 2) * hid)
                conv1x1_prepare(N * ho * wo, hid, cout)
                deep = max(deep, N * (ho + 2) * (wo + 2) * hid)
                flat = max(flat, N * ho * wo * cout)
            hl, wl = shapes[-1][6]
            conv1x1_prepare(N * hl * wl, shapes[-1][2], self.feat_c)
            flat = max(flat, N * hl * wl * self.feat_c)
            head_prepare(N, self.feat_c, self.classes)
            self._img = torch.zeros((N, H + 2, W + 2, IMG_C), dtype=f32, device=dev)
            self._flat = [torch.zeros(flat, dtype=f32, device=dev) for _ in range(2)]
            self._wide = torch.zeros(wide, dtype=f32, device=dev)
            self._deep = torch.zeros(deep, dtype=f32, device=dev)
            ws = lib().wino_head_workspace_bytes(N, self.feat_c, self.classes)
            self._ws = torch.empty((ws + 3) // 4, dtype=f32, device=dev)
            self._logits = torch.empty((N, self.classes), dtype=f32, device=dev)
        self._shape = (N, H, W)

    @staticmethod
    def _view(buf, *shape):
        n = 1
        for v in shape:
            n *= v
        return buf[:n].view(*shape)

    def _run(self, x, stages):
        N, H, W = self._shape
        h, w = _out_hw(H, W, 2)
        taps, bias, scale = self.stem
        a = conv3x3_s2_bn_relu(image_pack(x, IMG_C, out=self._img), taps, bias, scale, True,
                               out=self._view(self._wide, N, h + 2, w + 2, int(bias.numel())))
        cur, block_in, level = 0, None, 0   # block_in: the flat input of the block, None behind the stem
        for (expand, dw, project, s, residual), (cin, hid, cout, _, _, _, (ho, wo)) in zip(
                self.blocks, layer_shapes(self.width_mult, H, W)):
            if expand is not None:
                a = conv1x1_bn_ex(block_in, *expand, RELU | C_PADDED, out=self._view(self._wide, N, h + 2, w + 2, hid),
                                  hw=(h, w))
            d = dwconv3x3_bn_act(a, *dw, stride=s, act="relu6", in_cap=6.0, out=self._view(self._deep, N, ho + 2, wo + 2, hid))
            out = self._view(self._flat[cur], N * ho * wo, cout)
            conv1x1_bn_ex(d, *project, A_PADDED | (ADD_RESIDUAL if residual else 0), residual=block_in if residual else None,
                          out=out)
            block_in, cur, h, w, level = out, cur ^ 1, ho, wo, level + (s == 2)
            if stages is not None:   # a copy (the ping-pong tensors are rewritten two blocks on); a stride's last block stays
                stages[STAGES[level]] = out.view(N, h, w, cout).clone()
        B, bias, scale = self.last
        f = conv1x1_bn(block_in, B, bias, scale, True, out=self._view(self._flat[cur], N * h * w, self.feat_c))
        f.clamp_(max=6.0)   # torch plumbing: ReLU -> ReLU6 where no depthwise follows the GEMM
        avgpool_fc(f.view(N, h, w, self.feat_c), self.head_packed, self.classes, in_padded=False, out=self._logits,
                   workspace=self._ws)

    def forward(self, x: torch.Tensor, stages: bool = False):
        """x [N][3][H][W] float32 on the model's device -> logits [N][classes] (the model's own output tensor, rewritten
        by the next forward).  With stages, also {"stride2" .. "stride32"}: copies of the last block output at each of the
        five strides (features 1, 3, 6, 13 and 17; NHWC with the pad channels).  A new input shape re-runs prepare()."""
        self._begin(x)
        maps = {} if stages else None
        with torch.cuda.device(self.device):
            self._run(x.contiguous(), maps)
        if not stages:
            return self._logits
        return self._logits, maps


from .mobilenet_v3 import MobileNetV3  # noqa: E402  (mobilenet_v3.py: its block tables and expected_keys(arch, classes))

__all__ = ["MobileNetV2", "MobileNetV3", "SETTING", "STAGES", "blocks", "expected_keys", "layer_shapes"]
