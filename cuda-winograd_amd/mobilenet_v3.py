"""torchvision's MobileNetV3-Large and MobileNetV3-Small on the library's kernels.

``MobileNetV3.from_state_dict(sd, arch)`` takes a torchvision state dict (its key names: ``features.{i}.block.{j}.{0,1}``,
``...fc1``, ``...fc2``, ``classifier.0``, ``classifier.3``), folds every BN (eps 1e-3) and packs every filter once;
``model(x_nchw)`` returns the logits.  As in ``mobilenet.py`` every channel count is zero-padded up to a multiple of 64
(``CPAD``); pad channels carry zero weights, scale and bias and are exactly 0 through every activation and gate (the SE
vectors of pad channels are zero too: their gate is hardsigmoid(0) = 0.5 on a map that is exactly 0).  The squeeze width
of an SE block is not padded (it is a multiple of 8).  The forward is a straight chain of launches on the current stream:

- stem: ``image_pack``, ``conv3x3_s2_bn_relu(relu=False)``, then ``act_scale_pool`` with hardswish in place on the padded
  map (the first block's depthwise reads it and, in ``large``, its residual is a flat copy of it);
- a block: expand, ``conv1x1_bn_ex`` with C_PADDED and RELU in a ReLU block, no activation in a hardswish block;
  depthwise, ``dwconv_bn_act`` (K = 3 or 5) with act = relu, or in_act = act = hardswish (the expand's activation happens
  while the depthwise stages its input), emitting pool partials in an SE block; SE: ``fc_act`` C -> Cs with ReLU over the
  partials (x_scale = 1 / (H W)), ``fc_act`` Cs -> C with hardsigmoid, ``act_scale_pool`` with the gate; project,
  ``conv1x1_bn_ex`` with A_PADDED, plus ADD_RESIDUAL where the stride is 1 and the channels match;
- head: the last 1x1 without activation, ``act_scale_pool`` with hardswish emitting partials, ``fc_act`` with hardswish,
  ``fc_act`` into the logits.  Dropout is the identity at inference.

An SE block is six launches where a plain one is three; no torch arithmetic runs in the forward (one ``copy_`` makes the
flat residual of ``large``'s first block).  ``prepare(N, H, W)`` allocates the activations, the partial and gate buffers
and the logits and reserves the scratch of every 1x1 launch and the stem, so that a whole forward can be captured in one
``torch.cuda.graph``; ``forward`` reads nothing on the host.
"""
from __future__ import annotations

import torch

from . import (A_PADDED, ADD_RESIDUAL, C_PADDED, RELU, WinoError, _cus, _out_hw, act_scale_pool, act_scale_pool_plan,
               conv1x1_bn, conv1x1_bn_ex, conv1x1_prepare, conv3x3_s2_bn_relu, conv3x3_s2_prepare, dwconv_bn_act,
               dwconv_plan, fc_act, filter_pack_s2, image_pack)
from ._net import BN_KEYS, Net, check_state_dict
from .mobilenet import CPAD, IMG_C, MIN_HW, STAGES, _make_divisible, _pad

# torchvision's bneck_conf rows: (input channels, kernel, expanded channels, output channels, SE, activation, stride)
BLOCKS = {
    "large": ((16, 3, 16, 16, False, "RE", 1), (16, 3, 64, 24, False, "RE", 2), (24, 3, 72, 24, False, "RE", 1),
              (24, 5, 72, 40, True, "RE", 2), (40, 5, 120, 40, True, "RE", 1), (40, 5, 120, 40, True, "RE", 1),
              (40, 3, 240, 80, False, "HS", 2), (80, 3, 200, 80, False, "HS", 1), (80, 3, 184, 80, False, "HS", 1),
              (80, 3, 184, 80, False, "HS", 1), (80, 3, 480, 112, True, "HS", 1), (112, 3, 672, 112, True, "HS", 1),
              (112, 5, 672, 160, True, "HS", 2), (160, 5, 960, 160, True, "HS", 1), (160, 5, 960, 160, True, "HS", 1)),
    "small": ((16, 3, 16, 16, True, "RE", 2), (16, 3, 72, 24, False, "RE", 2), (24, 3, 88, 24, False, "RE", 1),
              (24, 5, 96, 40, True, "HS", 2), (40, 5, 240, 40, True, "HS", 1), (40, 5, 240, 40, True, "HS", 1),
              (40, 5, 120, 48, True, "HS", 1), (48, 5, 144, 48, True, "HS", 1), (48, 5, 288, 96, True, "HS", 2),
              (96, 5, 576, 96, True, "HS", 1), (96, 5, 576, 96, True, "HS", 1)),
}
LAST_C = {"large": 1280, "small": 1024}   # width of the classifier's hidden layer
STEM_C = 16
ACT = {"RE": "relu", "HS": "hardswish"}


def _table(arch: str):
    if arch not in BLOCKS:
        raise WinoError(f"unknown MobileNetV3 arch {arch!r}: one of {sorted(BLOCKS)}")
    return BLOCKS[arch]


def squeeze_channels(exp: int) -> int:
    return _make_divisible(exp // 4, 8)


def expected_keys(arch: str, classes: int):
    """{key: shape} of a torchvision mobilenet_v3_{arch} state dict (num_batches_tracked aside)."""
    exp = {}

    def conv_bn(p, shape):
        exp[f"{p}.0.weight"] = shape
        for k in BN_KEYS:
            exp[f"{p}.1.{k}"] = (shape[0],)

    conv_bn("features.0", (STEM_C, 3, 3, 3))
    rows = _table(arch)
    for i, (cin, k, hid, cout, se, _, _) in enumerate(rows, 1):
        p, j = f"features.{i}.block", 0
        if hid != cin:
            conv_bn(f"{p}.0", (hid, cin, 1, 1))
            j = 1
        conv_bn(f"{p}.{j}", (hid, 1, k, k))
        j += 1
        if se:
            cs = squeeze_channels(hid)
            exp[f"{p}.{j}.fc1.weight"], exp[f"{p}.{j}.fc1.bias"] = (cs, hid, 1, 1), (cs,)
            exp[f"{p}.{j}.fc2.weight"], exp[f"{p}.{j}.fc2.bias"] = (hid, cs, 1, 1), (hid,)
            j += 1
        conv_bn(f"{p}.{j}", (cout, hid, 1, 1))
    last_in = rows[-1][3]
    conv_bn(f"features.{len(rows) + 1}", (6 * last_in, last_in, 1, 1))
    exp["classifier.0.weight"], exp["classifier.0.bias"] = (LAST_C[arch], 6 * last_in), (LAST_C[arch],)
    exp["classifier.3.weight"], exp["classifier.3.bias"] = (classes, LAST_C[arch]), (classes,)
    return exp


class MobileNetV3(Net):
    """torchvision's mobilenet_v3_large / mobilenet_v3_small on the library's kernels, inference only."""

    def __init__(self, arch: str, classes: int, device):
        super().__init__(device)
        self.arch, self.classes = arch, classes

    @classmethod
    def from_state_dict(cls, sd, arch: str = "large", eps: float = 1e-3, device=None) -> "MobileNetV3":
        """Validate `sd` (torchvision key names) for mobilenet_v3_{arch}, fold every BN, zero-pad every channel count to a
        multiple of 64 and pack every filter on `device` (default: the current CUDA device).  The number of classes is
        read from classifier.3.weight."""
        _table(arch)
        name, k = f"mobilenet_v3_{arch}", "classifier.3.weight"
        if k not in sd:
            raise WinoError(f"state dict: missing key {k!r} for {name}")
        if sd[k].dim() != 2:
            raise WinoError(f"state dict: key {k!r} has shape {tuple(sd[k].shape)}, {name} needs a matrix")
        classes = int(sd[k].shape[0])
        check_state_dict(sd, expected_keys(arch, classes), name, "running_mean")
        return cls._load(sd, eps, device, arch, classes)

    # ------------------------------------------------------------------ loading
    def _bn(self, sd, prefix, eps, cp):
        bias, scale = self._fold_bn(sd, prefix, eps)
        z = bias.new_zeros(cp - bias.numel())
        return torch.cat([bias, z]), torch.cat([scale, z])

    def _pw(self, sd, p, eps):
        """A 1x1 conv + BN at p.0 / p.1 as (B [Cin padded][Cout padded], bias, scale)."""
        w = sd[f"{p}.0.weight"].detach().float()[:, :, 0, 0]
        o, i = int(w.shape[0]), int(w.shape[1])
        B = torch.zeros(_pad(i), _pad(o))
        B[:i, :o] = w.t()
        return (self._t(B), *self._bn(sd, f"{p}.1", eps, _pad(o)))

    def _fc(self, sd, p, rows, cols):
        """A Linear or 1x1 conv with bias at p as (W [rows][cols], b [rows]), zero-padded."""
        w = sd[f"{p}.weight"].detach().float().flatten(1)
        W, b = torch.zeros(rows, cols), torch.zeros(rows)
        W[:w.shape[0], :w.shape[1]] = w
        b[:w.shape[0]] = sd[f"{p}.bias"].detach().float()
        return self._t(W), self._t(b)

    def _pack(self, sd, eps):
        rows = _table(self.arch)
        ws = torch.zeros(_pad(STEM_C), IMG_C, 3, 3)
        ws[:STEM_C, :3] = sd["features.0.0.weight"].detach().float()
        self.stem = (filter_pack_s2(self._t(ws)), *self._bn(sd, "features.0.1", eps, _pad(STEM_C)))
        self.blocks = []   # (expand or None, (taps, bias, scale), SE (W1, b1, W2, b2) or None, project, act, stride, residual?)
        for i, (cin, k, hid, cout, se, act, s) in enumerate(rows, 1):
            p, j = f"features.{i}.block", 0
            expand = None
            if hid != cin:
                expand, j = self._pw(sd, f"{p}.0", eps), 1
            taps = torch.zeros(k, k, _pad(hid))
            taps[:, :, :hid] = sd[f"{p}.{j}.0.weight"].detach().float()[:, 0].permute(1, 2, 0)
            dw = (self._t(taps), *self._bn(sd, f"{p}.{j}.1", eps, _pad(hid)))
            j += 1
            gate = None
            if se:
                cs = squeeze_channels(hid)
                gate = (*self._fc(sd, f"{p}.{j}.fc1", cs, _pad(hid)), *self._fc(sd, f"{p}.{j}.fc2", _pad(hid), cs))
                j += 1
            self.blocks.append((expand, dw, gate, self._pw(sd, f"{p}.{j}", eps), ACT[act], s, s == 1 and cin == cout))
        last_in = rows[-1][3]
        self.last = self._pw(sd, f"features.{len(rows) + 1}", eps)
        self.feat_c = _pad(6 * last_in)
        self.fc1 = self._fc(sd, "classifier.0", LAST_C[self.arch], self.feat_c)
        self.fc2 = self._fc(sd, "classifier.3", self.classes, LAST_C[self.arch])
        torch.cuda.current_stream().synchronize()

    def layer_shapes(self, H: int, W: int):
        """[(Cin, hidden, Cout, kernel, stride, SE width or 0, (hin, win), (h, w))] per block for an H x W input, channels
        as run (padded)."""
        h, w = _out_hw(H, W, 2)
        out = []
        for cin, k, hid, cout, se, _, s in _table(self.arch):
            ho, wo = _out_hw(h, w, s)
            out.append((_pad(cin), _pad(hid), _pad(cout), k, s, squeeze_channels(hid) if se else 0, (h, w), (ho, wo)))
            h, w = ho, wo
        return out

    # ------------------------------------------------------------------ per input shape
    def prepare(self, N: int, H: int, W: int) -> None:
        """Allocate the activations (the packed image, two flat ping-pong tensors, one padded tensor each for the expanded
        map and the depthwise output), the pool partials, squeeze and gate buffers of the SE blocks, the head's buffers
        and the logits for [N][3][H][W] inputs, and reserve the stream scratch of every 1x1 launch and the stem on the
        current stream.  Call it before capturing a forward into a graph."""
        N, H, W = int(N), int(H), int(W)
        if N < 1 or H < MIN_HW or W < MIN_HW:
            raise WinoError(f"bad input shape N={N} H={H} W={W}: MobileNetV3 needs N >= 1 and H, W >= {MIN_HW}")
        dev, f32 = self.device, torch.float32
        shapes = self.layer_shapes(H, W)
        h1, w1 = _out_hw(H, W, 2)
        stem_k = int(self.stem[1].numel())
        flat, wide, deep, parts, sq, gate = N * h1 * w1 * stem_k, N * (h1 + 2) * (w1 + 2) * stem_k, 0, 1, 1, 1
        with torch.cuda.device(dev):
            cus = _cus(dev)
            conv3x3_s2_prepare(N, H, W, IMG_C, stem_k)
            for (expand, *_), (cin, hid, cout, k, s, cs, (h, w), (ho, wo)) in zip(self.blocks, shapes):
                if expand is not None:
                    conv1x1_prepare(N * h * w, cin, hid)
                    wide = max(wide, N * (h + 2) * (w + 2) * hid)
                conv1x1_prepare(N * ho * wo, hid, cout)
                deep = max(deep, N * (ho + 2) * (wo + 2) * hid)
                flat = max(flat, N * ho * wo * cout)
                if cs:
                    _, _, _, ty, tx = dwconv_plan(N, h, w, hid, k, s, cus)
                    parts, sq, gate = max(parts, N * ty * tx * hid), max(sq, N * cs), max(gate, N * hid)
            hl, wl = shapes[-1][7]
            conv1x1_prepare(N * hl * wl, shapes[-1][2], self.feat_c)
            flat = max(flat, N * hl * wl * self.feat_c)
            parts = max(parts, N * act_scale_pool_plan(N, hl, wl, self.feat_c)[1] * self.feat_c)
            self._img = torch.zeros((N, H + 2, W + 2, IMG_C), dtype=f32, device=dev)
            self._flat = [torch.zeros(flat, dtype=f32, device=dev) for _ in range(2)]
            self._wide = torch.zeros(wide, dtype=f32, device=dev)
            self._deep = torch.zeros(deep, dtype=f32, device=dev)
            self._parts = torch.zeros(parts, dtype=f32, device=dev)
            self._sq = torch.zeros(sq, dtype=f32, device=dev)
            self._gate = torch.zeros(gate, dtype=f32, device=dev)
            self._hidden = torch.empty((N, LAST_C[self.arch]), dtype=f32, device=dev)
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
        c0 = int(bias.numel())
        a = conv3x3_s2_bn_relu(image_pack(x, IMG_C, out=self._img), taps, bias, scale, False,
                               out=self._view(self._wide, N, h + 2, w + 2, c0))
        act_scale_pool(a, "hardswish", padded=True)
        cur, block_in, level = 0, None, 0   # block_in: the flat input of the block
        if self.blocks[0][6] or stages is not None:   # the first block's residual is the stem's map, flat
            block_in = self._view(self._flat[0], N * h * w, c0)
            block_in.view(N, h, w, c0).copy_(a[:, 1:-1, 1:-1, :])
            cur = 1
            if stages is not None:
                stages[STAGES[0]] = block_in.view(N, h, w, c0).clone()
        for (expand, dw, se, project, act, s, residual), (cin, hid, cout, k, _, cs, _, (ho, wo)) in zip(
                self.blocks, self.layer_shapes(H, W)):
            in_act = None
            if expand is not None:
                a = conv1x1_bn_ex(block_in, *expand, (RELU if act == "relu" else 0) | C_PADDED,
                                  out=self._view(self._wide, N, h + 2, w + 2, hid), hw=(h, w))
                in_act = None if act == "relu" else act
            d = self._view(self._deep, N, ho + 2, wo + 2, hid)
            if se is None:
                dwconv_bn_act(a, *dw, stride=s, act=act, in_act=in_act, out=d)
            else:
                _, _, _, ty, tx = dwconv_plan(N, h, w, hid, k, s, _cus(self.device))
                _, parts = dwconv_bn_act(a, *dw, stride=s, act=act, in_act=in_act, out=d,
                                         partials=self._view(self._parts, N, ty * tx, hid))
                sq = fc_act(parts, se[0], se[1], "relu", 1.0 / (ho * wo), out=self._view(self._sq, N, cs))
                gate = fc_act(sq, se[2], se[3], "hardsigmoid", out=self._view(self._gate, N, hid))
                act_scale_pool(d, "none", gate, padded=True)
            out = self._view(self._flat[cur], N * ho * wo, cout)
            conv1x1_bn_ex(d, *project, A_PADDED | (ADD_RESIDUAL if residual else 0), residual=block_in if residual else None,
                          out=out)
            block_in, cur, h, w, level = out, cur ^ 1, ho, wo, level + (s == 2)
            if stages is not None:
                stages[STAGES[level]] = out.view(N, h, w, cout).clone()
        B, bias, scale = self.last
        f = conv1x1_bn(block_in, B, bias, scale, False, out=self._view(self._flat[cur], N * h * w, self.feat_c))
        P = act_scale_pool_plan(N, h, w, self.feat_c)[1]
        _, parts = act_scale_pool(f.view(N, h, w, self.feat_c), "hardswish", partials=self._view(self._parts, N, P, self.feat_c))
        hid = fc_act(parts, *self.fc1, "hardswish", 1.0 / (h * w), out=self._hidden)
        fc_act(hid, *self.fc2, "none", out=self._logits)

    def forward(self, x: torch.Tensor, stages: bool = False):
        """x [N][3][H][W] float32 on the model's device -> logits [N][classes] (the model's own output tensor, rewritten
        by the next forward).  With stages, also {"stride2" .. "stride32"}: copies of the last map at each of the five
        strides (the activated stem map or, in `large`, block 1's output; then the last block output of each stride;
        NHWC with the pad channels).  A new input shape re-runs prepare()."""
        self._begin(x)
        maps = {} if stages else None
        with torch.cuda.device(self.device):
            self._run(x.contiguous(), maps)
        if not stages:
            return self._logits
        return self._logits, maps


__all__ = ["MobileNetV3", "BLOCKS", "LAST_C", "STAGES", "CPAD", "expected_keys", "squeeze_channels"]
