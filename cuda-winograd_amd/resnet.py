"""Whole torchvision ResNets (18, 34, 50, 101, 152), Wide ResNets (50-2, 101-2) and ResNeXts (50 32x4d, 101 32x8d,
101 64x4d) on the library's kernels.

``ResNet.from_state_dict(sd, arch)`` takes a torchvision state dict (its key names), folds every BN and packs every
filter once; ``model(x_nchw)`` returns the logits.  The forward is a straight chain of launches on the current
stream: the stem, the blocks, the head.

- ResNet-18 / -34 (basic blocks) keep the padded layout [N][H+2][W+2][C] from the stem on: the stem writes its
  zero ring, ``basic_block_s2`` opens conv3..conv5, ``basic_block`` runs in place on its stage's tensor, and the head
  reads the padded map without its ring.
- ResNet-50 / -101 / -152 (bottlenecks, torchvision's v1.5 placement) use the unpadded layout [N][H][W][C]:
  ``proj_block`` at stride 1 opens conv2, ``proj_block_v15`` opens conv3..conv5, and ``residual_block`` ping-pongs
  between the stage's two tensors.  The Wide ResNets are the same blocks with a middle width of 2 x planes.
- The ResNeXts use the same layout and ping-pong with the grouped 3x3 in the middle of every block:
  ``grouped_proj_block`` opens every stage (stride 1 in conv2, 2 after it), ``grouped_residual_block`` follows.

- The segmentation backbones (``replace_stride_with_dilation``, dense bottleneck nets only) keep a dilated stage at its
  input's resolution: its first block is ``proj_block`` at stride 1 or, where the stage before it was dilated too,
  ``dilated_proj_block`` at that stage's dilation; the rest are ``dilated_residual_block`` at the new dilation.

``prepare(N, H, W)`` allocates the activations and one shared workspace for an input shape and reserves every
launch's stream scratch, so that a whole forward can then be captured in one ``torch.cuda.graph``.
"""
from __future__ import annotations

from collections import namedtuple
from types import SimpleNamespace

import torch

from . import (WinoError, _out_hw, avgpool_fc, basic_block, basic_block_prepare, basic_block_s2,
               basic_block_s2_prepare, dilated_proj_block, dilated_proj_block_prepare, dilated_residual_block,
               dilated_residual_block_prepare, filter_pack_grouped, filter_pack_s2, filter_transform_f2, grouped_proj_block,
               grouped_proj_block_prepare, grouped_proj_block_workspace_bytes, grouped_residual_block,
               grouped_residual_block_prepare, head_pack, head_prepare, lib, proj_block, proj_block_prepare,
               proj_block_v15, proj_block_v15_prepare, proj_tail_pack, residual_block, residual_block_prepare,
               s2_proj_pack, stem, stem_filter_pack, stem_out_hw)
from ._net import BN_KEYS, Net, check_state_dict

# arch -> (bottleneck?, blocks per stage)
ARCHS = {
    "resnet18": (False, (2, 2, 2, 2)),
    "resnet34": (False, (3, 4, 6, 3)),
    "resnet50": (True, (3, 4, 6, 3)),
    "resnet101": (True, (3, 4, 23, 3)),
    "resnet152": (True, (3, 8, 36, 3)),
    "resnext50_32x4d": (True, (3, 4, 6, 3)),
    "resnext101_32x8d": (True, (3, 4, 23, 3)),
    "resnext101_64x4d": (True, (3, 4, 23, 3)),
    "wide_resnet50_2": (True, (3, 4, 6, 3)),
    "wide_resnet101_2": (True, (3, 4, 23, 3)),
}
# arch -> (groups, width_per_group) of its bottlenecks' 3x3; every other arch: (1, 64)
WIDTHS = {
    "resnext50_32x4d": (32, 4),
    "resnext101_32x8d": (32, 8),
    "resnext101_64x4d": (64, 4),
    "wide_resnet50_2": (1, 128),
    "wide_resnet101_2": (1, 128),
}
PLANES = (64, 128, 256, 512)


def mid_channels(arch: str, planes: int):
    """(groups, Cm) of a bottleneck of `arch`: the middle width planes * width_per_group / 64 * groups (torchvision's
    Bottleneck), in `groups` groups."""
    groups, wpg = WIDTHS.get(arch, (1, 64))
    return groups, planes * wpg // 64 * groups


# ---------------------------------------------------------------------------------------------------- the block table
# One row per block kind: everything the model does with a block.  `ld` loads from the state dict (w: a tensor on the
# device, w1x1: torch's [K][C][1][1] as the library's [C][K], bn: a folded BN); `s` is the block at one input size.
_Shape = namedtuple("_Shape", "N h w ho wo cin cm cout groups dilation",   # h x w: the block's input map, ho x wo: its
                    defaults=(1,))                                          # output
_Kind = namedtuple("_Kind", "stride pack workspace prepare run macs")
# stride:    of the block (a field, so that nothing reads it off a name)
# pack:      (ld, "layerL.b", groups) -> the block's packed parameters
# workspace: (s) -> bytes;  prepare: (s) -> None, reserves the launches' stream scratch
# run:       (x, params, groups, dilation, out, workspace) -> the output tensor
# macs:      (px, cin, cm, cout, groups) -> multiply-adds per image at px output pixels


def _bottleneck_kind(stride, mid_pack, workspace, prepare, run, proj):
    """A bottleneck row: 1x1, the 3x3 packed by mid_pack, then w3 with bn3 (identity) or the packed projection tail."""
    def pack(ld, p, groups):
        w1, bn1, bn2, bn3 = ld.w1x1(f"{p}.conv1.weight"), ld.bn(f"{p}.bn1"), ld.bn(f"{p}.bn2"), ld.bn(f"{p}.bn3")
        w2, w3 = mid_pack(ld.w(f"{p}.conv2.weight"), groups), ld.w1x1(f"{p}.conv3.weight")
        if not proj:
            return w1, bn1, w2, bn2, w3, bn3
        wp, bnp = ld.w1x1(f"{p}.downsample.0.weight"), ld.bn(f"{p}.downsample.1")
        return w1, bn1, w2, bn2, proj_tail_pack(w3, bn3, wp, bnp)

    def macs(px, cin, cm, cout, groups):   # torchvision's placement: the first 1x1 runs before the stride
        return px * (stride * stride * cin * cm + 9 * cm * (cm // groups) + cm * cout + (cin * cout if proj else 0))

    return _Kind(stride, pack, workspace, prepare, run, macs)


def _pack_basic(ld, p, groups):
    return (filter_transform_f2(ld.w(f"{p}.conv1.weight")), ld.bn(f"{p}.bn1"),
            filter_transform_f2(ld.w(f"{p}.conv2.weight")), ld.bn(f"{p}.bn2"))


def _pack_basic_s2(ld, p, groups):
    packed = s2_proj_pack(filter_pack_s2(ld.w(f"{p}.conv1.weight")), ld.bn(f"{p}.bn1"),
                          ld.w1x1(f"{p}.downsample.0.weight"), ld.bn(f"{p}.downsample.1"))
    return packed, filter_transform_f2(ld.w(f"{p}.conv2.weight")), ld.bn(f"{p}.bn2")


def _grouped_proj_kind(stride):
    return _bottleneck_kind(
        stride, filter_pack_grouped, lambda s: grouped_proj_block_workspace_bytes(s.N, s.h, s.w, s.cm, stride),
        lambda s: grouped_proj_block_prepare(s.N, s.h, s.w, s.cin, s.cm, s.cout, s.groups, stride),
        lambda x, p, g, d, out, ws: grouped_proj_block(x, *p, g, stride, out=out, workspace=ws), proj=True)


def _residual_workspace(s):
    return lib().wino_residual_block_workspace_bytes_hw(s.N, s.ho, s.wo, s.cm)


_dense = lambda w, groups: filter_transform_f2(w)
KINDS = {
    # ResNet-18 / -34: in place on the stage's tensor after its first block
    "basic": _Kind(1, _pack_basic, lambda s: lib().wino_basic_block_workspace_bytes_hw(s.N, s.ho, s.wo, s.cout),
                   lambda s: basic_block_prepare(s.N, s.ho, s.wo, s.cout),
                   lambda x, p, g, d, out, ws: basic_block(x, *p, out=out, workspace=ws),
                   lambda px, cin, cm, cout, groups: px * 9 * (cin * cout + cout * cout)),
    "basic_s2": _Kind(2, _pack_basic_s2, lambda s: lib().wino_basic_block_s2_workspace_bytes_hw(s.N, s.h, s.w, s.cout),
                      lambda s: basic_block_s2_prepare(s.N, s.h, s.w, s.cin, s.cout),
                      lambda x, p, g, d, out, ws: basic_block_s2(x, *p, out=out, workspace=ws),
                      lambda px, cin, cm, cout, groups: px * (9 * (cin * cout + cout * cout) + cin * cout)),
    # the bottleneck nets; at stride 1 the v1 and v1.5 placements are the same block
    "residual": _bottleneck_kind(1, _dense, _residual_workspace,
                                 lambda s: residual_block_prepare(s.N, s.cout, s.cm, s.ho, s.wo),
                                 lambda x, p, g, d, out, ws: residual_block(x, *p, out=out, workspace=ws), proj=False),
    "proj": _bottleneck_kind(1, _dense, lambda s: lib().wino_proj_block_workspace_bytes_hw(s.N, s.ho, s.wo, s.cm),
                             lambda s: proj_block_prepare(s.N, s.h, s.w, s.cin, s.cm, s.cout, 1),
                             lambda x, p, g, d, out, ws: proj_block(x, *p, 1, out=out, workspace=ws), proj=True),
    "proj_v15": _bottleneck_kind(2, lambda w, groups: filter_pack_s2(w),
                                 lambda s: lib().wino_proj_block_v15_workspace_bytes_hw(s.N, s.h, s.w, s.cm),
                                 lambda s: proj_block_v15_prepare(s.N, s.h, s.w, s.cin, s.cm, s.cout),
                                 lambda x, p, g, d, out, ws: proj_block_v15(x, *p, out=out, workspace=ws), proj=True),
    # the ResNeXts: the grouped 3x3 in every block, the stride on it
    "grouped_residual": _bottleneck_kind(
        1, filter_pack_grouped, _residual_workspace,
        lambda s: grouped_residual_block_prepare(s.N, s.ho, s.wo, s.cout, s.cm, s.groups),
        lambda x, p, g, d, out, ws: grouped_residual_block(x, *p, g, out=out, workspace=ws), proj=False),
    "grouped_proj": _grouped_proj_kind(1),
    "grouped_proj_s2": _grouped_proj_kind(2),
    # the dilated stages of a segmentation backbone: stride 1, the dilated 3x3 in the middle at the block's dilation
    "dilated_residual": _bottleneck_kind(
        1, lambda w, groups: filter_pack_s2(w), _residual_workspace,
        lambda s: dilated_residual_block_prepare(s.N, s.ho, s.wo, s.cout, s.cm, s.dilation),
        lambda x, p, g, d, out, ws: dilated_residual_block(x, *p, d, out=out, workspace=ws), proj=False),
    "dilated_proj": _bottleneck_kind(
        1, lambda w, groups: filter_pack_s2(w), lambda s: lib().wino_proj_block_workspace_bytes_hw(s.N, s.ho, s.wo, s.cm),
        lambda s: dilated_proj_block_prepare(s.N, s.h, s.w, s.cin, s.cm, s.cout, s.dilation),
        lambda x, p, g, d, out, ws: dilated_proj_block(x, *p, d, out=out, workspace=ws), proj=True),
}
NO_DILATION = (False, False, False)


def block_kind(bottleneck: bool, grouped: bool, stage: int, first: bool) -> str:
    """The KINDS row of a block: `first` of its stage (1..4) or not; conv2 opens at stride 1, conv3..conv5 at 2."""
    if not bottleneck:
        return "basic_s2" if first and stage > 1 else "basic"
    if not first:
        return "grouped_residual" if grouped else "residual"
    if grouped:
        return "grouped_proj" if stage == 1 else "grouped_proj_s2"
    return "proj" if stage == 1 else "proj_v15"


def check_dilation_arg(arch: str, replace_stride_with_dilation):
    """torchvision's replace_stride_with_dilation of `arch` as a tuple of three bools (layer2, layer3, layer4).  Only
    the dense bottleneck nets take a dilated stage: torchvision refuses it on the basic-block nets, and there is no
    dilated grouped 3x3."""
    if arch not in ARCHS:
        raise WinoError(f"unknown arch {arch!r}: one of {sorted(ARCHS)}")
    try:
        r = tuple(bool(v) for v in replace_stride_with_dilation)
    except TypeError:
        r = ()
    if len(r) != 3:
        raise WinoError("replace_stride_with_dilation must have three elements (layer2, layer3, layer4)")
    if any(r) and (not ARCHS[arch][0] or WIDTHS.get(arch, (1, 64))[0] > 1):
        raise WinoError(f"{arch}: replace_stride_with_dilation is for the dense bottleneck nets "
                        "(no dilated basic block, no dilated grouped 3x3)")
    return r


def dilated_block_plan(replace_stride_with_dilation, blocks):
    """torchvision's _make_layer rule, per stage a list of (kind, dilation) for the dense bottleneck nets: a dilated
    stage's stride becomes 1 and multiplies the dilation; its first block runs at the PREVIOUS dilation ("proj" at 1,
    "dilated_proj" otherwise), the rest at the new one ("residual" at 1, "dilated_residual" otherwise)."""
    plan, d = [], 1
    for L, nb in enumerate(blocks, 1):
        prev = d
        dilate = L > 1 and replace_stride_with_dilation[L - 2]
        if dilate:
            d *= 2
        if L == 1 or dilate:
            first = ("proj", 1) if prev == 1 else ("dilated_proj", prev)
        elif prev == 1:
            first = ("proj_v15", 1)
        else:
            raise WinoError(f"layer{L}: a stride-2 3x3 at dilation {prev} is not supported "
                            "(a dilated stage must be followed by dilated stages)")
        rest = ("residual", 1) if d == 1 else ("dilated_residual", d)
        plan.append([first] + [rest] * (nb - 1))
    return plan


def stage_shapes(arch: str, H: int, W: int, replace_stride_with_dilation=NO_DILATION):
    """[(name, C, h, w)] of the stem's output and of the four stages' outputs for an H x W input; a dilated stage
    (replace_stride_with_dilation, as torchvision's) keeps its input's size."""
    rswd = check_dilation_arg(arch, replace_stride_with_dilation)
    bottleneck, _ = ARCHS[arch]
    h, w = stem_out_hw(H, W)
    shapes = [("stem", 64, h, w)]
    for i, planes in enumerate(PLANES):
        if i and not rswd[i - 1]:
            h, w = _out_hw(h, w, 2)
        shapes.append((f"layer{i + 1}", planes * (4 if bottleneck else 1), h, w))
    return shapes


def expected_keys(arch: str, classes):
    """{key: shape} of a torchvision state dict of `arch` (num_batches_tracked aside); classes None: the headless
    body (no fc), as a detection backbone keeps it."""
    if arch not in ARCHS:
        raise WinoError(f"unknown arch {arch!r}: one of {sorted(ARCHS)}")
    bottleneck, blocks = ARCHS[arch]
    exp = {}

    def bn(prefix, c):
        for k in BN_KEYS:
            exp[f"{prefix}.{k}"] = (c,)

    exp["conv1.weight"] = (64, 3, 7, 7)
    bn("bn1", 64)
    cin = 64
    for L, (planes, nb) in enumerate(zip(PLANES, blocks), 1):
        for b in range(nb):
            p = f"layer{L}.{b}"
            stride = 2 if (b == 0 and L > 1) else 1
            if bottleneck:
                cout = planes * 4
                groups, cm = mid_channels(arch, planes)
                exp[f"{p}.conv1.weight"] = (cm, cin, 1, 1)
                exp[f"{p}.conv2.weight"] = (cm, cm // groups, 3, 3)
                exp[f"{p}.conv3.weight"] = (cout, cm, 1, 1)
                bn(f"{p}.bn1", cm), bn(f"{p}.bn2", cm), bn(f"{p}.bn3", cout)
            else:
                cout = planes
                exp[f"{p}.conv1.weight"] = (planes, cin, 3, 3)
                exp[f"{p}.conv2.weight"] = (planes, planes, 3, 3)
                bn(f"{p}.bn1", planes), bn(f"{p}.bn2", planes)
            if stride != 1 or cin != cout:
                exp[f"{p}.downsample.0.weight"] = (cout, cin, 1, 1)
                bn(f"{p}.downsample.1", cout)
            cin = cout
    if classes is not None:
        exp["fc.weight"] = (classes, cin)
        exp["fc.bias"] = (classes,)
    return exp


def validate_state_dict(sd, arch: str) -> int:
    """Checks every key and shape of `sd` against `arch` on the host; returns the class count.  Raises WinoError
    naming the first missing, unexpected or wrongly shaped key."""
    if "fc.weight" not in sd:
        raise WinoError("state dict: missing key 'fc.weight'")
    classes = int(sd["fc.weight"].shape[0])
    check_state_dict(sd, expected_keys(arch, classes), arch, "weight")
    return classes


class ResNet(Net):
    """A torchvision ResNet on the library's kernels, inference only (BN folded at load)."""

    # torchvision's replace_stride_with_dilation (layer2, layer3, layer4); at class level too, for an instance whose
    # block list is filled in without __init__ (flops() of a list built from key shapes)
    dilate = NO_DILATION

    def __init__(self, arch: str, classes: int, device, replace_stride_with_dilation=NO_DILATION):
        super().__init__(device)
        self.arch, self.classes = arch, classes
        self.dilate = check_dilation_arg(arch, replace_stride_with_dilation)
        self.bottleneck, self.blocks = ARCHS[arch]
        self.groups = WIDTHS.get(arch, (1, 64))[0]

    # ------------------------------------------------------------------ loading
    @classmethod
    def from_state_dict(cls, sd, arch: str, eps: float = 1e-5, device=None,
                        replace_stride_with_dilation=NO_DILATION) -> "ResNet":
        """Validate `sd` (torchvision key names) for `arch`, fold every BN (scale = gamma / sqrt(var + eps),
        bias = beta - mean * scale) and pack every filter on `device` (default: the current CUDA device).
        replace_stride_with_dilation: torchvision's argument of that name, for resnet50 / 101 / 152 and the Wide
        ResNets (the state dict's keys and shapes do not depend on it).  One restriction beyond torchvision's: every
        stage after a dilated one must be dilated too -- (False, False, True), (False, True, True) and (True, True, True)
        run, (True, False, False) raises WinoError, because it asks for a stride-2 3x3 at dilation 2, which the library
        does not have."""
        rswd = check_dilation_arg(arch, replace_stride_with_dilation)
        return cls._load(sd, eps, device, arch, validate_state_dict(sd, arch), replace_stride_with_dilation=rswd)

    def _pack(self, sd, eps):
        ld = self._pack_body(sd, eps)
        self.head_packed = head_pack(ld.w("fc.weight"), ld.w("fc.bias"))
        torch.cuda.current_stream().synchronize()

    def _pack_body(self, sd, eps, prefix: str = ""):
        """The stem and the four stages from sd[prefix + <torchvision's key>] (a detection backbone keeps the body
        under "body."); returns the loader."""
        def w1x1(key):   # torch's [K][C][1][1] -> the library's [C][K]
            w = sd[prefix + key]
            return self._t(w.reshape(w.shape[0], w.shape[1]).t())

        ld = SimpleNamespace(w=lambda key: self._t(sd[prefix + key]), w1x1=w1x1,
                             bn=lambda p: self._fold_bn(sd, prefix + p, eps))
        self.stem_packed = stem_filter_pack(ld.w("conv1.weight"), ld.bn("bn1"))
        self.layers = []   # per stage: (kind, cin, cm, cout, packed parameters) of its blocks, kind a KINDS row
        self.dilations = []   # per stage: the dilation of each block's 3x3 (1: none)
        cin = 64
        dilated = dilated_block_plan(self.dilate, self.blocks) if any(self.dilate) else None
        for L, (planes, nb) in enumerate(zip(PLANES, self.blocks), 1):
            cout = planes * 4 if self.bottleneck else planes
            cm = mid_channels(self.arch, planes)[1] if self.bottleneck else planes
            blocks, dils = [], []
            for b in range(nb):
                kind, d = dilated[L - 1][b] if dilated else (block_kind(self.bottleneck, self.groups > 1, L, b == 0), 1)
                blocks.append((kind, cin, cm, cout, KINDS[kind].pack(ld, f"layer{L}.{b}", self.groups)))
                dils.append(d)
                cin = cout
            self.layers.append(blocks)
            self.dilations.append(dils)
        self.feat_c = cin
        return ld

    # ------------------------------------------------------------------ per input shape
    def prepare(self, N: int, H: int, W: int) -> None:
        """Allocate the activations and the shared workspace for [N][3][H][W] inputs and reserve the stream scratch of
        every launch on the current stream.  Call it before capturing a forward into a graph."""
        N, H, W = int(N), int(H), int(W)
        dev, f32 = self.device, torch.float32
        with torch.cuda.device(dev):
            ws = max(self._prepare_body(N, H, W), lib().wino_head_workspace_bytes(N, self.feat_c, self.classes))
            head_prepare(N, self.feat_c, self.classes)
            self._ws = torch.empty((ws + 3) // 4, dtype=f32, device=dev)
            self._logits = torch.empty((N, self.classes), dtype=f32, device=dev)
        self._shape = (N, H, W)

    def _prepare_body(self, N: int, H: int, W: int) -> int:
        """The stem's and the stages' activations for [N][3][H][W] inputs, and their launches' stream scratch; returns
        the bytes of workspace the blocks need (the caller allocates self._ws).  On the model's device."""
        if N < 1 or H < 1 or W < 1:
            raise WinoError(f"bad input shape N={N} H={H} W={W}")
        dev, f32 = self.device, torch.float32
        shapes = stage_shapes(self.arch, H, W, self.dilate)
        pad = 0 if self.bottleneck else 2
        _, c0, h0, w0 = shapes[0]
        self._stem_out = torch.zeros((N, h0 + pad, w0 + pad, c0), dtype=f32, device=dev)
        self._stages = []   # per stage: the tensors its blocks write (two for the bottleneck ping-pong)
        ws = 0
        h, w = h0, w0
        for (name, c, ho, wo), blocks, dils in zip(shapes[1:], self.layers, self.dilations):
            bufs = [torch.zeros((N, ho + pad, wo + pad, c), dtype=f32, device=dev)
                    for _ in range(2 if self.bottleneck else 1)]
            self._stages.append(bufs)
            for (kind, cin, cm, cout, _), d in zip(blocks, dils):
                shape = _Shape(N, h, w, ho, wo, cin, cm, cout, self.groups, d)
                ws = max(ws, KINDS[kind].workspace(shape))
                KINDS[kind].prepare(shape)
                h, w = ho, wo
        return ws

    def _run_stages(self, x):
        outs = self._run_body(x)
        avgpool_fc(outs[-1], self.head_packed, self.classes, in_padded=not self.bottleneck, out=self._logits,
                   workspace=self._ws)
        return outs

    def _run_body(self, x):
        """The stem and the four stages; returns the stages' output tensors (padded for the basic-block nets)."""
        ws = self._ws
        stem(x, self.stem_packed, out_padded=not self.bottleneck, out=self._stem_out)
        cur = self._stem_out
        outs = []
        for bufs, blocks, dils in zip(self._stages, self.layers, self.dilations):
            for i, ((kind, _, _, _, p), d) in enumerate(zip(blocks, dils)):   # (bottlenecks ping-pong between the stage's two tensors)
                cur = KINDS[kind].run(cur, p, self.groups, d, bufs[i % len(bufs)], ws)
            outs.append(cur)
        return outs

    def _interior(self, t):
        return t if self.bottleneck else t[:, 1:-1, 1:-1, :]

    def forward(self, x: torch.Tensor, return_stages: bool = False):
        """x [N][3][H][W] float32 on the model's device -> logits [N][classes] (the model's own output tensor,
        rewritten by the next forward).  With return_stages, also {"stem", "layer1".."layer4"}: views of the
        activations (NHWC interiors), valid until the next forward.  A new input shape re-runs prepare()."""
        self._begin(x)
        with torch.cuda.device(self.device):
            outs = self._run_stages(x.contiguous())
        if not return_stages:
            return self._logits
        names = ["layer1", "layer2", "layer3", "layer4"]
        stages = {"stem": self._interior(self._stem_out)}
        stages.update({n: self._interior(t) for n, t in zip(names, outs)})
        return self._logits, stages

    def flops(self, H: int = 224, W: int = 224) -> float:
        """Algorithmic multiply-add FLOPs of one image (2 per MAC; convolutions and FC)."""
        shapes = stage_shapes(self.arch, H, W, self.dilate)
        Hc, Wc = _out_hw(H, W, 2)
        f = 2.0 * Hc * Wc * 64 * 147
        for (_, _, ho, wo), blocks in zip(shapes[1:], self.layers):
            for kind, cin, cm, cout, _ in blocks:
                f += 2.0 * KINDS[kind].macs(ho * wo, cin, cm, cout, self.groups)
        return f + 2.0 * self.feat_c * self.classes


__all__ = ["ARCHS", "WIDTHS", "ResNet", "stage_shapes", "dilated_block_plan", "expected_keys", "mid_channels", "validate_state_dict"]
