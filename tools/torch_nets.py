"""Random weights in torchvision's state-dict formats and the torch comparator of the tools/*_bench.py tools: eager torch
on channels-last fp32 with the same weights -- conv, BN as scale and bias, ReLU, add.  One ResNet body (plain, grouped,
wide or dilated, read off the weights and the dilation flags) and the heads as functions over its four stage outputs.
tests/test_tools_host.py holds all of it to the test suite's fp64 references."""
import torch
import torch.nn.functional as F

NO_DILATION = (False, False, False)
SEGMENTATION_DILATE = (False, True, True)   # torchvision's fcn_resnet* and deeplabv3_resnet*: output stride 8
FPN_CHANNELS = 256
ASPP_CIN, ASPP_CB = 2048, 256
ASPP_RATES = (12, 24, 36)


def image_batch(N, H, W, dev):
    """(x, x channels-last): the tools' input, uniform in [-1, 1), seeded with N."""
    x = (torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(N)) * 2 - 1).to(dev)
    return x, x.contiguous(memory_format=torch.channels_last)


# ---- state dicts -------------------------------------------------------------------------------------------------------
def random_state_dict(R, arch, seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in R.expected_keys(arch, 1000).items():
        if k.endswith(".weight") and len(shape) == 4:
            sd[k] = torch.randn(shape, generator=g) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
        elif k.endswith("running_var"):
            sd[k] = torch.rand(shape, generator=g) + 0.5
        elif k == "fc.weight":
            sd[k] = torch.randn(shape, generator=g) * (1.0 / shape[1]) ** 0.5
        elif k.endswith(".weight"):
            sd[k] = (torch.rand(shape, generator=g) + 0.5) * (0.2 if k.endswith(("bn3.weight",)) or
                                                               (k.endswith("bn2.weight") and "layer" in k and
                                                                not R.ARCHS[arch][0]) else 1.0)
        else:
            sd[k] = (torch.rand(shape, generator=g) - 0.5) * 0.2
    return sd


def fpn_state_dict(R, arch, seed=1):
    """(sd in BackboneWithFPN's key names, the plain ResNet dict of its body)."""
    CF = FPN_CHANNELS
    body = random_state_dict(R, arch, seed=seed)
    sd = {"body." + k: v for k, v in body.items() if not k.startswith("fc.")}
    g = torch.Generator().manual_seed(seed + 1)
    for i, (_, c, _, _) in enumerate(R.stage_shapes(arch, 64, 64)[1:]):
        sd[f"fpn.inner_blocks.{i}.0.weight"] = torch.randn(CF, c, 1, 1, generator=g) * (1.0 / c) ** 0.5
        sd[f"fpn.inner_blocks.{i}.0.bias"] = (torch.rand(CF, generator=g) - 0.5) * 0.2
        sd[f"fpn.layer_blocks.{i}.0.weight"] = torch.randn(CF, CF, 3, 3, generator=g) * (1.0 / (9 * CF)) ** 0.5
        sd[f"fpn.layer_blocks.{i}.0.bias"] = (torch.rand(CF, generator=g) - 0.5) * 0.2
    return sd, body


def fcn_state_dict(R, arch, classes=21, seed=1):
    g = torch.Generator().manual_seed(seed + 100)
    sd = {"backbone." + k: v for k, v in random_state_dict(R, arch, seed).items() if not k.startswith("fc.")}
    sd["classifier.0.weight"] = torch.randn(512, 2048, 3, 3, generator=g) * (2.0 / (2048 * 9)) ** 0.5
    sd["classifier.1.weight"] = torch.rand(512, generator=g) + 0.5
    sd["classifier.1.bias"] = (torch.rand(512, generator=g) - 0.5) * 0.2
    sd["classifier.1.running_mean"] = (torch.rand(512, generator=g) - 0.5) * 0.2
    sd["classifier.1.running_var"] = torch.rand(512, generator=g) + 0.5
    sd["classifier.4.weight"] = torch.randn(classes, 512, 1, 1, generator=g) * (1.0 / 512) ** 0.5
    sd["classifier.4.bias"] = torch.rand(classes, generator=g) - 0.5
    return sd


def deeplab_state_dict(R, arch, classes=21, seed=1):
    CIN, CB = ASPP_CIN, ASPP_CB
    g = torch.Generator().manual_seed(seed + 200)
    sd = {k: v for k, v in fcn_state_dict(R, arch, classes, seed).items() if not k.startswith("classifier.")}

    def conv_bn(conv, bn, shape):
        sd[conv + ".weight"] = torch.randn(shape, generator=g) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
        sd[bn + ".weight"] = torch.rand(shape[0], generator=g) + 0.5
        sd[bn + ".bias"] = (torch.rand(shape[0], generator=g) - 0.5) * 0.2
        sd[bn + ".running_mean"] = (torch.rand(shape[0], generator=g) - 0.5) * 0.2
        sd[bn + ".running_var"] = torch.rand(shape[0], generator=g) + 0.5

    a = "classifier.0."
    conv_bn(a + "convs.0.0", a + "convs.0.1", (CB, CIN, 1, 1))
    for i in (1, 2, 3):
        conv_bn(a + f"convs.{i}.0", a + f"convs.{i}.1", (CB, CIN, 3, 3))
    conv_bn(a + "convs.4.1", a + "convs.4.2", (CB, CIN, 1, 1))
    conv_bn(a + "project.0", a + "project.1", (CB, 5 * CB, 1, 1))
    conv_bn("classifier.1", "classifier.2", (CB, CB, 3, 3))
    sd["classifier.4.weight"] = torch.randn(classes, CB, 1, 1, generator=g) * (1.0 / CB) ** 0.5
    sd["classifier.4.bias"] = torch.rand(classes, generator=g) - 0.5
    return sd


def vgg_state_dict(V, arch, g):
    """He-scaled weights, zero biases, drawn from the generator g (vgg_bench goes on to draw its inputs from it)."""
    sd = {}
    for k, shape in V.expected_keys(arch, 1000, 4096).items():
        fan = shape[1] * (9 if len(shape) == 4 else 1) if len(shape) > 1 else 1
        sd[k] = torch.randn(shape, generator=g) * (2.0 / fan) ** 0.5 if len(shape) > 1 else torch.zeros(shape)
    return sd


# ---- the comparator ------------------------------------------------------------------------------------------------------
class TorchResNetBody:
    """The stem and the four stages of a torchvision ResNet, ResNeXt or Wide ResNet whose keys start with `prefix`;
    `dilate` is torchvision's replace_stride_with_dilation.  Holds every tensor of sd on dev (self.w, 4-d ones
    channels-last) and every BN as (scale, bias) (self.bn), for the heads below to use too."""

    def __init__(self, R, sd, arch, dev, prefix="", dilate=NO_DILATION, eps=1e-5):
        self.prefix = prefix
        self.bottleneck, blocks = R.ARCHS[arch]
        if any(dilate):   # per block (stride, dilation): torchvision's _make_layer rule
            self.plan = [[(2 if kind == "proj_v15" else 1, d) for kind, d in stage]
                         for stage in R.dilated_block_plan(dilate, blocks)]
        else:             # stride 2 on the first block of layers 2 to 4
            self.plan = [[(2 if (b == 0 and L > 1) else 1, 1) for b in range(nb)] for L, nb in enumerate(blocks, 1)]
        self.w = {k: v.to(dev).contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v.to(dev)
                  for k, v in sd.items()}
        self.bn = {}
        for k in sd:
            if k.endswith("running_var"):
                p = k[: -len(".running_var")]
                s = sd[p + ".weight"] / torch.sqrt(sd[k] + eps)
                self.bn[p] = (s.to(dev)[None, :, None, None], (sd[p + ".bias"] - sd[p + ".running_mean"] * s)
                              .to(dev)[None, :, None, None])

    def cb(self, t, conv, bn, stride=1, pad=0, dil=1, relu=True):
        """conv (its groups read off the weight), BN as scale and bias, ReLU."""
        s, b = self.bn[bn]
        w = self.w[conv]
        y = F.conv2d(t, w, stride=stride, padding=pad, dilation=dil, groups=t.shape[1] // w.shape[1]) * s + b
        return torch.relu(y) if relu else y

    def __call__(self, x):
        """The outputs of layer1..layer4.  The stride sits on the 3x3 of a bottleneck, on conv1 of a basic block."""
        q, cb = self.prefix, self.cb
        t = F.max_pool2d(cb(x, q + "conv1.weight", q + "bn1", 2, 3), 3, 2, 1)
        stages = []
        for L, stage in enumerate(self.plan, 1):
            for b, (st, d) in enumerate(stage):
                p = f"{q}layer{L}.{b}"
                if self.bottleneck:
                    y = cb(t, p + ".conv1.weight", p + ".bn1")
                    y = cb(y, p + ".conv2.weight", p + ".bn2", st, d, d)
                    y = cb(y, p + ".conv3.weight", p + ".bn3", relu=False)
                else:
                    y = cb(t, p + ".conv1.weight", p + ".bn1", st, 1)
                    y = cb(y, p + ".conv2.weight", p + ".bn2", 1, 1, relu=False)
                sc = t
                if p + ".downsample.0.weight" in self.w:
                    sc = cb(t, p + ".downsample.0.weight", p + ".downsample.1", st, relu=False)
                t = torch.relu(y + sc)
            stages.append(t)
        return stages


def classifier_head(body, stages):
    return F.linear(stages[3].mean(dim=(2, 3)), body.w["fc.weight"], body.w["fc.bias"])


def fpn_head(body, stages):
    """torchvision's FeaturePyramidNetwork and LastLevelMaxPool written out: levels 0..3 and the pool."""
    conv = lambda t, k, pad: F.conv2d(t, body.w[f"fpn.{k}.0.weight"], body.w[f"fpn.{k}.0.bias"], padding=pad)
    last = conv(stages[3], "inner_blocks.3", 0)
    out = [None, None, None, conv(last, "layer_blocks.3", 1)]
    for i in (2, 1, 0):
        lat = conv(stages[i], f"inner_blocks.{i}", 0)
        last = lat + F.interpolate(last, size=lat.shape[-2:], mode="nearest")
        out[i] = conv(last, f"layer_blocks.{i}", 1)
    return out + [F.max_pool2d(out[3], 1, 2, 0)]


def resize(t, size):
    return F.interpolate(t, size=size, mode="bilinear", align_corners=False)


def fcn_head(body, stages, size):
    t = body.cb(stages[3], "classifier.0.weight", "classifier.1", 1, 1)
    return resize(F.conv2d(t, body.w["classifier.4.weight"], body.w["classifier.4.bias"]), size)


def deeplab_head(body, stages, size):
    """ASPP, the 3x3 head and the classes."""
    t, a = stages[3], "classifier.0."
    br = [body.cb(t, a + "convs.0.0.weight", a + "convs.0.1")]
    for i, d in zip((1, 2, 3), ASPP_RATES):
        br.append(body.cb(t, a + f"convs.{i}.0.weight", a + f"convs.{i}.1", 1, d, d))
    pooled = body.cb(F.adaptive_avg_pool2d(t, 1), a + "convs.4.1.weight", a + "convs.4.2")
    br.append(pooled.expand(-1, -1, t.shape[2], t.shape[3]))
    t = body.cb(torch.cat(br, dim=1), a + "project.0.weight", a + "project.1")
    t = body.cb(t, "classifier.1.weight", "classifier.2", 1, 1)
    return resize(F.conv2d(t, body.w["classifier.4.weight"], body.w["classifier.4.bias"]), size)


def torch_vgg(sd, V, arch, dev):
    """A VGG without BN as a function of the channels-last input: F.conv2d + bias + relu + max_pool2d + linear."""
    assert not V.ARCHS[arch][1], f"{arch}: the BN variants are not written out here"
    convs = [(sd[f"features.{i}.weight"].to(dev).contiguous(memory_format=torch.channels_last),
              sd[f"features.{i}.bias"].to(dev), pool) for i, _, _, pool in V.conv_layers(arch)]
    fcs = [(sd[f"classifier.{i}.weight"].to(dev), sd[f"classifier.{i}.bias"].to(dev)) for i in (0, 3, 6)]

    def forward(x_cl):
        t = x_cl
        for w, b, pool in convs:
            t = torch.relu(F.conv2d(t, w, b, padding=1))
            if pool:
                t = F.max_pool2d(t, 2, 2)
        t = F.adaptive_avg_pool2d(t, (7, 7)).flatten(1)
        for i, (w, b) in enumerate(fcs):
            t = F.linear(t, w, b)
            if i < 2:
                t = torch.relu(t)
        return t
    return forward
