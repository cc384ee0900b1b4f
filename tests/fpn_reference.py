"""fp64 CPU references of the FPN neck for tests/test_gpu_fpn.py: the 1x1 layer with the upsampled residual
(WINO_RESIDUAL_UP2), one pyramid level, and torchvision's BackboneWithFPN read off a state dict -- each with
F.interpolate(mode="nearest") and F.max_pool2d(1, 2) written literally -- plus random weights in torchvision's key
names (the recipe of reference_nets.random_state_dict, extended by the FPN's convolutions)."""
import layer_refs as LR
from reference_nets import random_state_dict, reference_forward

LAYER_TOL = 2e-5   # what the project holds a single fp32 layer to (cases.TIGHT)


def up_hw(H, W):
    return (H + 1) // 2, (W + 1) // 2


def padded_nan(torch, t):
    """[N][H][W][C] -> [N][H+2][W+2][C] with a NaN ring: one ring read by a kernel shows in its result."""
    return LR.ring(t, float("nan"))


class Up2Layer:
    """One 1x1 layer Cin -> Kout on an N x H x W grid that adds the coarser map `top`; its operands as CPU masters
    (self.cpu) and device tensors (self.dev), and the fp64 result before the ReLU (self.pre, [N][H][W][Kout])."""

    def __init__(self, torch, dev, N, H, W, Cin, Kout, seed):
        self.torch, self.shape = torch, (N, H, W, Cin, Kout)
        g = torch.Generator().manual_seed(seed)
        r = lambda *sh: torch.rand(*sh, generator=g)
        Hc, Wc = up_hw(H, W)
        A = r(N, H, W, Cin) - 0.5
        B = LR.w11(r, Cin, Kout)
        b, s = LR.bn_pair(r, Kout)
        top = r(N, Hc, Wc, Kout) - 0.5
        self.cpu = {"A": A, "Ap": padded_nan(torch, A), "B": B, "b": b, "s": s, "top": padded_nan(torch, top)}
        self.dev = {k: v.to(dev) for k, v in self.cpu.items()}
        self.pre = LR.conv1x1(A, B, (b, s), False, top=top)

    def out_shape(self, pkg, flags):
        N, H, W, _, Kout = self.shape
        return (N, H + 2, W + 2, Kout) if flags & pkg.C_PADDED else (N, H, W, Kout)

    def run(self, pkg, flags, t=None, out=None):
        """`flags`: of RELU / A_PADDED / C_PADDED; the residual bits are added here.  `t`: the operands (self.dev)."""
        t = t or self.dev
        N, H, W, _, _ = self.shape
        if out is None:
            out = self.torch.full(self.out_shape(pkg, flags), float("nan"), device=t["B"].device)
        return pkg.conv1x1_bn_ex(t["Ap"] if flags & pkg.A_PADDED else t["A"], t["B"], t["b"], t["s"],
                                 flags | pkg.ADD_RESIDUAL | pkg.RESIDUAL_UP2, residual=t["top"], out=out, hw=(H, W))

    def check(self, pkg, flags, got, tag):
        torch = self.torch
        got = got.detach().cpu().double()
        if flags & pkg.C_PADDED:
            assert LR.ring_is(got, 0.0), f"{tag}: ring is not exactly 0"
            got = LR.interior(got)
        want = torch.relu(self.pre) if flags & pkg.RELU else self.pre
        assert got.shape == want.shape, f"{tag}: {tuple(got.shape)} != {tuple(want.shape)}"
        assert bool(torch.isfinite(got).all()), f"{tag}: non-finite values (not all written, or a ring was read)"
        err = LR.rel(got, want)
        print(f"{tag}: rel err {err:.3e}")
        assert err < LAYER_TOL, f"{tag}: rel err {err:.3e}"


# ---- one level ----------------------------------------------------------------------------------------------------------
def level_reference(torch, c, wl, bl, wo, bo, top_inner):
    """fp64: c [N][H][W][Cin], wl torch's [Cf][Cin][1][1], wo [Cf][Cf][3][3], top_inner [N][Hc][Wc][Cf] or None ->
    (inner, P), NHWC."""
    F = torch.nn.functional
    x = c.double().permute(0, 3, 1, 2)
    inner = F.conv2d(x, wl.double(), bl.double())
    if top_inner is not None:
        inner = inner + F.interpolate(top_inner.double().permute(0, 3, 1, 2), size=inner.shape[-2:], mode="nearest")
    P = F.conv2d(inner, wo.double(), bo.double(), padding=1)
    return inner.permute(0, 2, 3, 1), P.permute(0, 2, 3, 1)


# ---- whole backbones ------------------------------------------------------------------------------------------------------
def fpn_random_state_dict(torch, R, arch, out_channels=256, seed=0):
    """(sd, body): sd in torchvision's BackboneWithFPN key names -- body.<the recipe of random_state_dict, no fc>,
    He-scaled FPN convolutions with small biases -- and the plain ResNet state dict `body` (with an fc) the fp64
    reference forward reads."""
    body = random_state_dict(torch, R, arch, classes=8, seed=seed)
    sd = {"body." + k: v for k, v in body.items() if not k.startswith("fc.")}
    g = torch.Generator().manual_seed(seed + 4242)
    stage_c = [c for _, c, _, _ in R.stage_shapes(arch, 64, 64)[1:]]
    for i, c in enumerate(stage_c):
        sd[f"fpn.inner_blocks.{i}.0.weight"] = torch.randn(out_channels, c, 1, 1, generator=g) * (1.0 / c) ** 0.5
        sd[f"fpn.inner_blocks.{i}.0.bias"] = (torch.rand(out_channels, generator=g) - 0.5) * 0.2
        sd[f"fpn.layer_blocks.{i}.0.weight"] = (torch.randn(out_channels, out_channels, 3, 3, generator=g)
                                                * (1.0 / (9 * out_channels)) ** 0.5)
        sd[f"fpn.layer_blocks.{i}.0.bias"] = (torch.rand(out_channels, generator=g) - 0.5) * 0.2
    return sd, body


def fpn_reference_forward(torch, sd, body, x):
    """fp64 CPU forward of torchvision's BackboneWithFPN (FeaturePyramidNetwork + LastLevelMaxPool) in eval mode:
    {"0".."3", "pool"}, NHWC."""
    F = torch.nn.functional
    _, stages = reference_forward(torch, body, x)
    c = [stages[f"layer{i}"].permute(0, 3, 1, 2) for i in range(1, 5)]
    d = {k: v.double() for k, v in sd.items() if k.startswith("fpn.")}
    inner = lambda i, t: F.conv2d(t, d[f"fpn.inner_blocks.{i}.0.weight"], d[f"fpn.inner_blocks.{i}.0.bias"])
    layer = lambda i, t: F.conv2d(t, d[f"fpn.layer_blocks.{i}.0.weight"], d[f"fpn.layer_blocks.{i}.0.bias"], padding=1)
    last_inner = inner(3, c[3])
    results = [None, None, None, layer(3, last_inner)]
    for i in (2, 1, 0):
        lateral = inner(i, c[i])
        last_inner = lateral + F.interpolate(last_inner, size=lateral.shape[-2:], mode="nearest")
        results[i] = layer(i, last_inner)
    out = {str(i): t.permute(0, 2, 3, 1) for i, t in enumerate(results)}
    out["pool"] = F.max_pool2d(results[3], 1, 2, 0).permute(0, 2, 3, 1)
    return out
