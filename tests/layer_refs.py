"""The single fp64 definition of what each ResNet / VGG layer and block computes, shared by every suite (tests/cases.py,
tests/nonfinite.py, tests/sweep_cases.py and the layers' own GPU tests) and pinned against restatements without
F.conv2d in tests/test_layer_refs_host.py.  torch and numpy only: no GPU, no library.

One convention throughout.  Activations are NHWC interiors without rings, fp32 or fp64 (torch or numpy) in, fp64 torch
out, NHWC; the stem's input alone is NCHW.  3x3 and 7x7 weights are torch's [K][C/groups][kh][kw], as is the 1x1
shortcut `wd` of the stride-2 layers (every suite draws it that way); the other 1x1 weights are the library's
[Cin][Cout].  BN is the project's (bias, scale) pair.  Everything is torch fp64 ops, so NaN and Inf propagate as torch
propagates them (tests/nonfinite.py relies on it), in one order: conv * scale + bias, + residual, ReLU, pool.
`pre=True` returns a block's sum before its last ReLU; a single layer's is `relu=False`.

The segmentation and detection layers keep their own single definitions: dilated_cases.dilated_reference,
aspp_cases.cat_reference and aspp_reference, resize_cases.resize_reference, roi_cases.*_reference,
fpn_reference.level_reference."""
import numpy as np
import torch

F = torch.nn.functional


# ---- small pieces ----------------------------------------------------------------------------------------------------
def f64(a):
    """A torch fp64 CPU tensor of a torch tensor (any device) or a numpy array."""
    if hasattr(a, "detach"):
        return a.detach().cpu().double()
    return torch.from_numpy(np.array(a, np.float64))   # (a copy: a read-only array is no tensor's storage)


def nchw(x_nhwc):
    return f64(x_nhwc).permute(0, 3, 1, 2)


def nhwc(y_nchw):
    return y_nchw.permute(0, 2, 3, 1).contiguous()


def affine(y_nchw, bn):
    bias, scale = bn
    return y_nchw * f64(scale)[None, :, None, None] + f64(bias)[None, :, None, None]


def w1x1(w_io):
    """[Cin][Cout] (the library's 1x1 layout) -> [Cout][Cin][1][1]."""
    return f64(w_io).t()[:, :, None, None]


def ring(x_nhwc, value=0.0):
    """[N][H][W][C] -> [N][H+2][W+2][C] with the ring set to `value`."""
    return F.pad(x_nhwc, (0, 0, 1, 1, 1, 1), value=value)


def fill_ring(xp, value=0.0):
    """The ring of a padded [N][H+2][W+2][C] tensor set to `value` in place (no copy: the > 4 GiB tests)."""
    for r in (xp[:, 0], xp[:, -1], xp[:, :, 0], xp[:, :, -1]):
        r.fill_(value)
    return xp


def interior(xp):
    return xp[:, 1:-1, 1:-1, :]


def ring_mask(H=14, W=14):
    """The ring pixels of a padded [H+2][W+2] map, as a numpy bool mask."""
    r = np.ones((H + 2, W + 2), bool)
    r[1:-1, 1:-1] = False
    return r


def ring_is(t, value=0.0):
    """The ring of a padded [N][H+2][W+2][C] tensor or array is exactly `value`."""
    return all(bool((r == value).all()) for r in (t[:, 0], t[:, -1], t[:, :, 0], t[:, :, -1]))


def rel(got, want, floor=0.0):
    """max |got - want| / max(max |want|, floor) in fp64; the shapes agree and both sides are finite (no NaN, and no Inf
    either: inf - inf must never pass a tolerance comparison)."""
    g, w = f64(got), f64(want)
    assert g.shape == w.shape, (tuple(g.shape), tuple(w.shape))
    assert bool(torch.isfinite(g).all()), "got holds non-finite values"
    assert bool(torch.isfinite(w).all()), "the reference holds non-finite values"
    return float((g - w).abs().max() / max(float(w.abs().max()), floor))


# ---- the shared draws: `rand(*shape)` is the caller's generator, uniform in [0, 1) -----------------------------------
def conv_w(rand, K, C, k=3):
    return (rand(K, C, k, k) - 0.5) / np.sqrt(k * k * C) * 4


def w11(rand, i, o, gain=4):
    return (rand(i, o) - 0.5) / np.sqrt(i) * gain


def bn_pair(rand, K, negative_third=True):
    """(bias, scale), bias first; a negative scale on every third channel."""
    bias, scale = rand(K) - 0.5, rand(K) + 0.5
    if negative_third:
        scale[::3] *= -1
    return bias, scale


# ---- the layers ------------------------------------------------------------------------------------------------------
def _conv(x_nchw, w, bn, stride=1, padding=1, groups=1):
    return affine(F.conv2d(x_nchw, f64(w), stride=stride, padding=padding, groups=groups), bn)


def conv3x3(x, w, bn, relu, stride=1, groups=1, residual=None, pool=False, padding=1):
    """3x3 (pad 1) + BN (+ residual) (+ ReLU) (+ 2x2 max-pool; an odd last row or column is dropped).  padding=0: `x`
    brings its border along (a padded tensor with its zero ring, or a band of rows cut from a larger padded map)."""
    y = _conv(nchw(x), w, bn, stride, padding, groups)
    if residual is not None:
        y = y + nchw(residual)
    if relu:
        y = torch.relu(y)
    return nhwc(F.max_pool2d(y, 2, 2) if pool else y)


def conv1x1(x, w_io, bn, relu, stride=1, residual=None, top=None):
    """1x1 + BN (+ residual) (+ `top`, the coarser map, added at (y >> 1, x >> 1)) (+ ReLU)."""
    y = _conv(nchw(x), w1x1(w_io), bn, stride, 0)
    if residual is not None:
        y = y + nchw(residual)
    if top is not None:
        y = y + F.interpolate(nchw(top), size=y.shape[-2:], mode="nearest")
    return nhwc(torch.relu(y) if relu else y)


def basic_block(x, w1, bn1, w2, bn2, blocks=1, pre=False):
    """relu(BN(3x3(relu(BN(3x3(x))))) + x), `blocks` times in a row."""
    x = nchw(x)
    for _ in range(blocks):
        y = _conv(torch.relu(_conv(x, w1, bn1)), w2, bn2) + x
        x = torch.relu(y)
    return nhwc(y if pre else x)


def basic_block_s2(x, w1, bn1, wd, bnd, w2=None, bn2=None, pre=False):
    """(t1, sc, out) of the downsampling basic block: t1 the stride-2 3x3 + BN + ReLU, sc the stride-2 1x1 shortcut + BN
    of the same input (the fused layer conv3x3_s2_proj stops there: no `w2`, out None), out = relu(BN(3x3(t1)) + sc)."""
    xi = nchw(x)
    t1, sc = torch.relu(_conv(xi, w1, bn1, 2)), _conv(xi, wd, bnd, 2, 0)
    if w2 is None:
        return nhwc(t1), nhwc(sc), None
    y = _conv(t1, w2, bn2) + sc
    return nhwc(t1), nhwc(sc), nhwc(y if pre else torch.relu(y))


def bottleneck(x, w1, bn1, w2, bn2, w3, bn3, wp=None, bnp=None, stride=1, stride_on="first", groups=1, pre=False):
    """1x1 + BN + ReLU, 3x3 (grouped) + BN + ReLU, 1x1 + BN, + x (identity: no `wp`) or + BN(1x1 projection of x at
    `stride`), ReLU.  The stride is on the first 1x1 (v1) or on the 3x3 (v1.5, ResNeXt)."""
    assert stride_on in ("first", "3x3")
    xi = nchw(x)
    if stride_on == "first":
        xi, stride = xi[:, :, ::stride, ::stride], 1
    t1 = torch.relu(_conv(xi, w1x1(w1), bn1, 1, 0))
    t2 = torch.relu(_conv(t1, w2, bn2, stride, 1, groups))
    y = _conv(t2, w1x1(w3), bn3, 1, 0) + (xi if wp is None else _conv(xi, w1x1(wp), bnp, stride, 0))
    return nhwc(y if pre else torch.relu(y))


def stem(x_nchw, w, bn, pre=False):
    """7x7 / stride 2 / pad 3 + BN + ReLU + 3x3 / stride 2 / pad 1 max-pool; NCHW in, NHWC out (`pre`: the BN's output,
    before the ReLU and the pool)."""
    y = _conv(f64(x_nchw), w, bn, 2, 3)
    return nhwc(y if pre else F.max_pool2d(torch.relu(y), 3, 2, 1))


def avgpool_fc(feat, wfc, bfc):
    """[N][H][W][C] -> the mean over the map, then the classifier [classes][C] and its bias: [N][classes]."""
    return f64(feat).mean(dim=(1, 2)) @ f64(wfc).t() + f64(bfc)


def avgpool7(feat):
    """AdaptiveAvgPool2d(7): [N][H][W][C] -> [N][7][7][C]."""
    return nhwc(F.adaptive_avg_pool2d(nchw(feat), (7, 7)))
