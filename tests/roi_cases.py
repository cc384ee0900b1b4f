"""What the RoIAlign and R-CNN head tests share (tests/test_roi_host.py, test_gpu_roi_align.py, test_gpu_roi_heads.py):
the fp64 references in torch -- roi_align_reference (torchvision's CPU kernel, aligned=False, vectorised; the same
function in torch.float32 is the "straight fp32 restatement"), torchvision's level formula evaluated literally, the
thresholds rule of csrc/roi_align.hip restated, box_head_reference and mask_head_reference -- the base pyramid, and the
seeded box generator with its redraw rule.  Nothing here needs a GPU or the library to import."""
import functools
import math

import numpy as np
import torch

# ---- the base pyramid ------------------------------------------------------------------------------------------------------
IMAGE = (64, 48)                                   # H, W of the image the boxes live in
LEVEL_HW = ((16, 12), (8, 6), (4, 3), (2, 2))      # (h, w) of the four levels, strides 4 .. 32
SCALES = (1 / 4, 1 / 8, 1 / 16, 1 / 32)
N_IMAGES = 2
CHANNELS = (8, 64, 320)                            # 320: the lanes walk a second, partial 256-channel slab
CANONICAL_SCALE, CANONICAL_LEVEL = 16.0, 4         # boxes inside a 64 x 48 image reach all four levels
PS_COMBOS = tuple((P, S) for P in (1, 7, 14) for S in (1, 2, 3))     # what the parity test runs
EXACT_COMBOS = tuple((P, S) for P in (2, 4, 8) for S in (1, 2))      # ... and the exact-geometry subset
SAMPLE_MARGIN = 1e-3     # the redraw rule: no fp64 sample coordinate this close to -1 or to h / w
LEVEL_MARGIN = 1e-4      # ... and canonical_level + log2(sqrt(area) / canonical_scale) not this close to an integer
EXACT_TOL = 1e-6         # the exact-geometry subset: every coordinate and weight is exact in fp32


def pyramid(C, seed=0, hw=LEVEL_HW, N=N_IMAGES):
    """The level maps [N][h][w][C], float32, uniform in [-0.5, 0.5)."""
    g = torch.Generator().manual_seed(1000 * seed + C)
    return [torch.rand(N, h, w, C, generator=g) - 0.5 for h, w in hw]


def padded_nan(t):
    """[N][h][w][C] -> [N][h+2][w+2][C] with a NaN ring: one ring read by the kernel shows in its result."""
    N, h, w, C = t.shape
    p = torch.full((N, h + 2, w + 2, C), float("nan"), dtype=t.dtype)
    p[:, 1:-1, 1:-1, :] = t
    return p


# ---- levels ------------------------------------------------------------------------------------------------------------------
def torchvision_levels(rois, scales, canonical_scale=CANONICAL_SCALE, canonical_level=CANONICAL_LEVEL,
                       dtype=torch.float64):
    """torchvision's LevelMapper, literally, in `dtype`: floor(lvl0 + log2(sqrt(area) / s0) + eps) clamped to
    [k_min, k_max], minus k_min.  The area is that of the fp32 boxes computed in `dtype`.  Where torch's own result is
    undefined (area <= 0 or NaN: log2 gives -Inf / NaN) the level is 0, the library's rule."""
    if len(scales) == 1:
        return torch.zeros(rois.shape[0], dtype=torch.int64)
    k_min, k_max = -math.log2(scales[0]), -math.log2(scales[-1])
    b = rois.to(dtype)
    area = (b[:, 3] - b[:, 1]) * (b[:, 4] - b[:, 2])
    s = torch.sqrt(area)
    lvl = torch.floor(canonical_level + torch.log2(s / canonical_scale) + torch.tensor(1e-6, dtype=dtype))
    lvl = torch.clamp(lvl, min=k_min, max=k_max) - k_min
    return torch.where(area > 0, lvl, torch.zeros_like(lvl)).to(torch.int64)


def level_thresholds(scales, canonical_scale=CANONICAL_SCALE, canonical_level=CANONICAL_LEVEL):
    """The library's rule: the levels - 1 area thresholds (canonical_scale 2^(k0 + j - canonical_level - 1e-6))^2 in
    double, rounded to float32."""
    k0 = round(-math.log2(scales[0]))
    return [np.float32((canonical_scale * 2.0 ** (k0 + j - canonical_level - 1e-6)) ** 2) for j in range(1, len(scales))]


def threshold_levels(rois, scales, canonical_scale=CANONICAL_SCALE, canonical_level=CANONICAL_LEVEL):
    """A box's level is the number of thresholds its fp32 area reaches; an area <= 0 or NaN reaches none."""
    b = rois.to(torch.float32)
    area = (b[:, 3] - b[:, 1]) * (b[:, 4] - b[:, 2])
    lvl = torch.zeros(rois.shape[0], dtype=torch.int64)
    for t in level_thresholds(scales, canonical_scale, canonical_level):
        lvl += (area >= float(t)).to(torch.int64)
    return lvl


# ---- RoIAlign ----------------------------------------------------------------------------------------------------------------
def sample_coords(rois, scale, P, S, dtype=torch.float64):
    """(ys, xs) [R][P][S]: the sample coordinates of every bin, torchvision's operations in `dtype`.  `scale`: one number
    or a tensor [R]."""
    b = rois.to(dtype)
    sc = torch.as_tensor(scale, dtype=dtype)
    sx, sy, ex, ey = b[:, 1] * sc, b[:, 2] * sc, b[:, 3] * sc, b[:, 4] * sc
    one = torch.ones((), dtype=dtype)
    bin_w, bin_h = torch.maximum(ex - sx, one) / P, torch.maximum(ey - sy, one) / P
    p = torch.arange(P, dtype=dtype)[None, :, None]
    i = (torch.arange(S, dtype=dtype) + 0.5)[None, None, :]
    ys = sy[:, None, None] + p * bin_h[:, None, None] + i * bin_h[:, None, None] / S
    xs = sx[:, None, None] + p * bin_w[:, None, None] + i * bin_w[:, None, None] / S
    return ys, xs


def _axis_weights(v, size):
    """v [R][P][S] sample coordinates along an axis of `size` pixels -> (W, T) [R][P][size]: the summed weight of every
    pixel over the bin's in-range samples, and whether an in-range sample taps it (a tap of weight zero included)."""
    ok = (v >= -1) & (v <= size)
    c = torch.where(ok, v.clamp(min=0), torch.zeros_like(v))
    low = c.floor().to(torch.int64)
    edge = low >= size - 1
    low = torch.where(edge, torch.full_like(low, size - 1), low)
    high = torch.where(edge, low, low + 1)
    c = torch.where(edge, low.to(v.dtype), c)
    l = c - low.to(v.dtype)
    okf = ok.to(v.dtype)
    W = torch.zeros(v.shape[0], v.shape[1], size, dtype=v.dtype)
    W.scatter_add_(2, low, (1 - l) * okf)
    W.scatter_add_(2, high, l * okf)
    T = torch.zeros(v.shape[0], v.shape[1], size, dtype=v.dtype)
    T.scatter_add_(2, low, okf)
    T.scatter_add_(2, high, okf)
    return W, T > 0


def roi_align_reference(maps, rois, P, scales, sampling, levels, dtype=torch.float64, taps=False):
    """torchvision's roi_align(aligned=False) of every box on its level: maps [N][h][w][C] per level (unpadded), rois
    [R][5], `levels` [R] int64 -> [R][P][P][C] in `dtype`.  Separable: a bin's sum over its samples is Wy (x) Wx applied to
    the image, because a sample counts iff it is in range along both axes.  The library's rules for what torchvision
    leaves undefined: a batch index that is not an integer in [0, N) gives zeros, otherwise a non-finite coordinate NaN.
    With taps=True returns (out, touched): touched[r] = (level, image, Ty [P][h], Tx [P][w]) or None for a box that
    reads nothing -- output (r, ph, pw) reads pixel (y, x) of that map iff Ty[ph][y] and Tx[pw][x].  The maps must be
    finite (a zero weight times NaN would spread over the whole image here)."""
    R, C, N = rois.shape[0], maps[0].shape[3], maps[0].shape[0]
    out = torch.zeros(R, P, P, C, dtype=dtype)
    touched = [None] * R
    b = rois.to(torch.float64)
    bi = b[:, 0]
    image_ok = (bi >= 0) & (bi < N) & (bi == bi.floor())
    finite = torch.isfinite(b[:, 1:]).all(dim=1)
    out[image_ok & ~finite] = float("nan")
    good = image_ok & finite
    for l, m in enumerate(maps):
        sel = torch.nonzero(good & (levels == l)).flatten()
        if sel.numel() == 0:
            continue
        h, w = int(m.shape[1]), int(m.shape[2])
        ys, xs = sample_coords(rois[sel], scales[l], P, sampling, dtype)
        Wy, Ty = _axis_weights(ys, h)
        Wx, Tx = _axis_weights(xs, w)
        img = bi[sel].to(torch.int64)
        out[sel] = torch.einsum("rph,rqw,rhwc->rpqc", Wy, Wx, m.to(dtype)[img]) / (sampling * sampling)
        if taps:
            for j, r in enumerate(sel.tolist()):
                touched[r] = (l, int(img[j]), Ty[j], Tx[j])
    return (out, touched) if taps else out


def rel_err(got, want):
    """max |got - want| / max |want| of two tensors; both finite."""
    got, want = got.detach().cpu().double(), want.double()
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    assert bool(torch.isfinite(got).all()), "got holds non-finite values"
    assert bool(torch.isfinite(want).all()), "the reference holds non-finite values"
    return float((got - want).abs().max() / want.abs().max())


# ---- the box generator ---------------------------------------------------------------------------------------------------------
# (class, image, x1, y1, x2, y2) in image pixels.  The classes' properties are checked by tests/test_roi_host.py at P = 7,
# sampling = 2 (class_properties below).
TABLE = (
    ("interior_l0", 0, 5.3, 7.1, 11.9, 12.7), ("interior_l0", 1, 20.7, 30.2, 27.1, 36.9),
    ("interior_l1", 0, 10.2, 20.3, 21.4, 31.9), ("interior_l1", 1, 14.6, 9.8, 27.3, 22.1),
    ("interior_l2", 0, 8.5, 12.5, 30.1, 35.3), ("interior_l2", 1, 6.2, 20.4, 27.9, 44.6),
    ("interior_l3", 0, 1.3, 2.1, 46.7, 30.9), ("interior_l3", 1, 2.2, 8.4, 31.7, 60.3),
    ("clamp_left", 0, -3.1, 20.3, 3.3, 26.1), ("clamp_left", 1, -2.2, 40.4, 4.1, 45.7),
    ("clamp_top", 0, 13.3, -2.9, 19.1, 3.7), ("clamp_top", 1, 30.6, -1.7, 36.2, 4.9),
    ("clamp_right", 0, 41.3, 10.2, 47.6, 16.5), ("clamp_right", 1, 40.9, 50.3, 47.1, 56.2),
    ("clamp_bottom", 0, 10.4, 57.3, 16.9, 63.5), ("clamp_bottom", 1, 22.2, 56.9, 28.7, 63.1),
    ("zero_left", 0, -9.3, 8.2, -2.9, 14.3), ("zero_left", 1, -7.7, 33.1, -0.6, 38.4),
    ("zero_top", 0, 25.1, -8.8, 31.3, -2.1), ("zero_top", 1, 5.2, -7.4, 11.7, -0.9),
    ("zero_right", 0, 44.7, 21.3, 51.9, 26.8), ("zero_right", 1, 46.2, 3.3, 53.1, 9.6),
    ("zero_bottom", 0, 17.3, 61.1, 23.8, 68.4), ("zero_bottom", 1, 33.3, 62.2, 39.1, 69.9),
    ("outside", 0, 70.3, 80.1, 76.2, 86.7), ("outside", 1, -30.2, -25.3, -24.1, -19.4),
    ("outside", 0, 100.5, 120.5, 150.5, 170.5),
    ("thin", 0, 10.3, 20.1, 10.9, 26.3), ("thin", 1, 30.2, 40.7, 36.6, 41.2),
    ("flipped", 0, 20.5, 30.5, 14.2, 36.3), ("flipped", 1, 8.4, 44.1, 14.6, 38.9),      # x2 < x1; y2 < y1: area < 0
    ("flipped", 1, 25.5, 35.5, 20.1, 29.9), ("flipped", 0, 30.3, 20.2, 30.3, 20.2),      # both: area > 0; a point: area 0
    ("threshold_8", 0, 4.0, 8.0, 12.0, 16.0), ("threshold_8", 1, 10.0, 20.0, 26.0, 24.0),
    ("threshold_16", 0, 8.0, 16.0, 24.0, 32.0), ("threshold_16", 1, 2.0, 30.0, 34.0, 38.0),
    ("threshold_32", 0, 8.0, 16.0, 40.0, 48.0), ("threshold_32", 1, 0.0, 0.0, 64.0, 16.0),
    # edges on multiples of the level's stride: with P a power of two and sampling 1 or 2 every sample is dyadic
    ("exact", 0, 8.0, 12.0, 12.0, 20.0), ("exact", 1, 16.0, 24.0, 20.0, 28.0), ("exact", 0, -4.0, 4.0, 4.0, 8.0),
    ("exact", 0, 8.0, 16.0, 24.0, 24.0), ("exact", 1, 16.0, 8.0, 24.0, 32.0),
    ("exact", 0, 16.0, 16.0, 32.0, 48.0), ("exact", 1, 0.0, 16.0, 32.0, 32.0),
    ("exact", 0, 0.0, 0.0, 32.0, 64.0), ("exact", 1, 0.0, 0.0, 64.0, 32.0),
)
CLASSES = tuple(dict.fromkeys(row[0] for row in TABLE)) + ("random",)
N_RANDOM = 40


def min_sample_margin(rois, levels, combos, hw=LEVEL_HW, scales=SCALES):
    """[R]: the distance of each box's closest fp64 sample coordinate, over `combos` of (P, sampling), to -1 or to its
    level's h (y) / w (x): where RoIAlign is discontinuous."""
    m = torch.full((rois.shape[0],), float("inf"), dtype=torch.float64)
    sc = torch.tensor(scales, dtype=torch.float64)[levels]
    hh = torch.tensor([s[0] for s in hw], dtype=torch.float64)[levels][:, None]
    ww = torch.tensor([s[1] for s in hw], dtype=torch.float64)[levels][:, None]
    for P, S in combos:
        ys, xs = sample_coords(rois, sc, P, S)
        ys, xs = ys.flatten(1), xs.flatten(1)
        d = torch.cat([(ys + 1).abs(), (ys - hh).abs(), (xs + 1).abs(), (xs - ww).abs()], dim=1).min(dim=1).values
        m = torch.minimum(m, d)
    return m


def level_margin(rois, scales=SCALES):
    """[R]: the distance of canonical_level + log2(sqrt(area) / canonical_scale) to the nearest integer at which the level
    changes, k_min + 1 .. k_max (Inf for area <= 0)."""
    b = rois.to(torch.float64)
    area = (b[:, 3] - b[:, 1]) * (b[:, 4] - b[:, 2])
    k = CANONICAL_LEVEL + torch.log2(torch.sqrt(area.clamp(min=1e-300)) / CANONICAL_SCALE)
    k_min = round(-math.log2(scales[0]))
    edges = torch.arange(k_min + 1, k_min + len(scales), dtype=torch.float64)
    d = (k[:, None] - edges[None, :]).abs().min(dim=1).values
    return torch.where(area > 0, d, torch.full_like(k, float("inf")))


class Boxes:
    """The named table plus N_RANDOM seeded random boxes (log-uniform in size, so that all four levels are hit): rois
    [R][5] float32, names [R], levels [R] (fp64 formula), drawn / redrawn counts of the random part."""

    def __init__(self, seed=0):
        g = torch.Generator().manual_seed(seed)
        rows, names = [list(r[1:]) for r in TABLE], [r[0] for r in TABLE]
        self.drawn = self.redrawn = 0
        H, W = IMAGE
        while len(rows) < len(TABLE) + N_RANDOM:
            u = torch.rand(6, generator=g, dtype=torch.float64).tolist()
            size = 3.0 * (60.0 / 3.0) ** u[0]                  # sqrt(area), log-uniform in [3, 60]
            aspect = math.exp(1.4 * u[1] - 0.7)
            bw, bh = size * math.sqrt(aspect), size / math.sqrt(aspect)
            cx, cy = -4 + (W + 8) * u[2], -4 + (H + 8) * u[3]
            row = [float(int(u[4] * N_IMAGES)), cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2]
            self.drawn += 1
            roi = torch.tensor([row], dtype=torch.float32)     # (the margins are those of the fp32 box the kernel gets)
            lvl = torchvision_levels(roi, SCALES)
            if (float(min_sample_margin(roi, lvl, PS_COMBOS)) < SAMPLE_MARGIN
                    or float(level_margin(roi)) < LEVEL_MARGIN):
                self.redrawn += 1
                continue
            rows.append(row)
            names.append("random")
        self.rois = torch.tensor(rows, dtype=torch.float32)
        self.names = names
        self.levels = torchvision_levels(self.rois, SCALES)

    def index(self, name):
        return [i for i, n in enumerate(self.names) if n == name]


@functools.lru_cache(maxsize=None)
def boxes(seed=0):
    return Boxes(seed)


def class_properties(bx, P=7, S=2):
    """{class: [bool per box of the class]}: whether each table box has the property its class is named for."""
    res = {}
    for name in CLASSES[:-1]:
        idx = bx.index(name)
        res[name] = []
        for r in idx:
            roi, l = bx.rois[r:r + 1], int(bx.levels[r])
            h, w = LEVEL_HW[l]
            ys, xs = (v.flatten() for v in sample_coords(roi, SCALES[l], P, S))
            yin, xin = (ys >= -1) & (ys <= h), (xs >= -1) & (xs <= w)
            all_in = bool(yin.all() and xin.all())
            x1, y1, x2, y2 = (float(v) for v in roi[0, 1:])
            area = (np.float32(x2) - np.float32(x1)) * (np.float32(y2) - np.float32(y1))
            if name.startswith("interior_l"):
                ok = l == int(name[-1]) and all_in and bool((ys >= 0).all() and (xs >= 0).all())
            elif name.startswith("clamp_"):
                v, size = (xs, w) if name in ("clamp_left", "clamp_right") else (ys, h)
                low = name in ("clamp_left", "clamp_top")
                ok = all_in and bool(((v < 0) if low else (v > size - 1)).any())
            elif name.startswith("zero_"):
                v, size = (xs, w) if name in ("zero_left", "zero_right") else (ys, h)
                low = name in ("zero_left", "zero_top")
                ok = bool(((v < -1) if low else (v > size)).any()) and bool((yin[:, None] & xin[None, :]).any())
            elif name == "outside":
                ok = not bool((yin[:, None] & xin[None, :]).any())
            elif name == "thin":
                ok = min(x2 - x1, y2 - y1) * SCALES[l] < 1 and min(x2 - x1, y2 - y1) > 0
            elif name == "flipped":
                ok = x2 <= x1 or y2 <= y1
            elif name.startswith("threshold_"):
                ok = float(area) == float(name.split("_")[1]) ** 2
            else:   # exact: every coordinate a multiple of the level's stride
                ok = all(float(v) * SCALES[l] == round(float(v) * SCALES[l]) for v in (x1, y1, x2, y2))
            res[name].append(bool(ok))
    return res


@functools.lru_cache(maxsize=None)
def reference(C, P, S, seed=0, only=None):
    """The fp64 RoIAlign of boxes(seed) (or of its class `only`) on pyramid(C, seed) at (P, S): computed once per
    combination and shared; callers must not write into it."""
    bx = boxes(seed)
    idx = list(range(len(bx.names))) if only is None else bx.index(only)
    return roi_align_reference(pyramid(C, seed), bx.rois[idx], P, SCALES, S, bx.levels[idx])


# ---- the heads ---------------------------------------------------------------------------------------------------------------------
def box_head_state_dict(C, P, rep, classes, seed=0):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    rb = lambda n: (torch.rand(n, generator=g) - 0.5) * 0.2
    return {"box_head.fc6.weight": rn(rep, C * P * P) * (2.0 / (C * P * P)) ** 0.5 * 4, "box_head.fc6.bias": rb(rep),
            "box_head.fc7.weight": rn(rep, rep) * (2.0 / rep) ** 0.5, "box_head.fc7.bias": rb(rep),
            "box_predictor.cls_score.weight": rn(classes, rep) * (1.0 / rep) ** 0.5,
            "box_predictor.cls_score.bias": rb(classes),
            "box_predictor.bbox_pred.weight": rn(4 * classes, rep) * (1.0 / rep) ** 0.5,
            "box_predictor.bbox_pred.bias": rb(4 * classes)}


def box_head_reference(sd, pooled):
    """fp64: pooled [R][P][P][C] (NHWC) -> (class_logits, box_regression); the flatten in torchvision's (c, y, x) order."""
    F = torch.nn.functional
    d = {k: v.double() for k, v in sd.items()}
    x = pooled.double().permute(0, 3, 1, 2).flatten(1)
    x = torch.relu(F.linear(x, d["box_head.fc6.weight"], d["box_head.fc6.bias"]))
    x = torch.relu(F.linear(x, d["box_head.fc7.weight"], d["box_head.fc7.bias"]))
    return (F.linear(x, d["box_predictor.cls_score.weight"], d["box_predictor.cls_score.bias"]),
            F.linear(x, d["box_predictor.bbox_pred.weight"], d["box_predictor.bbox_pred.bias"]))


def mask_head_state_dict(C, classes, seed=0):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    rb = lambda n: (torch.rand(n, generator=g) - 0.5) * 0.2
    sd = {}
    for i in range(4):
        sd[f"mask_head.{i}.0.weight"] = rn(C, C, 3, 3) * (2.0 / (9 * C)) ** 0.5
        sd[f"mask_head.{i}.0.bias"] = rb(C)
    sd["mask_predictor.conv5_mask.weight"] = rn(C, C, 2, 2) * (2.0 / C) ** 0.5
    sd["mask_predictor.conv5_mask.bias"] = rb(C)
    sd["mask_predictor.mask_fcn_logits.weight"] = rn(classes, C, 1, 1) * (1.0 / C) ** 0.5
    sd["mask_predictor.mask_fcn_logits.bias"] = rb(classes)
    return sd


def mask_head_reference(sd, pooled):
    """fp64: pooled [R][P][P][C] (NHWC, unpadded) -> mask logits [R][classes][2P][2P]."""
    F = torch.nn.functional
    d = {k: v.double() for k, v in sd.items()}
    x = pooled.double().permute(0, 3, 1, 2)
    for i in range(4):
        x = torch.relu(F.conv2d(x, d[f"mask_head.{i}.0.weight"], d[f"mask_head.{i}.0.bias"], padding=1))
    x = torch.relu(F.conv_transpose2d(x, d["mask_predictor.conv5_mask.weight"], d["mask_predictor.conv5_mask.bias"],
                                      stride=2))
    return F.conv2d(x, d["mask_predictor.mask_fcn_logits.weight"], d["mask_predictor.mask_fcn_logits.bias"])
