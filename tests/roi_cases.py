"""What the RoIAlign and R-CNN head tests share (tests/test_roi_host.py, test_gpu_roi_align.py, test_gpu_roi_heads.py):
the fp64 references in torch -- roi_align_reference (torchvision's CPU kernel, aligned=False, vectorised; the same
function in torch.float32 is the "straight fp32 restatement"), torchvision's level formula evaluated literally, the
thresholds rule of csrc/roi_align.hip restated, box_head_reference and mask_head_reference -- the base pyramid, and the
seeded box generator with its redraw rule; then the same generator for any pyramid (Geometry, geometry_boxes), the cases
of the RoIAlign sweep (roi_sweep_cases, tests/test_gpu_roi_sweep.py) and of the heads' sweeps (box_head_cases,
mask_head_cases).  Nothing here needs a GPU or the library to import."""
import collections
import dataclasses
import functools
import math

import numpy as np
import torch

from layer_refs import rel as rel_err, ring  # noqa: F401  (rel_err: the tests' metric, read from here)

# ---- the base pyramid ------------------------------------------------------------------------------------------------------
IMAGE = (64, 48)                                   # H, W of the image the boxes live in
LEVEL_HW = ((16, 12), (8, 6), (4, 3), (2, 2))      # (h, w) of the four levels, strides 4 .. 32
SCALES = (1 / 4, 1 / 8, 1 / 16, 1 / 32)
N_IMAGES = 2
CHANNELS = (8, 64, 320)                            # 320: the lanes walk a second, partial 256-channel slab
CANONICAL_SCALE, CANONICAL_LEVEL = 16.0, 4         # boxes inside a 64 x 48 image reach all four levels
PS_COMBOS = tuple((P, S) for P in (1, 7, 14) for S in (1, 2, 3))     # what the parity test runs
EXACT_COMBOS = tuple((P, S) for P in (2, 4, 8) for S in (1, 2))      # ... and the exact-geometry subset
EXACT_COMBOS_S4 = tuple((P, 4) for P in (2, 4, 8))                   # ... at sampling 4 (tests/test_gpu_roi_sweep.py)
SAMPLE_MARGIN = 1e-3     # the redraw rule: no fp64 sample coordinate this close to -1 or to h / w
LEVEL_MARGIN = 1e-4      # ... and canonical_level + log2(sqrt(area) / canonical_scale) not this close to an integer
EXACT_TOL = 1e-6         # the exact-geometry subset: every coordinate and weight is exact in fp32


def pyramid(C, seed=0, hw=LEVEL_HW, N=N_IMAGES):
    """The level maps [N][h][w][C], float32, uniform in [-0.5, 0.5)."""
    g = torch.Generator().manual_seed(1000 * seed + C)
    return [torch.rand(N, h, w, C, generator=g) - 0.5 for h, w in hw]


def padded_nan(t):
    """[N][h][w][C] -> [N][h+2][w+2][C] with a NaN ring: one ring read by the kernel shows in its result."""
    return ring(t, float("nan"))


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


def level_margin(rois, scales=SCALES, canonical_scale=CANONICAL_SCALE, canonical_level=CANONICAL_LEVEL):
    """[R]: the distance of canonical_level + log2(sqrt(area) / canonical_scale) to the nearest integer at which the level
    changes, k_min + 1 .. k_max (Inf for area <= 0, and with one level)."""
    b = rois.to(torch.float64)
    area = (b[:, 3] - b[:, 1]) * (b[:, 4] - b[:, 2])
    k = canonical_level + torch.log2(torch.sqrt(area.clamp(min=1e-300)) / canonical_scale)
    if len(scales) == 1:
        return torch.full_like(k, float("inf"))
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


def has_property(name, roi, l, hw, scale, P=7, S=2, edge=None):
    """Whether the one box `roi` [1][5], which takes level `l` of size hw = (h, w) at `scale`, has the property its class
    `name` is named for, judged from the fp64 sample coordinates at (P, S).  `edge`: sqrt(area) of a threshold class."""
    h, w = hw
    ys, xs = (v.flatten() for v in sample_coords(roi, scale, P, S))
    yin, xin = (ys >= -1) & (ys <= h), (xs >= -1) & (xs <= w)
    all_in = bool(yin.all() and xin.all())
    x1, y1, x2, y2 = (float(v) for v in roi[0, 1:])
    with np.errstate(over="ignore"):
        area = (np.float32(x2) - np.float32(x1)) * (np.float32(y2) - np.float32(y1))
    if name.startswith("interior_l"):
        return l == int(name[-1]) and all_in and bool((ys >= 0).all() and (xs >= 0).all())
    if name.startswith("clamp_"):
        v, size = (xs, w) if name in ("clamp_left", "clamp_right") else (ys, h)
        low = name in ("clamp_left", "clamp_top")
        return all_in and bool(((v < 0) if low else (v > size - 1)).any())
    if name.startswith("zero_"):
        v, size = (xs, w) if name in ("zero_left", "zero_right") else (ys, h)
        low = name in ("zero_left", "zero_top")
        return bool(((v < -1) if low else (v > size)).any()) and bool((yin[:, None] & xin[None, :]).any())
    if name == "outside":
        return not bool((yin[:, None] & xin[None, :]).any())
    if name == "thin":
        return min(x2 - x1, y2 - y1) * scale < 1 and min(x2 - x1, y2 - y1) > 0
    if name == "flipped":
        return x2 <= x1 or y2 <= y1
    if name.startswith("threshold_"):
        return float(area) == float(edge) ** 2
    if name == "huge":   # finite, of magnitude 1e30 and more, and no sample anywhere near the map
        return max(abs(x1), abs(y1), abs(x2), abs(y2)) >= 1e30 and math.isfinite(x1 + y1 + x2 + y2) and not bool(
            (yin[:, None] & xin[None, :]).any())
    assert name == "exact", name   # every coordinate a multiple of the level's stride
    return all(float(v) * scale == round(float(v) * scale) for v in (x1, y1, x2, y2))


def class_properties(bx, P=7, S=2):
    """{class: [bool per box of the class]}: whether each table box has the property its class is named for."""
    res = {}
    for name in CLASSES[:-1]:
        res[name] = []
        for r in bx.index(name):
            l = int(bx.levels[r])
            edge = float(name.split("_")[1]) if name.startswith("threshold_") else None
            res[name].append(bool(has_property(name, bx.rois[r:r + 1], l, LEVEL_HW[l], SCALES[l], P, S, edge)))
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


# ---- any pyramid: a geometry, its boxes, and the sweep's cases ------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Geometry:
    """One pyramid the boxes live in.  `hw`: the (h, w) of each level, finest first; the scales are 2^-(k0 + l), or with
    one level `scale0` when that is given (a scale that is no power of two)."""
    image: tuple
    levels: int
    k0: int
    hw: tuple
    N: int
    canonical_scale: float = 224.0
    canonical_level: int = 4
    scale0: float = None

    @property
    def scales(self):
        if self.scale0 is not None:
            assert self.levels == 1
            return (float(self.scale0),)
        return tuple(2.0 ** -(self.k0 + l) for l in range(self.levels))

    @property
    def canon(self):
        return dict(canonical_scale=self.canonical_scale, canonical_level=self.canonical_level)

    def edges(self):
        """sqrt(area), in image pixels, at which a box moves up to level 1, 2, ..: levels - 1 of them."""
        return [self.canonical_scale * 2.0 ** (self.k0 + j - self.canonical_level) for j in range(1, self.levels)]


def ceil_geometry(image, levels, k0, N, canonical_scale=224.0, canonical_level=4, scale0=None):
    """The pyramid a backbone with `same` padding makes of `image`: every level ceil(image * scale)."""
    geo = Geometry(tuple(image), levels, k0, (), N, float(canonical_scale), int(canonical_level), scale0)
    hw = tuple((math.ceil(image[0] * s), math.ceil(image[1] * s)) for s in geo.scales)
    return dataclasses.replace(geo, hw=hw)


BASE_GEOMETRY = Geometry(IMAGE, 4, 2, LEVEL_HW, N_IMAGES, CANONICAL_SCALE, CANONICAL_LEVEL)
HUGE = ((1e30, 1e30, 3e38, 3e38), (-3e38, -3e38, -1e30, -1e30), (-1e30, 2.0, 3e38, 9.0))
NAMED_TRIES = 400        # proposals per named box before its class is left out of a geometry that has no room for it


def _sizes(geo, l, u, cap):
    """sqrt(area) log-uniform in level l's range, above 0.4 pixels of that level and below `cap`; None if there is none."""
    e = [0.0] + geo.edges() + [float("inf")]
    st = 1.0 / geo.scales[l]
    lo, hi = max(e[l] * 1.02, 0.4 * st), min(e[l + 1] * 0.98, cap)
    return lo * (hi / lo) ** u if hi > lo else None


def _propose(name, k, geo, u):
    """One candidate (x1, y1, x2, y2) of class `name` (its k-th box) from uniforms u[0..7]; None if the draw has no room."""
    H, W = geo.image
    lt = int(name[-1]) if name.startswith("interior_l") else min(int(u[0] * geo.levels), geo.levels - 1)
    st, (h, w) = 1.0 / geo.scales[lt], geo.hw[lt]
    if name.startswith("threshold_"):
        edge = geo.edges()[int(name[-1]) - 1]
        a = 2.0 ** (int(u[1] * 3) - 1)
        bw, bh = edge * a, edge / a
        x1, y1 = round(u[2] * (W - bw) * 4) / 4, round(u[3] * (H - bh) * 4) / 4
        return x1, y1, x1 + bw, y1 + bh
    if name.startswith("interior_l") or name == "flipped":
        s = _sizes(geo, lt, u[1], 0.95 * math.sqrt(H * W))
        if s is None:
            return None
        aspect = math.exp(1.4 * u[2] - 0.7)
        bw, bh = s * math.sqrt(aspect), s / math.sqrt(aspect)
        if bw > 0.98 * W:
            bw, bh = 0.98 * W, s * s / (0.98 * W)
        if bh > 0.98 * H:
            bw, bh = s * s / (0.98 * H), 0.98 * H
        if bw > W or bh > H:
            return None
        x1, y1 = u[3] * (W - bw), u[4] * (H - bh)
        if name == "flipped":   # x2 < x1; y2 < y1 (area < 0); both (area > 0); a point (area 0)
            return ((x1 + bw, y1, x1, y1 + bh), (x1, y1 + bh, x1 + bw, y1), (x1 + bw, y1 + bh, x1, y1), (x1, y1, x1, y1))[k % 4]
        return x1, y1, x1 + bw, y1 + bh
    # the small classes, placed in pixels of level lt's map: a box of at most 8 x 8 of them that the map has room for
    s = _sizes(geo, lt, u[1], st * min(8.0, min(h, w) + 0.5))
    if s is None:
        return None
    aspect = math.exp(0.6 * u[2] - 0.3)
    mw, mh = s * math.sqrt(aspect) / st, s / math.sqrt(aspect) / st
    if name == "thin":
        mw, mh = (0.2 + 0.7 * u[3], 2 + 4 * u[4]) if k % 2 else (2 + 4 * u[4], 0.2 + 0.7 * u[3])
    ew, eh = max(mw, 1.0), max(mh, 1.0)
    sx, sy = u[5] * max(w - mw, 0.0), u[6] * max(h - mh, 0.0)          # inside the map, unless the class says otherwise
    if name == "clamp_left":
        sx = -(0.15 + 0.8 * u[7])
    elif name == "clamp_top":
        sy = -(0.15 + 0.8 * u[7])
    elif name == "clamp_right":
        sx = w - (0.02 + 0.5 * u[7]) - mw
    elif name == "clamp_bottom":
        sy = h - (0.02 + 0.5 * u[7]) - mh
    elif name == "zero_left":
        sx = -1 - (0.15 + 0.5 * u[7]) * ew
    elif name == "zero_top":
        sy = -1 - (0.15 + 0.5 * u[7]) * eh
    elif name == "zero_right":
        sx = w - (0.3 + 0.5 * u[7]) * ew
    elif name == "zero_bottom":
        sy = h - (0.3 + 0.5 * u[7]) * eh
    elif name == "outside":
        sx = (w + 1.5 + 3 * u[7]) if k % 2 else -(mw + 2.5 + 3 * u[7])
        sy = sy if k % 2 else h + 1.5 + 3 * u[5]
    return sx * st, sy * st, (sx + mw) * st, (sy + mh) * st


def named_classes(geo):
    """The classes geometry_boxes tries for `geo`, two boxes each (first and last image), four of `flipped`."""
    names = [f"interior_l{l}" for l in range(geo.levels)]
    names += ["clamp_left", "clamp_top", "clamp_right", "clamp_bottom", "zero_left", "zero_top", "zero_right", "zero_bottom",
              "outside", "thin", "flipped"]
    return names + [f"threshold_{j}" for j in range(1, geo.levels)]


class GeoBoxes:
    """Boxes for one geometry: the named classes of `named_classes(geo)` drawn to the geometry (a class the geometry has no
    room for is left out; tests/test_roi_host.py says which may be), the HUGE rows, and `n` random log-uniform boxes.
    The same two redraw rules as Boxes, at the (P, sampling) of `combos`, with the geometry's own canonical values:
    rois [R][5] float32, names [R], levels [R] (fp64 formula), drawn / redrawn counts of the random part."""

    def __init__(self, geo, combos, seed, n):
        g = torch.Generator().manual_seed(seed)
        self.geo, self.drawn, self.redrawn = geo, 0, 0
        rows, names = [], []
        H, W = geo.image
        last = float(geo.N - 1)

        def margins_ok(roi, lvl, level_rule=True):
            if float(min_sample_margin(roi, lvl, combos, hw=geo.hw, scales=geo.scales)) < SAMPLE_MARGIN:
                return False
            return not level_rule or float(level_margin(roi, geo.scales, **geo.canon)) >= LEVEL_MARGIN

        for name in named_classes(geo):
            for k in range(4 if name == "flipped" else 2):
                img = (0.0, last)[k % 2]
                for _ in range(NAMED_TRIES):
                    u = torch.rand(8, generator=g, dtype=torch.float64).tolist()
                    box = _propose(name, k, geo, u)
                    if box is None:
                        continue
                    roi = torch.tensor([[img, *box]], dtype=torch.float32)
                    l = int(torchvision_levels(roi, geo.scales, **geo.canon))
                    edge = geo.edges()[int(name[-1]) - 1] if name.startswith("threshold_") else None
                    if (has_property(name, roi, l, geo.hw[l], geo.scales[l], edge=edge)
                            and margins_ok(roi, torch.tensor([l]), level_rule=edge is None)):
                        rows.append([img, *box])
                        names.append(name)
                        break
        for k, box in enumerate(HUGE):
            for img in (0.0, last):
                rows.append([img, *box])
                names.append("huge")
        e = geo.edges()
        st0 = 1.0 / geo.scales[0]
        lo = max(0.4 * st0, e[0] / 4) if e else 0.4 * st0
        hi = min(1.1 * max(H, W), e[-1] * 3) if e else 0.9 * max(H, W)
        assert lo < hi, (geo, lo, hi)
        while names.count("random") < n:
            u = torch.rand(6, generator=g, dtype=torch.float64).tolist()
            size = lo * (hi / lo) ** u[0]                       # sqrt(area), log-uniform
            aspect = math.exp(1.4 * u[1] - 0.7)
            bw, bh = size * math.sqrt(aspect), size / math.sqrt(aspect)
            cx, cy = (-0.08 + 1.16 * u[2]) * W, (-0.08 + 1.16 * u[3]) * H
            row = [float(min(int(u[4] * geo.N), geo.N - 1)), cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2]
            self.drawn += 1
            roi = torch.tensor([row], dtype=torch.float32)
            if not margins_ok(roi, torchvision_levels(roi, geo.scales, **geo.canon)):
                self.redrawn += 1
                continue
            rows.append(row)
            names.append("random")
        self.rois = torch.tensor(rows, dtype=torch.float32)
        self.names = names
        self.levels = torchvision_levels(self.rois, geo.scales, **geo.canon)

    def index(self, name):
        return [i for i, n in enumerate(self.names) if n == name]


@functools.lru_cache(maxsize=None)
def geometry_boxes(geo, combos, seed, n):
    return GeoBoxes(geo, tuple(combos), seed, n)


def geo_class_properties(gb, P=7, S=2):
    """class_properties for a GeoBoxes: {class: [bool per box]} over the named classes it holds, `huge` included."""
    res = collections.defaultdict(list)
    for r, name in enumerate(gb.names):
        if name == "random":
            continue
        l = int(gb.levels[r])
        edge = gb.geo.edges()[int(name[-1]) - 1] if name.startswith("threshold_") else None
        res[name].append(bool(has_property(name, gb.rois[r:r + 1], l, gb.geo.hw[l], gb.geo.scales[l], P, S, edge)))
    return dict(res)


RoiCase = collections.namedtuple("RoiCase", "name geo P S C in_padded out_padded defaults seed n")
SWEEP_RANDOM = 24        # random boxes per sweep case
DEFAULT_CANON = (224.0, 4)   # what roi_align / multiscale_roi_align take when no canonical_* is passed
# (image H, W), levels, k0, N, canonical scale, canonical level, P, sampling, C, in_padded, out_padded, scale0
_SWEEP = (
    ((61, 45), 4, 2, 2, 16, 4, 7, 1, 8, 0, 0, None),
    ((22, 19), 3, 0, 3, 24, 3, 4, 1, 252, 1, 0, None),
    ((70, 50), 1, 2, 1, 224, 4, 1, 1, 4, 0, 1, 0.25),
    ((150, 100), 2, 3, 5, 56, 4, 7, 2, 256, 1, 1, None),
    ((45, 37), 4, 1, 4, 16, 3, 14, 2, 260, 0, 0, None),
    ((300, 200), 3, 4, 2, 56, 4, 1, 2, 320, 1, 0, None),
    ((700, 500), 4, 5, 3, 56, 5, 7, 3, 516, 0, 1, None),
    ((20, 23), 2, 0, 1, 224, 5, 2, 3, 8, 1, 1, None),
    ((60, 70), 1, 2, 2, 224, 4, 1, 3, 260, 0, 0, 0.3),
    ((61, 45), 4, 2, 2, 16, 4, 7, 4, 320, 1, 1, None),
    ((170, 190), 3, 3, 5, 24, 3, 6, 4, 8, 1, 0, None),
    ((30, 47), 2, 1, 2, 16, 4, 1, 4, 256, 0, 1, None),
    ((60, 50), 2, 2, 2, 56, 4, 64, 2, 4, 0, 0, None),                 # the header's edge P = 64
    ((7, 90), 4, 2, 3, 16, 4, 7, 2, 8, 1, 0, None),                   # h = 1 levels; 2 x 23: wider than high
    ((40, 3), 3, 1, 2, 16, 5, 5, 3, 4, 0, 1, None),                   # w = 1 levels
    ((260, 236), 2, 3, 2, None, None, 7, 2, 256, 1, 1, None),         # the wrapper's defaults: level 1 from sqrt(area) 224
    ((134, 118), 3, 2, 3, None, None, 14, 2, 8, 0, 0, None),          # ... from 112, level 2 from 224
    ((21, 18), 4, 0, 5, 24, 5, 8, 2, 252, 1, 1, None),
    ((40, 30), 1, 1, 4, 224, 4, 3, 4, 516, 1, 0, 0.5),
    ((600, 650), 3, 5, 2, 56, 4, 2, 1, 260, 0, 1, None),
    ((330, 250), 2, 4, 1, 56, 3, 13, 2, 320, 0, 0, None),
    ((180, 190), 4, 3, 2, 24, 4, 5, 4, 4, 1, 1, None),
    ((90, 94), 3, 2, 3, 16, 3, 9, 3, 256, 0, 0, None),
    ((700, 400), 2, 5, 2, 224, 5, 4, 2, 8, 1, 0, None),
)


@functools.lru_cache(maxsize=None)
def roi_sweep_cases():
    """The RoIAlign sweep: a fixed list; tests/test_roi_host.py shows what it reaches.  A case with `defaults` goes through
    multiscale_roi_align with no canonical_* passed and the scales inferred from the image size."""
    cases = []
    for i, (image, levels, k0, N, cs, cl, P, S, C, ip, op, scale0) in enumerate(_SWEEP):
        defaults = cs is None
        cs, cl = DEFAULT_CANON if defaults else (cs, cl)
        geo = ceil_geometry(image, levels, k0, N, cs, cl, scale0)
        cases.append(RoiCase(f"sweep{i:02d}", geo, P, S, C, bool(ip), bool(op), defaults, 7000 + i, SWEEP_RANDOM))
    return tuple(cases)


def case_boxes(case):
    return geometry_boxes(case.geo, ((case.P, case.S),), case.seed, case.n)


def case_pyramid(case):
    return pyramid(case.C, case.seed, case.geo.hw, case.geo.N)


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """The fp64 RoIAlign of a sweep case: computed once and shared; callers must not write into it."""
    gb = case_boxes(case)
    return roi_align_reference(case_pyramid(case), gb.rois, case.P, case.geo.scales, case.S, gb.levels)


# ---- the heads, swept ----------------------------------------------------------------------------------------------------------
BoxHeadCase = collections.namedtuple("BoxHeadCase", "C P rep classes R seed")
MaskHeadCase = collections.namedtuple("MaskHeadCase", "C P classes R seed")
HEAD_FORMS = ("auto", "tiled", "stream_k", "latency")      # "auto": no knob; the others are knob sets of cases.PROJ_FORMS
HEAD_3X3_ALGO = {"tiled": "big", "stream_k": "big", "latency": "small"}   # what WINO_3X3_ALGO the mask head's 3x3 gets beside them


def _pad64(n):
    return (n + 63) // 64 * 64


def box_head_cases():
    """C x P with C P P % 32 == 0 (1568 = 32 x 49 is no multiple of 64), rep, classes whose 5 x classes straddle the
    64-column padding (60, 65), R around the 112-row tile."""
    rows = ((32, 7, 64, 1, 1), (64, 7, 192, 91, 300), (96, 4, 320, 12, 112), (160, 2, 64, 13, 113), (32, 8, 192, 2, 111),
            (64, 2, 320, 91, 2), (96, 7, 64, 13, 300), (160, 8, 192, 12, 1), (64, 4, 64, 2, 113), (160, 7, 320, 1, 112))
    return tuple(BoxHeadCase(*r, seed=8100 + i) for i, r in enumerate(rows))


def box_head_gemms(c):
    """{name: (M, Cin, Kout)} of the box head's three launches."""
    return {"fc6": (c.R, c.C * c.P * c.P, c.rep), "fc7": (c.R, c.rep, c.rep), "predictor": (c.R, c.rep, _pad64(5 * c.classes))}


def mask_head_cases():
    rows = ((64, 14, 91, 1), (64, 6, 3, 40), (128, 2, 65, 9), (128, 14, 1, 3), (64, 2, 64, 40), (128, 6, 91, 1),
            (64, 14, 65, 9), (128, 6, 64, 40))
    return tuple(MaskHeadCase(*r, seed=8200 + i) for i, r in enumerate(rows))


def mask_head_gemms(c):
    """{name: (M, Cin, Kout)} of the mask head's two GEMMs: the transposed convolution read through A_PADDED at N = R, and
    the logits whose A is the re-viewed output of the first."""
    M = c.R * c.P * c.P
    return {"deconv": (M, c.C, 4 * c.C), "logits": (4 * M, c.C, _pad64(c.classes))}
