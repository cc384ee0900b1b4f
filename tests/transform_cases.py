"""The image transform tests' helper: the fp64 reference of wino_image_transform_hw (normalise in fp64, then the exact
integer taps of resize_cases.axis_coords, into a zero batch), torchvision's size rule restated with torch's own ops,
torch's own fp32 CPU pipeline (normalise, interpolate, pad), the seeded image lists, the output footprint of a source
pixel, and the cases the host and the GPU tests both name.  Nothing here needs a GPU to import."""
import math

import numpy as np
import torch

from resize_cases import axis_coords

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
TOL = 2e-5                     # of max |want|: wino_resize_bilinear_hw's own bar for the same arithmetic
PAIRS = [((480, 640), (800, 1066)), ((427, 640), (799, 1199)), ((375, 500), (799, 1066)), ((333, 500), (799, 1201)),
         ((1200, 1800), (800, 1200))]      # (h, w) -> torch's (ho, wo) at min_size 800, max_size 1333

# name: (shapes, out_sizes or None for the size rule at (min_size, max_size), (min_size, max_size), size_divisible, C)
RULE = dict(shapes=[(13, 17), (30, 9), (20, 20)], sizes=[(24, 31), (40, 12), (24, 24)], min_max=(24, 40), batch=(64, 32))
CASES = {
    "rule": dict(shapes=RULE["shapes"], sizes=RULE["sizes"], batch=RULE["batch"]),
    "odd_wb": dict(shapes=RULE["shapes"], sizes=RULE["sizes"], batch=(40, 31)),                 # size_divisible = 1
    "explicit": dict(shapes=[(13, 17), (7, 5), (97, 33)], sizes=[(13, 17), (64, 45), (20, 7)], batch=(64, 48)),
    "wide": dict(shapes=[(9, 150), (11, 3)], sizes=[(20, 300), (3, 261)], batch=(24, 304)),     # two x-chunks, three row tiles
}


def size_rule(h: int, w: int, min_size: int, max_size: int):
    """torchvision's _resize_image_and_masks with torch's own ops: the fp32 scale factor, then interpolate's floor."""
    im = torch.tensor([h, w])
    mn, mx = torch.min(im).to(dtype=torch.float32), torch.max(im).to(dtype=torch.float32)
    s = torch.min(float(min_size) / mn, float(max_size) / mx).item()
    return math.floor(h * s), math.floor(w * s)


def images(shapes, C=3, dtype=torch.float32, seed=0):
    """The seeded list: float32 uniform in [0, 1), or uint8 over all 256 values."""
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        return [torch.randint(0, 256, (C, h, w), generator=g, dtype=torch.uint8) for h, w in shapes]
    return [torch.rand(C, h, w, generator=g) for h, w in shapes]


def mean_std(C):
    if C == 3:
        return IMAGENET_MEAN, IMAGENET_STD
    return tuple(0.3 + 0.17 * c for c in range(C)), tuple(0.21 + 0.4 * c for c in range(C))


def transform_reference(imgs, sizes, Hb, Wb, mean, std):
    """fp64 [N][C][Hb][Wb]: (v - mean) / std per pixel (a byte is byte / 255), the exact taps, every tap multiplied."""
    C = int(imgs[0].shape[0])
    out = np.zeros((len(imgs), C, Hb, Wb), dtype=np.float64)
    m, s = np.asarray(mean, np.float64)[:, None, None], np.asarray(std, np.float64)[:, None, None]
    for i, (t, (ho, wo)) in enumerate(zip(imgs, sizes)):
        x = t.numpy().astype(np.float64)
        if t.dtype == torch.uint8:
            x = x / 255.0
        x = (x - m) / s
        y0, y1, ly = axis_coords(x.shape[1], ho)
        x0, x1, lx = axis_coords(x.shape[2], wo)
        ly, lx = ly[:, None], lx[None, :]
        with np.errstate(invalid="ignore"):
            top = (1 - lx) * x[:, y0][:, :, x0] + lx * x[:, y0][:, :, x1]
            bot = (1 - lx) * x[:, y1][:, :, x0] + lx * x[:, y1][:, :, x1]
            out[i, :, :ho, :wo] = (1 - ly) * top + ly * bot
    return out


def torch_pipeline(imgs, sizes, Hb, Wb, mean, std):
    """torch's own fp32 CPU composition: normalise, interpolate to the size, copy into a zero batch."""
    C = int(imgs[0].shape[0])
    out = torch.zeros(len(imgs), C, Hb, Wb)
    m, s = torch.tensor(mean)[:, None, None], torch.tensor(std)[:, None, None]
    for i, (t, (ho, wo)) in enumerate(zip(imgs, sizes)):
        x = t.float() / 255.0 if t.dtype == torch.uint8 else t
        x = (x - m) / s
        out[i, :, :ho, :wo] = torch.nn.functional.interpolate(x[None], size=(ho, wo), mode="bilinear", align_corners=False)[0]
    return out.numpy()


def footprint(h, w, ho, wo, Hb, Wb, y, x):
    """bool [Hb][Wb]: the outputs of an h x w -> ho x wo plane one of whose four taps is source pixel (y, x)."""
    y0, y1, _ = axis_coords(h, ho)
    x0, x1, _ = axis_coords(w, wo)
    mark = np.zeros((Hb, Wb), dtype=bool)
    mark[:ho, :wo] = ((y0 == y) | (y1 == y))[:, None] & ((x0 == x) | (x1 == x))[None, :]
    return mark


def check(got, want, sizes, what=""):
    """got [N][C][Hb][Wb] float32 against the fp64 reference: TOL * max |want| inside, bitwise +0 in the pad region.
    Returns the error relative to max |want|."""
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.float32, (got.shape, want.shape, got.dtype)
    pad = np.ones(want.shape, dtype=bool)
    for i, (ho, wo) in enumerate(sizes):
        pad[i, :, :ho, :wo] = False
    assert not (got.view(np.int32)[pad] != 0).any(), f"{what}: the pad region is not +0 everywhere"
    scale = np.abs(want).max()
    err = float(np.abs(got.astype(np.float64) - want)[~pad].max() / scale)
    print(f"{what}: max |got - want| / max |want| = {err:.2e}")
    assert err <= TOL, (what, err)
    return err
