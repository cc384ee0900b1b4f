"""The image transform tests' helper: the fp64 reference of wino_image_transform_hw (normalise in fp64, then the exact
integer taps of resize_cases.axis_coords, into a zero batch), torchvision's size rule restated with torch's own ops,
torch's own fp32 CPU pipeline (normalise, interpolate, pad), the seeded image lists, the output footprint of a source
pixel, the cases the host and the GPU tests both name, the kernel's tile rule restated (tile_kinds) and the seeded sweep.
Nothing here needs a GPU to import."""
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
    # image 1 ends inside the first x-chunk: its tiles at x_first = 256 are pure padding beside live rows
    "pad_right": dict(shapes=[(9, 150), (11, 23)], sizes=[(20, 300), (17, 40)], batch=(24, 304)),
    # wo and ho on a tile edge and one off; Wb = 260: the second chunk is one lane wide (valid = 4, then 0); Hb = 9: a last
    # tile of one row.  Wb = 259: that lane has valid = 3
    "tile_edges": dict(shapes=[(5, 100), (8, 300), (4, 64)], sizes=[(7, 255), (8, 256), (9, 257)], batch=(9, 260)),
    "tile_edges_odd": dict(shapes=[(5, 100), (3, 7)], sizes=[(9, 257), (1, 256)], batch=(9, 259)),
    # batches one row high and 1, 2, 3 wide; a column batch: every source and output axis of length 1
    "thin1": dict(shapes=[(1, 1), (1, 6), (5, 1)], sizes=[(1, 1), (1, 1), (1, 1)], batch=(1, 1)),
    "thin2": dict(shapes=[(1, 1), (1, 6), (5, 1)], sizes=[(1, 2), (1, 2), (1, 1)], batch=(1, 2)),
    "thin3": dict(shapes=[(1, 1), (1, 6), (5, 1)], sizes=[(1, 3), (1, 2), (1, 3)], batch=(1, 3)),
    "thin_column": dict(shapes=[(5, 1), (1, 1), (7, 1), (1, 6)], sizes=[(5, 1), (3, 1), (4, 1), (9, 1)], batch=(9, 1)),
    "ratios": dict(shapes=[(2, 2), (1000, 3)], sizes=[(200, 200), (3, 1000)], batch=(200, 1000)),
}
THIN = ["thin1", "thin2", "thin3", "thin_column"]
TILE_W, TILE_ROWS, LANE_W = 256, 8, 4      # image_transform.hip's tile: 256 columns (four per lane) x 8 rows


def tile_kinds(sizes, Hb, Wb):
    """The kernel's tile rule restated: per image the tiles of TILE_ROWS x TILE_W of the Hb x Wb plane; a tile is a pad
    tile iff y_first >= ho or x_first >= wo.  Returns the set of kinds that occur."""
    kinds = set()
    for ho, wo in sizes:
        for y_first in range(0, Hb, TILE_ROWS):
            for x_first in range(0, Wb, TILE_W):
                y_end, x_end = min(y_first + TILE_ROWS, Hb), min(x_first + TILE_W, Wb)
                by_rows, by_cols = y_first >= ho, x_first >= wo
                if by_rows or by_cols:
                    kinds.add("pad by both" if by_rows and by_cols else "pad by rows only" if by_rows else "pad by columns only")
                else:
                    kinds.add("live")
                    if x_end > wo:
                        kinds.add("live with a zero tail in x")
                    if y_end > ho:
                        kinds.add("live with a zero tail in y")
                if y_end - y_first == 1:
                    kinds.add("one-row tile")
                if (x_end - x_first) % LANE_W:
                    kinds.add("valid < 4" + (" in a pad tile" if by_rows or by_cols else ""))
    return kinds


SWEEP_COUNT = 40


def sweep_specs():
    """SWEEP_COUNT seeded specs: N 1..5 images of C 1..4 channels, float32 or uint8, h, w 1..60 resized to ho, wo 1..300
    (the identity size now and then) in a batch of the maxima plus 0..40, divisible by nothing in particular."""
    rng = np.random.RandomState(20252)
    specs = []
    for index in range(SWEEP_COUNT):
        N, C = int(rng.randint(1, 6)), int(rng.randint(1, 5))
        shapes = [(int(rng.randint(1, 61)), int(rng.randint(1, 61))) for _ in range(N)]
        sizes = [s if rng.rand() < 0.15 else (int(rng.randint(1, 301)), int(rng.randint(1, 301))) for s in shapes]
        batch = tuple(max(s[d] for s in sizes) + int(rng.randint(0, 41)) for d in (0, 1))
        specs.append(dict(index=index, C=C, dtype="u8" if rng.rand() < 0.5 else "f32", shapes=shapes, sizes=sizes, batch=batch))
    return specs


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


def torch_pipeline(imgs, sizes, Hb, Wb, mean, std, dtype=torch.float32):
    """torch's own CPU composition in fp32 (or, dtype=torch.float64, with torch's source coordinates in double too):
    normalise, interpolate to the size, copy into a zero batch."""
    C = int(imgs[0].shape[0])
    out = torch.zeros(len(imgs), C, Hb, Wb, dtype=dtype)
    m, s = torch.tensor(mean, dtype=dtype)[:, None, None], torch.tensor(std, dtype=dtype)[:, None, None]
    for i, (t, (ho, wo)) in enumerate(zip(imgs, sizes)):
        x = t.to(dtype) / 255.0 if t.dtype == torch.uint8 else t.to(dtype)
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
