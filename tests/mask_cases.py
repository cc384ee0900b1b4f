"""The mask paste's fp64 reference and its cases (imports no test module; nothing here needs a GPU).

paste_reference is torchvision's maskrcnn_inference + paste_masks_in_image(padding=1) as winograd_mi355x.h words it:
sigmoid, a ring of zeros, the box grown by (M + 2) / M and truncated toward zero, and inside the window the bilinear
align_corners=False resize with exact integer source coordinates.  The box integers are computed twice: in numpy float32
in the kernel's operation order (what the kernel is expected to use) and in fp64; `int_margin` is the smallest distance
of an fp64 expanded coordinate from an integer, and the generator redraws a box until it is at least INT_MARGIN, so that
neither fp32 rounding nor a contraction into an fma can move a pixel column."""
import functools

import numpy as np

INT_MARGIN = 1e-3
ROWS = 16                     # output rows per workgroup of mask_paste.hip: what "several row blocks" means
LIM = 2.0 ** 30
CLASSES = ("inside", "cross_left", "cross_top", "larger", "one_pixel", "row_blocks",      # slots of image 0
           "cross_right", "cross_bottom", "outside", "inverted", "cut_by_image_hw")       # slots of image 1
LATTICE_M = (2, 4, 8, 16)     # (M + 2) / M is a binary fraction


def expand(boxes, M, dtype):
    """expand_boxes in `dtype`, in the kernel's order: [R][4] -> the expanded (ex1, ey1, ex2, ey2), clamped to +-2^30."""
    b = np.asarray(boxes).astype(dtype)
    scale = dtype(np.float64(M + 2) / np.float64(M))
    out = np.empty_like(b)
    with np.errstate(invalid="ignore", over="ignore"):
        for lo, hi in ((0, 2), (1, 3)):
            half = (b[:, hi] - b[:, lo]) * dtype(0.5) * scale
            c = (b[:, hi] + b[:, lo]) * dtype(0.5)
            out[:, lo], out[:, hi] = c - half, c + half
    return np.clip(out, dtype(-LIM), dtype(LIM))


def box_integers(boxes, M, dtype=np.float32):
    """(.to(int64) of the expanded boxes [R][4], finite [R]): truncation toward zero; a box with a coordinate that is not
    finite has finite False and integers 0."""
    b = np.asarray(boxes)
    finite = np.isfinite(b).all(axis=1)
    e = expand(np.where(finite[:, None], b, 0), M, dtype)
    return np.trunc(e).astype(np.int64), finite


def int_margin(boxes, M):
    """Per box, the smallest distance of an fp64 expanded coordinate from an integer (inf for a box that is not finite)."""
    b = np.asarray(boxes)
    finite = np.isfinite(b).all(axis=1)
    e = expand(np.where(finite[:, None], b, 0), M, np.float64)
    m = np.abs(e - np.rint(e)).min(axis=1)
    return np.where(finite, m, np.inf)


def image_ints(image_hw, H, W):
    hw = np.nan_to_num(np.asarray(image_hw, dtype=np.float64), nan=0.0)
    im_h = np.clip(np.trunc(np.clip(hw[:, 0], 0, H)), 0, H).astype(np.int64)
    im_w = np.clip(np.trunc(np.clip(hw[:, 1], 0, W)), 0, W).astype(np.int64)
    return im_h, im_w


def window(bi, im_h, im_w):
    """(x0, x1e, y0, y1e, w, h) of one box's integers; x0 >= x1e or y0 >= y1e: empty."""
    bx1, by1, bx2, by2 = (int(v) for v in bi)
    return (max(bx1, 0), min(bx2 + 1, im_w), max(by1, 0), min(by2 + 1, im_h), max(bx2 - bx1 + 1, 1),
            max(by2 - by1 + 1, 1))


def axis_coords(d, size_in, size_out):
    """resize.hip's exact integer source coordinates of outputs d (int64 array): (i0, i1, lambda in fp64)."""
    num = np.maximum((2 * d + 1) * size_in - size_out, 0)
    i0 = num // (2 * size_out)
    i1 = np.minimum(i0 + 1, size_in - 1)
    return i0, i1, (num - i0 * 2 * size_out).astype(np.float64) / np.float64(2 * size_out)


def plane_window(logit_plane, bi, im_h, im_w):
    """One finite box: ((y0, y1e, x0, x1e), values [y1e - y0][x1e - x0] in fp64) or None for an empty window.
    logit_plane: [M][M] of the selected class."""
    M = logit_plane.shape[0]
    x0, x1e, y0, y1e, w, h = window(bi, im_h, im_w)
    if x0 >= x1e or y0 >= y1e:
        return None
    with np.errstate(over="ignore"):
        prob = np.zeros((M + 2, M + 2))
        prob[1:-1, 1:-1] = 1.0 / (1.0 + np.exp(-logit_plane.astype(np.float64)))
    ya, yb, ly = axis_coords(np.arange(y0, y1e, dtype=np.int64) - int(bi[1]), M + 2, h)
    xa, xb, lx = axis_coords(np.arange(x0, x1e, dtype=np.int64) - int(bi[0]), M + 2, w)
    ly, lx = ly[:, None], lx[None, :]
    with np.errstate(invalid="ignore"):
        top = (1 - lx) * prob[np.ix_(ya, xa)] + lx * prob[np.ix_(ya, xb)]
        bot = (1 - lx) * prob[np.ix_(yb, xa)] + lx * prob[np.ix_(yb, xb)]
        return (y0, y1e, x0, x1e), (1 - ly) * top + ly * bot


def paste_reference(logits, labels, boxes, image_hw, H, W):
    """logits [R][classes][M][M], labels [R] ints, boxes [R][4] float32, image_hw [N][2] -> (planes [N][D][H][W] fp64,
    int_margin: the smallest over the boxes that are finite and carry a legal label)."""
    logits, labels, boxes = np.asarray(logits), np.asarray(labels).reshape(-1), np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    R, classes, M = logits.shape[0], logits.shape[1], logits.shape[2]
    N = np.asarray(image_hw).shape[0]
    D = R // N
    im_h, im_w = image_ints(image_hw, H, W)
    bi, finite = box_integers(boxes, M, np.float32)
    bi64, _ = box_integers(boxes, M, np.float64)
    margins = int_margin(boxes, M)
    out = np.zeros((N, D, H, W))
    margin = np.inf
    for r in range(R):
        n, lab = r // D, int(labels[r])
        if not 0 <= lab < classes:
            continue
        if not finite[r]:
            out[n, r % D, :im_h[n], :im_w[n]] = np.nan
            continue
        margin = min(margin, float(margins[r]))
        if margins[r] >= INT_MARGIN:
            assert (bi[r] == bi64[r]).all(), (r, boxes[r], bi[r], bi64[r])
        got = plane_window(logits[r, lab], bi[r], int(im_h[n]), int(im_w[n]))
        if got is not None:
            (y0, y1e, x0, x1e), v = got
            out[n, r % D, y0:y1e, x0:x1e] = v
    return out, margin


def paste_windows(labels, boxes, image_hw, M, classes, H, W):
    """bool [N][D][H][W]: the pixels inside each plane's window (the image window for a box that is not finite, nothing
    for an illegal label).  Everything outside is exactly 0."""
    labels, boxes = np.asarray(labels).reshape(-1), np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    R, N = boxes.shape[0], np.asarray(image_hw).shape[0]
    D = R // N
    im_h, im_w = image_ints(image_hw, H, W)
    bi, finite = box_integers(boxes, M, np.float32)
    inside = np.zeros((N, D, H, W), dtype=bool)
    for r in range(R):
        n = r // D
        if not 0 <= int(labels[r]) < classes:
            continue
        if not finite[r]:
            inside[n, r % D, :im_h[n], :im_w[n]] = True
            continue
        x0, x1e, y0, y1e, _, _ = window(bi[r], int(im_h[n]), int(im_w[n]))
        if x0 < x1e and y0 < y1e:
            inside[n, r % D, y0:y1e, x0:x1e] = True
    return inside


def to_gemm_rows(logits, ld, fill=np.nan):
    """[R][classes][M][M] -> the logits GEMM's [R P P 4][ld], rows (r, y, x, dy, dx); the columns past the classes hold
    `fill` (NaN: they are never read)."""
    R, classes, M = logits.shape[0], logits.shape[1], logits.shape[2]
    P = M // 2
    assert M == 2 * P and classes <= ld
    rows = np.full((R * P * P * 4, ld), fill, dtype=np.float32)
    rows[:, :classes] = logits.reshape(R, classes, P, 2, P, 2).transpose(0, 2, 4, 3, 5, 1).reshape(-1, classes)
    return rows


# ---- the margin-keeping generator ------------------------------------------------------------------------------------------
def case_image_hw(N, H, W):
    """Image 0 fills the plane; the others are smaller than (H, W) where there is room, with a fraction to truncate."""
    hw = np.array([[float(H), float(W)]] * N, dtype=np.float32)
    for n in range(1, N):
        hw[n] = (max(H - 3, 1) + 0.75, max(W - 2, 1) + 0.5)
    return hw


def properties(bi, im_h, im_w, H, W):
    """The named classes one box's integers fall into, as a set."""
    bx1, by1, bx2, by2 = (int(v) for v in bi)
    x0, x1e, y0, y1e, w, h = window(bi, im_h, im_w)
    if bx2 < bx1 and by2 >= by1:
        return {"inverted"}
    if bx2 < bx1 or by2 < by1:
        return set()
    if x0 >= x1e or y0 >= y1e:
        return {"outside"}
    p = set()
    if bx1 >= 0 and by1 >= 0 and bx2 + 1 <= im_w and by2 + 1 <= im_h:
        p.add("inside")
    if bx1 < 0 <= bx2 and bx2 + 1 <= im_w:
        p.add("cross_left")
    if by1 < 0 <= by2 and by2 + 1 <= im_h:
        p.add("cross_top")
    if bx1 >= 0 and bx1 < W < bx2 + 1:
        p.add("cross_right")
    if by1 >= 0 and by1 < H < by2 + 1:
        p.add("cross_bottom")
    if bx1 < 0 and by1 < 0 and bx2 + 1 > W and by2 + 1 > H:
        p.add("larger")
    if bx1 == bx2 and by1 == by2:
        p.add("one_pixel")
    if (y1e - 1) // ROWS - y0 // ROWS >= 2:
        p.add("row_blocks")
    if (im_w < W and im_w < bx2 + 1 <= W) or (im_h < H and im_h < by2 + 1 <= H):
        p.add("cut_by_image_hw")
    return p


@functools.lru_cache(maxsize=None)
def paste_boxes(N, D, H, W, M, seed=0):
    """(boxes [N D][4] float32, image_hw [N][2] float32, names: per box the named class it was drawn for or "random").
    Slot k of the batch gets the first drawn box of class CLASSES[k] (judged with the image of slot k) whose int_margin
    is at least INT_MARGIN; a class the geometry has no room for leaves its slot to a random box."""
    rng = np.random.RandomState(1000 * seed + 31 * H + 7 * W + M)
    hw = case_image_hw(N, H, W)
    im_h, im_w = image_ints(hw, H, W)
    n_draw = 6000
    lo, hi = -0.6 * np.array([W, H]) - 3, 1.6 * np.array([W, H]) + 3
    p1 = rng.uniform(lo, hi, size=(n_draw, 2))
    p2 = rng.uniform(lo, hi, size=(n_draw, 2))
    cand = np.concatenate([p1, p2], axis=1)
    tiny = rng.uniform(0, [W, H], size=(1500, 2))
    cand = np.concatenate([cand, np.concatenate([tiny, tiny + rng.uniform(0.01, 0.2, size=(1500, 2))], axis=1)])
    c = rng.uniform(0.2, 0.8, size=(1500, 2)) * [W, H]
    s = rng.uniform(0.05, 0.3, size=(1500, 2)) * [W, H]
    cand = np.concatenate([cand, np.concatenate([c - s, c + s], axis=1)]).astype(np.float32)
    ok = int_margin(cand, M) >= INT_MARGIN
    bi, _ = box_integers(cand, M, np.float64)
    R = N * D
    boxes, names = np.zeros((R, 4), np.float32), ["random"] * R
    free = [i for i in range(len(cand)) if ok[i]]
    used = set()
    for k, name in enumerate(CLASSES[:R]):
        n = k // D
        for i in free:
            if i not in used and name in properties(bi[i], int(im_h[n]), int(im_w[n]), H, W):
                boxes[k], names[k] = cand[i], name
                used.add(i)
                break
    for k in range(R):
        if names[k] == "random":
            i = next(i for i in free if i not in used)
            used.add(i)
            boxes[k] = cand[i]
    return boxes, hw, tuple(names)


def paste_logits(R, classes, M, seed=0):
    """[R][classes][M][M] float32, spread over both sides of the sigmoid."""
    return (np.random.RandomState(77 + seed).standard_normal((R, classes, M, M)) * 2).astype(np.float32)


def paste_labels(R, classes, seed=0):
    return np.random.RandomState(5 + seed).randint(0, classes, size=R).astype(np.int32)


# ---- the lattice case --------------------------------------------------------------------------------------------------------
LATTICE_TARGETS = (-0.5, -0.25, 0.0, 1.0, -1.0, 2.0, -0.75, 3.0, -2.0, 0.5, 1.25, 4.0)   # the expanded low coordinate


def _lattice_axis(M, size, target, k):
    """(lo, hi) on multiples of 1/4 whose expanded low coordinate is exactly `target`; every second box (k odd) has an
    expanded high coordinate that is an integer too."""
    scale = (M + 2) / M
    for want_int in (bool(k % 2), False):     # (where no size gives an integer, any size)
        for j in range(1 + k % 3, 64):        # a few sizes
            s = j * M / 4                     # lo = target + s / M stays on the lattice
            lo, hi = target + s / M, target + s / M + s
            ehi = target + s * scale
            if (4 * lo) % 1 or (4 * hi) % 1 or ehi < 1.5 or (want_int and ehi % 1):
                continue
            return lo, hi
    raise AssertionError((M, size, target))


@functools.lru_cache(maxsize=None)
def lattice_boxes(N, D, H, W, M):
    """Boxes whose expanded coordinates are exact in fp32 and land on integers and on -0.5 / -0.25 / -0.75 (truncation
    toward zero gives 0 where floor would give -1).  Returns (boxes, image_hw); fp32 and fp64 integers agree exactly."""
    assert M in LATTICE_M
    R = N * D
    boxes = np.zeros((R, 4), np.float32)
    for r in range(R):
        x1, x2 = _lattice_axis(M, W, LATTICE_TARGETS[r % len(LATTICE_TARGETS)], r)
        y1, y2 = _lattice_axis(M, H, LATTICE_TARGETS[(r + 5) % len(LATTICE_TARGETS)], r + 1)
        boxes[r] = (x1, y1, x2, y2)
    e32, e64 = expand(boxes, M, np.float32), expand(boxes, M, np.float64)
    assert (e32.astype(np.float64) == e64).all()
    frac = e64 - np.floor(e64)
    assert (frac == 0).any() and ((e64 < 0) & (e64 > -1)).any()
    hw = np.array([[float(H), float(W)]] * N, dtype=np.float32)
    return boxes, hw
