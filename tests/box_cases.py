"""What the box tests share (not a test module): the fp64 numpy references of box decoding (BoxCoder.decode_single +
clip_boxes_to_image, with np.minimum / np.clip, which propagate NaN), of torchvision's AnchorGenerator and of greedy batched
NMS, the seeded case generators, and (at the end) the detector's per-stage references -- the RPN head, filter_proposals,
postprocess_detections -- each written so that it can be fed the GPU's own input to that stage, with the seeded detector
and its whole fp64 forward.

NMS boxes are drawn on a quarter-pixel lattice with sides of at most 128 pixels, so coordinates, sides, areas,
intersections and unions are exact in fp32 and an fp32 IoU is the correctly rounded quotient of the exact operands: it
differs from the fp64 IoU by under 3e-8 relative.  They come in clusters (a seed box plus jitter), so suppression happens.

A test may compare decisions exactly only where the reference's own decisions are robust, so the reference reports the
smallest margin of every decision it made, and the generator redraws a box whose decision is fragile:
  * IOU_MARGIN: no pair (kept i, later j of its group) has an fp64 IoU within 1e-5 of the threshold.  Those pairs are all
    the IoU decisions greedy NMS makes: a row that is not kept suppresses nothing;
  * size_margin(min_size): no side within 1e-4 + 1e-3 min_size of min_size;
  * SCORE_MARGIN: no score within 1e-6 of the threshold.
At most REDRAW_CAP of a case's boxes may be redrawn (a generator that throws most draws away shapes its inputs).
A decision that is exact in both precisions needs no margin: an IoU that is NaN, infinite or exactly 0 or 1, and the
sides of lattice boxes against an fp32 min_size.  EqualityCase is built of such decisions alone, with every compare at
equality; SweepNmsCase mixes degenerate and infinite boxes into the clusters and keeps the margins under every
combination of extreme thresholds; OffLatticeCase leaves the lattice; decode_sweep_cases() are 40 legal decode launches
over the column layouts, grids, weights, clamps and image sizes the library accepts."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

CLIP = math.log(1000.0 / 16)
IOU_MARGIN = 1e-5
SCORE_MARGIN = 1e-6
REDRAW_CAP = 0.01
LATTICE = 0.25
INF = float("inf")


def size_margin(min_size: float) -> float:
    return 1e-4 + 1e-3 * min_size


def rel_err(got, want) -> float:
    """The project's metric, max |got - want| / max |want|, over numpy arrays; NaNs must sit in the same places."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "NaNs differ"
    if nan.all():
        return 0.0
    err, scale = float(np.abs(got - want)[~nan].max()), float(np.abs(want[~nan]).max())
    if scale == 0.0:                      # an all-zero reference: only an all-zero result matches it
        return 0.0 if err == 0.0 else INF
    return err / scale


# ---- anchors and decode ----------------------------------------------------------------------------------------------------
def base_anchors(sizes, ratios) -> torch.Tensor:
    """torchvision's AnchorGenerator.generate_anchors in torch float32: [len(ratios) * len(sizes)][4], ratio-major."""
    scales = torch.as_tensor(sizes, dtype=torch.float32)
    ar = torch.as_tensor(ratios, dtype=torch.float32)
    h_r = torch.sqrt(ar)
    w_r = 1 / h_r
    ws = (w_r[:, None] * scales[None, :]).view(-1)
    hs = (h_r[:, None] * scales[None, :]).view(-1)
    return (torch.stack([-ws, -hs, ws, hs], dim=1) / 2).round()


def grid_anchors(base, h: int, w: int, stride_y: int, stride_x: int, dtype=np.float64) -> np.ndarray:
    """AnchorGenerator.grid_anchors: [h * w][A][4], rows in the order (y, x)."""
    base = np.asarray(base, dtype=dtype)
    ys, xs = np.divmod(np.arange(h * w), w)
    shift = np.stack([xs * stride_x, ys * stride_y, xs * stride_x, ys * stride_y], axis=1).astype(dtype)
    return base[None, :, :] + shift[:, None, :]


def decode_reference(head, anchors, image_hw, A: int, weights=(1.0, 1.0, 1.0, 1.0), grid=None, delta_col: int = 0,
                     clamp: float = CLIP, dtype=np.float64) -> np.ndarray:
    """head [rows][ld], anchors [A][4] with grid=(h, w, stride_y, stride_x) or [rows][4] without, image_hw [N][2] ->
    boxes [N][rows_per_image * A][4], every operation in `dtype`."""
    f = dtype
    head = np.asarray(head, dtype=f)
    hw = np.asarray(image_hw, dtype=f)
    rows, N = head.shape[0], hw.shape[0]
    rpi = rows // N
    if grid is None:
        a4 = np.broadcast_to(np.asarray(anchors, dtype=f)[:, None, :], (rows, A, 4))
    else:
        gh, gw, sy, sx = grid
        a4 = np.tile(grid_anchors(anchors, gh, gw, sy, sx, f), (N, 1, 1))
    d = head[:, delta_col:delta_col + 4 * A].reshape(rows, A, 4)
    wx, wy, ww, wh = (f(v) for v in weights)
    half = f(0.5)
    with np.errstate(all="ignore"):
        w, h = a4[..., 2] - a4[..., 0], a4[..., 3] - a4[..., 1]
        cx, cy = a4[..., 0] + half * w, a4[..., 1] + half * h
        dx, dy = d[..., 0] / wx, d[..., 1] / wy
        dw, dh = np.minimum(d[..., 2] / ww, f(clamp)), np.minimum(d[..., 3] / wh, f(clamp))
        pcx, pcy = dx * w + cx, dy * h + cy
        pw, ph = np.exp(dw) * w, np.exp(dh) * h
        Himg = np.repeat(hw[:, 0], rpi)[:, None]
        Wimg = np.repeat(hw[:, 1], rpi)[:, None]
        zero = f(0)
        out = np.stack([np.clip(pcx - half * pw, zero, Wimg), np.clip(pcy - half * ph, zero, Himg),
                        np.clip(pcx + half * pw, zero, Wimg), np.clip(pcy + half * ph, zero, Himg)], axis=-1)
    assert out.dtype == f
    return out.reshape(N, rpi * A, 4)


class DecodeCase:
    """Seeded inputs of one decode launch in the RPN's column layout (scores at 0..A, deltas at A..5A) for grid mode, in
    the box head's (scores at 0..A, deltas at A..5A of kp columns) for boxes mode.  A few dw / dh lie above the clamp."""

    def __init__(self, N, A, ld, grid=None, rows_per_image=None, weights=(1.0, 1.0, 1.0, 1.0), seed=0):
        rng = np.random.RandomState(seed)
        self.N, self.A, self.ld, self.grid, self.weights = N, A, ld, grid, tuple(float(v) for v in weights)
        self.rpi = grid[0] * grid[1] if grid else rows_per_image
        rows = N * self.rpi
        self.delta_col, self.score_col, self.clamp = A, 0, CLIP
        assert 5 * A <= ld
        head = rng.uniform(-1, 1, (rows, ld))
        d = head[:, A:5 * A].reshape(rows, A, 4)
        d[..., :2] = rng.uniform(-0.5, 0.5, (rows, A, 2))
        d[..., 2:] = rng.uniform(-1.0, 1.0, (rows, A, 2))
        above = rng.rand(rows, A, 2) < 0.06                       # dw / dh above the clamp: up to twice it
        d[..., 2:][above] = rng.uniform(CLIP, 2 * CLIP, int(above.sum()))
        d *= np.asarray(self.weights)
        head[:, A:5 * A] = d.reshape(rows, 4 * A)
        self.above = int(above.sum())
        self.head = head.astype(np.float32)
        if grid:
            gh, gw, sy, sx = grid
            sizes = tuple(8.0 * (1 + i) for i in range(max(A // 3, 1)))
            ratios = (0.5, 1.0, 2.0)[: A // len(sizes)] if A >= 3 else (1.0,)
            self.anchors = base_anchors(sizes, ratios).numpy()
            assert self.anchors.shape == (A, 4)
            # image sizes that are no multiple of the stride, one per image
            self.image_hw = np.array([[gh * sy - 1 - (n % 3), gw * sx - 2 - n] for n in range(N)], dtype=np.float32)
        else:
            x1 = rng.randint(0, 4 * 150, rows) * LATTICE
            y1 = rng.randint(0, 4 * 100, rows) * LATTICE
            self.anchors = np.stack([x1, y1, x1 + rng.randint(4, 4 * 60, rows) * LATTICE,
                                     y1 + rng.randint(4, 4 * 60, rows) * LATTICE], axis=1).astype(np.float32)
            self.image_hw = np.array([[131.0 + 7 * n, 197.0 - 5 * n] for n in range(N)], dtype=np.float32)

    def reference(self, head=None, dtype=np.float64):
        return decode_reference(self.head if head is None else head, self.anchors, self.image_hw, self.A, self.weights,
                                self.grid, self.delta_col, self.clamp, dtype)

    def scores(self):
        """The score column as the kernel copies it, [N][rows_per_image * A]; None without one."""
        if self.score_col is None:
            return None
        return self.head[:, self.score_col:self.score_col + self.A].reshape(self.N, self.rpi * self.A)


GRID_SHAPES = ((1, 1), (3, 5), (13, 21))
GRID_CASES = [dict(N=N, A=A, ld=ld, grid=(h, w, 8 if h > 1 else 16, 8 if h > 3 else 12))
              for (h, w), A, ld, N in (((1, 1), 1, 64, 1), ((1, 1), 3, 64, 3), ((1, 1), 12, 128, 1), ((3, 5), 1, 128, 3),
                                       ((3, 5), 3, 64, 1), ((3, 5), 12, 64, 3), ((13, 21), 1, 64, 1), ((13, 21), 3, 128, 3),
                                       ((13, 21), 12, 64, 1), ((13, 21), 12, 128, 3))]
BOX_MODE_CASES = [dict(N=N, A=classes, ld=-(-5 * classes // 64) * 64, rows_per_image=rows // N, weights=(10.0, 10.0, 5.0, 5.0))
                  for rows, classes, N in ((1, 1, 1), (63, 2, 1), (63, 91, 3), (65, 5, 1), (65, 1, 5), (257, 2, 1),
                                           (257, 5, 1), (1, 91, 1))]


@functools.lru_cache(maxsize=None)
def decode_case(index: int, boxes_mode: bool = False) -> DecodeCase:
    return DecodeCase(seed=100 * boxes_mode + index, **(BOX_MODE_CASES if boxes_mode else GRID_CASES)[index])


# ---- decode: a sweep over the legal launches -----------------------------------------------------------------------------
SWEEP_A = (1, 2, 3, 5, 12, 15, 91)
SWEEP_WEIGHTS = ((1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0), (-10.0, 10.0, -5.0, 5.0), (0.5, 0.25, 3.0, 7.0))
SWEEP_CLAMPS = (CLIP, 0.0, -1.0, INF)
SWEEP_HW = ("usual", "zero", "fractional", "nothing_clips")
SWEEP_GRIDS = ((1, 1), (1, 40), (40, 1), (3, 5), (13, 21), (40, 40), (7, 1), (1, 9), (24, 17), (2, 2))
SWEEP_STRIDES = ((8, 8), (16, 12), (1, 1), (1, 5), (4, 32))               # (stride_y, stride_x)
SWEEP_SLICES = ((0, 0), (37, 11), (5, 0), (0, 3))                         # (out_offset, room behind)
SWEEP_BOX_ROWS = (1, 255, 256, 257, 300)                                  # with A = 1, N = 1: total at the 256-thread block edge
LAYOUTS = ("scores_deltas", "deltas_scores", "deltas_only", "gap_deltas", "scores_gap_deltas", "deltas_pad_scores",
           "odd_everything")


def decode_layout(kind: str, A: int):
    """(ld, delta_col, score_col or None) of a named column layout: every legal relation of the three appears."""
    pad64 = lambda n: -(-n // 64) * 64
    return {"scores_deltas": (5 * A, A, 0),                       # the RPN's order, ld = 5A: delta_col + 4A == ld
            "deltas_scores": (5 * A, 0, 4 * A),                   # deltas before the scores, score_col + A == ld
            "deltas_only": (4 * A, 0, None),                      # ld = 4A, no score column
            "gap_deltas": (4 * A + 1, 1, None),                   # ld = 4A + 1, delta_col no multiple of 4
            "scores_gap_deltas": (5 * A + 3, A + 3, 0),           # ld = 5A + 3
            "deltas_pad_scores": (pad64(5 * A + 2), 2, pad64(5 * A + 2) - A),
            "odd_everything": (5 * A + 11, 7, 4 * A + 8)}[kind]    # scores after the deltas, room behind both


def decode_sweep_specs():
    """40 seeded legal launches, 30 in grid mode and 10 in boxes mode; tests/test_boxes_host.py asserts the pins."""
    rng = np.random.RandomState(77)
    pick = lambda seq: seq[rng.randint(len(seq))]
    specs = []
    for i in range(30):
        A, (gh, gw) = SWEEP_A[i % 7], SWEEP_GRIDS[i % 10]
        ld, delta_col, score_col = decode_layout(LAYOUTS[(i + i // 7) % 7], A)
        specs.append(dict(N=1 + i % 4, A=A, ld=ld, delta_col=delta_col, score_col=score_col,
                          grid=(gh, gw) + SWEEP_STRIDES[(i + i // 5) % 5], rows_per_image=None,
                          weights=SWEEP_WEIGHTS[(i + i // 4) % 4], clamp=pick(SWEEP_CLAMPS), hw=SWEEP_HW[(i + i // 8) % 4],
                          slice=pick(SWEEP_SLICES)))
    for i in range(10):
        edge = i < 5
        A = 1 if edge else SWEEP_A[(2 * i) % 7]
        ld, delta_col, score_col = decode_layout(LAYOUTS[(3 * i + 1) % 7], A)
        specs.append(dict(N=1 if edge else 2 + i % 3, A=A, ld=ld, delta_col=delta_col, score_col=score_col, grid=None,
                          rows_per_image=SWEEP_BOX_ROWS[i % 5] if edge else (1, 63, 65, 300, 17)[i % 5],
                          weights=SWEEP_WEIGHTS[(i + 1) % 4], clamp=SWEEP_CLAMPS[(i + i // 4) % 4], hw=SWEEP_HW[(i + i // 3) % 4],
                          slice=pick(SWEEP_SLICES)))
    return specs


class DecodeSweepCase(DecodeCase):
    """One launch of decode_sweep_specs().  dx, dy in +-0.5 and dw, dh in +-1 of a side, 6 % of dw / dh between the
    default clamp and twice it (exp stays below e^8.3 = 3900 whatever the clamp; none where nothing is to clip, so that
    one huge box does not set the scale of the error), all times the weights; every other column is noise.  Base anchors
    are lattice boxes around the origin.  image_hw: "usual" cuts through the boxes, "zero" clips every box to 0,
    "fractional" is the usual plus (0.5, 0.25), "nothing_clips" is larger than every box."""

    def __init__(self, spec, seed):
        rng = np.random.RandomState(seed)
        N, A, ld, grid = spec["N"], spec["A"], spec["ld"], spec["grid"]
        self.spec, self.N, self.A, self.ld, self.grid = spec, N, A, ld, grid
        self.weights, self.clamp = tuple(float(v) for v in spec["weights"]), float(spec["clamp"])
        self.delta_col, self.score_col = spec["delta_col"], spec["score_col"]
        self.offset, self.extra = spec["slice"]
        self.rpi = grid[0] * grid[1] if grid else spec["rows_per_image"]
        rows, dc, hw = N * self.rpi, self.delta_col, spec["hw"]
        assert ld >= 1 and 0 <= dc and dc + 4 * A <= ld and (self.score_col is None or 0 <= self.score_col <= ld - A)
        head = rng.uniform(-1, 1, (rows, ld))
        d = np.concatenate([rng.uniform(-0.5, 0.5, (rows, A, 2)), rng.uniform(-1.0, 1.0, (rows, A, 2))], axis=2)
        above = (rng.rand(rows, A, 2) < 0.06) & (hw != "nothing_clips")
        d[..., 2:][above] = rng.uniform(CLIP, 2 * CLIP, int(above.sum()))
        head[:, dc:dc + 4 * A] = (d * np.asarray(self.weights)).reshape(rows, 4 * A)
        self.above = int(above.sum())
        self.head = head.astype(np.float32)
        if grid:
            gh, gw, sy, sx = grid
            c = rng.randint(-16, 17, (A, 2)) * LATTICE
            half = rng.randint(4, 4 * 40, (A, 2)) * LATTICE
            self.anchors = np.concatenate([c - half, c + half], axis=1).astype(np.float32)
            span = np.array([gh * sy + 30.0, gw * sx + 30.0])
        else:
            x1, y1 = rng.randint(0, 4 * 150, rows) * LATTICE, rng.randint(0, 4 * 100, rows) * LATTICE
            self.anchors = np.stack([x1, y1, x1 + rng.randint(4, 4 * 60, rows) * LATTICE,
                                     y1 + rng.randint(4, 4 * 60, rows) * LATTICE], axis=1).astype(np.float32)
            span = np.array([160.0, 210.0])
        usual = np.array([np.floor(0.7 * span) + (1 + n % 3, 2 + n) for n in range(N)])
        self.image_hw = {"usual": usual, "zero": 0 * usual, "fractional": usual + (0.5, 0.25),
                         "nothing_clips": 0 * usual + 4096.0}[hw].astype(np.float32)


@functools.lru_cache(maxsize=None)
def decode_sweep_cases():
    return tuple(DecodeSweepCase(spec, 500 + i) for i, spec in enumerate(decode_sweep_specs()))


# ---- NMS -----------------------------------------------------------------------------------------------------------------
class NmsResult:
    """One segment's greedy walk: keep (ascending indices), and the smallest margins of the decisions it made."""

    def __init__(self):
        self.keep, self.iou_margin, self.size_margin, self.score_margin = [], INF, INF, INF
        self.fragile = set()


def nms_reference(boxes, scores=None, groups=None, iou_thresh=0.5, min_size=0.0, score_thresh=-INF, max_out=None,
                  dtype=np.float64, exact_sides=False) -> NmsResult:
    """Greedy NMS of one segment, boxes [R][4] in priority order, every operation in `dtype`.  Decisions that are exact in
    fp32 and fp64 alike need no margin and are not reported as fragile: an IoU that is NaN, infinite or exactly 0 or 1 (an
    empty intersection, or an intersection equal to the union, is the same in both); and, with `exact_sides` (the caller's
    word that the boxes are on the lattice and min_size is an fp32 number), the sides, whose differences are then exact."""
    f = dtype
    b = np.asarray(boxes, dtype=f)
    R = b.shape[0]
    res = NmsResult()
    thr, ms = f(iou_thresh), f(min_size)
    with np.errstate(all="ignore"):
        w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
        cand = (w >= ms) & (h >= ms)
        side = np.minimum(np.abs(w.astype(np.float64) - min_size), np.abs(h.astype(np.float64) - min_size))
        near = np.nan_to_num(side, nan=INF) < (-INF if exact_sides else size_margin(min_size))
        res.size_margin = float(np.nan_to_num(side, nan=INF).min()) if R else INF
        if scores is not None:
            sc = np.asarray(scores, dtype=f)
            cand &= sc >= f(score_thresh)
            if math.isfinite(score_thresh):
                gap = np.nan_to_num(np.abs(sc.astype(np.float64) - score_thresh), nan=INF)
                res.score_margin = float(gap.min()) if R else INF
                near |= gap < SCORE_MARGIN
        res.fragile |= set(np.nonzero(near)[0].tolist())
        area = w * h
        g = None if groups is None else np.asarray(groups)
        dead = ~cand
        limit = R if max_out is None else max_out
        zero = f(0)
        for i in range(R):
            if dead[i]:
                continue
            res.keep.append(i)
            if len(res.keep) >= limit:
                break
            j = slice(i + 1, R)
            iw = np.maximum(np.minimum(b[i, 2], b[j, 2]) - np.maximum(b[i, 0], b[j, 0]), zero)
            ih = np.maximum(np.minimum(b[i, 3], b[j, 3]) - np.maximum(b[i, 1], b[j, 1]), zero)
            inter = iw * ih
            iou = inter / (area[i] + area[j] - inter)
            live = cand[j] if g is None else cand[j] & (g[j] == g[i])
            dead[j] |= live & (iou > thr)
            exact = ~np.isfinite(iou) | (iou == zero) | (iou == f(1))
            gap = np.where(live & ~exact, np.abs(iou.astype(np.float64) - iou_thresh), INF)
            if gap.size:
                res.iou_margin = min(res.iou_margin, float(gap.min()))
                res.fragile |= set((np.nonzero(gap < IOU_MARGIN)[0] + i + 1).tolist())
    return res


def batched_nms_reference(boxes, scores=None, groups=None, iou_thresh=0.5, min_size=0.0, score_thresh=-INF, max_out=None,
                          dtype=np.float64, exact_sides=False):
    """boxes [S][R][4] -> (keep [S][max_out] int32 padded with -1, count [S] int32, rois [S][max_out][5] float32,
    [NmsResult per segment])."""
    S, R = boxes.shape[:2]
    max_out = max(R, 1) if max_out is None else max_out
    keep = np.full((S, max_out), -1, dtype=np.int32)
    count = np.zeros(S, dtype=np.int32)
    rois = np.zeros((S, max_out, 5), dtype=np.float32)
    rois[:, :, 0] = -1
    results = []
    for s in range(S):
        r = nms_reference(boxes[s], None if scores is None else scores[s], None if groups is None else groups[s],
                          iou_thresh, min_size, score_thresh, max_out, dtype, exact_sides)
        k = len(r.keep)
        keep[s, :k], count[s] = r.keep, k
        rois[s, :k, 0] = s
        rois[s, :k, 1:] = np.asarray(boxes[s], dtype=np.float32)[r.keep]
        results.append(r)
    return keep, count, rois, results


def _cluster_boxes(rng, n, seeds):
    """n lattice boxes around `seeds` [(x1, y1, w, h) in quarter pixels]: a seed plus jitter of up to a third of a side."""
    k = rng.randint(0, len(seeds), n)
    x1, y1, w, h = (seeds[k, c] for c in range(4))
    jit = lambda side: (rng.randint(-1000, 1001, n) * side) // 3000
    x1, y1 = x1 + jit(w), y1 + jit(h)
    w, h = np.maximum(w + jit(w), 1), np.maximum(h + jit(h), 1)
    return (np.stack([x1, y1, x1 + w, y1 + h], axis=1) * LATTICE).astype(np.float32)


VARIANTS = ((True, True), (True, False), (False, True), (False, False))   # (groups in use, scores in use)


class NmsCase:
    """S segments of R lattice boxes with descending scores and `n_groups` groups, drawn until the fp64 walk under PARAMS
    meets no fragile decision in any of its `variants` (a walk cut short by max_out makes a subset of the full walk's)."""

    PARAMS = dict(iou_thresh=0.5, min_size=2.1, score_thresh=0.2)

    def __init__(self, R, S, seed=0, n_groups=3, spread=None, variants=VARIANTS):
        rng = np.random.RandomState(seed)
        self.R, self.S, self.variants = R, S, variants
        self.boxes = np.zeros((S, R, 4), dtype=np.float32)
        self.scores = np.zeros((S, R), dtype=np.float32)
        self.groups = rng.randint(0, n_groups, (S, R)).astype(np.int32)
        self.drawn, self.redrawn = S * R, 0
        for s in range(S):
            seeds = self._seeds(rng, max(1, R // 6) if spread is None else spread)
            self.boxes[s] = self._draw(rng, R, seeds)
            self.scores[s] = np.sort(rng.uniform(0.05, 1.0, R).astype(np.float32))[::-1]
            self._plant(rng, s)
            for _ in range(50):
                bad = set()
                for use_groups, use_scores, p in self._walks():
                    bad |= nms_reference(self.boxes[s], self.scores[s] if use_scores else None,
                                         self.groups[s] if use_groups else None, **p).fragile
                bad = sorted(bad)
                if not bad:
                    break
                self.redrawn += len(bad)
                self.boxes[s, bad] = self._draw(rng, len(bad), seeds)
                fresh = rng.uniform(0.05, 1.0, len(bad)).astype(np.float32)
                self.scores[s, bad] = fresh
                order = np.argsort(-self.scores[s], kind="stable")
                self.boxes[s], self.scores[s], self.groups[s] = self.boxes[s][order], self.scores[s][order], self.groups[s][order]
            else:
                raise AssertionError("the generator does not converge")

    @staticmethod
    def _seeds(rng, n_seeds):
        seeds = np.stack([rng.randint(0, 4 * 1600, n_seeds), rng.randint(0, 4 * 1200, n_seeds),
                          rng.randint(4, 4 * 96, n_seeds), rng.randint(4, 4 * 96, n_seeds)], axis=1)
        seeds[rng.rand(n_seeds) < 0.08, 2] = rng.randint(0, 12)              # some thin boxes, around min_size
        return seeds

    _draw = staticmethod(_cluster_boxes)

    def _plant(self, rng, s):
        """Boxes of a subclass's own put into segment s after the first draw (a fragile one is redrawn like any other)."""

    def _walks(self):
        """(groups in use, scores in use, the reference's parameters) of every walk the case must keep its margins in."""
        for use_groups, use_scores in self.variants:
            p = dict(self.PARAMS)
            if not use_scores:
                p.pop("score_thresh")
            yield use_groups, use_scores, p

    def expected(self, use_groups=True, use_scores=True, max_out=None):
        return _expected(self, use_groups, use_scores, max_out)


@functools.lru_cache(maxsize=None)
def _expected(case, use_groups, use_scores, max_out):
    p = dict(case.PARAMS)
    if not use_scores:
        p.pop("score_thresh")
    return batched_nms_reference(case.boxes, case.scores if use_scores else None, case.groups if use_groups else None,
                                 max_out=max_out, **p)


NMS_R = (1, 2, 63, 64, 65, 128, 129, 257, 700, 2049)
NMS_S = (1, 2, 5)
# one segment each past 64, 128 and 256 words of 64 boxes: the scan kernel's three wider instantiations.  Clusters of
# 40 boxes and two variants only: a walk of 16400 boxes takes the reference a second
NMS_WIDE_R = (4100, 8200, 16400)
WIDE_VARIANTS = (VARIANTS[0], VARIANTS[3])


# nb == W of three scan instantiations (R = 64 W) and the largest R the library takes, one segment each.  The 32768 case
# has 410 clusters (80 boxes each, so the walk is shorter) and the (groups, scores) variant only.  Host cost measured on
# a CPU: building the three cases takes 0.3 s, 2.6 s and 5.5 s, one fp64 reference walk 0.1 s, 0.8 s and 2.5 s
# (R = 32768: 7380 kept, 16 of 32768 boxes redrawn); the GPU test of R = 32768 took 4.1 s in all, the walks included
NMS_LIMIT_R = (4096, 16384, 32768)
NMS_MAX_R = 32768


@functools.lru_cache(maxsize=None)
def nms_case(R: int, S: int) -> NmsCase:
    if R == NMS_MAX_R:
        return NmsCase(R, S, seed=7 * R + S, spread=410, variants=VARIANTS[:1])
    if R in NMS_WIDE_R or R in NMS_LIMIT_R:
        return NmsCase(R, S, seed=7 * R + S, spread=R // 40, variants=WIDE_VARIANTS)
    return NmsCase(R, S, seed=7 * R + S)


class ClassCase:
    """Six segments of R = 48 boxes, one property each (names in NAMES), under PARAMS with groups."""

    NAMES = ("nothing_kept", "all_kept", "all_identical", "more_than_max_out", "groups_apart", "clusters")
    PARAMS = dict(iou_thresh=0.5, min_size=2.1)
    R, MAX_OUT = 48, 20

    def __init__(self):
        R = self.R
        rng = np.random.RandomState(11)
        grid = np.array([[40.0 * (i % 8), 40.0 * (i // 8), 40.0 * (i % 8) + 30.0, 40.0 * (i // 8) + 30.0] for i in range(R)],
                        dtype=np.float32)
        one = np.tile(np.array([[10.0, 20.0, 50.25, 70.5]], dtype=np.float32), (R, 1))
        flat = grid.copy()
        flat[:, 2] = flat[:, 0]                                       # zero width: below min_size
        pairs = grid[np.arange(R) // 2]                               # each box twice ...
        self.boxes = np.stack([flat, grid, one, grid, pairs, nms_case(R, 1).boxes[0]])
        self.groups = np.zeros((6, R), dtype=np.int32)
        self.groups[4] = np.arange(R) % 2                             # ... in two groups
        self.groups[5] = rng.randint(0, 3, R)

    def expected(self, use_groups=True, max_out=MAX_OUT):
        return batched_nms_reference(self.boxes, None, self.groups if use_groups else None, max_out=max_out, **self.PARAMS)


@functools.lru_cache(maxsize=None)
def class_case() -> ClassCase:
    return ClassCase()


# ---- NMS: every compare at equality -------------------------------------------------------------------------------------
def f32_below(v: float) -> float:
    return float(np.nextafter(np.float32(v), np.float32(-INF)))


def f32_above(v: float) -> float:
    return float(np.nextafter(np.float32(v), np.float32(INF)))


class EqualityCase:
    """16 segments of R = 130 lattice boxes whose every decisive quantity is exact in fp32 and fp64 alike, so a compare may
    sit at equality: the expected result is the fp64 reference's, and the fp32 restatement must give the same.
      * a pair (first, second) of PAIRS, IoU exactly PAIRS[k][2], at the rows PLACES[p] of segment 4 k + p: lanes 0 and 63
        of one block (the tie is in the diagonal word), rows 63 / 64 and 0 / 129 (an off-diagonal word), lanes 0 and 63
        of block 1.  Pairs 2 and 3 have sides of exactly 2.0 and 0.25, the two min_size values; the first of a pair has
        the score threshold as its score in every other segment, so what it suppresses hangs on `>=`;
      * every other row is a box that overlaps nothing, with a side of min_size - 0.25, min_size, min_size + 0.25 for both
        min_size values in turn, as its width or as its height, and a score of the threshold, its fp32 neighbour below,
        its neighbour above or 0.9; the rotation moves with the segment, so each of rows 0, 63, 64 and 129 has, in some
        segment, a side equal to either min_size and a score equal to the threshold."""

    R, S = 130, 16
    PLACES = ((0, 63), (63, 64), (0, 129), (64, 127))
    PAIRS = (((0, 0, 8, 4), (0, 0, 4, 4), 0.5), ((0, 0, 4, 4), (0, 0, 3, 4), 0.75), ((0, 0, 4, 2), (0, 0, 2, 2), 0.5),
             ((0, 0, 0.5, 0.25), (0, 0, 0.25, 0.25), 0.5))
    MIN_SIZES = (2.0, 0.25)
    SCORE_THRESH = 0.25
    SIDES = (1.75, 2.0, 2.25, 0.0, 0.25, 0.5, 8.0, 8.0)

    def __init__(self):
        R, S, thr = self.R, self.S, self.SCORE_THRESH
        score_of = np.array([f32_below(thr), thr, f32_above(thr), 0.9], dtype=np.float32)
        self.boxes = np.zeros((S, R, 4), dtype=np.float32)
        self.scores = np.zeros((S, R), dtype=np.float32)
        self.groups = np.tile((np.arange(R) % 3).astype(np.int32), (S, 1))
        self.pair_rows = []
        for s in range(S):
            r = np.arange(R)
            q = r + s + s // 4
            side = np.asarray(self.SIDES)[q % 8]
            tall = (q // 8) % 2 == 1
            w, h = np.where(tall, 8.0, side), np.where(tall, side, 8.0)
            self.boxes[s] = np.stack([32.0 * r, 0 * r, 32.0 * r + w, h], axis=1)
            self.scores[s] = score_of[q % 4]
            (i, j), (first, second, _) = self.PLACES[s % 4], self.PAIRS[s // 4]
            at = np.array([32.0 * i, 64.0, 32.0 * i, 64.0])
            self.boxes[s, i], self.boxes[s, j] = np.asarray(first) + at, np.asarray(second) + at
            self.scores[s, i] = thr if s % 2 == 0 else 0.9
            self.scores[s, j] = thr if s % 3 == 0 else f32_above(thr)
            self.groups[s, [i, j]] = 1
            self.pair_rows.append((i, j))
        assert np.array_equal(self.boxes, np.round(self.boxes * 4) / 4)

    @staticmethod
    def runs():
        """(iou_thresh, min_size) of every run: each pair's IoU and its fp32 neighbours, at both min_size values."""
        return [(t, ms) for v in (0.5, 0.75) for t in (f32_below(v), v, f32_above(v)) for ms in EqualityCase.MIN_SIZES]

    def expected(self, iou_thresh, min_size, use_groups=True, max_out=None, dtype=np.float64):
        return _equality_expected(self, iou_thresh, min_size, use_groups, max_out, dtype)


@functools.lru_cache(maxsize=None)
def _equality_expected(c, iou_thresh, min_size, use_groups, max_out, dtype):
    return batched_nms_reference(c.boxes, c.scores, c.groups if use_groups else None, iou_thresh, min_size, c.SCORE_THRESH,
                                 max_out, dtype)


@functools.lru_cache(maxsize=None)
def equality_case() -> EqualityCase:
    return EqualityCase()


# ---- NMS: the parameter and geometry sweep -----------------------------------------------------------------------------
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
SWEEP_R = (65, 257)
SWEEP_IOU = (-1.0, 0.0, 0.25, 0.75, 1.0, 2.0)
SWEEP_MIN_SIZE = (-INF, -1.0, 0.0, 2.1)
SWEEP_SCORE_THRESH = (None, -INF, 0.2, INF)          # None: no scores operand
SWEEP_GROUPS = (INT32_MIN, -1, 0, 7, INT32_MAX)
SPECIALS = ("zero_width", "zero_height", "zero_area_pair", "inverted_x", "inverted_y", "inverted_both", "touching",
            "x1_neg_inf", "x2_pos_inf", "all_inf", "x2_neg_inf", "y1_pos_inf")


def sweep_combos(iou_thresh=None):
    """(iou_thresh, min_size, score_thresh or None, groups in use) of every run of the sweep (of one iou_thresh when
    given); one run in three goes without groups."""
    out = []
    for a, iou in enumerate(SWEEP_IOU):
        for b, ms in enumerate(SWEEP_MIN_SIZE):
            for c, st in enumerate(SWEEP_SCORE_THRESH):
                if iou_thresh is None or iou == iou_thresh:
                    out.append((iou, ms, st, (a + b + c) % 3 != 0))
    return out


class SweepNmsCase(NmsCase):
    """The lattice cluster case with a fifth of each segment replaced by the boxes of SPECIALS (each kind in every
    segment, at seeded rows) and group ids from SWEEP_GROUPS, keeping its margins in every run of sweep_combos().  The
    sides need none: lattice sides are exact and every min_size but 2.1 is an fp32 number (2.1 is 0.1 from the lattice)."""

    def __init__(self, R, S=3, seed=0):
        super().__init__(R, S, seed=seed, n_groups=len(SWEEP_GROUPS))
        self.groups = np.asarray(SWEEP_GROUPS, dtype=np.int64)[self.groups].astype(np.int32)

    def _plant(self, rng, s):
        R, b = self.R, self.boxes[s]
        n = max(R // 5, len(SPECIALS) + 1)
        rows = rng.choice(R, n, replace=False)
        kinds = [SPECIALS[k % len(SPECIALS)] for k in range(n)]
        for k, (r, kind) in enumerate(zip(rows.tolist(), kinds)):
            x1, y1, x2, y2 = b[r].tolist()
            if kind == "zero_width":
                b[r] = (x1, y1, x1, y2)
            elif kind == "zero_height":
                b[r] = (x1, y1, x2, y1)
            elif kind == "zero_area_pair":                        # this row and the next planted one: the same zero-area box
                b[r] = b[rows[(k + 1) % n]] = (x1, y1, x1, y1)
            elif kind == "inverted_x":
                b[r] = (x2, y1, x1, y2)
            elif kind == "inverted_y":
                b[r] = (x1, y2, x2, y1)
            elif kind == "inverted_both":
                b[r] = (x2, y2, x1, y1)
            elif kind == "touching":                               # shares an edge with another row's box: intersection 0
                o = b[(r + 1) % R].tolist()
                b[r] = (o[2], o[1], o[2] + (x2 - x1), o[3])
            elif kind == "x1_neg_inf":
                b[r] = (-INF, y1, x2, y2)
            elif kind == "x2_pos_inf":
                b[r] = (x1, y1, INF, y2)
            elif kind == "all_inf":
                b[r] = (-INF, -INF, INF, INF)
            elif kind == "x2_neg_inf":
                b[r] = (x1, y1, -INF, y2)
            elif kind == "y1_pos_inf":
                b[r] = (x1, INF, x2, y2)

    def _walks(self):
        for iou, ms, st, use_groups in sweep_combos():
            p = dict(iou_thresh=iou, min_size=ms, exact_sides=ms != 2.1)
            if st is not None:
                p["score_thresh"] = st
            yield use_groups, st is not None, p

    def expected(self, combo, max_out=None, dtype=np.float64):
        return _sweep_expected(self, combo, max_out, dtype)


@functools.lru_cache(maxsize=None)
def _sweep_expected(c, combo, max_out, dtype):
    iou, ms, st, use_groups = combo
    return batched_nms_reference(c.boxes, None if st is None else c.scores, c.groups if use_groups else None, iou, ms,
                                 -INF if st is None else st, max_out, dtype)


@functools.lru_cache(maxsize=None)
def sweep_nms_case(R: int) -> SweepNmsCase:
    return SweepNmsCase(R, 3, seed=31 * R)


# ---- NMS: boxes off the lattice ---------------------------------------------------------------------------------------
OFF_LATTICE_R = (300, 3000)


class OffLatticeCase(NmsCase):
    """Clustered boxes with arbitrary fp32 coordinates in a 1333 x 800 frame, sides log-uniform in 4 .. 300 pixels around
    R / 50 seeds with a jitter of up to a third of a side: what a decode hands NMS.  Products and sums round in fp32
    here; the margins of the lattice cases (IOU_MARGIN is thirty times an fp32 IoU's error) are kept by redrawing."""

    PARAMS = dict(iou_thresh=0.5, min_size=4.5, score_thresh=0.2)

    def __init__(self, R, S=2, seed=0):
        super().__init__(R, S, seed=seed, spread=max(R // 50, 1), variants=WIDE_VARIANTS)

    @staticmethod
    def _seeds(rng, n_seeds):
        side = np.exp(rng.uniform(math.log(4.0), math.log(300.0), (n_seeds, 2)))
        return np.concatenate([rng.uniform(0, 1333, (n_seeds, 1)), rng.uniform(0, 800, (n_seeds, 1)), side], axis=1)

    @staticmethod
    def _draw(rng, n, seeds):
        k = rng.randint(0, len(seeds), n)
        x1, y1, w, h = (seeds[k, c] for c in range(4))
        jit = lambda side: rng.uniform(-1, 1, n) * side / 3
        x1, y1, w, h = x1 + jit(w), y1 + jit(h), w + jit(w), h + jit(h)
        return np.stack([x1, y1, x1 + w, y1 + h], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def off_lattice_case(R: int) -> OffLatticeCase:
    return OffLatticeCase(R, 2, seed=R)


# ---- NMS: many segments -------------------------------------------------------------------------------------------------
ONE_BOX_PARAMS = dict(iou_thresh=0.5, min_size=2.0, score_thresh=0.25)


@functools.lru_cache(maxsize=None)
def one_box_sources(K: int = 300):
    """K segments of one lattice box each, a candidate or not by a side (1.75, 2.0, 2.25 and larger, against min_size 2.0)
    and by its score (the threshold 0.25, its fp32 neighbours, and others): (boxes [K][1][4], scores [K][1], and the
    reference's keep / count / rois at max_out = 1)."""
    rng = np.random.RandomState(5)
    x1, y1 = rng.randint(0, 4000, K) * LATTICE, rng.randint(0, 4000, K) * LATTICE
    w = np.asarray([1.75, 2.0, 2.25, 40.0, 7.5])[rng.randint(0, 5, K)]
    h = np.asarray([1.75, 2.0, 2.25, 13.25, 90.0])[rng.randint(0, 5, K)]
    boxes = np.stack([x1, y1, x1 + w, y1 + h], axis=1).astype(np.float32).reshape(K, 1, 4)
    scores = np.asarray([f32_below(0.25), 0.25, f32_above(0.25), 0.05, 0.9], dtype=np.float32)[rng.randint(0, 5, K)]
    scores = scores.reshape(K, 1)
    keep, count, rois, _ = batched_nms_reference(boxes, scores, None, max_out=1, **ONE_BOX_PARAMS)
    return boxes, scores, keep, count, rois


def tile_segments(src_keep, src_count, src_rois, S: int):
    """The expected outputs of S segments that repeat K source segments cyclically (segment s is source s % K): the
    sources' keep and count, and their rois with column 0 set to s wherever a box was kept (float32 holds s < 2^24)."""
    assert S <= 1 << 24
    idx = np.arange(S) % src_keep.shape[0]
    keep, count, rois = src_keep[idx], src_count[idx], src_rois[idx]
    own = np.broadcast_to(np.arange(S, dtype=np.float32)[:, None], rois.shape[:2])
    rois[:, :, 0] = np.where(rois[:, :, 0] >= 0, own, np.float32(-1))
    return keep, count, rois


# ---- the detector: per-stage fp64 references, each usable on the GPU's own input to that stage --------------------------------
RPN_LEVELS = ("0", "1", "2", "3", "pool")
DETECTOR = dict(arch="resnet18", out_channels=64, classes=5, N=2, H=64, W=96, pre=50, post=20, detections=10, rep=128, P=7,
                seed=6)
BOX_WEIGHTS = (10.0, 10.0, 5.0, 5.0)
SCORE_THRESH = float(np.nextafter(np.float32(0.05), np.float32(1)))
RPN_PARAMS = dict(iou_thresh=0.7, min_size=1e-3, score_thresh=0.0)
DET_PARAMS = dict(iou_thresh=0.5, min_size=1e-2, score_thresh=SCORE_THRESH)


def detector_state_dict(resnet_module):
    """The seeded torchvision-named state dict of DETECTOR: backbone.*, rpn.*, roi_heads.* (float32)."""
    import fpn_reference
    import roi_cases
    d = DETECTOR
    C, A = d["out_channels"], 3
    fpn_sd, body = fpn_reference.fpn_random_state_dict(torch, resnet_module, d["arch"], C, seed=d["seed"])
    g = torch.Generator().manual_seed(d["seed"] + 99)
    rn = lambda *s: torch.randn(*s, generator=g)
    sd = {"backbone." + k: v for k, v in fpn_sd.items()}
    sd["rpn.head.conv.0.0.weight"] = rn(C, C, 3, 3) * (2.0 / (9 * C)) ** 0.5
    sd["rpn.head.conv.0.0.bias"] = rn(C) * 0.1
    sd["rpn.head.cls_logits.weight"] = rn(A, C, 1, 1) * (4.0 / C) ** 0.5
    sd["rpn.head.cls_logits.bias"] = rn(A) * 0.1
    sd["rpn.head.bbox_pred.weight"] = rn(4 * A, C, 1, 1) * (0.5 / C) ** 0.5
    sd["rpn.head.bbox_pred.bias"] = rn(4 * A) * 0.05
    head = roi_cases.box_head_state_dict(C, d["P"], d["rep"], d["classes"], seed=d["seed"])
    head["box_predictor.cls_score.weight"] = head["box_predictor.cls_score.weight"] * 2
    sd.update({"roi_heads." + k: v for k, v in head.items()})
    return sd, fpn_sd, body


def detector_input():
    d = DETECTOR
    return torch.rand(d["N"], 3, d["H"], d["W"], generator=torch.Generator().manual_seed(d["seed"] + 1)) - 0.5


def rpn_head_reference(sd, feats):
    """fp64 RPNHead on NHWC level maps {"0".."pool"} -> per level [N * h * w][5A]: A objectness logits, then 4A deltas."""
    F = torch.nn.functional
    w = {k[len("rpn.head."):]: v.double() for k, v in sd.items() if k.startswith("rpn.head.")}
    out = []
    for name in RPN_LEVELS:
        x = feats[name].double().permute(0, 3, 1, 2)
        t = torch.relu(F.conv2d(x, w["conv.0.0.weight"], w["conv.0.0.bias"], padding=1))
        cls = F.conv2d(t, w["cls_logits.weight"], w["cls_logits.bias"]).permute(0, 2, 3, 1)
        box = F.conv2d(t, w["bbox_pred.weight"], w["bbox_pred.bias"]).permute(0, 2, 3, 1)
        out.append(torch.cat([cls, box], dim=3).reshape(-1, cls.shape[3] * 5))
    return out


def min_gap(values) -> float:
    """The smallest distance between two neighbours of each row once sorted: 0 means a tie, whose order is nobody's."""
    v = np.sort(np.asarray(values, dtype=np.float64), axis=1)
    return float(np.diff(v, axis=1).min()) if v.shape[1] > 1 else INF


def filter_proposals_reference(boxes, logits, n_per_level, pre, post):
    """torchvision's filter_proposals on all levels' decoded boxes [N][total][4] and logits [N][total] (torch, any float
    dtype): per-level topk, one stable descending sort per image, greedy NMS in fp64 with groups = level."""
    idx, off = [], 0
    for n in n_per_level:
        idx.append(logits[:, off:off + n].topk(min(pre, n), dim=1, sorted=True).indices + off)
        off += n
    level = torch.cat([torch.full((min(pre, n),), l, dtype=torch.int32) for l, n in enumerate(n_per_level)])
    idx = torch.cat(idx, dim=1)
    slogit, order = torch.sort(logits.gather(1, idx), dim=1, descending=True, stable=True)
    sidx = idx.gather(1, order)
    sboxes = boxes.gather(1, sidx[:, :, None].expand(-1, -1, 4))
    prob = torch.sigmoid(slogit)
    r = dict(idx=idx, sorted_logits=slogit, sorted_boxes=sboxes, sorted_levels=level[order], sorted_scores=prob,
             tie_gap=min_gap(logits.numpy()))
    r.update(nms_stage(sboxes, prob, level[order], post, RPN_PARAMS))
    return r


def nms_stage(boxes, scores, groups, max_out, params):
    keep, count, rois, results = batched_nms_reference(boxes.numpy(), scores.numpy(), groups.numpy(), max_out=max_out, **params)
    return dict(keep=keep, count=count, rois=rois, iou_margin=min(r.iou_margin for r in results),
                size_margin=min(r.size_margin for r in results), score_margin=min(r.score_margin for r in results))


def postprocess_reference(head_out, rois, image_hw, classes, detections, max_candidates=None):
    """torchvision's postprocess_detections on the box head's packed output [R][>= 5 classes] (logits, then deltas), the
    proposals rois [R][5] (padding rows of index -1) and image_hw [N][2]: fp64 softmax and decode, the candidates' topk,
    greedy NMS in fp64 with groups = label."""
    N, R = image_hw.shape[0], rois.shape[0]
    per, fg = R // N, classes - 1
    prob = torch.softmax(head_out[:, :classes].double(), dim=-1)
    boxes = decode_reference(head_out.numpy(), rois[:, 1:5].numpy(), image_hw.numpy(), classes, BOX_WEIGHTS, None, classes)
    boxes = torch.from_numpy(boxes).view(N, per, classes, 4)[:, :, 1:].reshape(N, per * fg, 4)
    valid = (rois[:, 0] >= 0).view(N, per, 1)
    scores = (prob.view(N, per, classes)[:, :, 1:] * valid).reshape(N, per * fg)
    return dict(prob=prob, boxes=boxes, scores=scores)


def candidates_reference(boxes, scores, fg, detections, max_candidates=None):
    """The second half, on class boxes [N][M][4] and scores [N][M] (torch): topk, NMS, the padded detections."""
    M = scores.shape[1]
    kc = max(1, min(M, 8192 if max_candidates is None else max_candidates))
    top = scores.topk(kc, dim=1, sorted=True)
    cboxes = boxes.gather(1, top.indices[:, :, None].expand(-1, -1, 4))
    labels = (top.indices % fg + 1).to(torch.int32)
    r = dict(idx=top.indices, cand_boxes=cboxes, cand_scores=top.values, cand_labels=labels,
             overflow=(scores >= SCORE_THRESH).sum(dim=1) > kc,
             tie_gap=min_gap(np.where(scores.numpy() >= SCORE_THRESH / 2, scores.numpy(), -np.arange(M)[None, :] - 1.0)))
    r.update(nms_stage(cboxes, top.values, labels, detections, DET_PARAMS))
    keep = torch.from_numpy(r["keep"]).long()
    kept, at = keep >= 0, keep.clamp(min=0)
    r["det_boxes"] = cboxes.gather(1, at[:, :, None].expand(-1, -1, 4)) * kept[:, :, None]
    r["det_scores"] = top.values.gather(1, at) * kept
    r["det_labels"] = torch.where(kept, labels.gather(1, at).long(), torch.full_like(at, -1))
    return r


def detector_margins(filt, cand) -> dict:
    """The smallest decision margins the two NMS stages and the tie checks met."""
    return dict(iou=min(filt["iou_margin"], cand["iou_margin"]), size_rpn=filt["size_margin"], size_det=cand["size_margin"],
                score=min(filt["score_margin"], cand["score_margin"]), tie=min(filt["tie_gap"], cand["tie_gap"]))


def assert_margins(m: dict, factor: float = 1.0) -> None:
    """The generator's margins, times `factor`.  A side's margin is capped at min_size itself: a box clipped to an edge
    of the image has a side of exactly 0 in every precision, and no side lies further below min_size than that."""
    assert m["iou"] >= factor * IOU_MARGIN, m
    for key, p in (("size_rpn", RPN_PARAMS), ("size_det", DET_PARAMS)):
        assert m[key] >= min(factor * size_margin(p["min_size"]), p["min_size"]), m
    assert m["score"] >= factor * SCORE_MARGIN and m["tie"] > 0, m


def detector_reference_forward(resnet_module):
    """The whole detector of DETECTOR in fp64 on the CPU, stage by stage: a dict of every intermediate."""
    import fpn_reference
    import roi_cases
    d = DETECTOR
    sd, fpn_sd, body = detector_state_dict(resnet_module)
    x = detector_input()
    N, H, W, A = d["N"], d["H"], d["W"], 3
    feats = fpn_reference.fpn_reference_forward(torch, fpn_sd, body, x)
    image_hw = np.array([[float(H), float(W)]] * N)
    heads = rpn_head_reference(sd, feats)
    boxes, logits, n_per_level = [], [], []
    for l, name in enumerate(RPN_LEVELS):
        h, w = feats[name].shape[1:3]
        base = base_anchors((32.0 * 2 ** l,), (0.5, 1.0, 2.0)).numpy()
        boxes.append(decode_reference(heads[l].numpy(), base, image_hw, A, grid=(h, w, H // h, W // w), delta_col=A))
        logits.append(heads[l][:, :A].reshape(N, h * w * A))
        n_per_level.append(h * w * A)
    boxes, logits = torch.from_numpy(np.concatenate(boxes, axis=1)), torch.cat(logits, dim=1)
    filt = filter_proposals_reference(boxes, logits, n_per_level, d["pre"], d["post"])
    rois = torch.from_numpy(filt["rois"]).double().view(N * d["post"], 5)
    maps = [feats[k] for k in RPN_LEVELS[:4]]
    scales = [maps[l].shape[1] / H for l in range(4)]
    levels = roi_cases.threshold_levels(rois, scales, 224.0, 4)
    pooled = roi_cases.roi_align_reference(maps, rois, d["P"], scales, 2, levels)
    head_sd = {k[len("roi_heads."):]: v for k, v in sd.items() if k.startswith("roi_heads.")}
    cls, reg = roi_cases.box_head_reference(head_sd, pooled)
    post = postprocess_reference(torch.cat([cls, reg], dim=1), rois, torch.from_numpy(image_hw), d["classes"], d["detections"])
    cand = candidates_reference(post["boxes"], post["scores"], d["classes"] - 1, d["detections"])
    return dict(sd=sd, x=x, feats=feats, heads=heads, boxes=boxes, logits=logits, filt=filt, pooled=pooled, cls=cls, reg=reg,
                post=post, cand=cand, margins=detector_margins(filt, cand))
