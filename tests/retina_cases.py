"""The cases and the guarded-arena runs of RetinaNet's two kernels, shared by tests/test_retinanet_host.py,
tests/test_gpu_select_map.py and tests/test_gpu_retina_decode.py.

select_topk_map: a segment is handed over as its flat scores [N][n], n = h w cols, and poisoned_map lays them into the
interior of a padded NHWC map whose ring and pad columns hold NaN and +Inf alternately -- the two greatest keys of the
order, so a single stray read of them lands in the output.  The reference is tests/select_cases.py's numpy sort on the
flat scores.  retina_decode: DecodeLevel is one level's regression map (ring and pad columns NaN), base anchors, image
sizes and a seeded idx with padding rows."""
import functools

import numpy as np

import select_cases as sc

MAP_HW = ((1, 1), (3, 5), (7, 11), (13, 21))
MAP_COLS = ((1, 64), (9, 64), (45, 64), (819, 832))
MAP_IMAGES = (1, 3)
MAP_K = (1, 100, 1000)
MAP_CLASSES = ("distinct", "ties", "zeros", "nans")     # all distinct, ties across the cut, all equal, all NaN
# n = 2048 m - 1, 2048 m, 2048 m + 1 (one pixel, cols = n): around the chunk of a radix pass, on the one-launch side of 8192
# (m = 1, 4) and beyond it (m = 5)
CHUNK_N = tuple(2048 * m + d for m in (1, 4, 5) for d in (-1, 0, 1))


def pad64(v: int) -> int:
    return (int(v) + 63) // 64 * 64


def poisoned_map(flat: np.ndarray, h: int, w: int, cols: int, ld: int) -> np.ndarray:
    """flat [N][h w cols] -> float32 [N][h+2][w+2][ld]: the scores at [1 + y][1 + x][c], NaN and +Inf everywhere else."""
    N = flat.shape[0]
    m = np.full((N, h + 2, w + 2, ld), np.nan, dtype=np.float32)
    m.reshape(-1)[1::2] = np.inf
    m[:, 1:-1, 1:-1, :cols] = flat.reshape(N, h, w, cols)
    return m


def run_select_map(pkg, dev, flat, h, w, cols, ld, ks, thresh=None, aligns=None, tag="", out_offset=0, extra=0):
    """select_topk_map on the poisoned map of `flat` on the guarded arena at each of `aligns`, for every k of `ks`
    (clipped to n by the caller): a run into NaN-filled outputs and workspace, a second into garbage-filled ones, idx /
    vals / count compared exactly with the reference on the flat scores; the columns outside [out_offset, out_offset + k)
    keep both fills, and the arena check proves that nothing beside the tensors changed.  The workspace is exactly what
    select_map_workspace_bytes reports.  Returns {k: (idx, vals, count)}."""
    import torch

    import guarded
    N, n = flat.shape
    assert n == h * w * cols
    orders = sc.full_orders(flat, [n], [0], thresh)
    master = torch.from_numpy(poisoned_map(flat, h, w, cols, ld))
    got = {}
    for align in (guarded.ALIGNS if aligns is None else aligns):
        arena = guarded.Arena(torch, dev, align)
        m_t = arena.input(master, name="map")
        width = out_offset + max(ks) + extra
        idx = arena.output(N, width, name="idx").view(torch.int32)
        vals = arena.output(N, width, name="vals")
        count = arena.output(N, name="count").view(torch.int32)
        for k in ks:
            want = sc.expected(orders, flat, [k], [0])
            need = pkg.select_map_workspace_bytes(N, h, w, cols, k)
            assert need == pkg.select_workspace_bytes(N, n, k)
            ws = arena.workspace(need, name="workspace") if need else None
            for fill in (guarded.NAN_BITS, sc.GARBAGE):
                for t in (idx, vals, count, ws):
                    if t is not None:
                        t.view(torch.int32).fill_(fill)
                res = pkg.select_topk_map(m_t, cols, k, thresh, idx, vals, count, out_offset, ws)
                assert res[0] is idx and res[1] is vals and res[2] is count
                where = (f"select_topk_map {tag} N={N} h={h} w={w} cols={cols} ld={ld} k={k} thresh={thresh} align={align} "
                         f"fill={fill:#x} out_offset={out_offset}")
                arena.check(where)
                gi, gv, gc = idx.cpu().numpy(), vals.cpu().numpy(), count.cpu().numpy()
                outside = np.ones(width, dtype=bool)
                outside[out_offset:out_offset + k] = False
                for t in (gi, gv):
                    assert (t[:, outside].view(np.int32) == np.int32(fill)).all(), f"{where}: written outside the slice"
                gi, gv = gi[:, out_offset:out_offset + k], gv[:, out_offset:out_offset + k]
                assert np.array_equal(gc, want[2][:, 0]), (where, gc.tolist(), want[2][:, 0].tolist())
                assert np.array_equal(gi, want[0]), (where, np.nonzero(gi != want[0]))
                assert np.array_equal(gv.view(np.int32), want[1].view(np.int32)), where
                got[k] = (gi.copy(), gv.copy(), gc.copy())
    return got


MAP_SWEEP_COUNT = 24


@functools.lru_cache(maxsize=None)
def map_sweep_specs():
    """MAP_SWEEP_COUNT seeded legal layouts: N 1..3, h x w up to 13 x 21, cols anywhere in 1..ld with ld a multiple of 64
    up to 256 (so n lies on both sides of 8192), k 1..8192, a slice (out_offset, room behind) of a wider buffer, a class
    and a coin for a threshold.  The first two are pinned: a long segment into a slice, and cols == ld."""
    rng = np.random.RandomState(20252)
    names = sorted(sc.ALL_CLASSES)
    specs = []
    for index in range(MAP_SWEEP_COUNT):
        h, w = int(rng.randint(1, 14)), int(rng.randint(1, 22))
        ld = 64 * int(rng.randint(1, 5))
        cols = int(rng.choice([1, ld, rng.randint(1, ld + 1)]))
        N = int(rng.randint(1, 4))
        k = int(rng.choice([1, 2, 64, 65, 1000, 8192, rng.randint(1, 8193)]))
        off, extra = int(rng.choice([0, 0, 3, 37, 1000])), int(rng.choice([0, 0, 5, 64]))
        name = names[rng.randint(len(names))]
        thresh = [None, ("point", int(rng.randint(3)))][rng.randint(2)]
        if index == 0:
            N, h, w, cols, ld, k, off, extra, name = 2, 13, 21, 100, 128, 1000, 37, 11, "ties"
        elif index == 1:
            N, h, w, cols, ld, k, off, extra, name = 3, 5, 7, 64, 64, 300, 0, 0, "bits"
        specs.append(dict(index=index, N=N, h=h, w=w, cols=cols, ld=ld, k=min(k, h * w * cols), off=off, extra=extra,
                          name=name, thresh=thresh))
    return specs


def map_sweep_case(index):
    """(flat scores [N][n], the threshold or None) of spec `index`."""
    s = map_sweep_specs()[index]
    flat = sc.case(s["name"], s["N"], s["h"] * s["w"] * s["cols"], seed=500 + index)
    t = None if s["thresh"] is None else sc.threshold_points(flat)[s["thresh"][1]]
    return flat, t


# ---- retina_decode -----------------------------------------------------------------------------------------------------------
DECODE_HW = ((1, 1), (3, 5), (7, 11), (13, 21))
DECODE_A = (1, 9)
DECODE_K = (1, 5, 91)
RETINA_SIZES = ((32, 40, 50), (64, 80, 101), (128, 161, 203), (256, 322, 406), (512, 645, 812))
RETINA_RATIOS = (0.5, 1.0, 2.0)


def torchvision_base_anchors(scales, aspect_ratios) -> np.ndarray:
    """AnchorGenerator.generate_anchors transcribed to numpy float32, operation by operation: h_ratios = sqrt(ratios),
    w_ratios = 1 / h_ratios, ws = (w_ratios[:, None] * scales[None, :]).view(-1), hs likewise,
    round(stack([-ws, -hs, ws, hs], 1) / 2) with round-half-to-even."""
    scales = np.asarray(scales, dtype=np.float32)
    ratios = np.asarray(aspect_ratios, dtype=np.float32)
    h_ratios = np.sqrt(ratios)
    w_ratios = (np.float32(1) / h_ratios).astype(np.float32)
    ws = (w_ratios[:, None] * scales[None, :]).reshape(-1).astype(np.float32)
    hs = (h_ratios[:, None] * scales[None, :]).reshape(-1).astype(np.float32)
    return np.round(np.stack([-ws, -hs, ws, hs], axis=1) / np.float32(2)).astype(np.float32)


class DecodeLevel:
    """One level of `N` images: a regression map [N][h+2][w+2][ld_r] with the deltas of anchor a at columns 4a .. 4a + 3 of
    the interior pixels (a few dw / dh above the clamp) and NaN in the ring and the pad columns, base anchors [A][4], image
    sizes that are no multiple of the stride, and idx [N][rows]: per image `rows` distinct indices of the level's
    h w A K in random order, the last rows - count[i] of them -1."""

    def __init__(self, N, h, w, A, K, rows, seed=0):
        import box_cases as bc
        rng = np.random.RandomState(seed)
        self.N, self.h, self.w, self.A, self.K, self.ld = N, h, w, A, K, pad64(4 * A)
        self.grid = (h, w, 8 if h > 1 else 16, 8 if h > 3 else 12)
        d = np.empty((N, h, w, A, 4))
        d[..., :2] = rng.uniform(-0.5, 0.5, (N, h, w, A, 2))
        d[..., 2:] = rng.uniform(-1.0, 1.0, (N, h, w, A, 2))
        above = rng.rand(N, h, w, A, 2) < 0.06
        d[..., 2:][above] = rng.uniform(bc.CLIP, 2 * bc.CLIP, int(above.sum()))
        self.deltas = d.astype(np.float32)
        sizes = tuple(8.0 * (1 + i) for i in range(max(A // 3, 1)))
        ratios = (0.5, 1.0, 2.0) if A >= 3 else (1.0,)
        self.base = bc.base_anchors(sizes, ratios).numpy()
        assert self.base.shape == (A, 4)
        gh, gw, sy, sx = self.grid
        self.image_hw = np.array([[gh * sy - 1 - (n % 3), gw * sx - 2 - n] for n in range(N)], dtype=np.float32)
        total = h * w * A * K
        self.rows = rows
        self.count = np.array([min(total, max(rows - 3 * i - 1, 0)) for i in range(N)], dtype=np.int32)
        self.idx = np.full((N, rows), -1, dtype=np.int32)
        for i in range(N):
            self.idx[i, :self.count[i]] = rng.permutation(total)[:self.count[i]] if total < 1 << 20 else \
                rng.randint(0, total, self.count[i])

    def reg_map(self, deltas=None) -> np.ndarray:
        m = np.full((self.N, self.h + 2, self.w + 2, self.ld), np.nan, dtype=np.float32)
        m[:, 1:-1, 1:-1, :4 * self.A] = (self.deltas if deltas is None else deltas).reshape(self.N, self.h, self.w, 4 * self.A)
        return m

    def head_rows(self, deltas=None) -> np.ndarray:
        """The interior as box_decode's rows [N h w][ld] (pad columns zero)."""
        rows = np.zeros((self.N * self.h * self.w, self.ld), dtype=np.float32)
        rows[:, :4 * self.A] = (self.deltas if deltas is None else deltas).reshape(-1, 4 * self.A)
        return rows

    def gather(self, level_boxes: np.ndarray):
        """(boxes [N][rows][4], labels [N][rows]) of idx from a whole level's boxes [N][h w A][4]: zero box and label -1
        where idx < 0."""
        boxes = np.zeros((self.N, self.rows, 4), dtype=level_boxes.dtype)
        labels = np.full((self.N, self.rows), -1, dtype=np.int32)
        for i in range(self.N):
            live = self.idx[i] >= 0
            boxes[i, live] = level_boxes[i, self.idx[i, live] // self.K]
            labels[i, live] = self.idx[i, live] % self.K
        return boxes, labels


@functools.lru_cache(maxsize=None)
def decode_level(h, w, A, K, N=2, rows=37):
    return DecodeLevel(N, h, w, A, K, rows, seed=1000 * h + 10 * A + K)


def run_retina_decode(pkg, dev, c, deltas=None, offset=0, extra=0, aligns=None, tag=""):
    """retina_decode on level `c` on the guarded arena, into [N][offset + rows + extra] outputs, twice, bitwise equal;
    what lies outside the slice keeps its NaN fill.  Returns this launch's slice of (boxes, labels)."""
    import torch

    import guarded
    from gpu_support import as_f32
    total, first = offset + c.rows + extra, None
    idx_full = np.full((c.N, total), -7, dtype=np.int32)          # (rows outside the slice are never read as indices)
    idx_full[:, offset:offset + c.rows] = c.idx
    for align in (guarded.ALIGNS if aligns is None else aligns):
        arena = guarded.Arena(torch, dev, align)
        idx = arena.input(as_f32(idx_full), name="idx").view(torch.int32)
        reg = arena.input(torch.from_numpy(c.reg_map(deltas)), name="reg")
        base = arena.input(torch.from_numpy(c.base), name="base")
        hw = arena.input(torch.from_numpy(c.image_hw), name="image_hw")
        ob = arena.output(c.N, total, 4, name="boxes")
        ol = arena.output(c.N, total, name="labels").view(torch.int32)
        for _ in range(2):
            ob.fill_(float("nan")), ol.fill_(guarded.NAN_BITS)
            got = pkg.retina_decode(idx, reg, base, hw, c.grid, c.K, c.rows, ob, ol, offset)
            assert got[0] is ob and got[1] is ol
            arena.check(f"retina_decode {tag} align={align}")
            b, l = ob.cpu().numpy(), ol.cpu().numpy()
            outside = np.ones(total, dtype=bool)
            outside[offset:offset + c.rows] = False
            assert np.isnan(b[:, outside]).all() and (l[:, outside] == guarded.NAN_BITS).all(), "wrote outside its slice"
            cur = (b[:, offset:offset + c.rows].copy(), l[:, offset:offset + c.rows].copy())
            if first is None:
                first = cur
            assert np.array_equal(cur[0].view(np.int32), first[0].view(np.int32)) and np.array_equal(cur[1], first[1]), \
                f"{tag}: not bitwise reproducible (align {align})"
    return first
