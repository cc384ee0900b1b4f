"""The reference and the seeded cases of the segmented top-k / sort kernel (select.hip), shared by
tests/test_select_host.py, tests/test_gpu_select.py and tests/test_gpu_select_detector.py.

The reference is numpy: a sort of the 64-bit composite key (orderable(score) << 32) | (0xffffffff - index), with
orderable(x) = ~bits when the sign bit is set, else bits | 0x80000000, -0 mapped to +0 and every NaN to 0xffffffff
first.  tests/test_select_host.py shows that it is torch.sort(descending=True, stable=True) truncated to k.

Case classes (each a function (n, seed) -> float32 [n]): distinct, ties, zeros, nans, extremes.  threshold_points(x)
gives the thresholds a case is run at: a value that occurs and its fp32 neighbours on both sides."""
import functools

import numpy as np

F32_MAX = np.float32(3.4028234663852886e38)
DENORM = np.float32(1.401298464324817e-45)


def orderable(x: np.ndarray) -> np.ndarray:
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()
    nan = (b & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    b[b == np.uint32(0x80000000)] = 0
    neg = (b & np.uint32(0x80000000)) != 0
    key = np.where(neg, ~b, b | np.uint32(0x80000000))
    key[nan] = np.uint32(0xffffffff)
    return key


def composite(x: np.ndarray) -> np.ndarray:
    index = np.arange(x.shape[-1], dtype=np.uint64)
    return (orderable(x).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xffffffff) - index)


def topk_order(x: np.ndarray, k: int, thresh=None) -> np.ndarray:
    """Indices of the best min(k, candidates) elements of the 1-d float32 x, best first."""
    key = composite(x)
    order = np.argsort(key, kind="stable")[::-1]   # (the keys are unique)
    if thresh is not None:
        with np.errstate(invalid="ignore"):
            ok = x >= np.float32(thresh)           # (a NaN fails)
        order = order[ok[order]]
    return order[:k].astype(np.int64)


def _parts(stride, k, n, off):
    ks = list(k) if isinstance(k, (list, tuple)) else [int(k)]
    offs = [0] * len(ks) if off is None else (list(off) if isinstance(off, (list, tuple)) else [int(off)])
    ns = [stride - o for o in offs] if n is None else (list(n) if isinstance(n, (list, tuple)) else [int(n)])
    return ks, ns, offs


def full_orders(scores, ns, offs, thresh=None):
    """orders[i][p] = topk_order(image i's part p, 8192, thresh): computed once per input, a smaller k is its prefix."""
    return [[topk_order(scores[i, o:o + n], 8192, thresh) for n, o in zip(ns, offs)] for i in range(scores.shape[0])]


def expected(orders, scores, ks, offs, boxes=None):
    """(idx [N][sum k] int32, vals [N][sum k] float32, count [N][parts] int32, boxes [N][sum k][4] or None) as
    wino_select_topk_hw writes them, from full_orders' result."""
    N, parts, ksum = scores.shape[0], len(ks), sum(ks)
    idx = np.full((N, ksum), -1, dtype=np.int32)
    vals = np.zeros((N, ksum), dtype=np.float32)
    count = np.zeros((N, parts), dtype=np.int32)
    ob = None if boxes is None else np.zeros((N, ksum, 4), dtype=np.float32)
    for i in range(N):
        base = 0
        for p in range(parts):
            order = orders[i][p][:ks[p]] + offs[p]
            c = len(order)
            count[i, p] = c
            idx[i, base:base + c] = order
            vals[i, base:base + c] = scores[i, order]
            if ob is not None:
                ob[i, base:base + c] = boxes[i, order]
            base += ks[p]
    return idx, vals, count, ob


def select_reference(scores: np.ndarray, k, n=None, off=None, thresh=None, boxes=None):
    ks, ns, offs = _parts(scores.shape[1], k, n, off)
    return expected(full_orders(scores, ns, offs, thresh), scores, ks, offs, boxes)


# ---- case classes -------------------------------------------------------------------------------------------------------
def distinct(n, seed):
    return np.random.RandomState(seed).standard_normal(n).astype(np.float32)


TIE_VALUES = np.array([-3.5, -1.0, 0.0, 0.25, 0.25 + 2 ** -22, 2.0, 1e30], dtype=np.float32)


def ties(n, seed):
    rng = np.random.RandomState(seed)
    x = TIE_VALUES[rng.randint(len(TIE_VALUES), size=n)].copy()
    u = rng.rand(n)
    x[u < 0.05] = np.nan
    x[(u >= 0.05) & (u < 0.10)] = -0.0
    return x


def zeros(n, seed):
    return np.zeros(n, dtype=np.float32)


def nans(n, seed):
    return np.full(n, np.nan, dtype=np.float32)


EXTREME_VALUES = np.array([np.inf, -np.inf, 0.0, -0.0, DENORM, -DENORM, F32_MAX, -F32_MAX, 1.0, -1.0], dtype=np.float32)


def extremes(n, seed):
    rng = np.random.RandomState(seed)
    x = EXTREME_VALUES[rng.randint(len(EXTREME_VALUES), size=n)].copy()
    x[: min(n, len(EXTREME_VALUES))] = EXTREME_VALUES[:n]   # each of them at least once where n allows
    return x


CLASSES = {"distinct": distinct, "ties": ties, "zeros": zeros, "nans": nans, "extremes": extremes}


@functools.lru_cache(maxsize=None)
def _case(name, N, n, seed):
    x = np.stack([CLASSES[name](n, seed * 1000 + i) for i in range(N)]) if N else np.zeros((0, n), np.float32)
    x.setflags(write=False)
    return x


def case(name, N, n, seed=0):
    """float32 [N][n] of the class, read-only and shared between the tests."""
    return _case(name, int(N), int(n), int(seed))


def boxes_for(scores: np.ndarray) -> np.ndarray:
    """A payload [N][n][4] that names its row: (image, index, -index, NaN on every 7th row)."""
    N, n = scores.shape
    b = np.empty((N, n, 4), dtype=np.float32)
    b[:, :, 0] = np.arange(N, dtype=np.float32)[:, None]
    b[:, :, 1] = np.arange(n, dtype=np.float32)[None, :]
    b[:, :, 2] = -b[:, :, 1]
    b[:, :, 3] = 0.5
    b[:, ::7, 3] = np.nan
    return b


def threshold_points(x: np.ndarray):
    """A finite value that occurs in x (the median of the finite ones) and its fp32 neighbours below and above."""
    f = x[np.isfinite(x)]
    v = np.float32(np.sort(f.ravel())[f.size // 2]) if f.size else np.float32(0.0)
    return [float(np.nextafter(v, np.float32(-np.inf))), float(v), float(np.nextafter(v, np.float32(np.inf)))]


# ---- the shapes of tests/test_gpu_select.py -------------------------------------------------------------------------------
SIZES_N = [1, 2, 63, 64, 65, 1023, 1024, 1025, 4819, 8192, 8193, 70001]
SIZES_K = [1, 2, 64, 65, 1000, 8192]
IMAGES = [1, 2, 5]


# ---- the kernel on the guarded arena ------------------------------------------------------------------------------------------
GARBAGE = 0x5A5A5A5A   # the second run's fill of outputs and workspace (the first run's is NaN)


def run_select(pkg, dev, scores, k, n=None, off=None, thresh=None, boxes=None, aligns=None, tag="", orders=None,
               with_vals=True):
    """select_topk on numpy operands on the guarded arena at each of `aligns` (default: both placements): a run into
    NaN-filled outputs and workspace, a second into garbage-filled ones, each compared exactly with the reference (ints
    equal, values and boxes bit for bit); the arena check proves that nothing beside the tensors changed.  The workspace
    is exactly what select_workspace_bytes reports.  with_vals=False goes through the C entry point itself with vals =
    NULL; the vals tensor carved alongside must then keep its fill.  Returns (idx, vals, count, boxes) as numpy arrays."""
    import torch

    import guarded
    N, stride = scores.shape
    ks, ns, offs = _parts(stride, k, n, off)
    parts, ksum = len(ks), sum(ks)
    orders = full_orders(scores, ns, offs, thresh) if orders is None else orders
    want = expected(orders, scores, ks, offs, boxes)
    need = pkg.select_workspace_bytes(N, ns, ks)
    got = None
    for align in (guarded.ALIGNS if aligns is None else aligns):
        arena = guarded.Arena(torch, dev, align)
        sc_t = arena.input(torch.from_numpy(np.array(scores, dtype=np.float32)), name="scores")
        bx_t = None if boxes is None else arena.input(torch.from_numpy(boxes), name="boxes")
        idx = arena.output(N, ksum, name="idx").view(torch.int32)
        vals = arena.output(N, ksum, name="vals")
        count = arena.output(N, parts, name="count").view(torch.int32)
        ob = None if boxes is None else arena.output(N, ksum, 4, name="boxes_out")
        ws = arena.workspace(need, name="workspace") if need else None
        for fill in (guarded.NAN_BITS, GARBAGE):
            for t in (idx, vals, count, ob, ws):
                if t is not None:
                    t.view(torch.int32).fill_(fill)
            if with_vals:
                res = pkg.select_topk(sc_t, ks, ns, offs, thresh, bx_t, idx, vals, count, ob, ws)
                assert res[0] is idx and res[1] is vals and res[2] is count and (ob is None or res[3] is ob)
            else:
                p = lambda t: None if t is None else (t.data_ptr() or None)
                rc = pkg.lib().wino_select_topk_hw(
                    p(sc_t), N, stride, parts, (pkg.c_long * parts)(*offs), (pkg.c_int * parts)(*ns), (pkg.c_int * parts)(*ks),
                    0 if thresh is None else 1, 0.0 if thresh is None else float(thresh), p(idx), None, p(count), ksum,
                    p(bx_t), 0 if bx_t is None else stride, p(ob), p(ws), 0 if ws is None else ws.numel() * 4, pkg._stream())
                pkg._check(rc, "wino_select_topk_hw")
            where = f"select_topk {tag} N={N} n={ns} k={ks} off={offs} thresh={thresh} align={align} fill={fill:#x}"
            arena.check(where)
            got = (idx.cpu().numpy(), vals.cpu().numpy(), count.cpu().numpy(), None if ob is None else ob.cpu().numpy())
            assert np.array_equal(got[2], want[2]), (where, got[2].tolist(), want[2].tolist())
            assert np.array_equal(got[0], want[0]), (where, np.nonzero(got[0] != want[0]))
            if with_vals:
                assert np.array_equal(got[1].view(np.int32), want[1].view(np.int32)), where
            else:
                assert (got[1].view(np.int32) == np.int32(fill)).all(), f"{where}: vals = NULL was written"
            if ob is not None:
                assert np.array_equal(got[3].view(np.int32), want[3].view(np.int32)), where
    return got
