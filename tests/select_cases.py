"""The reference and the seeded cases of the segmented top-k / sort kernel (select.hip), shared by
tests/test_select_host.py, tests/test_gpu_select.py and tests/test_gpu_select_detector.py.

The reference is numpy: a sort of the 64-bit composite key (orderable(score) << 32) | (0xffffffff - index), with
orderable(x) = ~bits when the sign bit is set, else bits | 0x80000000, -0 mapped to +0 and every NaN to 0xffffffff
first.  tests/test_select_host.py shows that it is torch.sort(descending=True, stable=True) truncated to k.

Case classes (each a function (n, seed) -> float32 [n]): distinct, ties, zeros, nans, extremes (CLASSES), and, built from
bit patterns through from_orderable, the inverse of orderable: uniform random patterns and keys that differ in their low
10 or 21 bits only (RADIX_CLASSES).  threshold_points(x) gives the thresholds a case is run at: a value that occurs and
its fp32 neighbours on both sides.  radix_corner builds a segment whose k-th key lies at a named corner of find_digit in a
named pass, radix_hits restates what find_digit then meets; sweep_specs is the seeded list of legal layouts."""
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


# ---- classes built from bit patterns, for the radix passes ------------------------------------------------------------------
def from_orderable(key) -> np.ndarray:
    """The float32 whose orderable() is `key`: the inverse on every key that is no NaN's and not -0's (0x7fffffff)."""
    key = np.asarray(key, dtype=np.uint32)
    return np.where((key & np.uint32(0x80000000)) != 0, key & np.uint32(0x7fffffff), ~key).astype(np.uint32).view(np.float32)


def bit_patterns(n, seed):
    """Uniform 32-bit patterns: NaNs of both signs and any payload (0.8 % of them), denormals, both zeros."""
    return np.random.RandomState(seed).randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32)


def _narrow(low_bits, prefix):
    def make(n, seed):
        low = np.random.RandomState(seed).randint(0, 1 << low_bits, size=n).astype(np.uint32)
        return from_orderable(np.uint32(prefix & ~((1 << low_bits) - 1)) | low)
    return make


# 10 random low key bits: only pass 2 discriminates; 21: passes 1 and 2.  Keys 0xbf8..... are floats in [1, 1.25), keys
# 0x407..... floats in (-1.25, -1]
RADIX_CLASSES = {"bits": bit_patterns,
                 "narrow10": _narrow(10, 0xbf8a5c00), "narrow10_neg": _narrow(10, 0x40712c00),
                 "narrow21": _narrow(21, 0xbf800000), "narrow21_neg": _narrow(21, 0x40600000)}
ALL_CLASSES = dict(CLASSES, **RADIX_CLASSES)

PASS_SHIFT, PASS_BITS = (21, 10, 0), (11, 11, 10)      # select.hip's three digits, from the top
CORNER_PLACES = ("first", "last", "zero", "top")       # where the k-th key's digit lies (find_digit: a thread owns
CORNER_KINDS = ("kr1", "full", "full_highest")         # 8 bins in passes 0 and 1, 4 in pass 2), and the rank left in it
_D0, _D1 = 1530, 777                                   # the digits of the passes before the one a case aims at


def radix_corner(n, k, p, place, kind, seed=0):
    """float32 [n] whose k-th largest key has, in pass p, its digit at `place` -- the first or last bin a find_digit
    thread owns, bin 0 (passes 1 and 2), the histogram's last bin (in pass 0 that is NaN) -- with a rank left inside
    that bin of 1 (kind "kr1": k - 1 keys in higher bins) or equal to the bin's count ("full": k // 2 keys in higher
    bins; "full_highest": none, the bin is the highest occupied one).  None where the combination cannot be: bin 0 in
    pass 0 holds no score, nothing lies above the last bin, and k = 1 leaves no room above."""
    bins, sh = 1 << PASS_BITS[p], PASS_SHIFT[p]
    if (place == "zero" and p == 0) or n <= k:
        return None
    a = {"kr1": k - 1, "full": k // 2, "full_highest": 0}[kind]
    if (place == "top" or kind == "full_highest" or k == 1) and a > 0:
        return None
    if kind == "full" and a == 0:
        return None
    c = min(3, n - a - 1) if kind == "kr1" else k - a
    rng = np.random.RandomState(seed * 7919 + 31 * p + len(place) + 3 * len(kind) + k)
    mid = 1536 if p < 2 else 512
    d = {"first": mid, "last": mid - 1, "zero": 0, "top": bins - 1}[place]
    prefix = (0, _D0, (_D0 << 11) | _D1)[p]

    def keys(count, digit_lo, digit_hi, pre=prefix, shift=sh, width=PASS_BITS[p]):
        """`count` keys with the prefix `pre`, a digit in [digit_lo, digit_hi] and random bits below."""
        digit = rng.randint(digit_lo, digit_hi + 1, size=count).astype(np.uint64)
        low = rng.randint(0, 1 << shift, size=count).astype(np.uint64) if shift else np.zeros(count, np.uint64)
        return ((np.uint64(pre) << np.uint64(shift + width)) | (digit << np.uint64(shift)) | low).astype(np.uint32)

    top_digit = 2040 if p == 0 else bins - 1               # (pass 0: below +Inf's bin)
    d0 = d if p == 0 else _D0
    below = n - a - c
    near = below // 2 if (p > 0 and d > 0) else 0          # below, in the same histogram; the rest in lower pass-0 bins
    far_hi = min(d0 - 1, 2040)
    parts = [keys(c, d, d), keys(a, d + 1, top_digit) if a else np.zeros(0, np.uint32),
             keys(near, 0, d - 1) if near else np.zeros(0, np.uint32),
             keys(below - near, 8, far_hi, pre=0, shift=21, width=11)]
    x = from_orderable(np.concatenate(parts))
    return x[rng.permutation(n)]


def radix_corner_specs(k):
    """Every (pass, place, kind) radix_corner builds at this k."""
    return [(p, place, kind) for p in range(3) for place in CORNER_PLACES for kind in CORNER_KINDS
            if radix_corner(k + 8, k, p, place, kind) is not None]


def radix_hits(x, k):
    """What find_digit meets in each pass when it looks for the k-th largest key of x, restated with numpy: a set of
    (pass, corner), corner one of CORNER_PLACES, "highest" (no occupied bin above the digit's), "kr1" and "krfull"."""
    key = orderable(x).astype(np.uint64)
    T = np.sort(key)[::-1][k - 1]
    hits = set()
    for p, (sh, width) in enumerate(zip(PASS_SHIFT, PASS_BITS)):
        bins, own = 1 << width, (1 << width) >> 8
        hi, t = key >> np.uint64(sh), T >> np.uint64(sh)
        d = int(t) & (bins - 1)
        in_hist = (key >> np.uint64(sh + width)) == (T >> np.uint64(sh + width))
        kr, count = k - int((hi > t).sum()), int((hi == t).sum())
        assert 1 <= kr <= count
        found = {"first": d % own == 0, "last": d % own == own - 1, "zero": d == 0, "top": d == bins - 1,
                 "highest": not ((hi > t) & in_hist).any(), "kr1": kr == 1, "krfull": kr == count}
        hits |= {(p, name) for name, yes in found.items() if yes}
    return hits


@functools.lru_cache(maxsize=None)
def _case(name, N, n, seed):
    x = np.stack([ALL_CLASSES[name](n, seed * 1000 + i) for i in range(N)]) if N else np.zeros((0, n), np.float32)
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


# ---- a seeded sweep of legal layouts ------------------------------------------------------------------------------------------
SWEEP_COUNT = 40
SPECIAL_THRESHOLDS = [float("inf"), float("-inf"), 0.0, -0.0, float(DENORM), -float(DENORM), float(F32_MAX)]


def _sweep_k(rng, parts):
    ks = [int(rng.choice([1, 2, 64, 65, 1000, 8192, rng.randint(1, 8193)])) for _ in range(parts)]
    while sum(ks) > 12000:
        ks[int(np.argmax(ks))] = max(1, max(ks) // 2)
    return ks


@functools.lru_cache(maxsize=None)
def sweep_specs():
    """SWEEP_COUNT deterministic specs of legal calls: N 1..4, 1..8 parts of length 0, 1, short, 8192, 8193 or long (up
    to 30000) at offsets with random gaps and now and then an overlap, k 1..8192 with sum k <= 12000, a class per part,
    and a coin each for a threshold, boxes, a wider boxes_stride, a wider out_stride and vals = NULL.  The first three are
    pinned: the layouts tests/test_select_host.py asks the list for do not hang on the seed alone."""
    rng = np.random.RandomState(20251)
    names = sorted(ALL_CLASSES)
    specs = []
    for index in range(SWEEP_COUNT):
        N, parts = int(rng.randint(1, 5)), int(rng.randint(1, 9))
        ns = [int(rng.choice([0, 1, rng.randint(2, 8192), 8192, 8193, rng.randint(8194, 30001)])) for _ in range(parts)]
        classes = [names[rng.randint(len(names))] for _ in range(parts)]
        ks = _sweep_k(rng, parts)
        thresh = [None, ("point", int(rng.randint(3))), ("value", SPECIAL_THRESHOLDS[rng.randint(7)])][rng.randint(3)]
        if index == 0:       # long parts after short ones and short ones after long, an empty part
            N, ns, ks = 4, [300, 20481, 8193, 0, 12294, 77], [300, 1000, 8192, 5, 64, 100]
            classes = ["ties", "distinct", "bits", "zeros", "narrow10", "extremes"]
        elif index == 1:     # 24 segments
            N, ns, ks = 3, [8193, 1, 500, 9000, 8192, 2, 10000, 64], [64, 3, 500, 1, 1000, 2, 65, 64]
            classes = (names * 2)[:8]
        elif index == 2:     # fewer candidates than k in a long part: a seventh of the ties reach the threshold
            N, ns, ks, classes, thresh = 2, [700, 9000], [100, 4000], ["distinct", "ties"], ("value", float(TIE_VALUES[-1]))
        parts = len(ns)
        offs, cursor = [], int(rng.randint(0, 8))
        for p in range(parts):
            start = cursor + int(rng.randint(0, 50))
            if p and rng.rand() < 0.15:
                start = max(0, cursor - int(rng.randint(1, 200)))      # overlaps what lies before it
            offs.append(start | 1 if rng.rand() < 0.5 else start)
            cursor = max(cursor, offs[-1] + ns[p])
        stride = cursor + int(rng.randint(0, 30))
        ksum = sum(ks)
        specs.append(dict(index=index, N=N, n=ns, off=offs, k=ks, classes=classes, stride=max(stride, 1), thresh=thresh,
                          boxes=bool(rng.rand() < 0.6), boxes_stride=max(stride, 1) + int(rng.choice([0, 0, 1, 37])),
                          out_stride=ksum + int(rng.choice([0, 0, 3, 64])), with_vals=bool(rng.rand() < 0.75)))
    return specs


@functools.lru_cache(maxsize=None)
def _sweep_case(index):
    s = sweep_specs()[index]
    x = np.full((s["N"], s["stride"]), np.nan, dtype=np.float32)      # (a gap that were read would come first)
    for p, (n, off, name) in enumerate(zip(s["n"], s["off"], s["classes"])):
        for i in range(s["N"]):
            x[i, off:off + n] = ALL_CLASSES[name](n, 100000 + 1000 * index + 10 * p + i)
    x.setflags(write=False)
    kind = s["thresh"]
    if kind is None:
        t = None
    elif kind[0] == "value":
        t = kind[1]
    else:
        used = np.concatenate([x[:, off:off + n].ravel() for n, off in zip(s["n"], s["off"])])
        t = threshold_points(used)[kind[1]]
    return x, t


def sweep_case(index):
    """(scores [N][stride] read-only, the threshold or None) of spec `index`."""
    return _sweep_case(int(index))


# ---- the kernel on the guarded arena ------------------------------------------------------------------------------------------
GARBAGE = 0x5A5A5A5A   # the second run's fill of outputs and workspace (the first run's is NaN)


def run_select(pkg, dev, scores, k, n=None, off=None, thresh=None, boxes=None, aligns=None, tag="", orders=None,
               with_vals=True, out_stride=None, boxes_stride=None):
    """select_topk on numpy operands on the guarded arena at each of `aligns` (default: both placements): a run into
    NaN-filled outputs and workspace, a second into garbage-filled ones, each compared exactly with the reference (ints
    equal, values and boxes bit for bit); the arena check proves that nothing beside the tensors changed.  The workspace
    is exactly what select_workspace_bytes reports.  with_vals=False goes through the C entry point itself with vals =
    NULL; the vals tensor carved alongside must then keep its fill.  out_stride > sum k: the outputs' rows are that
    wide, and the columns behind sum k keep both fills.  boxes_stride > the scores' stride: the boxes' rows are that
    long, NaN behind the scores' stride, where nothing may be read.  Returns (idx, vals, count, boxes) as numpy arrays,
    sum k columns wide."""
    import torch

    import guarded
    N, stride = scores.shape
    ks, ns, offs = _parts(stride, k, n, off)
    parts, ksum = len(ks), sum(ks)
    orders = full_orders(scores, ns, offs, thresh) if orders is None else orders
    want = expected(orders, scores, ks, offs, boxes)
    need = pkg.select_workspace_bytes(N, ns, ks)
    width = ksum if out_stride is None else int(out_stride)
    bstride = stride if boxes_stride is None else int(boxes_stride)
    assert width >= ksum and bstride >= stride
    if boxes is not None and bstride > stride:
        boxes_in = np.full((N, bstride, 4), np.nan, dtype=np.float32)
        boxes_in[:, :stride] = boxes
    else:
        boxes_in = boxes
    got = None
    for align in (guarded.ALIGNS if aligns is None else aligns):
        arena = guarded.Arena(torch, dev, align)
        sc_t = arena.input(torch.from_numpy(np.array(scores, dtype=np.float32)), name="scores")
        bx_t = None if boxes is None else arena.input(torch.from_numpy(boxes_in), name="boxes")
        idx = arena.output(N, width, name="idx").view(torch.int32)
        vals = arena.output(N, width, name="vals")
        count = arena.output(N, parts, name="count").view(torch.int32)
        ob = None if boxes is None else arena.output(N, width, 4, name="boxes_out")
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
                    0 if thresh is None else 1, 0.0 if thresh is None else float(thresh), p(idx), None, p(count), width,
                    p(bx_t), 0 if bx_t is None else bstride, p(ob), p(ws), 0 if ws is None else ws.numel() * 4, pkg._stream())
                pkg._check(rc, "wino_select_topk_hw")
            where = (f"select_topk {tag} N={N} n={ns} k={ks} off={offs} thresh={thresh} align={align} fill={fill:#x} "
                     f"out_stride={width} boxes_stride={bstride}")
            arena.check(where)
            full = (idx.cpu().numpy(), vals.cpu().numpy(), count.cpu().numpy(), None if ob is None else ob.cpu().numpy())
            for t in (full[0], full[1], full[3]):
                if t is not None:
                    assert (t[:, ksum:].view(np.int32) == np.int32(fill)).all(), f"{where}: written behind sum k"
            got = (full[0][:, :ksum], full[1][:, :ksum], full[2], None if ob is None else full[3][:, :ksum])
            assert np.array_equal(got[2], want[2]), (where, got[2].tolist(), want[2].tolist())
            assert np.array_equal(got[0], want[0]), (where, np.nonzero(got[0] != want[0]))
            if with_vals:
                assert np.array_equal(got[1].view(np.int32), want[1].view(np.int32)), where
            else:
                assert (got[1].view(np.int32) == np.int32(fill)).all(), f"{where}: vals = NULL was written"
            if ob is not None:
                assert np.array_equal(got[3].view(np.int32), want[3].view(np.int32)), where
    return got
