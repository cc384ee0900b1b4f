"""Host tests of the segmented top-k / sort (no GPU): the numpy reference of tests/select_cases.py is torch's stable
descending sort truncated to k, for every case class; the constructed radix cases reach every corner of find_digit in
every pass and the layout sweep holds the layouts it is for (conditions on the GPU tests' inputs); the entry point and
the workspace query refuse every bad argument before any launch; the query is monotone and is what the entry point asks
for; select= rejects an unknown value."""
from ctypes import c_int, c_long

import numpy as np
import pytest
import torch

import select_cases as sc

SIZES = [1, 2, 7, 64, 65, 1000, 5000]
KS = [1, 2, 64, 1000, 8192]


@pytest.mark.parametrize("name", sorted(sc.ALL_CLASSES))
def test_reference_is_torchs_stable_descending_sort(name):
    for n in SIZES:
        x = sc.case(name, 2, n, seed=3)
        for row in x:
            want = torch.sort(torch.from_numpy(row.copy()), descending=True, stable=True).indices.numpy()
            for k in KS:
                got = sc.topk_order(row, k)
                assert np.array_equal(got, want[:k]), (name, n, k)


@pytest.mark.parametrize("name", sorted(sc.ALL_CLASSES))
def test_reference_is_torchs_topk_set_where_the_cut_is_clean(name):
    checked = 0
    for n in SIZES:
        row = sc.case(name, 1, n, seed=5)[0]
        key = np.sort(sc.orderable(row))[::-1]
        for k in KS:
            if k >= n or key[k - 1] == key[k]:     # the k-th and (k+1)-th values tie: torch's choice is its own
                continue
            want = torch.from_numpy(row.copy()).topk(k).indices.numpy()
            assert set(sc.topk_order(row, k).tolist()) == set(want.tolist()), (name, n, k)
            checked += 1
    assert checked or name in ("zeros", "nans")


def test_reference_threshold_is_greater_or_equal():
    for name in ("distinct", "ties", "extremes"):
        row = sc.case(name, 1, 1000, seed=7)[0]
        below, at, above = sc.threshold_points(row)
        assert (row == np.float32(at)).any()
        with np.errstate(invalid="ignore"):
            for t in (below, at, above):
                got = sc.topk_order(row, 8192, t)
                assert len(got) == int((row >= np.float32(t)).sum())
                assert not np.isnan(row[got]).any()
        equal = set(np.nonzero(row == np.float32(at))[0].tolist())      # >=, not >: in at the value, out just above it
        assert equal <= set(sc.topk_order(row, 8192, at).tolist()) and equal <= set(sc.topk_order(row, 8192, below).tolist())
        assert not equal & set(sc.topk_order(row, 8192, above).tolist())


def test_reference_layout_and_padding():
    x = sc.case("ties", 2, 40, seed=1)
    idx, vals, count, boxes = sc.select_reference(x, [3, 30, 4], [10, 20, 0], [0, 13, 40], boxes=sc.boxes_for(x))
    assert idx.shape == (2, 37) and count.tolist() == [[3, 20, 0]] * 2
    assert (idx[:, 23:33] == -1).all() and (vals[:, 23:33] == 0).all() and (boxes[:, 23:33] == 0).all()
    assert (idx[:, 33:] == -1).all()
    assert (idx[:, 3:23] >= 13).all() and (idx[:, 3:23] < 33).all()


# ---- the constructed radix cases and the sweep: conditions on the inputs --------------------------------------------------
def test_from_orderable_inverts_orderable():
    rng = np.random.RandomState(11)
    key = rng.randint(0x00800000, 0xff800000, size=20000, dtype=np.uint64).astype(np.uint32)
    key = key[key != np.uint32(0x7fffffff)]                       # (-0, which orderable maps to +0's key)
    assert np.array_equal(sc.orderable(sc.from_orderable(key)), key)
    for name, low_bits in (("narrow10", 10), ("narrow10_neg", 10), ("narrow21", 21), ("narrow21_neg", 21)):
        key = sc.orderable(sc.case(name, 1, 5000, seed=2)[0])
        assert len(set((key >> np.uint32(low_bits)).tolist())) == 1 and len(set(key.tolist())) > 900, name
        assert (sc.case(name, 1, 5000, seed=2)[0] < 0).all() == name.endswith("_neg")
    x = sc.case("bits", 1, 70001, seed=2)[0]
    b = x.view(np.uint32)
    assert np.isnan(x[b >> 31 == 0]).any() and np.isnan(x[b >> 31 == 1]).any()          # NaNs of both signs
    assert ((b & 0x7f800000) == 0).any()                                                # denormals (or zeros)


def test_radix_corner_cases_hit_every_corner_of_every_pass():
    """Every constructed case is what it says (its own pass, place and kind occur when the k-th key is looked for), and
    together the cases of every (n, k) the GPU test runs reach, in each of the three passes: the first and the last bin
    of a find_digit thread, the highest occupied bin, the histogram's last bin, bin 0 in passes 1 and 2, a rank of 1 and
    a rank equal to the bin's count."""
    want = {(p, c) for p in range(3) for c in ("first", "last", "highest", "top", "kr1", "krfull")} | {(1, "zero"), (2, "zero")}
    for n in (8193, 20481, 70001):
        for k in sc.SIZES_K:
            seen = set()
            specs = sc.radix_corner_specs(k)
            assert len(specs) >= 14
            for p, place, kind in specs:
                x = sc.radix_corner(n, k, p, place, kind, seed=1)
                assert x.shape == (n,) and x.dtype == np.float32
                hits = sc.radix_hits(x, k)
                need = {(p, place), (p, "kr1" if kind == "kr1" else "krfull")}
                if kind == "full_highest":
                    need.add((p, "highest"))
                assert need <= hits, (n, k, p, place, kind, sorted(hits))
                seen |= hits
                if n == 8193 and k in (2, 1000):                       # the reference on them is torch's sort as well
                    order = torch.sort(torch.from_numpy(x.copy()), descending=True, stable=True).indices.numpy()
                    assert np.array_equal(sc.topk_order(x, k), order[:k])
            assert want <= seen, (n, k, sorted(want - seen))


def test_sweep_specs_hold_the_layouts_they_are_for():
    specs = sc.sweep_specs()
    assert len(specs) == sc.SWEEP_COUNT == 40 and [s["index"] for s in specs] == list(range(40))
    longs = lambda s: [n > 8192 for n in s["n"]]
    assert sum(sum(longs(s)) >= 2 for s in specs) >= 5
    assert any(a and not b for s in specs for b, a in zip(longs(s), longs(s)[1:]))        # long after short
    assert any(b and not a for s in specs for b, a in zip(longs(s), longs(s)[1:]))        # short after long
    assert any(0 in s["n"] for s in specs) and any(k > n for s in specs for k, n in zip(s["k"], s["n"]))
    assert max(s["N"] * len(s["n"]) for s in specs) >= 24
    assert {s["N"] for s in specs} == {1, 2, 3, 4} and {len(s["n"]) for s in specs} >= {1, 2, 4, 8}
    assert {n for s in specs for n in s["n"]} >= {0, 1, 8192, 8193} and max(n for s in specs for n in s["n"]) > 20000
    starved = overlap = 0
    for s in specs:
        assert 1 <= len(s["n"]) <= 8 and all(1 <= k <= 8192 for k in s["k"]) and sum(s["k"]) <= 12000
        assert all(o >= 0 and o + n <= s["stride"] for o, n in zip(s["off"], s["n"]))
        assert s["out_stride"] >= sum(s["k"]) and s["boxes_stride"] >= s["stride"]
        ends = np.maximum.accumulate([o + n for o, n in zip(s["off"], s["n"])])
        overlap += any(o < e for o, e, n in zip(s["off"][1:], ends, s["n"][1:]) if n)
        x, t = sc.sweep_case(s["index"])
        assert x.shape == (s["N"], s["stride"]) and (t is None) == (s["thresh"] is None)
        if t is not None:
            with np.errstate(invalid="ignore"):
                starved += any(n > 8192 and ((x[:, o:o + n] >= np.float32(t)).sum(axis=1) < k).any()
                               for n, o, k in zip(s["n"], s["off"], s["k"]))
    assert starved >= 1 and overlap >= 2
    for key in ("boxes", "with_vals"):
        assert {s[key] for s in specs} == {True, False}
    assert any(s["thresh"] is None for s in specs) and {s["thresh"][0] for s in specs if s["thresh"]} == {"point", "value"}
    assert any(s["out_stride"] > sum(s["k"]) for s in specs) and any(s["boxes"] and s["boxes_stride"] > s["stride"] for s in specs)
    assert {c for s in specs for c in s["classes"]} == set(sc.ALL_CLASSES)


def test_sweep_workspaces_are_what_the_entry_point_asks_for(pkg):
    """For every spec of the sweep: one byte less than select_workspace_bytes is refused, the figure itself gets as far
    as the overlap check.  No launch."""
    for s in sc.sweep_specs():
        need = pkg.select_workspace_bytes(s["N"], s["n"], s["k"])
        assert (need > 0) == any(n > 8192 for n in s["n"])
        kw = dict(scores=0x40000000, N=s["N"], stride=s["stride"], off=tuple(s["off"]), n=tuple(s["n"]), k=tuple(s["k"]),
                  out_stride=s["out_stride"], idx=0x40000000)
        if need:
            assert _topk(pkg, ws=0x10000000, ws_bytes=need - 1, **kw) == ARG, s
            assert f"workspace too small: need {need} bytes" in pkg.lib().wino_last_error_string().decode()
        if max(s["n"]):                                  # (idx lies on the scores: with no score to read nothing would clash)
            assert _topk(pkg, ws=0x10000000 if need else None, ws_bytes=need, **kw) == ARG, s
            assert "must not overlap" in pkg.lib().wino_last_error_string().decode()


# ---- the C entry points' refusals ---------------------------------------------------------------------------------------
def _ints(v):
    return (c_int * len(v))(*v)


def _longs(v):
    return (c_long * len(v))(*v)


def _topk(pkg, scores=0x1000, N=2, stride=100, off=(0,), n=(100,), k=(10,), use_thresh=0, thresh=0.0, idx=0x100000,
          vals=0x200000, count=0x300000, out_stride=None, boxes_in=None, bstride=0, boxes_out=None, ws=None, ws_bytes=0):
    out_stride = sum(k) if out_stride is None else out_stride
    return pkg.lib().wino_select_topk_hw(scores, N, stride, len(k), _longs(off), _ints(n), _ints(k), use_thresh, thresh, idx,
                                         vals, count, out_stride, boxes_in, bstride, boxes_out, ws, ws_bytes, None)


def _bytes(pkg, N, n, k):
    """(0, bytes) from select_workspace_bytes, or (SHAPE, 0) where it refuses."""
    try:
        return 0, pkg.select_workspace_bytes(N, list(n), list(k))
    except pkg.WinoError as e:
        assert "select: unsupported shape" in str(e)
        return SHAPE, 0


SHAPE, ARG = -2, -3


def test_error_codes_are_the_headers(pkg):
    import re, os
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "winograd_mi355x.h")).read()
    assert int(re.search(r"WINO_E_SHAPE = (-\d+)", text).group(1)) == SHAPE
    assert int(re.search(r"WINO_E_ARG = (-\d+)", text).group(1)) == ARG


def test_select_refuses_bad_shapes_before_any_launch(pkg):
    bad = [dict(N=-1), dict(k=(0,)), dict(k=(8193,)), dict(n=(-1,)), dict(n=(101,)), dict(off=(1,)), dict(off=(-1,)),
           dict(stride=1 << 31, n=(5,)), dict(out_stride=9), dict(k=(5, 6), n=(10, 10), off=(0, 10), out_stride=10),
           dict(k=(1,) * 9, n=(1,) * 9, off=(0,) * 9), dict(N=65536),
           dict(boxes_in=0x400000, bstride=99, boxes_out=0x500000)]
    for kw in bad:
        assert _topk(pkg, **kw) == SHAPE, kw
        assert "select_topk: unsupported shape" in pkg.lib().wino_last_error_string().decode()
    assert pkg.lib().wino_select_topk_hw(0x1000, 2, 100, 0, _longs([0]), _ints([1]), _ints([1]), 0, 0.0, 0x100000, None,
                                         0x300000, 10, None, 0, None, None, 0, None) == SHAPE


def test_select_refuses_bad_arguments_before_any_launch(pkg):
    big = dict(stride=20000, n=(20000,), k=(100,))
    need = _bytes(pkg, 2, [20000], [100])[1]
    assert need > 0
    bad = [dict(scores=None), dict(idx=None), dict(count=None), dict(scores=0x1004), dict(idx=0x100008), dict(vals=0x200004),
           dict(count=0x300002), dict(boxes_in=0x400000, bstride=100, boxes_out=None),
           dict(boxes_in=0x400008, bstride=100, boxes_out=0x500000), dict(boxes_in=0x400000, bstride=100, boxes_out=0x500004),
           dict(use_thresh=1, thresh=float("nan")),
           dict(big, ws=None, ws_bytes=need), dict(big, ws=0x10000000, ws_bytes=need - 1), dict(big, ws=0x10000004, ws_bytes=need),
           dict(idx=0x1000), dict(vals=0x1000 + 96), dict(count=0x1000 + 4 * 196), dict(idx=0x200000 + 32),
           dict(count=0x100000 + 64), dict(boxes_in=0x400000, bstride=100, boxes_out=0x400000 + 1600),
           dict(boxes_in=0x400000, bstride=100, boxes_out=0x100000 - 16),
           dict(big, scores=0x20000000, ws=0x20000000 + 4096, ws_bytes=need),
           dict(big, scores=0x20000000, idx=0x10000000 + 16, ws=0x10000000, ws_bytes=need)]
    for kw in bad:
        assert _topk(pkg, **kw) == ARG, kw
    assert _topk(pkg, use_thresh=0, thresh=float("nan"), N=0) == 0          # (unused: not looked at)
    # nothing to do: no pointer is looked at, nothing is launched
    assert _topk(pkg, N=0, scores=None, idx=None, vals=None, count=None) == 0
    L = pkg.lib()
    assert L.wino_select_topk_hw(0x1000, 2, 100, 1, None, _ints([1]), _ints([1]), 0, 0.0, 0x100000, None, 0x300000, 10, None,
                                 0, None, None, 0, None) == ARG


def test_workspace_query_refuses_and_is_monotone(pkg):
    for N, n, k in [(-1, [5], [5]), (1, [-1], [5]), (1, [5], [0]), (1, [5], [8193]), (1, [], []), (1, [1] * 9, [1] * 9)]:
        assert _bytes(pkg, N, n, k)[0] == SHAPE, (N, n, k)
    assert _bytes(pkg, 0, [1 << 20], [8192]) == (0, 0)
    assert _bytes(pkg, 3, [8192, 100], [8192, 7]) == (0, 0)          # every segment sorts in one launch
    last = 0
    for n in [1, 8192, 8193, 10240, 10241, 70001, 1 << 22, (1 << 22) + 3, (1 << 31) - 1]:
        rc, b = _bytes(pkg, 2, [n], [1000])
        assert rc == 0 and b >= last and b % 16 == 0, (n, b, last)
        last = b
    assert last > 0
    last = 0
    for k in [1, 2, 64, 1000, 8191, 8192]:
        rc, b = _bytes(pkg, 2, [70001, 9000], [k, k])
        assert rc == 0 and b > last, (k, b, last)
        last = b
    assert _bytes(pkg, 4, [70001], [100])[1] > _bytes(pkg, 2, [70001], [100])[1]
    assert pkg.select_workspace_bytes(2, [70001, 9000], [8192, 8192]) == last
    assert pkg.select_workspace_bytes(2, 70001, 100) == _bytes(pkg, 2, [70001], [100])[1]
    with pytest.raises(pkg.WinoError, match="unsupported shape"):
        pkg.select_workspace_bytes(1, 5, 0)


def test_workspace_query_is_what_the_entry_point_asks_for(pkg):
    """The library refuses one byte less than select_workspace_bytes' answer and accepts exactly it: the refusal that
    then fires is the overlap check, which comes behind the workspace check."""
    for n, k in [([20000], [100]), ([8193, 70001, 5], [1, 8192, 5]), ([(1 << 22) + 3], [8192])]:
        need = pkg.select_workspace_bytes(2, n, k)
        kw = dict(scores=0x40000000, stride=sum(n), off=tuple(sum(n[:p]) for p in range(len(n))), n=tuple(n), k=tuple(k),
                  ws=0x10000000)
        assert _topk(pkg, ws_bytes=need - 1, **kw) == ARG
        assert f"workspace too small: need {need} bytes" in pkg.lib().wino_last_error_string().decode()
        assert _topk(pkg, ws_bytes=need, idx=0x40000000, **kw) == ARG
        assert "must not overlap" in pkg.lib().wino_last_error_string().decode()


def test_select_option_rejects_an_unknown_value(pkg):
    import importlib
    D = importlib.import_module("cuda_winograd_amd.detection")
    assert D.SELECTS == ("torch", "kernel")
    for bad in ("Kernel", "hip", None, 1):
        with pytest.raises(pkg.WinoError, match="select must be one of"):
            D.RPN.from_state_dict({}, select=bad)
        with pytest.raises(pkg.WinoError, match="select must be one of"):
            D.FasterRCNN.from_state_dict({}, "resnet18", select=bad)
        with pytest.raises(pkg.WinoError, match="select must be one of"):
            D.MaskRCNN.from_state_dict({}, "resnet18", select=bad)
        with pytest.raises(pkg.WinoError, match="select must be one of"):
            D.postprocess_detections(torch.zeros(4, 64), torch.zeros(4, 5), torch.zeros(2, 2), 3, select=bad)
    with pytest.raises(pkg.WinoError, match="no CPU path|must be a CUDA"):
        pkg.select_topk(torch.zeros(2, 8), 3)
