"""GPU tests of the segmented top-k / sort (wino_select_topk_hw) against the numpy reference of tests/select_cases.py,
which tests/test_select_host.py shows to be torch's stable descending sort.  Every comparison with the reference is
select_cases.run_select: on the guarded arena at both placements, into NaN-filled and then garbage-filled outputs and
workspace, idx / vals / count / boxes_out compared exactly (ints equal, values and boxes bit for bit), the workspace exactly
the size the query reports.  After the seeded classes come the constructed cases -- several long parts in one call, rows
wider than sum k and boxes with a stride of their own, candidate counts around k, the tie cut on every boundary, special
thresholds, the radix passes' corners -- and a seeded sweep of legal layouts.  The graph test carves its tensors from the
arena too.  Off the arena are only the calls that
let the wrapper allocate its own outputs, and the refusals, which launch nothing."""
import numpy as np
import pytest
import torch

import guarded
import select_cases as sc
from gpu_support import bits, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu
NAN = float("nan")
THRESHOLD_CLASSES = ("distinct", "ties", "extremes")


@pytest.mark.parametrize("n", sc.SIZES_N)
def test_select_is_exactly_the_reference(n, pkg, torch_dev):
    """Every case class at every k and N; the threshold cases (a value that occurs, and its two fp32 neighbours) of
    three classes likewise at every k and N.  n = 63 .. 65 and 1023 .. 1025 straddle a wave and a workgroup, 8192 / 8193 the one-launch sort and the
    radix select, 70001 has 35 chunks per segment with a ragged last one."""
    dev = torch_dev[1]
    for name in sorted(sc.CLASSES):
        for N in sc.IMAGES:
            x = sc.case(name, N, n)
            boxes = sc.boxes_for(x)
            orders = sc.full_orders(x, [n], [0])
            for k in sc.SIZES_K:
                sc.run_select(pkg, dev, x, k, boxes=boxes, tag=name, orders=orders)
    for name in THRESHOLD_CLASSES:
        for N in sc.IMAGES:
            x = sc.case(name, N, n)
            for t in sc.threshold_points(x):
                orders = sc.full_orders(x, [n], [0], t)
                for k in sc.SIZES_K:
                    _, _, count, _ = sc.run_select(pkg, dev, x, k, thresh=t, tag=f"{name} thresh", orders=orders)
                    with np.errstate(invalid="ignore"):
                        assert np.array_equal(count[:, 0], np.minimum((x >= np.float32(t)).sum(axis=1), k))


def test_select_many_small_segments(pkg, torch_dev):
    x = sc.case("ties", 300, 100, seed=2)
    sc.run_select(pkg, torch_dev[1], x, 17, boxes=sc.boxes_for(x), tag="300 segments")


def test_select_parts_in_the_rpn_slot_layout(pkg, torch_dev):
    """Five parts of unequal length at odd offsets (a segment starts 4-byte, not 16-byte aligned), one of them longer
    than 8192, one with k > n (padding rows in the middle of the row), one empty."""
    n, off, k = [9001, 300, 0, 77, 13], [1, 9003, 9400, 9401, 9479], [1000, 300, 5, 100, 13]
    for name in ("ties", "distinct"):
        x = sc.case(name, 3, 9500, seed=4)
        idx, vals, count, boxes = sc.run_select(pkg, torch_dev[1], x, k, n, off, boxes=sc.boxes_for(x), tag="parts")
        assert count.tolist() == [[1000, 300, 0, 77, 13]] * 3
        assert (idx[:, 1300:1305] == -1).all() and (idx[:, 1305 + 77:1405] == -1).all()
        assert (vals[:, 1305 + 77:1405] == 0).all() and (boxes[:, 1305 + 77:1405] == 0).all()
    for name in ("ties", "extremes"):          # with a threshold: fewer candidates than k in the long part too
        x = sc.case(name, 2, 9500, seed=5)
        t = sc.threshold_points(x)[1]
        sc.run_select(pkg, torch_dev[1], x, [8192, 300, 5, 100, 13], n, off, thresh=t, boxes=sc.boxes_for(x), tag="parts thresh")


def test_select_nan_segment_leaves_the_others_alone(pkg, torch_dev):
    n, off, k = [9000, 500], [0, 9000], [600, 500]
    x = sc.case("distinct", 4, 9500, seed=6)
    clean = sc.run_select(pkg, torch_dev[1], x, k, n, off, boxes=sc.boxes_for(x), aligns=(256,))
    for lo, hi, col0, col1 in ((0, 9000, 0, 600), (9000, 9500, 600, 1100)):        # image 1's long part, then its short one
        y = x.copy()
        y[1, lo:hi] = NAN
        got = sc.run_select(pkg, torch_dev[1], y, k, n, off, boxes=sc.boxes_for(y), tag="nan segment")
        assert (got[0][1, col0:col1] == np.arange(lo, lo + col1 - col0)).all()      # all NaN: index order
        mask = np.ones((4, 1100), dtype=bool)
        mask[1, col0:col1] = False
        for g, c in ((got[0], clean[0]), (got[1], clean[1]), (got[3], clean[3])):
            assert np.array_equal(g.view(np.int32)[mask], c.view(np.int32)[mask])
        assert np.array_equal(got[2], clean[2])


def test_select_large_segment_of_ties(pkg, torch_dev):
    """2^22 + 3 scores of seven values per image, k = 8192: 2049 workgroups per segment and pass, and the tie
    resolution discards millions of keys equal to the k-th."""
    n = (1 << 22) + 3
    x = sc.case("ties", 2, n, seed=8)
    idx, vals, count, _ = sc.run_select(pkg, torch_dev[1], x, 8192, tag="large")
    assert count.tolist() == [[8192]] * 2 and np.isnan(vals).all() and (np.diff(idx, axis=1) > 0).all()
    t = float(sc.TIE_VALUES[-1])
    sc.run_select(pkg, torch_dev[1], x, 8192, thresh=t, tag="large thresh")
    idx = sc.run_select(pkg, torch_dev[1], sc.case("zeros", 1, n), 8192, tag="large zeros")[0]
    assert np.array_equal(idx[0], np.arange(8192))


def test_select_without_vals_and_empty_inputs(pkg, torch_dev):
    """vals = NULL through the C entry point (a long part and a short one); rows of no scores and no images at all; and
    the wrapper's own allocation of its outputs, the one call here that cannot be on the arena."""
    _, dev = torch_dev
    x = sc.case("ties", 2, 9500, seed=9)
    sc.run_select(pkg, dev, x, [50, 60], [9000, 500], [0, 9000], boxes=sc.boxes_for(x), tag="no vals", with_vals=False)
    sc.run_select(pkg, dev, x, 50, thresh=sc.threshold_points(x)[1], tag="no vals, thresh", with_vals=False)
    idx, vals, count, _ = sc.run_select(pkg, dev, np.zeros((3, 0), dtype=np.float32), 4, tag="no scores")
    assert idx.tolist() == [[-1] * 4] * 3 and vals.tolist() == [[0.0] * 4] * 3 and count.tolist() == [[0]] * 3
    idx, _, count, _ = sc.run_select(pkg, dev, np.zeros((0, 9), dtype=np.float32), 4, tag="no images")
    assert idx.shape == (0, 4) and count.shape == (0, 1)
    y = sc.case("distinct", 2, 300, seed=9)
    idx, vals, count, boxes = pkg.select_topk(torch.from_numpy(y.copy()).to(dev), 7, boxes=torch.from_numpy(sc.boxes_for(y)).to(dev))
    torch.cuda.synchronize()
    for got, want in zip((idx, vals, count, boxes), sc.select_reference(y, 7, boxes=sc.boxes_for(y))):
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))


def test_select_replays_from_a_graph(pkg, torch_dev):
    """The seven launches of a long segment and the one launch of a short one, captured without a prepare on tensors
    carved from the guarded arena before the capture: two replays into NaN-filled buffers are bitwise the eager results
    and the reference's, and the arena is clean after each."""
    _, dev = torch_dev
    n, off, k = [20000, 700], [3, 20003], [1000, 800]
    x = sc.case("ties", 2, 20800, seed=10)
    want = sc.select_reference(x, k, n, off, boxes=sc.boxes_for(x))
    for align in guarded.ALIGNS:
        arena = guarded.Arena(torch, dev, align)
        xs = arena.input(torch.from_numpy(x.copy()), name="scores")
        bx = arena.input(torch.from_numpy(sc.boxes_for(x)), name="boxes")
        bufs = dict(idx=arena.output(2, 1800, name="idx").view(torch.int32), vals=arena.output(2, 1800, name="vals"),
                    count=arena.output(2, 2, name="count").view(torch.int32), boxes=arena.output(2, 1800, 4, name="boxes_out"),
                    ws=arena.workspace(pkg.select_workspace_bytes(2, n, k), name="workspace"))

        def run():
            pkg.select_topk(xs, k, n, off, None, bx, bufs["idx"], bufs["vals"], bufs["count"], bufs["boxes"], bufs["ws"])

        def poison():
            for t in bufs.values():
                t.view(torch.int32).fill_(guarded.NAN_BITS)

        poison()
        run()
        arena.check(f"eager align={align}")
        eager = {name: t.clone() for name, t in bufs.items() if name != "ws"}
        for name, w in zip(("idx", "vals", "count", "boxes"), want):
            assert np.array_equal(eager[name].cpu().numpy().view(np.int32), w.view(np.int32)), name
        sg = torch.cuda.Stream()
        sg.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=sg):
            run()
        for replay in range(2):
            poison()
            graph.replay()
            arena.check(f"replay {replay} align={align}")
            for name, t in eager.items():
                assert torch.equal(bits(bufs[name].view(torch.int32)), bits(t.view(torch.int32))), name
        del graph
    assert pkg.tickets_in_use() == 0


def test_select_refuses_with_device_pointers(pkg, torch_dev):
    """What only real tensors reach: the wrapper's operand checks, and the library's overlap, workspace and limit checks
    on device addresses; a refused call writes nothing."""
    _, dev = torch_dev
    z = lambda *s, **kw: torch.zeros(*s, device=dev, **kw)
    x = z(2, 9000)
    with pytest.raises(pkg.WinoError, match="out_idx must be a contiguous torch.int32"):
        pkg.select_topk(x, 5, out_idx=z(2, 5))
    with pytest.raises(pkg.WinoError, match="out_idx must be a contiguous torch.int32"):
        pkg.select_topk(x, 5, out_idx=z(2, 4, dtype=torch.int32))
    with pytest.raises(pkg.WinoError, match="same row length"):
        pkg.select_topk(x, 5, out_idx=z(2, 6, dtype=torch.int32))
    with pytest.raises(pkg.WinoError, match=r"boxes must be \[2\]\[stride\]\[4\]"):
        pkg.select_topk(x, 5, boxes=z(2, 9000, 3))
    with pytest.raises(pkg.WinoError, match="workspace too small"):
        pkg.select_topk(x, 5, workspace=z(10))
    with pytest.raises(pkg.WinoError, match="off has 1 entries for 2 parts"):
        pkg.select_topk(x, [5, 5], [10, 10], [0])
    idx = torch.full((2, 5), 9, dtype=torch.int32, device=dev)
    with pytest.raises(pkg.WinoError, match="unsupported shape"):
        pkg.select_topk(x, 8193, out_idx=torch.full((2, 8193), 9, dtype=torch.int32, device=dev))
    with pytest.raises(pkg.WinoError, match="rc=-2"):
        pkg.select_topk(x, 5, 9000, 1, out_idx=idx)
    with pytest.raises(pkg.WinoError, match="rc=-2"):
        pkg.select_topk(x, 5, boxes=z(2, 8999, 4), out_idx=idx)
    with pytest.raises(pkg.WinoError, match="rc=-3.*NaN"):
        pkg.select_topk(x, 5, score_thresh=NAN, out_idx=idx)
    with pytest.raises(pkg.WinoError, match="rc=-3.*overlap"):
        pkg.select_topk(x, 5, out_idx=idx, out_vals=x.view(-1)[:10].view(2, 5))             # vals inside the scores
    both = z(2, 5)
    with pytest.raises(pkg.WinoError, match="rc=-3.*overlap"):
        pkg.select_topk(x, 5, out_idx=both.view(torch.int32), out_vals=both)                # idx and vals the same memory
    need = pkg.select_workspace_bytes(2, 9000, 5)
    buf = z(18000 + need // 4)
    with pytest.raises(pkg.WinoError, match="rc=-3.*overlap"):
        pkg.select_topk(buf[:18000].view(2, 9000), 5, out_idx=idx, workspace=buf[17000:])   # workspace inside the scores
    torch.cuda.synchronize()
    assert bool((idx == 9).all()) and bool((x == 0).all())


# ---- constructed cases: several long parts, wider rows, counts around k, the tie cut, the radix passes' corners ---------------
LONG_PARTS = dict(n=[20481, 300, 8193, 0, 12294, 77], off=[3, 20491, 20801, 29001, 29011, 41311], k=[1000, 300, 8192, 5, 64, 100],
                  stride=41399)


def _permuted(layout, order):
    return {key: ([v[p] for p in order] if isinstance(v, list) else v) for key, v in layout.items()}


@pytest.mark.parametrize("layout", ["as_listed", "short_first", "overlapping"])
def test_select_several_long_parts(layout, pkg, torch_dev):
    """Six parts of every image, three of them longer than 8192 scores with 11, 5 and 7 chunks (the last ragged) -- lp,
    eq_off and cand_off are non-zero, and the two shorter long parts leave the grid's later chunks at once -- between
    short parts and an empty one, at odd offsets with gaps; the same parts with the short ones first and the long ones
    last; and with the second long part lying inside the first (the entry point lets parts overlap)."""
    L = dict(LONG_PARTS)
    if layout == "short_first":
        L = _permuted(L, [1, 3, 5, 2, 4, 0])
    elif layout == "overlapping":
        L["off"] = [3, 20491, 5001, 29001, 8001, 41311]        # 8193 from 5001 and 12294 from 8001: both inside the first
    assert sum(n > 8192 for n in L["n"]) == 3 and 0 in L["n"]
    for name in ("ties", "distinct"):
        x = sc.case(name, 3, L["stride"], seed=21)
        boxes = sc.boxes_for(x)
        for t in (None, sc.threshold_points(x)[1]):
            _, _, count, _ = sc.run_select(pkg, torch_dev[1], x, L["k"], L["n"], L["off"], thresh=t, boxes=boxes,
                                           tag=f"long parts {layout} {name}")
            if t is None:
                assert count.tolist() == [[min(k, n) for k, n in zip(L["k"], L["n"])]] * 3


@pytest.mark.parametrize("long_part", [False, True])
def test_select_wider_outputs_and_boxes(long_part, pkg, torch_dev):
    """out_stride > sum k: the columns behind sum k of idx, vals and boxes_out keep the NaN and the garbage fill.
    boxes_image_stride > image_stride: the box rows behind the scores' stride are NaN and never read; the payload names
    its row, so a box fetched with the scores' stride instead of the boxes' own shows in image 1 and 2."""
    n, off, k = ([9001, 300, 77], [1, 9003, 9400], [1000, 300, 100]) if long_part else ([700, 300, 77], [1, 703, 1100], [512, 300, 100])
    stride = off[-1] + n[-1] + 5
    for name, t in (("ties", None), ("distinct", None), ("ties", 0.25)):
        x = sc.case(name, 3, stride, seed=22)
        sc.run_select(pkg, torch_dev[1], x, k, n, off, thresh=t, boxes=sc.boxes_for(x), tag="wide", out_stride=sum(k) + 13,
                      boxes_stride=stride + 37)
    x = sc.case("ties", 2, stride, seed=23)
    sc.run_select(pkg, torch_dev[1], x, k, n, off, boxes=sc.boxes_for(x), tag="wide, no vals", with_vals=False,
                  out_stride=sum(k) + 4, boxes_stride=stride + 1)


@pytest.mark.parametrize("k,counts", [(64, (0, 1, 63, 64, 65)), (8192, (8191, 8192, 8193))])
def test_select_candidate_counts_around_k_in_a_long_segment(k, counts, pkg, torch_dev):
    """n = 10241 (six chunks, the last of one score) with exactly c scores at or above the threshold, at indices that
    include 0, 2047, 2048 and n - 1: c < k takes the segment down the `all` path (T = 0), c >= k through the radix
    select.  count = min(c, k) and the rows are exactly the reference's."""
    n, thresh = 10241, 0.5
    rng = np.random.RandomState(24)
    for c in counts:
        x = (rng.rand(2, n).astype(np.float32) * np.float32(0.4)).astype(np.float32)          # below the threshold
        for i in range(2):
            fixed = [0, 2047, 2048, n - 1][:c]
            rest = rng.permutation(np.setdiff1d(np.arange(n), fixed))[:c - len(fixed)]
            at = np.concatenate([fixed, rest]).astype(np.int64)
            x[i, at] = (0.5 + rng.rand(c) * 0.5).astype(np.float32)
            x[i, at[:c // 3]] = 0.5                                                          # some of them at equality
        assert ((x >= np.float32(thresh)).sum(axis=1) == c).all()
        _, _, count, _ = sc.run_select(pkg, torch_dev[1], x, k, thresh=thresh, boxes=sc.boxes_for(x), tag=f"{c} candidates")
        assert count.tolist() == [[min(c, k)]] * 2


TIE_CUT_NEED = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4096, 8191]


@pytest.mark.parametrize("front", [False, True], ids=["twos_behind", "twos_in_front"])
def test_select_tie_cut_on_every_boundary(front, pkg, torch_dev):
    """n = 10241 scores of 1.0 and `a` scores of 2.0, k = need + a: the gather takes the 2.0s and exactly the first
    `need` of the 1.0s in index order, so the cut `rank < need` falls behind element need - 1 of the equals -- on a lane,
    a wave (64), a round (256) and a chunk (2048) boundary and one to either side.  With the 2.0s behind the segment the
    j-th equal element has index j; with them in front, the ranks start from a shifted index."""
    n = 10241
    for a in (0, 1):
        x = np.ones((1, n), dtype=np.float32)
        if a:
            x[0, :a] = 2.0
        if not front:
            x = x[:, ::-1].copy()
        first_equal = a if front else 0
        for need in TIE_CUT_NEED:
            k = need + a
            if k > 8192:
                continue
            idx, vals, count, _ = sc.run_select(pkg, torch_dev[1], x, k, tag=f"tie cut need={need} a={a} front={front}")
            assert count.tolist() == [[k]]
            assert np.array_equal(idx[0, a:], np.arange(first_equal, first_equal + need))


def test_select_special_thresholds(pkg, torch_dev):
    """Thresholds of +-Inf, +-0, the smallest denormal of either sign and FLT_MAX on the class that holds all of them:
    count is numpy's (x >= t).sum(), so -0 admits +0 and +0 admits -0, and a denormal threshold is not flushed."""
    for n in (65, 8193):
        for N in (1, 2):
            x = sc.case("extremes", N, n, seed=25)
            for t in sc.SPECIAL_THRESHOLDS:
                orders = sc.full_orders(x, [n], [0], t)
                for k in (1, 64, 8192):
                    _, _, count, _ = sc.run_select(pkg, torch_dev[1], x, k, thresh=t, tag=f"thresh {t!r}", orders=orders)
                    assert np.array_equal(count[:, 0], np.minimum((x >= np.float32(t)).sum(axis=1), k)), (n, t, k)


RADIX_N = [8193, 20481, 70001]


@pytest.mark.parametrize("n", RADIX_N)
def test_select_bit_pattern_classes(n, pkg, torch_dev):
    """Uniform random bit patterns (NaNs of both signs and any payload, denormals) and keys that differ only in their
    low 10 or 21 bits (only pass 2, or passes 1 and 2, tell them apart; thousands of exact ties), positive and negative."""
    for name in sorted(sc.RADIX_CLASSES):
        for N in (1, 2):
            x = sc.case(name, N, n, seed=26)
            orders = sc.full_orders(x, [n], [0])
            for k in sc.SIZES_K:
                sc.run_select(pkg, torch_dev[1], x, k, boxes=sc.boxes_for(x) if k == 65 else None, tag=name, orders=orders,
                              aligns=(256,) if N == 1 else (16,))


@pytest.mark.parametrize("p", [0, 1, 2])
@pytest.mark.parametrize("n", RADIX_N)
def test_select_radix_corners(n, p, pkg, torch_dev):
    """find_digit driven to its corners in pass p: the k-th key's digit in the first and in the last bin a thread owns,
    in bin 0, in the histogram's last bin and in the highest occupied one, with a rank of 1 left in the bin and with the
    bin's whole count (tests/test_select_host.py shows that the constructed inputs do hit each of them).  N = 2 holds two
    draws of the case, N = 1 the first."""
    for k in sc.SIZES_K:
        for q, place, kind in sc.radix_corner_specs(k):
            if q != p:
                continue
            x = np.stack([sc.radix_corner(n, k, p, place, kind, seed) for seed in (0, 1)])
            tag = f"radix corner pass {p} {place} {kind}"
            sc.run_select(pkg, torch_dev[1], x, k, tag=tag, aligns=(16,))
            sc.run_select(pkg, torch_dev[1], x[:1], k, tag=tag, aligns=(256,))


@pytest.mark.parametrize("index", range(sc.SWEEP_COUNT))
def test_select_sweep(index, pkg, torch_dev):
    s = sc.sweep_specs()[index]
    x, t = sc.sweep_case(index)
    print(f"sweep {index}: {s} thresh={t!r}")
    sc.run_select(pkg, torch_dev[1], x, s["k"], s["n"], s["off"], thresh=t, boxes=sc.boxes_for(x) if s["boxes"] else None,
                  tag=f"sweep {index}", with_vals=s["with_vals"], out_stride=s["out_stride"],
                  boxes_stride=s["boxes_stride"] if s["boxes"] else None)
