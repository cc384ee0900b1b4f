"""GPU tests of the segmented top-k on a padded NHWC map (wino_select_topk_map_hw) against the numpy reference of
tests/select_cases.py applied to the flat gather of the real elements.  Every comparison is retina_cases.run_select_map:
on the guarded arena at both placements, into NaN-filled and then garbage-filled outputs and workspace, idx / vals /
count compared exactly.  The ring and the pad columns of every map hold NaN and +Inf, the greatest keys of the order: a
single stray read of them lands in the output."""
import numpy as np
import pytest
import torch

import guarded
import retina_cases as rc
import select_cases as sc
from gpu_support import bits, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu


def _ks(n):
    return sorted({min(k, n) for k in rc.MAP_K})


@pytest.mark.parametrize("cols,ld", rc.MAP_COLS)
@pytest.mark.parametrize("h,w", rc.MAP_HW)
def test_select_map_is_exactly_the_reference(h, w, cols, ld, pkg, torch_dev):
    """Every level size x (cols, ld) x N x k, for the classes all distinct, ties across the cut, all equal and all NaN,
    and for ties with a threshold that leaves fewer than k candidates (a seventh of the scores reach it).  n = h w cols
    runs from 1 to 223587: both sides of 8192, the one-launch sort and the radix select."""
    n = h * w * cols
    for N in rc.MAP_IMAGES:
        for name in rc.MAP_CLASSES:
            flat = sc.case(name, N, n, seed=40)
            rc.run_select_map(pkg, torch_dev[1], flat, h, w, cols, ld, _ks(n), tag=name,
                              aligns=guarded.ALIGNS if name == "ties" else (16,))
        flat = sc.case("ties", N, n, seed=41)
        t = float(sc.TIE_VALUES[-1])
        got = rc.run_select_map(pkg, torch_dev[1], flat, h, w, cols, ld, _ks(n), thresh=t, tag="ties thresh", aligns=(256,))
        with np.errstate(invalid="ignore"):
            cands = (flat >= np.float32(t)).sum(axis=1)
        for k, (_, _, count) in got.items():
            assert np.array_equal(count, np.minimum(cands, k))


@pytest.mark.parametrize("n", rc.CHUNK_N)
def test_select_map_chunk_edges(n, pkg, torch_dev):
    """One pixel of cols = n scores, ld rounded up: n = 2048 m - 1, 2048 m, 2048 m + 1 -- a radix pass's last chunk full,
    one short of full and one score long -- on both sides of 8192."""
    ld = rc.pad64(n)
    for N in rc.MAP_IMAGES:
        for name in ("ties", "distinct"):
            flat = sc.case(name, N, n, seed=42)
            rc.run_select_map(pkg, torch_dev[1], flat, 1, 1, n, ld, _ks(n), tag=f"chunk {name}", aligns=(256,) if N == 1 else (16,))
        flat = sc.case("ties", N, n, seed=43)
        rc.run_select_map(pkg, torch_dev[1], flat, 1, 1, n, ld, _ks(n), thresh=sc.threshold_points(flat)[1], tag="chunk thresh",
                          aligns=(16,))


def test_select_map_row_and_pixel_edges(pkg, torch_dev):
    """The k best scores are exactly the last column of every pixel, then the first: an address that slips by one column,
    one pixel or one row reads a neighbour (or the poison) instead."""
    h, w, cols, ld = 7, 11, 45, 64
    flat = np.zeros((2, h, w, cols), dtype=np.float32)
    flat[:, :, :, cols - 1] = 2.0 + np.arange(h * w, dtype=np.float32).reshape(h, w)
    flat[:, :, :, 0] = 1.0
    flat = flat.reshape(2, -1)
    got = rc.run_select_map(pkg, torch_dev[1], flat, h, w, cols, ld, [h * w, 2 * h * w], tag="edges")
    idx = got[2 * h * w][0]
    assert np.array_equal(idx[0, :h * w], (np.arange(h * w)[::-1] * cols + cols - 1))
    assert np.array_equal(idx[0, h * w:], np.arange(h * w) * cols)


@pytest.mark.parametrize("index", range(rc.MAP_SWEEP_COUNT))
def test_select_map_sweep(index, pkg, torch_dev):
    s = rc.map_sweep_specs()[index]
    flat, t = rc.map_sweep_case(index)
    print(f"sweep {index}: {s} thresh={t!r}")
    rc.run_select_map(pkg, torch_dev[1], flat, s["h"], s["w"], s["cols"], s["ld"], [s["k"]], thresh=t, tag=f"sweep {index}",
                      out_offset=s["off"], extra=s["extra"])


def test_select_map_replays_from_a_graph(pkg, torch_dev):
    """A long level (seven launches) and a short one (one launch) into two slices of one buffer, captured without a
    prepare on tensors carved from the guarded arena: two replays into NaN-filled buffers are bitwise the eager results
    and the reference's."""
    _, dev = torch_dev
    levels = [(13, 21, 45, 64, 1000), (3, 5, 45, 64, 675)]
    flats = [sc.case("ties", 2, h * w * cols, seed=44 + l) for l, (h, w, cols, _, _) in enumerate(levels)]
    arena = guarded.Arena(torch, dev, 16)
    maps = [arena.input(torch.from_numpy(rc.poisoned_map(f, h, w, cols, ld)), name=f"map{l}")
            for l, (f, (h, w, cols, ld, _)) in enumerate(zip(flats, levels))]
    K = sum(k for *_, k in levels)
    idx, vals = arena.output(2, K, name="idx").view(torch.int32), arena.output(2, K, name="vals")
    counts = [arena.output(2, name=f"count{l}").view(torch.int32) for l in range(2)]
    wss = [arena.workspace(max(pkg.select_map_workspace_bytes(2, h, w, cols, k), 16), name=f"ws{l}")
           for l, (h, w, cols, _, k) in enumerate(levels)]

    def run():
        off = 0
        for m, (h, w, cols, ld, k), c, ws in zip(maps, levels, counts, wss):
            pkg.select_topk_map(m, cols, k, None, idx, vals, c, off, ws)
            off += k

    def poison():
        for t in (idx, vals, *counts, *wss):
            t.view(torch.int32).fill_(guarded.NAN_BITS)

    poison()
    run()
    arena.check("eager")
    eager = [t.clone() for t in (idx, vals, *counts)]
    off = 0
    for f, (h, w, cols, ld, k), c in zip(flats, levels, counts):
        want = sc.select_reference(f, k)
        assert np.array_equal(idx[:, off:off + k].cpu().numpy(), want[0])
        assert np.array_equal(vals[:, off:off + k].cpu().numpy().view(np.int32), want[1].view(np.int32))
        assert np.array_equal(c.cpu().numpy(), want[2][:, 0])
        off += k
    sg = torch.cuda.Stream()
    sg.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=sg):
        run()
    for replay in range(2):
        poison()
        graph.replay()
        arena.check(f"replay {replay}")
        for t, e in zip((idx, vals, *counts), eager):
            assert torch.equal(bits(t.view(torch.int32)), bits(e.view(torch.int32)))
    del graph
    assert pkg.tickets_in_use() == 0


def test_select_map_refuses_with_device_pointers(pkg, torch_dev):
    """The wrapper's operand checks and the library's overlap, slice and workspace checks; a refused call writes nothing."""
    _, dev = torch_dev
    m = torch.zeros((2, 15, 23, 64), device=dev)
    idx = torch.full((2, 50), 9, dtype=torch.int32, device=dev)
    vals = torch.full((2, 50), 9.0, device=dev)
    with pytest.raises(pkg.WinoError, match="cols=65 of ld=64"):
        pkg.select_topk_map(m, 65, 5)
    with pytest.raises(pkg.WinoError, match="out_offset=3 needs out_idx"):
        pkg.select_topk_map(m, 45, 5, out_offset=3)
    with pytest.raises(pkg.WinoError, match=r"out_idx must be a contiguous torch.int32 CUDA\(HIP\) tensor \[2\]\[>= 51\]"):
        pkg.select_topk_map(m, 45, 5, out_idx=idx, out_vals=vals, out_offset=46)
    with pytest.raises(pkg.WinoError, match="unsupported shape"):
        pkg.select_topk_map(m, 45, 8193)
    with pytest.raises(pkg.WinoError, match="workspace too small"):
        pkg.select_topk_map(m, 45, 5, workspace=torch.zeros(10, device=dev))
    with pytest.raises(pkg.WinoError, match="rc=-3.*NaN"):
        pkg.select_topk_map(m, 45, 5, float("nan"), idx, vals)
    with pytest.raises(pkg.WinoError, match="rc=-3.*overlap"):
        pkg.select_topk_map(m, 45, 5, None, idx, m.view(-1)[:100].view(2, 50))             # vals inside the map
    torch.cuda.synchronize()
    assert bool((idx == 9).all()) and bool((vals == 9).all()) and bool((m == 0).all())
