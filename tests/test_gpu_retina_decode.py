"""GPU tests of RetinaNet's decode of the selected anchors (wino_retina_decode_hw): bit for bit box_decode in grid mode on
the whole level, gathered at idx // K, and against the fp64 decode reference of tests/box_cases.py at the bar
tests/test_gpu_boxes.py holds box_decode to (cases.TIGHT).  Every run is on the guarded arena at both alignments, twice,
bitwise equal; the regression map's ring and pad columns hold NaN."""
import numpy as np
import pytest
import torch

import box_cases as bc
import retina_cases as rc
from cases import TIGHT
from gpu_support import torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu


def _level_boxes(pkg, dev, c, deltas=None):
    """box_decode(grid=...) of the whole level on the interior rows: [N][h w A][4]."""
    head = torch.from_numpy(c.head_rows(deltas)).to(dev)
    boxes, _ = pkg.box_decode(head, torch.from_numpy(c.base).to(dev), torch.from_numpy(c.image_hw).to(dev), c.A, grid=c.grid)
    torch.cuda.synchronize()
    return boxes.cpu().numpy()


@pytest.mark.parametrize("K", rc.DECODE_K)
@pytest.mark.parametrize("A", rc.DECODE_A)
@pytest.mark.parametrize("h,w", rc.DECODE_HW)
def test_retina_decode_is_box_decode_at_the_selected_anchors(h, w, A, K, pkg, torch_dev):
    c = rc.decode_level(h, w, A, K)
    boxes, labels = rc.run_retina_decode(pkg, torch_dev[1], c, tag=f"{h}x{w} A={A} K={K}")
    want_boxes, want_labels = c.gather(_level_boxes(pkg, torch_dev[1], c))
    assert np.array_equal(labels, want_labels)
    assert np.array_equal(boxes.view(np.int32), want_boxes.view(np.int32)), "not box_decode's bits"
    ref = bc.decode_reference(c.head_rows(), c.base, c.image_hw, A, grid=c.grid, clamp=bc.CLIP)
    err = bc.rel_err(boxes, c.gather(ref)[0])
    print(f"{h}x{w} A={A} K={K}: count={c.count.tolist()} rel err {err:.2e}")
    assert err < TIGHT
    for i in range(c.N):                                           # rows past the count: a zero box and label -1
        assert (labels[i, c.count[i]:] == -1).all() and (boxes[i, c.count[i]:] == 0).all()
        assert (labels[i, :c.count[i]] >= 0).all()
    assert (c.count < c.rows).any()


def test_retina_decode_into_a_slice(pkg, torch_dev):
    c = rc.decode_level(13, 21, 9, 5)
    whole = rc.run_retina_decode(pkg, torch_dev[1], c, aligns=(256,))
    for offset, extra in ((37, 11), (0, 5), (1000, 0)):
        got = rc.run_retina_decode(pkg, torch_dev[1], c, offset=offset, extra=extra, tag="slice")
        assert np.array_equal(got[0].view(np.int32), whole[0].view(np.int32)) and np.array_equal(got[1], whole[1])


def test_retina_decode_nan_delta_stays_in_its_own_row(pkg, torch_dev):
    """A NaN delta reaches the rows that name its anchor, in the coordinates it feeds, and no other row: every other row
    keeps the clean run's bits."""
    c = rc.decode_level(7, 11, 9, 5)
    clean = rc.run_retina_decode(pkg, torch_dev[1], c, aligns=(256,))
    deltas = c.deltas.copy()
    hit = np.zeros((c.N, c.rows, 4), dtype=bool)
    for i in range(c.N):
        for j, coord in ((0, 0), (3, 1), (5, 2), (8, 3)):
            anchor = int(c.idx[i, j]) // c.K
            pixel, a = divmod(anchor, c.A)
            deltas[i, pixel // c.w, pixel % c.w, a, coord] = np.nan
            same = (c.idx[i] >= 0) & (c.idx[i] // c.K == anchor)
            hit[i, same, 0 if coord % 2 == 0 else 1] = True
            hit[i, same, 2 if coord % 2 == 0 else 3] = True
    boxes, labels = rc.run_retina_decode(pkg, torch_dev[1], c, deltas=deltas, tag="nan")
    assert np.isnan(boxes[hit]).all() and not np.isnan(boxes[~hit]).any()
    assert np.array_equal(boxes.view(np.int32)[~hit], clean[0].view(np.int32)[~hit]) and np.array_equal(labels, clean[1])
    want = c.gather(_level_boxes(pkg, torch_dev[1], c, deltas))[0]
    assert np.array_equal(boxes.view(np.int32), want.view(np.int32))


def test_retina_decode_refusals_and_empty_calls(pkg, torch_dev):
    _, dev = torch_dev
    c = rc.decode_level(3, 5, 9, 5)
    t = lambda a: torch.from_numpy(a).to(dev)
    idx, reg, base, hw = t(c.idx), t(c.reg_map()), t(c.base), t(c.image_hw)
    boxes = torch.full((c.N, c.rows, 4), 9.0, device=dev)
    labels = torch.full((c.N, c.rows), 9, dtype=torch.int32, device=dev)
    with pytest.raises(pkg.WinoError, match="idx must be a contiguous int32"):
        pkg.retina_decode(idx.float(), reg, base, hw, c.grid, c.K)
    with pytest.raises(pkg.WinoError, match="reg_map must be"):
        pkg.retina_decode(idx, reg, base, hw, (4, 5, 8, 8), c.K)
    with pytest.raises(pkg.WinoError, match="rows 30 .. 67 of 37"):
        pkg.retina_decode(idx, reg, base, hw, c.grid, c.K, out_boxes=boxes, out_labels=labels, out_offset=30, k=37)
    with pytest.raises(pkg.WinoError, match="rc=-2"):
        pkg.retina_decode(idx, reg, base, hw, c.grid, 0, out_boxes=boxes, out_labels=labels)
    with pytest.raises(pkg.WinoError, match="rc=-2"):                                     # 4 A > ld_r
        pkg.retina_decode(idx, reg[..., :32].contiguous(), base, hw, c.grid, c.K, out_boxes=boxes, out_labels=labels)
    with pytest.raises(pkg.WinoError, match="rc=-3.*overlap"):
        pkg.retina_decode(idx, reg, base, hw, c.grid, c.K, out_boxes=boxes, out_labels=idx)
    pkg.retina_decode(idx, reg, base, hw, c.grid, c.K, k=0, out_boxes=boxes, out_labels=labels)   # nothing to do
    torch.cuda.synchronize()
    assert bool((boxes == 9).all()) and bool((labels == 9).all())
    # an index past the level is a padding row, not an address
    bad = idx.clone()
    bad[:, 0] = c.h * c.w * c.A * c.K
    b, l = pkg.retina_decode(bad, reg, base, hw, c.grid, c.K)
    torch.cuda.synchronize()
    assert bool((l[:, 0] == -1).all()) and bool((b[:, 0] == 0).all()) and bool((l[0, 1:c.count[0]] >= 0).all())
