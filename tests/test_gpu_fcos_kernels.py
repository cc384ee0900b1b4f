"""GPU tests of FCOS's score-map kernel (wino_fcos_score_map_hw) and decode kernel (wino_fcos_decode_hw).  The score map
against the fp64 formula at cases.TIGHT with rings and pad columns untouched; the decode bit for bit against the torch-CPU
fp32 transcription of tests/fcos_cases.py and at TIGHT against fp64.  Every run is on the guarded arena at both placements,
twice, bitwise equal.  One more test holds retina_decode, whose rows the decode shares, to box_decode's bits."""
import numpy as np
import pytest
import torch

import box_cases as bc
import fcos_cases as fc
import retina_cases as rc
from cases import TIGHT
from gpu_support import torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("K", fc.SCORE_K)
@pytest.mark.parametrize("h,w", fc.SCORE_HW)
def test_score_map_against_fp64(h, w, K, pkg, torch_dev):
    c = fc.score_level(h, w, K)
    got = fc.run_score_map(pkg, torch_dev[1], c, tag=f"{h}x{w} K={K}")
    want = fc.score_reference(c.logits, c.ctr)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{h}x{w} K={K}: rel err {err:.2e}")
    assert np.isfinite(got).all() and err < TIGHT


def test_score_map_nan_and_extremes(pkg, torch_dev):
    """A NaN logit poisons its own score, a NaN centerness its own pixel, and nothing else changes a bit; a logit so low
    that the product underflows gives 0, one so high gives sqrt(sigmoid(ctr))."""
    c = fc.score_level(7, 11, 5)
    clean = fc.run_score_map(pkg, torch_dev[1], c, aligns=(256,))
    logits, ctr = c.logits.copy(), c.ctr.copy()
    logits[0, 2, 3, 4] = np.nan
    ctr[1, 6, 10] = np.nan
    logits[1, 0, 0, 0], logits[1, 0, 0, 1] = -200.0, 200.0
    got = fc.run_score_map(pkg, torch_dev[1], c, logits, ctr, tag="nan")
    hit = np.zeros(got.shape, dtype=bool)
    hit[0, 2, 3, 4] = True
    hit[1, 6, 10, :] = True
    assert np.isnan(got[hit]).all() and not np.isnan(got[~hit]).any()
    hit[1, 0, 0, :2] = True
    assert np.array_equal(got.view(np.int32)[~hit], clean.view(np.int32)[~hit])
    assert got[1, 0, 0, 0] == 0.0
    want = float(fc.score_reference(logits[1:2, 0, 0, 1:2], ctr[1:2, 0, 0])[0, 0])
    assert abs(got[1, 0, 0, 1] - want) < TIGHT


def test_score_map_refusals(pkg, torch_dev):
    _, dev = torch_dev
    c = fc.score_level(3, 5, 5)
    cls, reg = torch.from_numpy(c.cls_map()).to(dev), torch.from_numpy(c.reg_map()).to(dev)
    before = cls.clone()
    L, p = pkg.lib(), lambda t: t.data_ptr()
    call = lambda cp, rp, *a: L.wino_fcos_score_map_hw(cp, rp, *a, pkg._stream())
    ok = (c.N, c.h, c.w, c.K, c.ld_c, c.ld_r, fc.CTR_COL)
    for bad in ((-1, 3, 5, 5, 64, 64, 4), (2, 0, 5, 5, 64, 64, 4), (2, 3, 0, 5, 64, 64, 4), (2, 3, 5, 0, 64, 64, 4),
                (2, 3, 5, 65, 64, 64, 4), (2, 3, 5, 5, 62, 64, 4), (2, 3, 5, 5, 64, 64, 64), (2, 3, 5, 5, 64, 64, -1),
                (2, 3, (1 << 26) - 2, 5, 64, 64, 4)):
        assert call(p(cls), p(reg), *bad) == -2, bad
    assert call(0, 0, 0, 3, 5, 5, 64, 64, 4) == 0
    assert call(0, p(reg), *ok) == -3 and call(p(cls), 0, *ok) == -3
    assert call(p(cls) + 4, p(reg), *ok) == -3 and call(p(cls), p(reg) + 8, *ok) == -3
    assert call(p(cls), p(cls), *ok) == -3
    torch.cuda.synchronize()
    assert torch.equal(cls.view(torch.int32), before.view(torch.int32))
    with pytest.raises(pkg.WinoError, match="one level"):
        pkg.fcos_score_map(cls, reg[:, :-1].contiguous(), c.K)


@pytest.mark.parametrize("K", rc.DECODE_K)
@pytest.mark.parametrize("A", rc.DECODE_A)
@pytest.mark.parametrize("h,w", rc.DECODE_HW)
def test_fcos_decode_is_the_coder_in_fp32(h, w, A, K, pkg, torch_dev):
    c = rc.decode_level(h, w, A, K)
    boxes, labels = fc.run_fcos_decode(pkg, torch_dev[1], c, tag=f"{h}x{w} A={A} K={K}")
    want_boxes, want_labels = c.gather(fc.decode_fp32(c))
    assert np.array_equal(labels, want_labels)
    assert np.array_equal(boxes.view(np.int32), want_boxes.view(np.int32)), "not the fp32 transcription's bits"
    err = bc.rel_err(boxes, c.gather(fc.decode_fp64(c))[0])
    print(f"{h}x{w} A={A} K={K}: count={c.count.tolist()} rel err {err:.2e}")
    assert err < TIGHT
    for i in range(c.N):                                           # rows past the count: a zero box and label -1
        assert (labels[i, c.count[i]:] == -1).all() and (boxes[i, c.count[i]:] == 0).all()
        assert (labels[i, :c.count[i]] >= 0).all()
    assert (c.count < c.rows).any()
    assert (c.deltas < 0).any()                                    # the ReLU has something to do


def test_fcos_decode_into_a_slice(pkg, torch_dev):
    c = rc.decode_level(13, 21, 1, 5)
    whole = fc.run_fcos_decode(pkg, torch_dev[1], c, aligns=(256,))
    for offset, extra in ((37, 11), (0, 5), (1000, 0)):
        got = fc.run_fcos_decode(pkg, torch_dev[1], c, offset=offset, extra=extra, tag="slice")
        assert np.array_equal(got[0].view(np.int32), whole[0].view(np.int32)) and np.array_equal(got[1], whole[1])


def test_fcos_decode_nan_delta_stays_in_its_own_row(pkg, torch_dev):
    c = rc.decode_level(7, 11, 1, 5)
    clean = fc.run_fcos_decode(pkg, torch_dev[1], c, aligns=(256,))
    deltas = c.deltas.copy()
    hit = np.zeros((c.N, c.rows, 4), dtype=bool)
    for i in range(c.N):
        for j, coord in ((0, 0), (3, 1), (5, 2), (8, 3)):
            anchor = int(c.idx[i, j]) // c.K
            pixel, a = divmod(anchor, c.A)
            deltas[i, pixel // c.w, pixel % c.w, a, coord] = np.nan
            hit[i, (c.idx[i] >= 0) & (c.idx[i] // c.K == anchor), coord] = True     # a column feeds one coordinate
    boxes, labels = fc.run_fcos_decode(pkg, torch_dev[1], c, deltas=deltas, tag="nan")
    assert np.isnan(boxes[hit]).all() and not np.isnan(boxes[~hit]).any()
    assert np.array_equal(boxes.view(np.int32)[~hit], clean[0].view(np.int32)[~hit]) and np.array_equal(labels, clean[1])


def test_fcos_decode_refusals_and_padding_rows(pkg, torch_dev):
    _, dev = torch_dev
    c = rc.decode_level(3, 5, 1, 5)
    t = lambda a: torch.from_numpy(a).to(dev)
    idx, reg, base, hw = t(c.idx), t(c.reg_map()), t(c.base), t(c.image_hw)
    boxes = torch.full((c.N, c.rows, 4), 9.0, device=dev)
    labels = torch.full((c.N, c.rows), 9, dtype=torch.int32, device=dev)
    with pytest.raises(pkg.WinoError, match="idx must be a contiguous int32"):
        pkg.fcos_decode(idx.float(), reg, base, hw, c.grid, c.K)
    with pytest.raises(pkg.WinoError, match="reg_map must be"):
        pkg.fcos_decode(idx, reg, base, hw, (4, 5, 8, 8), c.K)
    with pytest.raises(pkg.WinoError, match="rows 30 .. 67 of 37"):
        pkg.fcos_decode(idx, reg, base, hw, c.grid, c.K, out_boxes=boxes, out_labels=labels, out_offset=30, k=37)
    with pytest.raises(pkg.WinoError, match="rc=-2"):
        pkg.fcos_decode(idx, reg, base, hw, c.grid, 0, out_boxes=boxes, out_labels=labels)
    with pytest.raises(pkg.WinoError, match="rc=-2"):                                     # 4 A > ld_r
        pkg.fcos_decode(idx, reg[..., :2].contiguous(), base, hw, c.grid, c.K, out_boxes=boxes, out_labels=labels)
    with pytest.raises(pkg.WinoError, match="rc=-3.*overlap"):
        pkg.fcos_decode(idx, reg, base, hw, c.grid, c.K, out_boxes=boxes, out_labels=idx)
    pkg.fcos_decode(idx, reg, base, hw, c.grid, c.K, k=0, out_boxes=boxes, out_labels=labels)   # nothing to do
    torch.cuda.synchronize()
    assert bool((boxes == 9).all()) and bool((labels == 9).all())
    bad = idx.clone()
    bad[:, 0] = c.h * c.w * c.A * c.K                              # an index past the level is a padding row, not an address
    b, l = pkg.fcos_decode(bad, reg, base, hw, c.grid, c.K)
    torch.cuda.synchronize()
    assert bool((l[:, 0] == -1).all()) and bool((b[:, 0] == 0).all()) and bool((l[0, 1:c.count[0]] >= 0).all())


@pytest.mark.parametrize("h,w,A,K", [(7, 11, 9, 5), (13, 21, 1, 91), (1, 1, 9, 1)])
def test_retina_decode_keeps_box_decode_bits(h, w, A, K, pkg, torch_dev):
    """retina_decode now takes its rows from the header the FCOS decode shares: still box_decode in grid mode, bit for bit."""
    c = rc.decode_level(h, w, A, K)
    boxes, labels = rc.run_retina_decode(pkg, torch_dev[1], c, tag=f"{h}x{w} A={A} K={K}")
    head = torch.from_numpy(c.head_rows()).to(torch_dev[1])
    level, _ = pkg.box_decode(head, torch.from_numpy(c.base).to(torch_dev[1]), torch.from_numpy(c.image_hw).to(torch_dev[1]),
                              c.A, grid=c.grid)
    torch.cuda.synchronize()
    want_boxes, want_labels = c.gather(level.cpu().numpy())
    assert np.array_equal(labels, want_labels) and np.array_equal(boxes.view(np.int32), want_boxes.view(np.int32))
