"""GPU tests of box decoding (wino_box_decode_hw) and batched NMS (wino_batched_nms_hw) against the fp64 references of
tests/box_cases.py: the decode at cases.TIGHT (tests/test_boxes_host.py shows that a straight fp32 restatement holds
TIGHT / 4), NMS exactly (the cases keep the generator's decision margins, and the fp32 walk makes the fp64 walk's
decisions).  Every run is on the guarded arena at both alignments, into NaN-filled outputs and a NaN-filled workspace,
twice, bitwise equal; int32 operands and outputs are views of arena storage."""
import numpy as np
import pytest
import torch

import box_cases as bc
import guarded
from cases import TIGHT
from gpu_support import bits, run_decode, run_nms, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu
NAN = float("nan")


# ---- decode ---------------------------------------------------------------------------------------------------------------
def check_decode(pkg, dev, c, tag, **kw):
    boxes, scores = run_decode(pkg, dev, c, tag=tag, **kw)
    err = bc.rel_err(boxes, c.reference())
    print(f"{tag}: N={c.N} rows/image={c.rpi} A={c.A} ld={c.ld}: {err:.2e}")
    assert err < TIGHT
    assert np.array_equal(scores.view(np.int32), c.scores().view(np.int32)), "the score column is copied bit for bit"


@pytest.mark.parametrize("index", range(len(bc.GRID_CASES)))
def test_decode_grid_mode(index, pkg, torch_dev):
    check_decode(pkg, torch_dev[1], bc.decode_case(index), f"grid {index}")


@pytest.mark.parametrize("index", range(len(bc.BOX_MODE_CASES)))
def test_decode_boxes_mode(index, pkg, torch_dev):
    check_decode(pkg, torch_dev[1], bc.decode_case(index, True), f"boxes {index}")


@pytest.mark.parametrize("index,mode", [(7, False), (5, False), (2, True)])
def test_decode_into_a_slice(index, mode, pkg, torch_dev):
    """A level's slice of an [N][total][4] / [N][total] buffer: offsets 37 and 0 with room behind."""
    c = bc.decode_case(index, mode)
    check_decode(pkg, torch_dev[1], c, "slice", offset=37, extra=11)
    check_decode(pkg, torch_dev[1], c, "slice", offset=0, extra=5)


@pytest.mark.parametrize("index,mode", [(7, False), (4, True)])
def test_decode_nonfinite_delta_stays_in_its_coordinates(index, mode, pkg, torch_dev):
    """A NaN delta gives NaN in the coordinates it feeds and nowhere else; +Inf / -Inf follow the fp64 reference (dw = +Inf
    takes the clamp); every other coordinate keeps the clean run's bits."""
    c = bc.decode_case(index, mode)
    clean, _ = run_decode(pkg, torch_dev[1], c, aligns=(256,))
    head = c.head.copy()
    rows, A = head.shape[0], c.A
    hit = np.zeros((rows, A, 4), dtype=bool)
    rng = np.random.RandomState(3)
    for n, value in enumerate([np.nan] * 8 + [np.inf] * 4 + [-np.inf] * 4):
        r, a, k = rng.randint(rows), rng.randint(A), n % 4
        head[r, c.delta_col + 4 * a + k] = value
        hit[r, a, [0, 2] if k % 2 == 0 else [1, 3]] = True
    got, scores = run_decode(pkg, torch_dev[1], c, head=head, tag="non-finite")
    want = c.reference(head)
    hit = hit.reshape(got.shape)
    assert int(np.isnan(want).sum()) >= 8 and not np.isnan(want[~hit]).any()
    assert bc.rel_err(got, want) < TIGHT                      # (NaNs in the same places)
    assert np.array_equal(got.view(np.int32)[~hit], clean.view(np.int32)[~hit])
    assert np.array_equal(scores.view(np.int32), c.scores().view(np.int32))


# ---- NMS ------------------------------------------------------------------------------------------------------------------
def check_nms(pkg, dev, c, use_groups, use_scores, max_out, aligns=guarded.ALIGNS):
    p = dict(c.PARAMS)
    if not use_scores:
        p.pop("score_thresh")
    want_keep, want_count, want_rois, _ = c.expected(use_groups, use_scores, max_out)
    m = max(c.R, 1) if max_out is None else max_out
    keep, count, rois = run_nms(pkg, dev, c.boxes, c.scores if use_scores else None, c.groups if use_groups else None, m,
                                p, aligns=aligns, tag=f"groups={use_groups} scores={use_scores}")
    assert np.array_equal(count, want_count), (c.R, c.S, max_out, count, want_count)
    assert np.array_equal(keep, want_keep), (c.R, c.S, max_out)
    assert np.array_equal(rois.view(np.int32), want_rois.view(np.int32)), (c.R, c.S, max_out)
    for s in range(c.S):
        assert (keep[s, count[s]:] == -1).all()


@pytest.mark.parametrize("R", bc.NMS_R)
def test_nms_is_exactly_the_reference(R, pkg, torch_dev):
    for S in bc.NMS_S:
        c = bc.nms_case(R, S)
        full = int(c.expected()[1][0])
        for max_out in (None, max(full // 2, 1), max(full, 1), full + 3):     # all, below, at and above segment 0's count
            check_nms(pkg, torch_dev[1], c, True, True, max_out)
        for use_groups, use_scores in bc.VARIANTS[1:]:
            check_nms(pkg, torch_dev[1], c, use_groups, use_scores, None, aligns=(16,))
        print(f"R={R} S={S}: kept {c.expected()[1].tolist()}")


@pytest.mark.parametrize("R", bc.NMS_WIDE_R)
def test_nms_wide_segments(R, pkg, torch_dev):
    """More than 64, 128 and 256 words per row: the scan kernel's three wider instantiations."""
    c = bc.nms_case(R, 1)
    for use_groups, use_scores in c.variants:
        check_nms(pkg, torch_dev[1], c, use_groups, use_scores, None, aligns=(256,))
    check_nms(pkg, torch_dev[1], c, True, True, int(c.expected()[1][0]) // 2, aligns=(16,))


def test_nms_case_classes(pkg, torch_dev):
    cc = bc.class_case()
    for use_groups in (True, False):
        for max_out in (cc.MAX_OUT, cc.R, 1):
            want_keep, want_count, want_rois, _ = cc.expected(use_groups, max_out)
            keep, count, rois = run_nms(pkg, torch_dev[1], cc.boxes, None, cc.groups if use_groups else None, max_out,
                                        cc.PARAMS, tag="classes")
            assert np.array_equal(keep, want_keep) and np.array_equal(count, want_count)
            assert np.array_equal(rois.view(np.int32), want_rois.view(np.int32))
    keep, count, _ = run_nms(pkg, torch_dev[1], cc.boxes, None, cc.groups, cc.MAX_OUT, cc.PARAMS, rois=False, aligns=(16,))
    assert np.array_equal(keep, cc.expected()[0])


def test_nms_nan_boxes_and_a_nan_segment(pkg, torch_dev):
    """A NaN coordinate or score takes its box out and changes nothing else's bits beyond what the reference says; a
    segment full of NaN boxes keeps nothing and leaves the other segments' outputs bitwise unchanged."""
    c = bc.nms_case(129, 5)
    p, m = c.PARAMS, 129
    clean = run_nms(pkg, torch_dev[1], c.boxes, c.scores, c.groups, m, p, aligns=(256,))
    boxes, scores = c.boxes.copy(), c.scores.copy()
    boxes[1, ::9, 2] = np.nan
    scores[3, 5::11] = np.nan
    want_keep, want_count, want_rois, _ = bc.batched_nms_reference(boxes, scores, c.groups, max_out=m, **p)
    keep, count, rois = run_nms(pkg, torch_dev[1], boxes, scores, c.groups, m, p, tag="nan boxes")
    assert np.array_equal(keep, want_keep) and np.array_equal(count, want_count)
    assert np.array_equal(rois.view(np.int32), want_rois.view(np.int32))
    assert not set(range(0, 129, 9)) & set(keep[1].tolist()) and not set(range(5, 129, 11)) & set(keep[3].tolist())
    boxes = c.boxes.copy()
    boxes[2] = np.nan
    keep, count, rois = run_nms(pkg, torch_dev[1], boxes, c.scores, c.groups, m, p, tag="nan segment")
    assert count[2] == 0 and (keep[2] == -1).all() and (rois[2, :, 0] == -1).all() and (rois[2, :, 1:] == 0).all()
    others = [0, 1, 3, 4]
    for got, ref in zip((keep, count, rois), clean):
        assert np.array_equal(got[others].view(np.int32), ref[others].view(np.int32))


def test_nms_without_boxes_or_segments(pkg, torch_dev):
    _, dev = torch_dev
    count = torch.full((3,), 7, dtype=torch.int32, device=dev)
    keep, got = pkg.batched_nms(torch.zeros(3, 0, 4, device=dev), count=count)
    torch.cuda.synchronize()
    assert got is count and count.tolist() == [0, 0, 0] and keep.tolist() == [[-1]] * 3
    keep, count, rois = pkg.batched_nms(torch.zeros(2, 0, 4, device=dev), max_out=3, rois_out=True)
    torch.cuda.synchronize()
    assert count.tolist() == [0, 0] and bool((keep == -1).all()) and tuple(keep.shape) == (2, 3)
    assert bool((rois[:, :, 0] == -1).all()) and bool((rois[:, :, 1:] == 0).all())       # padding rows: roi_align pools zeros
    keep, count, rois = pkg.batched_nms(torch.zeros(0, 9, 4, device=dev), max_out=4, rois_out=True)
    torch.cuda.synchronize()
    assert tuple(keep.shape) == (0, 4) and tuple(count.shape) == (0,) and tuple(rois.shape) == (0, 4, 5)
    boxes, scores = pkg.box_decode(torch.zeros(0, 64, device=dev), torch.zeros(0, 4, device=dev), torch.ones(2, 2, device=dev),
                                   3, score_col=0, delta_col=3)
    torch.cuda.synchronize()
    assert tuple(boxes.shape) == (2, 0, 4) and tuple(scores.shape) == (2, 0)


def test_wrappers_check_their_operands(pkg, torch_dev):
    _, dev = torch_dev
    z = lambda *s, **k: torch.zeros(*s, device=dev, **k)
    with pytest.raises(pkg.WinoError, match=r"groups must be a contiguous int32"):
        pkg.batched_nms(z(2, 8, 4), groups=z(2, 8))
    with pytest.raises(pkg.WinoError, match="workspace too small"):
        pkg.batched_nms(z(2, 65, 4), workspace=z(10))
    with pytest.raises(pkg.WinoError, match=r"keep must be a contiguous int32 CUDA\(HIP\) tensor of shape \(2, 8\)"):
        pkg.batched_nms(z(2, 8, 4), keep=z(2, 9, dtype=torch.int32))
    with pytest.raises(pkg.WinoError, match="anchors must have shape"):
        pkg.box_decode(z(15, 64), z(4, 4), z(1, 2), 3, grid=(3, 5, 8, 8))
    with pytest.raises(pkg.WinoError, match="grid 3x4"):
        pkg.box_decode(z(15, 64), z(3, 4), z(1, 2), 3, grid=(3, 4, 8, 8))
    with pytest.raises(pkg.WinoError, match=r"out_boxes must be \[1\]\[total >= 50\]"):
        pkg.box_decode(z(15, 64), z(3, 4), z(1, 2), 3, grid=(3, 5, 8, 8), out_boxes=z(1, 45, 4), out_offset=5)
    with pytest.raises(pkg.WinoError, match="rc=-2"):
        pkg.box_decode(z(15, 64), z(3, 4), z(1, 2), 3, grid=(3, 5, 8, 8), delta_col=60)


def test_decode_then_nms_replay_from_one_graph(pkg, torch_dev):
    """Neither call owns scratch: both go into one graph without a prepare, and two replays into NaN-filled buffers are
    bitwise the eager results.  The decoded boxes of each image are one NMS segment, classes as groups."""
    _, dev = torch_dev
    c = bc.decode_case(2, True)                      # 63 rows, 91 classes, N = 3
    S, R = c.N, c.rpi * c.A
    head, anc, hw = (torch.from_numpy(a).to(dev) for a in (c.head, c.anchors, c.image_hw))
    groups = (torch.arange(R, dtype=torch.int32, device=dev) % c.A).repeat(S, 1).contiguous()
    bufs = dict(boxes=torch.empty(S, R, 4, device=dev), scores=torch.empty(S, R, device=dev),
                keep=torch.empty(S, 40, dtype=torch.int32, device=dev), count=torch.empty(S, dtype=torch.int32, device=dev),
                rois=torch.empty(S, 40, 5, device=dev), ws=torch.empty(pkg.nms_workspace_bytes(S, R) // 4, device=dev))

    def run():
        pkg.box_decode(head, anc, hw, c.A, c.weights, None, c.delta_col, c.score_col, bufs["boxes"], bufs["scores"])
        pkg.batched_nms(bufs["boxes"], bufs["scores"], groups, 0.5, 1e-2, -0.5, 40, bufs["rois"], bufs["ws"], bufs["keep"],
                        bufs["count"])

    def poison():
        for k, t in bufs.items():
            (t.view(torch.float32) if t.dtype == torch.int32 else t).fill_(NAN)

    poison()
    run()
    torch.cuda.synchronize()
    eager = {k: t.clone() for k, t in bufs.items() if k != "ws"}
    assert int(eager["count"].min()) > 0
    sg = torch.cuda.Stream()
    sg.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=sg):
        run()
    for _ in range(2):
        poison()
        graph.replay()
        torch.cuda.synchronize()
        for k, t in eager.items():
            assert torch.equal(bits(bufs[k].view(torch.float32) if t.dtype == torch.int32 else bufs[k]),
                               bits(t.view(torch.float32) if t.dtype == torch.int32 else t)), k
    assert pkg.tickets_in_use() == 0
