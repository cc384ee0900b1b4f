"""GPU tests of the detectors' select="kernel" path (select_topk in RPN.forward and postprocess_detections) on the
seeded detector of box_cases.DETECTOR (resnet18, N = 2, 64 x 96): against select="torch", the code that was there before,
bit for bit wherever torch defines the order (tests/test_gpu_faster_rcnn.py's margins show that the logits there are
distinct; the zero scores of padding candidates tie, and torch's order among them is its own); from one graph; with a NaN
pixel; through Mask R-CNN; and on an RPN whose logits tie exactly, against the reference order of tests/select_cases.py."""
import importlib

import numpy as np
import pytest
import torch

import box_cases as bc
import roi_cases as rc
import select_cases as sc
from gpu_support import R, same_bits, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu
D = bc.DETECTOR
DET_KEYS = ("boxes", "scores", "labels", "count", "overflow")
RPN_STAGES = ("topk_idx", "sorted_boxes", "sorted_logits", "sorted_levels")
MASK_P = 14


def kwargs(dev, **more):
    return dict(num_classes=D["classes"], out_channels=D["out_channels"], P=D["P"], rpn_pre_nms_top_n=D["pre"],
                rpn_post_nms_top_n=D["post"], box_detections_per_img=D["detections"], device=dev, **more)


@pytest.fixture(scope="module")
def pair(pkg, R, torch_dev):
    sd, _, _ = bc.detector_state_dict(R)
    return (pkg.FasterRCNN.from_state_dict(sd, D["arch"], **kwargs(torch_dev[1])),
            pkg.FasterRCNN.from_state_dict(sd, D["arch"], **kwargs(torch_dev[1], select="kernel")), sd)


def test_faster_rcnn_kernel_select_is_the_torch_path(pair, torch_dev):
    ref, ker, _ = pair
    x = bc.detector_input().to(torch_dev[1])
    want, got = ref(x, stages=True), ker(x, stages=True)
    torch.cuda.synchronize()
    assert set(got) == set(want)
    for k in DET_KEYS + RPN_STAGES + ("rois", "proposal_scores", "rpn_keep", "rpn_count", "sorted_scores", "cand_scores",
                                      "det_keep"):
        assert same_bits(got[k], want[k]), k
    live = want["cand_scores"] != 0          # padding candidates score exactly 0 and tie: torch's order among them is its own
    assert int(live.sum()) > 0
    for k in ("cand_idx", "cand_labels", "cand_boxes"):
        assert same_bits(got[k][live], want[k][live]), k
    assert int(want["count"].min()) > 0


def test_kernel_select_replays_from_one_graph_and_keeps_a_nan_in_its_image(pkg, pair, torch_dev):
    _, m, _ = pair
    x = bc.detector_input().to(torch_dev[1])
    sg = torch.cuda.Stream()
    with torch.cuda.stream(sg):
        m.prepare(D["N"], D["H"], D["W"])
        eager = {k: v.clone() for k, v in m(x).items()}
    sg.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=sg):
        out = m(x)
    for _ in range(2):
        for k in ("boxes", "scores"):
            out[k].fill_(float("nan"))
        m.rpn._rois.fill_(float("nan")), m._pooled.fill_(float("nan")), m.box_head._scores.fill_(float("nan"))
        for t in m.rpn._sel.values():
            t.view(torch.int32).fill_(0x7FC00000)
        graph.replay()
        torch.cuda.synchronize()
        for k in DET_KEYS:
            assert same_bits(out[k], eager[k]), k
    with torch.cuda.stream(sg):
        assert pkg.tickets_in_use() == 0
    del graph
    x[0, 1, 30, 40] = float("nan")
    dirty = m(x)
    torch.cuda.synchronize()
    for k in DET_KEYS:
        assert same_bits(dirty[k][1], eager[k][1]), k
    assert int(eager["count"][1]) > 0


def test_mask_rcnn_kernel_select_is_the_torch_path(pkg, R, torch_dev):
    sd, _, _ = bc.detector_state_dict(R)
    full = dict(sd)
    full.update({"roi_heads." + k: v for k, v in rc.mask_head_state_dict(D["out_channels"], D["classes"],
                                                                         seed=D["seed"] + 2).items()})
    x = bc.detector_input().to(torch_dev[1])
    want = pkg.MaskRCNN.from_state_dict(full, D["arch"], mask_P=MASK_P, masks="both", **kwargs(torch_dev[1]))(x)
    m = pkg.MaskRCNN.from_state_dict(full, D["arch"], mask_P=MASK_P, masks="both", **kwargs(torch_dev[1], select="kernel"))
    assert m.select == "kernel" and m.rpn.select == "kernel"
    got = m(x)
    torch.cuda.synchronize()
    for k in DET_KEYS + ("masks", "masks_binary"):
        assert same_bits(got[k], want[k]), k
    assert int(want["count"].min()) > 0


def test_rpn_orders_exact_ties_by_the_lower_concatenated_index(pkg, R, torch_dev):
    """An RPN head whose objectness weights are zero: every position of every level has the logits (0.5, 0.5, -1.0) of
    its three anchors, so two thirds of all proposals tie exactly, within each level and across the levels.  Each level's
    top k and the sort over the concatenation must be the reference's: the lower index first."""
    sd = dict(bc.detector_state_dict(R)[0])
    sd["rpn.head.cls_logits.weight"] = torch.zeros_like(sd["rpn.head.cls_logits.weight"])
    sd["rpn.head.cls_logits.bias"] = torch.tensor([0.5, 0.5, -1.0])
    m = pkg.FasterRCNN.from_state_dict(sd, D["arch"], **kwargs(torch_dev[1], select="kernel"))
    out = m(bc.detector_input().to(torch_dev[1]), stages=True)
    torch.cuda.synchronize()
    logits, boxes = out["rpn_logits"].cpu().numpy(), out["rpn_boxes"].cpu().numpy()
    N, ns, ks = logits.shape[0], m.rpn._n, m.rpn._k
    assert set(np.unique(logits).tolist()) == {0.5, -1.0} and sum(ks) < sum(ns)
    offs = [sum(ns[:l]) for l in range(len(ns))]
    idx = sc.select_reference(logits, ks, ns, offs)[0].astype(np.int64)
    gathered = np.take_along_axis(logits, idx, axis=1)
    order = sc.select_reference(gathered, sum(ks))[0].astype(np.int64)
    sidx = np.take_along_axis(idx, order, axis=1)
    level_of = np.concatenate([np.full(k, l, dtype=np.int32) for l, k in enumerate(ks)])
    assert np.array_equal(out["topk_idx"].cpu().numpy(), idx)
    assert np.array_equal(out["sorted_logits"].cpu().numpy(), np.take_along_axis(gathered, order, axis=1))
    assert np.array_equal(out["sorted_levels"].cpu().numpy(), level_of[order])
    want_boxes = np.stack([boxes[i, sidx[i]] for i in range(N)])
    assert np.array_equal(out["sorted_boxes"].cpu().numpy().view(np.int32), want_boxes.view(np.int32))
    # among the tied 0.5s of the sorted row the concatenated index rises: levels in order, positions in order
    for i in range(N):
        tied = out["sorted_logits"][i].cpu().numpy() == 0.5
        assert tied.sum() > ks[0] and (np.diff(order[i][tied]) > 0).all() and (np.diff(level_of[order[i]][tied]) >= 0).all()


def test_kernel_select_limits_are_refused_at_prepare(pkg, R, torch_dev):
    sd, _, _ = bc.detector_state_dict(R)
    m = pkg.FasterRCNN.from_state_dict(sd, D["arch"], **kwargs(torch_dev[1], select="kernel", max_candidates=8193))
    with pytest.raises(pkg.WinoError, match="at most 8192 candidates"):
        m.prepare(D["N"], D["H"], D["W"])
    rpn_sd = {k[len("rpn."):]: v for k, v in sd.items() if k.startswith("rpn.")}
    rpn = pkg.RPN.from_state_dict(rpn_sd, D["out_channels"], pre_nms_top_n=5000, device=torch_dev[1], select="kernel")
    with pytest.raises(pkg.WinoError, match="at most 8192 proposals"):
        rpn.prepare(1, [(64, 64), (32, 32), (16, 16), (8, 8), (4, 4)], (256, 256))
    z = lambda *s: torch.zeros(*s, device=torch_dev[1])
    with pytest.raises(pkg.WinoError, match="at most 8192 candidates"):
        importlib.import_module("cuda_winograd_amd.detection").postprocess_detections(z(6000, 64), z(6000, 5), z(2, 2), 5, max_candidates=9000, select="kernel")
