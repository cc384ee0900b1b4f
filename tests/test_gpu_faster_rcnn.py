"""GPU tests of the composed detector (detection.FasterRCNN: ResNetFPN -> RPN -> multiscale_roi_align -> BoxHead ->
postprocess_detections) on box_cases.DETECTOR: resnet18, 64 channels, 5 classes, N = 2, 64 x 96 (levels 16x24 .. 1x2),
pre / post top-n 50 / 20, 10 detections.  With stages=True every stage is checked against the fp64 reference FED THE
GPU'S OWN INPUT to that stage: head outputs at NET_TOL, decoded boxes at TIGHT, top-k / sort / keep / rois / labels exactly;
the reference reports the smallest decision margin it met and the test asserts the generator's margins, so a fragile seed
fails loudly.  Then: one graph (which proves no host read), a NaN pixel, and the padding rows."""
import importlib

import numpy as np
import pytest
import torch

import box_cases as bc
import roi_cases as rc
from cases import TIGHT
from gpu_support import R, same_bits, torch_dev  # noqa: F401
from reference_nets import NET_TOL

pytestmark = pytest.mark.gpu
D = bc.DETECTOR
OUT_KEYS = ("boxes", "scores", "labels", "count", "overflow")


@pytest.fixture(scope="module")
def model(pkg, R, torch_dev):
    sd, _, _ = bc.detector_state_dict(R)
    m = pkg.FasterRCNN.from_state_dict(sd, D["arch"], num_classes=D["classes"], out_channels=D["out_channels"], P=D["P"],
                                       rpn_pre_nms_top_n=D["pre"], rpn_post_nms_top_n=D["post"],
                                       box_detections_per_img=D["detections"], device=torch_dev[1])
    return m, sd


def cpu(t):
    return t.detach().cpu()


def rel(got, want):
    return bc.rel_err(cpu(got).double().numpy(), np.asarray(want, dtype=np.float64))


def test_every_stage_against_fp64_on_the_gpus_own_input(model, torch_dev):
    m, sd = model
    N, H, W, A, classes = D["N"], D["H"], D["W"], 3, D["classes"]
    out = m(bc.detector_input().to(torch_dev[1]), stages=True)
    torch.cuda.synchronize()
    feats = {k: cpu(v if k == "pool" else v[:, 1:-1, 1:-1, :]) for k, v in out["features"].items()}
    assert [tuple(feats[k].shape[1:3]) for k in bc.RPN_LEVELS] == [(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)]
    image_hw = np.array([[float(H), float(W)]] * N)
    # the RPN head, and its decode in grid mode
    off, n_per_level = 0, []
    for l, (name, want) in enumerate(zip(bc.RPN_LEVELS, bc.rpn_head_reference(sd, feats))):
        h, w = feats[name].shape[1:3]
        head = cpu(out["rpn_head"][l])
        e = rel(head[:, :5 * A], want)
        n = h * w * A
        base = bc.base_anchors((32.0 * 2 ** l,), (0.5, 1.0, 2.0)).numpy()
        boxes = bc.decode_reference(head.numpy(), base, image_hw, A, grid=(h, w, H // h, W // w), delta_col=A)
        eb = rel(out["rpn_boxes"][:, off:off + n], boxes)
        print(f"level {name}: head {e:.2e}, decoded boxes {eb:.2e}")
        assert e < NET_TOL and eb < TIGHT
        assert same_bits(out["rpn_logits"][:, off:off + n], head[:, :A].reshape(N, n))
        off, n_per_level = off + n, n_per_level + [n]
    # filter_proposals on the GPU's boxes and logits
    filt = bc.filter_proposals_reference(cpu(out["rpn_boxes"]), cpu(out["rpn_logits"]), n_per_level, D["pre"], D["post"])
    assert torch.equal(cpu(out["topk_idx"]), filt["idx"])
    assert same_bits(out["sorted_logits"], filt["sorted_logits"]) and same_bits(out["sorted_boxes"], filt["sorted_boxes"])
    assert torch.equal(cpu(out["sorted_levels"]), filt["sorted_levels"])
    assert float((cpu(out["sorted_scores"]) - filt["sorted_scores"]).abs().max()) < 1e-6
    nms = bc.nms_stage(cpu(out["sorted_boxes"]), cpu(out["sorted_scores"]), cpu(out["sorted_levels"]), D["post"], bc.RPN_PARAMS)
    assert np.array_equal(cpu(out["rpn_keep"]).numpy(), nms["keep"]) and np.array_equal(cpu(out["rpn_count"]).numpy(), nms["count"])
    assert same_bits(out["rois"], torch.from_numpy(nms["rois"]))
    # the box head on the GPU's pooled tensor
    rois = cpu(out["rois"]).view(-1, 5)
    pad = rois[:, 0] < 0
    assert bool((cpu(out["pooled"])[pad] == 0).all())
    head_sd = {k[len("roi_heads."):]: v for k, v in sd.items() if k.startswith("roi_heads.")}
    cls, reg = rc.box_head_reference(head_sd, cpu(out["pooled"]))
    head_out = cpu(out["head_out"])
    e = rel(head_out[:, :5 * classes], torch.cat([cls, reg], dim=1).numpy())
    print(f"box head {e:.2e}")
    assert e < NET_TOL
    # postprocess_detections on the GPU's head output
    post = bc.postprocess_reference(head_out, rois, torch.from_numpy(image_hw), classes, D["detections"])
    ep, eb = rel(out["class_prob"], post["prob"].numpy()), rel(out["class_boxes"], post["boxes"].numpy())
    print(f"softmax {ep:.2e}, class boxes {eb:.2e}")
    assert ep < NET_TOL and eb < TIGHT
    cand = bc.candidates_reference(cpu(out["class_boxes"]), cpu(out["class_scores"]), classes - 1, D["detections"])
    assert torch.equal(cpu(out["cand_idx"]), cand["idx"]) and torch.equal(cpu(out["cand_labels"]), cand["cand_labels"])
    assert same_bits(out["cand_boxes"], cand["cand_boxes"]) and same_bits(out["cand_scores"], cand["cand_scores"])
    assert np.array_equal(cpu(out["det_keep"]).numpy(), cand["keep"]) and np.array_equal(cpu(out["count"]).numpy(), cand["count"])
    assert same_bits(out["boxes"], cand["det_boxes"]) and same_bits(out["scores"], cand["det_scores"])
    assert torch.equal(cpu(out["labels"]), cand["det_labels"]) and torch.equal(cpu(out["overflow"]), cand["overflow"])
    margins = bc.detector_margins(dict(filt, **nms), cand)
    print("margins", margins, "proposals", nms["count"].tolist(), "detections", cand["count"].tolist())
    bc.assert_margins(margins)
    assert int(cand["count"].min()) > 0
    # rows past count are zero with label -1, and to_lists gives torchvision's form
    for n, d in enumerate(m.to_lists(out)):
        c = int(cand["count"][n])
        assert tuple(d["boxes"].shape) == (c, 4) and bool((d["labels"] > 0).all())
        assert bool((cpu(out["boxes"])[n, c:] == 0).all()) and bool((cpu(out["labels"])[n, c:] == -1).all())


def test_one_graph_replays_bitwise(pkg, model, torch_dev):
    """The whole forward captured into one graph -- a host read of device data inside it would fail the capture -- replays
    bitwise equal to eager into NaN-filled buffers, and no ticket stays held."""
    m, _ = model
    x = bc.detector_input().to(torch_dev[1])
    sg = torch.cuda.Stream()
    with torch.cuda.stream(sg):
        m.prepare(*m._shape) if m._shape else m.prepare(D["N"], D["H"], D["W"])
        eager = {k: v.clone() for k, v in m(x).items()}
    sg.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=sg):
        out = m(x)
    for _ in range(2):
        for k in ("boxes", "scores"):
            out[k].fill_(float("nan"))
        m.rpn._rois.fill_(float("nan")), m._pooled.fill_(float("nan")), m.box_head._scores.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for k in OUT_KEYS:
            assert same_bits(out[k], eager[k]), k
    with torch.cuda.stream(sg):
        assert pkg.tickets_in_use() == 0
    del graph


def test_a_nan_pixel_stays_in_its_image(model, torch_dev):
    m, _ = model
    x = bc.detector_input().to(torch_dev[1])
    clean = {k: v.clone() for k, v in m(x).items()}
    x[0, 1, 30, 40] = float("nan")
    dirty = m(x)
    torch.cuda.synchronize()
    for k in OUT_KEYS:
        assert same_bits(dirty[k][1], clean[k][1]), k
    assert int(clean["count"][1]) > 0


def test_a_padding_roi_never_reaches_the_output(pkg, R, torch_dev):
    """An RPN score threshold that leaves each image fewer proposals than post_nms_top_n: the padding rows (index -1) pool
    zeros, score 0 and never appear among the detections, which are those of the kept proposals alone."""
    sd, _, _ = bc.detector_state_dict(R)
    kw = dict(num_classes=D["classes"], out_channels=D["out_channels"], P=D["P"], rpn_pre_nms_top_n=D["pre"],
              rpn_post_nms_top_n=D["post"], box_detections_per_img=D["detections"], device=torch_dev[1])
    x = bc.detector_input().to(torch_dev[1])
    full = pkg.FasterRCNN.from_state_dict(sd, D["arch"], **kw)(x, stages=True)
    cut = float(cpu(full["proposal_scores"])[:, 7].max()) + 1e-4          # at most 7 proposals per image pass
    out = pkg.FasterRCNN.from_state_dict(sd, D["arch"], rpn_score_thresh=cut, **kw)(x, stages=True)
    torch.cuda.synchronize()
    count = cpu(out["rpn_count"])
    assert int(count.max()) <= 7 and int(count.min()) >= 1
    rois = cpu(out["rois"])
    per, fg = D["post"], D["classes"] - 1
    for n in range(D["N"]):
        c = int(count[n])
        assert bool((rois[n, c:, 0] == -1).all()) and bool((rois[n, c:, 1:] == 0).all())
        assert bool((cpu(out["pooled"]).view(D["N"], per, -1)[n, c:] == 0).all())
        assert bool((cpu(out["class_scores"]).view(D["N"], per, fg)[n, c:] == 0).all())
        k = int(out["count"][n])
        src = cpu(out["cand_idx"])[n].gather(0, cpu(out["det_keep"])[n, :k].long()) // fg      # the proposal of each detection
        assert k > 0 and bool((src < c).all())


def test_more_candidates_than_max_candidates_raise_overflow(pkg, R, torch_dev):
    """postprocess_detections with max_candidates below the number of scores that pass the threshold: overflow is True
    for those images, and every output is candidates_reference's at that max_candidates, fed the GPU's own class boxes
    and scores."""
    det = importlib.import_module("cuda_winograd_amd.detection")
    m = pkg.FasterRCNN.from_state_dict(bc.detector_state_dict(R)[0], D["arch"], num_classes=D["classes"],
                                       out_channels=D["out_channels"], P=D["P"], rpn_pre_nms_top_n=D["pre"],
                                       rpn_post_nms_top_n=D["post"], box_detections_per_img=D["detections"],
                                       device=torch_dev[1])
    full = m(bc.detector_input().to(torch_dev[1]), stages=True)
    torch.cuda.synchronize()
    passing = (cpu(full["class_scores"]) >= bc.SCORE_THRESH).sum(dim=1)
    kc = int(passing.min()) // 2
    assert kc >= 4 and not bool(cpu(full["overflow"]).any()), passing
    hw = torch.tensor([[float(D["H"]), float(D["W"])]] * D["N"], device=torch_dev[1])
    stages = {}
    out = det.postprocess_detections(full["head_out"], full["rois"].view(-1, 5), hw, D["classes"],
                                     detections=D["detections"], max_candidates=kc, stages=stages)
    torch.cuda.synchronize()
    assert same_bits(stages["class_boxes"], full["class_boxes"]) and same_bits(stages["class_scores"], full["class_scores"])
    cand = bc.candidates_reference(cpu(stages["class_boxes"]), cpu(stages["class_scores"]), D["classes"] - 1,
                                   D["detections"], max_candidates=kc)
    assert cand["overflow"].tolist() == [True] * D["N"] and cpu(out["overflow"]).tolist() == [True] * D["N"]
    assert tuple(stages["cand_idx"].shape) == (D["N"], kc)
    assert torch.equal(cpu(stages["cand_idx"]), cand["idx"]) and torch.equal(cpu(stages["cand_labels"]), cand["cand_labels"])
    assert same_bits(stages["cand_boxes"], cand["cand_boxes"]) and same_bits(stages["cand_scores"], cand["cand_scores"])
    assert np.array_equal(cpu(stages["det_keep"]).numpy(), cand["keep"]) and np.array_equal(cpu(out["count"]).numpy(), cand["count"])
    assert same_bits(out["boxes"], cand["det_boxes"]) and same_bits(out["scores"], cand["det_scores"])
    assert torch.equal(cpu(out["labels"]), cand["det_labels"])
    print("passing", passing.tolist(), "max_candidates", kc, "margins", {k: cand[k] for k in ("iou_margin", "size_margin", "score_margin")})
    assert cand["iou_margin"] >= bc.IOU_MARGIN and cand["score_margin"] >= bc.SCORE_MARGIN and cand["tie_gap"] > 0
