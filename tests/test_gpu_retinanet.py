"""GPU tests of the composed detector (detection.RetinaNet: ResNetFPN with P6 / P7 -> RetinaNetHead -> per level
select_topk_map and retina_decode -> select_topk -> batched_nms) on retinanet_reference.RETINA: resnet18, 64 channels, 5
classes, N = 2, 64 x 96 (levels 8x12 .. 1x1), 40 candidates per level, 10 detections.  With stages=True every stage is
checked against the fp64 transcription of torchvision's head and postprocess_detections FED THE GPU'S OWN INPUT to that
stage: the head's maps at the layers' 2e-5, decoded boxes at TIGHT, the levels' selections, the order, the kept
detections and their labels exactly; the reference reports the smallest decision margin it met (threshold, neighbouring
scores, NMS IoU) and the test asserts the generators' margins of tests/box_cases.py, so a fragile seed fails loudly.
Then: count and padding rows, one graph bitwise equal to eager, and predict on two images of different sizes."""
import numpy as np
import pytest
import torch

import box_cases as bc
import dense_detector_checks as dc
import retinanet_reference as rr
from cases import TIGHT
from dense_detector_checks import cpu
from gpu_support import R, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu
D = rr.RETINA
LAYER_TOL = 2e-5


@pytest.fixture(scope="module")
def model(pkg, R, torch_dev):
    sd, _, _ = rr.detector_state_dict(R)
    m = pkg.RetinaNet.from_state_dict(sd, D["arch"], num_classes=D["classes"], score_thresh=D["score_thresh"],
                                      nms_thresh=D["nms_thresh"], detections_per_img=D["detections"],
                                      topk_candidates=D["topk"], sizes=D["sizes"], ratios=D["ratios"], device=torch_dev[1],
                                      out_channels=D["out_channels"])
    return m, sd


def rel(got, want):
    return bc.rel_err(cpu(got).double().numpy(), np.asarray(want, dtype=np.float64))


def test_every_stage_against_fp64_on_the_gpus_own_input(model, torch_dev):
    m, sd = model
    N, H, W, K, cols = D["N"], D["H"], D["W"], D["classes"], rr.A * D["classes"]
    out = m(rr.detector_input().to(torch_dev[1]), stages=True)
    torch.cuda.synchronize()
    feats = {k: cpu(v[:, 1:-1, 1:-1, :]) for k, v in out["features"].items()}
    assert [tuple(feats[k].shape[1:3]) for k in rr.LEVELS] == rr.LEVEL_HW
    image_hw = np.array([[float(H), float(W)]] * N)
    idx_all, logit_all, tie_gaps, thresh_margin, off = cpu(out["level_idx"]).numpy(), cpu(out["level_logits"]).numpy(), [], bc.INF, 0
    for l, ((h, w), (want_cls, want_reg)) in enumerate(zip(rr.LEVEL_HW, rr.head_reference(sd, feats))):
        # the head on the GPU's features: the padded maps' interiors and real columns; pad columns and rings exactly 0
        cls_map, reg_map = cpu(out["cls_maps"][l]), cpu(out["reg_maps"][l])
        assert tuple(cls_map.shape) == (N, h + 2, w + 2, 64) and tuple(reg_map.shape) == (N, h + 2, w + 2, 64)
        cls, reg = cls_map[:, 1:-1, 1:-1, :cols], reg_map[:, 1:-1, 1:-1, :4 * rr.A]
        ec, er = rel(cls, want_cls), rel(reg, want_reg)
        assert not cls_map[:, 1:-1, 1:-1, cols:].any() and not reg_map[:, 1:-1, 1:-1, 4 * rr.A:].any()
        for t in (cls_map, reg_map):
            assert not t[:, 0].any() and not t[:, -1].any() and not t[:, :, 0].any() and not t[:, :, -1].any()
        # the level's selection on the GPU's logits
        n, k = h * w * cols, min(D["topk"], h * w * cols)
        idx, count, tm, gap = rr.level_select_reference(cls.reshape(N, n).numpy(), D["topk"], D["score_thresh"])
        thresh_margin, tie_gaps = min(thresh_margin, tm), tie_gaps + [gap]
        got_idx = idx_all[:, off:off + k]
        assert np.array_equal(got_idx, idx), f"level {l}"
        assert np.array_equal(cpu(out["level_count"])[l].numpy(), count)
        want_logit = np.where(idx >= 0, np.take_along_axis(cls.reshape(N, n).numpy(), np.maximum(idx, 0), axis=1), np.float32(0))
        assert np.array_equal(logit_all[:, off:off + k].view(np.int32), want_logit.astype(np.float32).view(np.int32))
        # the decode of the selected anchors on the GPU's regression map
        base = bc.base_anchors(D["sizes"][l], D["ratios"]).numpy()
        boxes, labels = rr.decode_selected_reference(reg.numpy(), idx, base, (h, w, H // h, W // w), image_hw, K)
        eb = rel(out["cand_boxes"][:, off:off + k], boxes)
        assert np.array_equal(cpu(out["cand_labels"])[:, off:off + k].numpy(), labels)
        print(f"level {rr.LEVELS[l]}: cls {ec:.2e} reg {er:.2e} boxes {eb:.2e} count {count.tolist()} of k={k}")
        assert ec < LAYER_TOL and er < LAYER_TOL and eb < TIGHT
        off += k
    assert off == idx_all.shape[1]
    counts = cpu(out["level_count"]).numpy()
    assert (counts < np.array([min(D["topk"], h * w * cols) for h, w in rr.LEVEL_HW])[:, None]).any(), "no level has padding rows"
    assert (counts[0] == D["topk"]).all(), "the finest level does not fill its top-k"
    # scores: sigmoid where a row is kept, else exactly 0
    valid = idx_all >= 0
    scores = cpu(out["cand_scores"]).numpy()
    assert (scores[~valid] == 0).all() and np.abs(scores[valid] - rr.sigmoid64(logit_all[valid])).max() < 1e-6
    # the tail on the GPU's candidates: order, NMS, the padded detections
    det = rr.detections_reference(cpu(out["cand_boxes"]).numpy(), scores, cpu(out["cand_labels"]).numpy(), valid,
                                  D["nms_thresh"], D["detections"])
    dc.check_tail(m, out, det, valid, D["score_thresh"], rr.assert_margins, thresh_margin, tie_gaps)


def test_one_graph_replays_bitwise(pkg, model, torch_dev):
    """The whole forward captured into one graph -- a host read of device data inside it would fail the capture -- replays
    bitwise equal to eager into NaN-filled buffers, and no ticket stays held."""
    dc.check_one_graph_replays_bitwise(pkg, model[0], rr.detector_input().to(torch_dev[1]), lambda m: (
        m._b["idx"], m._b["vals"], m._b["boxes"], m._b["sboxes"], m._b["keep"]))


def test_predict_on_two_images_of_different_sizes(pkg, model, torch_dev):
    """predict is the shared detector path: image_transform -> forward on the batch with the resized sizes -> boxes x
    ratio.  Its boxes are forward's on the transformed batch times the ratio, bit for bit, and lie inside each image."""
    dc.check_predict_on_two_images_of_different_sizes(model[0], torch_dev[1], (D["N"], D["H"], D["W"]))
