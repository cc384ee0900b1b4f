"""GPU tests of the composed detector (detection.FCOS: ResNetFPN with P6 / P7 -> FCOSHead with GroupNorm -> per level
fcos_score_map, select_topk_map and fcos_decode -> select_topk -> batched_nms) on fcos_reference.FCOS: resnet18, 64
channels, 5 classes, N = 2, 64 x 96 (levels 8x12 .. 1x1), 40 candidates per level, 10 detections.  Every stage is checked
against the fp64 transcription of torchvision's head and postprocess_detections FED THE GPU'S OWN INPUT to that stage, at
the bars tests/test_gpu_retinanet.py uses: every launch of the head (convolution or GroupNorm) at the layers' 2e-5, and
the head as one stage at 2e-5 where a group holds 12 values or more (at the 1x1 level, groups of two values, it reads
2.9e-5 with every launch right: fcos_reference.head_reference), score maps
and decoded boxes at TIGHT, the levels' selections, the order, the kept detections and their labels exactly; the
reference's decision margins are held to tests/box_cases.py's.  Then: one graph bitwise equal to eager, and predict on two images of different sizes."""
import numpy as np
import pytest
import torch

import box_cases as bc
import dense_detector_checks as dc
import fcos_reference as fr
from cases import TIGHT
from dense_detector_checks import cpu
from gpu_support import R, same_bits, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu
D = fr.FCOS
LAYER_TOL = 2e-5


@pytest.fixture(scope="module")
def model(pkg, R, torch_dev):
    sd, _, _ = fr.detector_state_dict(R)
    m = pkg.FCOS.from_state_dict(sd, D["arch"], num_classes=D["classes"], score_thresh=D["score_thresh"],
                                 nms_thresh=D["nms_thresh"], detections_per_img=D["detections"], topk_candidates=D["topk"],
                                 sizes=D["sizes"], device=torch_dev[1], out_channels=D["out_channels"])
    return m, sd


def rel(got, want):
    return bc.rel_err(cpu(got).double().numpy(), np.asarray(want, dtype=np.float64))


def test_every_stage_against_fp64_on_the_gpus_own_input(pkg, model, torch_dev):
    m, sd = model
    N, H, W, K = D["N"], D["H"], D["W"], D["classes"]
    out = m(fr.detector_input().to(torch_dev[1]), stages=True)
    torch.cuda.synchronize()
    score_maps = [cpu(t) for t in out["cls_maps"]]                    # (the head below writes the same tensors again)
    idx_all, score_all = cpu(out["level_idx"]).numpy(), cpu(out["level_scores"]).numpy()
    feats = {k: cpu(v[:, 1:-1, 1:-1, :]) for k, v in out["features"].items()}
    assert [tuple(feats[k].shape[1:3]) for k in fr.LEVELS] == fr.LEVEL_HW
    # the head alone on the GPU's features: the logits the forward overwrote with scores
    cls_maps, reg_maps = m.head([out["features"][k] for k in fr.LEVELS])
    torch.cuda.synchronize()
    cls_maps, reg_maps = [cpu(t) for t in cls_maps], [cpu(t) for t in reg_maps]
    image_hw = np.array([[float(H), float(W)]] * N)
    tie_gaps, thresh_margin, off, negative = [], bc.INF, 0, False
    inner = lambda t: cpu(t)[:, 1:-1, 1:-1, :]
    whole_head = fr.head_reference(sd, feats)
    C, ones = D["out_channels"], m.head._ones
    for l, (h, w) in enumerate(fr.LEVEL_HW):
        # the head's launches one by one, each against fp64 on the GPU's own input to it: on a 1 x 1 level a group is two
        # values, and a GroupNorm multiplies the rounding of the convolution in front of it by up to 1 / sqrt(eps)
        worst, last = 0.0, []
        for (convs, norms, U, bias, kp), name in zip(m.head.towers, ("classification_head", "regression_head")):
            x = out["features"][fr.LEVELS[l]]
            for i, ((Ui, bi), (gamma, beta)) in enumerate(zip(convs, norms)):
                y = pkg.conv3x3_bn_relu(x, Ui, bi, ones[:C], relu=False)
                worst = max(worst, rel(inner(y), fr.conv_reference(sd, f"{name}.conv.{3 * i}", inner(x))))
                x = pkg.groupnorm_relu(y.clone(), gamma, beta, 32)
                worst = max(worst, rel(inner(x), fr.norm_reference(sd, f"{name}.conv.{3 * i + 1}", inner(y))))
            last.append((pkg.conv3x3_bn_relu(x, U, bias, ones[:kp], relu=False), inner(x)))
        torch.cuda.synchronize()
        cls_map, reg_map = cls_maps[l], reg_maps[l]
        assert same_bits(last[0][0], cls_map) and same_bits(last[1][0], reg_map), "the head's own launches differ"
        assert tuple(cls_map.shape) == (N, h + 2, w + 2, 64) and tuple(reg_map.shape) == (N, h + 2, w + 2, 64)
        assert same_bits(reg_map, out["reg_maps"][l]), "the head is not deterministic"
        cls, reg, ctr = cls_map[:, 1:-1, 1:-1, :K], reg_map[:, 1:-1, 1:-1, :4], reg_map[:, 1:-1, 1:-1, 4]
        ec = rel(cls, fr.conv_reference(sd, "classification_head.cls_logits", last[0][1]))
        er = rel(reg, fr.conv_reference(sd, "regression_head.bbox_reg", last[1][1]))
        et = rel(ctr, fr.conv_reference(sd, "regression_head.bbox_ctrness", last[1][1])[..., 0])
        assert worst < LAYER_TOL, (l, worst)
        # the head as one stage, from the GPU's features: the layers' bar where a group holds at least 12 values (levels
        # 0 .. 2); a group of 4 (1 x 2) or 2 (1 x 1) values multiplies the rounding in front of it by up to
        # 1 / sqrt(eps) = 316, and those levels are held to the launches above and to the bit-equal chain
        composed = [rel(t, want) for t, want in zip((cls, reg, ctr), whole_head[l])]
        assert max(composed) < LAYER_TOL or h * w * (C // 32) < 12, (l, composed)
        assert not cls_map[:, 1:-1, 1:-1, K:].any() and not reg_map[:, 1:-1, 1:-1, 5:].any()
        for t in (cls_map, reg_map, score_maps[l]):
            assert not t[:, 0].any() and not t[:, -1].any() and not t[:, :, 0].any() and not t[:, :, -1].any()
        # the score map on the GPU's logits and centerness; pad columns still exactly 0
        score = score_maps[l][:, 1:-1, 1:-1, :K]
        es = rel(score, fr.score_reference(cls.numpy(), ctr.numpy()))
        assert not score_maps[l][:, 1:-1, 1:-1, K:].any()
        # the level's selection on the GPU's scores
        n, k = h * w * K, min(D["topk"], h * w * K)
        flat = score.reshape(N, n).numpy()
        idx, count, tm, gap = fr.level_select_reference(flat, D["topk"], D["score_thresh"])
        thresh_margin, tie_gaps = min(thresh_margin, tm), tie_gaps + [gap]
        assert np.array_equal(idx_all[:, off:off + k], idx), f"level {l}"
        assert np.array_equal(cpu(out["level_count"])[l].numpy(), count)
        want_score = np.where(idx >= 0, np.take_along_axis(flat, np.maximum(idx, 0), axis=1), np.float32(0))
        assert np.array_equal(score_all[:, off:off + k].view(np.int32), want_score.astype(np.float32).view(np.int32))
        # the decode of the selected locations on the GPU's regression map
        base = bc.base_anchors(D["sizes"][l], (1.0,)).numpy()
        boxes, labels = fr.decode_selected_reference(reg.numpy(), idx, base, (h, w, H // h, W // w), image_hw, K)
        eb = rel(out["cand_boxes"][:, off:off + k], boxes)
        assert np.array_equal(cpu(out["cand_labels"])[:, off:off + k].numpy(), labels)
        print(f"level {fr.LEVELS[l]}: head as one stage {max(composed):.2e} tower layers {worst:.2e} cls {ec:.2e} reg {er:.2e} "
              f"ctr {et:.2e} score {es:.2e} boxes {eb:.2e} count {count.tolist()} of k={k}")
        assert ec < LAYER_TOL and er < LAYER_TOL and et < LAYER_TOL and es < TIGHT and eb < TIGHT
        negative = negative or bool((reg.numpy() < 0).any())
        off += k
    assert off == idx_all.shape[1]
    assert negative, "no regression output is negative: the decode's ReLU has nothing to do"
    counts = cpu(out["level_count"]).numpy()
    assert (counts < np.array([min(D["topk"], h * w * K) for h, w in fr.LEVEL_HW])[:, None]).any(), "no level has padding rows"
    assert (counts[0] == D["topk"]).all(), "the finest level does not fill its top-k"
    valid = idx_all >= 0
    assert (score_all[~valid] == 0).all() and (score_all[valid] > D["score_thresh"]).all()
    # the tail on the GPU's candidates: order, NMS, the padded detections
    det = fr.detections_reference(cpu(out["cand_boxes"]).numpy(), score_all, cpu(out["cand_labels"]).numpy(), valid,
                                  D["nms_thresh"], D["detections"])
    dc.check_tail(m, out, det, valid, D["score_thresh"], fr.assert_margins, thresh_margin, tie_gaps)


def test_one_graph_replays_bitwise(pkg, model, torch_dev):
    """The whole forward captured into one graph -- a host read of device data inside it would fail the capture -- replays
    bitwise equal to eager into NaN-filled buffers, and no ticket stays held."""
    dc.check_one_graph_replays_bitwise(pkg, model[0], fr.detector_input().to(torch_dev[1]), lambda m: (
        m._b["idx"], m._b["vals"], m._b["boxes"], m._b["sboxes"], m._b["keep"], *m.head._gn_ws))


def test_predict_on_two_images_of_different_sizes(pkg, model, torch_dev):
    """predict is the shared detector path: image_transform -> forward on the batch with the resized sizes -> boxes x
    ratio.  Its boxes are forward's on the transformed batch times the ratio, bit for bit, and lie inside each image."""
    dc.check_predict_on_two_images_of_different_sizes(model[0], torch_dev[1], (D["N"], D["H"], D["W"]))
