"""GPU tests of detection.KeypointHead and the composed detection.KeypointRCNN on box_cases.DETECTOR (resnet18, 64 channels,
N = 2, 64 x 96, 10 detections) with keypoint_cases.keypoint_head_state_dict(64, [64] * 8, 3) under roi_heads., keypoint_P =
4.  The head alone against fp64 at NET_TOL; with stages=True every keypoint stage against fp64 FED THE GPU'S OWN INPUT to
that stage (the rois bitwise from boxes / count, the head at NET_TOL, the kernel in the tolerance form: the detector's
boxes are its own, so no margin rule holds for them).  Then: the detections are FasterRCNN's bit for bit, rows past count
are zero, one graph (which proves no host read), predict on two images of different sizes, to_image_lists, a NaN pixel."""
import numpy as np
import pytest
import torch

import box_cases as bc
import keypoint_cases as kc
import transform_cases as tc
from gpu_support import R, same_bits, torch_dev  # noqa: F401
from reference_nets import NET_TOL

pytestmark = pytest.mark.gpu
D = bc.DETECTOR
KP_P, KP_K = 4, 3
WIDTHS = [64] * 8
DET_KEYS = ("boxes", "scores", "labels", "count", "overflow")
OUT_KEYS = DET_KEYS + ("keypoints", "keypoints_scores")
SHAPES, MIN_MAX = [(40, 60), (50, 45)], dict(min_size=64, max_size=96)


def kp_sd():
    return kc.keypoint_head_state_dict(D["out_channels"], WIDTHS, KP_K, seed=D["seed"] + 3)


def kwargs(dev, **more):
    return dict(num_classes=D["classes"], out_channels=D["out_channels"], P=D["P"], rpn_pre_nms_top_n=D["pre"],
                rpn_post_nms_top_n=D["post"], box_detections_per_img=D["detections"], device=dev, **more)


def full_sd(R):
    sd, _, _ = bc.detector_state_dict(R)
    full = dict(sd)
    full.update({"roi_heads." + k: v for k, v in kp_sd().items()})
    return full, sd


@pytest.fixture(scope="module")
def model(pkg, R, torch_dev):
    full, sd = full_sd(R)
    return pkg.KeypointRCNN.from_state_dict(full, D["arch"], keypoint_P=KP_P, **kwargs(torch_dev[1])), sd


def cpu(t):
    return t.detach().cpu()


@pytest.mark.parametrize("P", (2, 4))
def test_keypoint_head_against_fp64(pkg, torch_dev, P):
    dev, Rn, C = torch_dev[1], 3, 64
    sd = kp_sd()
    head = pkg.KeypointHead.from_state_dict(sd, C, dev)
    g = torch.Generator().manual_seed(P)
    pooled = torch.zeros(Rn, P + 2, P + 2, C)
    pooled[:, 1:-1, 1:-1] = torch.rand(Rn, P, P, C, generator=g) - 0.5
    x = pooled.to(dev)
    want = kc.keypoint_head_reference(sd, pooled[:, 1:-1, 1:-1])
    logits = cpu(head(x)).clone()
    rows, ld = head(x, raw=True)
    torch.cuda.synchronize()
    assert tuple(logits.shape) == (Rn, KP_K, 4 * P, 4 * P) and tuple(rows.shape) == (Rn * P * P, ld) and ld == 64
    assert same_bits(x, pooled), "the head wrote its input"
    e = bc.rel_err(logits.double().numpy(), want.numpy())
    composed = kc.compose_planes(cpu(rows).numpy(), cpu(head.bias).numpy(), Rn, KP_K, P)
    e_rows = bc.rel_err(composed, want.numpy())
    print(f"P={P}: keypoint head {e:.2e} (torch-composed logits), {e_rows:.2e} (the raw rows, composed in fp64)")
    assert e < NET_TOL and e_rows < NET_TOL
    assert bool((cpu(rows)[:, 16 * KP_K:] == 0).all())           # the padded columns of the GEMM
    # the kernel on the raw rows is the kernel on the composed logits
    rois = torch.tensor([[0, 1.5, 2.5, 20.25, 30.5], [1, 4.0, 4.0, 4.0 + 4 * P, 4.0 + 4 * P], [-1, 0, 0, 0, 0]], device=dev)
    a = pkg.heatmaps_to_keypoints(rows, rois, K=KP_K, M=4 * P, layout="deconv_rows", bias=head.bias, max_side=64)
    b = pkg.heatmaps_to_keypoints(logits.to(dev), rois, max_side=64)
    torch.cuda.synchronize()
    kc.check_tolerant((cpu(a[0]).numpy(), cpu(a[1]).numpy()), composed, cpu(rois).numpy(), max_side=64, tag="head rows")
    kc.check_tolerant((cpu(b[0]).numpy(), cpu(b[1]).numpy()), logits.double().numpy(), cpu(rois).numpy(), max_side=64,
                      tag="head planes")
    assert bool((a[0][2] == 0).all()) and bool((a[1][2] == 0).all())


def test_every_keypoint_stage_against_fp64_on_the_gpus_own_input(model, torch_dev):
    m, _ = model
    N, H, W, Dn, P, K = D["N"], D["H"], D["W"], D["detections"], KP_P, KP_K
    out = m(bc.detector_input().to(torch_dev[1]), stages=True)
    torch.cuda.synchronize()
    count, boxes = cpu(out["count"]), cpu(out["boxes"])
    assert int(count.min()) > 0, count
    # the keypoint rois: (n, box) for the detections, (-1, 0, 0, 0, 0) after them
    want_rois = torch.zeros(N, Dn, 5)
    want_rois[:, :, 0] = -1
    for n in range(N):
        c = int(count[n])
        want_rois[n, :c, 0] = float(n)
        want_rois[n, :c, 1:] = boxes[n, :c]
    assert same_bits(out["keypoint_rois"], want_rois)
    pad = (want_rois[:, :, 0] < 0).view(-1)
    pooled = cpu(out["keypoint_pooled"])
    assert tuple(pooled.shape) == (N * Dn, P + 2, P + 2, D["out_channels"])
    assert bool((pooled[pad] == 0).all()) and bool((pooled[~pad].abs().sum(dim=(1, 2, 3)) > 0).all())
    assert bool((pooled[:, 0] == 0).all()) and bool((pooled[:, :, -1] == 0).all())
    # the head on the GPU's pooled tensor: the raw rows, composed in fp64, against the fp64 head
    rows = cpu(out["keypoint_rows"])
    ld = int(rows.shape[1])
    assert tuple(rows.shape) == (N * Dn * P * P, ld) and ld % 64 == 0 and ld >= 16 * K
    bias = cpu(m.keypoint_head.bias).numpy()
    composed = kc.compose_planes(rows.numpy(), bias, N * Dn, K, P)
    want_logits = kc.keypoint_head_reference(kp_sd(), pooled[:, 1:-1, 1:-1, :])
    e = bc.rel_err(composed, want_logits.numpy())
    print(f"keypoint head {e:.2e}")
    assert e < NET_TOL
    # the kernel on the GPU's rows and rois, in the tolerance form
    kp, sc = cpu(out["keypoints"]).numpy(), cpu(out["keypoints_scores"]).numpy()
    assert kp.shape == (N, Dn, K, 3) and sc.shape == (N, Dn, K)
    worst = kc.check_tolerant((kp.reshape(N * Dn, K, 3), sc.reshape(N * Dn, K)), composed, want_rois.view(-1, 5).numpy(),
                              max_side=max(H, W), tag="model")
    print(f"keypoints: worst gap / score error {worst:.2e} of the range, detections {count.tolist()}")
    for n in range(N):
        c = int(count[n])
        assert (kp[n, c:] == 0).all() and (sc[n, c:] == 0).all() and (kp[n, :c, :, 2] == 1).all()
        b = boxes[n, :c].numpy()
        # a keypoint lies in its box (grown by one pixel where the box is thinner than one)
        lo, hi = b[:, None, :2], np.maximum(b[:, None, 2:], b[:, None, :2] + 1)
        assert (kp[n, :c, :, :2] >= lo).all() and (kp[n, :c, :, :2] <= hi).all()
    # to_lists gives torchvision's form
    for n, d in enumerate(m.to_lists(out)):
        c = int(count[n])
        assert tuple(d["boxes"].shape) == (c, 4) and tuple(d["keypoints"].shape) == (c, K, 3)
        assert tuple(d["keypoints_scores"].shape) == (c, K) and same_bits(d["keypoints"], out["keypoints"][n, :c])


def test_detections_are_faster_rcnns_bit_for_bit(pkg, model, torch_dev):
    m, sd = model
    x = bc.detector_input().to(torch_dev[1])
    want = pkg.FasterRCNN.from_state_dict(sd, D["arch"], **kwargs(torch_dev[1]))(x)
    got = m(x)
    torch.cuda.synchronize()
    for k in DET_KEYS:
        assert same_bits(got[k], want[k]), k
    assert "keypoints" not in want
    # select="kernel" passes through
    fk = pkg.FasterRCNN.from_state_dict(sd, D["arch"], **kwargs(torch_dev[1], select="kernel"))(x)
    full = dict(sd)
    full.update({"roi_heads." + k: v for k, v in kp_sd().items()})
    mk = pkg.KeypointRCNN.from_state_dict(full, D["arch"], keypoint_P=KP_P, **kwargs(torch_dev[1], select="kernel"))
    gk = mk(x)
    torch.cuda.synchronize()
    assert mk.select == "kernel" and mk.rpn.select == "kernel"
    for k in DET_KEYS:
        assert same_bits(gk[k], fk[k]), k


def test_rows_past_count_are_zero(pkg, model, R, torch_dev):
    """A box score threshold that leaves each image fewer detections than detections_per_img: the padding rows are rois of
    index -1, pool zeros, and their keypoints and scores are zero."""
    m, _ = model
    full, _ = full_sd(R)
    x = bc.detector_input().to(torch_dev[1])
    scores = cpu(m(x)["scores"])
    cut = float(scores[:, 6].max()) + 1e-4          # at most 6 detections per image pass
    out = pkg.KeypointRCNN.from_state_dict(full, D["arch"], keypoint_P=KP_P, box_score_thresh=cut,
                                           **kwargs(torch_dev[1]))(x, stages=True)
    torch.cuda.synchronize()
    count = cpu(out["count"])
    assert int(count.max()) <= 6 and int(count.min()) >= 1, count
    rois, pooled = cpu(out["keypoint_rois"]), cpu(out["keypoint_pooled"]).view(D["N"], D["detections"], -1)
    kp, sc = cpu(out["keypoints"]), cpu(out["keypoints_scores"])
    for n in range(D["N"]):
        c = int(count[n])
        assert bool((rois[n, c:, 0] == -1).all()) and bool((rois[n, c:, 1:] == 0).all()) and bool((rois[n, :c, 0] == n).all())
        assert bool((pooled[n, c:] == 0).all())
        assert bool((kp[n, c:] == 0).all()) and bool((sc[n, c:] == 0).all()) and bool((kp[n, :c, :, 2] == 1).all())


def test_one_graph_replays_bitwise(pkg, model, torch_dev):
    """The whole forward captured into one graph -- a host read of device data inside it would fail the capture -- replays
    bitwise equal to eager into NaN-filled buffers, and no ticket stays held."""
    m, _ = model
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
        for k in ("boxes", "scores", "keypoints", "keypoints_scores"):
            out[k].fill_(float("nan"))
        for t in (m.rpn._rois, m._pooled, m.box_head._scores, m._det_rois, m._kp_pooled, m.keypoint_head._rows):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for k in OUT_KEYS:
            assert same_bits(out[k], eager[k]), k
    with torch.cuda.stream(sg):
        assert pkg.tickets_in_use() == 0
    del graph


def test_predict_is_forward_times_the_ratio(pkg, model, torch_dev):
    """Two images of different sizes: predict's keypoints are forward's on the transformed batch (computed on the
    un-rescaled detections) times (rw, rh, 1) in fp32, its scores are forward's, and to_image_lists has torchvision's
    shapes.  Then the whole predict from one graph."""
    m, _ = model
    dev = torch_dev[1]
    imgs = [t.to(dev) for t in tc.images(SHAPES, 3, torch.float32, seed=21)]
    m.prepare_images(SHAPES, **MIN_MAX)
    sizes = [pkg.transform_size(h, w, **MIN_MAX) for h, w in SHAPES]
    Hb, Wb = pkg.batch_hw(sizes)
    batch = pkg.image_transform(imgs, sizes, Hb, Wb, pkg.IMAGENET_MEAN, pkg.IMAGENET_STD)
    hw = torch.tensor(sizes, dtype=torch.float32, device=dev)
    want = {k: v.clone() for k, v in m(batch, hw).items()}
    got = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in m.predict(imgs).items()}
    torch.cuda.synchronize()
    ratio = np.array([[np.float32(w) / np.float32(wo), np.float32(h) / np.float32(ho), 1.0]
                      for (h, w), (ho, wo) in zip(SHAPES, sizes)], dtype=np.float32)
    kp = cpu(want["keypoints"]).numpy() * ratio[:, None, None, :]
    assert kp.dtype == np.float32 and same_bits(got["keypoints"], torch.from_numpy(kp))
    assert same_bits(got["keypoints_scores"], want["keypoints_scores"])
    for k in ("scores", "labels", "count"):
        assert same_bits(got[k], want[k]), k
    count = cpu(got["count"]).tolist()
    assert sum(count) > 0 and got["original_sizes"] == list(SHAPES)
    lists = m.to_image_lists(got)
    for n, d in enumerate(lists):
        c = count[n]
        assert tuple(d["boxes"].shape) == (c, 4) and tuple(d["keypoints"].shape) == (c, KP_K, 3)
        assert tuple(d["keypoints_scores"].shape) == (c, KP_K) and tuple(d["labels"].shape) == (c,)
        assert bool((d["keypoints"][:, :, 2] == 1).all())
    # the whole predict from one graph
    sg = torch.cuda.Stream()
    with torch.cuda.stream(sg):
        m.prepare_images(SHAPES, **MIN_MAX)
        m.predict(imgs)
    sg.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=sg):
        out = m.predict(imgs)
    for k in ("boxes", "keypoints", "keypoints_scores"):
        out[k].fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for k in OUT_KEYS:
        assert same_bits(out[k], got[k]), k
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
    assert int(clean["count"][1]) > 0 and bool((clean["keypoints"][1, :, :, 2] == 1).any())
