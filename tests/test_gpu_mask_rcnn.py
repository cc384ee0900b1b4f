"""GPU tests of the composed detection.MaskRCNN on box_cases.DETECTOR (resnet18, 64 channels, 5 classes, N = 2, 64 x 96,
10 detections) with roi_cases.mask_head_state_dict(64, 5) under roi_heads., mask_P = 14.  With stages=True every new stage
is checked against fp64 FED THE GPU'S OWN INPUT to that stage: the mask rois bitwise from boxes / count, the mask head at
NET_TOL, the paste at TIGHT with the boxes' int_margin printed and asserted, so a fragile seed fails loudly.  Then: the
detections are FasterRCNN's bit for bit, one graph (which proves no host read), a NaN pixel, and to_lists."""
import numpy as np
import pytest
import torch

import box_cases as bc
import mask_cases as mc
import roi_cases as rc
from cases import TIGHT
from gpu_support import R, same_bits, torch_dev  # noqa: F401
from reference_nets import NET_TOL

pytestmark = pytest.mark.gpu
D = bc.DETECTOR
MASK_P = 14
DET_KEYS = ("boxes", "scores", "labels", "count", "overflow")
OUT_KEYS = DET_KEYS + ("masks", "masks_binary")
MODEL_MARGIN = 1e-4      # the boxes are the detector's own: what the seed must keep (the generator's cases keep 1e-3)


def mask_sd():
    return rc.mask_head_state_dict(D["out_channels"], D["classes"], seed=D["seed"] + 2)


def kwargs(dev):
    return dict(num_classes=D["classes"], out_channels=D["out_channels"], P=D["P"], rpn_pre_nms_top_n=D["pre"],
                rpn_post_nms_top_n=D["post"], box_detections_per_img=D["detections"], device=dev)


@pytest.fixture(scope="module")
def model(pkg, R, torch_dev):
    sd, _, _ = bc.detector_state_dict(R)
    full = dict(sd)
    full.update({"roi_heads." + k: v for k, v in mask_sd().items()})
    m = pkg.MaskRCNN.from_state_dict(full, D["arch"], mask_P=MASK_P, masks="both", **kwargs(torch_dev[1]))
    return m, sd


def cpu(t):
    return t.detach().cpu()


def test_every_mask_stage_against_fp64_on_the_gpus_own_input(model, torch_dev):
    m, _ = model
    N, H, W, Dn, classes, P = D["N"], D["H"], D["W"], D["detections"], D["classes"], MASK_P
    out = m(bc.detector_input().to(torch_dev[1]), stages=True)
    torch.cuda.synchronize()
    count, boxes, labels = cpu(out["count"]), cpu(out["boxes"]), cpu(out["labels"])
    assert int(count.min()) > 0, count
    # the mask rois: (n, box) for the detections, (-1, 0, 0, 0, 0) after them
    want_rois = torch.zeros(N, Dn, 5)
    want_rois[:, :, 0] = -1
    for n in range(N):
        c = int(count[n])
        want_rois[n, :c, 0] = float(n)
        want_rois[n, :c, 1:] = boxes[n, :c]
    assert same_bits(out["mask_rois"], want_rois)
    pad = (want_rois[:, :, 0] < 0).view(-1)
    pooled = cpu(out["mask_pooled"])
    assert tuple(pooled.shape) == (N * Dn, P + 2, P + 2, D["out_channels"])
    assert bool((pooled[pad] == 0).all()) and bool((pooled[~pad].abs().sum(dim=(1, 2, 3)) > 0).all())
    assert bool((pooled[:, 0] == 0).all()) and bool((pooled[:, :, -1] == 0).all())
    # the mask head on the GPU's pooled tensor; the raw logits are rows (r, y, x, dy, dx)
    raw = cpu(out["mask_logits"])
    kp = int(raw.shape[1])
    assert tuple(raw.shape) == (N * Dn * P * P * 4, kp) and kp % 64 == 0
    got_logits = raw.view(N * Dn, P, P, 2, 2, kp)[..., :classes].permute(0, 5, 1, 3, 2, 4).reshape(N * Dn, classes, 2 * P, 2 * P)
    want_logits = rc.mask_head_reference(mask_sd(), pooled[:, 1:-1, 1:-1, :])
    e = bc.rel_err(got_logits.double().numpy(), want_logits.numpy())
    print(f"mask head {e:.2e}")
    assert e < NET_TOL
    # the paste on the GPU's logits, labels and boxes
    hw = np.array([[float(H), float(W)]] * N, dtype=np.float32)
    want, margin = mc.paste_reference(got_logits.contiguous().numpy(), labels.numpy(), boxes.numpy(), hw, H, W)
    masks = cpu(out["masks"]).numpy()
    err = float(np.abs(masks - want).max())
    print(f"paste max |got - want| = {err:.2e}, int_margin {margin:.2e}, detections {count.tolist()}")
    assert margin >= MODEL_MARGIN
    assert err < TIGHT
    assert np.array_equal(cpu(out["masks_binary"]).numpy(), (masks > 0.5).astype(np.uint8))
    for n in range(N):
        c = int(count[n])
        assert (masks[n, c:] == 0).all() and all((masks[n, d] > 0).any() for d in range(c))
    # to_lists gives torchvision's form
    for n, d in enumerate(m.to_lists(out)):
        c = int(count[n])
        assert tuple(d["boxes"].shape) == (c, 4) and tuple(d["masks"].shape) == (c, 1, H, W)
        assert tuple(d["masks_binary"].shape) == (c, 1, H, W) and d["masks_binary"].dtype == torch.uint8
        assert same_bits(d["masks"][:, 0], out["masks"][n, :c])


def test_detections_are_faster_rcnns_bit_for_bit(pkg, model, torch_dev):
    m, sd = model
    x = bc.detector_input().to(torch_dev[1])
    want = pkg.FasterRCNN.from_state_dict(sd, D["arch"], **kwargs(torch_dev[1]))(x)
    got = m(x)
    torch.cuda.synchronize()
    for k in DET_KEYS:
        assert same_bits(got[k], want[k]), k
    assert "masks" not in want


def test_planes_past_count_are_zero(pkg, model, torch_dev):
    """A box score threshold that leaves each image fewer detections than detections_per_img: the padding rows carry
    label -1, are rois of index -1, pool zeros, and their planes are zero in both outputs."""
    m, sd = model
    full = dict(sd)
    full.update({"roi_heads." + k: v for k, v in mask_sd().items()})
    x = bc.detector_input().to(torch_dev[1])
    scores = cpu(m(x)["scores"])
    cut = float(scores[:, 6].max()) + 1e-4          # at most 6 detections per image pass
    out = pkg.MaskRCNN.from_state_dict(full, D["arch"], mask_P=MASK_P, masks="both", box_score_thresh=cut,
                                       **kwargs(torch_dev[1]))(x, stages=True)
    torch.cuda.synchronize()
    count = cpu(out["count"])
    assert int(count.max()) <= 6 and int(count.min()) >= 1, count
    rois, pooled = cpu(out["mask_rois"]), cpu(out["mask_pooled"]).view(D["N"], D["detections"], -1)
    for n in range(D["N"]):
        c = int(count[n])
        assert bool((cpu(out["labels"])[n, c:] == -1).all()) and bool((cpu(out["labels"])[n, :c] > 0).all())
        assert bool((rois[n, c:, 0] == -1).all()) and bool((rois[n, c:, 1:] == 0).all()) and bool((rois[n, :c, 0] == n).all())
        assert bool((pooled[n, c:] == 0).all())
        assert bool((cpu(out["masks"])[n, c:] == 0).all()) and bool((cpu(out["masks_binary"])[n, c:] == 0).all())
        assert all(bool((out["masks"][n, d] > 0).any()) for d in range(c))


def test_masks_argument_selects_the_outputs(pkg, model, R, torch_dev):
    m, sd = model
    full = dict(sd)
    full.update({"roi_heads." + k: v for k, v in mask_sd().items()})
    x = bc.detector_input().to(torch_dev[1])
    both = {k: v.clone() for k, v in m(x).items()}
    prob = pkg.MaskRCNN.from_state_dict(full, D["arch"], mask_P=MASK_P, **kwargs(torch_dev[1]))(x)
    binary = pkg.MaskRCNN.from_state_dict(full, D["arch"], mask_P=MASK_P, masks="binary", mask_threshold=0.5,
                                          **kwargs(torch_dev[1]))(x)
    torch.cuda.synchronize()
    assert "masks_binary" not in prob and "masks" not in binary
    assert same_bits(prob["masks"], both["masks"]) and same_bits(binary["masks_binary"], both["masks_binary"])


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
        for k in ("boxes", "scores", "masks"):
            out[k].fill_(float("nan"))
        out["masks_binary"].fill_(255)
        for t in (m.rpn._rois, m._pooled, m.box_head._scores, m._det_rois, m._mask_pooled, m.mask_head._scores):
            t.fill_(float("nan"))
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
    assert int(clean["count"][1]) > 0 and bool((clean["masks"][1] > 0).any())
