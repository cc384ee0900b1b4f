"""Host tests of the keypoint output stage, no GPU: tests/keypoint_cases.py's fp64 reference against a literal transcription
of torchvision's heatmaps_to_keypoints on torch-CPU fp64 F.interpolate(mode="bicubic"); the DECONV_ROWS gather and x2
upsample and pack_kps_deconv against fp64 F.conv_transpose2d + F.interpolate; the generator (every named case reaches its
margin within the cap, the classes are what they say); and what heatmaps_to_keypoints, KeypointHead and KeypointRCNN
refuse before the library or a device is touched."""
import importlib

import numpy as np
import pytest
import torch

import keypoint_cases as kc

F = torch.nn.functional
MS = (4, 8, 28, 56)
REAL = tuple(n for n in kc.BOX_CLASSES if n not in kc.SPECIAL)


def torchvision_heatmaps_to_keypoints(maps, rois):
    """torchvision.models.detection.roi_heads.heatmaps_to_keypoints, line by line; maps [R][K][M][M] fp64, rois [R][4]
    float32.  Also returns the positions."""
    offset_x = rois[:, 0]
    offset_y = rois[:, 1]
    widths = rois[:, 2] - rois[:, 0]
    heights = rois[:, 3] - rois[:, 1]
    widths = widths.clamp(min=1)
    heights = heights.clamp(min=1)
    widths_ceil = widths.ceil()
    heights_ceil = heights.ceil()
    num_keypoints = maps.shape[1]
    xy_preds = torch.zeros((len(rois), 3, num_keypoints), dtype=torch.float32)
    end_scores = torch.zeros((len(rois), num_keypoints), dtype=maps.dtype)
    positions = torch.zeros((len(rois), num_keypoints), dtype=torch.int64)
    for i in range(len(rois)):
        roi_map_width = int(widths_ceil[i].item())
        roi_map_height = int(heights_ceil[i].item())
        width_correction = widths[i] / roi_map_width
        height_correction = heights[i] / roi_map_height
        roi_map = F.interpolate(maps[i][:, None], size=(roi_map_height, roi_map_width), mode="bicubic",
                                align_corners=False)[:, 0]
        w = roi_map.shape[2]
        pos = roi_map.reshape(num_keypoints, -1).argmax(dim=1)
        x_int = pos % w
        y_int = torch.div(pos - x_int, w, rounding_mode="floor")
        x = (x_int.float() + 0.5) * width_correction
        y = (y_int.float() + 0.5) * height_correction
        xy_preds[i, 0, :] = x + offset_x[i]
        xy_preds[i, 1, :] = y + offset_y[i]
        xy_preds[i, 2, :] = 1
        end_scores[i, :] = roi_map[torch.arange(num_keypoints), y_int, x_int]
        positions[i] = pos
    return xy_preds.permute(0, 2, 1), end_scores, positions


@pytest.mark.parametrize("M", MS)
def test_reference_is_torchvision(M):
    K = 3
    rois, names = kc.class_rois(M, REAL)
    planes, _ = kc.draw_planes(rois, K, M, seed=M)
    want = kc.reference(planes, rois)
    assert (want["margin"] >= kc.MARGIN).all()
    xy, scores, pos = torchvision_heatmaps_to_keypoints(torch.from_numpy(planes).double(), torch.from_numpy(rois[:, 1:]))
    assert np.array_equal(pos.numpy(), want["pos"]), names
    err = float(np.abs(scores.numpy() - want["scores"]).max())
    print(f"M={M}: max |reference - torch fp64| = {err:.2e}")
    assert err < 1e-10
    assert np.array_equal(xy.numpy().view(np.uint32), want["xy"].view(np.uint32))


@pytest.mark.parametrize("M", (4, 8))
def test_cubic_coefficients_are_torchs_at_the_exact_cases(M):
    assert np.array_equal(kc.cubic_coefficients(0.0), [0, 1, 0, 0])
    c = kc.cubic_coefficients(np.array([0.25, 0.75])) * 256
    assert np.array_equal(c, np.round(c)) and np.array_equal(c.sum(axis=1), [256, 256])
    # identity: the resize is the plane; 2M: t is 0.75 then 0.25, and the first / last taps clamp
    W, T = kc.resize_weights(M, M)
    assert np.array_equal(W, np.eye(M))
    W2, _ = kc.resize_weights(M, 2 * M)
    assert np.array_equal(W2 * 256, np.round(W2 * 256)) and np.allclose(W2.sum(axis=1), 1, atol=0)
    planes = kc.exact_planes(M)
    want = kc.reference(planes, kc.exact_rois(M))
    a = (M * M) // 3
    # at identity a NaN at (y, x) reaches the outputs whose taps d - 1 .. d + 2 include it: the first is (y - 2, x - 2)
    first = lambda flat: max(flat // M - 2, 0) * M + max(flat % M - 2, 0)
    assert want["pos"][0, 1] == a and want["pos"][0, 2] == 0 and want["pos"][0, 3] == first(a) == want["pos"][0, 5]
    assert want["pos"][0, 4] == first(M * M - 1) and np.isnan(want["scores"][0, 3:]).all() and want["scores"][0, 1] == 64.0
    assert (want["scores"][:, 2] == 5.0).all() and (want["pos"][:, 2] == 0).all()
    assert np.isnan(want["scores"][1, 3:]).all()
    # every exact value is a float32
    big = kc.resize_plane(planes[1, 0], 2 * M, 2 * M)
    assert np.array_equal(big, big.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("P,K", ((1, 1), (2, 3), (7, 2), (14, 3)))
def test_gather_and_upsample_are_conv_transpose_and_interpolate(pkg, P, K):
    det = importlib.import_module("cuda_winograd_amd.detection")
    g = torch.Generator().manual_seed(P)
    R, C = 2, 8
    x = torch.randn(R, C, P, P, generator=g, dtype=torch.float64)
    w = torch.randn(C, K, 4, 4, generator=g, dtype=torch.float64)
    b = torch.randn(K, generator=g, dtype=torch.float64)
    B, bias = det.pack_kps_deconv(w, b)
    assert tuple(B.shape) == (C, -(-16 * K // 64) * 64) and bool((B[:, 16 * K:] == 0).all()) and torch.equal(bias, b)
    rows = (x.permute(0, 2, 3, 1).reshape(R * P * P, C) @ B).numpy()          # the GEMM's output, ld = pad64(16 K)
    low = F.conv_transpose2d(x, w, b, stride=2, padding=1)
    assert float(np.abs(kc.gather_low(rows, bias.numpy(), R, K, P) - low.numpy()).max()) < 1e-12
    up = F.interpolate(low, scale_factor=2, mode="bilinear", align_corners=False)
    assert float(np.abs(kc.compose_planes(rows, bias.numpy(), R, K, P) - up.numpy()).max()) < 1e-12
    # the torch composition KeypointHead(raw=False) uses
    cols = torch.from_numpy(rows)[:, :16 * K].view(R, P, P, 4, 4, K).permute(0, 5, 3, 4, 1, 2).reshape(R, 16 * K, P * P)
    folded = F.fold(cols, (2 * P, 2 * P), kernel_size=4, stride=2, padding=1) + b.view(1, K, 1, 1)
    assert float((folded - low).abs().max()) < 1e-12
    # to_deconv_rows is the header's index
    parts = np.arange(R * P * P * 16 * K, dtype=np.float32).reshape(R, P, P, 4, 4, K)
    r2 = kc.to_deconv_rows(parts, 16 * K + 5)
    assert r2[(1 * P + (P - 1)) * P + 0, (2 * 4 + 3) * K + (K - 1)] == parts[1, P - 1, 0, 2, 3, K - 1]
    assert np.isnan(r2[:, 16 * K:]).all()


@pytest.mark.parametrize("M", MS)
def test_generator_reaches_its_margin_and_the_classes_are_what_they_say(M):
    rois, names = kc.class_rois(M)
    assert tuple(names) == kc.BOX_CLASSES
    b = kc.box_arith(rois)
    at = {n: i for i, n in enumerate(names)}
    wc, hc, w, h = b["wc"], b["hc"], b["w"], b["h"]
    assert (b["kind"][[at[n] for n in REAL]] == 0).all()
    assert b["kind"][at["padding"]] == 1 and b["kind"][at["nonfinite"]] == 2 and b["kind"][at["oversize"]] == 2
    assert wc[at["identity"]] == hc[at["identity"]] == M and w[at["identity"]] == M
    assert wc[at["up_even"]] == 2 * M and hc[at["up_odd"]] == 3 * M and w[at["up_even"]] == 2 * M
    i = at["fractional"]
    assert w[i] != wc[i] and h[i] != hc[i] and b["cw"][i] != 1 and b["ch"][i] != 1 and wc[i] > M
    assert wc[at["down"]] < M and hc[at["down"]] < M
    i = at["one_pixel"]
    assert rois[i, 3] - rois[i, 1] < 1 and rois[i, 4] - rois[i, 2] < 1 and wc[i] == hc[i] == 1
    assert rois[at["inverted"], 3] < rois[at["inverted"], 1] and wc[at["inverted"]] == 1 and hc[at["inverted"]] > 1
    assert hc[at["thin_row"]] == 1 and wc[at["thin_row"]] > 1 and wc[at["thin_column"]] == 1 and hc[at["thin_column"]] > 1
    assert wc[at["wide"]] == 300 > 256 and hc[at["wide"]] == 3 and hc[at["tall"]] == 300 and wc[at["tall"]] == 3
    assert kc.MAX_SIDE >= 300 and rois[at["oversize"], 3] > kc.MAX_SIDE
    for K, seed in ((1, 0), (3, 1)):
        planes, draws = kc.draw_planes(rois, K, M, seed=seed)
        want = kc.reference(planes, rois)
        real = b["kind"] == 0
        assert (want["margin"][real] >= kc.MARGIN).all() and int(draws.max()) < kc.MAX_DRAWS
        assert (want["pos"][~real] == -1).all() and (want["scores"][at["padding"]] == 0).all()
        assert np.isnan(want["xy"][at["nonfinite"]]).all() and np.isnan(want["scores"][at["oversize"]]).all()
        print(f"M={M} K={K}: most draws {int(draws.max())}, mean {float(draws[real].mean()):.2f}")
    # the composed planes of DECONV_ROWS: every plane keeps the margin too, except `wide` and `tall` at P = 1
    parts, bias, draws, kept = kc.draw_deconv_parts(rois, 2, M // 4, seed=2)
    planes = kc.compose_planes(parts.reshape(-1, 32), bias, len(rois), 2, M // 4)
    margin = kc.reference(planes, rois)["margin"]
    assert (margin[kept & real[:, None]] >= kc.MARGIN).all()
    lost = sorted({names[r] for r in np.flatnonzero(~kept.all(axis=1))})
    assert lost == (["tall", "wide"] if M == 4 else []), lost


def test_a_nan_reaches_exactly_the_outputs_whose_taps_include_it():
    M = 8
    p = np.random.RandomState(0).standard_normal((M, M))
    p[3, 4] = np.nan
    same = kc.resize_plane(p, M, M)
    assert int(np.isnan(same).sum()) == 16 and np.isnan(same[1:5, 2:6]).all()      # the outputs d with 3 (4) in d - 1 .. d + 2
    big = kc.resize_plane(p, 20, 13)
    rows, cols = np.isnan(big).any(axis=1), np.isnan(big).any(axis=0)
    assert np.array_equal(np.isnan(big), np.outer(rows, cols)) and 0 < rows.sum() < 20 and 0 < cols.sum() < 13
    assert kc.plane_result(p, 20, 13)[0] == int(np.flatnonzero(np.isnan(big.reshape(-1)))[0])


# ---- what the wrapper and the model refuse before the library or a device is touched --------------------------------------
def test_heatmaps_to_keypoints_refuses_bad_arguments(pkg):
    maps, rois = torch.zeros(2, 3, 4, 4), torch.zeros(2, 5)
    for kw, msg in ((dict(layout="rows"), "layout"), (dict(max_side=0), "max_side"), (dict(max_side=16385), "max_side"),
                    (dict(), "CUDA")):
        with pytest.raises(pkg.WinoError, match=msg):
            pkg.heatmaps_to_keypoints(maps, rois, **kw)


def test_keypoint_head_validates_the_state_dict(pkg):
    det = importlib.import_module("cuda_winograd_amd.detection")
    sd = kc.keypoint_head_state_dict(64, [64] * 8, 3)
    assert det.validate_keypoint_head_state_dict(sd, 64) == 3
    assert sorted(det.expected_keypoint_head_keys(64, [64] * 8, 3)) == sorted(sd)
    mixed = kc.keypoint_head_state_dict(128, [64, 128, 64, 64, 192, 64, 64, 128], 17)
    assert det.validate_keypoint_head_state_dict(mixed, 128) == 17
    for d, msg in (({k: v for k, v in sd.items() if k != "keypoint_head.6.bias"}, "missing key 'keypoint_head.6.bias'"),
                   ({k: v for k, v in sd.items() if k != "keypoint_head.14.weight"}, "missing key 'keypoint_head.14.weight'"),
                   ({k: v for k, v in sd.items() if "kps_score_lowres.weight" not in k}, "missing key"),
                   (dict(sd, **{"keypoint_head.16.weight": torch.zeros(64, 64, 3, 3)}), "unexpected key 'keypoint_head.16.weight'"),
                   (dict(sd, **{"keypoint_head.1.weight": torch.zeros(1)}), "unexpected key 'keypoint_head.1.weight'"),
                   (dict(sd, **{"keypoint_head.2.bias": torch.zeros(32)}), "has shape"),
                   (dict(sd, **{"keypoint_predictor.kps_score_lowres.bias": torch.zeros(4)}), "has shape"),
                   (dict(sd, **{"keypoint_predictor.kps_score_lowres.weight": torch.zeros(64, 3, 2, 2)}), "has shape"),
                   (kc.keypoint_head_state_dict(64, [64] * 7 + [96], 3), "multiple of 64")):
        with pytest.raises(pkg.WinoError, match=msg):
            det.validate_keypoint_head_state_dict(d, 64)
    with pytest.raises(pkg.WinoError, match="has shape"):
        det.validate_keypoint_head_state_dict(sd, 128)
    with pytest.raises(pkg.WinoError, match="CUDA"):
        pkg.KeypointHead.from_state_dict(sd, 64, device="cpu")


def test_keypoint_rcnn_splits_and_validates_the_state_dict(pkg):
    det = importlib.import_module("cuda_winograd_amd.detection")
    kp = {"roi_heads." + k: v for k, v in kc.keypoint_head_state_dict(64, [64] * 8, 3).items()}
    sd = dict(kp)
    sd.update({"backbone.body.conv1.weight": torch.zeros(1), "rpn.head.cls_logits.bias": torch.zeros(3),
               "roi_heads.box_head.fc6.bias": torch.zeros(1)})
    rest, got = det.split_keypoint_state_dict(sd)
    assert sorted(got) == sorted(k[len("roi_heads."):] for k in kp)
    assert sorted(rest) == ["backbone.body.conv1.weight", "roi_heads.box_head.fc6.bias", "rpn.head.cls_logits.bias"]
    make = lambda d, **kw: pkg.KeypointRCNN.from_state_dict(d, "resnet18", out_channels=64, **kw)
    for P in (0, 17, -2):
        with pytest.raises(pkg.WinoError, match="keypoint_P"):
            make(sd, keypoint_P=P)
    with pytest.raises(pkg.WinoError, match="select must be one of"):
        make(sd, select="numpy")
    with pytest.raises(pkg.WinoError, match="missing key 'keypoint_predictor.kps_score_lowres.bias'"):
        make({k: v for k, v in sd.items() if k != "roi_heads.keypoint_predictor.kps_score_lowres.bias"})
    with pytest.raises(pkg.WinoError, match="unexpected key 'keypoint_head.3.weight'"):
        make(dict(sd, **{"roi_heads.keypoint_head.3.weight": torch.zeros(64, 64, 3, 3)}))
    with pytest.raises(pkg.WinoError, match="missing key 'keypoint_head.0.weight'"):
        make({k: v for k, v in sd.items() if not k.startswith("roi_heads.keypoint_")})
    # what is left is FasterRCNN's to judge, after the split
    with pytest.raises(pkg.WinoError, match="unexpected key 'keypoint_head.0.weight' for Faster R-CNN"):
        make(dict(sd, **{"keypoint_head.0.weight": torch.zeros(1)}))
    assert {"KeypointHead", "KeypointRCNN", "pack_kps_deconv", "split_keypoint_state_dict", "expected_keypoint_head_keys",
            "validate_keypoint_head_state_dict"} <= set(det.__all__)
