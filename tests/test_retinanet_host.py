"""Host tests of RetinaNet's parts (no GPU): the head's key validation in both spellings, the base anchors of
torchvision's RetinaNet sizes against a transcription of its generator, the backbone's keys with returned_layers and
P6 / P7, select_topk_map's workspace formula against the header and its refusals (a segment longer than 2^31 - 1 among
them), retina_decode's refusals, and the logit threshold's defining property."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import retina_cases as rc
import retinanet_reference as rr

SHAPE, ARG = -2, -3


@pytest.fixture(scope="module")
def D(pkg):
    return importlib.import_module("cuda_winograd_amd.detection")


@pytest.fixture(scope="module")
def FPN(pkg):
    return importlib.import_module("cuda_winograd_amd.fpn")


# ---- state dicts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("legacy", [False, True], ids=["conv.i.0", "legacy conv.2i"])
def test_head_keys_validate_in_both_spellings(legacy, pkg, D):
    sd = rr.head_state_dict(64, 9, 5, seed=1, legacy=legacy)
    assert D.validate_retinanet_head_state_dict(sd, 64, 9) == 5
    exp = D.expected_retinanet_head_keys(sd, 64, 9, 5)
    assert set(exp) == set(sd) and len(exp) == 20
    stem = "classification_head.conv.6" if legacy else "classification_head.conv.3.0"
    assert exp[f"{stem}.weight"] == (64, 64, 3, 3) and exp["classification_head.cls_logits.weight"] == (45, 64, 3, 3)
    assert exp["regression_head.bbox_reg.weight"] == (36, 64, 3, 3) and exp["regression_head.bbox_reg.bias"] == (36,)
    # the first wrong key is named: missing, unexpected, wrongly shaped
    missing = {k: v for k, v in sd.items() if k != f"{stem}.bias"}
    with pytest.raises(pkg.WinoError, match=re.escape(f"missing key '{stem}.bias' for the RetinaNet head")):
        D.validate_retinanet_head_state_dict(missing, 64, 9)
    with pytest.raises(pkg.WinoError, match="unexpected key 'regression_head.bbox_ctrness.weight'"):
        D.validate_retinanet_head_state_dict(dict(sd, **{"regression_head.bbox_ctrness.weight": torch.zeros(1)}), 64, 9)
    bad = dict(sd, **{"regression_head.bbox_reg.weight": torch.zeros(32, 64, 3, 3)})
    with pytest.raises(pkg.WinoError, match=r"'regression_head.bbox_reg.weight' has shape \(32, 64, 3, 3\).*\(36, 64, 3, 3\)"):
        D.validate_retinanet_head_state_dict(bad, 64, 9)
    with pytest.raises(pkg.WinoError, match="missing key 'classification_head.cls_logits.weight'"):
        D.validate_retinanet_head_state_dict({}, 64, 9)
    with pytest.raises(pkg.WinoError, match="46 channels for A=9"):
        D.validate_retinanet_head_state_dict(dict(sd, **{"classification_head.cls_logits.weight": torch.zeros(46, 64, 3, 3)}), 64, 9)
    with pytest.raises(pkg.WinoError, match="multiple of 64"):
        D.validate_retinanet_head_state_dict(rr.head_state_dict(96, 9, 5), 96, 9)
    # the two spellings do not mix inside a tower
    mixed = dict(sd)
    old, new = ("classification_head.conv.2", "classification_head.conv.1.0") if legacy else \
        ("classification_head.conv.1.0", "classification_head.conv.2")
    for part in ("weight", "bias"):
        mixed[f"{new}.{part}"] = mixed.pop(f"{old}.{part}")
    with pytest.raises(pkg.WinoError, match="state dict"):
        D.validate_retinanet_head_state_dict(mixed, 64, 9)


def test_last_convolution_is_zero_padded_to_64(D):
    w, b = torch.randn(819, 8, 3, 3), torch.randn(819)
    wp, bp = D.pack_retina_last(w, b)
    assert tuple(wp.shape) == (832, 8, 3, 3) and tuple(bp.shape) == (832,)
    assert torch.equal(wp[:819], w) and torch.equal(bp[:819], b) and not wp[819:].any() and not bp[819:].any()
    assert D.pack_retina_last(torch.randn(36, 8, 3, 3), torch.randn(36))[0].shape[0] == 64
    assert D.pack_retina_last(torch.randn(64, 8, 3, 3), torch.randn(64))[0].shape[0] == 64


def test_detector_refuses_bad_arguments_on_the_host(pkg, D):
    for bad in (0.0, 1.0, -0.5, float("nan")):
        with pytest.raises(pkg.WinoError, match="score_thresh"):
            D.RetinaNet.from_state_dict({}, "resnet18", score_thresh=bad)
    with pytest.raises(pkg.WinoError, match="topk_candidates=1639"):
        D.RetinaNet.from_state_dict({}, "resnet18", topk_candidates=1639)        # five levels of it pass 8192 rows
    with pytest.raises(pkg.WinoError, match="5 levels need 5 size tuples"):
        D.RetinaNet.from_state_dict({}, "resnet18", sizes=((32,),) * 4)
    with pytest.raises(pkg.WinoError, match="unexpected key 'rpn.head.conv.weight' for RetinaNet"):
        D.RetinaNet.from_state_dict({"rpn.head.conv.weight": torch.zeros(1)}, "resnet18")
    with pytest.raises(pkg.WinoError, match="missing key 'classification_head.cls_logits.weight'"):
        D.RetinaNet.from_state_dict({}, "resnet18")
    assert issubclass(D.RetinaNet, D._Detector) and issubclass(D.FasterRCNN, D._Detector)
    for name in ("prepare_images", "predict", "to_lists", "to_image_lists", "forward", "prepare"):      # shared, not copied
        assert name not in vars(D.RetinaNet) and name not in vars(D.FasterRCNN) and name in vars(D._Detector), name


# ---- anchors ------------------------------------------------------------------------------------------------------------------
def test_base_anchors_of_the_retinanet_sizes(D):
    assert D.RETINA_SIZES == rc.RETINA_SIZES == ((32, 40, 50), (64, 80, 101), (128, 161, 203), (256, 322, 406), (512, 645, 812))
    for sizes in rc.RETINA_SIZES:
        got = D.base_anchors(sizes, rc.RETINA_RATIOS).numpy()
        want = rc.torchvision_base_anchors(sizes, rc.RETINA_RATIOS)
        assert got.shape == (9, 4) and np.array_equal(got.view(np.int32), want.view(np.int32)), sizes
        assert np.array_equal(got[:, :2], -got[:, 2:])
    first = D.base_anchors(rc.RETINA_SIZES[0], rc.RETINA_RATIOS).numpy()
    # ratio-major: (ratio 0.5: 32, 40, 50), (1: ...), (2: ...); 32 / sqrt(0.5) / 2 = 22.63, 32 sqrt(0.5) / 2 = 11.31
    assert first[0].tolist() == [-23.0, -11.0, 23.0, 11.0] and first[3].tolist() == [-16.0, -16.0, 16.0, 16.0]
    assert first[8].tolist() == [-18.0, -35.0, 18.0, 35.0]


# ---- the backbone's keys --------------------------------------------------------------------------------------------------------
def test_fpn_keys_with_returned_layers_and_p6p7(pkg, FPN):
    default = FPN.expected_fpn_keys("resnet50", 256)
    assert default == FPN.expected_fpn_keys("resnet50", 256, (1, 2, 3, 4), "pool")
    assert sum(k.startswith("fpn.") for k in default) == 16 and not any("extra_blocks" in k for k in default)
    assert default["fpn.inner_blocks.0.0.weight"] == (256, 256, 1, 1) and default["fpn.inner_blocks.3.0.weight"] == (256, 2048, 1, 1)
    exp = FPN.expected_fpn_keys("resnet50", 256, (2, 3, 4), "p6p7")
    fpn = {k: v for k, v in exp.items() if k.startswith("fpn.")}
    assert {k: v for k, v in exp.items() if k.startswith("body.")} == {k: v for k, v in default.items() if k.startswith("body.")}
    assert len(fpn) == 16 and [fpn[f"fpn.inner_blocks.{i}.0.weight"][1] for i in range(3)] == [512, 1024, 2048]
    assert "fpn.inner_blocks.3.0.weight" not in fpn and "fpn.layer_blocks.2.0.bias" in fpn
    for name in ("p6", "p7"):
        assert fpn[f"fpn.extra_blocks.{name}.weight"] == (256, 256, 3, 3) and fpn[f"fpn.extra_blocks.{name}.bias"] == (256,)
    assert [FPN.expected_fpn_keys("resnet18", 64, (2, 3, 4), "p6p7")[f"fpn.inner_blocks.{i}.0.weight"][1] for i in range(3)] == [128, 256, 512]
    sd = {k: torch.zeros(v) for k, v in exp.items()}
    FPN.validate_fpn_state_dict(sd, "resnet50", 256, (2, 3, 4), "p6p7")
    with pytest.raises(pkg.WinoError, match="unexpected key 'fpn.extra_blocks.p6.weight'"):
        FPN.validate_fpn_state_dict(sd, "resnet50", 256, (2, 3, 4))
    with pytest.raises(pkg.WinoError, match="missing key 'fpn.extra_blocks.p7.bias'"):
        FPN.validate_fpn_state_dict({k: v for k, v in sd.items() if k != "fpn.extra_blocks.p7.bias"}, "resnet50", 256,
                                    (2, 3, 4), "p6p7")
    for bad in ((), (0, 1), (2, 4), (3, 2), (3, 4, 5)):
        with pytest.raises(pkg.WinoError, match="returned_layers"):
            FPN.expected_fpn_keys("resnet50", 256, bad, "p6p7")
    with pytest.raises(pkg.WinoError, match="extra_blocks"):
        FPN.expected_fpn_keys("resnet50", 256, (2, 3, 4), "p6")


# ---- select_topk_map: the workspace and the refusals ---------------------------------------------------------------------------
def _map(pkg, map_=0x40000000, N=2, h=13, w=21, cols=45, ld=64, k=100, use_thresh=0, thresh=0.0, idx=0x100000, vals=0x200000,
         count=0x300000, out_stride=None, out_offset=0, ws=None, ws_bytes=0):
    out_stride = out_offset + k if out_stride is None else out_stride
    return pkg.lib().wino_select_topk_map_hw(map_, N, h, w, cols, ld, k, use_thresh, thresh, idx, vals, count, out_stride,
                                             out_offset, ws, ws_bytes, None)


def _header_formula(N, n, k):
    """winograd_mi355x.h: three histograms of 2048 words and four words of list length per long segment, one word per
    chunk of 2048 scores, k 64-bit keys, each term rounded up to 16 bytes; 0 when n <= 8192."""
    if n <= 8192:
        return 0
    r16 = lambda b: (b + 15) // 16 * 16
    return r16(N * 6148 * 4) + r16(N * -(-n // 2048) * 4) + r16(N * k * 8)


def test_map_workspace_is_the_headers_formula(pkg):
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "winograd_mi355x.h")).read()
    assert "N * |L| * 6148 * 4" in text and "ceil(n[p] / 2048) * 4" in text and "sum_L k[p] * 8" in text
    L = pkg.lib()
    for N, h, w, cols, k in [(1, 1, 1, 1, 1), (2, 13, 21, 45, 1000), (3, 13, 21, 819, 1000), (2, 100, 168, 819, 1000),
                             (1, 1, 1, 8192, 8192), (1, 1, 1, 8193, 1), (2, 7, 1171, 1, 17), (65535, 1, 3, 3000, 2)]:
        n = h * w * cols
        want = _header_formula(N, n, k)
        assert pkg.select_map_workspace_bytes(N, h, w, cols, k) == want
        assert want == pkg.select_workspace_bytes(N, n, k)
        if want and N <= 3:           # one byte less is refused; the figure itself gets as far as the overlap check
            kw = dict(N=N, h=h, w=w, cols=cols, ld=rc.pad64(cols), k=k, ws=0x10000000)
            assert _map(pkg, ws_bytes=want - 1, **kw) == ARG
            assert f"workspace too small: need {want} bytes" in L.wino_last_error_string().decode()
            assert _map(pkg, ws_bytes=want, idx=0x40000000, **kw) == ARG
            assert "must not overlap" in L.wino_last_error_string().decode()
    for bad in ((2, 0, 5, 5, 5), (2, 5, 5, 5, 8193), (2, 5, 5, 0, 5), (-1, 5, 5, 5, 5)):
        with pytest.raises(pkg.WinoError, match="unsupported shape"):
            pkg.select_map_workspace_bytes(*bad)


def test_map_refuses_a_segment_longer_than_int32(pkg):
    """n = h w cols <= 2^31 - 1: beyond it the entry point and the query refuse, with a message that says why."""
    L = pkg.lib()
    assert _map(pkg, N=1, h=32768, w=65536, cols=1, ld=64, k=1) == SHAPE                       # n = 2^31
    assert "longer than 2^31 - 1" in L.wino_last_error_string().decode()
    assert _map(pkg, N=1, h=46341, w=46341, cols=1, ld=64, k=1) == SHAPE                       # 46341^2 = 2^31 + 88 k
    assert "longer than 2^31 - 1" in L.wino_last_error_string().decode()
    assert _map(pkg, N=1, h=1000, w=2700, cols=819, ld=832, k=1) == SHAPE                      # 2.2e9 through cols
    assert "longer than 2^31 - 1" in L.wino_last_error_string().decode()
    with pytest.raises(pkg.WinoError, match="longer than 2\\^31 - 1"):
        pkg.select_map_workspace_bytes(1, 32768, 65536, 1, 1)
    # 2^31 - 1 itself (a prime: one column of pixels) passes the length check; what is refused next is the NULL workspace
    top = (1 << 31) - 1
    assert pkg.select_map_workspace_bytes(1, top, 1, 1, 1) == _header_formula(1, top, 1)
    assert _map(pkg, N=1, h=top, w=1, cols=1, ld=1, k=1) == ARG
    assert "workspace too small" in L.wino_last_error_string().decode()


def test_map_refuses_bad_shapes_and_arguments_before_any_launch(pkg):
    L = pkg.lib()
    bad = [dict(N=-1), dict(N=65536), dict(h=0), dict(w=0), dict(cols=0), dict(cols=65), dict(k=0), dict(k=8193),
           dict(out_offset=-1), dict(out_offset=5, out_stride=104), dict(out_stride=1 << 31), dict(w=(1 << 26), ld=64, cols=1, h=1)]
    for kw in bad:
        assert _map(pkg, **kw) == SHAPE, kw
        assert "select_topk_map: unsupported shape" in L.wino_last_error_string().decode(), kw
    need = pkg.select_map_workspace_bytes(2, 13, 21, 45, 100)
    assert need > 0
    ws = dict(ws=0x10000000, ws_bytes=need)
    short = dict(h=3, w=5)                                           # n = 675: no workspace
    bad = [dict(ws, map_=None), dict(ws, idx=None), dict(ws, count=None), dict(ws, map_=0x40000004), dict(ws, idx=0x100008),
           dict(ws, vals=0x200004), dict(ws, count=0x300002), dict(ws, use_thresh=1, thresh=float("nan")),
           dict(ws=None, ws_bytes=need), dict(ws=0x10000000, ws_bytes=need - 1), dict(ws=0x10000004, ws_bytes=need),
           dict(short, idx=0x40000000), dict(short, vals=0x40000000 + 64), dict(short, count=0x40000000 + 128),
           dict(short, idx=0x200000 + 32), dict(short, count=0x100000 + 64), dict(ws, map_=0x10000000 - 4096)]
    for kw in bad:
        assert _map(pkg, **kw) == ARG, kw
    assert _map(pkg, N=0, map_=None, idx=None, vals=None, count=None) == 0       # nothing to do: no pointer is looked at
    # a slice of a wider buffer overlaps by its own rows only: idx at out_offset behind vals' end is no clash
    assert _map(pkg, **short, out_offset=4, out_stride=200, idx=0x200000 + 2 * 200 * 4 - 16, count=0x40000000) == ARG
    assert "must not overlap" in L.wino_last_error_string().decode()


# ---- retina_decode: the refusals ------------------------------------------------------------------------------------------------
def _decode(pkg, idx=0x100000, N=2, k=100, stride=None, offset=0, reg=0x40000000, h=13, w=21, ld=64, A=9, K=91, base=0x200000,
            sy=8, sx=8, hw=0x300000, clamp=4.135, boxes=0x400000, labels=0x500000):
    stride = offset + k if stride is None else stride
    return pkg.lib().wino_retina_decode_hw(idx, N, k, stride, offset, reg, h, w, ld, A, K, base, sy, sx, hw, clamp, boxes,
                                           labels, None)


def test_decode_refuses_before_any_launch(pkg):
    L = pkg.lib()
    bad = [dict(N=-1), dict(k=-1), dict(h=0), dict(w=0), dict(A=0), dict(K=0), dict(ld=35), dict(ld=0), dict(sy=0), dict(sx=0),
           dict(offset=-1), dict(offset=5, stride=104), dict(h=46341, w=46341, A=1, K=1, ld=4),
           dict(h=4096, w=4096, A=9, K=91), dict(N=1 << 20, k=1 << 11), dict(h=1, w=1 << 26, A=1, K=1)]
    for kw in bad:
        assert _decode(pkg, **kw) == SHAPE, kw
        assert "retina_decode: unsupported shape" in L.wino_last_error_string().decode(), kw
    bad = [dict(idx=None), dict(reg=None), dict(base=None), dict(hw=None), dict(boxes=None), dict(labels=None),
           dict(idx=0x100004), dict(reg=0x40000008), dict(base=0x200004), dict(hw=0x300008), dict(boxes=0x400004),
           dict(labels=0x500002), dict(clamp=float("nan")), dict(boxes=0x100000), dict(labels=0x100000 + 64),
           dict(labels=0x400000 + 160), dict(boxes=0x40000000 + 4096), dict(labels=0x200000), dict(boxes=0x300000)]
    for kw in bad:
        assert _decode(pkg, **kw) == ARG, kw
    assert _decode(pkg, N=0, idx=None, reg=None, boxes=None, labels=None) == 0
    assert _decode(pkg, k=0, idx=None, reg=None, boxes=None, labels=None) == 0


# ---- the logit threshold ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [0.05, 0.5, 0.3, 0.01, 0.95, 1e-6, 0.999])
def test_logit_threshold_is_the_fp32_successor(s, D):
    """t is an fp32 number with sigmoid(t) > s >= sigmoid(pred(t)) in fp64: `logit >= t` is `sigmoid(logit) > s`."""
    t = D.logit_threshold(s)
    at, below = rr.logit_threshold_bounds(t, s)
    assert at > s >= below, (s, t, at, below)
    if s == 0.5:
        assert 0 < t < 1e-15                          # sigmoid(0) = 0.5 is not > 0.5; fp64 tells 0.5 + t / 4 from 0.5 at 2^-51
    if s == 0.05:
        assert abs(t - np.log(0.05 / 0.95)) < 3e-7 and t < 0


def test_reference_select_is_torchs_topk_on_the_thresholded_scores():
    """level_select_reference against the literal torchvision lines, in torch fp64, on logits without ties."""
    rng = np.random.RandomState(5)
    logits = rng.standard_normal((2, 500)) * 2 - 2
    idx, count, thresh_margin, tie_gap = rr.level_select_reference(logits, 40, 0.05)
    assert thresh_margin > 0 and tie_gap > 0
    for i in range(2):
        scores = torch.sigmoid(torch.from_numpy(logits[i])).flatten()
        keep = scores > 0.05
        topk_idxs = torch.where(keep)[0]
        num_topk = min(40, int(topk_idxs.numel()))
        _, pos = scores[keep].topk(num_topk)
        assert count[i] == num_topk and np.array_equal(idx[i, :num_topk], topk_idxs[pos].numpy())
