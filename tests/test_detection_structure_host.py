"""Host-side checks of how the R-CNN detectors are put together -- no GPU needed: MaskRCNN and KeypointRCNN inherit
FasterRCNN's one prepare / forward / predict / to_lists / to_image_lists, the two state-dict splitters are one function, and
to_lists / to_image_lists on a hand-made CPU dict give torchvision's per-image lists for every set of output keys."""
import importlib

import pytest
import torch

N, D, K, H, W = 2, 3, 2, 5, 6
COUNT, SIZES = [2, 0], [(4, 6), (5, 3)]
ONE_PATH = ("prepare", "forward", "predict", "to_lists", "to_image_lists")


def test_the_detectors_define_no_path_of_their_own(pkg):
    for cls in (pkg.MaskRCNN, pkg.KeypointRCNN):
        assert issubclass(cls, pkg.FasterRCNN)
        assert not set(ONE_PATH + ("_prepare_outputs", "_prepare_for_predict")) & set(cls.__dict__), cls
        assert "from_state_dict" in cls.__dict__
        for name in ONE_PATH:
            assert getattr(cls, name) is getattr(pkg.FasterRCNN, name), (cls, name)


def test_the_splitters_are_one_function(pkg):
    det = importlib.import_module("cuda_winograd_amd.detection")
    sd = {"roi_heads.mask_head.0.0.bias": 1, "roi_heads.mask_predictor.x": 2, "roi_heads.keypoint_head.0.bias": 3,
          "roi_heads.keypoint_predictor.y": 4, "roi_heads.box_head.fc6.bias": 5, "backbone.body.conv1.weight": 6}
    rest, mask = det.split_mask_state_dict(sd)
    assert mask == {"mask_head.0.0.bias": 1, "mask_predictor.x": 2} and sorted(rest) == sorted(set(sd) - {
        "roi_heads.mask_head.0.0.bias", "roi_heads.mask_predictor.x"})
    rest, kp = det.split_keypoint_state_dict(sd)
    assert kp == {"keypoint_head.0.bias": 3, "keypoint_predictor.y": 4} and len(rest) == 4
    assert det._split_state_dict(sd, det.MASK_PREFIXES + det.KEYPOINT_PREFIXES)[0] == {
        "roi_heads.box_head.fc6.bias": 5, "backbone.body.conv1.weight": 6}


def result(keys):
    g = torch.Generator().manual_seed(5)
    full = {"boxes": torch.rand(N, D, 4, generator=g), "scores": torch.rand(N, D, generator=g),
            "labels": torch.randint(1, 5, (N, D), generator=g), "count": torch.tensor(COUNT, dtype=torch.int32),
            "overflow": torch.zeros(N, dtype=torch.bool), "masks": torch.rand(N, D, H, W, generator=g),
            "masks_binary": torch.randint(0, 2, (N, D, H, W), generator=g).to(torch.uint8),
            "keypoints": torch.rand(N, D, K, 3, generator=g), "keypoints_scores": torch.rand(N, D, K, generator=g),
            "original_sizes": list(SIZES)}
    return {k: v for k, v in full.items() if k in keys}


DET = ("boxes", "scores", "labels", "count", "overflow", "original_sizes")
MASKS, KEYPOINTS = ("masks", "masks_binary"), ("keypoints", "keypoints_scores")


@pytest.mark.parametrize("extra", [(), MASKS, ("masks",), KEYPOINTS, MASKS + KEYPOINTS], ids=lambda e: "+".join(e) or "faster")
def test_to_lists_and_to_image_lists(pkg, extra):
    out = result(DET + extra)
    kept = {k: v.clone() for k, v in out.items() if isinstance(v, torch.Tensor)}
    listed = ("boxes", "scores", "labels") + extra
    for cls in (pkg.FasterRCNN, pkg.MaskRCNN, pkg.KeypointRCNN):
        for crop, lists in ((False, cls.to_lists(out)), (True, cls.to_image_lists(out))):
            assert len(lists) == N
            for n, (c, (h, w), d) in enumerate(zip(COUNT, SIZES, lists)):
                assert tuple(d) == listed                      # these keys, in torchvision's order, and no others
                for k in listed:
                    want = out[k][n, :c]
                    if k in MASKS:
                        want = want[:, None, :h, :w] if crop else want[:, None]
                    assert d[k].dtype == out[k].dtype and d[k].shape == want.shape and torch.equal(d[k], want), (k, n, crop)
                    assert d[k].is_contiguous()
                    # a clone, not a view: it shares no memory with the model's tensor
                    lo, hi = out[k].data_ptr(), out[k].data_ptr() + out[k].numel() * out[k].element_size()
                    assert d[k].numel() == 0 or not lo <= d[k].data_ptr() < hi, (k, n, crop)
            # the exact shapes, spelled out: image 0 keeps 2 detections, image 1 none
            h0, w0 = (SIZES[0] if crop else (H, W))
            h1, w1 = (SIZES[1] if crop else (H, W))
            assert [tuple(d["boxes"].shape) for d in lists] == [(2, 4), (0, 4)]
            assert [tuple(d["labels"].shape) for d in lists] == [(2,), (0,)] and lists[0]["labels"].dtype == torch.int64
            for k in set(MASKS) & set(extra):
                assert [tuple(d[k].shape) for d in lists] == [(2, 1, h0, w0), (0, 1, h1, w1)]
            if extra[-2:] == KEYPOINTS:
                assert [tuple(d["keypoints"].shape) for d in lists] == [(2, K, 3), (0, K, 3)]
                assert [tuple(d["keypoints_scores"].shape) for d in lists] == [(2, K), (0, K)]
            if "masks_binary" in extra:
                assert lists[0]["masks_binary"].dtype == torch.uint8 and lists[0]["masks"].dtype == torch.float32
    # writing into a result leaves the model's tensors as they were
    for d in pkg.MaskRCNN.to_image_lists(out) + pkg.FasterRCNN.to_lists(out):
        for v in d.values():
            v.zero_()
    for k, v in kept.items():
        assert torch.equal(out[k], v), k


def test_a_model_object_calls_them_too(pkg):
    """m.to_lists(out): the static methods are reachable through an instance, which is how the GPU tests call them."""
    m = object.__new__(pkg.KeypointRCNN)
    out = result(DET + KEYPOINTS)
    assert [tuple(d["keypoints"].shape) for d in m.to_lists(out)] == [(2, K, 3), (0, K, 3)]
    assert [tuple(d["boxes"].shape) for d in m.to_image_lists(out)] == [(2, 4), (0, 4)]


def test_the_earlier_buffer_names_read_through_to_their_owner(pkg):
    """m._mask_pooled, m._masks, m._masks_bin, m._kp_pooled and head._a / head._b are read-only views of what the branch
    and the conv tower own: nothing is stored on the model under these names."""
    class Branch:
        pooled, _masks, _masks_bin = "pooled", "planes", None
    for cls, names in ((pkg.MaskRCNN, ("_mask_pooled", "_masks", "_masks_bin")), (pkg.KeypointRCNN, ("_kp_pooled",))):
        m = object.__new__(cls)
        m.branches = [Branch()]
        assert [getattr(m, n) for n in names] == ["pooled", "planes", None][:len(names)]
        assert not set(names) & set(vars(m))
        with pytest.raises(AttributeError):
            setattr(m, names[0], 1)
    head = object.__new__(pkg.MaskHead)
    head._acts = ["a", "b", "a", "b"]
    assert (head._a, head._b) == ("a", "b")
