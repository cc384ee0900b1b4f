"""GPU tests of FasterRCNN / MaskRCNN.predict on the seeded detector of box_cases.DETECTOR (resnet18, 64 channels) with
roi_cases.mask_head_state_dict under roi_heads., for both `select` values: two images, 40 x 60 and 50 x 45, at min_size 64,
max_size 96 resize to 64 x 96 and 71 x 64 in a 96 x 96 batch.  The detector's accuracy against fp64 is pinned by the
existing suites and the transform's by tests/test_gpu_transform.py, so these are exact comparisons: predict against the
composition from public pieces (image_transform, forward, the fp32 multiply by the ratios restated in numpy, paste_masks),
bit for bit.  Last, on the mask model and on a keypoint model (keypoint_P = 4, K = 3): a first forward prepares the model and
the branch's head exactly once each, and a branch head that refuses to prepare leaves the model unprepared."""
import numpy as np
import pytest
import torch

import box_cases as bc
import keypoint_cases as kc
import roi_cases as rc
import transform_cases as tc
from gpu_support import R, same_bits, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu
D = bc.DETECTOR
MASK_P = 14
SHAPES, SIZES, BATCH = [(40, 60), (50, 45)], [(64, 96), (71, 64)], (96, 96)
OTHER = [(40, 60), (44, 52)]
MIN_MAX = dict(min_size=64, max_size=96)
DET_KEYS = ("boxes", "scores", "labels", "count", "overflow")
MASK_KEYS = ("masks", "masks_binary")


def kwargs(dev, **more):
    return dict(num_classes=D["classes"], out_channels=D["out_channels"], P=D["P"], rpn_pre_nms_top_n=D["pre"],
                rpn_post_nms_top_n=D["post"], box_detections_per_img=D["detections"], device=dev, **more)


def build(pkg, R, dev, cls, select):
    sd, _, _ = bc.detector_state_dict(R)
    if cls == "mask":
        full = dict(sd)
        full.update({"roi_heads." + k: v for k, v in rc.mask_head_state_dict(D["out_channels"], D["classes"],
                                                                             seed=D["seed"] + 2).items()})
        return pkg.MaskRCNN.from_state_dict(full, D["arch"], mask_P=MASK_P, masks="both", **kwargs(dev, select=select))
    return pkg.FasterRCNN.from_state_dict(sd, D["arch"], **kwargs(dev, select=select))


@pytest.fixture(scope="module", params=[("faster", "torch"), ("faster", "kernel"), ("mask", "torch"), ("mask", "kernel")],
                ids=lambda p: "-".join(p))
def model(request, pkg, R, torch_dev):
    return build(pkg, R, torch_dev[1], *request.param), request.param[0] == "mask"


def images(dev, shapes=SHAPES, dtype=torch.float32):
    return [t.to(dev) for t in tc.images(shapes, 3, dtype, seed=21)]


def composition(pkg, m, is_mask, imgs, shapes):
    """predict from public pieces, on a model prepared for these images: (the expected dict, cloned; the ratios)."""
    sizes = [pkg.transform_size(h, w, **MIN_MAX) for h, w in shapes]
    Hb, Wb = pkg.batch_hw(sizes)
    batch = pkg.image_transform(imgs, sizes, Hb, Wb, pkg.IMAGENET_MEAN, pkg.IMAGENET_STD)
    hw = torch.tensor(sizes, dtype=torch.float32, device=batch.device)
    want = {k: v.clone() for k, v in m(batch, hw).items()}
    ratio = np.array([[np.float32(w) / np.float32(wo), np.float32(h) / np.float32(ho)] * 2
                      for (h, w), (ho, wo) in zip(shapes, sizes)], dtype=np.float32)
    boxes = want["boxes"].cpu().numpy() * ratio[:, None, :]
    assert boxes.dtype == np.float32
    want["boxes"] = torch.from_numpy(boxes)
    if is_mask:
        Hmax, Wmax = max(h for h, _ in shapes), max(w for _, w in shapes)
        orig = torch.tensor(shapes, dtype=torch.float32, device=batch.device)
        prob, binary = pkg.paste_masks(m.mask_head._scores, want["labels"].to(torch.int32), want["boxes"].to(batch.device), orig,
                                       Hmax, Wmax, M=2 * MASK_P, classes=D["classes"], layout="gemm_rows", want_binary=True,
                                       threshold=m.mask_threshold)
        want["masks"], want["masks_binary"] = prob.clone(), binary.clone()
    torch.cuda.synchronize()
    return want, sizes, (Hb, Wb)


def check_against_composition(pkg, m, is_mask, imgs, shapes):
    m.prepare_images(shapes, **MIN_MAX)
    want, sizes, batch = composition(pkg, m, is_mask, imgs, shapes)
    got = m.predict(imgs)
    torch.cuda.synchronize()
    assert m._tf["shape"] == (len(shapes), *batch) and m._tf["sizes"] == sizes
    assert got["original_sizes"] == list(shapes)
    for k in DET_KEYS + (MASK_KEYS if is_mask else ()):
        assert same_bits(got[k], want[k]), k
    count = got["count"].cpu().tolist()
    print(f"detections {count}")
    assert sum(count) > 0
    # every kept box lies inside its own image up to one fp32 rounding of the product: a coordinate is clipped to at
    # most wo, the ratio fl(w / wo) is within 2^-24 of w / wo, so fl(x * ratio) is at most the float32 after w
    boxes = got["boxes"].cpu().numpy()
    for n, (h, w) in enumerate(shapes):
        b = boxes[n, :count[n]]
        w1, h1 = (np.nextafter(np.float32(v), np.float32(np.inf)) for v in (w, h))
        assert (b >= 0).all() and (b[:, [0, 2]] <= w1).all() and (b[:, [1, 3]] <= h1).all(), (n, b)
        assert (boxes[n, count[n]:] == 0).all()
    return got


def test_predict_is_the_composition_from_public_pieces(pkg, model, torch_dev):
    m, is_mask = model
    assert [pkg.transform_size(h, w, **MIN_MAX) for h, w in SHAPES] == SIZES and pkg.batch_hw(SIZES) == BATCH
    imgs = images(torch_dev[1])
    got = check_against_composition(pkg, m, is_mask, imgs, SHAPES)
    if not is_mask:
        assert not set(MASK_KEYS) & set(got)
        lists = m.to_image_lists(got)
        assert [tuple(d["boxes"].shape) for d in lists] == [(c, 4) for c in got["count"].tolist()]
        return
    Dn, count = D["detections"], got["count"].cpu().tolist()
    masks, binary = got["masks"].cpu(), got["masks_binary"].cpu()
    assert tuple(masks.shape) == tuple(binary.shape) == (2, Dn, 50, 60) and binary.dtype == torch.uint8
    for n, (h, w) in enumerate(SHAPES):
        for t in (masks, binary):
            assert bool((t[n, :, h:] == 0).all()) and bool((t[n, :, :, w:] == 0).all()) and bool((t[n, count[n]:] == 0).all())
        assert all(bool((masks[n, d] > 0).any()) for d in range(count[n]))
    assert torch.equal(binary, (masks > m.mask_threshold).to(torch.uint8))
    lists = m.to_image_lists(got)
    for n, ((h, w), d) in enumerate(zip(SHAPES, lists)):
        c = count[n]
        assert tuple(d["boxes"].shape) == (c, 4) and tuple(d["masks"].shape) == tuple(d["masks_binary"].shape) == (c, 1, h, w)
        assert same_bits(d["masks"][:, 0], got["masks"][n, :c, :h, :w]) and same_bits(d["boxes"], got["boxes"][n, :c])


def test_uint8_images(pkg, model, torch_dev):
    m, is_mask = model
    imgs = images(torch_dev[1], dtype=torch.uint8)
    m.prepare_images(SHAPES, dtype=torch.uint8, **MIN_MAX)
    want = composition(pkg, m, is_mask, imgs, SHAPES)[0]
    got = m.predict(imgs)
    torch.cuda.synchronize()
    assert m._tf["key"][1] == torch.uint8
    for k in DET_KEYS + (MASK_KEYS if is_mask else ()):
        assert same_bits(got[k], want[k]), k


def test_a_list_of_other_shapes_re_prepares(pkg, model, torch_dev):
    m, is_mask = model
    dev = torch_dev[1]
    m.prepare_images(SHAPES, **MIN_MAX)
    m.predict(images(dev))
    first = m._tf
    imgs = images(dev, OTHER)
    got = m.predict(imgs)                    # new shapes: prepare_images again, with the parameters of the last one
    torch.cuda.synchronize()
    assert m._tf is not first and m._tf["key"] == (tuple(OTHER), torch.float32) and m._tf["params"] == first["params"]
    assert m._tf["params"]["min_size"] == 64 and got["original_sizes"] == OTHER
    kept = {k: got[k].clone() for k in DET_KEYS + (MASK_KEYS if is_mask else ())}
    want = composition(pkg, m, is_mask, imgs, OTHER)[0]
    for k, v in kept.items():
        assert same_bits(v, want[k]), k
    if is_mask:
        assert tuple(kept["masks"].shape) == (2, D["detections"], 44, 60)
    # the same list again does not
    again = m._tf
    m.predict(imgs)
    assert m._tf is again


def test_predict_from_one_graph_replays_bitwise(pkg, model, torch_dev):
    """prepare_images, then the whole predict captured into one graph -- a host read of device data inside it would fail
    the capture -- replays bitwise equal to eager into NaN-filled buffers, and no ticket stays held."""
    m, is_mask = model
    imgs = images(torch_dev[1])
    keys = DET_KEYS + (MASK_KEYS if is_mask else ())
    torch.cuda.synchronize()
    sg = torch.cuda.Stream()
    with torch.cuda.stream(sg):
        m.prepare_images(SHAPES, **MIN_MAX)
        eager = {k: v.clone() for k, v in m.predict(imgs).items() if k in keys}
    sg.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=sg):
        out = m.predict(imgs)
    for _ in range(2):
        for k in ("boxes", "scores") + (("masks",) if is_mask else ()):
            out[k].fill_(float("nan"))
        if is_mask:
            out["masks_binary"].fill_(255)
        for t in (m._tf["batch"], m.rpn._rois, m._pooled, m.box_head._scores):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for k in keys:
            assert same_bits(out[k], eager[k]), k
    with torch.cuda.stream(sg):
        assert pkg.tickets_in_use() == 0
    del graph


def test_forward_is_what_it_was_before_any_predict(pkg, R, torch_dev):
    """forward on a ready batch, on a model that has never run predict, against the same forward after a predict."""
    dev = torch_dev[1]
    x = bc.detector_input().to(dev)
    for cls in ("faster", "mask"):
        m = build(pkg, R, dev, cls, "torch")
        assert m._tf is None
        before = {k: v.clone() for k, v in m(x).items()}
        with pytest.raises(pkg.WinoError, match="shapes must be"):
            m.prepare_images([(40,)], **MIN_MAX)
        with pytest.raises(pkg.WinoError, match="rc=-2"):
            m.prepare_images([(1, 2000)], min_size=1, max_size=1)     # resizes to nothing: refused, parameters kept
        assert m._tf is None and m._tf_params["max_size"] == 1
        m.prepare_images(SHAPES, **MIN_MAX)
        m.predict(images(dev))
        if cls == "mask":                                              # predict needs none of forward's batch-size planes
            assert m._masks is None and m._masks_bin is None and tuple(m._tf["masks"].shape) == (2, D["detections"], 50, 60)
        after = m(x)
        torch.cuda.synchronize()
        assert set(after) == set(before) and "original_sizes" not in after
        for k in before:
            assert same_bits(after[k], before[k]), (cls, k)
        assert int(before["count"].min()) > 0
        if cls == "mask":
            assert tuple(after["masks"].shape) == (D["N"], D["detections"], D["H"], D["W"])


# ---- prepare, with a branch --------------------------------------------------------------------------------------------
def branch_model(pkg, R, dev, cls):
    """(a model that has never been prepared, its branch's head)."""
    if cls == "mask":
        m = build(pkg, R, dev, "mask", "torch")
        return m, m.mask_head
    full = dict(bc.detector_state_dict(R)[0])
    full.update({"roi_heads." + k: v for k, v in kc.keypoint_head_state_dict(D["out_channels"], [64] * 8, 3,
                                                                             seed=D["seed"] + 3).items()})
    m = pkg.KeypointRCNN.from_state_dict(full, D["arch"], keypoint_P=4, **kwargs(dev))
    return m, m.keypoint_head


def tensors(out):
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items() if isinstance(v, torch.Tensor)}


def count_calls(obj, tag, calls):
    """Wraps the bound obj.prepare on the object itself, so that calls through `self` are counted too."""
    bound = obj.prepare

    def prepare(*args, **kwargs):
        calls.append(tag)
        return bound(*args, **kwargs)
    obj.prepare = prepare


@pytest.mark.parametrize("cls", ("mask", "keypoint"))
def test_a_first_forward_prepares_once(pkg, R, torch_dev, cls):
    m, head = branch_model(pkg, R, torch_dev[1], cls)
    x = bc.detector_input().to(torch_dev[1])
    calls = []
    count_calls(m, "model", calls)
    count_calls(head, "head", calls)
    assert m._shape is None and head._shape is None
    first = tensors(m(x))
    assert sorted(calls) == ["head", "model"], calls
    assert m._shape == (D["N"], D["H"], D["W"])
    again = tensors(m(x))                         # the same shape: neither prepares again
    assert sorted(calls) == ["head", "model"], calls
    assert set(again) == set(first) and int(first["count"].min()) > 0
    for k in first:
        assert same_bits(again[k], first[k]), k


@pytest.mark.parametrize("cls", ("mask", "keypoint"))
def test_a_failed_branch_prepare_leaves_the_model_unprepared(pkg, R, torch_dev, cls):
    """The head's prepare is replaced on the Python object by one that raises before it launches anything."""
    dev = torch_dev[1]
    x = bc.detector_input().to(dev)
    want = tensors(branch_model(pkg, R, dev, cls)[0](x))
    m, head = branch_model(pkg, R, dev, cls)

    def refuse(*args, **kwargs):
        raise pkg.WinoError("stub: the head does not prepare")
    for was_prepared in (False, True):            # on a new model, and on one that has run
        head.prepare = refuse
        with pytest.raises(pkg.WinoError, match="stub"):
            m.prepare(D["N"], D["H"], D["W"])
        assert m._shape is None
        del head.prepare
        got = tensors(m(x))                        # prepares, and is what a fresh model returns
        assert m._shape == (D["N"], D["H"], D["W"])
        assert set(got) == set(want)
        for k in want:
            assert same_bits(got[k], want[k]), (was_prepared, k)
