"""The checks tests/test_gpu_retinanet.py and tests/test_gpu_fcos.py share, step for step: the tail of the detector on
the GPU's own candidates, one graph against eager, and predict against forward.  A support module, not a test module."""
import numpy as np
import torch

from gpu_support import same_bits

OUT_KEYS = ("boxes", "scores", "labels", "count")


def cpu(t):
    return t.detach().cpu()


def check_tail(m, out, det, valid, score_thresh, assert_margins, thresh_margin, tie_gaps):
    """The tail against `det`, the reference's detections_reference on the GPU's candidates (`valid`: idx >= 0): the order
    against the reference's orders, the count, bit-equal boxes and scores, the labels, the reference's decision margins
    (with the levels' `thresh_margin` and `tie_gaps`), and rows past count zero with label -1."""
    order = cpu(out["order"]).numpy()
    for i in range(order.shape[0]):
        c = len(det["orders"][i])
        assert np.array_equal(order[i, :c], det["orders"][i]) and not valid[i, order[i, c:]].any()
    assert np.array_equal(cpu(out["count"]).numpy(), det["count"])
    assert same_bits(out["boxes"], det["boxes"]) and same_bits(out["scores"], det["scores"])
    assert torch.equal(cpu(out["labels"]), torch.from_numpy(det["labels"]))
    print("margins: threshold", thresh_margin, "ties", tie_gaps, det["tie_gap"], "iou", det["iou_margin"], "detections",
          det["count"].tolist())
    assert_margins(thresh_margin, tie_gaps + [det["tie_gap"]], det["iou_margin"])
    assert int(det["count"].min()) > 0
    for n, d in enumerate(m.to_lists(out)):                           # rows past count: zero, label -1
        c = int(det["count"][n])
        assert tuple(d["boxes"].shape) == (c, 4) and bool((d["labels"] >= 0).all()) and bool((d["scores"] > score_thresh).all())
        assert bool((cpu(out["boxes"])[n, c:] == 0).all()) and bool((cpu(out["labels"])[n, c:] == -1).all())
        assert bool((cpu(out["scores"])[n, c:] == 0).all())


def check_one_graph_replays_bitwise(pkg, m, x, poison):
    """The whole forward captured into one graph -- a host read of device data inside it would fail the capture -- replays
    bitwise equal to eager into NaN-filled outputs and NaN-filled `poison(m)`, the model's 32-bit intermediate buffers
    (asked for after the prepare below, which allocates them anew), and no ticket stays held."""
    N, _, H, W = x.shape
    sg = torch.cuda.Stream()
    with torch.cuda.stream(sg):
        m.prepare(N, H, W)
        eager = {k: v.clone() for k, v in m(x).items()}
    sg.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=sg):
        out = m(x)
    for _ in range(2):
        for k in ("boxes", "scores"):
            out[k].fill_(float("nan"))
        for t in poison(m):
            t.view(torch.int32).fill_(0x7FC00000)
        graph.replay()
        torch.cuda.synchronize()
        for k in OUT_KEYS:
            assert same_bits(out[k], eager[k]), k
    with torch.cuda.stream(sg):
        assert pkg.tickets_in_use() == 0
    del graph


def check_predict_on_two_images_of_different_sizes(m, dev, shape):
    """predict is the shared detector path: image_transform -> forward on the batch with the resized sizes -> boxes x
    ratio.  Its boxes are forward's on the transformed batch times the ratio, bit for bit, and lie inside each image.
    Leaves the model prepared for `shape` = (N, H, W) again."""
    g = torch.Generator().manual_seed(3)
    images = [torch.rand(3, 50, 70, generator=g).to(dev), torch.rand(3, 64, 48, generator=g).to(dev)]
    m.prepare_images([t.shape for t in images], min_size=64, max_size=96)
    out = m.predict(images)
    torch.cuda.synchronize()
    got = {k: out[k].clone() for k in OUT_KEYS}
    tf = m._tf
    assert out["original_sizes"] == [(50, 70), (64, 48)] and tuple(tf["batch"].shape) == (2, 3, *tf["shape"][1:])
    ref = m(tf["batch"].clone(), tf["image_hw"])
    torch.cuda.synchronize()
    assert same_bits(got["boxes"], cpu(ref["boxes"] * tf["ratio"]))
    for k in ("scores", "labels", "count"):
        assert same_bits(got[k], cpu(ref[k])), k
    assert int(got["count"].min()) > 0
    for d, (h, w) in zip(m.to_image_lists(out), out["original_sizes"]):
        b = d["boxes"].cpu()
        assert bool((b[:, 0::2] <= w + 1e-3).all()) and bool((b[:, 1::2] <= h + 1e-3).all()) and bool((b >= 0).all())
    m.prepare(*shape)
