"""GPU tests of the R-CNN image transform (wino_image_transform_hw through pkg.image_transform) against the fp64
reference of tests/transform_cases.py at 2e-5 of max |want| -- wino_resize_bilinear_hw's own bar for the same arithmetic
-- with the pad region compared bitwise with +0.  Outputs are prefilled with NaN, so an element the launch does not write
fails either check.  Shapes are the smallest at which the kernel can go wrong: three images of different sizes in one
batch, an odd Wb (4-byte store tails, rows off 16 bytes), an identity size, an upscale, a down-scale beyond 4x, a batch of
two x-chunks and three row tiles, pad tiles to the right of an image, sizes on and one off every tile edge, axes of length
1, extreme ratios, C = 1 to 4, uint8 images at odd addresses, 33 images (two launches), and a seeded sweep of legal calls."""
import functools

import numpy as np
import pytest
import torch

import guarded
import transform_cases as tc
from gpu_support import torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def case(name, C, dtype):
    """(images on the CPU, mean, std, the fp64 reference): computed once, shared, never written."""
    c = tc.CASES[name]
    imgs = tc.images(c["shapes"], C, dtype, seed=11)
    mean, std = tc.mean_std(C)
    want = tc.transform_reference(imgs, c["sizes"], *c["batch"], mean, std)
    want.setflags(write=False)
    return imgs, mean, std, want


def on_device(imgs, dev):
    """The list on the device; uint8 images as views at odd addresses of one buffer (they need no alignment)."""
    if imgs[0].dtype != torch.uint8:
        return [t.to(dev) for t in imgs]
    buf = torch.zeros(sum(t.numel() + 3 for t in imgs) + 1, dtype=torch.uint8, device=dev)
    out, at = [], 1
    for t in imgs:
        at += (buf.data_ptr() + at + 1) % 2            # an odd address
        v = buf[at:at + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 2 == 1
        out.append(v)
        at += t.numel()
    return out


def run(pkg, dev, imgs, sizes, batch, mean, std):
    d = on_device(imgs, dev)
    out = torch.full((len(imgs), int(imgs[0].shape[0]), *batch), NAN, device=dev)
    got = pkg.image_transform(d, sizes, *batch, mean, std, out=out)
    torch.cuda.synchronize()
    assert got is out
    return out.cpu().numpy()


@pytest.mark.parametrize("C", [3, 1, 2, 4])
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_cases_against_fp64(pkg, torch_dev, name, dtype, C):
    c = tc.CASES[name]
    if name in ("rule", "odd_wb"):          # the sizes are torchvision's rule's, the batch is batch_hw's
        assert [pkg.transform_size(h, w, *tc.RULE["min_max"]) for h, w in c["shapes"]] == c["sizes"]
        assert pkg.batch_hw(c["sizes"], 32 if name == "rule" else 1) == c["batch"]
    imgs, mean, std, want = case(name, C, dtype)
    got = run(pkg, torch_dev[1], imgs, c["sizes"], c["batch"], mean, std)
    tc.check(got, want, c["sizes"], f"{name} C={C} {dtype}")


@pytest.mark.parametrize("name,image,at", [("rule", 1, (11, 4)), ("explicit", 0, (6, 8)), ("explicit", 2, (50, 20)),
                                           ("odd_wb", 1, (29, 8)), ("pad_right", 1, (5, 22)), ("pad_right", 0, (8, 149)),
                                           ("tile_edges", 2, (3, 63)), ("tile_edges", 0, (0, 99))])
def test_a_nan_pixel_reaches_exactly_its_footprint(pkg, torch_dev, name, image, at):
    """One NaN pixel in one channel of one image: NaN at exactly the outputs whose four taps include it (also under a
    zero weight, also at the identity size of "explicit" image 0), and no other bit of the batch changes."""
    c = tc.CASES[name]
    imgs, mean, std, _ = case(name, 3, torch.float32)
    clean = run(pkg, torch_dev[1], imgs, c["sizes"], c["batch"], mean, std)
    dirty_imgs = [t.clone() for t in imgs]
    dirty_imgs[image][1, at[0], at[1]] = NAN
    dirty = run(pkg, torch_dev[1], dirty_imgs, c["sizes"], c["batch"], mean, std)
    (h, w), (ho, wo) = c["shapes"][image], c["sizes"][image]
    mark = tc.footprint(h, w, ho, wo, *c["batch"], *at)
    assert 0 < mark.sum() < ho * wo
    assert not np.isnan(clean).any()
    assert np.array_equal(np.isnan(dirty[image, 1]), mark)
    same = dirty.view(np.int32) == clean.view(np.int32)
    same[image, 1][mark] = True
    assert same.all(), "a bit outside the footprint changed"


def test_33_images_split_into_launches_equal_single_calls(pkg, torch_dev):
    dev = torch_dev[1]
    shapes, sizes, batch = [(5, 7)] * 33, [(8, 11)] * 33, (8, 12)
    assert len(shapes) == pkg.TRANSFORM_MAX_IMAGES + 1
    imgs = tc.images(shapes, 3, seed=33)
    mean, std = tc.mean_std(3)
    got = run(pkg, dev, imgs, sizes, batch, mean, std)
    tc.check(got, tc.transform_reference(imgs, sizes, *batch, mean, std), sizes, "33 images")
    for i in range(33):
        one = run(pkg, dev, imgs[i:i + 1], sizes[:1], batch, mean, std)
        assert np.array_equal(one.view(np.int32)[0], got.view(np.int32)[i]), i
    assert not np.array_equal(got[32], got[0]) and not np.array_equal(got[32], got[31])


@pytest.mark.parametrize("align", guarded.ALIGNS)
@pytest.mark.parametrize("name", ["rule", "odd_wb", "pad_right"] + tc.THIN)
def test_guarded_arena(pkg, torch_dev, name, align):
    """Every image and the output between guards: no byte next to out changes, and the NaN that fills the guards behind
    and in front of every image never reaches a result."""
    c = tc.CASES[name]
    imgs, mean, std, want = case(name, 3, torch.float32)
    arena = guarded.Arena(torch, torch_dev[1], align)
    d = [arena.input(t, name=f"image{i}") for i, t in enumerate(imgs)]
    out = arena.output(len(imgs), 3, *c["batch"], name="out")
    for _ in range(2):
        out.fill_(NAN)
        assert pkg.image_transform(d, c["sizes"], *c["batch"], mean, std, out=out) is out
        arena.check(f"image_transform {name} align={align}")
        tc.check(out.cpu().numpy(), want, c["sizes"], f"guarded {name} align={align}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8], ids=["f32", "u8"])
def test_captured_into_a_graph_replays_on_new_contents(pkg, torch_dev, dtype):
    """No workspace, no scratch, no prepare: the call is captured as it is, and a replay reads the images' current
    contents."""
    dev = torch_dev[1]
    c = tc.CASES["rule"]
    imgs, mean, std, want = case("rule", 3, dtype)
    d = on_device(imgs, dev)
    out = torch.full((len(imgs), 3, *c["batch"]), NAN, device=dev)
    torch.cuda.synchronize()
    sg = torch.cuda.Stream()
    with torch.cuda.stream(sg):
        pkg.image_transform(d, c["sizes"], *c["batch"], mean, std, out=out)   # (the code object is loaded before the capture)
    sg.synchronize()
    out.fill_(NAN)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=sg):
        pkg.image_transform(d, c["sizes"], *c["batch"], mean, std, out=out)
    graph.replay()
    torch.cuda.synchronize()
    tc.check(out.cpu().numpy(), want, c["sizes"], f"graph {dtype}")
    other = tc.images(c["shapes"], 3, dtype, seed=12)
    for t, o in zip(d, other):
        t.copy_(o)                                   # in place: the captured pointers stay
    eager = pkg.image_transform(d, c["sizes"], *c["batch"], mean, std).clone()
    for _ in range(2):
        out.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), eager.view(torch.int32))
    tc.check(out.cpu().numpy(), tc.transform_reference(other, c["sizes"], *c["batch"], mean, std), c["sizes"], "replay")
    del graph


@pytest.mark.parametrize("index", range(tc.SWEEP_COUNT))
def test_transform_sweep(index, pkg, torch_dev):
    """Seeded legal calls: 1 to 5 images of 1 to 4 channels, either dtype (uint8 at odd addresses), sources up to 60 px,
    outputs up to 300 px in a batch that is a multiple of nothing, into a NaN-filled out."""
    s = tc.sweep_specs()[index]
    dtype = torch.uint8 if s["dtype"] == "u8" else torch.float32
    imgs = tc.images(s["shapes"], s["C"], dtype, seed=500 + index)
    mean, std = tc.mean_std(s["C"])
    want = tc.transform_reference(imgs, s["sizes"], *s["batch"], mean, std)
    got = run(pkg, torch_dev[1], imgs, s["sizes"], s["batch"], mean, std)
    tc.check(got, want, s["sizes"], f"sweep {index} {s}")
