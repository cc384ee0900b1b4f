"""Host-side checks of the R-CNN image transform (wino_image_transform_hw, wino_transform_size) -- no GPU needed: the
C-ABI symbols, the size rule against torch's own ops and against the shape F.interpolate itself returns, batch_hw, every
refusal (each fires before the GPU is touched), the tests' own fp64 reference against torch's fp32 and fp64 CPU pipelines
at the shapes the GPU tests run, and the kinds of tile those shapes reach."""
import ctypes
import math

import numpy as np
import pytest
import torch

import transform_cases as tc
from conftest import ROOT

E_SHAPE, E_ARG = -2, -3
NEW = ["wino_image_transform_hw", "wino_transform_size"]


def test_new_symbols_exported_and_declared(pkg):
    import os
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "winograd_mi355x.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name + "(" in hdr, name
        assert name in pkg.SIGNATURES, name
    assert "#define WINO_TRANSFORM_MAX_IMAGES 32" in hdr and pkg.TRANSFORM_MAX_IMAGES == 32
    assert "#define WINO_IMAGE_F32 0" in hdr and "#define WINO_IMAGE_U8 1" in hdr
    assert pkg.IMAGE_DTYPES == {torch.float32: 0, torch.uint8: 1}
    for name in ("transform_size", "batch_hw", "image_transform"):
        assert hasattr(pkg, name), name
    for cls in (pkg.FasterRCNN, pkg.MaskRCNN):
        for name in ("prepare_images", "predict", "to_image_lists"):
            assert hasattr(cls, name), (cls, name)
    assert not [s for s in pkg.SIGNATURES if "transform" in s and "workspace_bytes" in s]
    assert (pkg.IMAGENET_MEAN, pkg.IMAGENET_STD) == (tc.IMAGENET_MEAN, tc.IMAGENET_STD)


# ---- the size rule ------------------------------------------------------------------------------------------------------
def test_transform_size_is_torchs_at_the_named_pairs(pkg):
    for hw, want in tc.PAIRS:
        assert pkg.transform_size(*hw) == want == tc.size_rule(*hw, 800, 1333), hw
    # a true fp32 division would give 799 x 1066 here
    assert math.floor(480 * float(np.float32(800) / np.float32(480))) == 799
    for (h, w), want in zip(tc.RULE["shapes"], tc.RULE["sizes"]):
        assert pkg.transform_size(h, w, *tc.RULE["min_max"]) == want
    assert pkg.batch_hw(tc.RULE["sizes"]) == tc.RULE["batch"]


def _sweep(n=2000):
    rng = np.random.RandomState(2024)
    return [tuple(int(v) for v in rng.randint(1, 2001, 4)) for _ in range(n)]


def test_transform_size_equals_the_restated_rule_on_a_sweep(pkg):
    zero = 0
    for h, w, mn, mx in _sweep():
        want = tc.size_rule(h, w, mn, mx)
        if min(want) == 0:
            zero += 1
            with pytest.raises(pkg.WinoError, match="rc=-2"):
                pkg.transform_size(h, w, mn, mx)
        else:
            assert pkg.transform_size(h, w, mn, mx) == want, (h, w, mn, mx)
    print(f"{zero} of 2000 resize an axis to nothing and are refused")
    assert zero < 200


def test_transform_size_is_the_shape_interpolate_returns(pkg):
    done = 0
    for h, w, mn, mx in _sweep():
        if min(tc.size_rule(h, w, mn, mx)) == 0:
            continue
        im = torch.tensor([h, w])
        s = torch.min(float(mn) / torch.min(im).to(torch.float32), float(mx) / torch.max(im).to(torch.float32)).item()
        got = torch.nn.functional.interpolate(torch.zeros(1, 1, h, w), scale_factor=s, mode="bilinear",
                                              recompute_scale_factor=True, align_corners=False)
        assert tuple(got.shape[2:]) == pkg.transform_size(h, w, mn, mx), (h, w, mn, mx)
        done += 1
        if done == 32:
            break
    assert done == 32


def test_transform_size_refusals(pkg):
    L = pkg.lib()
    a, b = ctypes.c_int(-1), ctypes.c_int(-1)
    call = lambda *v: L.wino_transform_size(*v, ctypes.byref(a), ctypes.byref(b))
    assert call(480, 640, 800, 1333) == 0 and (a.value, b.value) == (800, 1066)
    for bad in [(0, 640, 800, 1333), (480, -1, 800, 1333), (480, 640, 0, 1333), (480, 640, 800, 0)]:
        assert call(*bad) == E_SHAPE, bad
    assert call(1, 2000, 1, 1) == E_SHAPE and "resizes to" in L.wino_last_error_string().decode()
    assert L.wino_transform_size(480, 640, 800, 1333, None, ctypes.byref(b)) == E_ARG
    assert L.wino_transform_size(480, 640, 800, 1333, ctypes.byref(a), None) == E_ARG


def test_batch_hw(pkg):
    assert pkg.batch_hw([(800, 1066), (799, 1199)]) == (800, 1216)
    assert pkg.batch_hw([(24, 31), (40, 12), (24, 24)], 1) == (40, 31)
    assert pkg.batch_hw([(64, 96)]) == (64, 96) and pkg.batch_hw([(65, 97)]) == (96, 128)
    assert pkg.batch_hw([(5, 7), (9, 2)], 5) == (10, 10)
    rng = np.random.RandomState(3)
    for _ in range(50):
        sizes = [tuple(int(v) for v in rng.randint(1, 500, 2)) for _ in range(rng.randint(1, 5))]
        d = int(rng.randint(1, 70))
        Hb, Wb = pkg.batch_hw(sizes, d)
        for got, side in ((Hb, max(s[0] for s in sizes)), (Wb, max(s[1] for s in sizes))):
            assert got % d == 0 and side <= got < side + d
    for bad in ([], None):
        with pytest.raises((pkg.WinoError, TypeError)):
            pkg.batch_hw(bad)
    with pytest.raises(pkg.WinoError, match="size_divisible"):
        pkg.batch_hw([(3, 3)], 0)


# ---- refusals -----------------------------------------------------------------------------------------------------------
IMG, OUT = 1 << 40, 2 << 40   # far apart: nothing overlaps by accident
OK = dict(N=2, C=3, dtype=0, hw=[(13, 17), (30, 9)], ohw=[(24, 31), (40, 12)], Hb=64, Wb=32, mean=tc.IMAGENET_MEAN,
          std=tc.IMAGENET_STD, out=OUT)


def _call(pkg, ptrs=..., null=(), **kw):
    a = dict(OK, **kw)
    N = a["N"]
    n = max(N, 1)
    if ptrs is ...:
        ptrs = [IMG + (1 << 30) * i for i in range(n)]
    arr = (ctypes.c_void_p * n)(*ptrs)
    flat = lambda v: (ctypes.c_int * (2 * n))(*[x for s in (list(v) * n)[:n] for x in s])
    f = lambda v: (ctypes.c_float * 4)(*(list(v) + [0.0] * 4)[:4])
    args = dict(images=arr, hw=flat(a["hw"]), ohw=flat(a["ohw"]), mean=f(a["mean"]), std=f(a["std"]))
    for k in null:
        args[k] = None
    out = None if a["out"] is None else ctypes.c_void_p(a["out"])
    return pkg.lib().wino_image_transform_hw(args["images"], args["hw"], args["ohw"], N, a["C"], a["dtype"], args["mean"],
                                             args["std"], out, a["Hb"], a["Wb"], None)


def test_every_refusal_fires_without_a_gpu(pkg):
    L = pkg.lib()
    err = lambda: L.wino_last_error_string().decode()
    nan, inf = float("nan"), float("inf")
    # shapes of the call
    for k, v in (("N", -1), ("C", 0), ("C", 5), ("C", -1), ("Hb", 0), ("Wb", -3)):
        assert _call(pkg, **{k: v}) == E_SHAPE and f"{k}={v}" in err(), (k, v)
    for v in (2, -1):
        assert _call(pkg, dtype=v) == E_ARG and f"dtype={v}" in err()
    # N == 0 is fine and needs nothing else
    assert _call(pkg, N=0, out=None, null=("images", "hw", "ohw", "mean", "std")) == 0
    # NULL pointers
    for k in ("images", "hw", "ohw", "mean", "std"):
        assert _call(pkg, null=(k,)) == E_ARG and "NULL" in err(), k
    assert _call(pkg, out=None) == E_ARG and "NULL" in err()
    assert _call(pkg, ptrs=[IMG, None]) == E_ARG and "NULL pointer (image 1)" in err()
    # alignment: out 16 bytes, a float image 4, a byte image none
    for off in (4, 8, 1):
        assert _call(pkg, out=OUT + off) == E_ARG and "aligned" in err(), off
    for off in (1, 2, 3):
        assert _call(pkg, ptrs=[IMG, IMG + (1 << 30) + off]) == E_ARG and "image 1" in err() and "4-byte aligned" in err()
        # ... which a byte image need not be: the call gets as far as the overlap check
        assert _call(pkg, ptrs=[IMG, IMG + (1 << 30) + off], dtype=1, out=IMG + (1 << 30)) == E_ARG and "overlap image 1" in err()
    # mean and std
    for c in range(3):
        for v in (nan, inf, -inf):
            bad = list(tc.IMAGENET_MEAN)
            bad[c] = v
            assert _call(pkg, mean=bad) == E_ARG and f"mean[{c}]" in err(), (c, v)
        for v in (0.0, -0.0, nan, inf, 1e-40):         # (1e-40: a denormal, whose fp32 reciprocal is infinite)
            bad = list(tc.IMAGENET_STD)
            bad[c] = v
            assert _call(pkg, std=bad) == E_ARG and f"std[{c}]" in err(), (c, v)
    assert _call(pkg, C=1, mean=[0.5, nan], std=[0.5, 0.0], out=IMG) == E_ARG and "overlap" in err()   # only C entries are read
    # per-image shapes
    for which in ("hw", "ohw"):
        for pos in (0, 1):
            for v in (0, -1):
                s = [list(x) for x in OK[which]]
                s[1][pos] = v
                assert _call(pkg, **{which: s}) == E_SHAPE and "image 1" in err() and f"={v}" in err(), (which, pos, v)
    assert _call(pkg, ohw=[(24, 31), (65, 12)]) == E_SHAPE and "65x12" in err()           # ho > Hb
    assert _call(pkg, ohw=[(24, 33), (40, 12)]) == E_SHAPE and "24x33" in err()           # wo > Wb
    assert _call(pkg, ohw=[(64, 32), (64, 32)], out=IMG) == E_ARG and "overlap" in err()  # ... and equal is fine
    # 2 ho h and 2 wo w below 2^31
    big = dict(Hb=32768, Wb=32768, C=1)
    assert _call(pkg, hw=[(32768, 1)] * 2, ohw=[(32768, 1)] * 2, **big) == E_SHAPE and "2*ho*h" in err()
    assert _call(pkg, hw=[(1, 32768)] * 2, ohw=[(1, 32768)] * 2, **big) == E_SHAPE and "2*wo*w" in err()
    assert _call(pkg, hw=[(32767, 1)] * 2, ohw=[(32768, 1)] * 2, out=IMG, **big) == E_ARG and "overlap" in err()
    # one image of out and one source image below 2^31 elements
    assert _call(pkg, Hb=32768, Wb=32768, C=2) == E_SHAPE and "one image of out" in err()
    four = dict(C=4, mean=[0.5] * 4, std=[0.25] * 4)
    assert _call(pkg, Hb=32768, Wb=16384, **four) == E_SHAPE and "one image of out" in err()
    assert _call(pkg, hw=[(13, 17), (32768, 16384)], **four) == E_SHAPE and "image 1" in err() and "32-bit" in err()
    assert _call(pkg, hw=[(13, 17), (32768, 16383)], out=IMG, **four) == E_ARG and "overlap" in err()
    # out against every image: N = 2, out is 2 x 3 x 64 x 32 floats, image 1 is 3 x 30 x 9 floats (bytes with dtype 1)
    out_b, p1 = 2 * 3 * 64 * 32 * 4, IMG + (1 << 30)
    for dtype, img_b in ((0, 3 * 30 * 9 * 4), (1, 3 * 30 * 9)):
        for out in (p1, (p1 + img_b - 1) // 16 * 16, p1 - out_b + 16):
            assert _call(pkg, out=out, dtype=dtype) == E_ARG and "overlap image 1" in err(), (dtype, out)
    assert _call(pkg, out=IMG, dtype=1) == E_ARG and "overlap image 0" in err()
    # the tiles of one plane (8 rows x 256 columns) are one launch's grid: fewer than 2^24
    assert _call(pkg, Hb=1 << 27, Wb=1, C=1, ohw=[(24, 1), (40, 1)]) == E_SHAPE and "16777216 tiles" in err()
    assert _call(pkg, Hb=(1 << 27) - 8, Wb=1, C=1, ohw=[(24, 1), (40, 1)], out=IMG) == E_ARG and "overlap" in err()


# ---- the tests' own reference, against torch ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tc.CASES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
def test_reference_agrees_with_torchs_fp32_pipeline(name, dtype):
    """Measured: at most 6.5e-6 of max |want| over shapes up to 97 px; the bar is three times that.  (At 480 x 640 torch's
    fp32 source coordinate is 7.6e-5 off the exact result, which is why the kernel is held to the fp64 reference.)
    "ratios" has a source of 1000 px, where that coordinate is as far off (measured 6.4e-5): there, as in every case, the
    reference is held to torch's pipeline in fp64, whose coordinates are doubles, at 1e-12 (measured: at most 1.2e-13)."""
    c = tc.CASES[name]
    for C in (3, 1):
        imgs = tc.images(c["shapes"], C, dtype, seed=5)
        mean, std = tc.mean_std(C)
        want = tc.transform_reference(imgs, c["sizes"], *c["batch"], mean, std)
        got = tc.torch_pipeline(imgs, c["sizes"], *c["batch"], mean, std)
        err = np.abs(got - want).max() / np.abs(want).max()
        exact = tc.torch_pipeline(imgs, c["sizes"], *c["batch"], mean, std, torch.float64)
        err64 = np.abs(exact - want).max() / np.abs(want).max()
        print(f"{name} C={C} {dtype}: reference against torch's fp32 pipeline: {err:.2e}, against its fp64 one: {err64:.2e}")
        assert err64 <= 1e-12
        if name != "ratios":       # (a 1000 px source: torch's fp32 source coordinate alone is 6e-5 off there)
            assert err <= 2e-5
        for i, (ho, wo) in enumerate(c["sizes"]):
            assert (want[i, :, ho:] == 0).all() and (want[i, :, :, wo:] == 0).all()


def test_the_cases_reach_every_kind_of_tile():
    """The kernel's tile rule restated (256 columns x 8 rows, a pad tile iff y_first >= ho or x_first >= wo): over all
    cases there is a pad tile by rows only, by columns only and by both, a live tile with a zero tail in x and one in y,
    a lane with fewer than four valid columns, and a tile of one row.  A condition on the inputs of the GPU tests."""
    per_case = {name: tc.tile_kinds(c["sizes"], *c["batch"]) for name, c in tc.CASES.items()}
    kinds = set().union(*per_case.values())
    assert kinds >= {"pad by rows only", "pad by columns only", "pad by both", "live", "live with a zero tail in x",
                     "live with a zero tail in y", "valid < 4", "valid < 4 in a pad tile", "one-row tile"}
    assert "pad by columns only" in per_case["pad_right"] and "pad by columns only" not in per_case["wide"]
    assert {"valid < 4", "one-row tile"} <= per_case["tile_edges_odd"] and "one-row tile" in per_case["tile_edges"]
    for name in ("pad_right", "tile_edges", "tile_edges_odd"):      # more than one x-chunk
        assert tc.CASES[name]["batch"][1] > tc.TILE_W
    c = tc.CASES["tile_edges"]
    assert {s[1] for s in c["sizes"]} == {255, 256, 257} and {s[0] for s in c["sizes"]} == {7, 8, 9}
    for name in tc.THIN:
        c = tc.CASES[name]
        assert all(min(s) == 1 for s in c["sizes"]) and all(min(s) == 1 for s in c["shapes"])
        assert min(c["batch"]) == 1
    for c in tc.CASES.values():
        assert all(ho <= c["batch"][0] and wo <= c["batch"][1] for ho, wo in c["sizes"])
    sweep = tc.sweep_specs()
    assert len(sweep) == tc.SWEEP_COUNT == 40 and {s["C"] for s in sweep} == {1, 2, 3, 4}
    assert {s["dtype"] for s in sweep} == {"f32", "u8"} and {len(s["shapes"]) for s in sweep} == {1, 2, 3, 4, 5}
    assert any(a == b for s in sweep for a, b in zip(s["shapes"], s["sizes"]))
    assert any(s["batch"][1] > tc.TILE_W for s in sweep) and any(s["batch"][1] % 4 for s in sweep)
    swept = set().union(*[tc.tile_kinds(s["sizes"], *s["batch"]) for s in sweep])
    assert swept >= {"pad by rows only", "pad by columns only", "pad by both", "valid < 4"}


def test_footprint_is_the_references_nan_set():
    (h, w), (ho, wo), (Hb, Wb) = tc.RULE["shapes"][1], tc.RULE["sizes"][1], tc.RULE["batch"]
    imgs = tc.images([(h, w)], 3, seed=1)
    imgs[0][1, 11, 4] = float("nan")
    want = tc.transform_reference(imgs, [(ho, wo)], Hb, Wb, *tc.mean_std(3))
    mark = tc.footprint(h, w, ho, wo, Hb, Wb, 11, 4)
    assert 0 < mark.sum() < ho * wo
    assert np.array_equal(np.isnan(want[0, 1]), mark) and not np.isnan(want[0, [0, 2]]).any()
