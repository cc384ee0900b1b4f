"""Host-side checks of the bilinear resize and label-map layer (wino_resize_bilinear_*) and of the segmentation networks'
aux state dict -- no GPU needed: the C-ABI symbols, the tests' own fp64 reference proven against torch's float64
interpolate (values, labels, NaN set), every refusal (each fires before the GPU is touched), the plan at the shapes the
GPU tests run, and the aux_classifier validation."""
import ctypes
import importlib
import os

import numpy as np
import pytest

from conftest import ROOT
from resize_cases import (DIRECT, DIRECT_SMALL, EXACT_WIDTHS, STAGED, STAGED_SHAPES, WORKLOAD, labels_of,
                          resize_reference, smallest_direct_channels)

E_SHAPE, E_ARG = -2, -3
NEW = ["wino_resize_bilinear_hw", "wino_resize_bilinear_plan"]
TORCH_SHAPES = [((9, 9), (65, 65)), ((7, 11), (49, 81)), ((5, 3), (33, 49)), ((9, 9), (4, 5)), ((1, 1), (7, 3)),
                ((2, 3), (1, 1)), ((3, 130), (8, 1030))]


def test_new_symbols_exported_and_declared(pkg):
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "winograd_mi355x.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name + "(" in hdr, name
        assert name in pkg.SIGNATURES, name
    assert "#define WINO_RESIZE_FORM_STAGED 1" in hdr and "#define WINO_RESIZE_FORM_DIRECT 2" in hdr
    assert (pkg.RESIZE_FORM_STAGED, pkg.RESIZE_FORM_DIRECT) == (STAGED, DIRECT) == (1, 2)
    for name in ("resize_bilinear", "resize_bilinear_plan"):
        assert hasattr(pkg, name), name
    assert not [s for s in pkg.SIGNATURES if "resize" in s and "workspace_bytes" in s]


# ---- the tests' own reference, proven against torch -----------------------------------------------------------------------
@pytest.mark.parametrize("hw,HW", TORCH_SHAPES)
def test_reference_equals_torch_float64(hw, HW):
    import torch
    (h, w), (Ho, Wo) = hw, HW
    g = torch.Generator().manual_seed(h * 131 + Wo)
    src = torch.rand(2, h, w, 8, generator=g, dtype=torch.float64) - 0.5
    want = torch.nn.functional.interpolate(src[..., :5].permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear",
                                           align_corners=False)
    got = resize_reference(src.numpy(), Ho, Wo, C=5)
    assert got.shape == tuple(want.shape) and got.dtype == np.float64
    err = np.abs(got - want.numpy()).max()
    print(f"{hw}->{HW}: reference against torch float64: {err:.2e}")
    assert err < 1e-12
    assert np.array_equal(labels_of(want.numpy()), want.argmax(1).numpy())
    # the padded layout reads the interior only
    ringed = torch.full((2, h + 2, w + 2, 8), float("nan"), dtype=torch.float64)
    ringed[:, 1:-1, 1:-1, :] = src
    assert np.array_equal(resize_reference(ringed.numpy(), Ho, Wo, C=5, in_padded=True), got)
    # a subset of rows is those rows
    rows = sorted({0, Ho // 2, Ho - 1})
    assert np.array_equal(resize_reference(src.numpy(), Ho, Wo, C=5, rows=rows), got[:, :, rows, :])


@pytest.mark.parametrize("at", [(4, 4), (5, 5)])
def test_reference_nan_set_equals_torch(at):
    """(9, 9) -> (65, 65): output 32 sits on source pixel 4 exactly (lambda = 0), so its tap on pixel 5 has weight zero
    and still carries a NaN there."""
    import torch
    src = torch.rand(1, 9, 9, 4, generator=torch.Generator().manual_seed(7), dtype=torch.float64) - 0.5
    src[0, at[0], at[1], 2] = float("nan")
    want = torch.nn.functional.interpolate(src.permute(0, 3, 1, 2), size=(65, 65), mode="bilinear",
                                           align_corners=False).numpy()
    got = resize_reference(src.numpy(), 65, 65)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(got[0, 2]).any() and not np.isnan(got[0, [0, 1, 3]]).any()
    if at == (5, 5):
        assert np.isnan(got[0, 2, 32, 32])                       # the zero-weight tap
    assert np.abs(got[~np.isnan(got)] - want[~np.isnan(want)]).max() < 1e-12
    assert np.array_equal(labels_of(got), torch.from_numpy(want).argmax(1).numpy())


# ---- refusals -----------------------------------------------------------------------------------------------------------
P = lambda v: ctypes.c_void_p(v)
SRC, OUT, LAB = 1 << 40, 2 << 40, 3 << 40   # far apart: nothing overlaps by accident
OK_SHAPE = dict(N=2, h=9, w=9, C=21, ld=64, in_padded=0, Ho=65, Wo=65)


def _call(pkg, src=SRC, out=OUT, lab=LAB, **kw):
    a = dict(OK_SHAPE, **kw)
    p = lambda v: None if v is None else P(v)
    return pkg.lib().wino_resize_bilinear_hw(p(src), p(out), p(lab), a["N"], a["h"], a["w"], a["C"], a["ld"],
                                             a["in_padded"], a["Ho"], a["Wo"], None)


def test_every_refusal_fires_without_a_gpu(pkg):
    L = pkg.lib()
    err = lambda: L.wino_last_error_string().decode()
    assert _call(pkg, src=None) == E_ARG and "NULL" in err()
    assert _call(pkg, out=None, lab=None) == E_ARG and "both NULL" in err()
    for k in ("src", "out", "lab"):
        assert _call(pkg, **{k: dict(src=SRC, out=OUT, lab=LAB)[k] + 4}) == E_ARG and "aligned" in err(), k
    for k in ("N", "h", "w", "Ho", "Wo", "C"):
        for v in (0, -1):
            assert _call(pkg, **{k: v}) == E_SHAPE and f"{k}={v}" in err(), (k, v)
    assert _call(pkg, C=65) == E_SHAPE and "C=65" in err()             # C > ld
    assert _call(pkg, C=4, ld=6) == E_SHAPE and "ld=6" in err()       # ld % 4
    for v in (2, -1):
        assert _call(pkg, in_padded=v) == E_SHAPE and f"in_padded={v}" in err()
    # one image below 2^31 elements: src, out; labels' image is out's with C = 1
    assert _call(pkg, h=32768, w=16384, ld=4, C=4) == E_SHAPE and "32-bit" in err()
    assert _call(pkg, Ho=8192, Wo=8192, C=32) == E_SHAPE and "32-bit" in err()
    assert _call(pkg, h=1, w=1, Ho=65536, Wo=32768, C=1, ld=4) == E_SHAPE and "32-bit" in err()
    # ... and the same out image is fine when only labels are wanted: recognised by the next check, the overlap
    assert _call(pkg, out=None, lab=SRC, Ho=8192, Wo=8192, C=32) == E_ARG and "overlap" in err()
    # 2 Ho h and 2 Wo w below 2^31
    assert _call(pkg, h=32768, w=1, Ho=32768, Wo=1, C=1, ld=4) == E_SHAPE and "2*Ho*h" in err()
    assert _call(pkg, h=1, w=32768, Ho=1, Wo=32768, C=1, ld=4) == E_SHAPE and "2*Wo*w" in err()
    assert _call(pkg, out=SRC, h=32768, w=1, Ho=32767, Wo=1, C=1, ld=4) == E_ARG and "overlap" in err()
    # pairwise disjoint: src [2][9][9][64], out [2][21][65][65], labels [2][65][65]
    in_b, out_b, lab_b = 2 * 81 * 64 * 4, 2 * 21 * 65 * 65 * 4, 2 * 65 * 65 * 4
    out_b, lab_b = out_b // 16 * 16, lab_b // 16 * 16                 # (pointers stay 16-byte aligned; each buffer is 8 bytes longer)
    for out in (SRC, SRC + in_b - 16, SRC - out_b + 16):
        assert _call(pkg, out=out) == E_ARG and "overlap" in err(), out
    for lab in (SRC, SRC + in_b - 16, SRC - lab_b + 16, OUT, OUT + out_b - 16, OUT - lab_b + 16):
        assert _call(pkg, lab=lab) == E_ARG and "overlap" in err(), lab
    assert _call(pkg, out=None, lab=SRC + 16) == E_ARG and "overlap" in err()
    # the padded source is larger: an out that begins where the unpadded one would end
    assert _call(pkg, out=SRC + in_b, in_padded=1) == E_ARG and "overlap" in err()


def test_plan_refusals(pkg):
    L = pkg.lib()
    f = ctypes.c_int(-1)
    plan = lambda *a: L.wino_resize_bilinear_plan(*a, ctypes.byref(f))
    assert plan(9, 9, 21, 64, 65, 65, 1, 0) == 0 and f.value == STAGED
    assert L.wino_resize_bilinear_plan(9, 9, 21, 64, 65, 65, 1, 0, None) == E_ARG
    assert plan(9, 9, 21, 64, 65, 65, 0, 0) == E_ARG
    for bad in [(0, 9, 21, 64, 65, 65), (9, 9, 0, 64, 65, 65), (9, 9, 65, 64, 65, 65), (9, 9, 4, 6, 65, 65),
                (9, 9, 21, 64, 0, 65), (9, 9, 21, 64, 65, -1), (32768, 1, 1, 4, 32768, 1), (1, 1, 32, 32, 8192, 8192)]:
        assert plan(*bad, 1, 1) == E_SHAPE, bad
    assert plan(1, 1, 32, 32, 8192, 8192, 0, 1) == 0               # labels alone: no out image to bound
    with pytest.raises(pkg.WinoError, match="rc=-2"):
        pkg.resize_bilinear_plan(9, 9, 21, 63, 65, 65)


def test_plan_forms(pkg):
    h, w, C, ld, Ho, Wo = WORKLOAD
    for want_out, want_labels in ((1, 0), (0, 1), (1, 1)):           # a function of the shape alone
        assert pkg.resize_bilinear_plan(h, w, C, ld, Ho, Wo, want_out, want_labels) == STAGED
    assert pkg.resize_bilinear_plan(33, 33, 21, 64, 260, 260) == STAGED
    for N, h, w, Ho, Wo, C, ld in STAGED_SHAPES:
        assert pkg.resize_bilinear_plan(h, w, C, ld, Ho, Wo) == STAGED, (h, w, Ho, Wo, C)
    for w, Wo in EXACT_WIDTHS:
        assert pkg.resize_bilinear_plan(1, w, 1, 4, 1, Wo) == STAGED, (w, Wo)
    assert pkg.resize_bilinear_plan(17, 17, 3, 4, 10923, 10923) == STAGED
    N, h, w, Ho, Wo, C, ld = DIRECT_SMALL
    assert pkg.resize_bilinear_plan(h, w, C, ld, Ho, Wo) == DIRECT
    # very many classes: two source rows x six columns (pitch 7) x C floats no longer fit in 64 KB
    C = smallest_direct_channels(pkg)
    assert C % 4 == 0 and pkg.resize_bilinear_plan(6, 6, C - 4, C - 4, 13, 11) == STAGED
    assert 2 * 7 * (C - 4) * 4 <= 64 << 10 < 2 * 7 * C * 4
    # the boundary of the down-scale rule: up to 4x per axis is staged
    assert pkg.resize_bilinear_plan(64, 12, 8, 8, 16, 3) == STAGED and pkg.resize_bilinear_plan(65, 12, 8, 8, 16, 3) == DIRECT
    assert pkg.resize_bilinear_plan(12, 13, 8, 8, 3, 3) == DIRECT


# ---- the aux head's state dict ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["fcn", "deeplabv3"])
def test_aux_state_dict_validation(pkg, net):
    import torch
    S = importlib.import_module("cuda_winograd_amd.segmentation")
    expected = getattr(S, f"expected_{net}_keys")
    validate = getattr(S, f"validate_{net}_state_dict")
    plain, exp = expected("resnet50", 21), expected("resnet50", 21, aux=True)
    aux_keys = sorted(set(exp) - set(plain))
    assert len(aux_keys) == 7 and all(k.startswith("aux_classifier.") for k in aux_keys)
    assert exp["aux_classifier.0.weight"] == (256, 1024, 3, 3) and exp["aux_classifier.1.running_var"] == (256,)
    assert exp["aux_classifier.4.weight"] == (21, 256, 1, 1) and exp["aux_classifier.4.bias"] == (21,)
    sd = {k: torch.empty(v) for k, v in exp.items()}
    sd["aux_classifier.1.num_batches_tracked"] = torch.tensor(1)
    assert validate(sd, "resnet50", aux=True) == 21 and validate(sd, "resnet50") == 21
    for k in aux_keys:
        bad = dict(sd)
        del bad[k]
        with pytest.raises(pkg.WinoError, match=f"missing key '{k}'"):
            validate(bad, "resnet50", aux=True)
        assert validate(bad, "resnet50") == 21                       # aux=False: accepted and ignored
        bad = dict(sd, **{k: torch.empty((3,) + tuple(exp[k]))})
        with pytest.raises(pkg.WinoError, match=f"'{k}' has shape"):
            validate(bad, "resnet50", aux=True)
        assert validate(bad, "resnet50") == 21
    bad = dict(sd, **{"aux_classifier.5.weight": torch.empty(3)})
    with pytest.raises(pkg.WinoError, match="unexpected key 'aux_classifier.5.weight'"):
        validate(bad, "resnet50", aux=True)
    assert validate(bad, "resnet50") == 21
    # the first of two broken keys is the one named
    bad = dict(sd)
    del bad["aux_classifier.0.weight"], bad["aux_classifier.4.bias"]
    with pytest.raises(pkg.WinoError, match="missing key 'aux_classifier.0.weight'"):
        validate(bad, "resnet50", aux=True)
