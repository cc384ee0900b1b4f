"""GPU tests of the bilinear resize and label-map layer (wino_resize_bilinear_hw) against the fp64 reference of
tests/resize_cases.py, at cases.TIGHT: parity in both forms and all three uses, exact coordinates at widths where an fp32
source coordinate fails, the label rules (gap rule, ties, NaN), the non-finite footprint, guard bands, a tensor past
4 GiB, determinism and graph replay."""
import numpy as np
import pytest

import guarded
from cases import TIGHT
from gpu_support import graph_replay_scenario, torch_dev  # noqa: F401
from layer_refs import rel as rel_err
from resize_cases import (DIRECT, DIRECT_SMALL, EXACT_WIDTHS, STAGED, STAGED_SHAPES, ResizeCase, axis_coords,
                          check_labels, labels_of, resize_reference, smallest_direct_channels)

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def check_case(c, form, what):
    """All three uses of one case: out alone, labels alone, both; the two outs and the two label maps agree bitwise."""
    assert c.form() == form, what
    want = c.reference()
    out, _ = c.run(True, False)
    err = rel_err(out, want)
    print(f"{what}: out {err:.2e}")
    assert err < TIGHT, what
    _, lab = c.run(False, True)
    check_labels(lab, want, TIGHT, what)
    assert lab.min() >= 0 and lab.max() < c.C
    out2, lab2 = c.run(True, True)
    assert np.array_equal(bits(out2), bits(out)) and np.array_equal(lab2, lab), what
    # with both, the label is the argmax of the values that were stored
    assert np.array_equal(lab2, labels_of(out2)), what
    assert c.pkg.tickets_in_use() == 0
    return out, lab


@pytest.mark.parametrize("in_padded", [False, True])
@pytest.mark.parametrize("shape", STAGED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity_staged(shape, in_padded, pkg, torch_dev):
    N, h, w, Ho, Wo, C, ld = shape
    c = ResizeCase(pkg, torch_dev, N, h, w, Ho, Wo, C, ld, seed=h * 7 + Wo, in_padded=in_padded)
    out, _ = check_case(c, STAGED, f"staged {shape} padded={in_padded}")
    if (h, w) == (Ho, Wo):   # the same formula runs, and finite results are the input bit for bit
        p = 1 if in_padded else 0
        src = c.src[:, p:p + h, p:p + w, :C].permute(0, 3, 1, 2).numpy()
        assert np.array_equal(bits(out), bits(src))


@pytest.mark.parametrize("in_padded", [False, True])
def test_parity_direct(in_padded, pkg, torch_dev):
    N, h, w, Ho, Wo, C, ld = DIRECT_SMALL
    check_case(ResizeCase(pkg, torch_dev, N, h, w, Ho, Wo, C, ld, seed=3, in_padded=in_padded), DIRECT,
               f"direct {DIRECT_SMALL} padded={in_padded}")
    C = smallest_direct_channels(pkg)
    check_case(ResizeCase(pkg, torch_dev, 1, 6, 6, 13, 11, C, C, seed=4, in_padded=in_padded), DIRECT,
               f"direct (6, 6)->(13, 11) C={C} padded={in_padded}")


@pytest.mark.parametrize("w,Wo", EXACT_WIDTHS)
def test_exact_coordinates(w, Wo, pkg, torch_dev):
    """Widths at which torch's fp32 source coordinate misses TIGHT by 6-17x: integer coordinates hold it."""
    c = ResizeCase(pkg, torch_dev, 1, 1, w, 1, Wo, 1, 4, seed=w)
    assert c.form() == STAGED
    out, lab = c.run(True, True)
    err = rel_err(out, c.reference())
    print(f"{w}->{Wo}: out {err:.2e}")
    assert err < TIGHT
    assert (lab == 0).all()


def test_labels_ties_go_to_the_lowest_index(pkg, torch_dev):
    torch, dev = torch_dev
    c = ResizeCase(pkg, torch_dev, 2, 7, 11, 49, 81, 21, 64, seed=11)
    c.src[..., 9] = c.src[..., 3]                  # two equal class columns, raised above the rest on half the pixels
    c.src[:, :, ::2, 3] += 1.0
    c.src[:, :, ::2, 9] += 1.0
    want = c.reference().copy()
    assert np.array_equal(want[:, 3], want[:, 9])
    won = labels_of(want) == 3
    assert won.mean() > 0.1 and not (labels_of(want) == 9).any()
    want[:, 9] = -1.0                              # (below every score: the gap rule then measures class 3 against the others)
    for use in ((False, True), (True, True)):
        _, lab = c.run(*use)
        check_labels(lab, want, TIGHT, "ties")
        assert (lab != 9).all() and (lab[won] == 3).all()


def test_labels_nan_counts_as_the_largest_and_the_first_wins(pkg, torch_dev):
    c = ResizeCase(pkg, torch_dev, 2, 9, 9, 65, 65, 21, 64, seed=12)
    _, clean = c.run(False, True)
    src = c.src.clone()
    src[1, 4, 5, 7] = float("nan")
    src[1, 4, 5, 12] = float("nan")
    want = c.reference(src)
    foot = np.isnan(want[:, 7])
    assert foot.any() and np.array_equal(foot, np.isnan(want[:, 12])) and not foot[0].any()
    for use in ((False, True), (True, True)):
        _, lab = c.run(*use, src=src)
        assert (lab[foot] == 7).all()
        assert np.array_equal(lab[~foot], clean[~foot])


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("shape", [STAGED_SHAPES[0], STAGED_SHAPES[3], DIRECT_SMALL], ids=["staged", "identity", "direct"])
def test_nonfinite_footprint(shape, value, pkg, torch_dev):
    N, h, w, Ho, Wo, C, ld = shape
    c = ResizeCase(pkg, torch_dev, N, h, w, Ho, Wo, C, ld, seed=13)
    clean, _ = c.run()
    src = c.src.clone()
    n, k = N - 1, C // 2
    y, x = int(axis_coords(h, Ho)[0][Ho // 2]), int(axis_coords(w, Wo)[0][Wo // 2])   # a pixel some output taps
    src[n, y, x, k] = value
    got, _ = c.run(src=src)
    want = c.reference(src)
    hit = ~np.isfinite(want)
    assert hit.any() and not np.delete(hit, k, axis=1).any() and not hit[:n].any()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and not np.isneginf(got).any()
    assert np.array_equal(bits(got)[~hit], bits(clean)[~hit])        # every other bit is the clean run's


@pytest.mark.parametrize("align", guarded.ALIGNS)
@pytest.mark.parametrize("shape", [STAGED_SHAPES[1], DIRECT_SMALL], ids=["staged", "direct"])
def test_guarded_arena(shape, align, pkg, torch_dev):
    torch, dev = torch_dev
    N, h, w, Ho, Wo, C, ld = shape
    form = STAGED if shape is STAGED_SHAPES[1] else DIRECT
    for in_padded in (False, True):
        c = ResizeCase(pkg, torch_dev, N, h, w, Ho, Wo, C, ld, seed=14, in_padded=in_padded)
        assert c.form() == form
        arena = guarded.Arena(torch, dev, align)
        src = arena.input(c.src, name="src")
        out = arena.output(N, C, Ho, Wo, name="out")
        lab = arena.output(N, Ho, Wo, name="labels").view(torch.int32)   # (the arena holds float32: NaN bits until written)
        pkg.resize_bilinear(src, Ho, Wo, C=C, in_padded=in_padded, out=out, labels=lab)
        arena.check(f"resize {shape} align={align} padded={in_padded}")
        got, labels = out.cpu().numpy(), lab.cpu().numpy()
        assert rel_err(got, c.reference()) < TIGHT                       # (finite: no NaN beside src reached a result)
        assert labels.min() >= 0 and labels.max() < C
        check_labels(labels, c.reference(), TIGHT, "arena")


def test_output_past_4gib(pkg, torch_dev):
    """N = 3, (17, 17) -> (10923, 10923), C = 3: out is 4.3 GB, images re-based in 64 bits."""
    torch, dev = torch_dev
    N, h, Ho, C = 3, 17, 10923, 3
    c = ResizeCase(pkg, torch_dev, N, h, h, Ho, Ho, C, 4, seed=15)
    assert c.form() == STAGED and N * C * Ho * Ho * 4 > 1 << 32
    out = torch.full((N, C, Ho, Ho), float("nan"), device=dev)
    pkg.resize_bilinear(c.src.to(dev), Ho, Ho, C=C, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    rows = sorted(set(range(8)) | set(range(Ho - 8, Ho)) | set(range(0, Ho, 997)))
    got = out[:, :, torch.tensor(rows, device=dev), :].cpu().numpy()
    del out
    want = resize_reference(c.src.numpy(), Ho, Ho, C=C, rows=rows)
    for n in range(N):
        err = rel_err(got[n], want[n])
        print(f"past 4 GiB: image {n}: {len(rows)} rows: {err:.2e}")
        assert err < TIGHT


@pytest.mark.parametrize("shape", [STAGED_SHAPES[1], DIRECT_SMALL], ids=["staged", "direct"])
def test_deterministic_and_graph_replay(shape, pkg, torch_dev):
    torch, dev = torch_dev
    N, h, w, Ho, Wo, C, ld = shape
    c = ResizeCase(pkg, torch_dev, N, h, w, Ho, Wo, C, ld, seed=16)
    a, b = c.run(True, True), c.run(True, True)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
    x = c.src.to(dev)

    def run_out(out=None, workspace=None):
        return pkg.resize_bilinear(x, Ho, Wo, C=C, out=out)[0]

    def run_labels(out=None, workspace=None):
        return pkg.resize_bilinear(x, Ho, Wo, C=C, labels=out, want_out=False, want_labels=True)[1]

    eager = graph_replay_scenario(pkg, torch_dev, run_out, lambda: None, 0)
    assert np.array_equal(bits(eager.cpu().numpy()), bits(a[0]))
    eager = graph_replay_scenario(pkg, torch_dev, run_labels, lambda: None, 0)
    assert np.array_equal(eager.cpu().numpy(), a[1])
