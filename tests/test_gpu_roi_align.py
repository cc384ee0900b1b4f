"""GPU tests of multi-scale RoIAlign (wino_roi_align_hw) against the fp64 reference of tests/roi_cases.py at cases.TIGHT
(tests/test_roi_host.py shows that a straight fp32 restatement of the arithmetic holds TIGHT / 4 on these inputs): the whole
box table at every (P, sampling, C) and layout, the exact-geometry subset at 1e-6, one level, the leak and non-finite
footprints, isolation of bad boxes, R = 0 and 1, an output past 4 GiB, graph replay and the wrappers.  Every run is on
the guarded arena at both alignments, into NaN-filled outputs, twice, bitwise equal."""
import pytest
import torch

import guarded
import roi_cases as rc
from cases import TIGHT
from gpu_support import graph_replay_scenario, torch_dev  # noqa: F401
from layer_refs import ring_is

pytestmark = pytest.mark.gpu
CANON = dict(canonical_scale=rc.CANONICAL_SCALE, canonical_level=rc.CANONICAL_LEVEL)


def bits(t):
    return t.contiguous().view(torch.int32)


def run(pkg, torch_dev, maps, rois, P, S, in_padded=False, out_padded=False, scales=rc.SCALES, aligns=guarded.ALIGNS,
        tag=""):
    """The kernel on CPU masters `maps` (unpadded; with in_padded they get a NaN ring) and `rois`, on the guarded arena at
    each of `aligns`, twice into a NaN-filled output; every run is bitwise the first.  Returns the output on the CPU."""
    _, dev = torch_dev
    src = [rc.padded_nan(m) for m in maps] if in_padded else maps
    q, R, C = (2 if out_padded else 0), rois.shape[0], maps[0].shape[3]
    first = None
    for align in aligns:
        arena = guarded.Arena(torch, dev, align)
        m = [arena.input(t, name=f"level{i}") for i, t in enumerate(src)]
        r = arena.input(rois, name="rois")
        out = arena.output(R, P + q, P + q, C, name="out")
        for _ in range(2):
            out.fill_(float("nan"))
            got = pkg.roi_align(m, r, P, scales, S, in_padded, out_padded, out=out, **CANON)
            assert got is out
            arena.check(f"roi_align {tag} P={P} S={S} C={C} padded={in_padded}/{out_padded} align={align}")
            cpu = out.cpu()
            if first is None:
                first = cpu
            assert torch.equal(bits(cpu), bits(first)), f"{tag}: not bitwise reproducible (align {align})"
    return first


def interior(got, out_padded):
    """The P x P interior of an output; a padded output's ring is exactly 0."""
    if not out_padded:
        return got
    assert ring_is(got, 0.0), "the ring is not exactly 0"
    return got[:, 1:-1, 1:-1, :]


LAYOUTS = [(False, False), (True, False), (False, True), (True, True)]


@pytest.mark.parametrize("C", rc.CHANNELS)
@pytest.mark.parametrize("P,S", rc.PS_COMBOS)
def test_parity_of_the_whole_table(P, S, C, pkg, torch_dev):
    bx, want, maps = rc.boxes(0), rc.reference(C, P, S), rc.pyramid(C)
    for in_padded, out_padded in LAYOUTS:
        got = interior(run(pkg, torch_dev, maps, bx.rois, P, S, in_padded, out_padded, tag="table"), out_padded)
        err = rc.rel_err(got, want)
        print(f"table P={P} S={S} C={C} padded={in_padded}/{out_padded}: {err:.2e}")
        assert err < TIGHT


@pytest.mark.parametrize("C", [64, 320])
@pytest.mark.parametrize("P,S", rc.EXACT_COMBOS)
def test_exact_geometry_subset(P, S, C, pkg, torch_dev):
    bx, want, maps = rc.boxes(0), rc.reference(C, P, S, only="exact"), rc.pyramid(C)
    rois = bx.rois[bx.index("exact")]
    for in_padded, out_padded in LAYOUTS:
        got = interior(run(pkg, torch_dev, maps, rois, P, S, in_padded, out_padded, tag="exact"), out_padded)
        err = rc.rel_err(got, want)
        print(f"exact P={P} S={S} C={C} padded={in_padded}/{out_padded}: {err:.2e}")
        assert err < rc.EXACT_TOL


@pytest.mark.parametrize("scale", [0.25, 0.3])
@pytest.mark.parametrize("P,S", [(7, 2), (14, 3), (1, 1)])
def test_one_level(P, S, scale, pkg, torch_dev):
    """levels = 1: every box takes level 0, whatever its area, at a power-of-two scale and at 0.3.  The boxes are the
    table's that keep the sample margin on this one map (the table was drawn for its own levels)."""
    bx, maps = rc.boxes(0), rc.pyramid(64)[:1]
    zeros = torch.zeros(len(bx.names), dtype=torch.int64)
    keep = rc.min_sample_margin(bx.rois, zeros, [(P, S)], hw=rc.LEVEL_HW[:1], scales=(scale,)) >= rc.SAMPLE_MARGIN
    assert int(keep.sum()) >= 0.8 * len(bx.names)
    rois = bx.rois[keep]
    want = rc.roi_align_reference(maps, rois, P, (scale,), S, zeros[keep])
    for in_padded, out_padded in LAYOUTS:
        got = interior(run(pkg, torch_dev, maps, rois, P, S, in_padded, out_padded, scales=(scale,), tag="one level"),
                       out_padded)
        err = rc.rel_err(got, want)
        print(f"one level scale={scale} P={P} S={S} padded={in_padded}/{out_padded}: {err:.2e}")
        assert err < TIGHT


@pytest.mark.parametrize("level,n,y,x,k,C", [(0, 0, 5, 3, 7, 64), (0, 1, 13, 11, 300, 320), (1, 1, 2, 3, 0, 64),
                                             (2, 0, 1, 1, 63, 64), (3, 1, 1, 0, 9, 64), (3, 0, 0, 1, 257, 320)])
def test_leak_one_hot(level, n, y, x, k, C, pkg, torch_dev):
    """A single 1 in one channel of one image of one level: exactly the outputs whose fp64 reference is non-zero are
    non-zero, and no box of the other image sees it."""
    bx = rc.boxes(0)
    maps = [torch.zeros(rc.N_IMAGES, h, w, C) for h, w in rc.LEVEL_HW]
    maps[level][n, y, x, k] = 1.0
    for P, S in ((7, 2), (14, 3)):
        want = rc.roi_align_reference(maps, bx.rois, P, rc.SCALES, S, bx.levels)
        lit = want != 0
        assert int(lit.sum()) > 0 and not bool(lit[bx.rois[:, 0] != n].any()) and not bool(lit[bx.levels != level].any())
        for in_padded, out_padded in ((False, False), (True, True)):
            got = interior(run(pkg, torch_dev, maps, bx.rois, P, S, in_padded, out_padded, tag="leak"), out_padded)
            assert torch.equal(got != 0, lit), f"P={P} S={S}: {int(((got != 0) != lit).sum())} outputs differ"
            assert not bool((got[bx.rois[:, 0] != n] != 0).any())
            err = rc.rel_err(got, want)
            print(f"leak level={level} P={P} S={S}: {int(lit.sum())} outputs lit, {err:.2e}")
            assert err < TIGHT


@pytest.mark.parametrize("level,n,y,x,k", [(0, 1, 8, 6, 5), (1, 0, 3, 2, 40), (3, 0, 1, 1, 63)])
def test_nan_pixel_footprint(level, n, y, x, k, pkg, torch_dev):
    """A NaN pixel changes exactly the outputs whose reference taps it -- a tap of weight zero included -- and every other
    output keeps the clean run's bits."""
    bx, maps, C = rc.boxes(0), rc.pyramid(64), 64
    dirty = [m.clone() for m in maps]
    dirty[level][n, y, x, k] = float("nan")
    for P, S in ((7, 2), (14, 1)):
        _, touched = rc.roi_align_reference(maps, bx.rois, P, rc.SCALES, S, bx.levels, taps=True)
        hit = torch.zeros(len(bx.names), P, P, C, dtype=torch.bool)
        for r, t in enumerate(touched):
            if t is not None and t[0] == level and t[1] == n:
                hit[r, :, :, k] = t[2][:, y][:, None] & t[3][:, x][None, :]
        assert int(hit.sum()) > 0
        for in_padded, out_padded in ((False, False), (True, True)):
            clean = interior(run(pkg, torch_dev, maps, bx.rois, P, S, in_padded, out_padded, aligns=(256,)), out_padded)
            got = interior(run(pkg, torch_dev, dirty, bx.rois, P, S, in_padded, out_padded, tag="nan"), out_padded)
            assert torch.equal(torch.isnan(got), hit), f"P={P} S={S}: NaN set differs in {int((torch.isnan(got) != hit).sum())}"
            assert torch.equal(bits(got)[~hit], bits(clean)[~hit])
        print(f"nan pixel level={level} P={P} S={S}: {int(hit.sum())} outputs")


@pytest.mark.parametrize("out_padded", [False, True])
def test_bad_boxes_are_isolated(out_padded, pkg, torch_dev):
    """Batch indices -1, N, 0.5 and NaN give zeros; a NaN or Inf coordinate gives NaN for that box alone; the other
    boxes are bitwise what they are without the bad boxes."""
    bx, maps, P, S = rc.boxes(0), rc.pyramid(64), 7, 2
    nan, inf = float("nan"), float("inf")
    clean = run(pkg, torch_dev, maps, bx.rois, P, S, True, out_padded, aligns=(256,))
    rois = bx.rois.clone()
    R = rois.shape[0]
    zero_at = {3: -1.0, 17: float(rc.N_IMAGES), 29: 0.5, 41: nan, R - 1: 1e9}
    nan_at = {0: (1, nan), 11: (2, inf), 23: (3, -inf), 37: (4, nan), 52: (1, inf)}
    for r, v in zero_at.items():
        rois[r, 0] = v
    for r, (col, v) in nan_at.items():
        rois[r, col] = v
    rois[41, 2] = nan                                  # a bad image index and a bad coordinate: zeros
    got = run(pkg, torch_dev, maps, rois, P, S, True, out_padded, tag="bad boxes")
    inner = interior(got, out_padded)                   # (checks the ring of every box, the bad ones included)
    for r in zero_at:
        assert bool((got[r] == 0).all()), r
    for r in nan_at:
        assert bool(torch.isnan(inner[r]).all()), r
    others = [r for r in range(R) if r not in zero_at and r not in nan_at]
    assert torch.equal(bits(got[others]), bits(clean[others]))


def test_no_boxes_and_one_box(pkg, torch_dev):
    _, dev = torch_dev
    bx, maps = rc.boxes(0), rc.pyramid(8)
    m = [t.to(dev) for t in maps]
    for out_padded in (False, True):
        out = pkg.roi_align(m, torch.zeros(0, 5, device=dev), 7, rc.SCALES, out_padded=out_padded, **CANON)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (0, 7 + 2 * out_padded, 7 + 2 * out_padded, 8)
    for r in (bx.index("interior_l2")[0], bx.index("clamp_right")[1]):
        want = rc.reference(8, 7, 2)[r:r + 1]
        for in_padded, out_padded in LAYOUTS:
            got = interior(run(pkg, torch_dev, maps, bx.rois[r:r + 1], 7, 2, in_padded, out_padded, tag="R=1"), out_padded)
            assert rc.rel_err(got, want) < TIGHT


def test_output_past_4gib(pkg, torch_dev):
    """One 4 x 3 level, C = 1024, P = 32 padded, 908 equal boxes: out is 4.3 GB, every box from its own 64-bit base.
    Every box's output is bitwise box 0's (compared on the device) and box 0 holds TIGHT against fp64."""
    _, dev = torch_dev
    C, P, scale = 1024, 32, 0.25
    box_bytes = (P + 2) * (P + 2) * C * 4
    R = (1 << 32) // box_bytes + 2
    assert R * box_bytes > 1 << 32
    g = torch.Generator().manual_seed(5)
    fmap = torch.rand(2, 4, 3, C, generator=g) - 0.5
    roi = torch.tensor([[1, 1.3, 0.9, 10.7, 14.2]])
    zeros = torch.zeros(1, dtype=torch.int64)
    assert float(rc.min_sample_margin(roi, zeros, [(P, 2)], hw=((4, 3),), scales=(scale,))) >= rc.SAMPLE_MARGIN
    want = rc.roi_align_reference([fmap], roi, P, (scale,), 2, zeros)
    out = torch.full((R, P + 2, P + 2, C), float("nan"), device=dev)
    pkg.roi_align(fmap.to(dev), roi.to(dev).repeat(R, 1), P, scale, 2, out_padded=True, out=out)
    torch.cuda.synchronize()
    first = out[0].view(torch.int32)
    for r0 in range(0, R, 128):
        assert bool((out[r0:r0 + 128].view(torch.int32) == first).all()), f"boxes {r0}.. differ from box 0"
    got = interior(out[:1].cpu(), True)
    del out
    err = rc.rel_err(got, want)
    print(f"past 4 GiB: R={R}: box 0 {err:.2e}")
    assert err < TIGHT


@pytest.mark.parametrize("out_padded", [False, True])
def test_graph_replay_without_prepare(out_padded, pkg, torch_dev):
    _, dev = torch_dev
    bx = rc.boxes(0)
    m, r = [rc.padded_nan(t).to(dev) for t in rc.pyramid(64)], bx.rois.to(dev)

    def launch(out=None, workspace=None):
        return pkg.roi_align(m, r, 14, rc.SCALES, 2, True, out_padded, out=out, **CANON)

    eager = graph_replay_scenario(pkg, torch_dev, launch, lambda: None, 0)
    assert rc.rel_err(interior(eager.cpu(), out_padded), rc.reference(64, 14, 2)) < TIGHT


def test_wrappers(pkg, torch_dev):
    """multiscale_roi_align: the list-of-boxes form equals the [K, 5] form, the inferred scales the explicit ones."""
    _, dev = torch_dev
    bx, maps = rc.boxes(0), rc.pyramid(64)
    assert tuple(pkg.infer_roi_scales(maps, rc.IMAGE)) == rc.SCALES
    assert tuple(pkg.infer_roi_scales([rc.padded_nan(t) for t in maps], rc.IMAGE, in_padded=True)) == rc.SCALES
    per_image = [bx.rois[bx.rois[:, 0] == n] for n in range(rc.N_IMAGES)]
    k5 = torch.cat(per_image).to(dev)
    as_list = [b[:, 1:].to(dev) for b in per_image]
    assert torch.equal(pkg.boxes_to_rois(as_list), k5) and pkg.boxes_to_rois(k5) is k5
    m = [t.to(dev) for t in maps]
    mp = [rc.padded_nan(t).to(dev) for t in maps]
    for P, out_padded in ((7, False), (14, True)):
        want = pkg.roi_align(m, k5, P, rc.SCALES, 2, out_padded=out_padded, **CANON)
        for feats, in_padded in ((m, False), (mp, True), ({str(i): t for i, t in enumerate(mp)} | {"pool": m[3]}, True)):
            for boxes in (k5, as_list):
                got = pkg.multiscale_roi_align(feats, boxes, rc.IMAGE, P, 2, in_padded, out_padded, **CANON)
                assert torch.equal(bits(got), bits(want))
    with pytest.raises(pkg.WinoError, match="different scales"):
        pkg.infer_roi_scales([torch.zeros(1, 16, 24, 8)], rc.IMAGE)       # 1/4 along y, 1/2 along x
    with pytest.raises(pkg.WinoError, match="rc=-3"):
        pkg.roi_align(m, k5, 7, (0.25, 0.125, 0.0625, 0.0625), **CANON)
