"""GPU sweep of multi-scale RoIAlign (wino_roi_align_hw) over the cases of roi_cases.roi_sweep_cases(): every sampling
1..4 (each launch_roi<S>), 1 to 4 levels, k0 0..5, 1 to 5 images, ceil-sized and one-pixel level maps, P up to the header's
64, channel counts around the 256-channel slab, all four layouts, other canonical values and the wrapper's defaults --
against the fp64 reference at cases.TIGHT (tests/test_roi_host.py shows that the fp32 restatement holds TIGHT / 4 on every
case).  Then what the fixed table of tests/test_gpu_roi_align.py leaves out: the exact-geometry subset, the one-hot leak
and the NaN footprint at sampling 4 and with two levels; a level map past 2^31 elements; and the loop that splits a call
into several launches, forced by the developer knob WINO_ROI_LAUNCH_TASKS.  Every run writes a NaN-filled output twice
and must repeat bit for bit; the sweep and the table runs lie on the guarded arena at both alignments."""
import collections

import pytest
import torch

import guarded
import roi_cases as rc
from cases import TIGHT
from gpu_support import torch_dev  # noqa: F401
from layer_refs import ring_is

pytestmark = pytest.mark.gpu
CANON = dict(canonical_scale=rc.CANONICAL_SCALE, canonical_level=rc.CANONICAL_LEVEL)
CHECKS = collections.Counter()      # arena checks that passed, by the test that asked


def bits(t):
    return t.contiguous().view(torch.int32)


def run(pkg, torch_dev, maps, rois, P, S, in_padded, out_padded, scales, canon, image=None, aligns=guarded.ALIGNS,
        tag="", count="other"):
    """The kernel on CPU masters `maps` (unpadded; with in_padded they get a NaN ring) and `rois`, on the guarded arena at
    each of `aligns`: two launches into a NaN-filled output of exactly its size, then one arena.check; every launch is
    bitwise the first.  canon = None goes through multiscale_roi_align with nothing but the image size: the scales
    inferred, the canonical values the wrapper's defaults.  Returns the output on the CPU."""
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
            if canon is None:
                got = pkg.multiscale_roi_align(m, r, image, P, S, in_padded, out_padded, out=out)
            else:
                got = pkg.roi_align(m, r, P, scales, S, in_padded, out_padded, out=out, **canon)
            assert got is out
            cpu = out.cpu()
            if first is None:
                first = cpu
            assert torch.equal(bits(cpu), bits(first)), f"{tag}: not bitwise reproducible (align {align})"
        arena.check(f"roi_align {tag} P={P} S={S} C={C} padded={in_padded}/{out_padded} align={align}")
        CHECKS[count] += 1
    return first


def interior(got, out_padded):
    """The P x P interior of an output; a padded output's ring is exactly 0."""
    if not out_padded:
        return got
    assert ring_is(got, 0.0), "the ring is not exactly 0"
    return got[:, 1:-1, 1:-1, :]


def test_roi_align_sweep(pkg, torch_dev):
    """Every case of roi_sweep_cases() at both placements.  Measured worst error against fp64: see DESIGN.md 3.2m."""
    cases = rc.roi_sweep_cases()
    before, seen, worst = CHECKS["sweep"], collections.defaultdict(set), 0.0
    for c in cases:
        geo, gb, want = c.geo, rc.case_boxes(c), rc.case_reference(c)
        got = run(pkg, torch_dev, rc.case_pyramid(c), gb.rois, c.P, c.S, c.in_padded, c.out_padded, geo.scales,
                  None if c.defaults else geo.canon, image=geo.image, tag=c.name, count="sweep")
        got = interior(got, c.out_padded)
        huge = gb.index("huge")
        good = [r for r in range(len(gb.names)) if r not in huge]
        assert not bool(torch.isnan(got[good]).any()), f"{c.name}: NaN in a good box"
        assert bool((got[huge] == 0).all()), f"{c.name}: a huge box is not zeros"
        err = rc.rel_err(got, want)
        worst = max(worst, err)
        print(f"{c.name} levels={geo.levels} k0={geo.k0} N={geo.N} finest={geo.hw[0]} P={c.P} S={c.S} C={c.C} "
              f"padded={c.in_padded}/{c.out_padded} defaults={c.defaults}: {err:.2e}")
        assert err < TIGHT, c.name
        for key, v in (("S", c.S), ("levels", geo.levels), ("P", c.P), ("defaults", c.defaults)):
            seen[key].add(v)
        if geo.levels > 1:
            seen["k0"].add(geo.k0)
    print(f"roi_align sweep: {len(cases)} cases, worst rel err {worst:.2e}")
    done = CHECKS["sweep"] - before
    assert done == 2 * len(cases), f"{done} guard checks for {len(cases)} cases at two placements"
    assert seen["S"] == {1, 2, 3, 4} and seen["levels"] == {1, 2, 3, 4} and 64 in seen["P"]
    assert seen["defaults"] == {False, True} and seen["k0"] - {2}
    assert pkg.tickets_in_use() == 0


@pytest.mark.parametrize("C", [64, 320])
@pytest.mark.parametrize("P", [2, 4, 8])
def test_exact_geometry_subset_at_sampling_4(P, C, pkg, torch_dev):
    """Edges on multiples of the level's stride, P a power of two, sampling 4: every sample is still dyadic."""
    bx, S = rc.boxes(0), 4
    assert (P, S) in rc.EXACT_COMBOS_S4
    want, maps = rc.reference(C, P, S, only="exact"), rc.pyramid(C)
    rois = bx.rois[bx.index("exact")]
    for in_padded, out_padded in ((False, False), (True, False), (False, True), (True, True)):
        got = interior(run(pkg, torch_dev, maps, rois, P, S, in_padded, out_padded, rc.SCALES, CANON, tag="exact"), out_padded)
        err = rc.rel_err(got, want)
        print(f"exact P={P} S={S} C={C} padded={in_padded}/{out_padded}: {err:.2e}")
        assert err < rc.EXACT_TOL
    assert pkg.tickets_in_use() == 0


# (levels, the (P, sampling) pairs, the lit / poisoned pixel: level, image, y, x, channel, C)
VARIANTS = {"sampling_4": (4, ((7, 4), (14, 4)), (0, 1, 13, 11, 300, 320)),
            "two_levels": (2, ((7, 2), (14, 3)), (1, 0, 3, 2, 9, 64))}


def table_on(levels, P, S):
    """The table's boxes on its first `levels` levels, those that keep the sample margin at (P, S) there (the table was
    drawn for four levels and sampling <= 3) and have no sample within 1e-6 of a whole pixel coordinate: there a tap's
    weight is zero up to rounding, and whether it is exactly zero is decided by the last bit, in the fp64 reference as
    much as in the kernel (the reference gives 1.6e-16 for one such tap), so "non-zero" means nothing for that output.
    Returns (rois, their levels, hw, scales)."""
    bx, hw, scales = rc.boxes(0), rc.LEVEL_HW[:levels], rc.SCALES[:levels]
    lv = rc.torchvision_levels(bx.rois, scales)
    assert torch.equal(lv, rc.threshold_levels(bx.rois, scales))
    keep = rc.min_sample_margin(bx.rois, lv, [(P, S)], hw=hw, scales=scales) >= rc.SAMPLE_MARGIN
    ys, xs = rc.sample_coords(bx.rois, torch.tensor(scales, dtype=torch.float64)[lv], P, S)
    for v, size in ((ys, 0), (xs, 1)):
        v = v.flatten(1)
        top = torch.tensor([s[size] for s in hw], dtype=torch.float64)[lv][:, None]
        on_pixel = ((v - v.round()).abs() < 1e-6) & (v > 0) & (v < top - 1)
        keep &= ~on_pixel.any(dim=1)
    assert int(keep.sum()) >= 0.7 * len(bx.names) and set(lv[keep].tolist()) == set(range(levels))
    assert set(bx.rois[keep, 0].tolist()) == {0.0, 1.0}
    return bx.rois[keep], lv[keep], hw, scales


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_leak_one_hot(variant, pkg, torch_dev):
    """A single 1 in one channel of one image of one level: exactly the outputs whose fp64 reference is non-zero are
    non-zero, and no box of another image or level sees it."""
    levels, combos, (level, n, y, x, k, C) = VARIANTS[variant]
    for P, S in combos:
        rois, lv, hw, scales = table_on(levels, P, S)
        maps = [torch.zeros(rc.N_IMAGES, h, w, C) for h, w in hw]
        maps[level][n, y, x, k] = 1.0
        want = rc.roi_align_reference(maps, rois, P, scales, S, lv)
        lit = want != 0
        assert int(lit.sum()) > 0 and not bool(lit[rois[:, 0] != n].any()) and not bool(lit[lv != level].any())
        for in_padded, out_padded in ((False, False), (True, True)):
            got = interior(run(pkg, torch_dev, maps, rois, P, S, in_padded, out_padded, scales, CANON, tag="leak"), out_padded)
            assert torch.equal(got != 0, lit), f"P={P} S={S}: {int(((got != 0) != lit).sum())} outputs differ"
            err = rc.rel_err(got, want)
            print(f"leak {variant} P={P} S={S}: {int(lit.sum())} outputs lit, {err:.2e}")
            assert err < TIGHT
    assert pkg.tickets_in_use() == 0


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_nan_pixel_footprint(variant, pkg, torch_dev):
    """A NaN pixel changes exactly the outputs whose reference taps it -- a tap of weight zero included -- and every other
    output keeps the clean run's bits."""
    levels, combos, (level, n, y, x, k, C) = VARIANTS[variant]
    for P, S in combos:
        rois, lv, hw, scales = table_on(levels, P, S)
        maps = rc.pyramid(C)[:levels]
        dirty = [m.clone() for m in maps]
        dirty[level][n, y, x, k] = float("nan")
        _, touched = rc.roi_align_reference(maps, rois, P, scales, S, lv, taps=True)
        hit = torch.zeros(rois.shape[0], P, P, C, dtype=torch.bool)
        for r, t in enumerate(touched):
            if t is not None and t[0] == level and t[1] == n:
                hit[r, :, :, k] = t[2][:, y][:, None] & t[3][:, x][None, :]
        assert int(hit.sum()) > 0
        for in_padded, out_padded in ((False, False), (True, True)):
            clean = interior(run(pkg, torch_dev, maps, rois, P, S, in_padded, out_padded, scales, CANON, aligns=(256,)),
                             out_padded)
            got = interior(run(pkg, torch_dev, dirty, rois, P, S, in_padded, out_padded, scales, CANON, tag="nan"), out_padded)
            assert torch.equal(torch.isnan(got), hit), f"P={P} S={S}: NaN set differs in {int((torch.isnan(got) != hit).sum())}"
            assert torch.equal(bits(got)[~hit], bits(clean)[~hit])
        print(f"nan pixel {variant} P={P} S={S}: {int(hit.sum())} outputs")
    assert pkg.tickets_in_use() == 0


@pytest.mark.parametrize("in_padded", [False, True])
def test_input_map_past_2gi_elements(in_padded, pkg, torch_dev):
    """One level at scale 1/4, C = 1024, 2049 images of 2^20 elements each (30 x 30 pixels in a ring, or 32 x 32 without
    one): 2^31 + 2^20 elements, 8.6 GB.  Image 1024 starts at byte 4 GiB, image 2048 at element 2^31; boxes in images
    0, 1023, 1024, 2047 and 2048 are held against the fp64 reference of those five images at TIGHT.  A wrong image base
    reads another image's finite data, an O(1) error.  It stops here: a map past 2^32 elements is 17 GB on a machine that
    others share, and the one product that forms the base is written in size_t, so an unsigned 32-bit slip would be a
    different expression from the one in the kernel, not a case this one misses."""
    _, dev = torch_dev
    C, N, P, S, scale = 1024, 2049, 7, 2, 0.25
    side = 30 if in_padded else 32
    full = side + 2 * in_padded
    assert full * full * C == 1 << 20 and N * full * full * C == (1 << 31) + (1 << 20)
    images = (0, 1023, 1024, 2047, 2048)
    px = side / scale
    shapes = ((20.3, 30.1, 60.7, 71.9), (px - 14.3, px - 12.1, px - 0.9, px - 1.3), (-2.1, -1.7, 9.3, 11.2))
    rows = [[float(n), *shapes[(i + j) % 3]] for i, n in enumerate(images) for j in range(3)] + [[2048.0, *shapes[0]]]
    rois = torch.tensor(rows, dtype=torch.float32)
    zeros = torch.zeros(len(rows), dtype=torch.int64)
    assert float(rc.min_sample_margin(rois, zeros, [(P, S)], hw=((side, side),), scales=(scale,)).min()) >= rc.SAMPLE_MARGIN
    fmap = None
    try:
        fmap = torch.empty((N, full, full, C), dtype=torch.float32, device=dev)
        g = torch.Generator(device=dev).manual_seed(17)
        for n0 in range(0, N, 128):
            n1 = min(n0 + 128, N)
            fmap[n0:n1] = torch.rand((n1 - n0, full, full, C), generator=g, device=dev)
        if in_padded:
            for ring in (fmap[:, 0], fmap[:, -1], fmap[:, :, 0], fmap[:, :, -1]):
                ring.fill_(float("nan"))
        inner = (lambda t: t[:, 1:-1, 1:-1, :]) if in_padded else (lambda t: t)
        host = torch.stack([inner(fmap[n:n + 1])[0].cpu() for n in images])          # the reference sees these five only
        ref_rois = rois.clone()
        ref_rois[:, 0] = torch.tensor([float(images.index(int(v))) for v in rois[:, 0].tolist()])
        want = rc.roi_align_reference([host], ref_rois, P, (scale,), S, zeros)
        r = rois.to(dev)
        out = torch.empty((len(rows), P, P, C), dtype=torch.float32, device=dev)
        first = None
        for _ in range(2):
            out.fill_(float("nan"))
            pkg.roi_align(fmap, r, P, scale, S, in_padded, out=out)
            torch.cuda.synchronize()
            first = out.cpu() if first is None else first
            assert torch.equal(bits(out.cpu()), bits(first))
    finally:
        del fmap
        torch.cuda.empty_cache()
    for n in images:
        sel = [i for i, row in enumerate(rows) if row[0] == n]
        print(f"map past 2^31 elements, in_padded={in_padded}, image {n}: {rc.rel_err(first[sel], want[sel]):.2e}")
    assert rc.rel_err(first, want) < TIGHT
    assert pkg.tickets_in_use() == 0


@pytest.mark.parametrize("P,S,padded", [(7, 2, True), (1, 2, False)])
def test_split_launch_loop(P, S, padded, pkg, knobs, torch_dev):
    """The loop that cuts a call at 2^31 output positions into launches of whole boxes, each with its own rois and out
    base, cut here by WINO_ROI_LAUNCH_TASKS into 8 launches of 12 boxes, the last of 4: bitwise the one launch."""
    bx, maps, C = rc.boxes(0), rc.pyramid(64), 64
    R, QQ = len(bx.names), (P + 2 * padded) ** 2
    knobs.unset("WINO_ROI_LAUNCH_TASKS")
    assert pkg.roi_align_launches(R, P, padded) == 1
    whole = run(pkg, torch_dev, maps, bx.rois, P, S, padded, padded, rc.SCALES, CANON, tag="one launch")
    knobs.set("WINO_ROI_LAUNCH_TASKS", 12 * QQ + QQ // 2)
    assert pkg.roi_align_launches(R, P, padded) == 8 and R == 7 * 12 + 4
    split = run(pkg, torch_dev, maps, bx.rois, P, S, padded, padded, rc.SCALES, CANON, tag="eight launches")
    knobs.unset("WINO_ROI_LAUNCH_TASKS")
    assert torch.equal(bits(split), bits(whole))
    err = rc.rel_err(interior(split, padded), rc.reference(C, P, S))
    print(f"split launch P={P} S={S} padded={padded}: {err:.2e}")
    assert err < TIGHT
    assert pkg.tickets_in_use() == 0
