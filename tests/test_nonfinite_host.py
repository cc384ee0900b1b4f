"""The oracle of tests/test_gpu_nonfinite.py proved before it is trusted on the GPU, no GPU: for every layer kind, at
the GPU test's shapes, each poison of the plan is put into the fp64 torch reference (F.conv2d / max_pool2d /
interpolate on the CPU) and the reference's non-finite set must lie inside the footprint that tests/nonfinite.py
declares; with a NaN it must equal the receptive field exactly (for the F(2x2) layers the 3x3 window, which lies inside
the declared tile footprint; for every other kind the footprint itself).  The seeded draw keeps its cap and its
mandatory poisons; the checker fails on each fault it is there to find."""
import pytest
import torch

import nonfinite as NF

LAYERS = list(NF.all_layers(torch))
BLOCKS = list(NF.blocks(torch))


def _nonfinite(layer, p):
    return ~torch.isfinite(layer.ref(layer.poisoned(p)))


@pytest.mark.parametrize("layer", LAYERS, ids=[l.tag.replace(" ", "_") for l in LAYERS])
def test_reference_stays_inside_the_footprint(layer):
    boundary, params, rest = NF.candidates(layer)
    seen = 0
    for p in boundary + params + rest:
        nf, mask = _nonfinite(layer, p), layer.footprint(p)
        assert nf.shape == mask.shape == tuple(layer.out_shape), (layer.tag, p.tag())
        assert not bool((nf & ~mask).any()), f"{layer.tag} {p.tag()}: the reference is non-finite outside the footprint"
        if not layer.single_pixel:
            assert not bool(mask.all()), f"{layer.tag} {p.tag()}: the footprint is the whole output"
        if p.value != p.value:
            field = layer.receptive_field(p) if p.where != "param" else mask
            assert bool((field & ~mask).sum() == 0), f"{layer.tag} {p.tag()}: the field leaves the footprint"
            assert bool(torch.equal(nf, field)), \
                f"{layer.tag} {p.tag()}: NaN set {int(nf.sum())} != receptive field {int(field.sum())}"
            seen += 1
        else:
            assert bool(nf.any()), f"{layer.tag} {p.tag()}: an infinity that the reference never shows"
    assert seen >= 2


@pytest.mark.parametrize("layer", LAYERS, ids=[l.tag.replace(" ", "_") for l in LAYERS])
def test_draw_keeps_its_cap_and_its_mandatory_poisons(layer):
    ps = NF.check_draw(layer, seed=17)
    assert ps != NF.draw(layer, seed=18)
    clean = layer.ref(layer.t)
    assert bool(torch.isfinite(clean).all())


@pytest.mark.parametrize("block", BLOCKS, ids=NF.BLOCKS)
def test_block_reference_stays_inside_the_poisoned_image(block):
    """The fp64 composition of every block: clean inputs give a finite output, every poison of the plan shows, and only
    in its own image."""
    assert bool(torch.isfinite(block.ref(block.t)).all())
    boundary, params, rest = NF.candidates(block)
    assert not params and len(boundary) >= 2
    for p in boundary + rest:
        nf, mask = _nonfinite(block, p), block.footprint(p)
        assert nf.shape == mask.shape == tuple(block.out_shape), (block.tag, p.tag())
        assert bool(nf.any()) and not bool((nf & ~mask).any()) and not bool(mask.all()), (block.tag, p.tag())
    NF.check_draw(block, seed=17)


def test_interval_arithmetic_at_the_edges():
    assert NF.conv_rows(0, 5, 3, 1, 1) == (0, 1) and NF.conv_rows(4, 5, 3, 1, 1) == (3, 4)
    assert NF.conv_rows(8, 5, 3, 2, 1) == (4, 4) and NF.conv_rows(1, 5, 3, 2, 1) == (0, 1)
    assert NF.conv_rows(1, 3, 1, 2, 0) is None and NF.conv_rows(2, 3, 1, 2, 0) == (1, 1)
    assert NF.wino_rows(0, 7) == (0, 1) and NF.wino_rows(1, 7) == (0, 3) and NF.wino_rows(6, 7) == (4, 6)
    assert NF.wino_pool_rows(6, 7) == (2, 2) and NF.wino_pool_rows(0, 2) == (0, 0)
    assert NF.up2_rows(3, 7) == (6, 6) and NF.up2_rows(0, 1) == (0, 0)
    assert NF.stem_rows(0, 224) == (0, 1) and NF.stem_rows(0, 1) == (0, 0)
    assert NF.adaptive_bins(0, 1) == (0, 6) and NF.adaptive_bins(13, 14) == (6, 6)


def _case():
    want = torch.zeros(2, 4, 4, 8, dtype=torch.float64)
    mask = NF.box(torch, want.shape, 1, (1, 2), (1, 2))
    want[1, 1:3, 1:3, :] = NF.NAN
    want[1, 1, 1, 0] = NF.INF
    clean = torch.zeros(want.shape)
    got = want.float()
    return clean, got, want, mask


def test_checker_passes_and_fails_where_it_should():
    clean, got, want, mask = _case()
    NF.check_poisoned(torch, clean, got, want, mask, 2e-5, "ok")
    g = got.clone(); g[1, 2, 2, 3] = 0.0                       # a swallowed NaN
    with pytest.raises(AssertionError, match="reference NaNs are not NaN"):
        NF.check_poisoned(torch, clean, g, want, mask, 2e-5, "swallowed")
    g = got.clone(); g[0, 3, 3, 7] = -0.0                      # one bit outside the footprint
    with pytest.raises(AssertionError, match="outside the footprint differ"):
        NF.check_poisoned(torch, clean, g, want, mask, 2e-5, "leak")
    g = got.clone(); g[1, 1, 1, 0] = -NF.INF                   # the other infinity
    with pytest.raises(AssertionError, match="reference Infs"):
        NF.check_poisoned(torch, clean, g, want, mask, 2e-5, "sign")
    g = got.clone(); g[1, 1, 1, 0] = NF.NAN                    # Inf - Inf: a Winograd kernel may, a direct one may not
    NF.check_poisoned(torch, clean, g, want, mask, 2e-5, "winograd")
    with pytest.raises(AssertionError, match="reference Infs"):
        NF.check_poisoned(torch, clean, g, want, mask, 2e-5, "direct", exact_inf=True)
    w = want.clone(); w[1, 1, 2, :] = 1.0                      # the band: finite reference inside the footprint
    g = got.clone(); g[1, 1, 2, :] = 1.0; g[1, 1, 2, 1] = NF.NAN
    NF.check_poisoned(torch, clean, g, w, mask, 2e-5, "band")
    g[1, 1, 2, 2] = 1.001
    with pytest.raises(AssertionError, match="inside the footprint are off"):
        NF.check_poisoned(torch, clean, g, w, mask, 2e-5, "third outcome")
    with pytest.raises(AssertionError, match="the poison did nothing"):
        NF.check_poisoned(torch, clean, clean, torch.zeros_like(want), mask, 2e-5, "nothing")
    with pytest.raises(AssertionError, match="containment was not compared"):
        NF.check_poisoned(torch, clean, got, want, torch.ones_like(mask), 2e-5, "vacuous")
    g = got.clone(); g[1, 1, 1, 0] = -NF.INF; g[1, 2, 2, 3] = NF.INF   # a weak poison: any non-finite value will do
    NF.check_poisoned(torch, clean, g, want, mask, 2e-5, "weak", any_nonfinite=True)
    g[1, 2, 2, 3] = 0.0
    with pytest.raises(AssertionError, match="are finite in the output"):
        NF.check_poisoned(torch, clean, g, want, mask, 2e-5, "weak, swallowed", any_nonfinite=True)
    w = want.clone(); w[0, 0, 0, 0] = NF.NAN
    with pytest.raises(AssertionError, match="outside the declared footprint"):
        NF.check_poisoned(torch, clean, got, w, mask, 2e-5, "oracle")
