"""GPU checks of the ResNet stem (wino_stem_hw: conv 7x7 s2 + BN + ReLU + max-pool 3x3 s2, one launch) and of the
classifier head (wino_avgpool_fc_hw).  Outputs go into NaN-filled buffers and are compared with fp64 references built
here (torch on the CPU): every shape class, both output layouts, negative BN scales, both forced forms, and a batch
whose input and output cross 2^32 bytes."""
import pytest

import layer_refs as LR
from gpu_support import torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu

TIGHT = 2e-5


def _stem_params(torch, K, seed, neg=True):
    g = torch.Generator().manual_seed(seed)
    w = (torch.rand(K, 3, 7, 7, generator=g, dtype=torch.float64) - 0.5) * 0.3
    scale = torch.rand(K, generator=g, dtype=torch.float64) + 0.5
    if neg:
        scale[::3] *= -1.0     # a negative scale turns the conv's minimum into the pool's maximum
    bias = torch.rand(K, generator=g, dtype=torch.float64) - 0.5
    return w, bias, scale


def _run_stem(pkg, torch, dev, x, w, bias, scale, padded):
    packed = pkg.stem_filter_pack(w.float().to(dev), (bias.float().to(dev), scale.float().to(dev)))
    N, _, H, W = x.shape
    Hp, Wp = pkg.stem_out_hw(H, W)
    p = 2 if padded else 0
    out = torch.full((N, Hp + p, Wp + p, w.shape[0]), float("nan"), device=dev)
    pkg.stem(x, packed, out_padded=padded, out=out)
    torch.cuda.synchronize()
    return out


def _check_stem(torch, got, want, padded):
    got = got.cpu().double()
    if padded:
        assert LR.ring_is(got, 0.0), "padded ring is not exactly 0"
        got = LR.interior(got)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert not torch.isnan(got).any(), "output not fully written"
    rel = LR.rel(got, want, floor=1e-30)
    assert rel < TIGHT, rel


CASES = [(1, 224, 224, 64), (2, 224, 224, 64), (33, 224, 224, 64), (1, 97, 131, 64), (2, 3, 5, 128), (1, 1, 1, 64),
         (1, 299, 299, 128), (4, 64, 48, 128)]


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("N,H,W,K", CASES)
def test_stem_matches_fp64(N, H, W, K, padded, pkg, torch_dev):
    torch, dev = torch_dev
    g = torch.Generator().manual_seed(N * 1000 + H + W + K)
    x = torch.rand(N, 3, H, W, generator=g) * 2 - 1
    w, bias, scale = _stem_params(torch, K, seed=H * W + K)
    got = _run_stem(pkg, torch, dev, x.to(dev), w, bias, scale, padded)
    _check_stem(torch, got, LR.stem(x, w, (bias, scale)), padded)


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("N,H,W,K,padded", [(1, 224, 224, 64, True), (3, 97, 131, 128, False),
                                            (2, 17, 9, 64, True), (40, 33, 35, 64, False)])
def test_stem_forced_forms(form, N, H, W, K, padded, pkg, torch_dev, knobs):
    """WINO_STEM_FORM forces each form on shapes whose automatic choice is the other one, too."""
    torch, dev = torch_dev
    knobs.set("WINO_STEM_FORM", form)
    assert pkg.stem_plan(N, H, W, K) == form
    x = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(7 + form)) * 2 - 1
    w, bias, scale = _stem_params(torch, K, seed=11 * form + H)
    got = _run_stem(pkg, torch, dev, x.to(dev), w, bias, scale, padded)
    _check_stem(torch, got, LR.stem(x, w, (bias, scale)), padded)


def test_stem_forms_agree_and_auto_picks_per_shape(pkg, torch_dev, knobs):
    torch, dev = torch_dev
    assert pkg.stem_plan(1, 224, 224, 64) == pkg.STEM_FORM_SMALL
    assert pkg.stem_plan(128, 224, 224, 64) == pkg.STEM_FORM_BIG
    x = (torch.rand(5, 3, 61, 77, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(dev)
    w, bias, scale = _stem_params(torch, 64, seed=5)
    outs = []
    for form in (1, 2):
        knobs.set("WINO_STEM_FORM", form)
        outs.append(_run_stem(pkg, torch, dev, x, w, bias, scale, False))
    # the same k order and BN in both forms: bitwise equal
    assert torch.equal(outs[0], outs[1])


def test_stem_past_4gib(pkg, torch_dev):
    """An input of 3.3 GB and an output of 4.3 GB (past 2^32 bytes): the first image, the last, and the ones whose
    output straddles byte 2^32."""
    torch, dev = torch_dev
    N, H, W, K = 5400, 224, 224, 64
    in_b, out_b = N * 3 * H * W * 4, N * 56 * 56 * K * 4
    assert out_b > 1 << 32
    free, _ = torch.cuda.mem_get_info()
    if free < in_b + out_b + (2 << 30):
        pytest.skip(f"needs {(in_b + out_b) / 2**30:.1f} GiB free, have {free / 2**30:.1f}")
    w, bias, scale = _stem_params(torch, K, seed=99)
    x = torch.empty(N, 3, H, W, device=dev)
    x.uniform_(-1, 1, generator=torch.Generator(device=dev).manual_seed(1))
    out = _run_stem(pkg, torch, dev, x, w, bias, scale, False)
    img_b = 56 * 56 * K * 4
    b = (1 << 32) // img_b
    for n in sorted({0, b - 1, b, b + 1, N - 1}):
        _check_stem(torch, out[n:n + 1], LR.stem(x[n:n + 1], w, (bias, scale)), False)
    del x, out
    torch.cuda.empty_cache()


# ---- head
@pytest.mark.parametrize("N,H,W,C,classes,padded", [(2, 7, 7, 512, 1000, True), (3, 7, 7, 2048, 1000, False),
                                                    (2, 7, 7, 512, 10, True), (1, 7, 7, 2048, 10, False),
                                                    (4, 4, 5, 512, 128, True), (5, 2, 3, 64, 1, False)])
def test_head_matches_fp64(N, H, W, C, classes, padded, pkg, torch_dev):
    torch, dev = torch_dev
    g = torch.Generator().manual_seed(N + C + classes)
    feat = torch.rand(N, H, W, C, generator=g, dtype=torch.float64) * 2
    wfc = (torch.rand(classes, C, generator=g, dtype=torch.float64) - 0.5) * 0.1
    bfc = torch.rand(classes, generator=g, dtype=torch.float64) - 0.5
    want = LR.avgpool_fc(feat, wfc, bfc)
    if padded:
        f = torch.full((N, H + 2, W + 2, C), float("nan"), dtype=torch.float64)   # the ring is not read
        f[:, 1:-1, 1:-1, :] = feat
    else:
        f = feat
    packed = pkg.head_pack(wfc.float().to(dev), bfc.float().to(dev))
    assert packed.numel() == pkg.lib().wino_head_elems(C, classes)
    out = torch.full((N, classes), float("nan"), device=dev)
    pkg.avgpool_fc(f.float().to(dev), packed, classes, in_padded=padded, out=out)
    torch.cuda.synchronize()
    got = out.cpu().double()
    assert not torch.isnan(got).any()
    rel = LR.rel(got, want)
    assert rel < TIGHT, rel
    assert pkg.tickets_in_use() == 0
