"""The pooled 3x3 layer (conv3x3_bn_relu_pool) and the two VGG kernels around it (image_pack, avgpool7_flatten) on an
MI355X, every tensor in the guarded arena (tests/guarded.py) at both placements, outputs pre-filled with NaN, no
stream-K ticket left held.

  * pooled layer == max_pool2d(plain layer), exactly: both run the same plan, and a max is exact;
  * pooled layer against an fp64 conv -> BN -> ReLU -> max_pool2d at the layer bar, 2e-5 relative: the fixed cases and
    a seeded sweep of 40 random legal shapes per form;
  * each form -- latency width CT 1 / 2 / 4 with and without a C-split, the throughput kernel on whole items and with
    a stream-K tail -- is forced by the developer knobs and confirmed by the plan queries;
  * one pooled case whose input exceeds 2^32 bytes (the launcher splits it; input and output strides differ);
  * image_pack bitwise against the permuted input, avgpool7_flatten against fp64 adaptive_avg_pool2d at 2e-5."""
import numpy as np
import pytest

import guarded as G
import layer_refs as LR
import shape_sweeps as S
from cases import ring_zero
from gpu_support import torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu

TIGHT = 2e-5          # the project's asserted layer bar
MAX_MACS = 3e8        # of one case's fp64 reference
GIB = 1 << 30


# form -> the knobs that force it (split / grid are filled in per shape)
FORMS = ["ct1", "ct1_split", "ct2", "ct2_split", "ct4", "ct4_split", "big_whole", "big_tail"]


def _items(N, H, W, K):
    return ((N * ((H + 1) // 2) * ((W + 1) // 2) + 63) // 64) * (K // 64)


def form_knobs(form, sh, rng):
    """The developer knobs that force `form` at shape `sh`."""
    if form.startswith("ct"):
        smax = max(1, min(8, (sh["C"] // 16) // 2))
        split = int(rng.randint(2, smax + 1)) if form.endswith("split") else 1
        return {"WINO_3X3_ALGO": "small", "WINO_SMALL_CT": int(form[2]), "WINO_SMALL_SPLIT": split}
    items = _items(sh["N"], sh["H"], sh["W"], sh["K"])
    if form == "big_whole":
        grid = int(rng.choice([g for g in range(1, items + 1) if items % g == 0]))
    else:
        grid = int(rng.randint(2, 2 * items + 40))
        while items % grid == 0:
            grid += 1
    return {"WINO_3X3_ALGO": "big", "WINO_SK_GRID": grid}


def legal(form, sh):
    if sh["H"] < 2 or sh["W"] < 2 or sh["C"] % 8 or sh["K"] % 64:
        return False
    if form.startswith("ct"):
        if sh["C"] % 16 or sh["K"] % (16 * int(form[2])):
            return False
        if form.endswith("split") and sh["C"] < 64:     # a split of 2 needs 8 tasks: 2 C / 16 >= 4 * 2
            return False
    return 9.0 * sh["N"] * sh["H"] * sh["W"] * sh["C"] * sh["K"] <= MAX_MACS


def assert_form(pkg, form, sh, kn):
    """The plan queries, under the forced knobs, name the form that was meant."""
    got, d = S.plan_3x3(pkg, sh["N"], sh["H"], sh["W"], sh["C"], sh["K"])
    if form.startswith("ct"):
        assert got == "latency" and d["ct"] == int(form[2]) and d["split"] == kn["WINO_SMALL_SPLIT"], (form, sh, got, d)
        assert (d["split"] > 1) == form.endswith("split"), (form, sh, d)
    else:
        assert got == "throughput" and d["grid"] == kn["WINO_SK_GRID"], (form, sh, got, d)
        assert (d["tail"] > 0) == (form == "big_tail"), (form, sh, d)


def pooled_cases(form, n=40):
    """`n` seeded random legal shapes for `form`, in the style of shape_sweeps: corners pinned on the first draws."""
    rng = np.random.RandomState(2200 + FORMS.index(form))
    pins = [{"H": 2}, {"W": 2}, {"H": 3, "W": 2}, {"odd": True}, {"K": 192}, {"C": 200}, {"H": 14, "W": 14}, {"N": 1}]
    step = 16 if form.startswith("ct") else 8
    cases = []
    for i in range(n):
        pin = pins[i] if i < len(pins) else {}
        for attempt in range(4000):
            sh = {"N": int(rng.randint(1, 7)), "H": int(rng.randint(2, 25)), "W": int(rng.randint(2, 25)),
                  "C": step * int(rng.randint(1, 200 // step + 1)), "K": int(rng.choice([64, 128, 192, 256]))}
            if attempt < 2000:
                if pin.get("odd"):
                    sh["H"] |= 1
                    sh["W"] |= 1
                sh.update({k: v for k, v in pin.items() if k != "odd"})
                if form.startswith("ct") and sh["C"] % 16:
                    sh["C"] = 208
            if legal(form, sh):
                break
        else:
            raise RuntimeError(f"{form}: no shape drawn")
        cases.append((sh, form_knobs(form, sh, rng), {"relu": i % 4 != 3, "nonneg": i % 3 == 1}))
    return cases


def _operands(torch, sh, seed, nonneg=False):
    g = torch.Generator().manual_seed(seed)
    N, H, W, C, K = (sh[k] for k in "NHWCK")
    x = torch.zeros(N, H + 2, W + 2, C)
    inner = torch.rand(N, H, W, C, generator=g)
    x[:, 1:-1, 1:-1, :] = inner if nonneg else inner * 2 - 1
    w = torch.randn(K, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    bias = torch.rand(K, generator=g) - 0.5
    scale = (torch.rand(K, generator=g) + 0.5) * torch.where(torch.rand(K, generator=g) < 0.2, -1.0, 1.0)
    return x, w, bias, scale


def run_case(pkg, knobs, torch_dev, form, sh, kn, flags, seed, exact):
    torch, dev = torch_dev
    import torch.nn.functional as F
    for k, v in kn.items():
        knobs.set(k, v)
    assert_form(pkg, form, sh, kn)
    N, H, W, C, K = (sh[k] for k in "NHWCK")
    x, w, bias, scale = _operands(torch, sh, seed, flags.get("nonneg", False))
    relu = flags["relu"]
    want = LR.conv3x3(LR.interior(x), w, (bias, scale), relu, pool=True)
    U = pkg.filter_transform_f2(w.to(dev))
    worst = 0.0
    for align in G.ALIGNS:
        arena = G.Arena(torch, dev, align)
        tag = f"[pool {form} {sh} relu={relu} align={align}]"
        xd, Ud = arena.input(x, name="in"), arena.input(U, name="U")
        bd, sd = arena.input(bias, name="bias"), arena.input(scale, name="scale")
        out = arena.output(N, H // 2 + 2, W // 2 + 2, K, name="out")
        got = pkg.conv3x3_bn_relu_pool(xd, Ud, bd, sd, relu, out=out)
        assert got.data_ptr() == out.data_ptr()
        if exact:
            plain = pkg.conv3x3_bn_relu(xd, Ud, bd, sd, relu, out=arena.output(N, H + 2, W + 2, K, name="plain"))
        arena.check(tag)
        assert pkg.tickets_in_use() == 0, tag
        o = out.cpu()
        assert not torch.isnan(o).any(), tag
        assert ring_zero(o), tag
        err = LR.rel(o[:, 1:-1, 1:-1, :], want, floor=1e-30)
        print(f"{tag} rel {err:.2e}")
        worst = max(worst, err)
        assert err < TIGHT, (tag, err)
        if exact:   # numeric equality: a max may return either sign of zero
            pooled = F.max_pool2d(plain.cpu()[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
            assert bool((o[:, 1:-1, 1:-1, :] == pooled).all()), tag
    return worst


FIXED = [(2, 14, 14), (3, 7, 7), (2, 13, 9), (5, 2, 3), (1, 57, 31)]


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("form", FORMS)
def test_pooled_layer_is_the_pool_of_the_plain_layer(form, relu, pkg, knobs, torch_dev):
    """Every form at 14x14 and the odd maps, ReLU on and off: exactly max_pool2d of the plain layer under the same
    plan, zero ring, and within 2e-5 of fp64."""
    rng = np.random.RandomState(7)
    for i, (N, H, W) in enumerate(FIXED):
        sh = {"N": N, "H": H, "W": W, "C": 64, "K": 64 if i % 2 == 0 or form.startswith("ct") else 128}
        kn = form_knobs(form, sh, rng)
        run_case(pkg, knobs, torch_dev, form, sh, kn, {"relu": relu}, 100 + i, exact=True)


def test_pooled_layer_automatic_plan(pkg, knobs, torch_dev):
    """The planner's own choice (no knob), one latency and one throughput shape."""
    torch, dev = torch_dev
    for sh, kind in (({"N": 1, "H": 28, "W": 28, "C": 64, "K": 64}, "latency"),
                     ({"N": 96, "H": 14, "W": 14, "C": 64, "K": 64}, "throughput")):
        assert S.plan_3x3(pkg, *(sh[k] for k in "NHWCK"))[0] == kind, sh
        x, w, bias, scale = _operands(torch, sh, 9)
        want = LR.conv3x3(LR.interior(x), w, (bias, scale), True, pool=True)
        arena = G.Arena(torch, dev, 16)
        out = arena.output(sh["N"], sh["H"] // 2 + 2, sh["W"] // 2 + 2, sh["K"])
        pkg.conv3x3_bn_relu_pool(arena.input(x), arena.input(pkg.filter_transform_f2(w.to(dev))), arena.input(bias),
                                 arena.input(scale), True, out=out)
        arena.check(str(sh))
        assert pkg.tickets_in_use() == 0
        assert ring_zero(out) and LR.rel(LR.interior(out), want, floor=1e-30) < TIGHT


@pytest.mark.parametrize("form", FORMS)
def test_pooled_layer_sweep(form, pkg, knobs, torch_dev):
    """40 seeded random legal shapes per form against fp64."""
    cases = pooled_cases(form)
    assert len(cases) >= 40
    worst = 0.0
    for i, (sh, kn, flags) in enumerate(cases):
        worst = max(worst, run_case(pkg, knobs, torch_dev, form, sh, kn, flags, 500 + i, exact=i % 4 == 0))
    print(f"pooled sweep {form}: {len(cases)} shapes, worst rel {worst:.2e}")


def test_pooled_layer_beyond_4gib(pkg, torch_dev):
    """5100 images of 56x56x64: the input is 4.4 GB, the launcher cuts the batch at 4928 images and advances the input
    by an un-pooled and the output by a pooled image stride.  Images on both sides of 2^31 and 2^32 bytes and of the
    cut against fp64."""
    torch, dev = torch_dev
    N, H, C, CUT = 5100, 56, 64, 4928
    P_in, P_out = (H + 2) * (H + 2) * C * 4, (H // 2 + 2) * (H // 2 + 2) * C * 4
    need = N * (P_in + P_out)
    free, _ = torch.cuda.mem_get_info()
    if free < need + GIB:
        pytest.skip(f"needs {(need + GIB) / GIB:.1f} GiB of free device memory, {free / GIB:.1f} free")
    assert N * P_in > 1 << 32
    idx = {0, N - 1, CUT - 1, CUT}
    for b in (1 << 31, 1 << 32):
        idx |= {b // P_in - 1, b // P_in, b // P_in + 1}
    idx = sorted(i for i in idx if 0 <= i < N)
    g = torch.Generator().manual_seed(71)
    w = torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    bias, scale = torch.rand(C, generator=g) - 0.5, torch.rand(C, generator=g) + 0.5
    gd = torch.Generator(device=dev).manual_seed(72)
    x = LR.fill_ring(torch.rand(N, H + 2, H + 2, C, device=dev, generator=gd).sub_(0.5))
    out = torch.full((N, H // 2 + 2, H // 2 + 2, C), float("nan"), device=dev)
    pkg.conv3x3_bn_relu_pool(x, pkg.filter_transform_f2(w.to(dev)), bias.to(dev), scale.to(dev), True, out=out)
    torch.cuda.synchronize()
    assert pkg.tickets_in_use() == 0
    assert bool(torch.isfinite(out).all()) and ring_zero(out)
    sel = torch.as_tensor(idx, device=dev)
    want = LR.conv3x3(LR.interior(x[sel]), w, (bias, scale), True, pool=True)
    assert LR.rel(LR.interior(out[sel]), want, floor=1e-30) < TIGHT
    del x, out
    torch.cuda.empty_cache()


@pytest.mark.parametrize("N,Cin,H,W,Cpad", [(1, 3, 33, 47, 16), (33, 3, 5, 7, 8), (2, 1, 9, 4, 8), (3, 8, 6, 11, 8),
                                             (1, 8, 1, 1, 16), (2, 3, 224, 224, 16)])
def test_image_pack_is_a_copy(N, Cin, H, W, Cpad, pkg, torch_dev):
    torch, dev = torch_dev
    x = torch.randn(N, Cin, H, W, generator=torch.Generator().manual_seed(N + H))
    want = torch.zeros(N, H + 2, W + 2, Cpad)
    want[:, 1:-1, 1:-1, :Cin] = x.permute(0, 2, 3, 1)
    for align in G.ALIGNS:
        arena = G.Arena(torch, dev, align)
        out = pkg.image_pack(arena.input(x, name="x"), Cpad, out=arena.output(N, H + 2, W + 2, Cpad, name="out"))
        arena.check(f"[image_pack {N} {Cin} {H} {W} {Cpad} align={align}]")
        got = out.cpu()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))   # bitwise: ring and pad channels +0


@pytest.mark.parametrize("N,H,W,C,padded", [(1, 7, 7, 512, True), (33, 1, 1, 64, True), (2, 8, 10, 32, False),
                                             (3, 13, 7, 4, True), (1, 3, 4, 128, False), (2, 31, 17, 8, True)])
def test_avgpool7_flatten(N, H, W, C, padded, pkg, torch_dev):
    torch, dev = torch_dev
    p = 1 if padded else 0
    x = torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(H * W + C))
    feat = torch.full((N, H + 2 * p, W + 2 * p, C), 1e30)     # a ring that is read shows
    feat[:, p:p + H, p:p + W, :] = x
    want = LR.avgpool7(x).reshape(N, 49 * C)
    for align in G.ALIGNS:
        arena = G.Arena(torch, dev, align)
        out = pkg.avgpool7_flatten(arena.input(feat, name="feat"), in_padded=padded, out=arena.output(N, 49 * C, name="out"))
        arena.check(f"[avgpool7 {N} {H} {W} {C} align={align}]")
        assert LR.rel(out, want, floor=1e-30) < TIGHT
