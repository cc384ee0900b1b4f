"""Non-finite values through the kernels' arithmetic: the poison plan, the footprint arithmetic and the one checker of
DESIGN.md section 1, "Non-finite values", shared by tests/test_nonfinite_host.py (the footprints against torch on the
CPU, no GPU) and tests/test_gpu_nonfinite.py (every layer on an MI355X).

One launch carries one poisoned element: a NaN, +Inf or -Inf in an activation pixel, a residual, a weight, a BN bias or
a BN scale.  `check_poisoned` then holds the launch to three things: where the fp64 reference of the poisoned inputs is
NaN the library is NaN, and where it is +-Inf the library has that Inf or NaN (propagation); outside the poisoned
element's footprint the output is bit for bit the same launch's output on the clean inputs (containment); inside the
footprint, where the reference is finite, an element is non-finite or within the layer's tolerance.

The footprints are plain index arithmetic on intervals, written here without torch's convolutions, so that the host
test can hold them against F.conv2d / max_pool2d / interpolate before the GPU test trusts them.

Two poisons are left out of every draw, and one is held to less, each for a reason that does not depend on any kernel:
  * an infinity that a ReLU flushes everywhere it reaches (a -Inf bias, a -Inf residual element, an infinite pixel of a
    4-channel group whose taps all have one sign): relu(-Inf) = 0, so the fp64 reference of that launch is finite
    everywhere and the check that "the poison did something" has nothing to find.  The reference alone decides this;
  * an infinite weight of a padded F(2x2) Winograd layer: at the border the direct reference multiplies the zero padding
    by the weight, 0 * Inf = NaN, while the transformed patch d0 - d2 has no zero there and gives +-Inf -- the contract
    orders the two only the other way round (reference Inf, Winograd NaN).  Such a poison (`weak`) is launched and held
    to containment, bitwise, outside its channel, to "non-finite wherever the reference is non-finite" in place of the
    NaN / Inf distinction, and to the band rule; a NaN weight is held to everything;
  * rings: a padded input's ring stays 0, as the layers require."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import layer_refs as LR
from cases import TIGHT
from fpn_reference import level_reference
from layer_refs import ring as _ring

NAN, INF = float("nan"), float("inf")
VALUES = (NAN, INF, -INF)
MAX_POISONS = 12


@dataclass(frozen=True)
class Poison:
    target: str          # the name of the master tensor
    index: tuple         # the element, in the master's own layout
    value: float
    where: str           # "first" / "last" (the two image-boundary pixels), "corner", "edge", "centre", or "param"
    k: int | None = None  # a parameter's output channel
    weak: bool = False    # held to containment and "non-finite where the reference is" only (see the module text)

    def tag(self):
        return f"{self.target}{list(self.index)}={self.value} ({self.where})"


# ---- interval arithmetic: (lo, hi) inclusive, None when empty -------------------------------------------------------
def _clip(lo, hi, n):
    lo, hi = max(lo, 0), min(hi, n - 1)
    return (lo, hi) if lo <= hi else None


def conv_rows(y, n_out, k, stride, pad):
    """Output rows o of a k-tap, stride-`stride`, pad-`pad` convolution or pool whose window holds input row y:
    o * stride - pad <= y <= o * stride - pad + k - 1."""
    return _clip(-((-(y + pad - k + 1)) // stride), (y + pad) // stride, n_out)


def wino_tiles(y, H):
    """F(2x2,3x3) tiles t (output rows 2t, 2t + 1) whose 4-row patch, padded rows 2t .. 2t + 3, holds interior row y
    (padded row y + 1)."""
    return _clip(-((-(y - 2)) // 2), (y + 1) // 2, (H + 1) // 2)


def wino_rows(y, H):
    t = wino_tiles(y, H)
    return _clip(2 * t[0], 2 * t[1] + 1, H)


def wino_pool_rows(y, H):
    """Pooled rows of those tiles (an odd H's clipped last tile has none)."""
    t = wino_tiles(y, H)
    return _clip(t[0], t[1], H // 2)


def up2_rows(yc, H):
    """Rows y of the finer map that read the coarser map's row yc = y >> 1."""
    return _clip(2 * yc, 2 * yc + 1, H)


def adaptive_bins(y, H, bins=7):
    """AdaptiveAvgPool bins i whose window [floor(i H / bins), ceil((i + 1) H / bins)) holds row y."""
    hit = [i for i in range(bins) if (i * H) // bins <= y < -((-(i + 1) * H) // bins)]
    return (hit[0], hit[-1])


def hull(f, iv, *args):
    """The image of an interval under a monotone row map f(y, *args)."""
    if iv is None:
        return None
    a, b = f(iv[0], *args), f(iv[1], *args)
    got = [v for v in (a, b) if v is not None]
    return (min(v[0] for v in got), max(v[1] for v in got)) if got else None


def stem_rows(y, H):
    """The stem: the 7x7 / s2 / p3 field dilated by the 3x3 / s2 / p1 pool."""
    Hc = (H - 1) // 2 + 1
    return hull(conv_rows, conv_rows(y, Hc, 7, 2, 3), (Hc - 1) // 2 + 1, 3, 2, 1)


def box(torch, shape, n=None, rows=None, cols=None, chans=None, ring=0):
    """A bool mask of an [N][H + 2 ring][W + 2 ring][K] output: image n (None: all), the interior rows / columns of the
    inclusive intervals (None: all; an empty interval: nothing), the channels of `chans` (None: all)."""
    m = torch.zeros(shape, dtype=torch.bool)
    N, Hp, Wp, K = shape
    full = lambda n_: (0, n_ - 2 * ring - 1)
    if rows == () or cols == ():
        return m
    r, c = rows or full(Hp), cols or full(Wp)
    ns = slice(None) if n is None else slice(n, n + 1)
    ks = slice(None) if chans is None else slice(chans[0], chans[1] + 1)
    m[ns, r[0] + ring:r[1] + ring + 1, c[0] + ring:c[1] + ring + 1, ks] = True
    return m


def _iv(v):
    return () if v is None else v


# ---- the poison plan --------------------------------------------------------------------------------------------------
def positions(N, H, W):
    """{name: (n, y, x)}: the first and the last interior pixel of image 1 (next in memory to image 0's last pixel and to
    image 2's first), one corner, one edge and one centre pixel.  (N = 1: image 0.)"""
    n1 = min(1, N - 1)
    return {"first": (n1, 0, 0), "last": (n1, H - 1, W - 1), "corner": (N - 1, 0, W - 1), "edge": (0, H // 2, 0),
            "centre": (0, H // 2, W // 2)}


def candidates(layer):
    """The whole cross product of the plan for one layer, as (mandatory boundary poisons, parameter poisons, the rest)."""
    boundary, params, rest = [], [], []
    for name, (N, H, W, C) in layer.acts.items():
        for where, (n, y, x) in positions(N, H, W).items():
            for c in sorted({0, C - 1}):
                for v in VALUES:
                    p = Poison(name, layer.act_index(name, n, y, x, c), v, where)
                    (boundary if where in ("first", "last") and name == layer.main else rest).append(p)
    for name, per_k in layer.params.items():
        for k, index in per_k:
            for v in VALUES:
                # (an infinite Winograd weight is held to the weaker check: see the module text)
                params.append(Poison(name, index, v, "param", k, weak=v == v and name in layer.wino_weights))
    return tuple([p for p in ps if layer.shows(p)] for ps in (boundary, params, rest))


def draw(layer, seed):
    """At most MAX_POISONS poisons, seeded: one at the first and one at the last interior pixel of image 1, one
    parameter, then a sample of everything else without repeats; every value occurs."""
    rng = np.random.RandomState(seed)
    boundary, params, rest = candidates(layer)
    pick = lambda pool: pool[int(rng.randint(len(pool)))]
    at = lambda where, keep: [p for p in boundary if p.where == where and keep(p.value)] or \
        [p for p in boundary if p.where == where]
    first, last = pick(at("first", lambda v: v != v)), pick(at("last", lambda v: v == INF))
    chosen = [first, last] + ([pick(params)] if params else [])
    pool = [p for p in boundary + params + rest if p not in chosen]
    # drop repeats of one element with another value's twin already in (distinct elements first)
    order = rng.permutation(len(pool))
    for i in order:
        if len(chosen) >= MAX_POISONS:
            break
        p = pool[int(i)]
        if not any(q.target == p.target and q.index == p.index for q in chosen):
            chosen.append(p)
    for i in order:      # a small layer has fewer distinct elements than the cap: the other values of the same ones
        if len(chosen) >= MAX_POISONS:
            break
        if pool[int(i)] not in chosen:
            chosen.append(pool[int(i)])
    if not any(p.value == -INF for p in chosen) and len(chosen) > 3:
        chosen[-1] = pick([p for p in pool if p.value == -INF])
    return chosen


def check_draw(layer, seed):
    """What the host test asserts of a draw: the cap, the mandatory poisons, no repeats, all three values."""
    ps = draw(layer, seed)
    assert 3 <= len(ps) <= MAX_POISONS and len(set(ps)) == len(ps), (layer.tag, len(ps))
    N, H, W, _ = layer.acts[layer.main]
    pos = positions(N, H, W)
    for where in ("first", "last"):
        n, y, x = pos[where]
        assert any(p.target == layer.main and p.where == where and layer.pixel_of(p) == (n, y, x) for p in ps), \
            (layer.tag, where)
    assert not layer.params or any(p.where == "param" for p in ps), layer.tag
    assert {repr(p.value) for p in ps} == {"nan", "inf", "-inf"}, layer.tag
    assert ps == draw(layer, seed), "the draw is not a function of its seed"
    return ps


# ---- the checker ------------------------------------------------------------------------------------------------------
def check_poisoned(torch, got_clean, got_poisoned, want_poisoned, footprint_mask, tol, tag, exact_inf=False,
                   single_pixel=False, any_nonfinite=False):
    """Points 1-3 of the contract for one poisoned launch.  got_*: the library's fp32 outputs of the same launch on the
    clean and on the poisoned inputs; want_poisoned: the fp64 reference of the poisoned inputs, the same shape;
    footprint_mask: where the poison may show.  exact_inf: a direct kernel, which must give the reference's Inf.
    single_pixel: the output is one pixel, so nothing lies outside the footprint (named by the caller, never guessed).
    any_nonfinite: point 1 asks only that the library is non-finite wherever the reference is (a `weak` poison)."""
    gc, gp = got_clean.detach().cpu(), got_poisoned.detach().cpu()
    want, mask = want_poisoned, footprint_mask
    assert gc.shape == gp.shape == want.shape == mask.shape, (tag, gc.shape, gp.shape, want.shape, mask.shape)
    assert gc.dtype == gp.dtype == torch.float32 and want.dtype == torch.float64, tag
    outside = ~mask
    if not single_pixel:
        assert bool(outside.any()), f"{tag}: nothing lies outside the footprint, containment was not compared"
    ref_nf = ~torch.isfinite(want)
    assert bool(ref_nf[mask].any()), f"{tag}: the reference is finite everywhere: the poison did nothing"
    assert not bool(ref_nf[outside].any()), f"{tag}: the reference is non-finite outside the declared footprint"
    # 2. containment, bitwise, against the library's own clean run
    leak = (gc.view(torch.int32) != gp.view(torch.int32)) & outside
    if bool(leak.any()):
        at = [tuple(int(v) for v in i) for i in leak.nonzero()[:4]]
        raise AssertionError(f"{tag}: {int(leak.sum())} elements outside the footprint differ from the clean run, "
                             f"first at {at}: clean {[float(gc[i]) for i in at]} poisoned {[float(gp[i]) for i in at]}")
    # 1. propagation
    ref_nan, got_nan = torch.isnan(want), torch.isnan(gp)
    if any_nonfinite:
        finite = ref_nf & torch.isfinite(gp)
        assert not bool(finite.any()), f"{tag}: {int(finite.sum())} of {int(ref_nf.sum())} non-finite reference elements " \
                                       f"are finite in the output, first at {[tuple(int(v) for v in i) for i in finite.nonzero()[:4]]}"
        ref_nan = ref_nan & False
    lost = ref_nan & ~got_nan
    if bool(lost.any()):
        at = [tuple(int(v) for v in i) for i in lost.nonzero()[:4]]
        raise AssertionError(f"{tag}: {int(lost.sum())} of {int(ref_nan.sum())} reference NaNs are not NaN in the "
                             f"output, first at {at}: got {[float(gp[i]) for i in at]}")
    ref_inf = torch.isinf(want) & (not any_nonfinite)
    same_inf = gp.double() == want
    bad = ref_inf & ~(same_inf if exact_inf else (same_inf | got_nan))
    if bool(bad.any()):
        at = [tuple(int(v) for v in i) for i in bad.nonzero()[:4]]
        raise AssertionError(f"{tag}: {int(bad.sum())} reference Infs are neither that Inf{'' if exact_inf else ' nor NaN'}"
                             f", first at {at}: want {[float(want[i]) for i in at]} got {[float(gp[i]) for i in at]}")
    # 3. the band: inside the footprint, reference finite
    band = mask & ~ref_nf
    if bool(band.any()):
        scale = float(want[~ref_nf].abs().max())
        g = gp.double()
        off = band & torch.isfinite(g) & ~((g - want).abs() <= tol * scale)
        if bool(off.any()):
            at = [tuple(int(v) for v in i) for i in off.nonzero()[:4]]
            raise AssertionError(f"{tag}: {int(off.sum())} finite elements inside the footprint are off the reference "
                                 f"by more than {tol} * {scale:.3g}, first at {at}: want {[float(want[i]) for i in at]} "
                                 f"got {[float(gp[i]) for i in at]}")


# ---- the layers: masters, fp64 references, footprints ---------------------------------------------------------------
def s2_out(h):
    return (h - 1) // 2 + 1


class Layer:
    """One layer kind at one shape: `t` the clean CPU masters in torch's own layouts (activations NHWC without rings),
    `acts` the poisonable activations {name: (N, H, W, C)} with `main` the layer's input, `params` {name: [(k, index),
    ..]} at output channels 0 and K - 1, `ref(t)` the fp64 reference and `footprint(p)` the mask, both of the
    library's whole output (rings included; several outputs of one shape are stacked in front), `run(pkg, d)` the
    launch on device copies of the masters."""
    relu = False
    exact_inf = False        # a direct kernel
    wino_weights = ()
    main = "x"
    tol = TIGHT
    single_pixel = False

    def __init__(self, torch, tag, seed):
        self.torch, self.tag = torch, tag
        self.g = torch.Generator().manual_seed(seed)
        self.t, self.acts, self.params = {}, {}, {}

    def rand(self, *shape):
        return self.torch.rand(*shape, generator=self.g)

    def act(self, name, N, H, W, C):
        self.t[name] = self.rand(N, H, W, C) - 0.5
        self.acts[name] = (N, H, W, C)

    def bn(self, K, b="b", s="s"):
        """bias and scale, a negative scale on every third channel; both poisonable at channels 0 and K - 1."""
        self.t[b], self.t[s] = LR.bn_pair(self.rand, K)
        for name in (b, s):
            self.params[name] = [(k, (k,)) for k in sorted({0, K - 1})]

    def act_index(self, name, n, y, x, c):
        return (n, y, x, c)

    def pixel_of(self, p):
        return tuple(p.index[:3])

    def poisoned(self, p):
        t = dict(self.t)
        t[p.target] = t[p.target].clone()
        assert bool(self.torch.isfinite(t[p.target][p.index])), "one element, finite before"
        t[p.target][p.index] = p.value
        return t

    def shows(self, p):
        """Does the fp64 reference show this poison at all?  (An infinity under a ReLU can vanish; so does any value
        at a pixel that a strided 1x1 never reads.)"""
        return not bool(self.torch.isfinite(self.ref(self.poisoned(p))).all())

    def to(self, dev, t):
        return {k: v.to(dev) for k, v in t.items()}


class Conv3x3(Layer):
    """The fused F(2x2) 3x3: mode "plain" (conv3x3_bn_relu), "res" (conv3x3_bn_add_relu, the residual's ring NaN) or
    "pool" (conv3x3_bn_relu_pool)."""
    wino_weights = ("w",)

    def __init__(self, torch, mode, relu, N, H, W, C, K, seed):
        super().__init__(torch, f"3x3 {mode} relu={int(relu)} {N}x{H}x{W} {C}->{K}", seed)
        self.mode, self.relu, self.shape = mode, relu, (N, H, W, C, K)
        self.act("x", N, H, W, C)
        self.t["w"] = LR.conv_w(self.rand, K, C)
        self.params["w"] = [(0, (0, C - 1, 0, 2)), (K - 1, (K - 1, 0, 1, 1))]
        self.bn(K)
        if mode == "res":
            self.act("res", N, H, W, K)
        Ho, Wo = (H // 2, W // 2) if mode == "pool" else (H, W)
        self.out_shape = (N, Ho + 2, Wo + 2, K)

    def run(self, pkg, d):
        torch = self.torch
        x, U = _ring(d["x"]), pkg.filter_transform_f2(d["w"])
        out = torch.full(self.out_shape, NAN, device=x.device)
        if self.mode == "plain":
            return pkg.conv3x3_bn_relu(x, U, d["b"], d["s"], relu=self.relu, out=out)
        if self.mode == "pool":
            return pkg.conv3x3_bn_relu_pool(x, U, d["b"], d["s"], relu=self.relu, out=out)
        return pkg.conv3x3_bn_add_relu(x, U, d["b"], d["s"], _ring(d["res"], NAN), relu=self.relu, out=out)

    def ref(self, t):
        return _ring(LR.conv3x3(t["x"], t["w"], (t["b"], t["s"]), self.relu, residual=t.get("res"),
                                pool=self.mode == "pool"))

    def footprint(self, p):
        N, H, W, C, K = self.shape
        if p.where == "param":
            return box(self.torch, self.out_shape, chans=(p.k, p.k), ring=1)
        n, y, x, c = p.index
        if p.target == "res":
            return box(self.torch, self.out_shape, n, (y, y), (x, x), (c, c), ring=1)
        rows = wino_pool_rows if self.mode == "pool" else wino_rows
        return box(self.torch, self.out_shape, n, _iv(rows(y, H)), _iv(rows(x, W)), ring=1)

    def receptive_field(self, p):
        """The exact field of an activation poison (the host test's second check): the 3x3 window, pooled 2x2."""
        N, H, W, C, K = self.shape
        if p.target == "res":
            return self.footprint(p)
        n, y, x, c = p.index
        r, q = conv_rows(y, H, 3, 1, 1), conv_rows(x, W, 3, 1, 1)
        if self.mode == "pool":
            r, q = hull(conv_rows, r, H // 2, 2, 2, 0), hull(conv_rows, q, W // 2, 2, 2, 0)
        return box(self.torch, self.out_shape, n, _iv(r), _iv(q), ring=1)


class Conv1x1(Layer):
    """conv1x1_bn_ex under `flags` (bits of pkg.RELU / A_PADDED / C_PADDED / ADD_RESIDUAL / RESIDUAL_UP2, passed as
    numbers so that the host test needs no library): A's ring and the coarse map's ring NaN."""
    RELU, A_PADDED, C_PADDED, ADD_RESIDUAL, RESIDUAL_UP2 = 1, 2, 4, 8, 16
    exact_inf = True
    main = "A"

    def __init__(self, torch, flags, N, H, W, Cin, Kout, seed):
        super().__init__(torch, f"1x1 flags={flags} {N}x{H}x{W} {Cin}->{Kout}", seed)
        self.flags, self.relu, self.shape = flags, bool(flags & self.RELU), (N, H, W, Cin, Kout)
        self.act("A", N, H, W, Cin)
        self.t["B"] = LR.w11(self.rand, Cin, Kout)
        self.params["B"] = [(0, (Cin - 1, 0)), (Kout - 1, (0, Kout - 1))]
        self.bn(Kout)
        self.up2 = bool(flags & self.RESIDUAL_UP2)
        if self.up2:
            self.act("top", N, (H + 1) // 2, (W + 1) // 2, Kout)
        elif flags & self.ADD_RESIDUAL:
            self.act("res", N, H, W, Kout)
        self.ring = 1 if flags & self.C_PADDED else 0
        self.out_shape = (N, H + 2 * self.ring, W + 2 * self.ring, Kout)
        self.single_pixel = (N, H, W) == (1, 1, 1)

    def run(self, pkg, d):
        torch = self.torch
        N, H, W, Cin, Kout = self.shape
        A = _ring(d["A"], NAN) if self.flags & self.A_PADDED else d["A"]
        res = _ring(d["top"], NAN) if self.up2 else d.get("res")
        out = torch.full(self.out_shape, NAN, device=A.device)
        return pkg.conv1x1_bn_ex(A, d["B"], d["b"], d["s"], self.flags, residual=res, out=out, hw=(H, W))

    def ref(self, t):
        y = LR.conv1x1(t["A"], t["B"], (t["b"], t["s"]), self.relu, residual=t.get("res"), top=t.get("top"))
        return _ring(y) if self.ring else y

    def footprint(self, p):
        N, H, W, Cin, Kout = self.shape
        mk = lambda *a, **kw: box(self.torch, self.out_shape, *a, ring=self.ring, **kw)
        if p.where == "param":
            return mk(chans=(p.k, p.k))
        n, y, x, c = p.index
        if p.target == "A":
            return mk(n, (y, y), (x, x))
        if p.target == "res":
            return mk(n, (y, y), (x, x), (c, c))
        return mk(n, _iv(up2_rows(y, H)), _iv(up2_rows(x, W)), (c, c))

    receptive_field = footprint


class ConvS2(Layer):
    """The stride-2 3x3 as an implicit GEMM: conv3x3_s2_bn_relu, or (proj) conv3x3_s2_proj, whose two outputs t1 and
    sc are stacked [2][N][H+2][W+2][K]; sc's ring is not touched (pre-filled 0 here)."""
    exact_inf = True

    def __init__(self, torch, proj, relu, N, Hin, Win, C, K, seed):
        super().__init__(torch, f"3x3/s2 {'proj' if proj else 'plain'} relu={int(relu)} {N}x{Hin}x{Win} {C}->{K}", seed)
        self.proj, self.relu, self.shape = proj, relu or proj, (N, Hin, Win, C, K)
        self.act("x", N, Hin, Win, C)
        self.t["w"] = LR.conv_w(self.rand, K, C)
        self.params["w"] = [(0, (0, C - 1, 0, 2)), (K - 1, (K - 1, 0, 1, 1))]
        self.bn(K)
        self.H, self.W = s2_out(Hin), s2_out(Win)
        self.one = (N, self.H + 2, self.W + 2, K)
        if proj:
            self.t["wd"] = LR.conv_w(self.rand, K, C, k=1)
            self.params["wd"] = [(0, (0, C - 1, 0, 0)), (K - 1, (K - 1, 0, 0, 0))]
            self.bn(K, "bd", "sd")
        self.out_shape = (2,) + self.one if proj else self.one

    def run(self, pkg, d):
        torch = self.torch
        x, taps = _ring(d["x"]), pkg.filter_pack_s2(d["w"])
        if not self.proj:
            return pkg.conv3x3_s2_bn_relu(x, taps, d["b"], d["s"], relu=self.relu,
                                          out=torch.full(self.one, NAN, device=x.device))
        K, C = d["w"].shape[:2]
        packed = pkg.s2_proj_pack(taps, (d["b"], d["s"]), d["wd"].view(K, C).t().contiguous(), (d["bd"], d["sd"]))
        t1, sc = pkg.conv3x3_s2_proj(x, packed, t1=torch.full(self.one, NAN, device=x.device),
                                     sc=torch.zeros(self.one, device=x.device))
        return torch.stack((t1, sc))

    def ref(self, t):
        if not self.proj:
            return _ring(LR.conv3x3(t["x"], t["w"], (t["b"], t["s"]), self.relu, stride=2))
        t1, sc, _ = LR.basic_block_s2(t["x"], t["w"], (t["b"], t["s"]), t["wd"], (t["bd"], t["sd"]))
        return self.torch.stack((_ring(t1), _ring(sc)))

    def footprint(self, p):
        N, Hin, Win, C, K = self.shape
        mk = lambda *a, **kw: box(self.torch, self.one, *a, ring=1, **kw)
        none = self.torch.zeros(self.one, dtype=self.torch.bool)
        if p.where == "param":
            m = mk(chans=(p.k, p.k))
            t1, sc = (m, none) if p.target in ("w", "b", "s") else (none, m)
        else:
            n, y, x, c = p.index
            t1 = mk(n, _iv(conv_rows(y, self.H, 3, 2, 1)), _iv(conv_rows(x, self.W, 3, 2, 1)))
            sc = mk(n, _iv(conv_rows(y, self.H, 1, 2, 0)), _iv(conv_rows(x, self.W, 1, 2, 0)))
        return self.torch.stack((t1, sc)) if self.proj else t1

    receptive_field = footprint


class Grouped(Layer):
    """conv3x3_grouped_bn_relu: C channels in C / Cg groups, stride 1 or 2."""
    exact_inf = True

    def __init__(self, torch, relu, stride, N, Hin, Win, C, Cg, seed):
        super().__init__(torch, f"grouped relu={int(relu)} s{stride} {N}x{Hin}x{Win} C={C} Cg={Cg}", seed)
        self.relu, self.stride, self.shape, self.groups = relu, stride, (N, Hin, Win, C, Cg), C // Cg
        self.act("x", N, Hin, Win, C)
        self.t["w"] = LR.conv_w(self.rand, C, Cg)
        self.params["w"] = [(0, (0, Cg - 1, 0, 2)), (C - 1, (C - 1, 0, 1, 1))]
        self.bn(C)
        self.H, self.W = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
        self.out_shape = (N, self.H + 2, self.W + 2, C)

    def run(self, pkg, d):
        torch = self.torch
        x = _ring(d["x"])
        return pkg.conv3x3_grouped_bn_relu(x, pkg.filter_pack_grouped(d["w"], self.groups), d["b"], d["s"], self.groups,
                                           stride=self.stride, relu=self.relu,
                                           out=torch.full(self.out_shape, NAN, device=x.device))

    def ref(self, t):
        return _ring(LR.conv3x3(t["x"], t["w"], (t["b"], t["s"]), self.relu, stride=self.stride, groups=self.groups))

    def footprint(self, p):
        N, Hin, Win, C, Cg = self.shape
        if p.where == "param":
            return box(self.torch, self.out_shape, chans=(p.k, p.k), ring=1)
        n, y, x, c = p.index
        g = c // Cg
        return box(self.torch, self.out_shape, n, _iv(conv_rows(y, self.H, 3, self.stride, 1)),
                   _iv(conv_rows(x, self.W, 3, self.stride, 1)), (g * Cg, g * Cg + Cg - 1), ring=1)

    receptive_field = footprint


class Stem(Layer):
    """stem: x is NCHW [N][3][H][W]."""
    relu = True
    exact_inf = True

    def __init__(self, torch, padded, N, H, W, K, seed):
        super().__init__(torch, f"stem padded={int(padded)} {N}x{H}x{W} K={K}", seed)
        self.padded, self.shape = padded, (N, H, W, K)
        self.t["x"] = self.rand(N, 3, H, W) * 2 - 1
        self.acts["x"] = (N, H, W, 3)
        self.t["w"] = (self.rand(K, 3, 7, 7) - 0.5) * 0.3
        self.params["w"] = [(0, (0, 2, 0, 6)), (K - 1, (K - 1, 0, 3, 3))]
        self.bn(K)
        self.Hp, self.Wp = s2_out(s2_out(H)), s2_out(s2_out(W))
        self.ring = 1 if padded else 0
        self.out_shape = (N, self.Hp + 2 * self.ring, self.Wp + 2 * self.ring, K)
        self.single_pixel = (N, self.Hp, self.Wp) == (1, 1, 1)

    def act_index(self, name, n, y, x, c):
        return (n, c, y, x)

    def pixel_of(self, p):
        return (p.index[0], p.index[2], p.index[3])

    def run(self, pkg, d):
        packed = pkg.stem_filter_pack(d["w"], (d["b"], d["s"]))
        return pkg.stem(d["x"], packed, out_padded=self.padded,
                        out=self.torch.full(self.out_shape, NAN, device=d["x"].device))

    def ref(self, t):
        y = LR.stem(t["x"], t["w"], (t["b"], t["s"]))
        return _ring(y) if self.ring else y

    def footprint(self, p):
        N, H, W, K = self.shape
        if p.where == "param":
            return box(self.torch, self.out_shape, chans=(p.k, p.k), ring=self.ring)
        n, c, y, x = p.index
        return box(self.torch, self.out_shape, n, _iv(stem_rows(y, H)), _iv(stem_rows(x, W)), ring=self.ring)

    receptive_field = footprint


class Head(Layer):
    """avgpool_fc: the output [N][classes] is handled as [N][1][1][classes]."""
    exact_inf = True
    main = "feat"

    def __init__(self, torch, padded, N, H, W, C, classes, seed):
        super().__init__(torch, f"head padded={int(padded)} {N}x{H}x{W} C={C} classes={classes}", seed)
        self.padded, self.shape = padded, (N, H, W, C, classes)
        self.t["feat"] = self.rand(N, H, W, C) * 2 - 1
        self.acts["feat"] = (N, H, W, C)
        self.t["wfc"] = (self.rand(classes, C) - 0.5) / np.sqrt(C) * 2
        self.t["bfc"] = self.rand(classes) - 0.5
        ks = sorted({0, classes - 1})
        self.params["wfc"] = [(k, (k, C - 1 if k == 0 else 0)) for k in ks]
        self.params["bfc"] = [(k, (k,)) for k in ks]
        self.out_shape = (N, 1, 1, classes)

    def run(self, pkg, d):
        N, H, W, C, classes = self.shape
        f = _ring(d["feat"], NAN) if self.padded else d["feat"]
        out = self.torch.full((N, classes), NAN, device=f.device)
        return pkg.avgpool_fc(f, pkg.head_pack(d["wfc"], d["bfc"]), classes, in_padded=self.padded,
                              out=out).view(self.out_shape)

    def ref(self, t):
        return LR.avgpool_fc(t["feat"], t["wfc"], t["bfc"]).view(self.out_shape)

    def footprint(self, p):
        if p.where == "param":
            return box(self.torch, self.out_shape, chans=(p.k, p.k))
        return box(self.torch, self.out_shape, p.index[0])

    receptive_field = footprint


class ImagePack(Layer):
    """image_pack: NCHW -> padded NHWC with zero pad channels; a copy, so the footprint is the one element."""
    exact_inf = True

    def __init__(self, torch, N, Cin, H, W, Cpad, seed):
        super().__init__(torch, f"image_pack {N}x{Cin}x{H}x{W} Cpad={Cpad}", seed)
        self.shape = (N, Cin, H, W, Cpad)
        self.t["x"] = self.rand(N, Cin, H, W) * 2 - 1
        self.acts["x"] = (N, H, W, Cin)
        self.out_shape = (N, H + 2, W + 2, Cpad)

    act_index, pixel_of = Stem.act_index, Stem.pixel_of

    def run(self, pkg, d):
        return pkg.image_pack(d["x"], self.shape[4], out=self.torch.full(self.out_shape, NAN, device=d["x"].device))

    def ref(self, t):
        N, Cin, H, W, Cpad = self.shape
        y = self.torch.zeros(self.out_shape, dtype=self.torch.float64)
        y[:, 1:-1, 1:-1, :Cin] = t["x"].double().permute(0, 2, 3, 1)
        return y

    def footprint(self, p):
        n, c, y, x = p.index
        return box(self.torch, self.out_shape, n, (y, y), (x, x), (c, c), ring=1)

    receptive_field = footprint


class AvgPool7(Layer):
    """avgpool7_flatten: [N][49 C] in (h, w, c) order is handled as [N][7][7][C]."""
    exact_inf = True
    main = "feat"

    def __init__(self, torch, padded, N, H, W, C, seed):
        super().__init__(torch, f"avgpool7 padded={int(padded)} {N}x{H}x{W} C={C}", seed)
        self.padded, self.shape = padded, (N, H, W, C)
        self.act("feat", N, H, W, C)
        self.out_shape = (N, 7, 7, C)

    def run(self, pkg, d):
        f = _ring(d["feat"], NAN) if self.padded else d["feat"]
        out = self.torch.full((self.shape[0], 49 * self.shape[3]), NAN, device=f.device)
        return pkg.avgpool7_flatten(f, in_padded=self.padded, out=out).view(self.out_shape)

    def ref(self, t):
        return LR.avgpool7(t["feat"])

    def footprint(self, p):
        N, H, W, C = self.shape
        n, y, x, c = p.index
        return box(self.torch, self.out_shape, n, adaptive_bins(y, H), adaptive_bins(x, W), (c, c))

    receptive_field = footprint


# ---- driving one layer --------------------------------------------------------------------------------------------------
class Plan:
    """The poisons of one layer with their fp64 references and masks, computed once and shared by every launch form."""

    def __init__(self, layer, seed):
        self.layer, self.seed = layer, seed
        self.items = []
        for p in draw(layer, seed):
            t = layer.poisoned(p)
            self.items.append((p, t, layer.ref(t), layer.footprint(p)))


def run_plan(pkg, torch, dev, plan, form=""):
    """The clean launch, then every poisoned one: the contract, and after each the stream's state check (a NaN in data
    is not a state error).  Returns the number of poisoned launches."""
    layer = plan.layer
    clean = layer.run(pkg, layer.to(dev, layer.t)).clone()
    assert bool(torch.equal(layer.run(pkg, layer.to(dev, layer.t)), clean)), f"[{layer.tag} {form}]: two clean launches differ"
    for p, t, want, mask in plan.items:
        got = layer.run(pkg, layer.to(dev, t))
        pkg.stream_check()
        check_poisoned(torch, clean, got, want, mask, layer.tol, f"[{layer.tag} {form} seed={plan.seed} {p.tag()}]",
                       exact_inf=layer.exact_inf, single_pixel=layer.single_pixel, any_nonfinite=p.weak)
    assert pkg.tickets_in_use() == 0, f"[{layer.tag} {form}]: a stream-K ticket is still held"
    return len(plan.items)


# ---- blocks: the poisoned image is the footprint ----------------------------------------------------------------------
class Block(Layer):
    """One block at N = 2: x [N][H][W][C] poisoned, the footprint the whole of the poisoned image (the composition of
    its layers' footprints lies inside it), the reference the fp64 composition."""
    N = 2
    relu = True

    def footprint(self, p):
        return box(self.torch, self.out_shape[-4:], p.index[0], ring=self.ring).expand(self.out_shape).clone()

    def nan_out(self, dev):
        return self.torch.full(self.out_shape, NAN, device=dev)


class Bottleneck(Block):
    """residual_block / grouped_residual_block (identity) and proj_block / proj_block_v15 / grouped_proj_block."""
    ring = 0

    def __init__(self, torch, kind, H, W, Cin, Cm, C4, stride, groups, seed):
        super().__init__(torch, f"{kind} 2x{H}x{W} {Cin}/{Cm}/{C4} s{stride} g{groups}", seed)
        self.kind, self.stride, self.groups = kind, stride, groups
        self.identity = kind in ("residual_block", "grouped_residual_block")
        self.act("x", self.N, H, W, Cin)
        self.t["w1"], self.t["w3"] = LR.w11(self.rand, Cin, Cm), LR.w11(self.rand, Cm, C4)
        self.t["w2"] = LR.conv_w(self.rand, Cm, Cm // groups)
        self.bn(Cm, "b1", "s1"), self.bn(Cm, "b2", "s2"), self.bn(C4, "b3", "s3")
        if not self.identity:
            self.t["wp"] = LR.w11(self.rand, Cin, C4, 2)
            self.bn(C4, "bp", "sp")
        self.params = {}
        self.case_shape = {"N": self.N, "Hin": H, "Win": W, "Cin": Cin, "Cm": Cm, "C4": C4}   # (shape_sweeps.Case)
        if kind == "proj_block":
            self.case_shape["stride"] = stride
        self.out_shape = (self.N, (H - 1) // stride + 1, (W - 1) // stride + 1, C4)

    def run(self, pkg, d):
        bn = lambda i: (d[f"b{i}"], d[f"s{i}"])
        out = self.nan_out(d["x"].device)
        last = (d["w3"], bn(3)) if self.identity else (pkg.proj_tail_pack(d["w3"], bn(3), d["wp"], bn("p")),)
        if self.kind == "residual_block":
            return pkg.residual_block(d["x"], d["w1"], bn(1), pkg.filter_transform_f2(d["w2"]), bn(2), *last, out=out)
        if self.kind == "proj_block":
            return pkg.proj_block(d["x"], d["w1"], bn(1), pkg.filter_transform_f2(d["w2"]), bn(2), *last, self.stride,
                                  out=out)
        if self.kind == "proj_block_v15":
            return pkg.proj_block_v15(d["x"], d["w1"], bn(1), pkg.filter_pack_s2(d["w2"]), bn(2), *last, out=out)
        wg = pkg.filter_pack_grouped(d["w2"], self.groups)
        if self.kind == "grouped_residual_block":
            return pkg.grouped_residual_block(d["x"], d["w1"], bn(1), wg, bn(2), *last, self.groups, out=out)
        return pkg.grouped_proj_block(d["x"], d["w1"], bn(1), wg, bn(2), *last, self.groups, self.stride, out=out)

    def ref(self, t):
        bn = lambda i: (t[f"b{i}"], t[f"s{i}"])
        proj = () if self.identity else (t["wp"], bn("p"))
        return LR.bottleneck(t["x"], t["w1"], bn(1), t["w2"], bn(2), t["w3"], bn(3), *proj, stride=self.stride,
                             stride_on="first" if self.kind == "proj_block" else "3x3", groups=self.groups)   # v1: on the first 1x1


class Basic(Block):
    """basic_block (C -> C) and basic_block_s2 (C -> K at stride 2): padded in, padded out."""
    ring = 1

    def __init__(self, torch, H, W, C, K, s2, seed):
        super().__init__(torch, f"basic_block{'_s2' if s2 else ''} 2x{H}x{W} {C}->{K}", seed)
        self.s2 = s2
        self.act("x", self.N, H, W, C)
        self.t["w1"], self.t["w2"] = LR.conv_w(self.rand, K, C), LR.conv_w(self.rand, K, K)
        self.bn(K, "b1", "s1"), self.bn(K, "b2", "s2")
        if s2:
            self.t["wd"] = LR.conv_w(self.rand, K, C, k=1)
            self.bn(K, "bd", "sd")
        self.params = {}
        Ho, Wo = (s2_out(H), s2_out(W)) if s2 else (H, W)
        self.out_shape = (self.N, Ho + 2, Wo + 2, K)

    def run(self, pkg, d):
        x, out = _ring(d["x"]), self.nan_out(d["x"].device)
        U2, bn2 = pkg.filter_transform_f2(d["w2"]), (d["b2"], d["s2"])
        if not self.s2:
            return pkg.basic_block(x, pkg.filter_transform_f2(d["w1"]), (d["b1"], d["s1"]), U2, bn2, out=out)
        K, C = d["w1"].shape[:2]
        packed = pkg.s2_proj_pack(pkg.filter_pack_s2(d["w1"]), (d["b1"], d["s1"]),
                                  d["wd"].view(K, C).t().contiguous(), (d["bd"], d["sd"]))
        return pkg.basic_block_s2(x, packed, U2, bn2, out=out)

    def ref(self, t):
        bn1, bn2 = (t["b1"], t["s1"]), (t["b2"], t["s2"])
        if self.s2:
            return _ring(LR.basic_block_s2(t["x"], t["w1"], bn1, t["wd"], (t["bd"], t["sd"]), t["w2"], bn2)[2])
        return _ring(LR.basic_block(t["x"], t["w1"], bn1, t["w2"], bn2))


class FpnLevel(Block):
    """fpn_level with a top: (inner, P) stacked [2][N][H+2][W+2][Cf]; c and the coarser inner map are poisonable."""
    ring = 1
    main = "c"

    def __init__(self, torch, H, W, Cin, Cf, seed):
        super().__init__(torch, f"fpn_level 2x{H}x{W} {Cin}->{Cf}", seed)
        self.act("c", self.N, H, W, Cin)
        self.act("top", self.N, (H + 1) // 2, (W + 1) // 2, Cf)
        self.t["wl"], self.t["wo"] = LR.w11(self.rand, Cin, Cf), LR.conv_w(self.rand, Cf, Cf)
        self.t["bl"], self.t["bo"] = self.rand(Cf) - 0.5, self.rand(Cf) - 0.5
        self.out_shape = (2, self.N, H + 2, W + 2, Cf)

    def run(self, pkg, d):
        torch = self.torch
        one = self.out_shape[1:]
        inner, P = pkg.fpn_level(d["c"], d["wl"], d["bl"], pkg.filter_transform_f2(d["wo"]), d["bo"],
                                 top=_ring(d["top"], NAN), inner=torch.full(one, NAN, device=d["c"].device),
                                 out=torch.full(one, NAN, device=d["c"].device))
        return torch.stack((inner, P))

    def ref(self, t):
        inner, P = level_reference(self.torch, t["c"], LR.w1x1(t["wl"]), t["bl"], t["wo"], t["bo"], t["top"])
        return self.torch.stack((_ring(inner.contiguous()), _ring(P.contiguous())))


def blocks(torch):
    yield Bottleneck(torch, "residual_block", 7, 5, 128, 64, 128, 1, 1, seed=801)
    yield Bottleneck(torch, "proj_block", 15, 15, 128, 64, 128, 2, 1, seed=802)   # (odd: the strided 1x1 reads the last pixel;
    yield Bottleneck(torch, "proj_block_v15", 15, 15, 128, 64, 128, 2, 1, seed=803)   #  128 output pixels: stream-K is legal)
    yield Basic(torch, 7, 5, 64, 64, False, seed=804)
    yield Basic(torch, 9, 8, 32, 64, True, seed=805)
    yield Bottleneck(torch, "grouped_residual_block", 7, 5, 128, 128, 128, 1, 32, seed=806)
    yield Bottleneck(torch, "grouped_proj_block", 9, 8, 64, 128, 128, 2, 32, seed=807)
    yield FpnLevel(torch, 7, 5, 64, 64, seed=808)


BLOCKS = ["residual_block", "proj_block", "proj_block_v15", "basic_block", "basic_block_s2", "grouped_residual_block",
          "grouped_proj_block", "fpn_level"]


# ---- the cases: the smallest shapes at which each index path can go wrong ---------------------------------------------
# N = 3 at 7x5: 12 tiles per image, so one 64-tile item holds all three images and a clipped last tile column; 6x6: whole
# tiles.  C = 8 and 72 take the throughput kernel only (the latency kernel needs C % 16 == 0): C = 80 runs it.
SHAPES_3X3 = [(3, 7, 5), (3, 6, 6)]
CK_3X3 = [(C, K) for C in (8, 72, 80) for K in (64, 128)]
MODES_3X3 = {"plain": (True, False), "res": (True, False), "pool": (True, False)}   # mode -> the relu settings


def forms_3x3(N, H, W, K):
    """The forced forms of tests/shape_sweeps.py at this shape: the throughput kernel with a grid that leaves a stream-K
    tail and in whole rounds, the latency kernel with split 1 and split 2."""
    items = ((N * ((H + 1) // 2) * ((W + 1) // 2) + 63) // 64) * (K // 64)
    return {"auto": {},
            "big_tail": {"WINO_3X3_ALGO": "big", "WINO_SK_GRID": items + 1 + (items == 1)},   # 3 for 1 or 2 items
            "big_whole": {"WINO_3X3_ALGO": "big", "WINO_SK_GRID": items},
            "small_split1": {"WINO_3X3_ALGO": "small", "WINO_SMALL_CT": 1, "WINO_SMALL_SPLIT": 1},
            "small_split2": {"WINO_3X3_ALGO": "small", "WINO_SMALL_CT": 2, "WINO_SMALL_SPLIT": 2}}


def layers_3x3(torch, mode, N, H, W):
    for i, (C, K) in enumerate(CK_3X3):
        for relu in MODES_3X3[mode]:
            yield Conv3x3(torch, mode, relu, N, H, W, C, K, seed=1000 + 10 * i + relu + 100 * H)


# (3, 7, 5): M = 105 is one 112-row tile over three images; (3, 14, 14): 5 1/4 tiles that cross image boundaries
SHAPES_1X1 = [(3, 7, 5), (3, 14, 14), (1, 1, 1)]
CHANNELS_1X1 = [(32, 64), (160, 256)]
_F = Conv1x1
FLAGS_1X1 = [_F.RELU, _F.A_PADDED | _F.C_PADDED, _F.A_PADDED | _F.RELU | _F.ADD_RESIDUAL, _F.C_PADDED | _F.ADD_RESIDUAL,
             _F.ADD_RESIDUAL | _F.RESIDUAL_UP2 | _F.RELU,
             _F.ADD_RESIDUAL | _F.RESIDUAL_UP2 | _F.A_PADDED | _F.C_PADDED]   # every bit on and off


def layers_1x1(torch, N, H, W, Cin, Kout):
    for flags in FLAGS_1X1:
        yield Conv1x1(torch, flags, N, H, W, Cin, Kout, seed=2000 + flags + H + Cin)


S2_SHAPE = (3, 9, 8, 32, 64)


def layers_s2(torch):
    yield ConvS2(torch, False, True, *S2_SHAPE, seed=3001)
    yield ConvS2(torch, False, False, *S2_SHAPE, seed=3002)
    yield ConvS2(torch, True, True, *S2_SHAPE, seed=3003)


# 7x5 and 9x8 take 8-wide tiles at both strides; 6x12 takes 16-wide tiles at stride 1 and 5x20 (10 wide out) at stride 2
SHAPES_GROUPED = [(3, 7, 5), (3, 9, 8), (3, 6, 12), (3, 5, 20)]


def layers_grouped(torch, N, H, W):
    # Cg = 4, 8, 16 share a 16-channel MFMA tile among 4, 2, 1 groups (each its own select); 64 contracts over its group
    for Cg in (4, 8, 16, 64):
        for stride in (1, 2):
            yield Grouped(torch, stride == 1 or Cg == 4, stride, N, H, W, 128, Cg, seed=4000 + Cg + stride + H)


def layers_stem(torch):
    for i, (H, W, K) in enumerate([(3, 5, 128), (17, 9, 64), (1, 1, 64)]):   # the smallest maps of test_gpu_stem_head.py
        for padded in (False, True):
            yield Stem(torch, padded, 3, H, W, K, seed=5000 + 2 * i + padded)


def layers_head(torch):
    for i, (H, W, C, classes) in enumerate([(1, 1, 64, 10), (2, 3, 96, 70), (2, 3, 512, 128)]):
        for padded in (False, True):
            yield Head(torch, padded, 3, H, W, C, classes, seed=6000 + 2 * i + padded)


def layers_pack(torch):
    yield ImagePack(torch, 3, 3, 7, 5, 16, seed=7001)
    yield ImagePack(torch, 3, 1, 6, 6, 8, seed=7002)
    for i, (H, W, C) in enumerate([(7, 5, 8), (14, 14, 32), (1, 1, 4), (9, 8, 32)]):
        yield AvgPool7(torch, bool(i % 2), 3, H, W, C, seed=7010 + i)


def all_layers(torch):
    """Every single-launch layer of the GPU test, for the host test."""
    for mode in MODES_3X3:
        for shape in SHAPES_3X3:
            yield from layers_3x3(torch, mode, *shape)
    for shape in SHAPES_1X1:
        for ch in CHANNELS_1X1:
            yield from layers_1x1(torch, *shape, *ch)
    yield from layers_s2(torch)
    for shape in SHAPES_GROUPED:
        yield from layers_grouped(torch, *shape)
    yield from layers_stem(torch)
    yield from layers_head(torch)
    yield from layers_pack(torch)
