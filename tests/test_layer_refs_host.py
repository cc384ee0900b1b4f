"""tests/layer_refs.py pinned, on the CPU: each function against a restatement that shares no code with it and never
calls F.conv2d -- explicit tap loops over shifted slices in numpy fp64 (`taps`), or the composition of the oracle's own
layers (oracle.conv1x1_bn / conv3x3_bn_relu_direct / residual_block) for the ungrouped bottlenecks.

The shapes are the smallest at which an indexing slip shows: N = 2, 5 x 4 (odd by even, not square: at stride 2 the
3 x 2 output's last row reads the last input row and its last column does not), C = 4, K = 6, two groups, a 3 x 2 top,
the pool dropping the odd row, the stem on 2 x 3 x 9 x 10, avgpool7 on 9 x 8, two basic blocks in a row.

The bar, rel < 1e-12: both sides are fp64 and a sum has at most 9 * 49 * 3 = 1323 terms, 1323 * 2.2e-16 = 3e-13, with
one order of magnitude left for the different order of summation.  Each function also gets one NaN planted in one input
element: both restatements are NaN at exactly the same outputs (here the ReLU is where(y < 0, 0, y), which keeps NaN)."""
import numpy as np
import pytest
import torch

import layer_refs as LR

BAR = 1e-12
N, H, W, C, K = 2, 5, 4, 4, 6


# ---- the restatement --------------------------------------------------------------------------------------------------
def taps(x, w, stride=1, pad=1, groups=1):
    """x [N][H][W][C], w [K][C/groups][kh][kw] -> [N][Ho][Wo][K]: one einsum per tap over a strided slice of the
    zero-padded input."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    n, h, wd, c = x.shape
    k, cg, kh, kw = w.shape
    ho, wo = (h + 2 * pad - kh) // stride + 1, (wd + 2 * pad - kw) // stride + 1
    xp = np.zeros((n, h + 2 * pad, wd + 2 * pad, c))
    xp[:, pad:pad + h, pad:pad + wd, :] = x
    y, kg = np.zeros((n, ho, wo, k)), k // groups
    for g in range(groups):
        for r in range(kh):
            for s in range(kw):
                patch = xp[:, r:r + stride * (ho - 1) + 1:stride, s:s + stride * (wo - 1) + 1:stride, g * cg:(g + 1) * cg]
                y[..., g * kg:(g + 1) * kg] += np.einsum("nhwc,kc->nhwk", patch, w[g * kg:(g + 1) * kg, :, r, s])
    return y


def bn(y, p):
    return y * np.asarray(p[1], np.float64) + np.asarray(p[0], np.float64)


def relu(y):
    return np.where(y < 0, 0, y)


def one(w_io):
    """[Cin][Cout] -> [Cout][Cin][1][1]."""
    return np.asarray(w_io, np.float64).T[:, :, None, None]


def pool(y, k, stride, pad):
    """Max-pool of [N][H][W][C] with -inf padding; np.maximum keeps a NaN."""
    n, h, w, c = y.shape
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    yp = np.full((n, h + 2 * pad, w + 2 * pad, c), -np.inf)
    yp[:, pad:pad + h, pad:pad + w, :] = y
    out = np.full((n, ho, wo, c), -np.inf)
    for r in range(k):
        for s in range(k):
            out = np.maximum(out, yp[:, r:r + stride * (ho - 1) + 1:stride, s:s + stride * (wo - 1) + 1:stride, :])
    return out


def up2(top, h, w):
    return np.asarray(top, np.float64)[:, np.arange(h) >> 1][:, :, np.arange(w) >> 1]


# ---- the draws and the two checks -------------------------------------------------------------------------------------
@pytest.fixture
def rand():
    g = torch.Generator().manual_seed(1234)
    return lambda *shape: torch.rand(*shape, generator=g)


def act(rand, *shape):
    return rand(*shape) - 0.5


def check(ref, mine, x, tag="", at=(1, -1, -2, -3)):
    """`ref(x)` (layer_refs) against `mine(x)` (the restatement), each a tensor or a tuple of them: at BAR on the clean
    input, and the same NaN set with one NaN planted in x[at] (image 1, the last row, an even column: a stride of 2
    reads it)."""
    tup = lambda r: r if isinstance(r, tuple) else (r,)
    for a, b in zip(tup(ref(x)), tup(mine(x.numpy())), strict=True):
        assert a.dtype == torch.float64, tag
        assert LR.rel(a, b) < BAR, tag
    xn = x.clone()
    xn[at] = float("nan")
    hit = 0
    for a, b in zip(tup(ref(xn)), tup(mine(xn.numpy())), strict=True):
        nan = torch.isnan(a).numpy()
        assert np.array_equal(nan, np.isnan(b)), f"{tag}: the NaN sets differ"
        assert np.isfinite(b[~nan]).all() and LR.rel(a[~torch.isnan(a)], b[~nan]) < BAR, tag
        hit += int(nan.sum())
        assert not nan.all(), f"{tag}: NaN everywhere says nothing"
    assert hit > 0, f"{tag}: the NaN reached no output"


# ---- the small pieces -------------------------------------------------------------------------------------------------
def test_small_pieces(rand):
    x = act(rand, N, H, W, C)
    assert LR.nchw(x).shape == (N, C, H, W) and LR.nchw(x).dtype == torch.float64
    assert torch.equal(LR.nhwc(LR.nchw(x)), x.double())
    assert torch.equal(LR.nchw(x.numpy()), LR.nchw(x))                       # numpy in, the same values
    b, s = rand(C), rand(C)
    assert torch.equal(LR.affine(LR.nchw(x), (b, s)), LR.nchw(x.double() * s.double() + b.double()))
    w = rand(C, K)
    assert LR.w1x1(w).shape == (K, C, 1, 1) and float(LR.w1x1(w)[5, 2, 0, 0]) == float(w[2, 5])
    xp = LR.ring(x, 7.0)
    assert xp.shape == (N, H + 2, W + 2, C) and torch.equal(LR.interior(xp), x)
    m = LR.ring_mask(H, W)
    assert m.shape == (H + 2, W + 2) and m.sum() == 2 * (H + 2) + 2 * W and bool((xp[:, m, :] == 7.0).all())
    assert LR.ring_is(xp, 7.0) and not LR.ring_is(xp, 0.0) and LR.ring_is(LR.ring(x)) and LR.ring_is(xp.numpy(), 7.0)
    for spot in ((0, 0, 2), (1, H + 1, 0), (0, 3, 0), (1, 2, W + 1)):       # one pixel of each side
        bad = xp.clone()
        bad[spot] = 0.0
        assert not LR.ring_is(bad, 7.0), spot
    assert torch.isnan(LR.ring(x, float("nan"))[0, 0, 0, 0])
    y = LR.fill_ring(xp.clone())
    assert LR.ring_is(y) and torch.equal(LR.interior(y), x)


def test_rel():
    want = torch.tensor([[1.0, -4.0], [2.0, 0.0]], dtype=torch.float64)
    got = want.float() + torch.tensor([[0.0, 0.0], [0.5, 0.0]])
    assert LR.rel(got, want) == 0.125 and LR.rel(got.numpy(), want.numpy()) == 0.125
    assert LR.rel(torch.zeros(2), torch.zeros(2), floor=1e-30) == 0.0
    assert LR.rel(torch.full((2,), 1e-31), torch.zeros(2), floor=1e-30) == pytest.approx(0.1)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(AssertionError, match="got holds non-finite"):
            LR.rel(torch.tensor([1.0, bad]), torch.ones(2))
        with pytest.raises(AssertionError, match="the reference holds non-finite"):
            LR.rel(torch.ones(2), torch.tensor([1.0, bad]))
    with pytest.raises(AssertionError):
        LR.rel(torch.ones(2, 1), torch.ones(2))


def test_draws(rand):
    w = LR.conv_w(rand, K, C)
    assert w.shape == (K, C, 3, 3) and float(w.abs().max()) <= 2 / np.sqrt(9 * C)
    assert LR.conv_w(rand, K, C, k=1).shape == (K, C, 1, 1)
    assert LR.w11(rand, C, K).shape == (C, K) and float(LR.w11(rand, C, K, 2).abs().max()) <= 1 / np.sqrt(C)
    bias, scale = LR.bn_pair(rand, 7)
    assert [bool(v < 0) for v in scale] == [True, False, False, True, False, False, True]
    assert float(bias.abs().max()) <= 0.5 and float(scale.abs().min()) >= 0.5
    assert bool((LR.bn_pair(rand, 7, negative_third=False)[1] > 0).all())
    # the draw order is the caller's: bias first, then scale
    g1, g2 = (torch.Generator().manual_seed(5) for _ in range(2))
    b, s = LR.bn_pair(lambda *sh: torch.rand(*sh, generator=g1), 4, negative_third=False)
    assert torch.equal(b, torch.rand(4, generator=g2) - 0.5) and torch.equal(s, torch.rand(4, generator=g2) + 0.5)


# ---- the layers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("stride,groups", [(1, 1), (2, 1), (1, 2), (2, 2)])
def test_conv3x3(stride, groups, with_res, on, rand):
    x, w, p = act(rand, N, H, W, C), LR.conv_w(rand, K, C // groups), LR.bn_pair(rand, K)
    res = act(rand, N, (H - 1) // stride + 1, (W - 1) // stride + 1, K) if with_res else None
    act_ = relu if on else (lambda y: y)
    mine = lambda v: act_(bn(taps(v, w, stride, 1, groups), p) + (res.numpy().astype(np.float64) if with_res else 0))
    check(lambda v: LR.conv3x3(v, w, p, on, stride=stride, groups=groups, residual=res), mine, x)
    if stride == 2:
        assert LR.conv3x3(x, w, p, on, stride=2, groups=groups).shape == (N, 3, 2, K)


@pytest.mark.parametrize("on", [True, False], ids=["relu", "linear"])
def test_conv3x3_pool_and_own_border(on, rand):
    x, w, p = act(rand, N, H, W, C), LR.conv_w(rand, K, C), LR.bn_pair(rand, K)
    act_ = relu if on else (lambda y: y)
    got = LR.conv3x3(x, w, p, on, pool=True)
    assert got.shape == (N, 2, 2, K)                                         # the odd fifth row is dropped
    check(lambda v: LR.conv3x3(v, w, p, on, pool=True), lambda v: pool(act_(bn(taps(v, w), p)), 2, 2, 0), x)
    # padding=0: the zero ring of a padded input is the padding
    assert torch.equal(LR.conv3x3(LR.ring(x), w, p, on, padding=0), LR.conv3x3(x, w, p, on))
    # a NaN residual element stays in its own element
    res = act(rand, N, H, W, K)
    res[1, 2, 3, 4] = float("nan")
    nan = torch.isnan(LR.conv3x3(x, w, p, on, residual=res))
    assert int(nan.sum()) == 1 and bool(nan[1, 2, 3, 4])


@pytest.mark.parametrize("on", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("form", ["plain", "residual", "up2", "stride2"])
def test_conv1x1(form, on, rand):
    x, w, p = act(rand, N, H, W, C), LR.w11(rand, C, K), LR.bn_pair(rand, K)
    res = act(rand, N, H, W, K) if form == "residual" else None
    top = act(rand, N, 3, 2, K) if form == "up2" else None
    stride = 2 if form == "stride2" else 1
    act_ = relu if on else (lambda y: y)
    add = res.numpy().astype(np.float64) if res is not None else up2(top.numpy(), H, W) if top is not None else 0
    mine = lambda v: act_(bn(taps(v, one(w), stride, 0), p) + add)
    check(lambda v: LR.conv1x1(v, w, p, on, stride=stride, residual=res, top=top), mine, x)
    if top is not None:   # the coarser map's pixel (1, 2, 1) lands on rows 4 (5 is past the map) and columns 2, 3
        top[1, 2, 1, 0] = float("nan")
        nan = torch.isnan(LR.conv1x1(x, w, p, on, top=top))
        assert int(nan.sum()) == 2 and bool(nan[1, 4, 2, 0]) and bool(nan[1, 4, 3, 0])


def test_basic_block_s2_and_its_first_layer(rand):
    x = act(rand, N, H, W, C)
    w1, wd, w2 = LR.conv_w(rand, K, C), LR.conv_w(rand, K, C, k=1), LR.conv_w(rand, K, K)
    p1, pd, p2 = (LR.bn_pair(rand, K) for _ in range(3))
    t1 = lambda v: relu(bn(taps(v, w1, 2), p1))
    sc = lambda v: bn(taps(v, wd, 2, 0), pd)
    check(lambda v: LR.basic_block_s2(v, w1, p1, wd, pd)[:2], lambda v: (t1(v), sc(v)), x, "layer")
    assert LR.basic_block_s2(x, w1, p1, wd, pd)[2] is None
    for pre in (False, True):
        out = lambda v: (relu if not pre else (lambda y: y))(bn(taps(t1(v), w2), p2) + sc(v))
        check(lambda v: LR.basic_block_s2(v, w1, p1, wd, pd, w2, p2, pre=pre), lambda v: (t1(v), sc(v), out(v)), x,
              f"block pre={pre}")
    assert LR.basic_block_s2(x, w1, p1, wd, pd, w2, p2)[2].shape == (N, 3, 2, K)


@pytest.mark.parametrize("blocks", [1, 2])
def test_basic_block(blocks, rand):
    x, w1, w2 = act(rand, N, H, W, C), LR.conv_w(rand, C, C), LR.conv_w(rand, C, C)
    p1, p2 = LR.bn_pair(rand, C), LR.bn_pair(rand, C)

    def mine(v, pre=False):
        v = np.asarray(v, np.float64)
        for i in range(blocks):
            y = bn(taps(relu(bn(taps(v, w1), p1)), w2), p2) + v
            v = relu(y)
        return y if pre else v
    check(lambda v: LR.basic_block(v, w1, p1, w2, p2, blocks), mine, x)
    check(lambda v: LR.basic_block(v, w1, p1, w2, p2, blocks, pre=True), lambda v: mine(v, True), x, "pre")


def _oracle_bottleneck(O, x, s, w1, p1, w2, p2, w3, p3, wp=None, pp=None):
    """The composition of the oracle's layers: xs = x[:, ::s, ::s], 1x1 + BN + ReLU, 3x3 (pad 1) + BN + ReLU, 1x1 + BN,
    + xs or + BN(xs . wp), ReLU."""
    n = lambda a: a.numpy() if hasattr(a, "numpy") else a
    w1, w2, w3, p1, p2, p3 = n(w1), n(w2), n(w3), [n(v) for v in p1], [n(v) for v in p2], [n(v) for v in p3]
    xs = np.asarray(x, np.float64)[:, ::s, ::s, :]
    if wp is None:
        return O.residual_block(xs, w1, p1, w2, p2, w3, p3)
    n_, h, w, cin = xs.shape
    cm = w1.shape[1]
    t1p = np.zeros((n_, h + 2, w + 2, cm))
    t1p[:, 1:-1, 1:-1, :] = O.conv1x1_bn(xs.reshape(-1, cin), w1, p1[0], p1[1], True).reshape(n_, h, w, cm)
    t2 = O.conv3x3_bn_relu_direct(t1p, w2, p2[1], p2[0], True)[:, 1:-1, 1:-1, :]
    t3 = O.conv1x1_bn(t2.reshape(-1, cm), w3, p3[0], p3[1], False)
    sc = O.conv1x1_bn(xs.reshape(-1, cin), n(wp), n(pp[0]), n(pp[1]), False)
    return np.maximum(t3 + sc, 0).reshape(n_, h, w, -1)


BOTTLENECKS = {"identity": (False, 1, "first", 1), "v1 stride 1": (True, 1, "first", 1), "v1 stride 2": (True, 2, "first", 1),
               "v1.5": (True, 2, "3x3", 1), "grouped identity": (False, 1, "3x3", 2), "grouped stride 1": (True, 1, "3x3", 2),
               "grouped stride 2": (True, 2, "3x3", 2)}


@pytest.mark.parametrize("kind", sorted(BOTTLENECKS))
def test_bottleneck(kind, rand, O):
    proj, stride, on, groups = BOTTLENECKS[kind]
    Cm, C4 = 4, (K if proj else C)
    x = act(rand, N, H, W, C)
    w1, w2, w3 = LR.w11(rand, C, Cm), LR.conv_w(rand, Cm, Cm // groups), LR.w11(rand, Cm, C4)
    p1, p2, p3 = LR.bn_pair(rand, Cm), LR.bn_pair(rand, Cm), LR.bn_pair(rand, C4)
    wp, pp = (LR.w11(rand, C, C4, 2), LR.bn_pair(rand, C4)) if proj else (None, None)

    def mine(v, pre=False):
        v = np.asarray(v, np.float64)
        s1, s2 = (stride, 1) if on == "first" else (1, stride)
        t2 = relu(bn(taps(relu(bn(taps(v, one(w1), s1, 0), p1)), w2, s2, 1, groups), p2))
        y = bn(taps(t2, one(w3), 1, 0), p3) + (bn(taps(v, one(wp), stride, 0), pp) if proj else v)
        return y if pre else relu(y)
    ref = lambda v, pre=False: LR.bottleneck(v, w1, p1, w2, p2, w3, p3, wp, pp, stride=stride, stride_on=on,
                                             groups=groups, pre=pre)
    check(ref, mine, x)
    check(lambda v: ref(v, True), lambda v: mine(v, True), x, "pre")
    assert ref(x).shape == (N, (H - 1) // stride + 1, (W - 1) // stride + 1, C4)
    if on == "first" and groups == 1:   # the oracle's own layers, composed
        check(ref, lambda v: _oracle_bottleneck(O, v, stride, w1, p1, w2, p2, w3, p3, wp, pp), x, "oracle")


def test_stem(rand):
    x = rand(2, 3, 9, 10) * 2 - 1
    w, p = (rand(K, 3, 7, 7) - 0.5) * 0.3, LR.bn_pair(rand, K)
    pre = lambda v: bn(taps(np.transpose(v, (0, 2, 3, 1)), w, 2, 3), p)
    check(lambda v: LR.stem(v, w, p), lambda v: pool(relu(pre(v)), 3, 2, 1), x)
    check(lambda v: LR.stem(v, w, p, pre=True), pre, x, "pre")
    assert LR.stem(x, w, p).shape == (2, 3, 3, K) and LR.stem(x, w, p, pre=True).shape == (2, 5, 5, K)


def test_avgpool_fc_and_avgpool7(rand):
    feat, wfc, bfc = rand(N, H, W, C) * 2, LR.w11(rand, K, C, 2), rand(K) - 0.5
    head = lambda v: np.einsum("nhwc,kc->nk", np.asarray(v, np.float64), wfc.numpy().astype(np.float64)) / (H * W) + bfc.numpy()
    check(lambda v: LR.avgpool_fc(v, wfc, bfc), head, feat, "avgpool_fc")
    assert LR.avgpool_fc(feat, wfc, bfc).shape == (N, K)

    def bins(v):
        v = np.asarray(v, np.float64)
        n, h, w, c = v.shape
        out = np.zeros((n, 7, 7, c))
        for i in range(7):
            for j in range(7):
                out[:, i, j] = v[:, (i * h) // 7:-((-(i + 1) * h) // 7), (j * w) // 7:-((-(j + 1) * w) // 7)].mean(axis=(1, 2))
        return out
    check(LR.avgpool7, bins, act(rand, N, 9, 8, C), "avgpool7")
