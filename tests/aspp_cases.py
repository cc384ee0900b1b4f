"""The concat projection's (wino_conv1x1_cat_bn_hw) and the ASPP module's (wino_aspp_hw) cases: fp64 numpy references
-- the concat layer as the GEMM over the concatenated sources with a bias row per image, the module as torchvision's
ASPP composed of tests/dilated_cases.py's dilated reference -- and the case classes with the library's run beside the
reference.  The module reference is proven against a float64 torch composition in tests/test_aspp_host.py.  Nothing here
needs a GPU to import."""
import numpy as np

from cases import TIGHT, ring_mask
from dilated_cases import dilated_reference

A_PADDED, C_PADDED, RELU = 2, 4, 1

# (N, H, W, S, Cs, Kout): the concat layer's parity shapes
CAT_SHAPES = [
    (2, 9, 9, 4, 64, 64),        # the basic case
    (5, 5, 5, 2, 32, 64),        # one tile spans five images' biases, one k-step per source
    (3, 7, 11, 5, 96, 192),      # tile boundaries mid-image, three k-steps per source, Kout % 128 != 0
    (8, 1, 1, 4, 64, 128),       # every row its own image
    (2, 17, 13, 3, 64, 64),      # three sources, each image about two tiles, the image boundary mid-tile
    (1, 33, 33, 4, 256, 256),    # DeepLab's own source width, ten tiles
]
# the forced forms: 8-wave tiles with 2 k-steps per source, 4-wave tiles with 3 per source
CAT_FORM_SHAPES = [(2, 28, 28, 4, 64, 256), (3, 15, 13, 5, 96, 128)]
# (N, H, W, Cin, Cb, Kout, rates): the module's parity shapes
ASPP_SHAPES = [
    (2, 9, 9, 64, 64, 64, (1, 2, 3)),            # the basic case
    (1, 7, 11, 128, 64, 128, (2, 4, 12)),        # rate 12 overreaches the map
    (3, 5, 5, 96, 128, 64, (12, 24, 36)),        # torchvision's rates, only centre taps
    (1, 33, 33, 256, 256, 256, (4, 8, 12)),      # DeepLab's branch width
]


def cat_reference(srcs, w, bias_per_image, scale, relu):
    """fp64: srcs S x [N][H][W][Cs], w [S*Cs][Kout], bias_per_image [N][Kout], scale [Kout] -> [N][H][W][Kout]."""
    a = np.concatenate([np.asarray(s, np.float64) for s in srcs], axis=-1)
    y = a @ np.asarray(w, np.float64) * np.asarray(scale, np.float64)
    y = y + np.asarray(bias_per_image, np.float64)[:, None, None, :]
    return np.maximum(y, 0) if relu else y


def aspp_reference(xp, w0, bn0, ws, bns, rates, w_pool, bn_pool, w_proj, bn_proj, pooled=True):
    """fp64 ASPP.  xp [N][H+2][W+2][Cin] (zero ring); w0, w_pool [Cin][Cb]; ws three [Cb][Cin][3][3]; w_proj [5 Cb][Kout];
    bn = (bias, scale).  pooled=False leaves the pooled branch out of the join (its rows of w_proj meet zeros): what a
    dropped per-image bias would compute.  Returns [N][H][W][Kout]."""
    f = lambda a: np.asarray(a, np.float64)
    xp = f(xp)
    x = xp[:, 1:-1, 1:-1, :]
    N, H, W, Cin = x.shape
    act = lambda y, bn: np.maximum(y * f(bn[1]) + f(bn[0]), 0)
    branches = [act(x @ f(w0), bn0)]
    for w, bn, d in zip(ws, bns, rates):
        branches.append(dilated_reference(xp, f(w), f(bn[1]), f(bn[0]), d, True))
    bp = act(x.mean(axis=(1, 2)) @ f(w_pool), bn_pool)                       # [N][Cb]
    bp = np.broadcast_to(bp[:, None, None, :], branches[0].shape) if pooled else np.zeros_like(branches[0])
    return act(np.concatenate(branches + [bp], axis=-1) @ f(w_proj), bn_proj)


class CatLayer:
    """One concat layer's tensors.  The sources live in one device buffer `spacing` floats apart; with gap > 0 the
    spacing exceeds a source by `gap` floats of NaN, and padded sources carry NaN rings: neither may reach a result."""

    def __init__(self, pkg, torch_dev, N, H, W, S, Cs, Kout, seed):
        self.torch, self.dev = torch_dev
        self.pkg = pkg
        torch = self.torch
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.srcs = [torch.rand(N, H, W, Cs, generator=g) - 0.5 for _ in range(S)]
        self.w = (torch.rand(S * Cs, Kout, generator=g) - 0.5) / np.sqrt(S * Cs) * 4
        self.bias = torch.rand(N, Kout, generator=g) - 0.5          # a row of its own per image
        self.scale = torch.rand(Kout, generator=g) + 0.5
        self.wt, self.bt, self.st = self.w.to(self.dev), self.bias.to(self.dev), self.scale.to(self.dev)
        self.N, self.H, self.W, self.S, self.Cs, self.Kout = N, H, W, S, Cs, Kout
        self._ref = {}

    def sources(self, padded=False, gap=0):
        """The S sources as views of one NaN-filled device buffer, `gap` floats (a multiple of 4) between them."""
        torch = self.torch
        p = 2 if padded else 0
        shape = (self.N, self.H + p, self.W + p, self.Cs)
        n = int(np.prod(shape))
        buf = torch.full((self.S * (n + gap),), float("nan"), device=self.dev)
        views = []
        for j, s in enumerate(self.srcs):
            v = buf[j * (n + gap): j * (n + gap) + n].view(shape)
            (v[:, 1:-1, 1:-1, :] if padded else v).copy_(s)
            views.append(v)
        return views

    def run(self, relu=True, a_padded=False, c_padded=False, gap=0, srcs=None, bias=None, out=None):
        flags = (RELU if relu else 0) | (A_PADDED if a_padded else 0) | (C_PADDED if c_padded else 0)
        p = 2 if c_padded else 0
        if out is None:
            out = self.torch.full((self.N, self.H + p, self.W + p, self.Kout), float("nan"), device=self.dev)
        if srcs is None:
            srcs = self.sources(a_padded, gap)
        return self.pkg.conv1x1_cat_bn(srcs, self.wt, self.bt if bias is None else bias, self.st, flags, out=out)

    def reference(self, relu=True):
        if relu not in self._ref:   # computed once, shared, left unchanged
            r = cat_reference([s.numpy() for s in self.srcs], self.w.numpy(), self.bias.numpy(), self.scale.numpy(), relu)
            r.setflags(write=False)
            self._ref[relu] = r
        return self._ref[relu]

    def check(self, O, got, relu=True, c_padded=False, what=""):
        g = got.cpu().numpy()
        assert np.isfinite(g).all(), what
        if c_padded:
            assert (g[:, ring_mask(self.H, self.W), :] == 0).all(), "output ring is not zero"
            g = g[:, 1:-1, 1:-1, :]
        want = self.reference(relu)
        assert g.shape == want.shape
        err = O.rel_error(g, want)
        print(f"concat 1x1 {self.N}x{self.H}x{self.W} S={self.S} Cs={self.Cs} Kout={self.Kout} relu={relu} {what}: "
              f"rel err {err:.2e}")
        assert err < TIGHT
        if relu:
            assert (want > 0).mean() > 0.2   # both sides of the ReLU


class AsppCase:
    """One ASPP module's tensors and its fp64 reference.  Image n's input has mean 0.4 (n + 1): the pooled branch then
    differs from image to image and carries weight in the result (checked on the CPU by pooled_share)."""

    def __init__(self, pkg, torch_dev, N, H, W, Cin, Cb, Kout, rates, seed):
        self.torch, self.dev = torch_dev
        self.pkg = pkg
        torch = self.torch
        g = torch.Generator(device="cpu").manual_seed(seed)
        r = lambda *s: torch.rand(*s, generator=g) - 0.5
        x = torch.zeros(N, H + 2, W + 2, Cin)
        x[:, 1:-1, 1:-1, :] = r(N, H, W, Cin) + 0.4 * (torch.arange(N, dtype=torch.float32)[:, None, None, None] + 1)
        self.x = x
        self.w0 = r(Cin, Cb) / np.sqrt(Cin) * 4
        self.ws = [r(Cb, Cin, 3, 3) / np.sqrt(9 * Cin) * 4 for _ in range(3)]      # [K][C][3][3]
        self.w_pool = r(Cin, Cb) / np.sqrt(Cin) * 4
        self.w_proj = r(5 * Cb, Kout) / np.sqrt(5 * Cb) * 4
        self.bn = [(r(c), r(c) + 1.0) for c in (Cb, Cb, Cb, Cb, Cb, Kout)]         # b0, three dilated, pool, proj: (bias, scale)
        self.rates = tuple(rates)
        self.N, self.H, self.W, self.Cin, self.Cb, self.Kout = N, H, W, Cin, Cb, Kout
        self._ref = {}
        if pkg is not None:
            t = lambda a: a.contiguous().to(self.dev)
            self.xt, self.w0t, self.w_poolt, self.w_projt = t(self.x), t(self.w0), t(self.w_pool), t(self.w_proj)
            self.taps = [pkg.filter_pack_s2(t(w)) for w in self.ws]
            self.bnt = [(t(b), t(s)) for b, s in self.bn]

    def workspace_bytes(self):
        return self.pkg.aspp_workspace_bytes(self.N, self.H, self.W, self.Cin, self.Cb, self.Kout)

    def run(self, out=None, workspace=None, x=None):
        torch = self.torch
        if out is None:
            out = torch.full((self.N, self.H + 2, self.W + 2, self.Kout), float("nan"), device=self.dev)
        if workspace is None:
            workspace = torch.full((self.workspace_bytes() // 4,), float("nan"), device=self.dev)
        return self.pkg.aspp(self.xt if x is None else x, self.w0t, self.bnt[0], self.taps, self.bnt[1:4], self.rates,
                             self.w_poolt, self.bnt[4], self.w_projt, self.bnt[5], out=out, workspace=workspace)

    def reference(self, pooled=True):
        if pooled not in self._ref:   # computed once, shared, left unchanged
            n = lambda a: a.numpy()
            bn = [(n(b), n(s)) for b, s in self.bn]
            ref = aspp_reference(n(self.x), n(self.w0), bn[0], [n(w) for w in self.ws], bn[1:4], self.rates,
                                 n(self.w_pool), bn[4], n(self.w_proj), bn[5], pooled)
            ref.setflags(write=False)
            self._ref[pooled] = ref
        return self._ref[pooled]

    def pooled_share(self):
        """max |full - without the pooled branch| / max |full|, per image: what a dropped per-image bias would cost."""
        full, without = self.reference(True), self.reference(False)
        return [float(np.abs(full[n] - without[n]).max() / np.abs(full).max()) for n in range(self.N)]

    def check(self, O, got):
        g = got.cpu().numpy()
        assert np.isfinite(g).all()
        assert (g[:, ring_mask(self.H, self.W), :] == 0).all(), "output ring is not zero"
        want = self.reference()
        err = O.rel_error(g[:, 1:-1, 1:-1, :], want)
        print(f"aspp {self.N}x{self.H}x{self.W} Cin={self.Cin} Cb={self.Cb} Kout={self.Kout} rates={self.rates}: "
              f"rel err {err:.2e}")
        assert err < TIGHT
        assert (want > 0).mean() > 0.2   # both sides of the final ReLU
        assert self.pkg.tickets_in_use() == 0
