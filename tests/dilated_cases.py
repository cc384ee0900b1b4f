"""The dilated 3x3 layer's and the dilated bottleneck blocks' cases: an fp64 numpy reference of the layer (an im2col
with the taps outside the image redirected to a pixel of the zero ring, the layer's own definition), the footprint of
one input element, and the case classes with the library's run beside the reference.  The reference and the footprint
are proven against torch's conv2d(padding=d, dilation=d) in tests/test_dilated_host.py.  Nothing here needs a GPU to
import."""
import numpy as np

from cases import TIGHT, ring_mask

# (N, H, W, C, K, d): the parity shapes
LAYER_SHAPES = [
    (2, 9, 9, 64, 128, 2),       # the basic case
    (1, 7, 7, 64, 64, 4),        # the dilation is past half the map
    (2, 5, 9, 96, 192, 3),       # an odd dilation, 3 k-steps per tap, K % 128 != 0
    (1, 3, 3, 32, 64, 12),       # only the centre tap is in the image
    (8, 1, 1, 64, 128, 2),       # a 1x1 map
    (2, 17, 13, 128, 64, 4),     # a 112-row tile straddles two images
    (1, 33, 33, 256, 256, 2),    # ten row tiles, boundaries mid-line
    (2, 14, 14, 64, 64, 1),      # also against conv3x3_direct
]
# the forced forms: 8-wave tiles with 2 k-steps per tap, 4-wave tiles with 3 per tap
FORM_SHAPES = [(2, 28, 28, 64, 256, 2), (3, 15, 13, 96, 128, 4)]
FORMS = {
    "tiled": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 0},
    "stream_k": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1},
    # ranges that start and end inside taps (C / 32 k-steps per tap)
    "split_24": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1, "WINO_1X1_SK_GRID": 24},
    "split_40": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1, "WINO_1X1_SK_GRID": 40},
    "split_104": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1, "WINO_1X1_SK_GRID": 104},
}
# (N, H, W, Cin, Cm, C4, d)
RESIDUAL_BLOCK = (2, 9, 9, 256, 64, 256, 2)
PROJ_BLOCK = (1, 7, 11, 128, 64, 256, 4)


def dilated_reference(xp, w, scale, bias, d, relu=True):
    """fp64: xp [N][H+2][W+2][C] (ring of width one, zero), w [K][C][3][3] -> [N][H][W][K].  Tap (dy, dx) of output pixel
    (y, x) is padded pixel (1 + y + d(dy-1), 1 + x + d(dx-1)) when that is inside the image, and the ring pixel (1 + y, 0)
    of the pixel's own padded line otherwise."""
    xp = np.asarray(xp, np.float64)
    w = np.asarray(w, np.float64)
    N, Hp, Wp, C = xp.shape
    H, W, K = Hp - 2, Wp - 2, w.shape[0]
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    cols = np.empty((N, H, W, 9, C))
    for dy in range(3):
        for dx in range(3):
            ty, tx = ys + d * (dy - 1), xs + d * (dx - 1)
            ok = (ty >= 0) & (ty < H) & (tx >= 0) & (tx < W)
            py = np.where(ok, ty + 1, ys + 1)
            px = np.where(ok, tx + 1, 0)
            cols[:, :, :, 3 * dy + dx, :] = xp[:, py, px, :]
    B = w.transpose(2, 3, 1, 0).reshape(9 * C, K)
    y = cols.reshape(N * H * W, 9 * C) @ B
    y = y * np.asarray(scale, np.float64)[None, :] + np.asarray(bias, np.float64)[None, :]
    if relu:
        y = np.maximum(y, 0)
    return y.reshape(N, H, W, K)


def footprint(H, W, y, x, d):
    """The output pixels that read input pixel (y, x): (y - d(dy-1), x - d(dx-1)) inside the image, as a bool [H][W]."""
    m = np.zeros((H, W), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            oy, ox = y - d * dy, x - d * dx
            if 0 <= oy < H and 0 <= ox < W:
                m[oy, ox] = True
    return m


class DilLayer:
    """One layer's tensors: the padded input with a zero ring, [K][C][3][3] weights, folded BN vectors."""

    def __init__(self, pkg, torch_dev, N, H, W, C, K, d, seed):
        self.torch, self.dev = torch_dev
        self.pkg = pkg
        torch = self.torch
        g = torch.Generator(device="cpu").manual_seed(seed)
        x = torch.zeros(N, H + 2, W + 2, C)
        x[:, 1:-1, 1:-1, :] = torch.rand(N, H, W, C, generator=g) - 0.5
        self.x = x
        self.w = (torch.rand(K, C, 3, 3, generator=g) - 0.5) / np.sqrt(9 * C) * 4
        self.bias = torch.rand(K, generator=g) - 0.5
        self.scale = torch.rand(K, generator=g) + 0.5
        self.xt, self.wt = x.to(self.dev), self.w.to(self.dev)
        self.bt, self.st = self.bias.to(self.dev), self.scale.to(self.dev)
        self.taps = pkg.filter_pack_s2(self.wt)
        self.N, self.H, self.W, self.C, self.K, self.d = N, H, W, C, K, d
        self._ref = {}

    def run(self, relu=True, x=None, out=None):
        if out is None:
            out = self.torch.full((self.N, self.H + 2, self.W + 2, self.K), float("nan"), device=self.dev)
        return self.pkg.conv3x3_dilated_bn_relu(self.xt if x is None else x, self.taps, self.bt, self.st, self.d,
                                                relu=relu, out=out)

    def reference(self, relu=True):
        if relu not in self._ref:   # computed once, shared, left unchanged
            r = dilated_reference(self.x.numpy(), self.w.numpy(), self.scale.numpy(), self.bias.numpy(), self.d, relu)
            r.setflags(write=False)
            self._ref[relu] = r
        return self._ref[relu]

    def check(self, O, got, relu=True):
        g = got.cpu().numpy()
        assert np.isfinite(g).all()
        assert (g[:, ring_mask(self.H, self.W), :] == 0).all(), "output ring is not zero"
        want = self.reference(relu)
        err = O.rel_error(g[:, 1:-1, 1:-1, :], want)
        print(f"dilated {self.N}x{self.H}x{self.W} C={self.C} K={self.K} d={self.d} relu={relu}: rel err {err:.2e}")
        assert err < TIGHT
        if relu:
            assert (want > 0).mean() > 0.2   # both sides of the ReLU


class DilBlock:
    """One dilated bottleneck block's tensors and its fp64 composition: the identity block (Cin == C4, proj False) or
    the projection block with the fused tail."""

    def __init__(self, pkg, torch_dev, N, H, W, Cin, Cm, C4, d, proj, seed):
        self.torch, self.dev = torch_dev
        torch = self.torch
        self.pkg = pkg
        g = torch.Generator(device="cpu").manual_seed(seed)
        r = lambda *s: torch.rand(*s, generator=g) - 0.5
        self.x = r(N, H, W, Cin)
        self.w1 = r(Cin, Cm) / np.sqrt(Cin) * 4
        self.w2 = r(Cm, Cm, 3, 3) / np.sqrt(9 * Cm) * 4        # [K][C][3][3]
        self.w3 = r(Cm, C4) / np.sqrt(Cm) * 4
        self.wp = r(Cin, C4) / np.sqrt(Cin) * 2
        self.bn = [(r(c), r(c) + 1.0) for c in (Cm, Cm, C4, C4)]   # (bias, scale)
        t = lambda a: a.contiguous().to(self.dev)
        self.xt, self.w1t, self.w3t, self.wpt = t(self.x), t(self.w1), t(self.w3), t(self.wp)
        self.bnt = [(t(b), t(s)) for b, s in self.bn]
        self.taps = pkg.filter_pack_s2(t(self.w2))
        self.tail = pkg.proj_tail_pack(self.w3t, self.bnt[2], self.wpt, self.bnt[3]) if proj else None
        self.N, self.H, self.W, self.Cin, self.Cm, self.C4, self.d, self.proj = N, H, W, Cin, Cm, C4, d, proj
        self._ref = None

    def workspace_bytes(self):
        L = self.pkg.lib()
        q = L.wino_proj_block_workspace_bytes_hw if self.proj else L.wino_residual_block_workspace_bytes_hw
        return q(self.N, self.H, self.W, self.Cm)

    def run(self, out=None, workspace=None):
        torch = self.torch
        if out is None:
            out = torch.full((self.N, self.H, self.W, self.C4), float("nan"), device=self.dev)
        if workspace is None:
            workspace = torch.full((self.workspace_bytes() // 4,), float("nan"), device=self.dev)
        if self.proj:
            return self.pkg.dilated_proj_block(self.xt, self.w1t, self.bnt[0], self.taps, self.bnt[1], self.tail, self.d,
                                               out=out, workspace=workspace)
        return self.pkg.dilated_residual_block(self.xt, self.w1t, self.bnt[0], self.taps, self.bnt[1], self.w3t,
                                               self.bnt[2], self.d, out=out, workspace=workspace)

    def reference(self):
        """fp64 composition: 1x1 + BN + ReLU, the dilated 3x3 (dilated_reference) + BN + ReLU, 1x1 + BN, the shortcut
        (x, or BN(x . wp)), ReLU."""
        if self._ref is None:
            f = lambda a: a.numpy().astype(np.float64)
            x = f(self.x)
            N, H, W, Cin = x.shape
            bn = [(f(b), f(s)) for b, s in self.bn]
            t1 = np.maximum(x.reshape(-1, Cin) @ f(self.w1) * bn[0][1] + bn[0][0], 0)
            t1p = np.zeros((N, H + 2, W + 2, self.Cm))
            t1p[:, 1:-1, 1:-1, :] = t1.reshape(N, H, W, self.Cm)
            t2 = dilated_reference(t1p, f(self.w2), bn[1][1], bn[1][0], self.d, True).reshape(-1, self.Cm)
            t3 = t2 @ f(self.w3) * bn[2][1] + bn[2][0]
            sc = (x.reshape(-1, Cin) @ f(self.wp) * bn[3][1] + bn[3][0]) if self.proj else x.reshape(-1, Cin)
            self._ref = np.maximum(t3 + sc, 0).reshape(N, H, W, self.C4)
            self._ref.setflags(write=False)
        return self._ref

    def check(self, O, got):
        g = got.cpu().numpy()
        assert np.isfinite(g).all()
        want = self.reference()
        assert g.shape == want.shape
        err = O.rel_error(g, want)
        print(f"dilated {'proj' if self.proj else 'residual'} block d={self.d}: rel err {err:.2e}")
        assert err < TIGHT
        assert (want > 0).mean() > 0.2   # both sides of the final ReLU
        assert self.pkg.tickets_in_use() == 0
