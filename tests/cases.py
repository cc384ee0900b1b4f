"""The case classes and tables that more than one test module uses: one layer's or block's tensors (CPU masters,
device copies), the library's run of it and its fp64 reference; the forced-form tables of the 1x1-kernel families; the
small helpers around them.  tests/shape_sweeps.py, the layers' own GPU tests and tests/test_gpu_large_tensors.py (which
borrows the reference methods for the few images it checks) all read them from here.  Nothing here needs a GPU to
import."""
import numpy as np

import layer_refs as LR
from layer_refs import interior, ring_mask  # noqa: F401  (ring_mask: read from here by the layers' tests)
from layer_refs import ring_is as ring_zero  # noqa: F401  (the ring of a padded tensor is exactly zero)

REL = 1e-3       # BASELINE.json's north_star bar: max|got - want| / max|want|
TIGHT = 2e-5     # what fp32 F(2x2,3x3) is held to, so that an indexing slip cannot hide under REL


def to_dev(torch_dev, a):
    torch, dev = torch_dev
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def rand_layer(rng, N, C, K):
    x = (rng.rand(N, 16, 16, C) - 0.5).astype(np.float32)
    w = (rng.rand(K, C, 3, 3) - 0.5).astype(np.float32)
    s = (rng.rand(K) - 0.5).astype(np.float32)
    b = (rng.rand(K) - 0.5).astype(np.float32)
    return x, w, s, b

def padded(torch, N, H, W, C, g, ring=0.0):
    """[N][H+2][W+2][C], interior uniform in [-0.5, 0.5), the ring set to `ring`."""
    return LR.ring(torch.rand(N, H, W, C, generator=g) - 0.5, ring)

# ---- the residual 3x3 layer and the identity basic block ------------------------------------------------------------
class ResLayer:
    """One residual layer's tensors (CPU masters and device copies) and the library's run of it."""

    def __init__(self, pkg, torch_dev, N, H, W, C, K, seed):
        self.torch, self.dev = torch_dev
        torch = self.torch
        self.pkg = pkg
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.x = padded(torch, N, H, W, C, g)
        # the residual's ring is never read: NaN there would reach any output that read it
        self.res = padded(torch, N, H, W, K, g, ring=float("nan"))
        self.w = (torch.rand(K, C, 3, 3, generator=g) - 0.5) / np.sqrt(9 * C) * 4
        self.bias = torch.rand(K, generator=g) - 0.5
        self.scale = torch.rand(K, generator=g) + 0.5
        t = lambda a: a.contiguous().to(self.dev)
        self.xt, self.rt, self.bt, self.st = t(self.x), t(self.res), t(self.bias), t(self.scale)
        self.U = pkg.filter_transform_f2(t(self.w))
        self.N, self.H, self.W, self.C, self.K = N, H, W, C, K

    def run(self, relu=True, res=None, out=None):
        torch = self.torch
        if out is None:
            out = torch.full((self.N, self.H + 2, self.W + 2, self.K), float("nan"), device=self.dev)
        return self.pkg.conv3x3_bn_add_relu(self.xt, self.U, self.bt, self.st, self.rt if res is None else res,
                                            relu=relu, out=out)

    def reference(self, relu=True, idx=None):
        pick = (lambda a: a) if idx is None else (lambda a: a[idx])
        return LR.conv3x3(interior(pick(self.x)), self.w, (self.bias, self.scale), relu,
                          residual=interior(pick(self.res))).numpy()

    def check(self, O, got, relu=True, idx=None):
        g = got.cpu().numpy()
        if idx is not None:
            g = g[idx]
        assert (g[:, ring_mask(self.H, self.W), :] == 0).all(), "out's ring is not zero"
        inner = g[:, 1:-1, 1:-1, :]
        assert np.isfinite(inner).all()
        want = self.reference(relu, idx)
        assert inner.shape == want.shape
        assert O.rel_error(inner, want) < TIGHT
        if relu:
            assert 0.2 < (want > 0).mean() < 0.8   # both sides of the ReLU
        else:
            assert (want < 0).mean() > 0.2
        assert self.pkg.tickets_in_use() == 0

class BasicBlock:
    def __init__(self, pkg, torch_dev, N, H, W, C, seed):
        self.torch, self.dev = torch_dev
        torch = self.torch
        self.pkg = pkg
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.x = padded(torch, N, H, W, C, g)
        self.w = [(torch.rand(C, C, 3, 3, generator=g) - 0.5) / np.sqrt(9 * C) * 4 for _ in range(2)]
        self.bn = [(torch.rand(C, generator=g) - 0.5, torch.rand(C, generator=g) + 0.5) for _ in range(2)]
        t = lambda a: a.contiguous().to(self.dev)
        self.xt = t(self.x)
        self.U = [pkg.filter_transform_f2(t(w)) for w in self.w]
        self.bnt = [(t(b), t(s)) for b, s in self.bn]
        self.N, self.H, self.W, self.C = N, H, W, C

    def run(self, x=None, out=None, workspace=None):
        torch = self.torch
        if out is None:
            out = torch.full((self.N, self.H + 2, self.W + 2, self.C), float("nan"), device=self.dev)
        if workspace is None:
            need = self.pkg.lib().wino_basic_block_workspace_bytes_hw(self.N, self.H, self.W, self.C)
            workspace = torch.full((need // 4,), float("nan"), device=self.dev)
        return self.pkg.basic_block(self.xt if x is None else x, self.U[0], self.bnt[0], self.U[1], self.bnt[1],
                                    out=out, workspace=workspace)

    def reference(self, xpadded, blocks=1):
        """fp64 on the CPU, `blocks` times in a row."""
        return LR.basic_block(interior(xpadded), self.w[0], self.bn[0], self.w[1], self.bn[1], blocks).numpy()

    def check(self, O, got, blocks=1):
        g = got.cpu().numpy()
        assert (g[:, ring_mask(self.H, self.W), :] == 0).all(), "out's ring is not zero"
        want = self.reference(self.x, blocks)
        assert np.isfinite(g).all()
        assert O.rel_error(g[:, 1:-1, 1:-1, :], want) < TIGHT
        assert (want > 0).mean() > 0.2
        assert self.pkg.tickets_in_use() == 0

# ---- the stride-2 3x3 layer, its forced forms, the downsampling basic block ------------------------------------------
class S2Layer:
    """One layer's tensors: the padded input with a zero ring, [K][C][3][3] weights, folded BN vectors."""

    def __init__(self, pkg, torch_dev, N, Hin, Win, C, K, seed):
        self.torch, self.dev = torch_dev
        self.pkg = pkg
        torch = self.torch
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.x = x = padded(torch, N, Hin, Win, C, g)
        self.w = (torch.rand(K, C, 3, 3, generator=g) - 0.5) / np.sqrt(9 * C) * 4
        self.bias = torch.rand(K, generator=g) - 0.5
        self.scale = torch.rand(K, generator=g) + 0.5
        self.xt, self.wt = x.to(self.dev), self.w.to(self.dev)
        self.bt, self.st = self.bias.to(self.dev), self.scale.to(self.dev)
        self.taps = pkg.filter_pack_s2(self.wt)
        self.N, self.Hin, self.Win, self.C, self.K = N, Hin, Win, C, K
        self.H, self.W = (Hin - 1) // 2 + 1, (Win - 1) // 2 + 1

    def run(self, relu=True):
        out = self.torch.full((self.N, self.H + 2, self.W + 2, self.K), float("nan"), device=self.dev)
        return self.pkg.conv3x3_s2_bn_relu(self.xt, self.taps, self.bt, self.st, relu=relu, out=out)

    def reference(self, idx=None, relu=True):
        """fp64 on the CPU: interior of the padded input -> 3x3 (stride 2, padding 1) -> BN -> ReLU, [n][H][W][K]."""
        x = self.x if idx is None else self.x[idx]
        return LR.conv3x3(interior(x), self.w, (self.bias, self.scale), relu, stride=2).numpy()

    def check(self, O, got, idx=None, relu=True):
        g = got.cpu().numpy()
        if idx is not None:
            g = g[idx]
        assert np.isfinite(g).all()
        assert (g[:, ring_mask(self.H, self.W), :] == 0).all(), "output ring is not zero"
        want = self.reference(idx, relu)
        assert O.rel_error(g[:, 1:-1, 1:-1, :], want) < TIGHT
        if relu:
            assert (want > 0).mean() > 0.2   # both sides of the ReLU

# (knob settings) -> a forced form
S2_FORMS = {f"latency_ks{ks}_rt{rt}_ct{ct}": {"WINO_1X1_ALGO": "small", "WINO_1X1_SMALL_KS": ks, "WINO_1X1_SMALL_RT": rt,
                                          "WINO_1X1_SMALL_CT": ct}
         for ks in (1, 2, 4) for rt in (1, 2) for ct in (1, 2, 4)}
S2_FORMS.update({
    "tiled": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 0},
    "stream_k": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1},
    # ranges that start and end inside taps (C / 32 k-steps per tap)
    "split_24": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1, "WINO_1X1_SK_GRID": 24},
    "split_40": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1, "WINO_1X1_SK_GRID": 40},
    "split_104": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1, "WINO_1X1_SK_GRID": 104},
})
# (N, Hin, Win, C, K): 8-wave tiles (K = 256) with 2 k-steps per tap, 4-wave tiles (K = 128) with 3 per tap
S2_FORM_SHAPES = [(2, 28, 28, 64, 256), (3, 15, 13, 96, 128)]


def s2_legal(form, shape):
    """The latency forms the planner accepts for this shape (conv1x1.hip small1_legal): K = 9C in 16-channel chunks per
    wave, the workgroup's columns a divisor of K."""
    kn = S2_FORMS[form]
    if kn["WINO_1X1_ALGO"] != "small":
        return True
    C, K, ks, ct = shape[3], shape[4], kn["WINO_1X1_SMALL_KS"], kn["WINO_1X1_SMALL_CT"]
    return (9 * C) % (16 * ks) == 0 and K % ((4 // ks) * ct * 16) == 0

class S2Block:
    """One downsampling block's parameters (CPU masters, device copies, the packed buffer) and its fp64 reference."""

    def __init__(self, pkg, torch_dev, N, Hin, Win, C, K, seed):
        self.torch, self.dev = torch_dev
        torch = self.torch
        self.pkg = pkg
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.x = x = padded(torch, N, Hin, Win, C, g)
        self.w1 = (torch.rand(K, C, 3, 3, generator=g) - 0.5) / np.sqrt(9 * C) * 4
        self.wd = (torch.rand(K, C, 1, 1, generator=g) - 0.5) / np.sqrt(C) * 4
        self.w2 = (torch.rand(K, K, 3, 3, generator=g) - 0.5) / np.sqrt(9 * K) * 4
        vec = lambda lo: torch.rand(K, generator=g) + lo
        self.b1, self.s1 = vec(-0.5), vec(0.5)
        self.bd, self.sd = vec(-0.5), vec(0.5)
        self.b2, self.s2 = vec(-0.5), vec(0.5)
        t = lambda a: a.contiguous().to(self.dev)
        self.xt = t(x)
        self.taps = pkg.filter_pack_s2(t(self.w1))
        self.packed = pkg.s2_proj_pack(self.taps, (t(self.b1), t(self.s1)), t(self.wd.view(K, C).t()),
                                       (t(self.bd), t(self.sd)))
        self.U2 = pkg.filter_transform_f2(t(self.w2))
        self.bn1 = (t(self.b1), t(self.s1))
        self.bn2 = (t(self.b2), t(self.s2))
        self.N, self.Hin, self.Win, self.C, self.K = N, Hin, Win, C, K
        self.H, self.W = (Hin - 1) // 2 + 1, (Win - 1) // 2 + 1

    def nan(self):
        return self.torch.full((self.N, self.H + 2, self.W + 2, self.K), float("nan"), device=self.dev)

    def layer(self):
        return self.pkg.conv3x3_s2_proj(self.xt, self.packed, t1=self.nan(), sc=self.nan())

    def plain(self):
        return self.pkg.conv3x3_s2_bn_relu(self.xt, self.taps, *self.bn1, relu=True, out=self.nan())

    def block(self, out=None, workspace=None):
        return self.pkg.basic_block_s2(self.xt, self.packed, self.U2, self.bn2,
                                       out=self.nan() if out is None else out, workspace=workspace)

    def reference(self, idx=None, block=True):
        """fp64 on the CPU: (t1, sc, out), each [n][H][W][K] (out None unless `block`)."""
        tail = (self.w2, (self.b2, self.s2)) if block else ()
        out = LR.basic_block_s2(interior(self.x if idx is None else self.x[idx]), self.w1, (self.b1, self.s1), self.wd,
                                (self.bd, self.sd), *tail)
        return tuple(None if t is None else t.numpy() for t in out)

    def check_layer(self, O, t1, sc, idx=None):
        a, b = t1.cpu().numpy(), sc.cpu().numpy()
        if idx is not None:
            a, b = a[idx], b[idx]
        ring = ring_mask(self.H, self.W)
        assert np.isfinite(a).all()
        assert (a[:, ring, :] == 0).all(), "t1's ring is not zero"
        assert np.isfinite(b[:, 1:-1, 1:-1, :]).all(), "sc's interior is not all written"
        assert np.isnan(b[:, ring, :]).all(), "sc's ring was written"
        want_t1, want_sc, _ = self.reference(idx, block=False)
        assert O.rel_error(a[:, 1:-1, 1:-1, :], want_t1) < TIGHT
        assert O.rel_error(b[:, 1:-1, 1:-1, :], want_sc) < TIGHT
        assert (want_t1 > 0).mean() > 0.2 and (want_sc < 0).mean() > 0.2   # both sides of t1's ReLU; sc has none

    def check_block(self, O, out, idx=None):
        g = out.cpu().numpy()
        if idx is not None:
            g = g[idx]
        assert np.isfinite(g).all()
        assert (g[:, ring_mask(self.H, self.W), :] == 0).all(), "out's ring is not zero"
        want = self.reference(idx)[2]
        assert O.rel_error(g[:, 1:-1, 1:-1, :], want) < TIGHT
        assert (want > 0).mean() > 0.2

# ---- the projection bottleneck blocks -------------------------------------------------------------------------------
def proj_weights(rng, Cin, Cm, C4):
    w1 = ((rng.rand(Cin, Cm) - 0.5) / np.sqrt(Cin) * 4).astype(np.float32)
    w2 = ((rng.rand(Cm, Cm, 3, 3) - 0.5) / np.sqrt(9 * Cm) * 4).astype(np.float32)
    w3 = ((rng.rand(Cm, C4) - 0.5) / np.sqrt(Cm) * 4).astype(np.float32)
    wp = ((rng.rand(Cin, C4) - 0.5) / np.sqrt(Cin) * 2).astype(np.float32)
    bn = [((rng.rand(c) - 0.5).astype(np.float32), (rng.rand(c) + 0.5).astype(np.float32)) for c in (Cm, Cm, C4, C4)]
    return w1, w2, w3, wp, bn

# (knob settings) -> the forms both 1x1 launches are forced into
PROJ_FORMS = {
    "latency": {"WINO_1X1_ALGO": "small"},
    "latency_ks2": {"WINO_1X1_ALGO": "small", "WINO_1X1_SMALL_KS": 2},
    "latency_ks4": {"WINO_1X1_ALGO": "small", "WINO_1X1_SMALL_KS": 4},
    "tiled": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 0},
    "stream_k": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1},
    # ranges that do not line up with the tail's phase boundary (Cm/32 = 4 k-steps of t2, then 8 of x)
    "split_24": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1, "WINO_1X1_SK_GRID": 24},
    "split_40": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1, "WINO_1X1_SK_GRID": 40},
    "split_104": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1, "WINO_1X1_SK_GRID": 104},
}

class V15Block:
    """One block's tensors (folded BN vectors, NHWC activations) and the library's run of it."""

    def __init__(self, pkg, torch_dev, N, Hin, Win, Cin, Cm, C4, seed):
        self.torch, self.dev = torch_dev
        torch = self.torch
        self.pkg = pkg
        g = torch.Generator(device="cpu").manual_seed(seed)
        r = lambda *s: torch.rand(*s, generator=g) - 0.5
        self.x = r(N, Hin, Win, Cin)
        self.w1 = r(Cin, Cm) / np.sqrt(Cin) * 4
        self.w2 = r(Cm, Cm, 3, 3) / np.sqrt(9 * Cm) * 4        # [K][C][3][3]
        self.w3 = r(Cm, C4) / np.sqrt(Cm) * 4
        self.wp = r(Cin, C4) / np.sqrt(Cin) * 2
        self.bn = [(r(c), r(c) + 1.0) for c in (Cm, Cm, C4, C4)]   # (bias, scale)
        t = lambda a: a.contiguous().to(self.dev)
        self.xt, self.w1t, self.w3t, self.wpt = t(self.x), t(self.w1), t(self.w3), t(self.wp)
        self.bnt = [(t(b), t(s)) for b, s in self.bn]
        self.taps = pkg.filter_pack_s2(t(self.w2))
        self.tail = pkg.proj_tail_pack(self.w3t, self.bnt[2], self.wpt, self.bnt[3])
        self.H, self.W = (Hin - 1) // 2 + 1, (Win - 1) // 2 + 1
        self.N, self.Hin, self.Win, self.Cin, self.Cm, self.C4 = N, Hin, Win, Cin, Cm, C4

    def run(self, out=None, workspace=None):
        """The fused block, into NaN-filled output and workspace unless given."""
        torch = self.torch
        if out is None:
            out = torch.full((self.N, self.H, self.W, self.C4), float("nan"), device=self.dev)
        if workspace is None:
            need = self.pkg.lib().wino_proj_block_v15_workspace_bytes_hw(self.N, self.Hin, self.Win, self.Cm)
            workspace = torch.full((need // 4,), float("nan"), device=self.dev)
        return self.pkg.proj_block_v15(self.xt, self.w1t, self.bnt[0], self.taps, self.bnt[1], self.tail,
                                       out=out, workspace=workspace)

    def reference(self, idx=None):
        """fp64 on the CPU: 1x1 at stride 1, 3x3 at stride 2 with pad 1, 1x1, plus the stride-2 projection, ReLU."""
        x, bn = self.x if idx is None else self.x[idx], self.bn
        return LR.bottleneck(x, self.w1, bn[0], self.w2, bn[1], self.w3, bn[2], self.wp, bn[3], stride=2,
                             stride_on="3x3").numpy()

    def check(self, O, got, idx=None):
        g = got.cpu().numpy()
        if idx is not None:
            g = g[idx]
        assert np.isfinite(g).all()
        want = self.reference(idx)
        assert g.shape == want.shape
        assert O.rel_error(g, want) < TIGHT
        assert (want > 0).mean() > 0.2   # both sides of the final ReLU
        assert self.pkg.tickets_in_use() == 0
