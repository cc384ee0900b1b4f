"""One guarded run per sweep case: the per-entry-point case runners that tests/test_gpu_shape_sweeps.py drives over
the generators of tests/shape_sweeps.py and tests/test_gpu_guard_bands.py calls with hand-made cases.  Sweep holds a
case's fp32 tensors (CPU masters; device copies on a guarded arena of tests/guarded.py), the fp64 reference pieces and
the checks; each runner launches twice per placement, compares with the fp64 reference at TIGHT and ends each placement
in arena.check, which CHECKS counts by entry point."""
import collections
import types

import numpy as np

import aspp_cases as AC
import guarded as G
import layer_refs as LR
import resize_cases as RC
import shape_sweeps as S
from cases import TIGHT
from dilated_cases import dilated_reference
from forms_1x1 import knobs_set
from fpn_reference import level_reference
from layer_refs import bn_pair, conv_w, interior, ring, w11

SENTINEL = 1234.5
CHECKS = collections.Counter()   # arena.check calls that passed, by entry point
WORST = {}                       # the largest relative error close() saw, by entry point
# the first seed of the segmentation entries' sweeps (case i takes seed + i): tests/test_shape_sweeps_host.py rebuilds
# the same tensors for the conditions it proves on the references
SEEDS = {"conv3x3_dilated_bn_relu": 1000, "dilated_block": 1100, "conv1x1_cat_bn": 1200, "aspp": 1300,
         "resize_bilinear": 1400, "conv3x3_grouped_bn_relu": 1500, "grouped_block": 1600, "fpn_level": 1700}


class Sweep:
    """fp32 tensors drawn for one case (CPU masters; `dev` copies), fp64 reference helpers, and the checks."""

    def __init__(self, torch, dev, case, pkg, seed):
        self.torch, self.dev, self.case, self.pkg = torch, dev, case, pkg
        self.g = torch.Generator().manual_seed(seed)
        self.tag = self.base_tag = case.tag()
        self.arena = None

    def passes(self):
        """One pass per placement of the tensors, each on an arena of its own and ended by done()."""
        for align in G.ALIGNS:
            self.arena = G.Arena(self.torch, self.dev, align=align)
            self.tag = f"{self.base_tag[:-1]} align={align}]"
            yield align
            self.done()
        self.arena = None

    def rand(self, *shape):
        return self.torch.rand(*shape, generator=self.g)

    def act(self, *shape):
        """Activations: uniform in [-0.5, 0.5), or in [0, 1) (non-zero mean, as after a ReLU) for nonneg cases."""
        r = self.rand(*shape)
        return r if self.case.flags.get("nonneg") else r - 0.5

    def nan(self, *shape, name=None):
        """A NaN-filled output between sentinel guards."""
        return self.arena.output(*shape, name=name)

    def ws(self, nbytes, query):
        """A NaN-filled workspace of exactly `nbytes` (whole floats), what size query `query` reported, between sentinel
        guards."""
        return self.arena.workspace(nbytes, name="workspace", query=query)

    def d(self, t, name=None):
        """A read-only operand between NaN guards (a tensor the library packed is re-homed there for its consumer)."""
        return self.arena.input(t, name=name)

    def packed(self, pack, shape, name, *args):
        """What a pack entry point makes of `args`: written into a guarded output of exactly `shape` (the size query's
        count), then re-homed as a read-only operand for its consumer."""
        shape = (int(shape),) if isinstance(shape, int) else tuple(shape)
        out = self.nan(*shape, name=name + " (pack out)")
        got = pack(*args, out=out)
        assert got.data_ptr() == out.data_ptr(), self.tag
        return self.d(got, name)

    def U(self, w, name="U"):
        K, C = w.shape[:2]
        return self.packed(self.pkg.filter_transform_f2, self.pkg.lib().wino_filter_f2_elems(C, K), name,
                           self.d(w, name + ".w"))

    def bnd(self, bn, name="bn"):
        return self.d(bn[0], name + ".bias"), self.d(bn[1], name + ".scale")

    def buf(self, t, name="buf"):
        """A fresh guarded copy of `t` that the launch writes in place."""
        return self.arena.input(t, name=name, in_place=True)

    # checks
    def close(self, got, want, what="out"):
        assert tuple(got.shape) == tuple(want.shape), f"{self.tag} {what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
        assert bool(self.torch.isfinite(got).all()), f"{self.tag} {what}: non-finite values (not all written)"
        err = LR.rel(got, want)
        WORST[self.case.entry] = max(WORST.get(self.case.entry, 0.0), err)
        assert err < TIGHT, f"{self.tag} {what}: rel err {err:.3e}"

    def ring_is(self, got, value, what="out"):
        assert LR.ring_is(got.detach().cpu(), value), f"{self.tag} {what}: ring is not exactly {value}"

    def both_sides(self, pre):
        pos, neg = int((pre > 0).sum()), int((pre < 0).sum())
        assert pos > 0 and neg > 0, f"{self.tag}: the ReLU sees one side only ({pos} > 0, {neg} < 0)"

    def same(self, a, b, what="out"):
        assert self.torch.equal(a, b), f"{self.tag} {what}: two launches differ"

    def agree(self, outs, want, what="out", padded=False):
        """Two launches' outputs: the first against the reference (of a padded one the ring is exactly 0 and the interior
        is compared), the second bitwise the first."""
        if padded:
            self.ring_is(outs[0], 0.0, what)
        self.close(interior(outs[0]) if padded else outs[0], want, what)
        self.same(outs[0], outs[1], what)

    def done(self):
        assert self.pkg.tickets_in_use() == 0, f"{self.tag}: a stream-K ticket is still held"
        self.arena.check(self.tag)
        CHECKS[self.case.entry] += 1



def start(pkg, knobs, torch_dev, case, seed):
    """The sweep's tensors, with the plan query asked (under the case's knobs) that the forced form is taken."""
    torch, dev = torch_dev
    sw = Sweep(torch, dev, case, pkg, seed)
    plan = S.plan_form(pkg, case)
    bad = S.check_forced(case, plan)
    assert bad is None, f"{sw.tag}: {bad}"
    sw.tag = sw.base_tag = f"{sw.tag[:-1]} plan={plan['form']}]"
    return sw


def run_sweep(entry, run, pkg, knobs, torch_dev, seed0):
    """Every case of the entry point's generator, and the count that none was left out at either placement."""
    cases = S.GENERATORS[entry]()
    before = CHECKS[entry]
    WORST.pop(entry, None)
    for i, case in enumerate(cases):
        assert case.entry == entry
        with knobs_set(knobs, case.knobs):
            run(pkg, knobs, torch_dev, case, seed0 + i)
    done = CHECKS[entry] - before
    if entry in WORST:
        print(f"{entry}: {len(cases)} cases, worst rel err {WORST[entry]:.2e}")
    assert done == 2 * len(cases), f"{entry}: {done} guard checks for {len(cases)} cases at two placements"


# ---- one FPN level -------------------------------------------------------------------------------------------------------
def fpn_level_case(pkg, knobs, torch_dev, case, seed):
    """inner = conv1x1(c) + bias [+ nearest-upsampled top], P = conv3x3(inner) + bias: c and top carry NaN rings (not
    read), inner and P rings of exact 0, both held against fpn_reference.level_reference."""
    sw = start(pkg, knobs, torch_dev, case, seed)
    torch, nan = sw.torch, float("nan")
    N, H, W, Cin, Cf = case.N, case.H, case.W, case.Cin, case.Cf
    c = sw.act(N, H, W, Cin)
    wl, wo = conv_w(sw.rand, Cf, Cin, k=1), conv_w(sw.rand, Cf, Cf)
    bl, bo = sw.rand(Cf) - 0.5, sw.rand(Cf) - 0.5
    top = sw.act(N, (H + 1) // 2, (W + 1) // 2, Cf) if case.flags["top"] else None
    want_inner, want_P = level_reference(torch, c, wl, bl, wo, bo, top)
    for _ in sw.passes():
        cd = sw.d(ring(c, nan) if case.flags["c_padded"] else c, "c")
        wld, U = sw.d(wl.reshape(Cf, Cin).t().contiguous(), "w_lat"), sw.U(wo)
        bld, bod, ones = sw.d(bl, "b_lat"), sw.d(bo, "b_out"), sw.d(torch.ones(Cf), "ones")
        topd = sw.d(ring(top, nan), "top") if top is not None else None
        outs = []
        for _ in range(2):
            outs.append(pkg.fpn_level(cd, wld, bld, U, bod, top=topd, c_padded=case.flags["c_padded"], ones=ones,
                                      inner=sw.nan(N, H + 2, W + 2, Cf, name="inner"), out=sw.nan(N, H + 2, W + 2, Cf, name="P")))
        for k, (name, want) in enumerate((("inner", want_inner), ("P", want_P))):
            sw.agree((outs[0][k], outs[1][k]), want, name, padded=True)


# ---- the residual 3x3 ------------------------------------------------------------------------------------------------
def residual_case(pkg, knobs, torch_dev, case, seed):
    sw = start(pkg, knobs, torch_dev, case, seed)
    N, H, W, C, K = case.N, case.H, case.W, case.C, case.K
    relu, in_place = case.flags["relu"], case.flags["in_place"]
    x = ring(sw.act(N, H, W, C))
    res = ring(sw.act(N, H, W, K), float("nan"))   # the residual's ring is not read
    w, bn = conv_w(sw.rand, K, C), bn_pair(sw.rand, K)
    pre = LR.conv3x3(interior(x), w, bn, False, residual=interior(res))
    want = sw.torch.relu(pre) if relu else pre
    if relu:
        sw.both_sides(pre)
    for _ in sw.passes():
        xd, U = sw.d(x, "x"), sw.U(w)
        bd, sd = sw.bnd(bn)
        resd = None if in_place else sw.d(res, "residual")
        outs = []
        for _ in range(2):
            if in_place:
                buf = sw.buf(res)   # a fresh copy before each launch
                got = pkg.conv3x3_bn_add_relu(xd, U, bd, sd, buf, relu=relu, out=buf)
                assert got.data_ptr() == buf.data_ptr(), sw.tag
            else:
                got = pkg.conv3x3_bn_add_relu(xd, U, bd, sd, resd, relu=relu, out=sw.nan(N, H + 2, W + 2, K))
            outs.append(got)
        sw.agree(outs, want, padded=True)


# ---- the identity basic block ----------------------------------------------------------------------------------------
def basic_block_case(pkg, knobs, torch_dev, case, seed):
    sw = start(pkg, knobs, torch_dev, case, seed)
    N, H, W, C = case.N, case.H, case.W, case.C
    x = ring(sw.act(N, H, W, C))
    w1, w2, bn1, bn2 = conv_w(sw.rand, C, C), conv_w(sw.rand, C, C), bn_pair(sw.rand, C), bn_pair(sw.rand, C)
    pre = LR.basic_block(interior(x), w1, bn1, w2, bn2, pre=True)
    sw.both_sides(pre)
    want = sw.torch.relu(pre)
    need = pkg.lib().wino_basic_block_workspace_bytes_hw(N, H, W, C)
    for _ in sw.passes():
        U1, U2 = sw.U(w1, "U1"), sw.U(w2, "U2")
        bnd1, bnd2 = sw.bnd(bn1, "bn1"), sw.bnd(bn2, "bn2")
        xd = None if case.flags["in_place"] else sw.d(x, "x")
        outs = []
        for _ in range(2):
            ws = sw.ws(need, "wino_basic_block_workspace_bytes_hw")
            if case.flags["in_place"]:
                buf = sw.buf(x)
                got = pkg.basic_block(buf, U1, bnd1, U2, bnd2, out=buf, workspace=ws)
                assert got.data_ptr() == buf.data_ptr(), sw.tag
            else:
                got = pkg.basic_block(xd, U1, bnd1, U2, bnd2, out=sw.nan(N, H + 2, W + 2, C), workspace=ws)
            outs.append(got)
        sw.agree(outs, want, padded=True)


# ---- the stride-2 3x3, the fused stride-2 3x3 + shortcut, the downsampling basic block ---------------------------
class S2Case:
    """A stride-2 case's tensors: padded x, the 3x3 and 1x1 shortcut weights, their BNs, and the fp64 pre1 (t1 before
    its ReLU) and sc, NHWC."""

    def __init__(self, sw, case, with_block=False):
        N, Hin, Win, C, K = case.N, case.Hin, case.Win, case.C, case.K
        self.H, self.W = S._s2(Hin), S._s2(Win)
        self.x = ring(sw.act(N, Hin, Win, C))
        self.w1, self.wd = conv_w(sw.rand, K, C), conv_w(sw.rand, K, C, k=1)
        self.bn1, self.bnd = bn_pair(sw.rand, K), bn_pair(sw.rand, K)
        self.pre1 = LR.conv3x3(interior(self.x), self.w1, self.bn1, False, stride=2)
        self.sc = LR.conv1x1(interior(self.x), self.wd[:, :, 0, 0].t(), self.bnd, False, stride=2)
        self.shape = (N, self.H + 2, self.W + 2, K)
        if with_block:
            self.w2, self.bn2 = conv_w(sw.rand, K, K), bn_pair(sw.rand, K)

    def place(self, sw):
        """The device operands of one pass, on sw's arena."""
        K, C = self.w1.shape[:2]
        self.xd = sw.d(self.x, "x")
        self.taps = sw.packed(sw.pkg.filter_pack_s2, (3, 3, C, K), "taps", sw.d(self.w1, "w1"))
        self.bn1d, self.bndd = sw.bnd(self.bn1, "bn1"), sw.bnd(self.bnd, "bnd")

    def packed(self, sw):
        K, C = self.w1.shape[:2]
        return sw.packed(sw.pkg.s2_proj_pack, sw.pkg.lib().wino_s2_proj_elems(C, K), "packed",
                         self.taps, self.bn1d, sw.d(self.wd.view(K, C).t(), "wd"), self.bndd)


def s2_case(pkg, knobs, torch_dev, case, seed):
    sw = start(pkg, knobs, torch_dev, case, seed)
    L = S2Case(sw, case)
    relu = case.flags["relu"]
    if relu:
        sw.both_sides(L.pre1)
    want = sw.torch.relu(L.pre1) if relu else L.pre1
    for _ in sw.passes():
        L.place(sw)
        outs = [pkg.conv3x3_s2_bn_relu(L.xd, L.taps, *L.bn1d, relu=relu, out=sw.nan(*L.shape)) for _ in range(2)]
        sw.agree(outs, want, padded=True)


def s2_proj_case(pkg, knobs, torch_dev, case, seed):
    sw = start(pkg, knobs, torch_dev, case, seed)
    L = S2Case(sw, case)
    sw.both_sides(L.pre1)
    for _ in sw.passes():
        L.place(sw)
        packed = L.packed(sw)
        runs = []
        for _ in range(2):
            sc = sw.nan(*L.shape, name="sc")
            sc[:, 0, :, :] = sc[:, -1, :, :] = SENTINEL   # sc's ring is not touched
            sc[:, :, 0, :] = sc[:, :, -1, :] = SENTINEL
            runs.append(pkg.conv3x3_s2_proj(L.xd, packed, t1=sw.nan(*L.shape, name="t1"), sc=sc))
        (t1, sc), (t1b, scb) = runs
        sw.ring_is(t1, 0.0, "t1")
        sw.ring_is(sc, SENTINEL, "sc")
        sw.close(t1[:, 1:-1, 1:-1, :], sw.torch.relu(L.pre1), "t1")
        sw.close(sc[:, 1:-1, 1:-1, :], L.sc, "sc")
        plain = pkg.conv3x3_s2_bn_relu(L.xd, L.taps, *L.bn1d, relu=True, out=sw.nan(*L.shape))
        sw.same(t1, plain, "t1 against the plain stride-2 layer:")
        sw.same(t1, t1b, "t1")
        sw.same(sc, scb, "sc")


def basic_block_s2_case(pkg, knobs, torch_dev, case, seed):
    sw = start(pkg, knobs, torch_dev, case, seed)
    L = S2Case(sw, case, with_block=True)
    pre = LR.basic_block_s2(interior(L.x), L.w1, L.bn1, L.wd, L.bnd, L.w2, L.bn2, pre=True)[2]
    sw.both_sides(pre)
    want = sw.torch.relu(pre)
    need = pkg.lib().wino_basic_block_s2_workspace_bytes_hw(case.N, case.Hin, case.Win, case.K)
    for _ in sw.passes():
        L.place(sw)
        packed, U2 = L.packed(sw), sw.U(L.w2, "U2")
        bn2 = sw.bnd(L.bn2, "bn2")
        outs = [pkg.basic_block_s2(L.xd, packed, U2, bn2, out=sw.nan(*L.shape),
                                   workspace=sw.ws(need, "wino_basic_block_s2_workspace_bytes_hw"))
                for _ in range(2)]
        sw.agree(outs, want, padded=True)


# ---- the projection bottleneck blocks ------------------------------------------------------------------------------
class ProjCase:
    def __init__(self, sw, case):
        N, Hin, Win, Cin, Cm, C4 = case.N, case.Hin, case.Win, case.Cin, case.Cm, case.C4
        self.x = sw.act(N, Hin, Win, Cin)
        r = sw.rand
        self.w1, self.w2, self.w3, self.wp = w11(r, Cin, Cm), conv_w(r, Cm, Cm), w11(r, Cm, C4), w11(r, Cin, C4, 2)
        self.bn = [bn_pair(sw.rand, c) for c in (Cm, Cm, C4, C4)]

    def place(self, sw):
        """The device operands of one pass, on sw's arena."""
        self.xd, self.w1d = sw.d(self.x, "x"), sw.d(self.w1, "w1")
        self.bnd = [sw.bnd(b, f"bn{i}") for i, b in enumerate(self.bn)]
        Cin, Cm, C4 = self.w1.shape[0], self.w1.shape[1], self.w3.shape[1]
        self.tail = sw.packed(sw.pkg.proj_tail_pack, sw.pkg.lib().wino_proj_tail_elems(Cm, Cin, C4), "tail",
                              sw.d(self.w3, "w3"), self.bnd[2], sw.d(self.wp, "wp"), self.bnd[3])

    def reference(self, sw, stride, v15):
        """(pre-ReLU sum, output) in fp64, NHWC."""
        bn = self.bn
        pre = LR.bottleneck(self.x, self.w1, bn[0], self.w2, bn[1], self.w3, bn[2], self.wp, bn[3], stride=stride,
                            stride_on="3x3" if v15 else "first", pre=True)
        return pre, sw.torch.relu(pre)


def proj_case(pkg, knobs, torch_dev, case, seed):
    sw = start(pkg, knobs, torch_dev, case, seed)
    B, st = ProjCase(sw, case), case.stride
    pre, want = B.reference(sw, st, v15=False)
    sw.both_sides(pre)
    H, W = (case.Hin - 1) // st + 1, (case.Win - 1) // st + 1
    need = pkg.lib().wino_proj_block_workspace_bytes_hw(case.N, H, W, case.Cm)
    for _ in sw.passes():
        B.place(sw)
        U2 = sw.U(B.w2, "U2")
        outs = [pkg.proj_block(B.xd, B.w1d, B.bnd[0], U2, B.bnd[1], B.tail, st, out=sw.nan(case.N, H, W, case.C4),
                               workspace=sw.ws(need, "wino_proj_block_workspace_bytes_hw")) for _ in range(2)]
        sw.agree(outs, want)


def v15_case(pkg, knobs, torch_dev, case, seed):
    sw = start(pkg, knobs, torch_dev, case, seed)
    B = ProjCase(sw, case)
    pre, want = B.reference(sw, 2, v15=True)
    sw.both_sides(pre)
    H, W = S._s2(case.Hin), S._s2(case.Win)
    need = pkg.lib().wino_proj_block_v15_workspace_bytes_hw(case.N, case.Hin, case.Win, case.Cm)
    for _ in sw.passes():
        B.place(sw)
        taps = sw.packed(pkg.filter_pack_s2, (3, 3, case.Cm, case.Cm), "taps", sw.d(B.w2, "w2"))
        outs = [pkg.proj_block_v15(B.xd, B.w1d, B.bnd[0], taps, B.bnd[1], B.tail, out=sw.nan(case.N, H, W, case.C4),
                                   workspace=sw.ws(need, "wino_proj_block_v15_workspace_bytes_hw")) for _ in range(2)]
        sw.agree(outs, want)


# ---- the grouped 3x3 and the ResNeXt blocks ----------------------------------------------------------------------------
def grouped_case(pkg, knobs, torch_dev, case, seed):
    sw = start(pkg, knobs, torch_dev, case, seed)
    N, Hin, Win, C, groups, stride, relu = case.N, case.Hin, case.Win, case.C, case.groups, case.stride, case.flags["relu"]
    H, W = S.grouped_out(Hin, Win, stride)
    x = ring(sw.act(N, Hin, Win, C))          # the ring is read: zero, as the contract says
    w, bn = conv_w(sw.rand, C, C // groups), bn_pair(sw.rand, C)
    pre = LR.conv3x3(interior(x), w, bn, False, stride=stride, groups=groups)
    if relu:
        sw.both_sides(pre)
    want = sw.torch.relu(pre) if relu else pre
    elems = pkg.lib().wino_conv3x3_grouped_filter_elems(C, groups)
    for _ in sw.passes():
        xd = sw.d(x, "x")
        packed = sw.packed(pkg.filter_pack_grouped, elems, "packed", sw.d(w, "w"), groups)
        assert packed.numel() == elems, sw.tag
        bd, sd = sw.bnd(bn)
        outs = [pkg.conv3x3_grouped_bn_relu(xd, packed, bd, sd, groups, stride=stride, relu=relu,
                                            out=sw.nan(N, H + 2, W + 2, C)) for _ in range(2)]
        sw.agree(outs, want, padded=True)


def grouped_block_case(pkg, knobs, torch_dev, case, seed):
    sw = start(pkg, knobs, torch_dev, case, seed)
    N, Hin, Win, Cin, Cm, C4 = case.N, case.Hin, case.Win, case.Cin, case.Cm, case.C4
    groups, stride, proj = case.groups, case.stride, case.proj
    H, W = S.grouped_out(Hin, Win, stride)
    x = sw.act(N, Hin, Win, Cin)
    r = sw.rand
    w1, wg, w3, wp = w11(r, Cin, Cm), conv_w(r, Cm, Cm // groups), w11(r, Cm, C4), w11(r, Cin, C4, 2)
    bn = [bn_pair(r, c) for c in (Cm, Cm, C4, C4)]
    pre = LR.bottleneck(x, w1, bn[0], wg, bn[1], w3, bn[2], *((wp, bn[3]) if proj else ()), stride=stride,
                        stride_on="3x3", groups=groups, pre=True)
    sw.both_sides(pre)
    want = sw.torch.relu(pre)
    L = pkg.lib()
    query, need = S.grouped_block_workspace(pkg, case)
    for _ in sw.passes():
        xd, w1d = sw.d(x, "x"), sw.d(w1, "w1")
        bnd = [sw.bnd(b, f"bn{i}") for i, b in enumerate(bn[:3 + proj])]
        wgd = sw.packed(pkg.filter_pack_grouped, L.wino_conv3x3_grouped_filter_elems(Cm, groups), "wg", sw.d(wg, "wg.w"),
                        groups)
        if proj:
            tail = sw.packed(pkg.proj_tail_pack, L.wino_proj_tail_elems(Cm, Cin, C4), "tail", sw.d(w3, "w3"), bnd[2],
                             sw.d(wp, "wp"), bnd[3])
            run = lambda: pkg.grouped_proj_block(xd, w1d, bnd[0], wgd, bnd[1], tail, groups, stride,
                                                 out=sw.nan(N, H, W, C4), workspace=sw.ws(need, query))
        else:
            w3d = sw.d(w3, "w3")
            run = lambda: pkg.grouped_residual_block(xd, w1d, bnd[0], wgd, bnd[1], w3d, bnd[2], groups,
                                                     out=sw.nan(N, H, W, C4), workspace=sw.ws(need, query))
        outs = [run(), run()]
        sw.agree(outs, want)


# ---- the stem and the head -----------------------------------------------------------------------------------------
def stem_case(pkg, knobs, torch_dev, case, seed):
    sw = start(pkg, knobs, torch_dev, case, seed)
    N, H, W, K, padded = case.N, case.H, case.W, case.K, case.flags["padded"]
    x = sw.rand(N, 3, H, W) * 2 - 1
    w = (sw.rand(K, 3, 7, 7) - 0.5) * 0.3
    bn = bn_pair(sw.rand, K)
    pre = LR.stem(x, w, bn, pre=True)
    sw.both_sides(pre)
    want = LR.stem(x, w, bn)
    Hp, Wp = pkg.stem_out_hw(H, W)
    p = 2 if padded else 0
    for _ in sw.passes():
        packed = sw.packed(pkg.stem_filter_pack, pkg.lib().wino_stem_filter_elems(K), "packed", sw.d(w, "w"),
                           sw.bnd(bn))
        xd = sw.d(x, "x")
        outs = [pkg.stem(xd, packed, out_padded=padded, out=sw.nan(N, Hp + p, Wp + p, K)) for _ in range(2)]
        sw.agree(outs, want, padded=padded)


def head_case(pkg, knobs, torch_dev, case, seed):
    sw = start(pkg, knobs, torch_dev, case, seed)
    N, H, W, C, classes, padded = case.N, case.H, case.W, case.C, case.classes, case.flags["padded"]
    feat = sw.rand(N, H, W, C) * 2            # post-ReLU features
    wfc = (sw.rand(classes, C) - 0.5) / np.sqrt(C) * 2
    bfc = sw.rand(classes) - 0.5
    want = LR.avgpool_fc(feat, wfc, bfc)
    f = ring(feat, float("nan")) if padded else feat   # the padded input's ring is not read
    need = pkg.lib().wino_head_workspace_bytes(N, C, classes)
    for _ in sw.passes():
        packed = sw.packed(pkg.head_pack, pkg.lib().wino_head_elems(C, classes), "packed",
                           sw.d(wfc, "wfc"), sw.d(bfc, "bfc"))
        fd = sw.d(f, "feat")
        outs = [pkg.avgpool_fc(fd, packed, classes, in_padded=padded, out=sw.nan(N, classes),
                               workspace=sw.ws(need, "wino_head_workspace_bytes")) for _ in range(2)]
        sw.agree(outs, want, "logits")


# ---- the dilated 3x3 and the dilated bottleneck blocks ----------------------------------------------------------------
def dilated_case(pkg, knobs, torch_dev, case, seed):
    sw = start(pkg, knobs, torch_dev, case, seed)
    N, H, W, C, K, d, relu = case.N, case.H, case.W, case.C, case.K, case.d, case.flags["relu"]
    x = ring(sw.act(N, H, W, C))          # the ring is read: zero, as the contract says
    w, bn = conv_w(sw.rand, K, C), bn_pair(sw.rand, K)
    pre = sw.torch.from_numpy(dilated_reference(x.numpy(), w.numpy(), bn[1].numpy(), bn[0].numpy(), d, relu=False))
    if relu:
        sw.both_sides(pre)
    want = sw.torch.relu(pre) if relu else pre
    for _ in sw.passes():
        xd = sw.d(x, "x")
        taps = sw.packed(pkg.filter_pack_s2, (3, 3, C, K), "taps", sw.d(w, "w"))
        bd, sd = sw.bnd(bn)
        outs = [pkg.conv3x3_dilated_bn_relu(xd, taps, bd, sd, d, relu=relu, out=sw.nan(N, H + 2, W + 2, K))
                for _ in range(2)]
        sw.agree(outs, want, padded=True)


def dilated_block_case(pkg, knobs, torch_dev, case, seed):
    sw = start(pkg, knobs, torch_dev, case, seed)
    N, H, W, Cin, Cm, C4, d, proj = case.N, case.H, case.W, case.Cin, case.Cm, case.C4, case.d, case.proj
    B = ProjCase(sw, types.SimpleNamespace(N=N, Hin=H, Win=W, Cin=Cin, Cm=Cm, C4=C4))
    f = lambda a: a.numpy().astype(np.float64)
    bn = [(f(b), f(s)) for b, s in B.bn]
    x2 = f(B.x).reshape(-1, Cin)
    t1p = np.zeros((N, H + 2, W + 2, Cm))
    t1p[:, 1:-1, 1:-1, :] = np.maximum(x2 @ f(B.w1) * bn[0][1] + bn[0][0], 0).reshape(N, H, W, Cm)
    t2 = dilated_reference(t1p, f(B.w2), bn[1][1], bn[1][0], d, True).reshape(-1, Cm)
    sc = (x2 @ f(B.wp) * bn[3][1] + bn[3][0]) if proj else x2
    pre = sw.torch.from_numpy((t2 @ f(B.w3) * bn[2][1] + bn[2][0] + sc).reshape(N, H, W, C4))
    sw.both_sides(pre)
    L = pkg.lib()
    query = "wino_proj_block_workspace_bytes_hw" if proj else "wino_residual_block_workspace_bytes_hw"
    need = getattr(L, query)(N, H, W, Cm)
    for _ in sw.passes():
        xd, w1d = sw.d(B.x, "x"), sw.d(B.w1, "w1")
        bnd = [sw.bnd(b, f"bn{i}") for i, b in enumerate(B.bn[:3 + proj])]
        taps = sw.packed(pkg.filter_pack_s2, (3, 3, Cm, Cm), "taps", sw.d(B.w2, "w2"))
        if proj:
            last = sw.packed(pkg.proj_tail_pack, L.wino_proj_tail_elems(Cm, Cin, C4), "tail", sw.d(B.w3, "w3"), bnd[2],
                             sw.d(B.wp, "wp"), bnd[3])
            run = lambda: pkg.dilated_proj_block(xd, w1d, bnd[0], taps, bnd[1], last, d, out=sw.nan(N, H, W, C4),
                                                 workspace=sw.ws(need, query))
        else:
            last = sw.d(B.w3, "w3")
            run = lambda: pkg.dilated_residual_block(xd, w1d, bnd[0], taps, bnd[1], last, bnd[2], d,
                                                     out=sw.nan(N, H, W, C4), workspace=sw.ws(need, query))
        outs = [run(), run()]
        sw.agree(outs, sw.torch.relu(pre))


# ---- the concat projection and ASPP ------------------------------------------------------------------------------------
def cat_case(pkg, knobs, torch_dev, case, seed):
    sw = start(pkg, knobs, torch_dev, case, seed)
    torch = sw.torch
    N, H, W, S, Cs, Kout, gap = case.N, case.H, case.W, case.S, case.Cs, case.Kout, case.gap
    relu, a_pad, c_pad = case.flags["relu"], case.flags["a_padded"], case.flags["c_padded"]
    srcs = [sw.act(N, H, W, Cs) for _ in range(S)]
    w = (sw.rand(S * Cs, Kout) - 0.5) / np.sqrt(S * Cs) * 4
    bias = sw.rand(N, Kout) * 8 - 4            # a neighbouring image's row is far outside TIGHT
    scale = bn_pair(sw.rand, Kout)[1]
    pre = torch.from_numpy(AC.cat_reference([s.numpy() for s in srcs], w.numpy(), bias.numpy(), scale.numpy(), False))
    if relu:
        sw.both_sides(pre)
    want = torch.relu(pre) if relu else pre
    # the sources in one buffer, `stride` floats apart: NaN between them and in the rings of padded sources
    shape = (N, H + 2, W + 2, Cs) if a_pad else (N, H, W, Cs)
    n = int(np.prod(shape))
    stride = n + gap
    master = torch.full(((S - 1) * stride + n,), float("nan"))
    for j, src in enumerate(srcs):
        v = master[j * stride: j * stride + n].view(shape)
        (v[:, 1:-1, 1:-1, :] if a_pad else v).copy_(src)
    flags = (AC.RELU if relu else 0) | (AC.A_PADDED if a_pad else 0) | (AC.C_PADDED if c_pad else 0)
    out_shape = (N, H + 2, W + 2, Kout) if c_pad else (N, H, W, Kout)
    for _ in sw.passes():
        buf = sw.d(master, "sources")
        views = [buf[j * stride: j * stride + n].view(shape) for j in range(S)]
        wd, bd, sd = sw.d(w, "w"), sw.d(bias, "bias_per_image"), sw.d(scale, "scale")
        outs = [pkg.conv1x1_cat_bn(views, wd, bd, sd, flags, out=sw.nan(*out_shape)) for _ in range(2)]
        sw.agree(outs, want, padded=c_pad)


class AsppProblem:
    """An ASPP case's tensors (image n's input is shifted by 0.2 n: the pooled branch differs from image to image) and
    its fp64 reference, with and without the pooled branch."""

    def __init__(self, sw, case):
        N, H, W, Cin, Cb, Kout = case.N, case.H, case.W, case.Cin, case.Cb, case.Kout
        shift = 0.2 * sw.torch.arange(N, dtype=sw.torch.float32)[:, None, None, None]
        self.x = ring(sw.act(N, H, W, Cin) + shift)
        r = sw.rand
        self.w0, self.ws = w11(r, Cin, Cb), [conv_w(r, Cb, Cin) for _ in range(3)]
        self.w_pool, self.w_proj = w11(r, Cin, Cb), w11(r, 5 * Cb, Kout)
        self.bn = [bn_pair(sw.rand, c) for c in (Cb, Cb, Cb, Cb, Cb, Kout)]   # b0, three dilated, pool, proj
        self.rates = tuple(case.rates)

    def reference(self, pooled=True):
        n = lambda a: a.numpy()
        bn = [(n(b), n(s)) for b, s in self.bn]
        return AC.aspp_reference(n(self.x), n(self.w0), bn[0], [n(w) for w in self.ws], bn[1:4], self.rates,
                                 n(self.w_pool), bn[4], n(self.w_proj), bn[5], pooled)


def aspp_case(pkg, knobs, torch_dev, case, seed):
    sw = start(pkg, knobs, torch_dev, case, seed)
    N, H, W, Cin, Cb, Kout = case.N, case.H, case.W, case.Cin, case.Cb, case.Kout
    P = AsppProblem(sw, case)
    want = sw.torch.from_numpy(P.reference())
    assert float((want > 0).double().mean()) > 0.05 and bool((want == 0).any()), f"{sw.tag}: the ReLU sees one side only"
    need = pkg.aspp_workspace_bytes(N, H, W, Cin, Cb, Kout)
    for _ in sw.passes():
        xd, w0, w_pool, w_proj = sw.d(P.x, "x"), sw.d(P.w0, "w0"), sw.d(P.w_pool, "w_pool"), sw.d(P.w_proj, "w_proj")
        taps = [sw.packed(pkg.filter_pack_s2, (3, 3, Cin, Cb), f"taps{i}", sw.d(w, f"w{i + 1}")) for i, w in enumerate(P.ws)]
        bnd = [sw.bnd(b, f"bn{i}") for i, b in enumerate(P.bn)]
        outs = [pkg.aspp(xd, w0, bnd[0], taps, bnd[1:4], P.rates, w_pool, bnd[4], w_proj, bnd[5],
                         out=sw.nan(N, H + 2, W + 2, Kout), workspace=sw.ws(need, "aspp_workspace_bytes"))
                for _ in range(2)]
        sw.agree(outs, want, padded=True)


# ---- the bilinear resize and label map ---------------------------------------------------------------------------------
def resize_src(sw, case):
    """src [N][h(+2)][w(+2)][ld]: the classes uniform in [-0.5, 0.5), NaN in the columns past C and in the ring."""
    N, h, w, C, ld = case.N, case.h, case.w, case.C, case.ld
    x = sw.torch.full((N, h, w, ld), float("nan"))
    x[..., :C] = sw.rand(N, h, w, C) - 0.5
    return ring(x, float("nan")) if case.flags["in_padded"] else x


def resize_case(pkg, knobs, torch_dev, case, seed):
    sw = start(pkg, knobs, torch_dev, case, seed)
    torch = sw.torch
    N, Ho, Wo, C, padded, use = case.N, case.Ho, case.Wo, case.C, case.flags["in_padded"], case.outputs
    src = resize_src(sw, case)
    want = RC.resize_reference(src.numpy(), Ho, Wo, C, padded)
    for _ in sw.passes():
        xd = sw.d(src, "src")
        runs = []
        for _ in range(2):
            out = sw.nan(N, C, Ho, Wo, name="out") if use != "labels" else None
            # (the arena holds float32: an unwritten label keeps the NaN bit pattern, which is no class)
            lab = sw.nan(N, Ho, Wo, name="labels").view(torch.int32) if use != "out" else None
            o, l = pkg.resize_bilinear(xd, Ho, Wo, C=C, in_padded=padded, out=out, labels=lab,
                                       want_out=out is not None, want_labels=lab is not None)
            assert (o is None) == (out is None) and (l is None) == (lab is None), sw.tag
            runs.append((o, l))
        (o, l), (o2, l2) = runs
        if o is not None:
            sw.close(o, torch.from_numpy(want))
            sw.same(o.view(torch.int32), o2.view(torch.int32))
        if l is not None:
            lab = l.cpu().numpy()
            assert lab.min() >= 0 and lab.max() < C, f"{sw.tag}: labels outside [0, {C}) (not all written)"
            RC.check_labels(lab, want, TIGHT, sw.tag)
            sw.same(l, l2, "labels")
        if use == "both":   # the label is the argmax of the values that were stored
            assert np.array_equal(l.cpu().numpy(), RC.labels_of(o.cpu().numpy())), f"{sw.tag}: labels != argmax(out)"
