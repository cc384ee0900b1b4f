"""Guard-band tests of what no sweep reaches: every tensor of a launch lies on the guarded arena of tests/guarded.py
(inputs between NaN guards, outputs and workspaces of exactly the queried size between sentinel guards), every case
runs at both placements (256-byte aligned, and 16 mod 256: the weakest pointer winograd_mi355x.h accepts), is compared
with its fp64 reference at TIGHT, and ends in arena.check: no guard touched, no read-only operand written.

Covered here: the pack and filter-transform entry points at their smallest legal shape, a ResNet stage shape and
K = 64 x odd with the smallest C (through their consumers' sweep cases, tests/sweep_cases.py, where no index
function is exported); conv1x1_bn_ex in every operand form x launch form; residual_block(_hw); the F(4x4) compatibility
path; the direct comparators; and that every *_workspace_bytes* query is exercised at exactly its size somewhere.

Not covered: the other tests past 4 GiB (tests/test_gpu_large_tensors.py, test_stem_past_4gib) build their tensors
in place on the device, have no CPU masters and exist for 64-bit offsets, which they check; guards on their outputs can
follow.  Whole-network runs are left out because resnet.py allocates its own activations.  The library-owned stream-K
scratch (slabs, tickets, error word) cannot be guarded from outside.  What a guard proves: no store outside the tensor,
and no load outside it whose value reaches the result; a load that is out of range and discarded is not seen."""
import ctypes

import numpy as np
import pytest

import guarded as G
import layer_refs as LR
import shape_sweeps as S
import sweep_cases as SC
from cases import TIGHT
from forms_1x1 import knobs_set as _knobs
from gpu_support import torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu


def _close(got, want, tag):
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else got
    assert got.shape == want.shape, f"{tag}: shape {got.shape} != {want.shape}"
    assert np.isfinite(got).all(), f"{tag}: non-finite values (not all written, or a guard was read)"
    err = LR.rel(got, want, floor=1e-30)
    print(f"{tag}: rel err {err:.3e}")
    assert err < TIGHT, f"{tag}: rel err {err:.3e}"


# ---- the guards can fail on the device too ---------------------------------------------------------------------------
def test_a_planted_store_past_an_output_is_caught(pkg, torch_dev):
    """A real launch into an arena output, then one float stored by the test itself just past that output (and, in a
    second round, just before it): arena.check must raise and name the tensor, the side and the offset."""
    torch, dev = torch_dev
    rng = np.random.RandomState(5)
    A, B = (rng.rand(113, 64) - 0.5).astype(np.float32), (rng.rand(64, 64) - 0.5).astype(np.float32)
    b, s = (rng.rand(64) - 0.5).astype(np.float32), (rng.rand(64) + 0.5).astype(np.float32)
    want = (A.astype(np.float64) @ B) * s + b
    for align in G.ALIGNS:
        for side, text in (("back", "4 bytes written starting 0 bytes past the end"),
                           ("front", "4 bytes written starting 4 bytes before the start")):
            arena = G.Arena(torch, dev, align=align)
            t = lambda a: arena.input(torch.from_numpy(a))
            out = arena.output(113, 64, name="victim")
            pkg.conv1x1_bn(t(A), t(B), t(b), t(s), False, out=out)
            arena.check("clean")
            slot = next(x for x in arena.slots if x.name == "victim")
            raw = slot.buf                                        # the whole allocation, guards included
            raw[slot.start + slot.numel if side == "back" else slot.start - 1] = 1.0
            with pytest.raises(G.GuardError) as e:
                arena.check("planted")
            msg = str(e.value)
            assert msg.startswith("planted: victim (output, (113, 64))") and f"{side} guard" in msg and text in msg, msg
            assert msg.count("guard:") == 1, msg                  # nothing else is blamed
            _close(out, want, f"planted align={align}")           # the tensor itself is untouched


# ---- pack and filter-transform entry points --------------------------------------------------------------------------
PACK_CK = [(8, 64), (128, 128), (8, 192)]   # smallest legal; a ResNet stage; K = 64 x odd with the smallest C


def _f2_index(L, C, K):
    e, c, k = np.meshgrid(np.arange(16), np.arange(C), np.arange(K), indexing="ij")
    idx = np.fromiter((L.wino_filter_f2_index(C, K, int(a), int(b), int(d))
                       for a, b, d in zip(e.ravel(), c.ravel(), k.ravel())), dtype=np.int64, count=e.size)
    assert idx.min() == 0 and idx.max() == 16 * C * K - 1 and np.unique(idx).size == idx.size, "not a permutation"
    return idx


@pytest.mark.parametrize("C,K", PACK_CK)
def test_filter_transform_and_import_kernels(C, K, pkg, O, torch_dev):
    """filter_transform_f2_kernel and filter_import_f4_kernel into exactly wino_filter_f2_elems floats: every element
    of U is where wino_filter_f2_index says, recomputed in fp64 (G g G^T) on the CPU."""
    torch, dev = torch_dev
    L = pkg.lib()
    rng = np.random.RandomState(C + K)
    w = (rng.rand(K, C, 3, 3) - 0.5).astype(np.float32)
    u36 = np.einsum('xr,kcrs,ys->xyck', O.G_F4, w.astype(np.float64), O.G_F4).reshape(36, C, K).astype(np.float32)
    want = O.f2_filter_transform(w).reshape(-1)             # [16][C][K], fp64
    n = L.wino_filter_f2_elems(C, K)
    assert n == 16 * C * K
    idx = _f2_index(L, C, K)
    for align in G.ALIGNS:
        arena = G.Arena(torch, dev, align=align)
        U1 = pkg.filter_transform_f2(arena.input(torch.from_numpy(w), name="w"), out=arena.output(n, name="U1"))
        U2 = pkg.filter_import_f4(arena.input(torch.from_numpy(u36), name="u36"), out=arena.output(n, name="U2"))
        tag = f"[filter C={C} K={K} align={align}]"
        _close(U1.cpu().numpy()[idx], want, tag + " transform_f2")
        _close(U2.cpu().numpy()[idx], want, tag + " import_f4")
        arena.check(tag)


def _case(entry, shape, **flags):
    return S.Case(entry, shape, None, None, flags)


# each pack entry point without an index function, through its consumer's sweep case (the pack writes through out= into
# exactly *_elems floats between guards, the consumer reads it from a guarded address; fp64 reference at TIGHT)
PACK_CASES = [
    # filter_pack_s2 + s2_proj_pack_kernel -> conv3x3_s2_proj
    (SC.s2_proj_case, _case("conv3x3_s2_proj", {"N": 1, "Hin": 2, "Win": 2, "C": 32, "K": 64}, nonneg=False)),
    (SC.s2_proj_case, _case("conv3x3_s2_proj", {"N": 1, "Hin": 56, "Win": 56, "C": 64, "K": 128}, nonneg=True)),
    (SC.s2_proj_case, _case("conv3x3_s2_proj", {"N": 2, "Hin": 9, "Win": 7, "C": 32, "K": 192}, nonneg=False)),
    # filter_pack_s2 alone -> conv3x3_s2_bn_relu
    (SC.s2_case, _case("conv3x3_s2_bn_relu", {"N": 1, "Hin": 1, "Win": 1, "C": 32, "K": 64}, nonneg=False, relu=False)),
    (SC.s2_case, _case("conv3x3_s2_bn_relu", {"N": 2, "Hin": 28, "Win": 28, "C": 128, "K": 256}, nonneg=True, relu=True)),
    (SC.s2_case, _case("conv3x3_s2_bn_relu", {"N": 3, "Hin": 5, "Win": 11, "C": 32, "K": 320}, nonneg=False, relu=True)),
    # proj_tail_pack_kernel -> proj_block
    (SC.proj_case, _case("proj_block", {"N": 1, "Hin": 1, "Win": 1, "Cin": 32, "Cm": 64, "C4": 64, "stride": 1},
                          nonneg=False)),
    (SC.proj_case, _case("proj_block", {"N": 1, "Hin": 56, "Win": 56, "Cin": 64, "Cm": 64, "C4": 256, "stride": 1},
                          nonneg=True)),
    (SC.proj_case, _case("proj_block", {"N": 2, "Hin": 5, "Win": 7, "Cin": 32, "Cm": 64, "C4": 192, "stride": 2},
                          nonneg=False)),
    # stem_pack_kernel -> stem
    (SC.stem_case, _case("stem", {"N": 1, "H": 1, "W": 1, "K": 64}, padded=False)),
    (SC.stem_case, _case("stem", {"N": 1, "H": 224, "W": 224, "K": 64}, padded=True)),
    (SC.stem_case, _case("stem", {"N": 2, "H": 9, "W": 11, "K": 192}, padded=False)),
    # head_pack_kernel -> avgpool_fc
    (SC.head_case, _case("avgpool_fc", {"N": 1, "H": 1, "W": 1, "C": 32, "classes": 1}, padded=False)),
    (SC.head_case, _case("avgpool_fc", {"N": 2, "H": 7, "W": 7, "C": 512, "classes": 1000}, padded=True)),
    (SC.head_case, _case("avgpool_fc", {"N": 3, "H": 2, "W": 3, "C": 32, "classes": 192}, padded=False)),
]


@pytest.mark.parametrize("run,case", PACK_CASES, ids=[c.tag() for _, c in PACK_CASES])
def test_pack_kernels_through_their_consumers(run, case, pkg, knobs, torch_dev):
    assert S.macs(case) <= S.MAX_MACS
    before = SC.CHECKS[case.entry]
    run(pkg, knobs, torch_dev, case, 4000 + len(case.tag()))
    assert SC.CHECKS[case.entry] - before == 2, "both placements were checked"


def test_filter_pack_s2_layout(pkg, torch_dev):
    """filter_pack_s2 is w.permute(2, 3, 1, 0) whatever computes it: exact, into a guarded [3][3][C][K]."""
    torch, dev = torch_dev
    g = torch.Generator().manual_seed(12)
    for C, K in ((32, 64), (64, 128), (32, 192)):
        w = torch.rand(K, C, 3, 3, generator=g) - 0.5
        for align in G.ALIGNS:
            arena = G.Arena(torch, dev, align=align)
            taps = pkg.filter_pack_s2(arena.input(w, name="w"), out=arena.output(3, 3, C, K, name="taps"))
            assert torch.equal(taps.cpu(), w.permute(2, 3, 1, 0)), (C, K, align)
            arena.check(f"[filter_pack_s2 C={C} K={K} align={align}]")


# ---- conv1x1_bn_ex / _hw: every operand form x every launch form -----------------------------------------------------
# The two ranged forms of the tiled kernel share their knobs; the shape decides (sk1_grid in conv1x1.hip): with fewer
# ranges of the model's best length than CUs a tile's k-steps are split over short ranges that stay inside the tile
# (split-K, grid below the CU count); otherwise one or two ranges per CU run through the (row tile, k-step) space,
# stop inside a tile and go on in the next (stream-K).
RANGED = {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1}
FORMS_1X1 = {"auto": {},
             "tiled": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 0},
             "split_k": RANGED,
             "stream_k": RANGED,
             "latency": {"WINO_1X1_ALGO": "small"}}
# (N, H, W, Cin, Kout), all 32 k-steps deep: M = 1; M = 113 (one row past a row tile, K = 64 x 3); a ragged ResNet
# shape (conv4's 1024 -> 256 at 3 images: 5.25 row tiles); the same layer at 20 images (35 row tiles: 2240 (tile,
# k-step) units, enough for a range per CU)
M1, M113, M588, M3920 = (1, 1, 1, 1024, 256), (1, 1, 113, 1024, 192), (3, 14, 14, 1024, 256), (20, 14, 14, 1024, 256)
# the (shape, form) pairs the plan accepts: the three small shapes are too small for stream-K, the large one too large
# for split-K; the latency form is for few pixel rows
PAIRS_1X1 = ([(sh, f) for sh in (M1, M113, M588) for f in ("auto", "tiled", "split_k", "latency")]
             + [(M3920, f) for f in ("auto", "tiled", "stream_k")])


def _form_taken(pkg, M, Cin, Kout, cus=S.CUS):
    """The form the plan queries give the GEMM under the knobs currently set: latency, tiled, split_k or stream_k."""
    if pkg.small_plan_1x1_full(M, Cin, Kout, cus)[0]:
        return "latency"
    grid, row_tiles, col_blocks, k_steps, sk = (ctypes.c_int() for _ in range(5))
    rc = pkg.lib().wino_conv1x1_plan(M, Cin, Kout, cus, *[ctypes.byref(v) for v in (grid, row_tiles, col_blocks, k_steps, sk)])
    assert rc == 0, rc
    if not sk.value:
        return "tiled"
    step = 8
    while step % col_blocks.value:
        step += 8
    units = row_tiles.value * col_blocks.value * k_steps.value
    assert step <= grid.value <= units, (grid.value, units)
    # stream-K grids are the CU count or twice it, rounded down to whole XCD groups of column blocks
    return "stream_k" if grid.value >= cus - cus % step else "split_k"


def _operand_forms(pkg):
    R, A, C, ADD = pkg.RELU, pkg.A_PADDED, pkg.C_PADDED, pkg.ADD_RESIDUAL
    # the four forms alone, then residual_block's first (padded out + ReLU) and last (padded in + residual + ReLU)
    # launches, then everything at once
    return [0, R, A, C, ADD, C | R, A | ADD | R, A | C | ADD, A | C | ADD | R]


@pytest.mark.parametrize("shape,form", PAIRS_1X1, ids=["x".join(map(str, sh)) + "-" + f for sh, f in PAIRS_1X1])
def test_conv1x1_operand_forms(shape, form, pkg, knobs, torch_dev):
    """PLAIN, A_PADDED, C_PADDED (with its ring pass: zeros in out's ring and nothing else -- the back guard starts right
    behind the last ring pixel), ADD_RESIDUAL and residual_block's combinations, in each launch form -- tiled, split-K,
    stream-K, latency -- at the shapes whose plan takes it (asserted from the plan queries); fp64 reference on the
    CPU."""
    torch, dev = torch_dev
    N, H, W, Cin, Kout = shape
    M = N * H * W
    rng = np.random.RandomState(M + Cin)
    A = (rng.rand(N, H, W, Cin) - 0.5).astype(np.float32)
    Ap = ((rng.rand(N, H + 2, W + 2, Cin) - 0.5) * 50).astype(np.float32)
    Ap[:, 1:-1, 1:-1, :] = A
    B = ((rng.rand(Cin, Kout) - 0.5) / np.sqrt(Cin) * 4).astype(np.float32)
    b, s = (rng.rand(Kout) - 0.5).astype(np.float32), (rng.rand(Kout) + 0.5).astype(np.float32)
    s[::3] *= -1
    Rm = (rng.rand(M, Kout) - 0.5).astype(np.float32)
    lin = (A.reshape(M, Cin).astype(np.float64) @ B.astype(np.float64)) * s.astype(np.float64) + b.astype(np.float64)
    with _knobs(knobs, FORMS_1X1[form]):
        planned = _form_taken(pkg, M, Cin, Kout)
        assert form in ("auto", planned), f"{shape}: the plan takes the {planned} form, not the {form} form"
        for flags in _operand_forms(pkg):
            pre = lin + Rm if flags & pkg.ADD_RESIDUAL else lin
            want = np.maximum(pre, 0) if flags & pkg.RELU else pre
            if flags & pkg.RELU:
                assert (pre > 0).any() and (pre < 0).any()
            for align in G.ALIGNS:
                arena = G.Arena(torch, dev, align=align)
                t = lambda a, name: arena.input(torch.from_numpy(a), name=name)
                out = arena.output(*((N, H + 2, W + 2, Kout) if flags & pkg.C_PADDED else (M, Kout)), name="out")
                pkg.conv1x1_bn_ex(t(Ap, "A (padded)") if flags & pkg.A_PADDED else t(A, "A"), t(B, "B"), t(b, "bias"),
                                  t(s, "scale"), flags, residual=t(Rm, "residual") if flags & pkg.ADD_RESIDUAL else None,
                                  out=out, hw=(H, W))
                tag = f"[conv1x1_bn_ex {shape} form={form} plan={planned} flags={flags} align={align}]"
                got = out.cpu().numpy()
                if flags & pkg.C_PADDED:
                    assert LR.ring_is(got, 0.0), f"{tag}: ring is not exactly 0"
                    got = got[:, 1:-1, 1:-1, :].reshape(M, Kout)
                _close(got, want, tag)
                assert pkg.tickets_in_use() == 0, tag
                arena.check(tag)


def test_conv1x1_pairs_cover_every_launch_form():
    """Each of the issue's shapes (M = 1, M = 113, the ragged one) runs in the tiled, split-K and latency forms, and
    stream-K runs where it is legal; that a pair really takes its form is asserted in the test above."""
    for sh in (M1, M113, M588):
        assert {f for s_, f in PAIRS_1X1 if s_ == sh} == {"auto", "tiled", "split_k", "latency"}
    assert {f for _, f in PAIRS_1X1} == set(FORMS_1X1)
    assert (M3920, "stream_k") in PAIRS_1X1


# ---- residual_block / residual_block_hw ---------------------------------------------------------------------------------
THROUGHPUT = {"WINO_3X3_ALGO": "big", "WINO_1X1_ALGO": "big"}


@pytest.mark.parametrize("N,H,W,forced", [(1, 14, 14, {}), (1, 7, 9, {}), (5, 14, 14, THROUGHPUT), (5, 9, 11, THROUGHPUT),
                                          (3, 7, 7, THROUGHPUT)],
                         ids=["N1-14x14", "N1-7x9", "N5-14x14-throughput", "N5-9x11-throughput", "N3-7x7-throughput"])
def test_residual_block_between_guards(N, H, W, forced, pkg, knobs, torch_dev):
    """The bottleneck block with a workspace of exactly wino_residual_block_workspace_bytes(_hw): N = 1 in the forms
    the planner takes (the latency kernels: asserted), ragged batches with the throughput kernels forced.  A third pass
    puts the workspace at 16 mod 256 too, the checked minimum: the block carves t1 and t2 from it."""
    torch, dev = torch_dev
    C4, Cm = 256, 64
    g = torch.Generator().manual_seed(N * 100 + H)
    r = lambda *sh: torch.rand(*sh, generator=g)
    x = r(N, H, W, C4) - 0.5
    w1, w3 = (r(C4, Cm) - 0.5) / np.sqrt(C4) * 4, (r(Cm, C4) - 0.5) / np.sqrt(Cm) * 4
    w2 = (r(Cm, Cm, 3, 3) - 0.5) / np.sqrt(9 * Cm) * 4
    bn = [(r(c) - 0.5, r(c) + 0.5) for c in (Cm, Cm, C4)]
    pre = LR.bottleneck(x, w1, bn[0], w2, bn[1], w3, bn[2], pre=True)
    assert bool((pre > 0).any()) and bool((pre < 0).any())
    want = torch.relu(pre).numpy()
    L = pkg.lib()
    need = L.wino_residual_block_workspace_bytes_hw(N, H, W, Cm)
    if (H, W) == (14, 14):
        assert L.wino_residual_block_workspace_bytes(N, Cm) == need
    assert need == 2 * N * (H + 2) * (W + 2) * Cm * 4
    queries = ["wino_residual_block_workspace_bytes_hw"] + ["wino_residual_block_workspace_bytes"] * ((H, W) == (14, 14))
    with _knobs(knobs, forced):
        forms = (S.form_1x1(pkg, N * H * W, C4, Cm), S.plan_3x3(pkg, N, H, W, Cm, Cm)[0], S.form_1x1(pkg, N * H * W, Cm, C4))
        if forced:
            assert "latency" not in forms, forms
        else:
            assert forms == ("latency",) * 3, f"N={N} {H}x{W}: the planner takes {forms}, not the latency forms"
        for align, ws_align in ((256, 256), (16, 256), (16, 16)):
            arena = G.Arena(torch, dev, align=align)
            d = lambda t, name: arena.input(t, name=name)
            U2 = pkg.filter_transform_f2(d(w2, "w2"), out=arena.output(L.wino_filter_f2_elems(Cm, Cm), name="U2 (pack out)"))
            bnd = [(d(p[0], f"bn{i}.bias"), d(p[1], f"bn{i}.scale")) for i, p in enumerate(bn)]
            ws = arena.workspace(need, align=ws_align, name="workspace", query=queries)
            assert ws.numel() * 4 == need and ws.data_ptr() % 256 == ws_align % 256
            out = pkg.residual_block(d(x, "x"), d(w1, "w1"), bnd[0], d(U2, "U2"), bnd[1], d(w3, "w3"), bnd[2],
                                     out=arena.output(N, H, W, C4, name="out"), workspace=ws)
            tag = f"[residual_block N={N} H={H} W={W} C4={C4} Cm={Cm} {'throughput' if forced else 'auto'} align={align} workspace at {ws_align}]"
            _close(out, want, tag)
            assert pkg.tickets_in_use() == 0, tag
            arena.check(tag)


# ---- the F(4x4) compatibility path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 13])
def test_f4_compat_path_between_guards(N, pkg, O, torch_dev):
    """The reference's three stages with V and M in a workspace of exactly wino_conv3x3_f4_workspace_bytes, against the
    fp64 direct convolution."""
    torch, dev = torch_dev
    C, K = 64, 128
    rng = np.random.RandomState(40 + N)
    x = (rng.rand(N, 16, 16, C) - 0.5).astype(np.float32)
    w = (rng.rand(K, C, 3, 3) - 0.5).astype(np.float32)
    s, b = (rng.rand(K) - 0.5).astype(np.float32), (rng.rand(K) - 0.5).astype(np.float32)
    u36 = np.einsum('xr,kcrs,ys->xyck', O.G_F4, w.astype(np.float64), O.G_F4).reshape(36, C, K).astype(np.float32)
    need = pkg.lib().wino_conv3x3_f4_workspace_bytes(N, C, K)
    for relu in (True, False):
        want = O.conv3x3_bn_relu_direct(x, w, s, b, relu=relu)
        for align in G.ALIGNS:
            arena = G.Arena(torch, dev, align=align)
            t = lambda a, name: arena.input(torch.from_numpy(a), name=name)
            ws = arena.workspace(need, name="workspace", query="wino_conv3x3_f4_workspace_bytes")
            assert ws.numel() * 4 == need
            out = pkg.conv3x3_f4_bn_relu(t(x, "x"), t(u36, "u36"), t(b, "bias"), t(s, "scale"), relu=relu,
                                         out=arena.output(N, 16, 16, K, name="out"), workspace=ws)
            tag = f"[conv3x3_f4_bn_relu N={N} C={C} K={K} relu={relu} align={align}]"
            got = out.cpu().numpy()
            assert LR.ring_is(got, 0.0), f"{tag}: ring is not exactly 0"
            _close(got, want, tag)
            arena.check(tag)


# ---- the direct comparators ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W,C,K", [(1, 1, 1, 8, 64), (2, 5, 3, 24, 64), (3, 14, 14, 16, 192)])
def test_conv3x3_direct_between_guards(N, H, W, C, K, pkg, O, torch_dev):
    torch, dev = torch_dev
    rng = np.random.RandomState(N + H + C)
    x = (rng.rand(N, H + 2, W + 2, C) - 0.5).astype(np.float32)
    w = (rng.rand(K, C, 3, 3) - 0.5).astype(np.float32)
    s, b = (rng.rand(K) - 0.5).astype(np.float32), (rng.rand(K) - 0.5).astype(np.float32)
    for relu in (True, False):
        want = O.conv3x3_bn_relu_direct(x, w, s, b, relu=relu)[:, 1:-1, 1:-1, :]
        for align in G.ALIGNS:
            arena = G.Arena(torch, dev, align=align)
            t = lambda a, name: arena.input(torch.from_numpy(a), name=name)
            out = pkg.conv3x3_direct(t(x, "x"), t(w, "w"), t(b, "bias"), t(s, "scale"), relu=relu,
                                     out=arena.output(N, H + 2, W + 2, K, name="out"))
            tag = f"[conv3x3_direct N={N} H={H} W={W} C={C} K={K} relu={relu} align={align}]"
            _close(out.cpu().numpy()[:, 1:-1, 1:-1, :], want, tag)
            arena.check(tag)


@pytest.mark.parametrize("M,Cin,Kout", [(1, 32, 64), (113, 96, 192), (588, 256, 64)])
def test_conv1x1_direct_between_guards(M, Cin, Kout, pkg, O, torch_dev):
    torch, dev = torch_dev
    rng = np.random.RandomState(M + Cin)
    A, B = (rng.rand(M, Cin) - 0.5).astype(np.float32), (rng.rand(Cin, Kout) - 0.5).astype(np.float32)
    s, b = (rng.rand(Kout) - 0.5).astype(np.float32), (rng.rand(Kout) - 0.5).astype(np.float32)
    for relu in (True, False):
        want = O.conv1x1_bn(A, B, b, s, relu)
        for align in G.ALIGNS:
            arena = G.Arena(torch, dev, align=align)
            t = lambda a, name: arena.input(torch.from_numpy(a), name=name)
            out = pkg.conv1x1_direct(t(A, "A"), t(B, "B"), t(b, "bias"), t(s, "scale"), relu,
                                     out=arena.output(M, Kout, name="out"))
            tag = f"[conv1x1_direct M={M} Cin={Cin} Kout={Kout} relu={relu} align={align}]"
            _close(out, want, tag)
            arena.check(tag)


# ---- every workspace query is run at exactly its size ------------------------------------------------------------------
def test_every_workspace_query_has_a_guarded_run(pkg, knobs, O, torch_dev):
    """For every *_workspace_bytes* symbol of the ABI, one small block is run here with a workspace of exactly the
    reported size between sentinel guards, and the arena counts the run (guarded.WORKSPACE_RUNS: incremented by a
    passing arena.check for the query the workspace was carved for).  A size query added to the ABI without such a run
    fails here."""
    runs = {
        "wino_residual_block_workspace_bytes": lambda: test_residual_block_between_guards(1, 14, 14, {}, pkg, knobs, torch_dev),
        "wino_residual_block_workspace_bytes_hw": lambda: test_residual_block_between_guards(1, 7, 9, {}, pkg, knobs, torch_dev),
        "wino_conv3x3_f4_workspace_bytes": lambda: test_f4_compat_path_between_guards(1, pkg, O, torch_dev),
        "wino_basic_block_workspace_bytes_hw": lambda: SC.basic_block_case(
            pkg, knobs, torch_dev, _case("basic_block", {"N": 1, "H": 2, "W": 3, "C": 64}, in_place=False, nonneg=False), 1),
        "wino_basic_block_s2_workspace_bytes_hw": lambda: SC.basic_block_s2_case(
            pkg, knobs, torch_dev, _case("basic_block_s2", {"N": 1, "Hin": 3, "Win": 4, "C": 32, "K": 64}, nonneg=False), 2),
        "wino_proj_block_workspace_bytes_hw": lambda: SC.proj_case(
            pkg, knobs, torch_dev, _case("proj_block", {"N": 1, "Hin": 2, "Win": 3, "Cin": 32, "Cm": 64, "C4": 64, "stride": 1},
                                         nonneg=False), 3),
        "wino_proj_block_v15_workspace_bytes_hw": lambda: SC.v15_case(
            pkg, knobs, torch_dev, _case("proj_block_v15", {"N": 1, "Hin": 3, "Win": 2, "Cin": 32, "Cm": 64, "C4": 64},
                                         nonneg=False), 4),
        "wino_head_workspace_bytes": lambda: SC.head_case(
            pkg, knobs, torch_dev, _case("avgpool_fc", {"N": 2, "H": 1, "W": 2, "C": 32, "classes": 5}, padded=False), 5),
    }
    queries = {s for s in pkg.ABI_SYMBOLS if "workspace_bytes" in s}
    assert queries == set(runs), queries ^ set(runs)
    for q, run in runs.items():
        before = G.WORKSPACE_RUNS[q]
        run()
        assert G.WORKSPACE_RUNS[q] - before >= 2, f"{q}: no guarded run at both placements was counted"
