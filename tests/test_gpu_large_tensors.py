"""Every layer and block past 2 GiB and 4 GiB tensors (run with `-m gpu` on an MI355X).

The kernels address their tensors through buffer descriptors: 32-bit sizes and 32-bit byte offsets.  The library
re-bases them (the 1x1 kernels at every tile's first row, the 3x3 launcher by cutting a batch into launches whose
tensors stay below 4 GiB), so each entry point takes tensors of any size.  Here every operand form and block runs at a
batch whose tensors cross 2^31 and 2^32 bytes, into NaN-filled outputs and workspaces:

* on the GPU, the whole output is finite and its padded ring exactly zero;
* the images around each boundary (n = 2^31 // P and 2^32 // P, with n - 1 and n + 1, for every tensor of P bytes per
  image that crosses it), both sides of every batch cut, the first and the last image match an fp64 reference on the
  CPU (the suite's own: the oracle module and the reference methods of the other GPU test files) at TIGHT;
* a second launch gives the same bits on those images, and no stream-K ticket is left held.

The box kernels are plain HIP with 64-bit addresses: batched NMS runs at its widest segments, with a
workspace past 4 GiB and at its largest segment counts, box decode with a head and with an output past 4 GiB.  The image
transform and the segmented select (at the end) run at the limits their entry points accept: coord()'s 2 out in < 2^31, an
out past 4 GiB, the largest source image, scores addressed past 2^31 elements, the longest segment and the most segments.

Inputs are built on the device from a seeded generator; a case skips when the card has less free memory than it needs
(at most about 20 GiB for the layers; about 60 GiB for the select past 2^31 elements, whose boxes have a stride of 2^30
rows of 16 bytes)."""
import ctypes
import types

import numpy as np
import pytest

import box_cases as bc
import layer_refs as LR
import select_cases as sc
import transform_cases as tc
from aspp_cases import cat_reference
from cases import TIGHT, S2Block, V15Block, proj_weights, ring_zero
from dilated_cases import dilated_reference
from fpn_reference import level_reference
from gpu_support import run_nms, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu

GIB = 1 << 30
NAN = float("nan")

FORMS_1X1 = {
    "default": {},
    "tiled": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 0},
    "stream_k": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1},
}


@pytest.fixture
def free_after(torch_dev):
    torch, _ = torch_dev
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _need(torch, nbytes):
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes + GIB:
        pytest.skip(f"needs {(nbytes + GIB) / GIB:.1f} GiB of free device memory, {free / GIB:.1f} free")


def _set(knobs, form):
    for k, v in form.items():
        knobs.set(k, v)


def _images(N, per_image_bytes, cuts=()):
    """The images to check: both sides of 2^31 and 2^32 bytes for every tensor of P bytes per image that crosses them,
    both sides of every batch cut, the first and the last."""
    s = {0, N - 1}
    for P in per_image_bytes:
        for b in (1 << 31, 1 << 32):
            if N * P > b:
                n = b // P
                s |= {n - 1, n, n + 1}
    for c in cuts:
        s |= {c - 1, c}
    return sorted(i for i in s if 0 <= i < N)


def _rand(torch, dev, shape, seed, out=None):
    """Uniform in [-0.5, 0.5) from a seeded generator on the device (into `out` when given: the same values again)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    if out is not None:
        return torch.rand(out.shape, device=dev, generator=g, out=out).sub_(0.5)
    return torch.rand(*shape, device=dev, generator=g).sub_(0.5)


def _padded_rand(torch, dev, N, H, W, C, seed, out=None):
    """[N][H+2][W+2][C], interior uniform in [-0.5, 0.5), zero ring; built in place (no interior-sized temporary)."""
    return LR.fill_ring(_rand(torch, dev, (N, H + 2, W + 2, C), seed, out=out))


def _finite(torch, t):
    """Every element finite, on the GPU, a slab of images at a time."""
    step = max(1, (1 << 28) // max(1, t[0].numel()))
    return all(bool(torch.isfinite(t[i:i + step]).all()) for i in range(0, t.shape[0], step))


def _pick(torch, t, idx):
    return t[torch.as_tensor(idx, device=t.device)].cpu()


def _check_padded(O, torch, out, idx, want, name=""):
    """out [N][H+2][W+2][K] on the GPU: finite, zero ring, the images idx against want [n][H][W][K]."""
    assert _finite(torch, out), name
    assert ring_zero(out), name
    got = _pick(torch, out, idx)
    assert O.rel_error(got[:, 1:-1, 1:-1, :].numpy(), want) < TIGHT, name
    return got


# ------------------------------------------------------------------ the residual 3x3 (a batch cut into two launches)
N_3X3, H_3X3, C_3X3 = 5100, 56, 64
CUT_3X3 = 4928   # the first launch: the largest multiple of 64 images whose tensors stay below 4 GiB


@pytest.mark.parametrize("form", ["default", "stream_k_tail"])
@pytest.mark.parametrize("in_place", [False, True])
def test_residual_3x3_beyond_4gib(form, in_place, pkg, O, torch_dev, knobs, free_after):
    """conv3x3_bn_add_relu, 5100 images of 56x56x64: in, res and out are 4.4 GB each; the launcher cuts the batch
    at 4928 and advances in, res and out together.  Out of place and in place (res is out); the planner's form, and
    the throughput kernel forced with a grid that leaves a stream-K tail in both launches."""
    torch, dev = torch_dev
    N, H, C = N_3X3, H_3X3, C_3X3
    P = (H + 2) * (H + 2) * C * 4
    _need(torch, (2 if in_place else 3) * N * P)
    if form == "stream_k_tail":
        knobs.set("WINO_3X3_ALGO", "big")
        knobs.set("WINO_SK_GRID", 1000)   # 60368 and 2107 items: tails of 368 and 107
    idx = _images(N, [P], cuts=[CUT_3X3])
    g = torch.Generator(device="cpu").manual_seed(71)
    w = (torch.rand(C, C, 3, 3, generator=g) - 0.5) / np.sqrt(9 * C) * 4
    bias, scale = torch.rand(C, generator=g) - 0.5, torch.rand(C, generator=g) + 0.5
    U, bt, st = pkg.filter_transform_f2(w.to(dev)), bias.to(dev), scale.to(dev)
    x = _padded_rand(torch, dev, N, H, H, C, 72)
    res = _padded_rand(torch, dev, N, H, H, C, 73)
    want = LR.conv3x3(LR.interior(_pick(torch, x, idx)), w, (bias, scale), True,
                      residual=LR.interior(_pick(torch, res, idx))).numpy()
    out = res if in_place else torch.empty_like(x)
    first = None
    for rep in range(2):
        if in_place and rep:   # the first launch overwrote the residual: the same values again
            _padded_rand(torch, dev, N, H, H, C, 73, out=res)
        if not in_place:
            out.fill_(NAN)
        got = pkg.conv3x3_bn_add_relu(x, U, bt, st, res, out=out)
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        assert pkg.tickets_in_use() == 0
        g_idx = _check_padded(O, torch, out, idx, want, f"rep {rep}")
        if first is None:
            first = g_idx
        assert torch.equal(g_idx, first)
    assert 0.2 < (want > 0).mean() < 0.8
    del x, res, out, got


def test_basic_block_beyond_4gib(pkg, O, torch_dev, free_after):
    """basic_block, 5100 images of 56x56x64: x, out and the workspace (t1) are 4.4 GB each; both convolutions are
    cut at 4928 images, the second reading x as its residual."""
    torch, dev = torch_dev
    N, H, C = N_3X3, H_3X3, C_3X3
    P = (H + 2) * (H + 2) * C * 4
    _need(torch, 3 * N * P)
    idx = _images(N, [P], cuts=[CUT_3X3])
    g = torch.Generator(device="cpu").manual_seed(81)
    ws_ = [(torch.rand(C, C, 3, 3, generator=g) - 0.5) / np.sqrt(9 * C) * 4 for _ in range(2)]
    bn = [(torch.rand(C, generator=g) - 0.5, torch.rand(C, generator=g) + 0.5) for _ in range(2)]
    U = [pkg.filter_transform_f2(w.to(dev)) for w in ws_]
    bnt = [(b.to(dev), s.to(dev)) for b, s in bn]
    x = _padded_rand(torch, dev, N, H, H, C, 82)
    x_idx = _pick(torch, x, idx)
    want = LR.basic_block(LR.interior(x_idx), ws_[0], bn[0], ws_[1], bn[1]).numpy()
    need = pkg.lib().wino_basic_block_workspace_bytes_hw(N, H, H, C)
    assert need == N * P
    out = torch.empty_like(x)
    ws = torch.empty(need // 4, device=dev)
    first = None
    for rep in range(2):
        out.fill_(NAN)
        ws.fill_(NAN)
        pkg.basic_block(x, U[0], bnt[0], U[1], bnt[1], out=out, workspace=ws)
        torch.cuda.synchronize()
        assert pkg.tickets_in_use() == 0
        g_idx = _check_padded(O, torch, out, idx, want, f"rep {rep}")
        assert _finite(torch, ws.view(N, H + 2, H + 2, C)) and ring_zero(ws.view(N, H + 2, H + 2, C))
        if first is None:
            first = g_idx
        assert torch.equal(g_idx, first)
    assert (want > 0).mean() > 0.2
    del x, out, ws


# ------------------------------------------------------------------ the chained 1x1 (A_PADDED, C_PADDED, ADD_RESIDUAL)
@pytest.mark.parametrize("form", sorted(FORMS_1X1))
def test_conv1x1_chaining_forms_beyond_4gib(form, pkg, O, torch_dev, knobs, free_after):
    """conv1x1_bn_ex at 56x56, 256 -> 256, 1400 images: A unpadded 4.5 GB or padded 4.8 GB, the residual 4.5 GB, out
    4.5 GB or (C_PADDED) 4.8 GB.  Every combination of A_PADDED, C_PADDED and ADD_RESIDUAL (with the ReLU), in the
    planner's form, tiled and stream-K."""
    torch, dev = torch_dev
    N, H, C, K = 1400, 56, 256, 256
    M = N * H * H
    Pu, Pp = H * H * C * 4, (H + 2) * (H + 2) * C * 4
    _need(torch, N * (Pu + Pp) + N * H * H * K * 4 + N * (H + 2) * (H + 2) * K * 4)
    _set(knobs, FORMS_1X1[form])
    idx = _images(N, [Pu, Pp])
    rng = np.random.RandomState(91)
    B = ((rng.rand(C, K) - 0.5) / np.sqrt(C) * 4).astype(np.float32)
    s = (rng.rand(K) + 0.5).astype(np.float32)
    b = (rng.rand(K) - 0.5).astype(np.float32)
    Bt, st, bt = (torch.from_numpy(a).to(dev) for a in (B, s, b))
    Ap = _rand(torch, dev, (N, H + 2, H + 2, C), 92)
    Ap[:, 0].fill_(NAN)                     # A_PADDED does not read the ring
    Ap[:, :, -1].fill_(1e6)
    Au = _rand(torch, dev, (N, H, H, C), 93)
    R = _rand(torch, dev, (M, K), 94)
    out_buf = torch.empty(N * (H + 2) * (H + 2) * K, device=dev)
    # the fp64 reference of the checked images: BN(A . B), then the residual and the ReLU per combination
    pick = lambda t: _pick(torch, t, idx).double().numpy()
    yp = O.conv1x1_bn(pick(Ap)[:, 1:-1, 1:-1, :].reshape(-1, C), B, b, s, False).reshape(len(idx), H, H, K)
    yu = O.conv1x1_bn(pick(Au).reshape(-1, C), B, b, s, False).reshape(len(idx), H, H, K)
    r_idx = pick(R.view(N, H, H, K))
    for flags in range(1, 8):
        a_pad, c_pad, add = bool(flags & 1), bool(flags & 2), bool(flags & 4)
        f = pkg.RELU | (pkg.A_PADDED if a_pad else 0) | (pkg.C_PADDED if c_pad else 0) | (pkg.ADD_RESIDUAL if add else 0)
        want = (yp if a_pad else yu) + (r_idx if add else 0)
        want = np.maximum(want, 0)
        out = out_buf.view(N, H + 2, H + 2, K) if c_pad else out_buf[:M * K].view(M, K)
        first = None
        for rep in range(2):
            out_buf.fill_(NAN)
            got = pkg.conv1x1_bn_ex(Ap if a_pad else Au, Bt, bt, st, f, residual=R if add else None, out=out)
            assert got.data_ptr() == out_buf.data_ptr()
            torch.cuda.synchronize()
            assert pkg.tickets_in_use() == 0, flags
            if c_pad:
                g_idx = _check_padded(O, torch, out, idx, want, f"flags {flags}")
            else:
                o4 = out.view(N, H, H, K)
                assert _finite(torch, o4), flags
                g_idx = _pick(torch, o4, idx)
                assert O.rel_error(g_idx.numpy(), want) < TIGHT, flags
            if first is None:
                first = g_idx
            assert torch.equal(g_idx, first), flags
        assert 0.2 < (want > 0).mean() < 0.8, flags
    del Ap, Au, R, out_buf, out, got


# ------------------------------------------------------------------ the stride-2 3x3 (A_TAPS) and its fused form
@pytest.mark.parametrize("form", sorted(FORMS_1X1))
def test_conv3x3_s2_beyond_4gib(form, pkg, O, torch_dev, knobs, free_after):
    """conv3x3_s2_bn_relu at conv3 (56 -> 28), 128 -> 128, 5200 images: the input is 9.0 GB (past 2^31, 2^32, 3 x 2^31
    and 2^33), the output 2.4 GB (past 2^31)."""
    torch, dev = torch_dev
    N, Hin, C, K = 5200, 56, 128, 128
    H = (Hin - 1) // 2 + 1
    Pin, Pout = (Hin + 2) * (Hin + 2) * C * 4, (H + 2) * (H + 2) * K * 4
    _need(torch, N * (Pin + Pout))
    _set(knobs, FORMS_1X1[form])
    idx = _images(N, [Pin, Pout])
    g = torch.Generator(device="cpu").manual_seed(101)
    w = (torch.rand(K, C, 3, 3, generator=g) - 0.5) / np.sqrt(9 * C) * 4
    bias, scale = torch.rand(K, generator=g) - 0.5, torch.rand(K, generator=g) + 0.5
    taps, bt, st = pkg.filter_pack_s2(w.to(dev)), bias.to(dev), scale.to(dev)
    x = _padded_rand(torch, dev, N, Hin, Hin, C, 102)
    want = LR.conv3x3(LR.interior(_pick(torch, x, idx)), w, (bias, scale), True, stride=2).numpy()
    out = torch.empty(N, H + 2, H + 2, K, device=dev)
    first = None
    for rep in range(2):
        out.fill_(NAN)
        pkg.conv3x3_s2_bn_relu(x, taps, bt, st, relu=True, out=out)
        torch.cuda.synchronize()
        assert pkg.tickets_in_use() == 0
        g_idx = _check_padded(O, torch, out, idx, want, f"rep {rep}")
        if first is None:
            first = g_idx
        assert torch.equal(g_idx, first)
    assert (want > 0).mean() > 0.2
    del x, out


@pytest.mark.parametrize("form", sorted(FORMS_1X1))
def test_downsampling_block_beyond_4gib(form, pkg, O, torch_dev, knobs, free_after):
    """conv3x3_s2_proj (A_TAPS_PROJ) and basic_block_s2 at the conv3 entry, 64 -> 128, 5100 images: x is 4.4 GB,
    t1, sc, out and the workspace 2.35 GB each (past 2^31)."""
    torch, dev = torch_dev
    N, Hin, C, K = 5100, 56, 64, 128
    H = (Hin - 1) // 2 + 1
    Pin, Pout = (Hin + 2) * (Hin + 2) * C * 4, (H + 2) * (H + 2) * K * 4
    _need(torch, N * (Pin + 2 * Pout))
    _set(knobs, FORMS_1X1[form])
    idx = _images(N, [Pin, Pout])
    g = torch.Generator(device="cpu").manual_seed(111)
    ref = types.SimpleNamespace(torch=torch)
    ref.w1 = (torch.rand(K, C, 3, 3, generator=g) - 0.5) / np.sqrt(9 * C) * 4
    ref.wd = (torch.rand(K, C, 1, 1, generator=g) - 0.5) / np.sqrt(C) * 4
    ref.w2 = (torch.rand(K, K, 3, 3, generator=g) - 0.5) / np.sqrt(9 * K) * 4
    vec = lambda lo: torch.rand(K, generator=g) + lo
    ref.b1, ref.s1, ref.bd, ref.sd, ref.b2, ref.s2 = vec(-0.5), vec(0.5), vec(-0.5), vec(0.5), vec(-0.5), vec(0.5)
    t = lambda a: a.contiguous().to(dev)
    packed = pkg.s2_proj_pack(pkg.filter_pack_s2(t(ref.w1)), (t(ref.b1), t(ref.s1)), t(ref.wd.view(K, C).t()),
                              (t(ref.bd), t(ref.sd)))
    U2, bn2 = pkg.filter_transform_f2(t(ref.w2)), (t(ref.b2), t(ref.s2))
    x = _padded_rand(torch, dev, N, Hin, Hin, C, 112)
    ref.x = _pick(torch, x, idx)
    want_t1, want_sc, want = S2Block.reference(ref)
    # the fused layer alone: t1 as the plain stride-2 layer writes it, sc's interior (its ring is not touched)
    t1 = torch.empty(N, H + 2, H + 2, K, device=dev)
    sc = torch.empty_like(t1)
    first = None
    for rep in range(2):
        t1.fill_(NAN)
        sc.fill_(NAN)
        pkg.conv3x3_s2_proj(x, packed, t1=t1, sc=sc)
        torch.cuda.synchronize()
        assert pkg.tickets_in_use() == 0
        a = _check_padded(O, torch, t1, idx, want_t1, f"t1 rep {rep}")
        assert _finite(torch, sc[:, 1:-1, 1:-1, :])
        assert bool(torch.isnan(sc[:, 0]).all()) and bool(torch.isnan(sc[:, :, -1]).all()), "sc's ring was written"
        b = _pick(torch, sc, idx)[:, 1:-1, 1:-1, :]   # (the ring stays NaN)
        assert O.rel_error(b.numpy(), want_sc) < TIGHT
        if first is None:
            first = (a, b)
        assert torch.equal(a, first[0]) and torch.equal(b, first[1])
    del t1, sc
    torch.cuda.empty_cache()
    # the block: out and the workspace (t1)
    need = pkg.lib().wino_basic_block_s2_workspace_bytes_hw(N, Hin, Hin, K)
    assert need == N * Pout
    out = torch.empty(N, H + 2, H + 2, K, device=dev)
    ws = torch.empty(need // 4, device=dev)
    first = None
    for rep in range(2):
        out.fill_(NAN)
        ws.fill_(NAN)
        pkg.basic_block_s2(x, packed, U2, bn2, out=out, workspace=ws)
        torch.cuda.synchronize()
        assert pkg.tickets_in_use() == 0
        g_idx = _check_padded(O, torch, out, idx, want, f"block rep {rep}")
        if first is None:
            first = g_idx
        assert torch.equal(g_idx, first)
    assert (want > 0).mean() > 0.2 and (want_sc < 0).mean() > 0.2
    del x, out, ws


# ------------------------------------------------------------------ the bottleneck blocks
N_BLK, H_BLK = 1400, 56


@pytest.mark.parametrize("form", ["default", "stream_k"])
@pytest.mark.parametrize("stride", [2, 1])
def test_proj_block_beyond_4gib(stride, form, pkg, O, torch_dev, knobs, free_after):
    """proj_block (A_STRIDED at stride 2, the plain 1x1 at stride 1, A_TWO in the tail) at the conv3 entry, 256 -> 128
    -> 512, 1400 images: x is 4.5 GB; out 2.2 GB (stride 2) or 9.0 GB (stride 1); the workspace 1.3 or 4.8 GB."""
    torch, dev = torch_dev
    N, Hin, Cin, Cm, C4 = N_BLK, H_BLK, 256, 128, 512
    H = (Hin - 1) // stride + 1
    Px, Pout, Pt = Hin * Hin * Cin * 4, H * H * C4 * 4, (H + 2) * (H + 2) * Cm * 4
    need = pkg.lib().wino_proj_block_workspace_bytes_hw(N, H, H, Cm)
    assert need == 2 * N * Pt
    _need(torch, N * (Px + Pout) + need)
    _set(knobs, FORMS_1X1[form])
    idx = _images(N, [Px, Pout, Pt])
    rng = np.random.RandomState(121 + stride)
    w1, w2, w3, wp, bn = proj_weights(rng, Cin, Cm, C4)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    bnt = [(t(b), t(s)) for b, s in bn]
    U2 = pkg.filter_transform_f2(t(w2))
    tail = pkg.proj_tail_pack(t(w3), bnt[2], t(wp), bnt[3])
    x = _rand(torch, dev, (N, Hin, Hin, Cin), 122)
    want = LR.bottleneck(_pick(torch, x, idx), w1, bn[0], w2, bn[1], w3, bn[2], wp, bn[3], stride=stride).numpy()
    out = torch.empty(N, H, H, C4, device=dev)
    ws = torch.empty(need // 4, device=dev)
    first = None
    for rep in range(2):
        out.fill_(NAN)
        ws.fill_(NAN)
        pkg.proj_block(x, t(w1), bnt[0], U2, bnt[1], tail, stride, out=out, workspace=ws)
        torch.cuda.synchronize()
        assert pkg.tickets_in_use() == 0
        assert _finite(torch, out)
        t12 = ws.view(2 * N, H + 2, H + 2, Cm)
        assert _finite(torch, t12) and ring_zero(t12)
        g_idx = _pick(torch, out, idx)
        assert O.rel_error(g_idx.numpy(), want) < TIGHT, rep
        if first is None:
            first = g_idx
        assert torch.equal(g_idx, first)
    assert (want > 0).mean() > 0.2
    del x, out, ws


def test_proj_block_v15_beyond_4gib(pkg, O, torch_dev, free_after):
    """proj_block_v15 at the conv3 entry, 256 -> 128 -> 512, 1400 images: x is 4.5 GB, t1 (at the input's 56x56)
    2.4 GB, out 2.2 GB."""
    torch, dev = torch_dev
    N, Hin, Cin, Cm, C4 = N_BLK, H_BLK, 256, 128, 512
    H = (Hin - 1) // 2 + 1
    Px, Pout, Pt1 = Hin * Hin * Cin * 4, H * H * C4 * 4, (Hin + 2) * (Hin + 2) * Cm * 4
    need = pkg.lib().wino_proj_block_v15_workspace_bytes_hw(N, Hin, Hin, Cm)
    _need(torch, N * (Px + Pout) + need)
    idx = _images(N, [Px, Pout, Pt1])
    g = torch.Generator(device="cpu").manual_seed(131)
    r = lambda *s: torch.rand(*s, generator=g) - 0.5
    ref = types.SimpleNamespace(torch=torch)
    ref.w1 = r(Cin, Cm) / np.sqrt(Cin) * 4
    ref.w2 = r(Cm, Cm, 3, 3) / np.sqrt(9 * Cm) * 4
    ref.w3 = r(Cm, C4) / np.sqrt(Cm) * 4
    ref.wp = r(Cin, C4) / np.sqrt(Cin) * 2
    ref.bn = [(r(c), r(c) + 1.0) for c in (Cm, Cm, C4, C4)]
    t = lambda a: a.contiguous().to(dev)
    bnt = [(t(b), t(s)) for b, s in ref.bn]
    taps = pkg.filter_pack_s2(t(ref.w2))
    tail = pkg.proj_tail_pack(t(ref.w3), bnt[2], t(ref.wp), bnt[3])
    x = _rand(torch, dev, (N, Hin, Hin, Cin), 132)
    ref.x = _pick(torch, x, idx)
    want = V15Block.reference(ref)
    out = torch.empty(N, H, H, C4, device=dev)
    ws = torch.empty(need // 4, device=dev)
    first = None
    for rep in range(2):
        out.fill_(NAN)
        ws.fill_(NAN)
        pkg.proj_block_v15(x, t(ref.w1), bnt[0], taps, bnt[1], tail, out=out, workspace=ws)
        torch.cuda.synchronize()
        assert pkg.tickets_in_use() == 0
        assert _finite(torch, out)
        g_idx = _pick(torch, out, idx)
        assert O.rel_error(g_idx.numpy(), want) < TIGHT, rep
        if first is None:
            first = g_idx
        assert torch.equal(g_idx, first)
    assert (want > 0).mean() > 0.2
    del x, out, ws


def test_residual_block_beyond_4gib(pkg, O, torch_dev, free_after):
    """residual_block (wino_residual_block_hw) at 56x56, 256 -> 64 -> 256, 1400 images: x and out are 4.5 GB each,
    the workspace (two padded intermediates) 2.4 GB."""
    torch, dev = torch_dev
    N, H, C4, Cm = N_BLK, H_BLK, 256, 64
    P, Pt = H * H * C4 * 4, (H + 2) * (H + 2) * Cm * 4
    need = pkg.lib().wino_residual_block_workspace_bytes_hw(N, H, H, Cm)
    assert need == 2 * N * Pt
    _need(torch, 2 * N * P + need)
    idx = _images(N, [P, Pt])
    rng = np.random.RandomState(141)
    w1 = ((rng.rand(C4, Cm) - 0.5) / np.sqrt(C4) * 4).astype(np.float32)
    w2 = ((rng.rand(Cm, Cm, 3, 3) - 0.5) / np.sqrt(9 * Cm) * 4).astype(np.float32)
    w3 = ((rng.rand(Cm, C4) - 0.5) / np.sqrt(Cm) * 4).astype(np.float32)
    bn = [((rng.rand(c) - 0.5).astype(np.float32), (rng.rand(c) + 0.5).astype(np.float32)) for c in (Cm, Cm, C4)]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    bnt = [(t(b), t(s)) for b, s in bn]
    U2 = pkg.filter_transform_f2(t(w2))
    x = _rand(torch, dev, (N, H, H, C4), 142)
    want = O.residual_block(_pick(torch, x, idx).numpy(), w1, bn[0], w2, bn[1], w3, bn[2])
    out = torch.empty_like(x)
    ws = torch.empty(need // 4, device=dev)
    first = None
    for rep in range(2):
        out.fill_(NAN)
        ws.fill_(NAN)
        pkg.residual_block(x, t(w1), bnt[0], U2, bnt[1], t(w3), bnt[2], out=out, workspace=ws)
        torch.cuda.synchronize()
        assert pkg.tickets_in_use() == 0
        assert _finite(torch, out)
        t12 = ws.view(2 * N, H + 2, H + 2, Cm)
        assert _finite(torch, t12) and ring_zero(t12)
        g_idx = _pick(torch, out, idx)
        assert O.rel_error(g_idx.numpy(), want) < TIGHT, rep
        if first is None:
            first = g_idx
        assert torch.equal(g_idx, first)
    assert (want > 0).mean() > 0.2
    del x, out, ws


# ------------------------------------------------------------------ the dilated 3x3 (A_DIL) and the concat projection (A_CAT)
@pytest.mark.parametrize("form", sorted(FORMS_1X1))
def test_dilated_3x3_beyond_4gib(form, pkg, O, torch_dev, knobs, free_after):
    """conv3x3_dilated_bn_relu at 62x62, 64 -> 64, dilation 3, 4100 images: one padded image is exactly 1 MiB, so in and
    out are 4.3 GB each and images 2048 and 4096 start on 2^31 and 2^32 bytes -- the per-lane centre offsets, the tap
    offset that wraps modulo 2^32 and the window's clipping at both ends of the tensor, in the planner's form, whole
    tiles and stream-K."""
    torch, dev = torch_dev
    N, H, C, K, d = 4100, 62, 64, 64, 3
    P = (H + 2) * (H + 2) * C * 4
    assert P == 1 << 20 and N * P > 1 << 32
    _need(torch, 2 * N * P)
    _set(knobs, FORMS_1X1[form])
    if form != "default":
        assert pkg.conv3x3_dilated_plan(N, H, H, C, K, d) == (pkg.FORM_TILED if form == "tiled" else pkg.FORM_STREAM_K)
    idx = _images(N, [P])
    assert {2047, 2048, 4095, 4096} <= set(idx)
    g = torch.Generator(device="cpu").manual_seed(161)
    w = (torch.rand(K, C, 3, 3, generator=g) - 0.5) / np.sqrt(9 * C) * 4
    bias, scale = torch.rand(K, generator=g) - 0.5, torch.rand(K, generator=g) + 0.5
    taps, bt, st = pkg.filter_pack_s2(w.to(dev)), bias.to(dev), scale.to(dev)
    x = _padded_rand(torch, dev, N, H, H, C, 162)
    want = dilated_reference(_pick(torch, x, idx).numpy(), w.numpy(), scale.numpy(), bias.numpy(), d, True)
    out = torch.empty(N, H + 2, H + 2, K, device=dev)
    first = None
    for rep in range(2):
        out.fill_(NAN)
        pkg.conv3x3_dilated_bn_relu(x, taps, bt, st, d, relu=True, out=out)
        torch.cuda.synchronize()
        assert pkg.tickets_in_use() == 0
        g_idx = _check_padded(O, torch, out, idx, want, f"rep {rep}")
        if first is None:
            first = g_idx
        assert torch.equal(g_idx, first)
    assert 0.2 < (want > 0).mean() < 0.8
    del x, out


@pytest.mark.parametrize("form", ["default", "stream_k"])
def test_conv1x1_cat_output_beyond_4gib(form, pkg, O, torch_dev, knobs, free_after):
    """conv1x1_cat_bn at 32x32, 2 sources x 32 -> 256, C_PADDED, 4200 images: the sources (0.55 GB each) stay inside
    one descriptor while the padded output is 5.0 GB, past 2^31 at image 1814 and 2^32 at image 3628.  Every image has a
    bias row of its own in [-4, 4): the images on both sides of each boundary must have read theirs."""
    torch, dev = torch_dev
    N, H, S, Cs, Kout = 4200, 32, 2, 32, 256
    Psrc, Pout = H * H * Cs * 4, (H + 2) * (H + 2) * Kout * 4
    assert N * Pout > 1 << 32 and S * N * Psrc < 1 << 32
    _need(torch, S * N * Psrc + N * Pout)
    _set(knobs, FORMS_1X1[form])
    if form != "default":
        assert pkg.conv1x1_cat_plan(N, H, H, S, Cs, Kout) == pkg.FORM_STREAM_K
    idx = _images(N, [Pout])
    g = torch.Generator(device="cpu").manual_seed(171)
    w = (torch.rand(S * Cs, Kout, generator=g) - 0.5) / np.sqrt(S * Cs) * 4
    bias = torch.rand(N, Kout, generator=g) * 8 - 4
    scale = torch.rand(Kout, generator=g) + 0.5
    wt, bt, st = w.to(dev), bias.to(dev), scale.to(dev)
    srcs = _rand(torch, dev, (S, N, H, H, Cs), 172)
    want = cat_reference([_pick(torch, srcs[j], idx).numpy() for j in range(S)], w.numpy(), bias[idx].numpy(),
                         scale.numpy(), True)
    out = torch.empty(N, H + 2, H + 2, Kout, device=dev)
    first = None
    for rep in range(2):
        out.fill_(NAN)
        got = pkg.conv1x1_cat_bn(srcs, wt, bt, st, pkg.RELU | pkg.C_PADDED, out=out)
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        assert pkg.tickets_in_use() == 0
        g_idx = _check_padded(O, torch, out, idx, want, f"rep {rep}")
        if first is None:
            first = g_idx
        assert torch.equal(g_idx, first)
    assert 0.2 < (want > 0).mean() < 0.8
    del srcs, out, got


E_SHAPE, E_ARG = -2, -3   # WINO_E_SHAPE, WINO_E_ARG


@pytest.mark.parametrize("S", [2, 8])
def test_conv1x1_cat_at_the_descriptor_edge(S, pkg, O, torch_dev, free_after):
    """conv1x1_cat_bn (2, 9, 9, S x 64 -> 64) at the largest src_stride the entry point accepts: the tile's one
    descriptor then ends just under 2^32 bytes, and the last source's rows sit at its far end.  The sources lie in one
    4.3 GB allocation that is NaN between them; the whole output is checked.  The next stride is refused as a shape
    error and nothing is launched."""
    torch, dev = torch_dev
    N, H, W, Cs, Kout = 2, 9, 9, 64, 64
    n = N * H * W * Cs
    L = pkg.lib()
    ptr = lambda v: ctypes.c_void_p(v)

    def accepted(stride):
        # host addresses with out placed on the sources: a shape that passes is refused as an overlap, the next check,
        # so no call here launches anything
        rc = L.wino_conv1x1_cat_bn_hw(ptr(1 << 32), stride, ptr(2 << 32), ptr(3 << 32), ptr(4 << 32), ptr(1 << 32),
                                      N, H, W, S, Cs, Kout, pkg.RELU, None)
        assert rc in (E_SHAPE, E_ARG), rc
        return rc == E_ARG

    lo, hi = n // 4, 1 << 30   # in steps of 4 floats
    assert accepted(4 * lo) and not accepted(4 * hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if accepted(4 * mid) else (lo, mid)
    stride = 4 * lo
    # the header's inequality, rows = 112 (unpadded sources)
    assert (112 * Cs + (S - 1) * stride) * 4 < 1 << 32 <= (112 * Cs + (S - 1) * (stride + 4)) * 4
    total = (S - 1) * stride + n
    _need(torch, 4 * total)
    buf = torch.full((total,), NAN, device=dev)
    views = [buf[j * stride: j * stride + n].view(N, H, W, Cs) for j in range(S)]
    g = torch.Generator(device="cpu").manual_seed(181 + S)
    srcs = [torch.rand(N, H, W, Cs, generator=g) - 0.5 for _ in range(S)]
    for v, src in zip(views, srcs):
        v.copy_(src)
    w = (torch.rand(S * Cs, Kout, generator=g) - 0.5) / np.sqrt(S * Cs) * 4
    bias = torch.rand(N, Kout, generator=g) * 8 - 4
    scale = torch.rand(Kout, generator=g) + 0.5
    wt, bt, st = w.to(dev), bias.to(dev), scale.to(dev)
    want = cat_reference([a.numpy() for a in srcs], w.numpy(), bias.numpy(), scale.numpy(), True)
    out = torch.empty(N, H, W, Kout, device=dev)
    first = None
    for rep in range(2):
        out.fill_(NAN)
        pkg.conv1x1_cat_bn(views, wt, bt, st, pkg.RELU, out=out)
        torch.cuda.synchronize()
        assert pkg.tickets_in_use() == 0
        got = out.cpu()
        assert bool(torch.isfinite(got).all()), rep
        assert O.rel_error(got.numpy(), want) < TIGHT, rep
        if first is None:
            first = got
        assert torch.equal(got, first)
    assert 0.2 < (want > 0).mean() < 0.8
    # one float more of stride, and the next multiple of 4: shape errors before anything is launched
    out.fill_(NAN)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for more in (1, 4):
        rc = L.wino_conv1x1_cat_bn_hw(ptr(buf.data_ptr()), stride + more, ptr(wt.data_ptr()), ptr(bt.data_ptr()),
                                      ptr(st.data_ptr()), ptr(out.data_ptr()), N, H, W, S, Cs, Kout, pkg.RELU, stream)
        assert rc == E_SHAPE, (more, rc)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and pkg.tickets_in_use() == 0
    del buf, views, out


# ------------------------------------------------------------------ the grouped 3x3 (64-bit image bases, 32-bit offsets inside)
def _grouped_weights(torch, dev, pkg, C, groups, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    Cg = C // groups
    w = (torch.rand(C, Cg, 3, 3, generator=g) - 0.5) / np.sqrt(9 * Cg) * 4
    bias, scale = torch.rand(C, generator=g) - 0.5, torch.rand(C, generator=g) + 0.5
    return w, bias, scale, pkg.filter_pack_grouped(w.to(dev), groups), bias.to(dev), scale.to(dev)


# (stride, Hin, Win, C, groups, N, tile width): 8-wide tiles at stride 1, 16-wide at stride 2
GROUPED_BATCHES = [(1, 6, 7, 128, 4, 116600, 8), (2, 3, 19, 64, 16, 349600, 16)]


@pytest.mark.parametrize("stride,Hin,Win,C,groups,N,tw", GROUPED_BATCHES, ids=["s1_tw8", "s2_tw16"])
def test_grouped_3x3_batch_beyond_4gib(stride, Hin, Win, C, groups, N, tw, pkg, O, torch_dev, free_after):
    """conv3x3_grouped_bn_relu over a batch of small images: 116600 of 6x7x128 at stride 1 (in and out 4.3 GB each),
    349600 of 3x19x64 at stride 2 (in 9.4 GB, out 4.3 GB) -- input and output both cross 2^31 and 2^32 bytes, at images
    of their own, so every workgroup's 64-bit re-basing of its image is exercised on both tensors."""
    torch, dev = torch_dev
    H, W = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    Pin, Pout = (Hin + 2) * (Win + 2) * C * 4, (H + 2) * (W + 2) * C * 4
    assert N * Pout > 1 << 32 and N * Pin > 1 << 32
    assert pkg.conv3x3_grouped_plan(N, Hin, Win, C, groups, stride)[0] == tw
    _need(torch, N * (Pin + Pout))
    idx = _images(N, [Pin, Pout])
    assert len(idx) >= 8
    w, bias, scale, packed, bt, st = _grouped_weights(torch, dev, pkg, C, groups, 191 + stride)
    x = _padded_rand(torch, dev, N, Hin, Win, C, 192 + stride)
    want = LR.conv3x3(_pick(torch, x, idx), w, (bias, scale), True, stride=stride, groups=groups, padding=0).numpy()
    out = torch.empty(N, H + 2, W + 2, C, device=dev)
    first = None
    for rep in range(2):
        out.fill_(NAN)
        got = pkg.conv3x3_grouped_bn_relu(x, packed, bt, st, groups, stride=stride, relu=True, out=out)
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        g_idx = _check_padded(O, torch, out, idx, want, f"rep {rep}")
        if first is None:
            first = g_idx
        assert torch.equal(g_idx, first)
    assert 0.2 < (want > 0).mean() < 0.8
    del x, out, got


def _bands(rows, width=2):
    """Sorted, merged [lo, hi] ranges of `width` rows on either side of each row of `rows`."""
    out = []
    for lo, hi in sorted((r - width, r + width) for r in rows):
        if out and lo <= out[-1][1] + 1:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return out


def test_grouped_3x3_largest_accepted_image(pkg, O, torch_dev, free_after):
    """conv3x3_grouped_bn_relu on the largest image the layer accepts: 5790 x 5790 x 64 at stride 2, one padded image of
    5792^2 * 64 = 2^31 - 458752 elements (8.6 GB; 5791 is refused, tests/test_grouped_host.py), out 2895 x 2895 (2.1 GB),
    16-wide tiles.  The kernel's 32-bit offsets inside the image run to their limit.  Whole output rows against fp64, each
    band a convolution of a few input rows: the first and the last rows, the rows that read the padded input rows in
    which byte 2^31 and byte 2^32 of the input fall, and the output's own row at byte 2^31 -- the last columns of every
    band (a clipped 16-wide tile) on their own as well."""
    torch, dev = torch_dev
    N, Hin, C, groups, stride = 1, 5790, 64, 16, 2
    H = (Hin - 1) // stride + 1
    in_row, out_row = (Hin + 2) * C * 4, (H + 2) * C * 4
    assert (Hin + 2) ** 2 * C < 1 << 31 <= (Hin + 3) ** 2 * C
    assert (Hin + 2) * in_row > 1 << 32 and (H + 2) * out_row > 1 << 31
    tw, kc, tiles_y, tiles_x = pkg.conv3x3_grouped_plan(N, Hin, Hin, C, groups, stride)
    assert (tw, kc) == (16, 16) and tiles_x >= 2 and H % tw
    _need(torch, (Hin + 2) * in_row + (H + 2) * out_row)
    # output rows: the ends; those whose three padded input rows 2 oy .. 2 oy + 2 hold a byte boundary of the input; the
    # one at the output's byte 2^31 (padded output row r is output row r - 1)
    rows = {0, H - 1}
    for b in (1 << 31, 1 << 32):
        rows.add(min(H - 1, (b // in_row) // 2))
    rows.add(min(H - 1, max(0, (1 << 31) // out_row - 1)))
    bands = [(max(0, lo), min(H - 1, hi)) for lo, hi in _bands(rows)]
    assert 3 <= len(bands) <= 5 and sum(hi - lo + 1 for lo, hi in bands) <= 25
    w, bias, scale, packed, bt, st = _grouped_weights(torch, dev, pkg, C, groups, 201)
    x = _padded_rand(torch, dev, N, Hin, Hin, C, 202)
    # (padding=0: the zero ring is the padding left and right, and a band brings the rows above and below it along)
    want = [LR.conv3x3(x[:, 2 * lo:2 * hi + 3].cpu(), w, (bias, scale), True, stride=stride, groups=groups, padding=0).numpy()
            for lo, hi in bands]
    out = torch.empty(N, H + 2, H + 2, C, device=dev)
    first = None
    for rep in range(2):
        out.fill_(NAN)
        pkg.conv3x3_grouped_bn_relu(x, packed, bt, st, groups, stride=stride, relu=True, out=out)
        torch.cuda.synchronize()
        assert _finite(torch, out) and ring_zero(out), rep
        got = [out[:, lo + 1:hi + 2, 1:-1, :].cpu() for lo, hi in bands]
        for (lo, hi), g_, w_ in zip(bands, got, want):
            assert g_.shape == w_.shape, (lo, hi)
            assert O.rel_error(g_.numpy(), w_) < TIGHT, (rep, lo, hi)
            assert O.rel_error(g_.numpy()[:, :, -tw:], w_[:, :, -tw:]) < TIGHT, (rep, lo, hi, "last columns")
        if first is None:
            first = got
        assert all(torch.equal(a, b) for a, b in zip(got, first))
    assert all(0.2 < (w_ > 0).mean() < 0.8 for w_ in want)
    del x, out


# ------------------------------------------------------------------ the largest filter matrix the 3x3 accepts
def test_3x3_largest_accepted_filter(pkg, O, torch_dev, knobs, free_after):
    """C = 8192, K = 8128: U is 3.97 GiB (the throughput kernel reads it through one descriptor, so its high offsets
    are those of the last channel chunks and out-channel blocks), w 2.2 GiB.  One 4x4 image keeps the fp64 reference
    cheap; all K output channels are checked, in both kernels."""
    torch, dev = torch_dev
    N, H, C, K = 1, 4, 8192, 8128
    assert 16 * C * K * 4 < (1 << 32) <= 16 * C * (K + 64) * 4
    _need(torch, (9 + 16) * C * K * 4)
    g = torch.Generator(device=dev).manual_seed(151)
    w = (torch.rand(K, C, 3, 3, device=dev, generator=g) - 0.5) / np.sqrt(9 * C) * 4
    bias = torch.rand(K, device=dev, generator=g) - 0.5
    scale = torch.rand(K, device=dev, generator=g) + 0.5
    x = _padded_rand(torch, dev, N, H, H, C, 152)
    U = pkg.filter_transform_f2(w)
    torch.cuda.synchronize()
    w_cpu = w.cpu().numpy()
    del w
    torch.cuda.empty_cache()
    want = O.conv3x3_bn_relu_direct(x.cpu().numpy(), w_cpu, scale.cpu().numpy(), bias.cpu().numpy())
    del w_cpu
    out = torch.empty(N, H + 2, H + 2, K, device=dev)
    for algo in ("big", "small"):
        knobs.set("WINO_3X3_ALGO", algo)
        assert pkg.small_plan_3x3(N, C, K, H=H, W=H)[0] == (algo == "small")
        first = None
        for rep in range(2):
            out.fill_(NAN)
            pkg.conv3x3_bn_relu(x, U, bias, scale, relu=True, out=out)
            torch.cuda.synchronize()
            assert pkg.tickets_in_use() == 0
            got = out.cpu()
            assert np.isfinite(got.numpy()).all(), algo
            assert (got[:, 0] == 0).all() and (got[:, -1] == 0).all() and (got[:, :, 0] == 0).all() \
                and (got[:, :, -1] == 0).all(), algo
            assert O.rel_error(got.numpy(), want) < TIGHT, algo
            # the last out-channel block alone: its filters sit at U's highest offsets
            assert O.rel_error(got.numpy()[..., -64:], want[..., -64:]) < TIGHT, algo
            if first is None:
                first = got
            assert torch.equal(got, first), algo
    assert 0.2 < (want[:, 1:-1, 1:-1, :] > 0).mean() < 0.8
    del x, U, out


# ------------------------------------------------------------------ one FPN level
def test_fpn_level_beyond_4gib(pkg, O, torch_dev, free_after):
    """fpn_level, 1025 images of 126 x 126, Cin = 32 -> Cf = 64, with the top-down read: inner and P are 4 MiB per image,
    4.3 GB each, so image 1024 starts at byte 2^32 of both; the lateral writes inner past it and reads top at
    (y >> 1, x >> 1) of the same image, the 3x3 reads inner and writes P past it.  c (2.1 GB, unpadded) crosses 2^31
    bytes.  top, [1025][65 + 2][65 + 2][64], stays below 2^31 bytes: pushing it past would take an inner and a P of
    17 GB each, and the kernel forms the coarse row's address (up2_row) in long.  On the device: both rings exactly 0,
    every value finite; images 0, 512 and 1024 and those around 2^31 bytes of inner against the fp64 chain at TIGHT."""
    torch, dev = torch_dev
    N, H, W, Cin, Cf = 1025, 126, 126, 32, 64
    P = (H + 2) * (W + 2) * Cf * 4
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    top_bytes = N * (Hc + 2) * (Wc + 2) * Cf * 4
    assert P == 4 << 20 and 1024 * P == 1 << 32 and top_bytes < 1 << 31
    _need(torch, 2 * N * P + N * H * W * Cin * 4 + top_bytes)
    idx = sorted({0, 512, 1024} | set(_images(N, [P])))
    g = torch.Generator(device="cpu").manual_seed(91)
    wl = (torch.rand(Cf, Cin, 1, 1, generator=g) - 0.5) / np.sqrt(Cin) * 4
    wo = (torch.rand(Cf, Cf, 3, 3, generator=g) - 0.5) / np.sqrt(9 * Cf) * 4
    bl, bo = torch.rand(Cf, generator=g) - 0.5, torch.rand(Cf, generator=g) - 0.5
    c = _rand(torch, dev, (N, H, W, Cin), 92)
    top = _rand(torch, dev, (N, Hc + 2, Wc + 2, Cf), 93)
    for ring in (top[:, 0], top[:, -1], top[:, :, 0], top[:, :, -1]):       # the coarse map's ring is not read
        ring.fill_(NAN)
    want_inner, want_P = level_reference(torch, _pick(torch, c, idx), wl, bl, wo, bo,
                                         _pick(torch, top, idx)[:, 1:-1, 1:-1, :])
    wld, U = wl.reshape(Cf, Cin).t().contiguous().to(dev), pkg.filter_transform_f2(wo.to(dev))
    bld, bod, ones = bl.to(dev), bo.to(dev), torch.ones(Cf, device=dev)
    inner = torch.empty((N, H + 2, W + 2, Cf), device=dev)
    out = torch.empty_like(inner)
    first = None
    for rep in range(2):
        inner.fill_(NAN)
        out.fill_(NAN)
        got = pkg.fpn_level(c, wld, bld, U, bod, top=top, ones=ones, inner=inner, out=out)
        assert got[0].data_ptr() == inner.data_ptr() and got[1].data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        assert pkg.tickets_in_use() == 0
        picked = (_check_padded(O, torch, inner, idx, want_inner.numpy(), f"inner, rep {rep}"),
                  _check_padded(O, torch, out, idx, want_P.numpy(), f"P, rep {rep}"))
        if first is None:
            first = picked
        assert torch.equal(picked[0], first[0]) and torch.equal(picked[1], first[1])
    errs = [O.rel_error(first[k][:, 1:-1, 1:-1, :].numpy(), w.numpy()) for k, w in enumerate((want_inner, want_P))]
    print(f"fpn_level past 4 GiB, images {idx}: inner {errs[0]:.2e} P {errs[1]:.2e}")
    del c, top, inner, out, got


# ------------------------------------------------------------------ batched NMS at its limits, box decode past 4 GiB
def _assert_nms(got, want, tag):
    for name, g, w in zip(("count", "keep", "rois"), (got[1], got[0], got[2]), (want[1], want[0], want[2])):
        if g is not None:
            assert np.array_equal(g.view(np.int32), w.view(np.int32)), (tag, name)


@pytest.mark.parametrize("R", bc.NMS_LIMIT_R)
def test_nms_full_width_segments(R, pkg, torch_dev, free_after):
    """ceil(R / 64) equal to the scan kernel's thread count along the words (R = 4096 and 16384: W = 64 and 256), and
    the largest segment the library takes (R = 32768, W = 512, a 128 MiB bit matrix): exactly the fp64 reference, all of
    it and cut at half the kept count."""
    torch, dev = torch_dev
    _need(torch, 2 * (pkg.nms_workspace_bytes(1, R) + (256 << 20)))
    c = bc.nms_case(R, 1)
    for use_groups, use_scores in c.variants:
        p = dict(c.PARAMS)
        if not use_scores:
            p.pop("score_thresh")
        got = run_nms(pkg, dev, c.boxes, c.scores if use_scores else None, c.groups if use_groups else None, R, p,
                      aligns=(256,), tag=f"full width groups={use_groups}")
        _assert_nms(got, c.expected(use_groups, use_scores), (R, use_groups, use_scores))
    count = int(c.expected()[1][0])
    got = run_nms(pkg, dev, c.boxes, c.scores, c.groups, count // 2, c.PARAMS, aligns=(16,), tag="full width, cut")
    _assert_nms(got, c.expected(True, True, count // 2), (R, "cut"))
    print(f"R={R}: kept {count}, redrawn {c.redrawn} of {c.drawn}")


def test_nms_workspace_beyond_4gib(pkg, torch_dev, free_after):
    """2100 segments of 4100 boxes: the bit matrix is 2100 x 4100 x 65 words, 4.48 GB, NaN-filled.  The segments repeat
    the three of nms_case(4100, 3) cyclically, so a segment that read a wrapped address would see another case's bits.
    Every segment's keep, count and rois equal its source's reference, rois column 0 its own index; the segments on
    both sides of byte 2^31 and byte 2^32 of the workspace are checked by name."""
    torch, dev = torch_dev
    S, R = 2100, 4100
    per = R * 65 * 8
    assert pkg.nms_workspace_bytes(S, R) == S * per > (1 << 32) + (1 << 27)
    _need(torch, S * per + S * R * (16 + 4 + 4 + 4 + 20) * 2 + GIB)
    c = bc.nms_case(R, 3)
    assert len({c.boxes[k].tobytes() for k in range(3)}) == 3
    idx = np.arange(S) % 3
    src = c.expected()
    assert len({tuple(src[0][k].tolist()) for k in range(3)}) == 3
    want = bc.tile_segments(*src[:3], S)
    got = run_nms(pkg, dev, c.boxes[idx], c.scores[idx], c.groups[idx], R, c.PARAMS, aligns=(256,), tag="workspace > 4 GiB")
    named = sorted({0, S - 1} | {b // per + d for b in (1 << 31, 1 << 32) for d in (-1, 0, 1)})
    assert named == [0, 1006, 1007, 1008, 2013, 2014, 2015, 2099]
    for s in named:
        k = int(want[1][s])
        assert got[1][s] == k == src[1][s % 3] and np.array_equal(got[0][s], src[0][s % 3]), s
        assert (got[2][s, :k, 0] == s).all() and np.array_equal(got[2][s, :, 1:], src[2][s % 3][:, 1:]), s
    _assert_nms(got, want, "every segment")


def test_nms_many_segments(pkg, torch_dev, free_after):
    """S = 70001 segments of 65 boxes (two words per row), the seven of nms_case(65, 7) repeated."""
    torch, dev = torch_dev
    S, R = 70001, 65
    _need(torch, GIB)
    c = bc.nms_case(R, 7)
    idx = np.arange(S) % 7
    want = bc.tile_segments(*c.expected()[:3], S)
    got = run_nms(pkg, dev, c.boxes[idx], c.scores[idx], c.groups[idx], R, c.PARAMS, aligns=(256,), tag="70001 segments")
    _assert_nms(got, want, S)
    assert got[2][S - 1, 0, 0] == S - 1


@pytest.mark.parametrize("S,rois", [((1 << 22) - 1, True), (1 << 22, True), ((1 << 24) - 1, False)])
def test_nms_one_box_segments_up_to_the_limit(S, rois, pkg, torch_dev, free_after):
    """R = 1, max_out = 1 on both sides of S = 2^22 (the scan kernel has one workgroup of 1024 threads per segment, and
    a launch takes fewer than 2^32 threads along x, so the library cuts the scan into launches of at most 2^22 - 1
    segments) and at the largest S the library takes, 2^24 - 1.  One launch each, into NaN-filled outputs."""
    torch, dev = torch_dev
    _need(torch, 2 * S * (16 + 4 + 8 + 4 + 4 + 20) + GIB)
    boxes, scores, keep, count, src_rois = bc.one_box_sources()
    idx = np.arange(S) % boxes.shape[0]
    want = bc.tile_segments(keep, count, src_rois, S)
    got = run_nms(pkg, dev, boxes[idx], scores[idx], None, 1, bc.ONE_BOX_PARAMS, rois=rois, aligns=(256,), repeats=1,
                  tag=f"S={S}")
    _assert_nms(got, want, S)
    last = max(s for s in range(S - 300, S) if want[1][s])
    assert got[0][last, 0] == 0 and (not rois or got[2][last, 0, 0] == np.float32(last))


DECODE_HEAD = dict(N=3, rpi=699051, A=3, ld=520, delta_col=520 - 12, score_col=5, weights=(10.0, 10.0, 5.0, 5.0))


def _decode_rows(torch, head, anchors, image_hw, rows, d):
    """fp64 boxes [len(rows)][A][4] of the picked rows of a boxes-mode head, image by image."""
    out = np.zeros((len(rows), d["A"], 4))
    h, a = _pick(torch, head, rows).numpy(), _pick(torch, anchors, rows).numpy()
    for n in range(d["N"]):
        m = np.array([r // d["rpi"] == n for r in rows])
        if m.any():
            out[m] = bc.decode_reference(h[m], a[m], image_hw[n:n + 1], d["A"], d["weights"], None,
                                         d["delta_col"]).reshape(-1, d["A"], 4)
    return out, h


def test_box_decode_head_beyond_4gib(pkg, torch_dev, free_after):
    """Boxes mode on a head of 3 x 699051 rows of 520 floats, 4.36 GB, deltas in the row's last 12 columns and scores at
    column 5: the rows on both sides of byte 2^31 and byte 2^32 of the head, the first and last row of every image and
    1000 seeded rows against fp64 at TIGHT; the whole output finite; a second launch gives the same bits."""
    torch, dev = torch_dev
    d = DECODE_HEAD
    N, rpi, A, ld = d["N"], d["rpi"], d["A"], d["ld"]
    rows = N * rpi
    assert rows * ld * 4 > (1 << 32) + (1 << 25)
    _need(torch, rows * ld * 4 + 2 * rows * A * 20 + rows * 16)
    head = _rand(torch, dev, (rows, ld), 301).mul_(4.0)                   # deltas / weights: +-0.2 and +-0.4
    g = torch.Generator(device=dev).manual_seed(302)
    anchors = torch.rand(rows, 4, device=dev, generator=g)
    anchors[:, 0].mul_(600.0), anchors[:, 1].mul_(400.0)
    anchors[:, 2] = anchors[:, 0] + 1.0 + 120.0 * anchors[:, 2]
    anchors[:, 3] = anchors[:, 1] + 1.0 + 120.0 * anchors[:, 3]
    image_hw = np.array([[420.0, 610.5], [333.25, 700.0], [512.0, 512.0]], dtype=np.float32)
    hw = torch.from_numpy(image_hw).to(dev)
    pick = {0, rows - 1} | {n * rpi + e for n in range(N) for e in (0, rpi - 1)}
    pick |= {b // (4 * ld) + e for b in (1 << 31, 1 << 32) for e in (-1, 0, 1)}
    pick |= set(np.random.RandomState(303).randint(0, rows, 1000).tolist())
    pick = sorted(pick)
    want, picked_head = _decode_rows(torch, head, anchors, image_hw, pick, d)
    out_b = torch.empty(N, rpi * A, 4, device=dev)
    out_s = torch.empty(N, rpi * A, device=dev)
    first = None
    for rep in range(2):
        out_b.fill_(NAN), out_s.fill_(NAN)
        pkg.box_decode(head, anchors, hw, A, d["weights"], None, d["delta_col"], d["score_col"], out_b, out_s)
        torch.cuda.synchronize()
        assert _finite(torch, out_b) and _finite(torch, out_s)
        got_b = _pick(torch, out_b.view(rows, A, 4), pick).numpy()
        got_s = _pick(torch, out_s.view(rows, A), pick).numpy()
        err = bc.rel_err(got_b, want)
        assert err < TIGHT, (rep, err)
        assert np.array_equal(got_s.view(np.int32), picked_head[:, d["score_col"]:d["score_col"] + A].view(np.int32))
        if first is None:
            first = (out_b.clone(), out_s.clone())
        assert torch.equal(out_b.view(torch.int32), first[0].view(torch.int32))
        assert torch.equal(out_s.view(torch.int32), first[1].view(torch.int32))
    print(f"box_decode, head past 4 GiB, {len(pick)} rows: {err:.2e}")
    del head, anchors, out_b, out_s, first


def _count_not_nan(torch, t):
    flat, total = t.reshape(-1), 0
    for i in range(0, flat.numel(), 1 << 28):
        total += int((~torch.isnan(flat[i:i + (1 << 28)])).sum())
    return total


def test_box_decode_output_beyond_4gib(pkg, torch_dev, free_after):
    """out_boxes [2][2^28 + 4096][4], 8.6 GB, and out_scores to match, NaN-filled; a small grid-mode head written at
    out_offset = 2^28 - 100: image 0's slice of the boxes straddles byte 2^32, image 1's slice lies beyond it (and, for
    the scores, beyond byte 2^31).  Both slices at TIGHT and the scores bit for bit; counted on the device, the elements
    that are not NaN are exactly the two slices'."""
    torch, dev = torch_dev
    total, off = (1 << 28) + 4096, (1 << 28) - 100
    _need(torch, 2 * total * 20 + GIB)
    c = bc.decode_case(7)                                                  # 13 x 21, A = 3, N = 3 -> the first two images
    N, per = 2, c.rpi * c.A
    assert off * 16 < (1 << 32) < (off + per) * 16 and off + per <= total
    head_np, hw_np = c.head[:N * c.rpi], c.image_hw[:N]
    want = bc.decode_reference(head_np, c.anchors, hw_np, c.A, c.weights, c.grid, c.delta_col)
    head, anc, hw = (torch.from_numpy(a).to(dev) for a in (head_np, c.anchors, hw_np))
    out_b = torch.empty(N, total, 4, device=dev)
    out_s = torch.empty(N, total, device=dev)
    for rep in range(2):
        out_b.fill_(NAN), out_s.fill_(NAN)
        pkg.box_decode(head, anc, hw, c.A, c.weights, c.grid, c.delta_col, c.score_col, out_b, out_s, off)
        torch.cuda.synchronize()
        got_b, got_s = out_b[:, off:off + per].cpu().numpy(), out_s[:, off:off + per].cpu().numpy()
        err = bc.rel_err(got_b, want)
        assert err < TIGHT, (rep, err)
        assert np.array_equal(got_s.view(np.int32), head_np[:, :c.A].reshape(N, per).view(np.int32))
        assert _count_not_nan(torch, out_b) == N * per * 4 and _count_not_nan(torch, out_s) == N * per
    print(f"box_decode, output past 4 GiB: {err:.2e}")
    del out_b, out_s


# ------------------------------------------------------------------ the image transform at its accepted limits
@pytest.mark.parametrize("axis", ["rows", "columns"])
def test_transform_at_the_coordinate_bound(axis, pkg, torch_dev, free_after):
    """C = 1, a source of 32767 x 1 resized to 32768 x 1 (and the transposed one): 2 ho h = 2^31 - 65536, the last pair the
    entry point accepts (tests/test_transform_host.py shows 32768 refused), and coord()'s (2 d + 1) in - out reaches
    2147352577 in int.  The whole output against the fp64 reference, whose coordinates are int64."""
    torch, dev = torch_dev
    h, ho = 32767, 32768
    assert 2 * ho * h == (1 << 31) - 65536 and (2 * (ho - 1) + 1) * h - ho == 2147352577
    shape, size = ((h, 1), (ho, 1)) if axis == "rows" else ((1, h), (1, ho))
    imgs = tc.images([shape], 1, seed=41)
    mean, std = tc.mean_std(1)
    want = tc.transform_reference(imgs, [size], *size, mean, std)
    out = torch.full((1, 1, *size), NAN, device=dev)
    pkg.image_transform([imgs[0].to(dev)], [size], *size, mean, std, out=out)
    torch.cuda.synchronize()
    tc.check(out.cpu().numpy(), want, [size], f"coordinate bound, {axis}")


def _count(torch, flat, pred):
    return sum(int(pred(flat[i:i + (1 << 28)]).sum()) for i in range(0, flat.numel(), 1 << 28))


def test_transform_output_beyond_4gib(pkg, torch_dev, free_after):
    """out [5][4][8192][8192], 5.4 GB prefilled with NaN, five small sources resized to a 16 x 16 corner: counted on the
    device no NaN is left and every element outside the corners is bitwise +0; each image's corner is bitwise what a call
    with that image alone writes, and the fp64 reference's at the transform's own bar."""
    torch, dev = torch_dev
    N, C, Hb, Wb, size = 5, 4, 8192, 8192, (16, 16)
    assert N * C * Hb * Wb * 4 == 5 << 30 and 4 * C * Hb * Wb * 4 == 1 << 32      # image 4 starts at byte 2^32
    _need(torch, (N + 1) * C * Hb * Wb * 4)
    shapes = [(5, 7), (9, 4), (16, 16), (3, 3), (1, 20)]
    imgs = tc.images(shapes, C, seed=42)
    mean, std = tc.mean_std(C)
    d = [t.to(dev) for t in imgs]
    out = torch.full((N, C, Hb, Wb), NAN, device=dev)
    pkg.image_transform(d, [size] * N, Hb, Wb, mean, std, out=out)
    torch.cuda.synchronize()
    flat = out.view(-1)
    assert _count(torch, flat, torch.isnan) == 0
    corners = out[:, :, :16, :16].contiguous()
    nonzero = lambda t: t.view(torch.int32) != 0
    assert _count(torch, flat, nonzero) == int(nonzero(corners).sum()), "an element outside the corners is not +0"
    assert int(nonzero(corners).sum()) > N * C * 250
    tc.check(corners.cpu().numpy(), tc.transform_reference(imgs, [size] * N, *size, mean, std), [size] * N, "corners")
    one = torch.empty((1, C, Hb, Wb), device=dev)
    for i in range(N):
        one.fill_(NAN)
        pkg.image_transform(d[i:i + 1], [size], Hb, Wb, mean, std, out=one)
        assert torch.equal(one[0, :, :16, :16].contiguous().view(torch.int32), corners[i].view(torch.int32)), i
    del out, one, flat


def test_transform_largest_source_image(pkg, torch_dev, free_after):
    """One float32 source of 4 x 32768 x 16383, 8 GiB and the largest the entry point accepts (one column more is refused,
    tests/test_transform_host.py), resized to 8 x 8: the taps lie up to 2^31 - 2^15 elements into the image.  The
    reference gathers the 4 * 64 * 4 taps with torch indexing on the device and interpolates them in fp64."""
    torch, dev = torch_dev
    C, h, w, size = 4, 32768, 16383, (8, 8)
    assert C * h * w < 1 << 31 <= C * h * (w + 1)
    _need(torch, C * h * w * 4 + GIB)
    src = _rand(torch, dev, (C, h, w), 43).add_(0.5)
    mean, std = tc.mean_std(C)
    out = torch.full((1, C, *size), NAN, device=dev)
    pkg.image_transform([src], [size], *size, mean, std, out=out)
    torch.cuda.synchronize()
    y0, y1, ly = tc.axis_coords(h, size[0])
    x0, x1, lx = tc.axis_coords(w, size[1])
    assert (C - 1) * h * w + int(y1.max()) * w + int(x1.max()) > (1 << 31) - (1 << 29)      # the farthest tap
    t = lambda a: torch.as_tensor(a, device=dev)
    m = torch.tensor(mean, dtype=torch.float64, device=dev)[:, None, None]
    s = torch.tensor(std, dtype=torch.float64, device=dev)[:, None, None]
    tap = lambda ys, xs: (src[:, t(ys)][:, :, t(xs)].double() - m) / s
    ly_t, lx_t = t(ly)[:, None], t(lx)[None, :]
    top = (1 - lx_t) * tap(y0, x0) + lx_t * tap(y0, x1)
    bot = (1 - lx_t) * tap(y1, x0) + lx_t * tap(y1, x1)
    want = ((1 - ly_t) * top + ly_t * bot).cpu().numpy()[None]
    tc.check(out.cpu().numpy(), want, [size], "largest source")
    del src


# ------------------------------------------------------------------ the segmented select at its accepted limits
def test_select_scores_beyond_2gi_elements(pkg, torch_dev, free_after):
    """N = 3 at image_stride = 2^30: image 2 starts at element 2^31 of the scores (12 GiB, torch.empty) and byte 2^35 of
    the boxes, which have a longer stride of their own.  A long part and a short one sit at the end of every row; only
    those ranges are initialised.  The reference is numpy over them; the box payload names its image and its place."""
    torch, dev = torch_dev
    N, stride, bstride = 3, 1 << 30, (1 << 30) + 64
    n, off, k = [19000, 500], [stride - 20000, stride - 500], [1000, 600]
    _need(torch, N * stride * 4 + N * bstride * 16 + GIB)
    scores = torch.empty((N, stride), device=dev)
    boxes = torch.empty((N, bstride, 4), device=dev)
    x = [[sc.case(name, N, n_p, seed=44 + p)[i] for p, (name, n_p) in enumerate(zip(("ties", "distinct"), n))] for i in range(N)]
    b = [[np.stack([np.full(n_p, i), np.arange(n_p), -np.arange(n_p), np.full(n_p, 0.5 + p)], axis=1).astype(np.float32)
          for p, n_p in enumerate(n)] for i in range(N)]
    for i in range(N):
        for p in range(2):
            scores[i, off[p]:off[p] + n[p]] = torch.from_numpy(x[i][p].copy()).to(dev)
            boxes[i, off[p]:off[p] + n[p]] = torch.from_numpy(b[i][p]).to(dev)
    ksum = sum(k)
    idx = torch.full((N, ksum), -7, dtype=torch.int32, device=dev)
    vals, ob = torch.full((N, ksum), NAN, device=dev), torch.full((N, ksum, 4), NAN, device=dev)
    count = torch.full((N, 2), -7, dtype=torch.int32, device=dev)
    ws = torch.full((pkg.select_workspace_bytes(N, n, k) // 4,), NAN, device=dev)
    for thresh in (None, 0.25):
        pkg.select_topk(scores, k, n, off, thresh, boxes, idx, vals, count, ob, ws)
        torch.cuda.synchronize()
        got = [t.cpu().numpy() for t in (idx, vals, count, ob)]
        for i in range(N):
            base = 0
            for p in range(2):
                order = sc.topk_order(x[i][p], k[p], thresh)
                c = len(order)
                assert got[2][i, p] == c and (p == 0 or c < k[p])
                assert np.array_equal(got[0][i, base:base + c], order + off[p]) and (got[0][i, base + c:base + k[p]] == -1).all()
                assert np.array_equal(got[1][i, base:base + c].view(np.int32), x[i][p][order].view(np.int32))
                assert np.array_equal(got[3][i, base:base + c].view(np.int32), b[i][p][order].view(np.int32)), (i, p)
                assert not got[1][i, base + c:base + k[p]].any() and not got[3][i, base + c:base + k[p]].any()
                base += k[p]
    del scores, boxes


LONGEST_SEGMENT = (1 << 31) - 1      # the longest the entry point accepts


def longest_segment(pkg, torch, dev, n):
    """One segment of n scores, k = 8192: zeros written on the device and 300 planted distinct positive values, among
    them index 0, index n - 1 and both sides of several chunk boundaries.  The result is known by construction: the
    planted ones by value, then the lowest indices that were not planted (equal scores go to the lower index).
    Returns the seconds the call took."""
    import time
    k, chunk = 8192, 2048
    rng = np.random.RandomState(45)
    chunks = (n + chunk - 1) // chunk
    at = {0, n - 1, n - 2}
    for c in (1, 2, 3, 255, 256, chunks // 2, chunks - 1):
        at |= {c * chunk - 1, c * chunk}
    at |= {int(v) for v in rng.randint(0, 3000, 40)} | {int(v) for v in rng.randint(0, n, 250)}
    at = np.array(sorted(at), dtype=np.int64)
    assert 250 < len(at) < 320 and at[0] == 0 and at[-1] == n - 1
    values = (1.0 + rng.permutation(len(at))).astype(np.float32)
    scores = torch.zeros((1, n), device=dev)
    scores[0, torch.from_numpy(at).to(dev)] = torch.from_numpy(values).to(dev)
    idx = torch.full((1, k), -7, dtype=torch.int32, device=dev)
    vals = torch.full((1, k), NAN, device=dev)
    count = torch.full((1, 1), -7, dtype=torch.int32, device=dev)
    ws = torch.full((pkg.select_workspace_bytes(1, n, k) // 4,), NAN, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pkg.select_topk(scores, k, out_idx=idx, out_vals=vals, out_count=count, workspace=ws)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    by_value = at[np.argsort(-values, kind="stable")]
    rest = np.setdiff1d(np.arange(k + len(at)), at)[:k - len(at)]
    assert count.cpu().tolist() == [[k]]
    assert np.array_equal(idx.cpu().numpy()[0], np.concatenate([by_value, rest]))
    want_vals = np.concatenate([np.sort(values)[::-1], np.zeros(k - len(at), np.float32)])
    assert np.array_equal(vals.cpu().numpy()[0].view(np.int32), want_vals.view(np.int32))
    del scores
    return seconds


@pytest.mark.parametrize("n", [1 << 30, LONGEST_SEGMENT], ids=["2^30", "2^31-1"])
def test_select_longest_segment(n, pkg, torch_dev, free_after):
    """The longest segment the entry point accepts, and half of it: the gather's scan over the earlier chunks' tie counts
    is quadratic in the chunks, so the second run does four times the first one's scan (DESIGN.md section 3.2p has the
    measured times)."""
    torch, dev = torch_dev
    _need(torch, n * 4 + GIB)
    seconds = longest_segment(pkg, torch, dev, n)
    print(f"select_topk, one segment of {n} scores, k = 8192: {seconds:.3f} s")


@pytest.mark.parametrize("N,parts", [(65535, 1), (13107, 5)])
def test_select_most_segments(N, parts, pkg, torch_dev, free_after):
    """N parts = 65535, the most the entry point takes (the grid's y carries the segment): four distinct scores per
    segment, k = 2.  The rows are a rotation by the segment's number, so a segment that read another's scores shows."""
    torch, dev = torch_dev
    S = N * parts
    assert S == 65535
    base = np.array([0.5, -2.0, 3.0, 1.0], dtype=np.float32)
    x = np.stack([np.roll(base, s % 4) + np.float32(s % 7) for s in range(S)]).reshape(N, parts * 4)
    off = [4 * p for p in range(parts)]
    idx, vals, count = pkg.select_topk(torch.from_numpy(x).to(dev), [2] * parts, [4] * parts, off)
    torch.cuda.synchronize()
    seg = x.reshape(N, parts, 4)
    order = np.argsort(-seg, axis=2, kind="stable")[:, :, :2]
    assert (count.cpu().numpy() == 2).all()
    assert np.array_equal(idx.cpu().numpy().reshape(N, parts, 2), order + np.array(off)[None, :, None])
    assert np.array_equal(vals.cpu().numpy().reshape(N, parts, 2), np.take_along_axis(seg, order, axis=2))
