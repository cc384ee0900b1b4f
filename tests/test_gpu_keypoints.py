"""GPU tests of wino_keypoints_hw / heatmaps_to_keypoints on the guarded arena, at both placements of guarded.ALIGNS, against
the fp64 reference of tests/keypoint_cases.py (itself held to torchvision by tests/test_keypoint_host.py): every named box
class in both layouts (positions exact where the margin rule holds, x and y bit-equal to the float32 restatement, scores
within cases.TIGHT of the plane's range), the exact cases bit for bit, DECONV_ROWS against PLANES on the torch-composed
planes, the special rows, a NaN map element, R = 0, every refusal of the header, a seeded sweep of random layouts in the
tolerance form, a graph, and one `maps` past 2^31 elements."""
import functools

import numpy as np
import pytest
import torch

import guarded
import keypoint_cases as kc
from cases import TIGHT
from gpu_support import torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu
MS = (4, 8, 28, 56)
KS = (1, 3, 17)
NAN = float("nan")
INF = float("inf")
F = torch.nn.functional


def pad64(n):
    return -(-n // 64) * 64


def run_kp(pkg, dev, maps, rois, layout="planes", K=None, M=None, bias=None, max_side=kc.MAX_SIDE, aligns=guarded.ALIGNS,
           tag=""):
    """The launch on numpy operands, on the guarded arena at each of `aligns`, twice into NaN-filled outputs; every run is
    bitwise the first.  Returns (keypoints [R][K][3], scores [R][K]) as numpy."""
    R = rois.shape[0]
    K = maps.shape[1] if layout == "planes" else K
    first = None
    for align in aligns:
        arena = guarded.Arena(torch, dev, align)
        mp = arena.input(torch.from_numpy(np.ascontiguousarray(maps)), name="maps")
        ro = arena.input(torch.from_numpy(np.ascontiguousarray(rois)), name="rois")
        b = None if bias is None else arena.input(torch.from_numpy(bias), name="bias")
        kp, sc = arena.output(R, K, 3, name="keypoints"), arena.output(R, K, name="scores")
        for _ in range(2):
            kp.fill_(NAN), sc.fill_(NAN)
            got = pkg.heatmaps_to_keypoints(mp, ro, K=K, M=M, layout=layout, bias=b, max_side=max_side, out=kp,
                                            scores_out=sc)
            assert got[0] is kp and got[1] is sc
            arena.check(f"heatmaps_to_keypoints {tag} {layout} R={R} K={K} M={M} align={align}")
            cur = (kp.cpu().numpy(), sc.cpu().numpy())
            if first is None:
                first = cur
            for x, y in zip(cur, first):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"{tag}: not bitwise reproducible"
    return first


@functools.lru_cache(maxsize=None)
def class_case(M, K):
    """The fourteen named classes at (M, K), computed once: planes under the margin rule, the DECONV_ROWS parts, and both
    references."""
    rois, names = kc.class_rois(M)
    planes, _ = kc.draw_planes(rois, K, M, seed=100 * M + K)
    want = kc.reference(planes, rois)
    P = M // 4
    parts, bias, _, kept = kc.draw_deconv_parts(rois, K, P, seed=100 * M + K + 1)
    composed = kc.compose_planes(parts.reshape(-1, 16 * K), bias, len(rois), K, P)
    return dict(rois=rois, names=names, planes=planes, want=want, parts=parts, bias=bias, kept=kept, composed=composed,
                want_rows=kc.reference(composed, rois))


def torch_composed(parts, bias, K, P):
    """The planes KeypointHead(raw=False) would compose in torch (float32, on the CPU): fold + bias + x2 upsample."""
    R = parts.shape[0]
    cols = torch.from_numpy(parts).permute(0, 5, 3, 4, 1, 2).reshape(R, 16 * K, P * P)
    low = F.fold(cols, (2 * P, 2 * P), kernel_size=4, stride=2, padding=1) + torch.from_numpy(bias).view(1, K, 1, 1)
    return F.interpolate(low, scale_factor=2, mode="bilinear", align_corners=False).numpy()


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", MS)
def test_every_class_in_both_layouts(pkg, torch_dev, M, K):
    c = class_case(M, K)
    dev, rois, P = torch_dev[1], c["rois"], M // 4
    assert tuple(c["names"]) == kc.BOX_CLASSES and (c["want"]["margin"][c["want"]["kind"] == 0] >= kc.MARGIN).all()
    one = (M + K) % len(kc.BOX_CLASSES)                       # R = 1: one class, another in every case
    for lo, hi in ((0, 7), (7, 14), (one, one + 1)):          # R = 7, 7, 1
        sub = {k: v[lo:hi] for k, v in c["want"].items() if k != "box"}
        e = kc.check_exact(run_kp(pkg, dev, c["planes"][lo:hi], rois[lo:hi], tag="classes"), sub, tag=f"planes {lo}:{hi}")
        print(f"M={M} K={K} planes rows {lo}:{hi}: worst score error {e:.2e} of the range")
        subr = {k: v[lo:hi] for k, v in c["want_rows"].items() if k != "box"}
        kept = c["kept"][lo:hi]
        loose = {(r, k) for r, k in zip(*np.nonzero(~kept))}
        plain = None
        for ld in sorted({16 * K, pad64(16 * K)}):
            rows = kc.to_deconv_rows(c["parts"][lo:hi], ld)
            got = run_kp(pkg, dev, rows, rois[lo:hi], "deconv_rows", K, M, c["bias"], tag=f"classes ld={ld}")
            if plain is None:
                plain = got
            assert kc.same_bits(got[0], plain[0]) and kc.same_bits(got[1], plain[1]), "ld changes the result"
        # exact positions where the margin rule held; the tolerance form on the planes it could not hold for
        strict = {k: v.copy() for k, v in subr.items()}
        for r, k in loose:
            strict["xy"][r, k], strict["scores"][r, k] = plain[0][r, k], plain[1][r, k]
        kc.check_exact(plain, strict, tag=f"deconv_rows {lo}:{hi}")
        if loose:
            kc.check_tolerant(plain, c["composed"][lo:hi], rois[lo:hi], pairs=loose, tag=f"deconv_rows loose {lo}:{hi}")
        # DECONV_ROWS equals PLANES on the torch-composed planes
        tc = torch_composed(c["parts"][lo:hi], c["bias"], K, P)
        ref = run_kp(pkg, dev, tc, rois[lo:hi], aligns=(256,), tag="composed")
        for r in range(hi - lo):
            if subr["kind"][r] != 0:
                continue
            for k in range(K):
                err = abs(float(ref[1][r, k]) - float(plain[1][r, k])) / subr["range"][r, k]
                assert err < TIGHT, (r, k, err)
                if kept[r, k]:
                    assert kc.same_bits(ref[0][r, k], plain[0][r, k]), (r, k)


@pytest.mark.parametrize("M", MS)
def test_exact_cases_are_bit_for_bit(pkg, torch_dev, M):
    """identity (coefficients (0, 1, 0, 0)) and a box of 2M (t in {0.25, 0.75}) on small-integer planes: every product
    and sum is exact in fp32, so the scores are the fp64 reference's bit for bit: two equal maxima (the lower index
    wins), an all-equal plane (index 0), a NaN before and after a larger value, two NaNs."""
    rois, planes = kc.exact_rois(M), kc.exact_planes(M)
    want = kc.reference(planes, rois)
    kp, sc = run_kp(pkg, torch_dev[1], planes, rois, tag="exact")
    assert kc.same_bits(kp, want["xy"])
    assert kc.same_bits(sc, want["scores"].astype(np.float32))
    assert (want["pos"][:, 2] == 0).all() and np.isnan(sc[:, 3:]).all() and (sc[:, 2] == 5).all()
    assert sc[0, 1] == 64 and want["pos"][0, 1] == (M * M) // 3


def test_special_rows_stay_in_their_row(pkg, torch_dev):
    M, K = 8, 3
    c = class_case(M, K)
    dev = torch_dev[1]
    keep = [i for i, n in enumerate(c["names"]) if n in ("identity", "fractional", "down", "up_odd", "one_pixel")]
    rois, planes = c["rois"][keep].copy(), c["planes"][keep].copy()
    clean = run_kp(pkg, dev, planes, rois, aligns=(256,))
    parts = c["parts"][keep]
    clean_rows = run_kp(pkg, dev, kc.to_deconv_rows(parts, 64), rois, "deconv_rows", K, M, c["bias"], aligns=(256,))
    specials = [("padding", (-1.0, 0, 0, 0, 0)), ("padding", (NAN, 1, 2, 30, 40)), ("padding", (-0.5, 1, 2, 30, 40)),
                ("padding", (-INF, NAN, NAN, NAN, NAN)),
                ("nan", (0, NAN, 2, 30, 40)), ("nan", (1, 1, INF, 30, 40)), ("nan", (0, 1, 2, -INF, 40)), ("nan", (0, 1, 2, 30, NAN)),
                ("nan", (0, -3e38, 2, 3e38, 40)), ("nan", (0, 1, 2, 1 + kc.MAX_SIDE + 0.5, 40)),
                ("nan", (0, 1, 2, 30, 2 + kc.MAX_SIDE + 0.25)), ("real", (0, 1, 2, 1 + kc.MAX_SIDE, 2 + 0.5))]
    for at, (kind, row) in enumerate(specials):
        r = at % len(keep)
        ro, pl, pa = rois.copy(), planes.copy(), parts.copy()
        ro[r] = row
        if kind != "real":
            pl[r], pa[r] = NAN, NAN       # (a special row reads no map)
        for layout, got, base in (("planes", run_kp(pkg, dev, pl, ro, tag=f"special {at}"), clean),
                                  ("deconv_rows", run_kp(pkg, dev, kc.to_deconv_rows(pa, 64), ro, "deconv_rows", K, M, c["bias"],
                                                         tag=f"special {at}"), clean_rows)):
            if kind == "padding":
                assert (got[0][r] == 0).all() and (got[1][r] == 0).all(), (at, layout)
            elif kind == "nan":
                assert np.isnan(got[0][r]).all() and np.isnan(got[1][r]).all(), (at, layout)
            else:   # wc = max_side exactly is still a real row
                assert np.isfinite(got[0][r]).all() and np.isfinite(got[1][r]).all() and (got[0][r, :, 2] == 1).all()
            for q in range(len(keep)):
                if q != r:
                    assert kc.same_bits(got[0][q], base[0][q]) and kc.same_bits(got[1][q], base[1][q]), (at, layout, q)


def test_a_nan_map_element_changes_no_other_plane(pkg, torch_dev):
    M, K = 8, 3
    c = class_case(M, K)
    dev = torch_dev[1]
    keep = [i for i, n in enumerate(c["names"]) if n in ("identity", "fractional", "down", "up_odd")]
    rois, planes, parts = c["rois"][keep], c["planes"][keep], c["parts"][keep]
    clean = run_kp(pkg, dev, planes, rois, aligns=(256,))
    clean_rows = run_kp(pkg, dev, kc.to_deconv_rows(parts, 64), rois, "deconv_rows", K, M, c["bias"], aligns=(256,))
    for r, k, (Y, X) in ((0, 1, (3, 4)), (1, 0, (0, 0)), (2, 2, (7, 7)), (3, 1, (5, 2))):
        dirty = planes.copy()
        dirty[r, k, Y, X] = NAN
        want = kc.reference(dirty, rois)
        got = run_kp(pkg, dev, dirty, rois, tag="nan element")
        assert np.isnan(got[1][r, k]) and np.isnan(want["scores"][r, k])
        assert kc.same_bits(got[0][r, k], want["xy"][r, k])          # the first output whose taps include it
        mask = np.ones((len(keep), K), dtype=bool)
        mask[r, k] = False
        assert kc.same_bits(got[0][mask], clean[0][mask]) and kc.same_bits(got[1][mask], clean[1][mask])
        # DECONV_ROWS: one partial product of (r, k); the composed reference says where it reaches
        dp = parts.copy()
        dp[r, Y % (M // 4), X % (M // 4), 1, 2, k] = NAN
        composed = kc.compose_planes(dp.reshape(-1, 16 * K), c["bias"], len(keep), K, M // 4)
        wantr = kc.reference(composed, rois)
        gotr = run_kp(pkg, dev, kc.to_deconv_rows(dp, 64), rois, "deconv_rows", K, M, c["bias"], tag="nan part")
        assert np.isnan(wantr["scores"][r, k]) and np.isnan(gotr[1][r, k]) and kc.same_bits(gotr[0][r, k], wantr["xy"][r, k])
        assert kc.same_bits(gotr[0][mask], clean_rows[0][mask]) and kc.same_bits(gotr[1][mask], clean_rows[1][mask])


def test_captured_without_a_prepare_replays_bitwise(pkg, torch_dev):
    M, K = 28, 3
    c = class_case(M, K)
    dev = torch_dev[1]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rows, ro, bias = t(kc.to_deconv_rows(c["parts"], 64)), t(c["rois"]), t(c["bias"])
    eager = [e.clone() for e in pkg.heatmaps_to_keypoints(rows, ro, K=K, M=M, layout="deconv_rows", bias=bias,
                                                          max_side=kc.MAX_SIDE)]
    kp, sc = torch.empty_like(eager[0]), torch.empty_like(eager[1])
    sg = torch.cuda.Stream()
    sg.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=sg):
        pkg.heatmaps_to_keypoints(rows, ro, K=K, M=M, layout="deconv_rows", bias=bias, max_side=kc.MAX_SIDE, out=kp,
                                  scores_out=sc)
    for _ in range(2):
        kp.fill_(7.0), sc.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(kp.view(torch.int32), eager[0].view(torch.int32))
        assert torch.equal(sc.view(torch.int32), eager[1].view(torch.int32))
    del graph


def test_every_refusal_comes_before_a_launch(pkg, torch_dev):
    R, K, M, ld = 5, 3, 8, 64
    P = M // 4
    dev = torch_dev[1]
    maps = torch.zeros(max(R * K * M * M, R * P * P * ld), device=dev)
    bias = torch.zeros(64, device=dev)
    rois = torch.tensor([[0.0, 1.0, 1.0, 9.0, 9.0]] * R + [[0.0] * 5] * 3, device=dev)   # (room behind for the + 16)
    kp = torch.full((R * K * 3 + 8,), NAN, device=dev)
    sc = torch.full((R * K + 8,), NAN, device=dev)
    big = torch.full((R * K * M * M + 64,), NAN, device=dev)   # for the overlaps
    ok = dict(maps=maps.data_ptr(), layout=1, bias=bias.data_ptr(), rois=rois.data_ptr(), R=R, K=K, M=M, ld=ld,
              max_side=512, keypoints=kp.data_ptr(), scores=sc.data_ptr())

    def call(**kw):
        a = dict(ok, **kw)
        return pkg.lib().wino_keypoints_hw(a["maps"], a["layout"], a["bias"], a["rois"], a["R"], a["K"], a["M"], a["ld"],
                                           a["max_side"], a["keypoints"], a["scores"], pkg._stream())

    E_SHAPE, E_ARG = -2, -3
    arg = [dict(maps=None), dict(rois=None), dict(keypoints=None), dict(scores=None), dict(bias=None),
           dict(layout=0), dict(layout=2), dict(layout=-1)]                      # (layout 0 with a bias)
    arg += [{k: ok[k] + 4} for k in ("maps", "bias", "rois", "keypoints", "scores")]
    rows_bytes = 4 * R * P * P * ld
    arg += [dict(keypoints=ok["maps"]), dict(scores=ok["maps"]), dict(keypoints=ok["rois"]), dict(scores=ok["rois"]),
            dict(keypoints=ok["bias"]), dict(scores=ok["bias"]), dict(keypoints=big.data_ptr(), scores=big.data_ptr() + 16),
            dict(maps=big.data_ptr(), scores=big.data_ptr() + rows_bytes - 16),
            dict(layout=0, bias=None, maps=big.data_ptr(), keypoints=big.data_ptr() + 4 * R * K * M * M - 16)]
    shape = [dict(R=-1), dict(K=0), dict(K=-3), dict(M=0), dict(M=68), dict(M=6), dict(M=7), dict(ld=16 * K - 1), dict(ld=0),
             dict(max_side=0), dict(max_side=16385), dict(max_side=-1), dict(layout=0, bias=None, M=65),
             dict(layout=0, bias=None, M=0), dict(layout=0, bias=None, K=0)]
    for kw in arg:
        assert call(**kw) == E_ARG, kw
    for kw in shape:
        assert call(**kw) == E_SHAPE, kw
    for kw in (dict(R=0), dict(R=0, maps=None, rois=None, bias=None, keypoints=None, scores=None)):
        assert call(**kw) == 0, kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(kp).all()) and bool(torch.isnan(sc).all()) and bool(torch.isnan(big).all())
    # PLANES ignores ld and takes any 1 <= M <= 64; the largest legal limits
    assert call() == 0 and call(layout=0, bias=None, ld=0, M=7) == 0 and call(max_side=16384, ld=16 * K) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(kp[:R * K * 3]).any()) and bool(torch.isnan(kp[R * K * 3:]).all())
    assert not bool(torch.isnan(sc[:R * K]).any()) and bool(torch.isnan(sc[R * K:]).all())
    # the wrapper: R = 0 launches nothing and returns empty tensors
    e = pkg.heatmaps_to_keypoints(torch.zeros(0, K, M, M, device=dev), torch.zeros(0, 5, device=dev))
    assert tuple(e[0].shape) == (0, K, 3) and tuple(e[1].shape) == (0, K)
    for kw, msg in ((dict(K=K + 1), "but maps is"), (dict(bias=bias[:K]), "no bias"), (dict(layout="deconv_rows"), "needs K and M")):
        with pytest.raises(pkg.WinoError, match=msg):
            pkg.heatmaps_to_keypoints(torch.zeros(R, K, M, M, device=dev), rois[:R], **kw)
    for kw, msg in ((dict(M=6), "M = 4 P"), (dict(bias=None), "needs bias"), (dict(ld=128), "but maps is"),
                    (dict(K=5), "16 K <= ld"), (dict(bias=bias[:K + 1]), "bias must be")):
        args = dict(K=K, M=M, layout="deconv_rows", bias=bias[:K])
        args.update(kw)
        with pytest.raises(pkg.WinoError, match=msg):
            pkg.heatmaps_to_keypoints(torch.zeros(R * P * P, ld, device=dev), rois[:R], **args)


def sweep_layouts(n=24, seed=2024):
    """n random legal layouts: (layout, M, K, ld, R, seed)."""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        rows = bool(i % 2)
        M = int(4 * rng.randint(1, 17)) if rows else int(rng.randint(1, 65))
        K = int(rng.randint(1, 21))
        ld = 16 * K + int(rng.choice([0, 1, 3, 16, 48])) if rows else 0
        out.append(("deconv_rows" if rows else "planes", M, K, ld, int(rng.randint(1, 10)), int(rng.randint(1 << 30))))
    return out


@pytest.mark.parametrize("layout,M,K,ld,R,seed", sweep_layouts())
def test_seeded_sweep_in_the_tolerance_form(pkg, torch_dev, layout, M, K, ld, R, seed):
    """Random layouts, box sizes up to 120 px and placements, no margin rule: the kernel's position must have an fp64
    value within TIGHT x range of the fp64 maximum and its score must be within TIGHT of the fp64 value there."""
    rng = np.random.RandomState(seed)
    rois = np.zeros((R, 5), dtype=np.float32)
    rois[:, 0] = rng.randint(0, 3, R)
    rois[:, 1:3] = rng.uniform(-50, 900, (R, 2))
    rois[:, 3:5] = rois[:, 1:3] + rng.choice([0.3, 1.0, 7.5, 33.25, 64.0, 119.9], (R, 2)) * rng.uniform(0.5, 1.0, (R, 2))
    if R > 2:
        rois[rng.randint(R)] = (-1, 0, 0, 0, 0)
    if layout == "planes":
        planes = rng.standard_normal((R, K, M, M)).astype(np.float32)
        got = run_kp(pkg, torch_dev[1], planes, rois, tag="sweep")
    else:
        P = M // 4
        parts = (rng.standard_normal((R, P, P, 4, 4, K)) * 0.5).astype(np.float32)
        bias = rng.standard_normal(K).astype(np.float32)
        planes = kc.compose_planes(parts.reshape(-1, 16 * K), bias, R, K, P)
        got = run_kp(pkg, torch_dev[1], kc.to_deconv_rows(parts, ld), rois, layout, K, M, bias, tag="sweep")
    worst = kc.check_tolerant(got, planes, rois, tag=f"sweep {layout} M={M} K={K} ld={ld} R={R}")
    print(f"{layout} M={M} K={K} ld={ld} R={R}: worst gap / score error {worst:.2e} of the range")


def test_maps_past_2_31_elements(pkg, torch_dev):
    """PLANES, K = 17, M = 56, R = 40 283: the last row starts past element 2^31.  Padding rows everywhere (they read
    nothing, so the 8.6 GB are never initialised) except one-pixel and identity boxes at the first and last rows."""
    K, M, R = 17, 56, 40283
    dev = torch_dev[1]
    assert (R - 1) * K * M * M > 1 << 31
    maps = torch.empty((R, K, M, M), dtype=torch.float32, device=dev)
    rois = np.zeros((R, 5), dtype=np.float32)
    rois[:, 0] = -1
    real = {0: "one_pixel", 1: "identity", R - 2: "identity", R - 1: "one_pixel"}
    for r, name in real.items():
        rois[r] = kc.class_roi(name, M, r % 2)
    rows = sorted(real)
    planes, _ = kc.draw_planes(rois[rows], K, M, seed=9)
    want = kc.reference(planes, rois[rows])
    for j, r in enumerate(rows):
        maps[r].copy_(torch.from_numpy(planes[j]))
    kp = torch.full((R, K, 3), NAN, device=dev)
    sc = torch.full((R, K), NAN, device=dev)
    pkg.heatmaps_to_keypoints(maps, torch.from_numpy(rois).to(dev), max_side=kc.MAX_SIDE, out=kp, scores_out=sc)
    torch.cuda.synchronize()
    kc.check_exact((kp[rows].cpu().numpy(), sc[rows].cpu().numpy()), want, tag="past 2^31")
    pad = torch.ones(R, dtype=torch.bool, device=dev)
    pad[rows] = False
    assert int(torch.count_nonzero(kp[pad])) == 0 and int(torch.count_nonzero(sc[pad])) == 0   # (a NaN left counts)
