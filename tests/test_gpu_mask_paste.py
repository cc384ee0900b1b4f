"""GPU tests of wino_mask_paste_hw / paste_masks on the guarded arena, at both placements of guarded.ALIGNS: against the
fp64 reference of tests/mask_cases.py (itself held to torchvision by tests/test_mask_paste_host.py) at cases.TIGHT, exact
zeros outside every window, exact window geometry on the lattice boxes, the binary output, illegal labels, values that are
not finite, the two layouts bit for bit, a graph, every refusal of the header, and one output past 4 GiB."""
import numpy as np
import pytest
import torch

import guarded
import mask_cases as mc
from cases import TIGHT
from gpu_support import as_f32, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu
N, D, NCLS = 2, 6, 5
SHAPES = ((40, 56), (37, 53), (5, 1), (130, 19))
MS = (2, 8, 28, 62)
NAN = float("nan")
NAN_BYTES = np.frombuffer(np.array([guarded.NAN_BITS], dtype="<u4").tobytes(), dtype=np.uint8)
LAYOUTS = (("planes", None), ("gemm_rows", 64), ("gemm_rows", 128))


def run_paste(pkg, dev, logits, labels, boxes, hw, H, W, layout="planes", ld=None, want=("out", "binary"), threshold=0.5,
              aligns=guarded.ALIGNS, tag=""):
    """The launch on numpy operands (logits in the planes layout; converted for gemm_rows), on the guarded arena at each
    of `aligns`, twice into NaN-filled outputs; every run is bitwise the first.  Returns (out, binary) as numpy or None."""
    R, classes, M = logits.shape[:3]
    n = N * D * H * W
    first = None
    for align in aligns:
        arena = guarded.Arena(torch, dev, align)
        src = logits if layout == "planes" else mc.to_gemm_rows(logits, ld)
        lg = arena.input(torch.from_numpy(np.ascontiguousarray(src)), name="logits")
        lb = arena.input(as_f32(labels.astype(np.int32)), name="labels").view(torch.int32)
        bx = arena.input(torch.from_numpy(boxes), name="boxes")
        ihw = arena.input(torch.from_numpy(hw), name="image_hw")
        out = arena.output(N, D, H, W, name="out") if "out" in want else None
        raw = arena.output((n + 3) // 4, name="binary").view(torch.uint8) if "binary" in want else None
        binary = None if raw is None else raw[:n].view(N, D, H, W)
        for _ in range(2):
            if out is not None:
                out.fill_(NAN)
            if raw is not None:
                raw.view(torch.float32).fill_(NAN)
            got = pkg.paste_masks(lg, lb, bx, ihw, H, W, M=M, classes=classes, layout=layout, out=out, binary=binary,
                                  want_out=False, threshold=threshold)
            assert got[0] is out and got[1] is binary
            arena.check(f"paste_masks {tag} {layout} ld={ld} H={H} W={W} M={M} align={align}")
            if raw is not None:   # the bytes that round the uint8 tensor up to whole floats
                assert np.array_equal(raw[n:].cpu().numpy(), NAN_BYTES[n % 4:] if n % 4 else NAN_BYTES[:0])
            cur = (None if out is None else out.cpu().numpy(), None if binary is None else binary.cpu().numpy())
            if first is None:
                first = cur
            for x, y in zip(cur, first):
                assert x is None or np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{tag}: not bitwise reproducible"
    return first


def case(H, W, M):
    boxes, hw, names = mc.paste_boxes(N, D, H, W, M)
    return mc.paste_logits(N * D, NCLS, M), mc.paste_labels(N * D, NCLS), boxes, hw, names


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_parity_both_layouts(pkg, torch_dev, H, W, M):
    logits, labels, boxes, hw, names = case(H, W, M)
    want, margin = mc.paste_reference(logits, labels, boxes, hw, H, W)
    inside = mc.paste_windows(labels, boxes, hw, M, NCLS, H, W)
    assert margin >= mc.INT_MARGIN
    if (H, W) in ((40, 56), (130, 19)):
        assert set(names) >= set(mc.CLASSES)
    ref = None
    for layout, ld in LAYOUTS:
        out, binary = run_paste(pkg, torch_dev[1], logits, labels, boxes, hw, H, W, layout, ld, tag="parity")
        err = float(np.abs(out.astype(np.float64) - want).max())
        print(f"H={H} W={W} M={M} {layout} ld={ld}: max |got - want| = {err:.2e}, int_margin {margin:.2e}")
        assert np.isfinite(out).all() and err < TIGHT
        assert (out[~inside] == 0).all() and out.min() >= 0 and out.max() <= 1
        assert np.array_equal(binary, (out > 0.5).astype(np.uint8))
        if ref is None:
            ref = out
        assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), "the two layouts differ"
    if inside.sum() > 200:
        # both sides of the threshold occur (how many lie above it depends on M: at M = 2 the ring is half the map)
        assert (ref[inside] > 0.5).sum() > 20 and (ref[inside] <= 0.5).sum() > 20


def test_every_class_is_present_somewhere():
    seen = set()
    for H, W in SHAPES:
        for M in MS:
            seen |= set(mc.paste_boxes(N, D, H, W, M)[2])
    assert seen >= set(mc.CLASSES)


@pytest.mark.parametrize("M", mc.LATTICE_M)
def test_lattice_windows_are_exact(pkg, torch_dev, M):
    H, W = 40, 56
    boxes, hw = mc.lattice_boxes(N, D, H, W, M)
    logits, labels = mc.paste_logits(N * D, NCLS, M), mc.paste_labels(N * D, NCLS)
    want, _ = mc.paste_reference(logits, labels, boxes, hw, H, W)
    for layout, ld in LAYOUTS[:2]:
        out, _ = run_paste(pkg, torch_dev[1], logits, labels, boxes, hw, H, W, layout, ld, want=("out",), tag="lattice")
        assert np.array_equal(out != 0, want != 0)
        assert float(np.abs(out - want).max()) < TIGHT


@pytest.mark.parametrize("H,W,M", ((37, 53, 28), (130, 19, 8), (5, 1, 2)))
def test_binary_alone_and_fp32_alone_are_the_both_runs(pkg, torch_dev, H, W, M):
    logits, labels, boxes, hw, _ = case(H, W, M)
    for thr in (0.5, 0.25, -1.0, 1.0):
        both = run_paste(pkg, torch_dev[1], logits, labels, boxes, hw, H, W, "gemm_rows", 64, threshold=thr)
        assert np.array_equal(both[1], (both[0] > np.float32(thr)).astype(np.uint8))
        only_b = run_paste(pkg, torch_dev[1], logits, labels, boxes, hw, H, W, "gemm_rows", 64, want=("binary",), threshold=thr)
        only_f = run_paste(pkg, torch_dev[1], logits, labels, boxes, hw, H, W, "gemm_rows", 64, want=("out",), threshold=thr)
        assert only_b[0] is None and np.array_equal(only_b[1], both[1])
        assert only_f[1] is None and np.array_equal(only_f[0].view(np.uint32), both[0].view(np.uint32))


def test_illegal_labels_give_zero_planes_and_read_nothing(pkg, torch_dev):
    H, W, M = 40, 56, 28
    logits, labels, boxes, hw, _ = case(H, W, M)
    clean, _ = run_paste(pkg, torch_dev[1], logits, labels, boxes, hw, H, W, aligns=(256,))
    labels, logits, boxes = labels.copy(), logits.copy(), boxes.copy()
    bad = {0: -1, 4: NCLS, 7: -2 ** 31, 11: 2 ** 31 - 1}
    for r, v in bad.items():
        labels[r] = v
        logits[r] = NAN
    boxes[4] = NAN   # (a padding row's box is not read either)
    for layout, ld in LAYOUTS[:2]:
        out, binary = run_paste(pkg, torch_dev[1], logits, labels, boxes, hw, H, W, layout, ld, tag="labels")
        for r in range(N * D):
            if r in bad:
                assert (out[r // D, r % D] == 0).all() and (binary[r // D, r % D] == 0).all()
            else:
                assert np.array_equal(out[r // D, r % D].view(np.uint32), clean[r // D, r % D].view(np.uint32))


def test_nan_logit_has_the_references_footprint(pkg, torch_dev):
    H, W, M = 40, 56, 8
    logits, labels, boxes, hw, names = case(H, W, M)
    clean, _ = run_paste(pkg, torch_dev[1], logits, labels, boxes, hw, H, W, aligns=(256,))
    for r, (Y, X) in ((names.index("inside"), (3, 4)), (names.index("larger"), (4, 4)), (names.index("cross_right"), (0, 0))):
        dirty = logits.copy()
        dirty[r, labels[r], Y, X] = NAN
        dirty[r, (labels[r] + 1) % NCLS] = NAN   # (another class's mask is not read)
        want, _ = mc.paste_reference(dirty, labels, boxes, hw, H, W)
        for layout, ld in LAYOUTS[:2]:
            out, binary = run_paste(pkg, torch_dev[1], dirty, labels, boxes, hw, H, W, layout, ld, tag="nan logit")
            assert np.array_equal(np.isnan(out), np.isnan(want)) and np.isnan(want[r // D, r % D]).any()
            assert (binary[np.isnan(out)] == 0).all()
            keep = ~np.isnan(want)
            assert float(np.abs(out[keep] - want[keep]).max()) < TIGHT
            for q in range(N * D):
                if q != r:
                    assert np.array_equal(out[q // D, q % D].view(np.uint32), clean[q // D, q % D].view(np.uint32))


def test_box_that_is_not_finite_fills_its_image_window_with_nan(pkg, torch_dev):
    H, W, M = 37, 53, 28
    logits, labels, boxes, hw, _ = case(H, W, M)
    clean, _ = run_paste(pkg, torch_dev[1], logits, labels, boxes, hw, H, W, aligns=(256,))
    im_h, im_w = mc.image_ints(hw, H, W)
    for r, col, v in ((2, 0, NAN), (8, 3, float("inf")), (9, 1, -float("inf"))):
        b = boxes.copy()
        b[r, col] = v
        out, binary = run_paste(pkg, torch_dev[1], logits, labels, b, hw, H, W, "gemm_rows", 64, tag="nan box")
        n, d = r // D, r % D
        assert np.isnan(out[n, d, :im_h[n], :im_w[n]]).all()
        assert (out[n, d, im_h[n]:] == 0).all() and (out[n, d, :, im_w[n]:] == 0).all() and (binary[n, d] == 0).all()
        for q in range(N * D):
            if q != r:
                assert np.array_equal(out[q // D, q % D].view(np.uint32), clean[q // D, q % D].view(np.uint32))


def test_captured_without_a_prepare_replays_bitwise(pkg, torch_dev):
    H, W, M = 37, 53, 28
    dev = torch_dev[1]
    logits, labels, boxes, hw, _ = case(H, W, M)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    lg, lb, bx, ihw = t(mc.to_gemm_rows(logits, 64)), t(labels), t(boxes), t(hw)
    eager = pkg.paste_masks(lg, lb, bx, ihw, H, W, M=M, classes=NCLS, layout="gemm_rows", want_binary=True)
    eager = [e.clone() for e in eager]
    out, binary = torch.empty_like(eager[0]), torch.empty_like(eager[1])
    sg = torch.cuda.Stream()
    sg.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=sg):
        pkg.paste_masks(lg, lb, bx, ihw, H, W, M=M, classes=NCLS, layout="gemm_rows", out=out, binary=binary)
    for _ in range(2):
        out.fill_(NAN), binary.fill_(255)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), eager[0].view(torch.int32)) and torch.equal(binary, eager[1])
    del graph


def test_every_refusal_comes_before_a_launch(pkg, torch_dev):
    H, W, M, ld = 8, 12, 4, 64
    dev = torch_dev[1]
    R = N * D
    lg = torch.zeros(R * M * M, ld, device=dev)
    lb = torch.zeros(R, dtype=torch.int32, device=dev)
    bx = torch.tensor([[1.0, 1.0, 6.0, 6.0]] * R, device=dev)
    hw = torch.tensor([[float(H), float(W)]] * N, device=dev)
    out = torch.full((N, D, H, W), NAN, device=dev)
    binary = torch.full((N, D, H, W), 7, dtype=torch.uint8, device=dev)
    big = torch.full((max(R * M * M * ld, N * D * H * W) + 64,), NAN, device=dev)   # for the overlaps
    ok = dict(logits=lg.data_ptr(), layout=1, labels=lb.data_ptr(), boxes=bx.data_ptr(), image_hw=hw.data_ptr(), N=N, D=D,
              classes=NCLS, M=M, ld=ld, H=H, W=W, threshold=0.5, out=out.data_ptr(), binary=binary.data_ptr())

    def call(**kw):
        a = dict(ok, **kw)
        return pkg.lib().wino_mask_paste_hw(a["logits"], a["layout"], a["labels"], a["boxes"], a["image_hw"], a["N"], a["D"],
                                            a["classes"], a["M"], a["ld"], a["H"], a["W"], a["threshold"], a["out"],
                                            a["binary"], pkg._stream())

    E_SHAPE, E_ARG = -2, -3
    arg = [dict(logits=None), dict(labels=None), dict(boxes=None), dict(image_hw=None), dict(out=None, binary=None),
           dict(threshold=NAN), dict(layout=2), dict(layout=-1)]
    arg += [{k: ok[k] + 4} for k in ("logits", "labels", "boxes", "image_hw", "out")] + [dict(binary=ok["binary"] + 1)]
    arg += [dict(out=ok["logits"]), dict(binary=ok["logits"]), dict(out=ok["boxes"]), dict(binary=ok["labels"]),
            dict(binary=ok["image_hw"]), dict(out=big.data_ptr(), binary=big.data_ptr() + 16),
            dict(out=big.data_ptr(), logits=big.data_ptr() + 4 * N * D * H * W - 16)]
    shape = [dict(M=0), dict(M=63), dict(M=3), dict(M=64), dict(classes=0), dict(classes=ld + 1), dict(N=-1), dict(D=-1),
             dict(H=0), dict(W=0), dict(H=65536, W=32768), dict(layout=0, M=63), dict(layout=0, classes=0)]
    for kw in arg:
        assert call(**kw) == E_ARG, kw
    for kw in shape:
        assert call(**kw) == E_SHAPE, kw
    for kw in (dict(N=0), dict(D=0), dict(N=0, logits=None, out=None, binary=None)):
        assert call(**kw) == 0, kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool((binary == 7).all()) and bool(torch.isnan(big).all())
    assert call() == 0 and call(layout=0, ld=0, classes=ld) == 0                 # PLANES ignores ld; [R][64][4][4] is lg's size
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any())


def test_past_4_gib(pkg, torch_dev):
    """N = 1, D = 5, 16384 x 16384 fp32: 5 GiB.  Boxes sit in the first and in the last plane; their windows are checked
    against the reference, everything else is zero by device-side reductions."""
    H = W = 16384
    M, Dn = 28, 5
    dev = torch_dev[1]
    boxes = np.array([[16000.3, 15900.2, 16300.6, 16420.4], [0, 0, 0, 0], [20000.5, 3.5, 20100.25, 90.5], [5.5, 5.5, 50.25, 60.5],
                      [-40.4, 16100.3, 70.6, 16380.7]], dtype=np.float32)
    labels = np.array([3, -1, 1, NCLS, 0], dtype=np.int32)
    hw = np.array([[float(H), float(W)]], dtype=np.float32)
    logits = mc.paste_logits(Dn, NCLS, M, seed=3)
    bi, _ = mc.box_integers(boxes, M, np.float32)
    bi64, _ = mc.box_integers(boxes, M, np.float64)
    assert (bi == bi64).all() and (mc.int_margin(boxes, M)[[0, 4]] > 0.01).all()   # (an fp32 ulp is 0.001 out there)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = torch.full((1, Dn, H, W), NAN, device=dev)
    assert out.numel() * 4 > 1 << 32
    pkg.paste_masks(t(mc.to_gemm_rows(logits, 64)), t(labels), t(boxes), t(hw), H, W, M=M, classes=NCLS, layout="gemm_rows",
                    out=out)
    torch.cuda.synchronize()
    inside = 0
    for d in (0, 4):
        (y0, y1e, x0, x1e), want = mc.plane_window(logits[d, labels[d]], bi[d], H, W)
        got = out[0, d, y0:y1e, x0:x1e]
        err = float((got.double().cpu() - torch.from_numpy(want)).abs().max())
        print(f"plane {d}: window rows {y0}..{y1e} columns {x0}..{x1e}, max |got - want| = {err:.2e}")
        assert err < TIGHT and y1e - y0 > 100 and x1e - x0 > 50
        inside += int(torch.count_nonzero(got))
    assert inside > 0 and int(torch.count_nonzero(out)) == inside     # (a NaN left unwritten counts as non-zero)
