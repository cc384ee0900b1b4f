"""The fp64 reference of wino_keypoints_hw's contract (include/winograd_mi355x.h) and the cases its tests share.  Imports no
test module and needs no GPU.

The reference restates the contract: the box arithmetic in numpy float32, operation by operation; the bicubic resize
(exact integer source coordinates, not clamped at 0; torch's cubic convolution coefficients at A = -0.75; taps clamped
into [0, M); all 16 taps always multiplied, so a NaN reaches exactly the outputs whose taps include it), the
DECONV_ROWS gather and the x2 bilinear upsample in fp64; the argmax under torch.argmax's rules.

Named box classes (`BOX_CLASSES`, `class_rois`), small by design, and standard normal maps drawn under the margin rule: a
plane is redrawn until the fp64 best value beats the second best by at least MARGIN = 1e-4 of the plane's range (5 x
cases.TIGHT: an error within TIGHT of the range on each value cannot move the argmax), at most MAX_DRAWS times."""
import functools

import numpy as np

from cases import TIGHT

MARGIN = 5 * TIGHT
MAX_DRAWS = 64
MAX_SIDE = 512          # what the tests pass as max_side: above `wide` and `tall`, below `oversize`
F32 = np.float32
BOX_CLASSES = ("identity", "up_even", "up_odd", "fractional", "down", "one_pixel", "inverted", "thin_row", "thin_column",
               "wide", "tall", "padding", "nonfinite", "oversize")
SPECIAL = ("padding", "nonfinite", "oversize")


# ---- the contract, restated --------------------------------------------------------------------------------------------
def box_arith(rois, max_side=MAX_SIDE):
    """rois [R][5] -> dict of per-row arrays: kind (0 real, 1 padding, 2 NaN row), w, h, cw, ch (float32), wc, hc (int64;
    1 on the special rows)."""
    r = np.asarray(rois, dtype=F32).reshape(-1, 5)
    n, x1, y1, x2, y2 = (r[:, i] for i in range(5))
    with np.errstate(all="ignore"):
        pad = ~(n >= 0)
        finite = np.isfinite(r[:, 1:]).all(axis=1)
        w = np.maximum(x2 - x1, F32(1))
        h = np.maximum(y2 - y1, F32(1))
        bad = ~pad & (~finite | ~(w <= F32(max_side)) | ~(h <= F32(max_side)))
    kind = np.where(pad, 1, np.where(bad, 2, 0))
    real = kind == 0
    w, h = np.where(real, w, F32(1)).astype(F32), np.where(real, h, F32(1)).astype(F32)
    wcf, hcf = np.ceil(w), np.ceil(h)
    return dict(kind=kind, w=w, h=h, wc=wcf.astype(np.int64), hc=hcf.astype(np.int64), cw=(w / wcf).astype(F32),
                ch=(h / hcf).astype(F32), x1=x1, y1=y1)


def cubic_coefficients(t):
    """torch's get_cubic_upsample_coefficients at A = -0.75, fp64: [..., 4] for the taps i - 1 .. i + 2."""
    A = -0.75
    t = np.asarray(t, dtype=np.float64)
    c1 = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1
    c2 = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    return np.stack([c2(t + 1), c1(t), c1(1 - t), c2(2 - t)], axis=-1)


@functools.lru_cache(maxsize=None)
def resize_weights(M: int, out: int):
    """(W [out][M] fp64, T [out][M] bool): output d = sum_j W[d][j] src[j]; T marks the source indices d's four taps touch
    (also where the coefficient is 0)."""
    d = np.arange(out, dtype=np.int64)
    num = (2 * d + 1) * M - out
    i = num // (2 * out)                                   # numpy's // floors
    t = (num - i * 2 * out).astype(np.float64) / float(2 * out)
    c = cubic_coefficients(t)
    W, T = np.zeros((out, M)), np.zeros((out, M), dtype=bool)
    for j in range(4):
        idx = np.clip(i - 1 + j, 0, M - 1)
        np.add.at(W, (d, idx), c[:, j])
        T[d, idx] = True
    return W, T


def resize_plane(plane, hc: int, wc: int):
    """The contract's hc x wc bicubic resize of one M x M plane in fp64, NaNs with the taps' footprint."""
    p = np.asarray(plane, dtype=np.float64)
    M = p.shape[0]
    Wy, Ty = resize_weights(M, int(hc))
    Wx, Tx = resize_weights(M, int(wc))
    nan = np.isnan(p)
    out = Wy @ np.where(nan, 0.0, p) @ Wx.T
    if nan.any():
        out[(Ty.astype(np.float64) @ nan.astype(np.float64) @ Tx.T.astype(np.float64)) > 0] = np.nan
    return out


def argmax_torch(flat):
    """torch.argmax over a 1-d array: the first NaN if there is one, else the first of the greatest values."""
    nan = np.flatnonzero(np.isnan(flat))
    return int(nan[0]) if nan.size else int(np.argmax(flat))


def plane_range(plane) -> float:
    p = np.asarray(plane, dtype=np.float64)
    p = p[np.isfinite(p)]
    return max(float(p.max() - p.min()), 1e-30) if p.size else 1.0


def plane_result(plane, hc: int, wc: int):
    """(pos, value at pos, margin = (best - second best) / the plane's range; inf when there is one output or a NaN)."""
    big = resize_plane(plane, hc, wc).reshape(-1)
    pos = argmax_torch(big)
    if big.size == 1 or np.isnan(big).any():
        return pos, float(big[pos]), float("inf")
    top = np.partition(big, big.size - 2)[-2:]
    return pos, float(big[pos]), float(top[1] - top[0]) / plane_range(plane)


def keypoint_xy(pos, b, r):
    """The float32 restatement of the output: ((x_i + 0.5) cw + x1, (y_i + 0.5) ch + y1, 1) of row r."""
    wc = int(b["wc"][r])
    yi, xi = divmod(int(pos), wc)
    x = (F32(xi) + F32(0.5)) * b["cw"][r] + b["x1"][r]
    y = (F32(yi) + F32(0.5)) * b["ch"][r] + b["y1"][r]
    return np.array([x, y, F32(1)], dtype=F32)


def reference(planes, rois, max_side=MAX_SIDE):
    """planes [R][K][M][M] (any float dtype), rois [R][5] -> dict(pos [R][K] int64, -1 on special rows; xy [R][K][3]
    float32; scores [R][K] fp64; margin [R][K]; range [R][K]; kind [R])."""
    planes = np.asarray(planes)
    R, K = planes.shape[:2]
    b = box_arith(rois, max_side)
    pos = np.full((R, K), -1, dtype=np.int64)
    xy, scores = np.zeros((R, K, 3), dtype=F32), np.zeros((R, K))
    margin, rng = np.full((R, K), np.inf), np.ones((R, K))
    for r in range(R):
        if b["kind"][r] == 2:
            xy[r], scores[r] = np.nan, np.nan
        if b["kind"][r] != 0:
            continue
        for k in range(K):
            pos[r, k], scores[r, k], margin[r, k] = plane_result(planes[r, k], b["hc"][r], b["wc"][r])
            xy[r, k] = keypoint_xy(pos[r, k], b, r)
            rng[r, k] = plane_range(planes[r, k])
    return dict(pos=pos, xy=xy, scores=scores, margin=margin, range=rng, kind=b["kind"], box=b)


# ---- the DECONV_ROWS layout -----------------------------------------------------------------------------------------
def gather_low(rows, bias, R: int, K: int, P: int):
    """rows [R P P][ld] -> low [R][K][2P][2P] in fp64: the at most four partial products per output pixel, summed in
    ascending (ky, kx), the bias added last."""
    rows = np.asarray(rows, dtype=np.float64)
    t = rows[:, :16 * K].reshape(R, P, P, 4, 4, K)
    low = np.zeros((R, K, 2 * P, 2 * P))
    span = lambda k: (1 if k == 0 else 0, P - 1 if k == 3 else P)   # the inputs i with 0 <= 2 i - 1 + k < 2 P
    for ky in range(4):
        ya, yb = span(ky)
        for kx in range(4):
            xa, xb = span(kx)
            if ya < yb and xa < xb:   # oy = 2 iy - 1 + ky, ox = 2 ix - 1 + kx
                low[:, :, 2 * ya - 1 + ky:2 * yb - 1 + ky:2, 2 * xa - 1 + kx:2 * xb - 1 + kx:2] += \
                    t[:, ya:yb, xa:xb, ky, kx, :].transpose(0, 3, 1, 2)
    return low + np.asarray(bias, dtype=np.float64)[None, :, None, None]


@functools.lru_cache(maxsize=None)
def upsample2_weights(L: int):
    """(W [2L][L] fp64, T [2L][L]): the bilinear align_corners=False x2 upsample with the exact integer coordinate, clamped
    at 0; T marks the two taps of an output (also where lambda is 0: both are always multiplied)."""
    W, T = np.zeros((2 * L, L)), np.zeros((2 * L, L))
    for d in range(2 * L):
        num = max((2 * d + 1) * L - 2 * L, 0)
        i0 = num // (4 * L)
        i1 = min(i0 + 1, L - 1)
        lam = (num - i0 * 4 * L) / (4.0 * L)
        W[d, i0] += 1 - lam
        W[d, i1] += lam
        T[d, i0] = T[d, i1] = 1
    return W, T


def compose_planes(rows, bias, R: int, K: int, P: int):
    """The M x M planes (M = 4P) the DECONV_ROWS layout stands for, fp64 [R][K][M][M]; a NaN partial product reaches the
    low pixel it is summed into and from there the outputs whose taps include that pixel."""
    low = gather_low(rows, bias, R, K, P)
    U, T = upsample2_weights(2 * P)
    nan = np.isnan(low)
    out = np.einsum("ya,rkab,xb->rkyx", U, np.where(nan, 0.0, low), U)
    if nan.any():
        out[np.einsum("ya,rkab,xb->rkyx", T, nan.astype(np.float64), T) > 0] = np.nan
    return out


def to_deconv_rows(parts, ld: int):
    """parts [R][P][P][4][4][K] float32 -> rows [R P P][ld], the columns past 16 K NaN (they are never read)."""
    R, P, _, _, _, K = parts.shape
    rows = np.full((R * P * P, ld), np.nan, dtype=F32)
    rows[:, :16 * K] = parts.reshape(R * P * P, 16 * K)
    return rows


# ---- the named boxes ---------------------------------------------------------------------------------------------------
def class_roi(name: str, M: int, n: int = 0):
    """One RoIAlign row (n, x1, y1, x2, y2) of class `name` for M x M heatmaps."""
    m = float(M)
    box = {
        "identity": (3.0, 5.0, 3.0 + m, 5.0 + m),
        "up_even": (2.0, 1.0, 2.0 + 2 * m, 1.0 + 2 * m),
        "up_odd": (0.0, 4.0, 3 * m, 4.0 + 3 * m),
        "fractional": (1.25, 2.5, 1.25 + 1.7 * m + 0.3, 2.5 + 1.3 * m + 0.35),
        "down": (6.5, 7.25, 6.5 + 0.6 * m, 7.25 + 0.4 * m + 0.7),
        "one_pixel": (7.25, 9.5, 7.75, 9.875),
        "inverted": (20.0, 6.0, 10.0, 6.0 + 1.5 * m),
        "thin_row": (2.0, 3.0, 2.0 + 2.5 * m, 3.75),
        "thin_column": (4.0, 1.0, 4.5, 1.0 + 2.5 * m),
        "wide": (1.5, 2.5, 301.25, 5.125),
        "tall": (2.5, 1.5, 5.125, 301.25),
        "padding": (0.0, 0.0, 0.0, 0.0),
        "nonfinite": (float("nan"), 1.0, 5.0, 6.0),
        "oversize": (0.0, 0.0, MAX_SIDE + 0.5, 4.0),
    }[name]
    return np.array([-1.0 if name == "padding" else float(n), *box], dtype=F32)


def class_rois(M: int, names=BOX_CLASSES, R=None):
    """[R][5]: the named classes in turn (repeated to R rows), image index alternating 0 / 1."""
    names = list(names)
    R = len(names) if R is None else int(R)
    rows = [class_roi(names[r % len(names)], M, r % 2) for r in range(R)]
    return np.stack(rows), [names[r % len(names)] for r in range(R)]


# ---- maps under the margin rule ----------------------------------------------------------------------------------------
class MarginError(RuntimeError):
    pass


def draw_planes(rois, K: int, M: int, seed: int = 0, max_side=MAX_SIDE):
    """Standard normal planes [R][K][M][M] float32, each redrawn until it keeps MARGIN at its row's box (special rows
    keep their first draw).  Returns (planes, draws [R][K]); raises MarginError past MAX_DRAWS."""
    rng = np.random.RandomState(seed)
    b = box_arith(rois, max_side)
    R = len(b["kind"])
    planes, draws = np.zeros((R, K, M, M), dtype=F32), np.ones((R, K), dtype=np.int64)
    for r in range(R):
        for k in range(K):
            for n in range(1, MAX_DRAWS + 1):
                planes[r, k] = rng.standard_normal((M, M)).astype(F32)
                draws[r, k] = n
                if b["kind"][r] != 0 or plane_result(planes[r, k], b["hc"][r], b["wc"][r])[2] >= MARGIN:
                    break
            else:
                raise MarginError(f"row {r} plane {k}: no draw of {MAX_DRAWS} keeps the margin")
    return planes, draws


def draw_deconv_parts(rois, K: int, P: int, seed: int = 0, max_side=MAX_SIDE):
    """Partial products [R][P][P][4][4][K] float32 (normal, scaled so that the composed planes are near standard normal) and
    bias [K], the block of each (r, k) redrawn until the composed fp64 plane keeps MARGIN.  Returns (parts, bias, draws,
    kept [R][K]).  Unlike draw_planes it does not raise: a composed plane is an x2 bilinear upsample, smooth by construction,
    and at P = 1 (a ramp between four values) its 300-pixel resize has a smooth interior maximum whose neighbours lie
    within MARGIN at every draw (measured yield 0.00 at P = 1 and 0.18 at P = 2 for `wide`).  Such a plane keeps its last
    draw with kept = False, and its tests hold it to the tolerance form instead of an exact position."""
    rng = np.random.RandomState(seed)
    b = box_arith(rois, max_side)
    R = len(b["kind"])
    bias = rng.standard_normal(K).astype(F32)
    parts, draws = np.zeros((R, P, P, 4, 4, K), dtype=F32), np.ones((R, K), dtype=np.int64)
    kept = np.ones((R, K), dtype=bool)
    for r in range(R):
        for k in range(K):
            for n in range(1, MAX_DRAWS + 1):
                block = (rng.standard_normal((P, P, 4, 4)) * 0.5).astype(F32)
                draws[r, k] = n
                if b["kind"][r] != 0:
                    break
                plane = compose_planes(block.reshape(P * P, 16), bias[k:k + 1], 1, 1, P)[0, 0]
                if plane_result(plane, b["hc"][r], b["wc"][r])[2] >= MARGIN:
                    break
            else:
                kept[r, k] = False
            parts[r, :, :, :, :, k] = block
    return parts, bias, draws, kept


# ---- exact cases: every product exact in fp32 --------------------------------------------------------------------------
def exact_rois(M: int):
    """Two rows whose resize is exact in fp32 on small-integer maps: identity (coefficients (0, 1, 0, 0)) and a box of
    exactly 2M (t in {0.25, 0.75}: coefficients with denominator 256)."""
    return np.stack([class_roi("identity", M, 0), class_roi("up_even", M, 1)])


def exact_planes(M: int, K: int = 6, seed: int = 0):
    """[2][K][M][M] small-integer planes for exact_rois: k = 0 random integers, 1 two equal maxima, 2 all equal, 3 a NaN
    before a larger value, 4 a NaN after a larger value, 5 two NaNs (the first wins)."""
    rng = np.random.RandomState(seed)
    planes = rng.randint(-3, 4, size=(2, K, M, M)).astype(F32)
    last = M * M - 1
    a, b = (M * M) // 3, (2 * M * M) // 3
    for r in range(2):
        flat = planes[r].reshape(K, -1)
        if K > 1:
            flat[1, a] = flat[1, b] = 64.0
        if K > 2:
            flat[2, :] = 5.0
        if K > 3:
            flat[3, a], flat[3, b] = np.nan, 64.0
        if K > 4:
            flat[4, a], flat[4, last] = 64.0, np.nan
        if K > 5:
            flat[5, a] = flat[5, b] = np.nan
    return planes


# ---- what the GPU tests assert ----------------------------------------------------------------------------------------
def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def pos_from_xy(xy, b, r):
    """The flat index a keypoint (x, y) of row r stands for."""
    wc, hc = int(b["wc"][r]), int(b["hc"][r])
    xi = int(round((float(xy[0]) - float(b["x1"][r])) / float(b["cw"][r]) - 0.5))
    yi = int(round((float(xy[1]) - float(b["y1"][r])) / float(b["ch"][r]) - 0.5))
    return min(max(yi, 0), hc - 1) * wc + min(max(xi, 0), wc - 1)


def check_exact(got, want, rows=None, tag=""):
    """Positions exact (x, y bit-equal to the float32 restatement of the reference's position) and scores within TIGHT of
    the plane's range; special rows zeros / NaN."""
    kp, sc = got
    rows = range(len(want["kind"])) if rows is None else rows
    worst = 0.0
    for r in rows:
        kind = want["kind"][r]
        if kind == 1:
            assert (kp[r] == 0).all() and (sc[r] == 0).all(), (tag, r)
        elif kind == 2:
            assert np.isnan(kp[r]).all() and np.isnan(sc[r]).all(), (tag, r)
        else:
            assert same_bits(kp[r], want["xy"][r]), (tag, r, kp[r], want["xy"][r])
            nan = np.isnan(want["scores"][r])
            assert np.array_equal(np.isnan(sc[r]), nan), (tag, r)
            err = np.abs(sc[r].astype(np.float64) - want["scores"][r])[~nan] / want["range"][r][~nan]
            worst = max(worst, float(err.max()) if err.size else 0.0)
    assert worst < TIGHT, (tag, worst)
    return worst


def check_tolerant(got, planes, rois, max_side=MAX_SIDE, pairs=None, tag=""):
    """The tolerance form: the kernel's position is a position of the box (its float32 restatement is the output bit for
    bit), its fp64 value is within TIGHT x range of the fp64 maximum, and the score is within TIGHT x range of the fp64
    value there.  `pairs`: the (r, k) to check (default: all); special rows zeros / NaN."""
    kp, sc = got
    b = box_arith(rois, max_side)
    R, K = sc.shape
    worst = 0.0
    for r in range(R):
        if b["kind"][r] == 1:
            assert (kp[r] == 0).all() and (sc[r] == 0).all(), (tag, r)
        elif b["kind"][r] == 2:
            assert np.isnan(kp[r]).all() and np.isnan(sc[r]).all(), (tag, r)
        else:
            for k in range(K):
                if pairs is not None and (r, k) not in pairs:
                    continue
                big = resize_plane(planes[r, k], b["hc"][r], b["wc"][r]).reshape(-1)
                rng = plane_range(planes[r, k])
                pos = pos_from_xy(kp[r, k], b, r)
                assert same_bits(kp[r, k], keypoint_xy(pos, b, r)), (tag, r, k)
                gap = float(big.max() - big[pos]) / rng
                err = abs(float(sc[r, k]) - float(big[pos])) / rng
                worst = max(worst, gap, err)
                assert gap < TIGHT and err < TIGHT, (tag, r, k, gap, err)
    return worst


# ---- the head ------------------------------------------------------------------------------------------------------------
def keypoint_head_state_dict(C: int, widths, K: int, seed: int = 0):
    """KeypointRCNNHeads(C, widths) + KeypointRCNNPredictor(widths[-1], K) under the names they have below roi_heads."""
    import torch
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    rb = lambda n: (torch.rand(n, generator=g) - 0.5) * 0.2
    sd, c = {}, C
    for i, w in enumerate(widths):
        sd[f"keypoint_head.{2 * i}.weight"] = rn(w, c, 3, 3) * (2.0 / (9 * c)) ** 0.5
        sd[f"keypoint_head.{2 * i}.bias"] = rb(w)
        c = w
    sd["keypoint_predictor.kps_score_lowres.weight"] = rn(c, K, 4, 4) * (1.0 / c) ** 0.5
    sd["keypoint_predictor.kps_score_lowres.bias"] = rb(K)
    return sd


def keypoint_head_reference(sd, pooled, stop_at_low: bool = False):
    """fp64: pooled [R][P][P][C] (NHWC, unpadded) -> keypoint logits [R][K][4P][4P] (stop_at_low: the transposed
    convolution's [R][K][2P][2P])."""
    import torch
    F = torch.nn.functional
    d = {k: v.double() for k, v in sd.items()}
    x = pooled.double().permute(0, 3, 1, 2)
    for i in range(8):
        x = torch.relu(F.conv2d(x, d[f"keypoint_head.{2 * i}.weight"], d[f"keypoint_head.{2 * i}.bias"], padding=1))
    x = F.conv_transpose2d(x, d["keypoint_predictor.kps_score_lowres.weight"],
                           d["keypoint_predictor.kps_score_lowres.bias"], stride=2, padding=1)
    return x if stop_at_low else F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
