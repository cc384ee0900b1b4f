"""The cases, references and guarded-arena runs of FCOS's two kernels, shared by tests/test_fcos_host.py and
tests/test_gpu_fcos_kernels.py.  Nothing here needs a GPU to import.

fcos_score_map: ScoreLevel is one level's class-logit map and regression map; rings, pad columns and every regression
column but the centerness hold NaN, so a single stray read of them shows in a score.  fcos_decode: the levels are
tests/retina_cases.py's DecodeLevel (regression map with NaN ring and pad columns, base anchors, image sizes, a seeded idx
with padding rows); the references are a torch-CPU fp32 transcription of BoxLinearCoder(normalize_by_size=True).decode
on relu(columns), operation by operation, and the same in fp64."""
import functools

import numpy as np

import retina_cases as rc

SCORE_HW = ((1, 1), (1, 2), (3, 5), (7, 11), (13, 21))
SCORE_K = (1, 5, 91)
CTR_COL = 4


class ScoreLevel:
    def __init__(self, N, h, w, K, seed=0):
        rng = np.random.RandomState(seed)
        self.N, self.h, self.w, self.K, self.ld_c, self.ld_r = N, h, w, K, rc.pad64(K), 64
        self.logits = rng.uniform(-6, 4, (N, h, w, K)).astype(np.float32)
        self.ctr = rng.uniform(-3, 3, (N, h, w)).astype(np.float32)

    def cls_map(self, logits=None):
        m = np.full((self.N, self.h + 2, self.w + 2, self.ld_c), np.nan, dtype=np.float32)
        m[:, 1:-1, 1:-1, :self.K] = self.logits if logits is None else logits
        return m

    def reg_map(self, ctr=None):
        m = np.full((self.N, self.h + 2, self.w + 2, self.ld_r), np.nan, dtype=np.float32)
        m[:, 1:-1, 1:-1, CTR_COL] = self.ctr if ctr is None else ctr
        return m


@functools.lru_cache(maxsize=None)
def score_level(h, w, K, N=2):
    return ScoreLevel(N, h, w, K, seed=100 * h + 10 * w + K)


def score_reference(logits, ctr):
    """sqrt(sigmoid(logit) * sigmoid(ctr)) in fp64: [N][h][w][K]."""
    sig = lambda v: 1.0 / (1.0 + np.exp(-np.asarray(v, np.float64)))
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt(sig(logits) * sig(ctr)[..., None])


def run_score_map(pkg, dev, c, logits=None, ctr=None, aligns=None, tag=""):
    """fcos_score_map on level `c` on the guarded arena, twice from a fresh copy of the logits, bitwise equal.  Pad
    columns and the ring of the class map keep their NaN bits; the regression map is unchanged.  Returns [N][h][w][K]."""
    import torch

    import guarded
    master = torch.from_numpy(c.cls_map(logits))
    first = None
    for align in (guarded.ALIGNS if aligns is None else aligns):
        arena = guarded.Arena(torch, dev, align)
        cls = arena.input(master, name="cls", in_place=True)
        reg = arena.input(torch.from_numpy(c.reg_map(ctr)), name="reg")
        for _ in range(2):
            cls.copy_(master)
            assert pkg.fcos_score_map(cls, reg, c.K, CTR_COL) is cls
            arena.check(f"fcos_score_map {tag} align={align}")
            got = cls.cpu().numpy()
            keep = np.ones(got.shape, dtype=bool)
            keep[:, 1:-1, 1:-1, :c.K] = False
            assert (got.view(np.int32)[keep] == np.int32(guarded.NAN_BITS)).all(), f"{tag}: ring or pad columns written"
            cur = got[:, 1:-1, 1:-1, :c.K].copy()
            if first is None:
                first = cur
            assert np.array_equal(cur.view(np.int32), first.view(np.int32)), f"{tag}: not bitwise reproducible"
    return first


# ---- fcos_decode -------------------------------------------------------------------------------------------------------------
def _decode(c, deltas, dtype):
    """BoxLinearCoder(normalize_by_size=True).decode on relu(deltas) of every anchor of level `c`, then
    clip_boxes_to_image, in torch on the CPU in `dtype`, in the kernel's order of operations: [N][h w A][4]."""
    import torch
    d = torch.from_numpy(np.ascontiguousarray(c.deltas if deltas is None else deltas)).to(dtype).reshape(c.N, c.h * c.w, c.A, 4)
    d = torch.where(d < 0, torch.zeros((), dtype=dtype), d)                   # the head's ReLU; NaN stays
    gh, gw, sy, sx = c.grid
    ys, xs = torch.meshgrid(torch.arange(c.h), torch.arange(c.w), indexing="ij")
    ox, oy = xs.reshape(-1).to(dtype) * float(sx), ys.reshape(-1).to(dtype) * float(sy)
    anc = torch.from_numpy(c.base).to(dtype)[None, :, :] + torch.stack([ox, oy, ox, oy], dim=1)[:, None, :]   # [h w][A][4]
    cx, cy = 0.5 * (anc[..., 0] + anc[..., 2]), 0.5 * (anc[..., 1] + anc[..., 3])
    aw, ah = anc[..., 2] - anc[..., 0], anc[..., 3] - anc[..., 1]
    x1, y1 = cx - d[..., 0] * aw, cy - d[..., 1] * ah
    x2, y2 = cx + d[..., 2] * aw, cy + d[..., 3] * ah
    hw = torch.from_numpy(c.image_hw).to(dtype)
    H, W = hw[:, 0].reshape(-1, 1, 1), hw[:, 1].reshape(-1, 1, 1)
    clip = lambda v, hi: torch.where(v < 0, torch.zeros((), dtype=dtype), torch.where(v > hi, hi.expand_as(v), v))
    return torch.stack([clip(x1, W), clip(y1, H), clip(x2, W), clip(y2, H)], dim=-1).reshape(c.N, -1, 4).numpy()


def decode_fp32(c, deltas=None):
    import torch
    return _decode(c, deltas, torch.float32)


def decode_fp64(c, deltas=None):
    import torch
    return _decode(c, deltas, torch.float64)


def coder_formula(anchor, ltrb, image_hw):
    """One box by the coder's formula in plain Python floats (fp64): the check of the references themselves."""
    x1, y1, x2, y2 = (float(v) for v in anchor)
    l, t, r, b = (max(float(v), 0.0) for v in ltrb)
    cx, cy, w, h = 0.5 * (x1 + x2), 0.5 * (y1 + y2), x2 - x1, y2 - y1
    H, W = (float(v) for v in image_hw)
    box = (cx - l * w, cy - t * h, cx + r * w, cy + b * h)
    return [min(max(box[0], 0.0), W), min(max(box[1], 0.0), H), min(max(box[2], 0.0), W), min(max(box[3], 0.0), H)]


def run_fcos_decode(pkg, dev, c, deltas=None, offset=0, extra=0, aligns=None, tag=""):
    """fcos_decode on level `c` on the guarded arena, into [N][offset + rows + extra] outputs, twice, bitwise equal; what
    lies outside the slice keeps its NaN fill.  Returns this launch's slice of (boxes, labels)."""
    import torch

    import guarded
    from gpu_support import as_f32
    total, first = offset + c.rows + extra, None
    idx_full = np.full((c.N, total), -7, dtype=np.int32)
    idx_full[:, offset:offset + c.rows] = c.idx
    for align in (guarded.ALIGNS if aligns is None else aligns):
        arena = guarded.Arena(torch, dev, align)
        idx = arena.input(as_f32(idx_full), name="idx").view(torch.int32)
        reg = arena.input(torch.from_numpy(c.reg_map(deltas)), name="reg")
        base = arena.input(torch.from_numpy(c.base), name="base")
        hw = arena.input(torch.from_numpy(c.image_hw), name="image_hw")
        ob = arena.output(c.N, total, 4, name="boxes")
        ol = arena.output(c.N, total, name="labels").view(torch.int32)
        for _ in range(2):
            ob.fill_(float("nan")), ol.fill_(guarded.NAN_BITS)
            got = pkg.fcos_decode(idx, reg, base, hw, c.grid, c.K, c.rows, ob, ol, offset)
            assert got[0] is ob and got[1] is ol
            arena.check(f"fcos_decode {tag} align={align}")
            b, l = ob.cpu().numpy(), ol.cpu().numpy()
            outside = np.ones(total, dtype=bool)
            outside[offset:offset + c.rows] = False
            assert np.isnan(b[:, outside]).all() and (l[:, outside] == guarded.NAN_BITS).all(), "wrote outside its slice"
            cur = (b[:, offset:offset + c.rows].copy(), l[:, offset:offset + c.rows].copy())
            if first is None:
                first = cur
            assert np.array_equal(cur[0].view(np.int32), first[0].view(np.int32)) and np.array_equal(cur[1], first[1]), \
                f"{tag}: not bitwise reproducible (align {align})"
    return first
