"""Seeded random-shape generators for the ResNet entry points, the grouped 3x3 layer and the two ResNeXt blocks, and the
segmentation path (the dilated 3x3 layer and its bottleneck blocks, the concat projection, ASPP, the bilinear resize),
shared by tests/test_shape_sweeps_host.py (every case is
legal and the draws reach the corners they claim, no GPU) and tests/test_gpu_shape_sweeps.py (every case against an
fp64 reference on an MI355X).

Each generator returns a fixed list of Case: the shape, the forced developer knobs (None: the automatic choice, named
by the plan query), and the flags.  The draws span the legal envelope winograd_mi355x.h states for the entry point, not
only ResNet's stage shapes; each case is bounded so that its fp64 CPU reference stays below MAX_MACS multiply-adds.
`plan_form` is the one place that asks the library's host-side plan queries which form a case takes."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np

# the latency forms the plan queries accept are those of the existing forced-form tests (one table per family)
from cases import PROJ_FORMS, S2_FORMS, s2_legal
from dilated_cases import FORMS as DIL_FORMS
from resize_cases import DIRECT, STAGED, smallest_direct_channels

MAX_MACS = 2e9
MAX_SUM_MACS = 1e10   # the segmentation entries: all of a generator's references together
CUS = 256


@dataclass(frozen=True)
class Case:
    entry: str
    shape: dict
    knobs: dict | None = None     # WINO_* developer knobs of a forced form; None = the planner's choice
    form: str | None = None       # the forced form's name (None = automatic)
    flags: dict = field(default_factory=dict)

    def __getattr__(self, name):   # case.N, case.C, ... read the shape
        shape = object.__getattribute__(self, "shape")
        if name in shape:
            return shape[name]
        raise AttributeError(name)

    def tag(self) -> str:
        s = " ".join(f"{k}={v}" for k, v in self.shape.items())
        f = " ".join(f"{k}" for k, v in self.flags.items() if v)
        return f"[{self.entry} {s} form={self.form or 'auto'} {f}]".replace(" ]", "]")


def _s2(h: int) -> int:
    return (h - 1) // 2 + 1


def stem_out(H: int, W: int):
    return _s2(_s2(H)), _s2(_s2(W))


def head_cols(classes: int) -> int:
    return (classes + 63) // 64 * 64


def macs(case: Case) -> float:
    """Multiply-adds of the case's fp64 reference."""
    s = case.shape
    e = case.entry
    if e == "conv3x3_bn_add_relu":
        return 9.0 * s["N"] * s["H"] * s["W"] * s["C"] * s["K"]
    if e == "basic_block":
        return 18.0 * s["N"] * s["H"] * s["W"] * s["C"] * s["C"]
    if e in ("conv3x3_s2_bn_relu", "conv3x3_s2_proj", "basic_block_s2"):
        px = s["N"] * _s2(s["Hin"]) * _s2(s["Win"])
        m = px * 10.0 * s["C"] * s["K"]
        return m + (9.0 * px * s["K"] * s["K"] if e == "basic_block_s2" else 0)
    if e in ("proj_block", "proj_block_v15"):
        stride = s.get("stride", 2)
        px_in = s["N"] * s["Hin"] * s["Win"]
        px = s["N"] * ((s["Hin"] - 1) // stride + 1) * ((s["Win"] - 1) // stride + 1)
        first = (px_in if e == "proj_block_v15" else px) * s["Cin"] * s["Cm"]
        return first + px * (9.0 * s["Cm"] * s["Cm"] + (s["Cm"] + s["Cin"]) * s["C4"])
    if e == "stem":
        return 147.0 * s["N"] * _s2(s["H"]) * _s2(s["W"]) * s["K"]
    if e == "avgpool_fc":
        return float(s["N"]) * s["C"] * (s["H"] * s["W"] + s["classes"])
    if e == "conv3x3_dilated_bn_relu":
        return 9.0 * s["N"] * s["H"] * s["W"] * s["C"] * s["K"]
    if e == "dilated_block":
        px = float(s["N"]) * s["H"] * s["W"]
        return px * (s["Cin"] * s["Cm"] + 9.0 * s["Cm"] * s["Cm"] + (s["Cm"] + (s["Cin"] if s["proj"] else 0)) * s["C4"])
    if e == "conv1x1_cat_bn":
        return float(s["N"]) * s["H"] * s["W"] * s["S"] * s["Cs"] * s["Kout"]
    if e == "aspp":
        px = float(s["N"]) * s["H"] * s["W"]
        return px * (28.0 * s["Cin"] * s["Cb"] + 5.0 * s["Cb"] * s["Kout"]) + s["N"] * s["Cb"] * (s["Cin"] + s["Kout"])
    if e == "resize_bilinear":
        return 4.0 * s["N"] * s["C"] * s["Ho"] * s["Wo"]
    if e == "fpn_level":
        return float(s["N"]) * s["H"] * s["W"] * (s["Cin"] * s["Cf"] + 9.0 * s["Cf"] * s["Cf"])
    if e == "conv3x3_grouped_bn_relu":
        H, W = grouped_out(s["Hin"], s["Win"], s["stride"])
        return 9.0 * s["N"] * H * W * s["C"] * (s["C"] // s["groups"])
    if e == "grouped_block":
        H, W = grouped_out(s["Hin"], s["Win"], s["stride"])
        px = float(s["N"]) * H * W
        return (float(s["N"]) * s["Hin"] * s["Win"] * s["Cin"] * s["Cm"] + px * 9.0 * s["Cm"] * (s["Cm"] // s["groups"])
                + px * (s["Cm"] + (s["Cin"] if s["proj"] else 0)) * s["C4"])
    raise KeyError(e)


def _pinned(sh, pin):
    """The shape with the pinned dimensions of `pin` set; "odd" makes the map (and a stride-2 output) odd x odd."""
    sh = dict(sh)
    if pin.get("odd"):
        for a in ("H", "W", "Hin", "Win"):
            if a in sh:
                sh[a] |= 1
                if a.endswith("in") and _s2(sh[a]) % 2 == 0:
                    sh[a] += 2
    sh.update({k: v for k, v in pin.items() if k != "odd"})
    return sh


def _draw(rng, make, ok=lambda sh: True, entry=None, pin=None):
    """Draw shapes with `make(rng)` until one, with `pin`'s dimensions set where the form allows them, is accepted by
    `ok` and stays within the reference budget."""
    for i in range(4000):
        sh = make(rng)
        if pin and i < 2000:
            sh = _pinned(sh, pin)
        if ok(sh) and macs(Case(entry, sh)) <= MAX_MACS:
            return sh
    raise RuntimeError(f"{entry}: no shape drawn")


def _flags(rng, i, relu=True, in_place=False):
    """relu on / off, in place / out of place, non-negative (post-ReLU) inputs; alternated so that every value of
    each flag occurs."""
    f = {"nonneg": bool(i % 3 == 1)}
    if relu:
        f["relu"] = bool(i % 4 != 3)
    if in_place:
        f["in_place"] = bool((i // 2) % 2)
    return f


# ---- the residual 3x3 (conv3x3_bn_add_relu) and the identity basic block ----------------------------------------
def _items_3x3(N, H, W, K):
    """Work items of the 3x3 throughput kernel: 64 tiles x 64 out-channels."""
    return ((N * ((H + 1) // 2) * ((W + 1) // 2) + 63) // 64) * (K // 64)


def residual_3x3_cases():
    rng = np.random.RandomState(3311)
    cases = []
    # throughput grids with and without a stream-K tail, latency block widths and splits, the automatic choice
    forms = ["auto"] * 6 + ["big_tail"] * 4 + ["big_whole"] * 2 + ["small"] * 7
    # corners pinned on the first draws: 1-wide maps, odd x odd, C % 64 != 0, K = 192
    pins = [{"H": 1}, {"W": 1}, {"odd": True}, {"K": 192}, {"C": 200}, {"odd": True, "K": 192}, {"C": 40}]
    for i, form in enumerate(forms):
        c16 = form == "small" or (form == "auto" and i % 2 == 0)   # the latency kernel takes C % 16 == 0

        def make(r):
            step = 16 if c16 else 8
            return {"N": int(r.randint(1, 7)), "H": int(r.randint(1, 25)), "W": int(r.randint(1, 25)),
                    "C": step * int(r.randint(1, 200 // step + 1)), "K": int(r.choice([64, 128, 192, 256]))}

        ok = (lambda sh: sh["C"] % 16 == 0) if c16 else (lambda sh: True)
        sh = _draw(rng, make, ok, "conv3x3_bn_add_relu", pins[i % len(pins)] if i < 2 * len(pins) else None)
        knobs = None
        if form.startswith("big"):
            items = _items_3x3(sh["N"], sh["H"], sh["W"], sh["K"])
            if form == "big_whole":
                grid = int(rng.choice([g for g in range(1, items + 1) if items % g == 0]))
            else:
                grid = int(rng.randint(2, 2 * items + 40))
                while items % grid == 0:
                    grid += 1
            knobs = {"WINO_3X3_ALGO": "big", "WINO_SK_GRID": grid}
        elif form == "small":
            smax = max(1, min(8, (sh["C"] // 16) // 2))   # the splits test_gpu_latency.py treats as legal
            knobs = {"WINO_3X3_ALGO": "small", "WINO_SMALL_CT": (1, 2, 4)[i % 3],
                     "WINO_SMALL_SPLIT": int(rng.randint(1, smax + 1))}
        cases.append(Case("conv3x3_bn_add_relu", sh, knobs, None if form == "auto" else form,
                          _flags(rng, i, in_place=True)))
    return cases


def basic_block_cases():
    rng = np.random.RandomState(1834)
    pins = [{"H": 1}, {"W": 1}, {"odd": True}, {"C": 192}, {"C": 64, "odd": True}]
    cases = []
    for i in range(14):
        def make(r):
            return {"N": int(r.randint(1, 7)), "H": int(r.randint(1, 25)), "W": int(r.randint(1, 25)),
                    "C": int(r.choice([64, 128, 192, 256]))}

        sh = _draw(rng, make, entry="basic_block", pin=pins[i] if i < len(pins) else None)
        cases.append(Case("basic_block", sh, None, None, {"in_place": bool(i % 2), "nonneg": bool(i % 3 == 1)}))
    # the automatic throughput kernel inside the block: more 16-tile blocks than CUs (outside N <= 6)
    cases.append(Case("basic_block", {"N": 72, "H": 16, "W": 15, "C": 64}, None, None,
                      {"in_place": True, "nonneg": True}))
    return cases


# ---- the stride-2 3x3, the fused stride-2 3x3 + shortcut, the downsampling basic block ---------------------------
def _s2_make(r):
    return {"N": int(r.randint(1, 9)), "Hin": int(r.randint(1, 41)), "Win": int(r.randint(1, 41)),
            "C": 32 * int(r.randint(1, 16)), "K": 64 * int(r.randint(1, 9))}


def _s2_ok(form):
    kn = S2_FORMS.get(form)

    def ok(sh):
        if kn is None:
            return True
        if not s2_legal(form, (sh["N"], sh["Hin"], sh["Win"], sh["C"], sh["K"])):
            return False
        if kn["WINO_1X1_ALGO"] == "small":
            return (9 * sh["C"]) // kn["WINO_1X1_SMALL_KS"] >= 64   # the planner's shortest K loop per wave
        if kn.get("WINO_1X1_SK") == 1:   # enough (row tile, k-step) ranges for a stream-K grid
            return sh["C"] >= 64 and sh["N"] * _s2(sh["Hin"]) * _s2(sh["Win"]) >= 64 and _grid_fits(kn, sh["K"])
        return True
    return ok


def _grid_fits(kn, *cols):
    """A forced WINO_1X1_SK_GRID is rounded down to a multiple of 8 and of the column blocks: keep it non-zero."""
    return all((c // 64) in (1, 2, 4, 8) for c in cols) or "WINO_1X1_SK_GRID" not in kn


# 1x1 output maps (Hin <= 2), odd output maps, C % 64 != 0, K % 128 != 0
S2_PINS = [{"Hin": 1}, {"Win": 2}, {"odd": True}, {"C": 96}, {"K": 192}, {"C": 160, "K": 320}]
# each automatic form on a shape of its own (the tiled form only past N <= 8)
S2_AUTO = [{"N": 3, "Hin": 2, "Win": 3, "C": 64, "K": 64}, {"N": 18, "Hin": 27, "Win": 34, "C": 32, "K": 128}, {"N": 9, "Hin": 1, "Win": 8, "C": 480, "K": 64},
           {"N": 4, "Hin": 27, "Win": 29, "C": 480, "K": 192}]


def _s2_cases(entry, seed, forms):
    rng = np.random.RandomState(seed)
    cases = []
    for i, form in enumerate(forms):
        pin = S2_PINS[i % len(S2_PINS)] if i < 2 * len(S2_PINS) else None
        sh = _draw(rng, _s2_make, _s2_ok(form), entry, pin)
        flags = {"nonneg": bool(i % 3 == 1)}
        if entry == "conv3x3_s2_bn_relu":
            flags["relu"] = bool(i % 4 != 3)
        cases.append(Case(entry, sh, dict(S2_FORMS[form]) if form != "auto" else None,
                          None if form == "auto" else form, flags))
    for j, sh in enumerate(S2_AUTO):
        flags = {"nonneg": j % 2 == 0, **({"relu": j != 1} if entry == "conv3x3_s2_bn_relu" else {})}
        cases.append(Case(entry, dict(sh), None, None, flags))
    return cases


def conv3x3_s2_cases():
    return _s2_cases("conv3x3_s2_bn_relu", 2202, sorted(S2_FORMS) + ["auto"] * 4)


def conv3x3_s2_proj_cases():
    return _s2_cases("conv3x3_s2_proj", 2303, sorted(S2_FORMS) + ["auto"] * 4)


def basic_block_s2_cases():
    return _s2_cases("basic_block_s2", 2404, ["auto"] * 14)


# ---- the projection bottleneck blocks ------------------------------------------------------------------------------
def _proj_make(stride):
    def make(r):
        sh = {"N": int(r.randint(1, 7)), "Hin": int(r.randint(1, 31)), "Win": int(r.randint(1, 31)),
              "Cin": 32 * int(r.randint(1, 17)), "Cm": 64 * int(r.randint(1, 9)), "C4": 64 * int(r.randint(1, 9))}
        if stride:
            sh["stride"] = stride
        return sh
    return make


def _proj_ok(knobs):
    def ok(sh):
        if knobs is None:
            return True
        Cin = sh["Cin"]
        if knobs["WINO_1X1_ALGO"] == "small":
            ks = knobs.get("WINO_1X1_SMALL_KS", 1)
            # both launches (K = Cin, then Cm + Cin) in 16 ks chunks, at least 64 per wave when ks > 1
            return Cin % (16 * ks) == 0 and (ks == 1 or Cin // ks >= 64)
        if knobs.get("WINO_1X1_SK") == 1:
            st = sh.get("stride", 2)
            return (Cin >= 128 and sh["N"] * ((sh["Hin"] - 1) // st + 1) * ((sh["Win"] - 1) // st + 1) >= 112
                    and _grid_fits(knobs, sh["Cm"], sh["C4"]))
        return True
    return ok


PROJ_PINS = [{"Hin": 1}, {"Win": 1}, {"odd": True}, {"Cin": 96}, {"C4": 192}, {"Cin": 224, "Cm": 192}]


def proj_block_cases():
    rng = np.random.RandomState(5150)
    cases = []
    forms = [(f, s) for f in sorted(PROJ_FORMS) for s in (1, 2)] + [("auto", 1), ("auto", 2)] * 3
    for i, (form, stride) in enumerate(forms):
        kn = dict(PROJ_FORMS[form]) if form != "auto" else None
        pin = PROJ_PINS[i % len(PROJ_PINS)] if i < 2 * len(PROJ_PINS) else None
        sh = _draw(rng, _proj_make(stride), _proj_ok(kn), "proj_block", pin)
        cases.append(Case("proj_block", sh, kn, None if form == "auto" else form, {"nonneg": bool(i % 3 == 1)}))
    # the automatic tiled and stream-K forms of both launches: batches past N <= 6
    for sh in ({"N": 20, "Hin": 18, "Win": 26, "Cin": 96, "Cm": 64, "C4": 64, "stride": 1},
               {"N": 16, "Hin": 29, "Win": 19, "Cin": 352, "Cm": 64, "C4": 64, "stride": 1}):
        cases.append(Case("proj_block", sh, None, None, {"nonneg": True}))
    return cases


V15_FORMS = {"tiled": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 0},
             "stream_k": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1}}


def proj_block_v15_cases():
    rng = np.random.RandomState(1515)
    cases = []
    forms = ["auto"] * 8 + ["tiled"] * 3 + ["stream_k"] * 4
    for i, form in enumerate(forms):
        kn = dict(V15_FORMS[form]) if form != "auto" else None
        pin = PROJ_PINS[i % len(PROJ_PINS)] if i < 2 * len(PROJ_PINS) else None
        sh = _draw(rng, _proj_make(None), _proj_ok(kn), "proj_block_v15", pin)
        cases.append(Case("proj_block_v15", sh, kn, None if form == "auto" else form, {"nonneg": bool(i % 3 == 1)}))
    # the automatic tiled and stream-K forms of each launch: batches past N <= 6
    for sh in ({"N": 18, "Hin": 26, "Win": 14, "Cin": 160, "Cm": 192, "C4": 320},
               {"N": 35, "Hin": 10, "Win": 26, "Cin": 480, "Cm": 64, "C4": 448},
               {"N": 18, "Hin": 58, "Win": 57, "Cin": 32, "Cm": 64, "C4": 64}):
        cases.append(Case("proj_block_v15", sh, None, None, {"nonneg": True}))
    return cases


# ---- the stem and the head -----------------------------------------------------------------------------------------
def stem_cases():
    rng = np.random.RandomState(7749)
    pins = [{"H": 1}, {"W": 1}, {"odd": True}, {"K": 192}, {"K": 320}, {"H": 2, "W": 3}]
    cases = []
    for i, form in enumerate(["auto"] * 6 + ["big"] * 6 + ["small"] * 6):
        def make(r):
            return {"N": int(r.randint(1, 7)), "H": int(r.randint(1, 261)), "W": int(r.randint(1, 261)),
                    "K": int(r.choice([64, 128, 192, 256, 320]))}

        sh = _draw(rng, make, entry="stem", pin=pins[i % len(pins)])
        kn = {"WINO_STEM_FORM": {"big": 1, "small": 2}[form]} if form != "auto" else None
        cases.append(Case("stem", sh, kn, None if form == "auto" else form, {"padded": bool(i % 2)}))
    # the automatic big form: batches of larger maps
    cases.append(Case("stem", {"N": 6, "H": 203, "W": 181, "K": 64}, None, None, {"padded": True}))
    cases.append(Case("stem", {"N": 31, "H": 172, "W": 1, "K": 192}, None, None, {"padded": False}))
    return cases


HEAD_FORMS = {"latency": {"WINO_1X1_ALGO": "small"},
              "tiled": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 0},
              "stream_k": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1}}


def head_cases():
    rng = np.random.RandomState(1000)
    pins = [{"H": 1}, {"W": 1}, {"odd": True}, {"C": 96}, {"classes": 1000}, {"classes": 64 * 7}, {"classes": 1},
            {"C": 2080, "classes": 1100}]
    cases = []
    for i, form in enumerate(["auto"] * 8 + ["latency"] * 4 + ["tiled"] * 4 + ["stream_k"] * 4):
        def make(r):
            sh = {"N": int(r.randint(1, 41)), "H": int(r.randint(1, 10)), "W": int(r.randint(1, 10)),
                  "C": 32 * int(r.randint(1, 66)), "classes": int(r.randint(1, 1101))}
            if r.rand() < 0.3:
                sh["classes"] = 64 * int(r.randint(1, 18))
            return sh

        ok = (lambda sh: sh["C"] >= 512 and head_cols(sh["classes"]) // 64 in (1, 2, 4, 8, 16)) \
            if form == "stream_k" else (lambda sh: True)
        sh = _draw(rng, make, ok, "avgpool_fc", pins[i % len(pins)])
        cases.append(Case("avgpool_fc", sh, HEAD_FORMS.get(form), None if form == "auto" else form,
                          {"padded": bool(i % 2)}))
    # the automatic stream-K GEMM: a batch past N <= 40
    cases.append(Case("avgpool_fc", {"N": 291, "H": 3, "W": 4, "C": 1760, "classes": 404}, None, None, {"padded": True}))
    return cases


# ---- the segmentation path: the dilated 3x3, its bottleneck blocks, the concat projection, ASPP, the resize ---------
SEG_MACS = 3e8   # per case, so that a generator's references together stay below MAX_SUM_MACS


def _pkg():
    """The library, for the two corners that only a host-side plan query can place (nothing here touches a GPU)."""
    import __graft_entry__ as ge
    return ge.load_package()


def dil_class(H, W, d):
    """The reach class of a dilation against the map: 0 d < min(H, W); 1 W <= d < H (only the vertical taps are live);
    2 H <= d < W; 3 d >= max(H, W) (only the centre tap)."""
    if d < min(H, W):
        return 0
    if d >= max(H, W):
        return 3
    return 1 if W <= d < H else 2


def _dil_d(r, H, W, cls):
    """A dilation of reach class `cls` for the map, or None when the map has none."""
    lo, hi = min(H, W), max(H, W)
    if cls == 0 and lo == 1:      # a one-line map has no d below both sides: the class of its long side
        cls = 3 if hi == 1 else (2 if H == 1 else 1)
    if cls == 0:
        return int(r.randint(1, lo))
    if cls == 3:
        return hi + int(r.randint(0, 12))
    if (cls == 1) != (W < H) or H == W:
        return None
    return int(r.randint(lo, hi))


def largest_dilation(pkg, N, H, W, C, K):
    """The largest dilation check_dilated accepts for the shape: bisected on the plan query's own refusal."""
    def ok(d):
        try:
            pkg.conv3x3_dilated_plan(N, H, W, C, K, d)
            return True
        except pkg.WinoError:
            return False
    lo, hi = 1, 1 << 30
    assert ok(lo) and not ok(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return lo


WIDE_MAP = {"N": 1, "H": 3, "W": 2001, "C": 32, "K": 64}   # the map of the largest-dilation corner

# forced forms on shapes that take them (8- and 4-wave tiles; 64-, 128- and 320-wide outputs; 1, 2, 3, 4, 5 k-steps per
# tap): grids with a range boundary inside a tap, on a tap boundary, and (C = 32) on nothing else
DIL_FORCED = [
    ((2, 28, 28, 64, 256, 2), "split_24"), ((3, 15, 13, 96, 128, 4), "split_40"), ((3, 11, 9, 128, 192, 2), "split_104"),
    ((5, 6, 6, 160, 128, 7), "stream_k"), ((2, 10, 10, 64, 320, 2), "split_40"), ((1, 20, 20, 32, 64, 2), "split_24"),
    ((2, 9, 11, 64, 64, 3), "tiled"), ((2, 8, 8, 96, 64, 9), "tiled"), ((1, 12, 12, 64, 64, 2), "stream_k"),
]
# corners pinned on the automatic draws: d = 1; one-line maps longer than d; odd x odd; a tile over >= 3 images; one
# k-step per tap; an odd number > 1; C >= 512; K % 128 != 0
DIL_PINS = [{"d": 1}, {"H": 1, "cls": 2}, {"W": 1, "cls": 1}, {"odd": True}, {"N": 4, "H": 5, "W": 7}, {"C": 32}, {"C": 96},
            {"C": 512, "K": 64}, {"K": 320}, {"K": 192}, {"C": 32, "N": 6}, {"C": 160}]


def dilated_cases():
    rng = np.random.RandomState(6161)
    entry = "conv3x3_dilated_bn_relu"
    cases = []
    for i in range(20):
        pin = dict(DIL_PINS[i]) if i < len(DIL_PINS) else {}
        cls = pin.pop("cls", i % 4)
        for _ in range(4000):
            sh = {"N": int(rng.randint(1, 7)), "H": int(rng.randint(1, 23)), "W": int(rng.randint(1, 23)),
                  "C": 32 * int(rng.randint(1, 9)), "K": int(rng.choice([64, 128, 192, 256, 320]))}
            sh = _pinned(sh, {k: v for k, v in pin.items() if k != "d"})
            if sh["H"] == 1 or sh["W"] == 1:     # a one-line map: the line is longer than d
                sh["H" if sh["W"] == 1 else "W"] += 6
            sh["d"] = pin.get("d") or _dil_d(rng, sh["H"], sh["W"], cls)
            if sh["d"] and macs(Case(entry, sh)) <= SEG_MACS:
                break
        else:
            raise RuntimeError(f"{entry}: no shape drawn")
        cases.append(Case(entry, sh, None, None, _flags(rng, i)))
    # the whole tensor inside one tile's window; the largest dilation the wide map takes; automatic whole tiles
    extra = [{"N": 3, "H": 3, "W": 3, "C": 64, "K": 128, "d": 5},
             {**WIDE_MAP, "d": largest_dilation(_pkg(), *WIDE_MAP.values())},
             {"N": 12, "H": 20, "W": 20, "C": 32, "K": 64, "d": 2}]
    for sh in extra:
        cases.append(Case(entry, sh, None, None, _flags(rng, len(cases))))
    for (N, H, W, C, K, d), form in DIL_FORCED:
        sh = {"N": N, "H": H, "W": W, "C": C, "K": K, "d": d}
        cases.append(Case(entry, sh, dict(DIL_FORMS[form]), form, _flags(rng, len(cases))))
    return cases


BLOCK_FORMS = V15_FORMS
# (N, H, W, Cin, Cm, C4, d, proj, form): every launch of the block in the forced form
BLOCK_FORCED = [
    ((2, 12, 12, 256, 128, 256, 2, False), "stream_k"), ((3, 10, 12, 128, 128, 256, 4, True), "stream_k"),
    ((2, 9, 9, 256, 64, 256, 2, False), "tiled"), ((1, 7, 11, 128, 64, 192, 4, True), "tiled"),
]
BLOCK_PINS = [{"H": 1}, {"W": 1}, {"Cm": 64}, {"Cm": 192}, {"C4": 192}, {"Cm": 320, "C4": 320}, {"odd": True}, {"Cm": 64, "C4": 320}]


def dilated_block_cases():
    rng = np.random.RandomState(6262)
    entry = "dilated_block"
    cases = []
    for i in range(16):
        proj = bool(i % 2)
        pin = BLOCK_PINS[(i // 2) % len(BLOCK_PINS)] if i < 2 * len(BLOCK_PINS) else {}
        cls = (0, 3, 1, 2)[(i // 2 + i % 2) % 4]
        for _ in range(4000):
            sh = {"N": int(rng.randint(1, 7)), "H": int(rng.randint(1, 19)), "W": int(rng.randint(1, 19)),
                  "Cin": 32 * int(rng.randint(1, 13)), "Cm": 64 * int(rng.randint(1, 6)), "C4": 64 * int(rng.randint(1, 7))}
            sh = _pinned(sh, pin)
            if not proj:
                sh["Cin"] = sh["C4"]
            sh["d"] = _dil_d(rng, sh["H"], sh["W"], cls)
            sh["proj"] = proj
            if sh["d"] and macs(Case(entry, sh)) <= SEG_MACS / 2:
                break
        else:
            raise RuntimeError(f"{entry}: no shape drawn")
        cases.append(Case(entry, sh, None, None, {"nonneg": bool(i % 3 == 1)}))
    # the automatic whole-tile form of the last 1x1 launch: a batch past its latency form
    cases.append(Case(entry, {"N": 8, "H": 20, "W": 21, "Cin": 64, "Cm": 64, "C4": 320, "d": 3, "proj": True}, None, None,
                      {"nonneg": True}))
    for (N, H, W, Cin, Cm, C4, d, proj), form in BLOCK_FORCED:
        sh = {"N": N, "H": H, "W": W, "Cin": Cin, "Cm": Cm, "C4": C4, "d": d, "proj": proj}
        cases.append(Case(entry, sh, dict(BLOCK_FORMS[form]), form, {"nonneg": bool(len(cases) % 3 == 1)}))
    return cases


# forced forms of the concat layer: 1 .. 8 k-steps per source; grids with a range boundary inside a source and on one
CAT_FORCED = [
    ((2, 28, 28, 4, 64, 256), "split_24"), ((3, 15, 13, 5, 96, 128), "split_40"), ((1, 16, 16, 8, 256, 64), "split_104"),
    ((3, 7, 11, 5, 96, 192), "stream_k"), ((2, 12, 12, 3, 160, 320), "split_40"), ((8, 1, 1, 4, 64, 128), "stream_k"),
    ((2, 9, 9, 4, 64, 64), "tiled"), ((3, 7, 11, 5, 96, 192), "tiled"), ((30, 14, 14, 2, 32, 64), "split_24"),
]
# M % 112 == 0; every row its own image; a tile over >= 3 images; one k-step per source, an odd number, DeepLab's width;
# Kout % 128 != 0
CAT_PINS = [{"N": 2, "H": 7, "W": 8}, {"N": 9, "H": 1, "W": 1}, {"N": 5, "H": 3, "W": 4}, {"Cs": 32}, {"Cs": 96}, {"Cs": 256},
            {"Kout": 192}, {"Cs": 32, "S": 8}, {"N": 4, "H": 14, "W": 14, "S": 2}, {"odd": True}]


def _cat_flags(i):
    return {"relu": bool(i % 3 != 2), "a_padded": bool(i % 2), "c_padded": bool((i // 2) % 2), "nonneg": bool(i % 5 == 1)}


def cat_cases():
    rng = np.random.RandomState(6363)
    entry = "conv1x1_cat_bn"
    cases = []

    def add(sh, form):
        i = len(cases)
        p = 2 if _cat_flags(i)["a_padded"] else 0
        n = sh["N"] * (sh["H"] + p) * (sh["W"] + p) * sh["Cs"]
        # between two sources: nothing, the smallest legal gap, more than a source
        sh["gap"] = (0, 4, n + 4 * int(rng.randint(1, 64)))[i % 3]
        cases.append(Case(entry, sh, dict(DIL_FORMS[form]) if form else None, form, _cat_flags(i)))

    for i in range(16):
        def make(r):
            return {"N": int(r.randint(1, 9)), "H": int(r.randint(1, 15)), "W": int(r.randint(1, 15)),
                    "S": int(r.choice([2, 3, 5, 8])), "Cs": 32 * int(r.randint(1, 9)),
                    "Kout": int(r.choice([64, 128, 192, 256, 320]))}
        add(_draw(rng, make, lambda sh: macs(Case(entry, sh)) <= SEG_MACS, entry, CAT_PINS[i] if i < len(CAT_PINS) else None),
            None)
    for (N, H, W, S, Cs, Kout), form in CAT_FORCED:
        add({"N": N, "H": H, "W": W, "S": S, "Cs": Cs, "Kout": Kout}, form)
    return cases


# (H, W, rates): ascending, non-ascending, two equal; one rate past the map, all three; a 1x1 map
ASPP_RATES = [((9, 9), (1, 2, 3)), ((7, 11), (4, 2, 12)), ((6, 8), (3, 3, 5)), ((5, 5), (12, 24, 36)), ((1, 1), (1, 2, 3)),
              ((8, 6), (2, 9, 2)), ((1, 9), (2, 4, 6)), ((10, 3), (1, 3, 2))]
ASPP_PINS = [{"Cb": 64}, {"Cb": 192}, {"Cb": 320, "Kout": 64}, {"N": 3}, {"Cin": 32, "Cb": 64, "Kout": 128}, {"N": 4, "Cb": 128}]


def aspp_cases():
    rng = np.random.RandomState(6464)
    entry = "aspp"
    cases = []
    for i in range(14):
        (H, W), rates = ASPP_RATES[i % len(ASPP_RATES)]
        if i >= len(ASPP_RATES):
            H, W = int(rng.randint(1, 13)), int(rng.randint(1, 13))
            rates = tuple(int(v) for v in rng.randint(1, 16, size=3))

        def make(r):
            return {"N": int(r.randint(1, 5)), "H": H, "W": W, "Cin": 32 * int(r.randint(1, 7)),
                    "Cb": int(r.choice([64, 128, 192, 320])), "Kout": int(r.choice([64, 128, 192, 256]))}
        sh = _draw(rng, make, lambda sh: macs(Case(entry, sh)) <= SEG_MACS / 2, entry, ASPP_PINS[i % len(ASPP_PINS)])
        sh["rates"] = rates
        cases.append(Case(entry, sh, None, None, {"nonneg": bool(i % 3 == 1)}))
    # the join's automatic stream-K form: more k-steps than the small draws reach
    cases.append(Case(entry, {"N": 3, "H": 12, "W": 12, "Cin": 32, "Cb": 192, "Kout": 64, "rates": (2, 13, 5)}, None, None,
                      {"nonneg": False}))
    return cases


# (N, h, w, Ho, Wo, C, ld): up by a fraction on both axes (Wo % 4 = 3, Ho % 8 != 0); up on one axis and down on the other;
# the identity; a mild down-scale; more than 4x down on one axis only; one-line and one-pixel inputs and outputs; two
# x-segments of an odd width; the direct form past 256 columns; N >= 3
RESIZE_SHAPES = [
    (2, 9, 7, 23, 19, 21, 24), (1, 8, 12, 20, 5, 5, 8), (1, 9, 9, 9, 9, 4, 4), (2, 12, 10, 5, 7, 64, 64),
    (2, 40, 6, 8, 9, 8, 16), (3, 1, 7, 5, 13, 3, 4), (1, 6, 1, 11, 2, 2, 4), (2, 5, 9, 1, 17, 6, 8), (2, 7, 4, 9, 1, 1, 4),
    (1, 3, 40, 9, 301, 2, 4), (1, 30, 70, 5, 259, 3, 4), (3, 5, 3, 33, 49, 5, 8), (1, 4, 90, 12, 19, 12, 20),
    (2, 6, 5, 14, 518, 3, 12),
]
LDS_MAP = (6, 40, 9, 64)   # (h, w, Ho, Wo) of the case that is direct because no block fits in LDS


def resize_cases():
    rng = np.random.RandomState(6565)
    entry = "resize_bilinear"
    shapes = [dict(zip(("N", "h", "w", "Ho", "Wo", "C", "ld"), s)) for s in RESIZE_SHAPES]
    h, w, Ho, Wo = LDS_MAP
    C = smallest_direct_channels(_pkg(), h, w, Ho, Wo)
    shapes.append({"N": 1, "h": h, "w": w, "Ho": Ho, "Wo": Wo, "C": C, "ld": C})
    for _ in range(7):
        C = int(rng.randint(1, 25))
        shapes.append({"N": int(rng.randint(1, 4)), "h": int(rng.randint(1, 13)), "w": int(rng.randint(1, 13)),
                       "Ho": int(rng.randint(1, 41)), "Wo": int(rng.randint(1, 41)), "C": C,
                       "ld": (C + 3) // 4 * 4 + int(rng.choice([0, 4, 8]))})
    cases = []
    for i, sh in enumerate(shapes):
        sh["outputs"] = ("both", "out", "labels")[i % 3]
        cases.append(Case(entry, sh, None, None, {"in_padded": bool((i // 3) % 2)}))
    return cases


# ---- the grouped 3x3 and the two ResNeXt blocks ------------------------------------------------------------------------
GROUPED_CGS = (4, 8, 16, 32, 64)
# rows of a workgroup's output tile, by (stride, tile width): wino_conv3x3_grouped_plan names the width, the kernel's
# header comment (conv3x3_grouped.hip) the rows: four 16-pixel row tiles at stride 1, two at stride 2
GROUPED_TILE_H = {(1, 16): 4, (1, 8): 8, (2, 16): 2, (2, 8): 4}


def grouped_out(Hin, Win, stride):
    return (Hin - 1) // stride + 1, (Win - 1) // stride + 1


def grouped_form(pkg, N, Hin, Win, C, groups, stride):
    """The kernel instantiation of the grouped layer, by name, and the plan query's four answers."""
    tw, kc, ty, tx = pkg.conv3x3_grouped_plan(N, Hin, Win, C, groups, stride)
    return {"form": f"s{stride}_tw{tw}_kc{kc}", "tw": tw, "kc": kc, "tiles_y": ty, "tiles_x": tx}


def _grouped_map(r, stride, tw, pin, k):
    """(Hin, Win) whose output takes `tw`-wide tiles.  pin["many"]: at least two tiles down and across, the last ones
    exactly full (pin["full"]) or clipped; pin["H"] / pin["W"] / pin["Hin"] / pin["Win"]: that size; k: two bits, the
    parities of a stride-2 input."""
    oh = GROUPED_TILE_H[(stride, tw)]
    if pin.get("many"):
        lo, hi = (17, 24) if tw == 8 else (25, 32)     # (9 .. 16 wide takes one 16-wide tile, not two 8-wide ones)
        rows = int(r.randint(2, 4))
        W = hi if pin.get("full") else int(r.randint(lo, hi))
        H = rows * oh if pin.get("full") else (rows - 1) * oh + int(r.randint(1, oh))
    else:
        lo, hi = (1, 8) if tw == 8 else (9, 16)
        W, H = int(r.randint(lo, hi + 1)), int(r.randint(1, 2 * oh + 2))
    H, W = pin.get("H", H), pin.get("W", W)
    if pin.get("odd"):
        H, W = H | 1, W - 1 + W % 2
    if stride == 1:
        return H, W
    return pin.get("Hin", 2 * H - 1 + (k & 1)), pin.get("Win", 2 * W - 1 + (k >> 1 & 1))


# (stride, tile width, Cg, pins): every instantiation at least once, Cg = 4, 8, 16 (one select each) at both widths, and
# per (stride, width) one map of full tiles and one of clipped ones, two or more down and across; one-line outputs,
# a 1x1 output of a 2x2 input, the dense C = 64 layer, three channel blocks, three images
GROUPED_ROWS = [
    (1, 16, 4, {"many": True, "full": True}), (1, 16, 8, {"many": True}), (1, 16, 16, {"H": 1}),
    (1, 16, 32, {"many": True, "N": 3, "C": 192}), (1, 16, 64, {"C": 64}),
    (1, 8, 4, {"many": True, "full": True}), (1, 8, 8, {"many": True}), (1, 8, 16, {"W": 1}), (1, 8, 32, {"odd": True}),
    (1, 8, 64, {"many": True, "C": 192}),
    (2, 16, 4, {"many": True, "full": True}), (2, 16, 8, {"many": True}), (2, 16, 16, {"Hin": 2}),
    (2, 16, 32, {"many": True, "N": 3}), (2, 16, 64, {"C": 256}),
    (2, 8, 4, {"many": True, "full": True}), (2, 8, 8, {"many": True}), (2, 8, 16, {"Win": 1, "N": 4}), (2, 8, 32, {"C": 64}),
    (2, 8, 64, {"C": 64, "Hin": 2, "Win": 2}),
]


def grouped_cases():
    rng = np.random.RandomState(7171)
    entry = "conv3x3_grouped_bn_relu"
    cases = []
    for i, (stride, tw, Cg, pin) in enumerate(GROUPED_ROWS):
        Hin, Win = _grouped_map(rng, stride, tw, pin, i)
        C = pin.get("C") or int(rng.choice([c for c in (64, 128, 192, 256) if c % Cg == 0]))
        sh = {"N": pin.get("N") or int(rng.randint(1, 4)), "Hin": Hin, "Win": Win, "C": C, "groups": C // Cg, "stride": stride}
        cases.append(Case(entry, sh, None, None, _flags(rng, i)))
    for i in range(len(cases), len(cases) + 10):   # the whole envelope: whatever instantiation the shape takes
        Cg = int(rng.choice(GROUPED_CGS))
        C = 64 * int(rng.randint(1, 5))
        sh = {"N": int(rng.randint(1, 5)), "Hin": int(rng.randint(1, 41)), "Win": int(rng.randint(1, 67)), "C": C,
              "groups": C // Cg, "stride": int(rng.randint(1, 3))}
        cases.append(Case(entry, sh, None, None, _flags(rng, i)))
    return cases


GBLOCK_FORMS = V15_FORMS
# one pin per (Cg, block) draw, in the order the generator walks them
GBLOCK_PINS = [{"H": 1}, {"W": 1}, {"odd": True}, {"Cm": 64}, {"Cm": 192}, {"C4": 192}, {"odd": True}, {"Cin": 96},
               {"Cm": 64, "H": 1}, {"Cm": 192, "C4": 320}, {"Cin": 160, "Cm": 128, "C4": 320}, {"W": 1}, {"Cm": 64}, {"N": 3},
               {"Cm": 192}]
# (N, Hin, Win, Cin, Cm, C4, groups, stride, proj): both 1x1 launches in the forced form
GBLOCK_FORCED = [
    ((2, 12, 12, 256, 128, 256, 32, 1, False), "stream_k"), ((3, 10, 12, 128, 128, 256, 16, 1, True), "stream_k"),
    ((2, 19, 24, 128, 64, 256, 4, 2, True), "stream_k"), ((2, 9, 9, 256, 64, 256, 2, 1, False), "tiled"),
    ((1, 7, 11, 128, 64, 192, 1, 2, True), "tiled"),
]
GBLOCK_KEYS = ("N", "Hin", "Win", "Cin", "Cm", "C4", "groups", "stride", "proj")


def grouped_block_cases():
    rng = np.random.RandomState(7272)
    entry = "grouped_block"
    cases = []
    for i, (Cg, (proj, stride)) in enumerate((Cg, kind) for Cg in GROUPED_CGS for kind in ((False, 1), (True, 1), (True, 2))):
        pin = GBLOCK_PINS[i]
        tw = 8 if pin.get("W") == 1 else (8, 16)[i % 2]
        for _ in range(4000):
            Hin, Win = _grouped_map(rng, stride, tw, pin, i)
            Cm = pin.get("Cm") or int(rng.choice([c for c in (64, 128, 192, 256) if c % Cg == 0]))
            C4 = pin.get("C4") or 64 * int(rng.randint(1, 6))
            Cin = (pin.get("Cin") or 32 * int(rng.randint(1, 9))) if proj else C4
            if not proj or len({Cin, Cm, C4}) == 3:
                break
        sh = {"N": pin.get("N") or int(rng.randint(1, 4)), "Hin": Hin, "Win": Win, "Cin": Cin, "Cm": Cm, "C4": C4,
              "groups": Cm // Cg, "stride": stride, "proj": proj}
        cases.append(Case(entry, sh, None, None, {"nonneg": bool(i % 3 == 1)}))
    # the automatic whole-tile form of the last 1x1 launch: a batch past its latency form
    cases.append(Case(entry, dict(zip(GBLOCK_KEYS, (8, 20, 21, 64, 64, 320, 16, 1, True))), None, None, {"nonneg": True}))
    for shape, form in GBLOCK_FORCED:
        cases.append(Case(entry, dict(zip(GBLOCK_KEYS, shape)), dict(GBLOCK_FORMS[form]), form,
                          {"nonneg": bool(len(cases) % 3 == 1)}))
    return cases


# ---- one level of the Feature Pyramid Network ---------------------------------------------------------------------------
# the forced forms of the level's second launch, the Winograd 3x3 Cf -> Cf: the throughput kernel with and without a
# stream-K tail, the latency kernel without and with a C split (the knob sets of nonfinite.forms_3x3, spelt out by
# fpn_out_knobs); the first launch, the lateral 1x1 with the top-down read, takes the forms of forms_1x1.FORMS
FPN_OUT_FORMS = ("auto", "big_tail", "big_whole", "small_split1", "small_split2")
FPN_CIN, FPN_CF = (32, 96, 160, 256), (64, 128, 192, 256)
# H = 1, W = 1, odd x odd (the last row and column read a coarse pixel alone), every Cin and three Cf
FPN_PINS = [{"H": 1, "Cin": 32}, {"W": 1, "Cf": 64}, {"odd": True, "Cin": 96, "Cf": 192}, {"Cin": 160, "Cf": 128},
            {"Cin": 256, "Cf": 192}, {"odd": True, "Cf": 64}, {"Cin": 32, "Cf": 128}, {"N": 6, "Cin": 96}]
FPN_MACS = MAX_MACS / 4
# the automatic forms no draw of the envelope takes: the stream-K lateral needs more k-steps (Cin = 512), the throughput
# 3x3 more tiles than six images have
FPN_AUTO = [{"N": 6, "H": 40, "W": 40, "Cin": 512, "Cf": 64}, {"N": 72, "H": 16, "W": 15, "Cin": 32, "Cf": 64}]


def fpn_lateral_forms():
    import forms_1x1   # (forms_1x1 imports this module)
    return forms_1x1.FORMS


def fpn_lateral_legal(form, sh):
    """Whether the lateral GEMM of the shape can take the forced form: the latency kernel's divisibility rules
    (conv1x1.hip small1_legal), a stream-K grid with a range for every column block."""
    import forms_1x1
    kn = forms_1x1.FORMS[form]
    M, Cin, Cf = sh["N"] * sh["H"] * sh["W"], sh["Cin"], sh["Cf"]
    if form.startswith("latency"):
        ks, ct = kn["WINO_1X1_SMALL_KS"], kn["WINO_1X1_SMALL_CT"]
        return Cin % (16 * ks) == 0 and Cf % ((4 // ks) * ct * 16) == 0 and not (ks > 1 and Cin // ks < 64)
    if form.startswith("sk"):
        return forms_1x1.sk_plan(M, Cin, Cf, kn["WINO_1X1_SK_GRID"])[0]
    return True


def fpn_out_knobs(form, sh):
    items = _items_3x3(sh["N"], sh["H"], sh["W"], sh["Cf"])
    return {"auto": {},
            "big_tail": {"WINO_3X3_ALGO": "big", "WINO_SK_GRID": items + 1 + (items == 1)},
            "big_whole": {"WINO_3X3_ALGO": "big", "WINO_SK_GRID": items},
            "small_split1": {"WINO_3X3_ALGO": "small", "WINO_SMALL_CT": 1, "WINO_SMALL_SPLIT": 1},
            "small_split2": {"WINO_3X3_ALGO": "small", "WINO_SMALL_CT": 2, "WINO_SMALL_SPLIT": 2}}[form]


def fpn_forms():
    """(lateral form, 3x3 form) of every forced case: each lateral form once, the 3x3 forms in turn beside them."""
    laterals = [f for f in fpn_lateral_forms() if f != "auto"]
    return [(lat, FPN_OUT_FORMS[i % len(FPN_OUT_FORMS)]) for i, lat in enumerate(laterals)]


def fpn_level_cases():
    rng = np.random.RandomState(7373)
    entry = "fpn_level"
    cases = []

    def make(r):
        return {"N": int(r.randint(1, 7)), "H": int(r.randint(1, 41)), "W": int(r.randint(1, 41)),
                "Cin": int(r.choice(FPN_CIN)), "Cf": int(r.choice(FPN_CF))}

    def flags(i):
        return {"top": bool(i % 4 != 3), "c_padded": bool(i % 3 == 0), "nonneg": bool(i % 5 == 1)}

    pairs = [("auto", "auto")] * len(FPN_PINS) + fpn_forms()
    for i, (lat, out) in enumerate(pairs):
        ok = lambda sh: macs(Case(entry, sh)) <= FPN_MACS and fpn_lateral_legal(lat, sh)
        sh = _draw(rng, make, ok, entry, FPN_PINS[i % len(FPN_PINS)])
        knobs = {**fpn_lateral_forms()[lat], **fpn_out_knobs(out, sh)}
        cases.append(Case(entry, sh, knobs or None, f"{lat}+{out}" if knobs else None, flags(i)))
    for sh in FPN_AUTO:
        cases.append(Case(entry, dict(sh), None, None, flags(len(cases))))
    return cases


GENERATORS = {
    "fpn_level": fpn_level_cases,
    "conv3x3_grouped_bn_relu": grouped_cases,
    "grouped_block": grouped_block_cases,
    "conv3x3_dilated_bn_relu": dilated_cases,
    "dilated_block": dilated_block_cases,
    "conv1x1_cat_bn": cat_cases,
    "aspp": aspp_cases,
    "resize_bilinear": resize_cases,
    "conv3x3_bn_add_relu": residual_3x3_cases,
    "basic_block": basic_block_cases,
    "conv3x3_s2_bn_relu": conv3x3_s2_cases,
    "conv3x3_s2_proj": conv3x3_s2_proj_cases,
    "basic_block_s2": basic_block_s2_cases,
    "proj_block": proj_block_cases,
    "proj_block_v15": proj_block_v15_cases,
    "stem": stem_cases,
    "avgpool_fc": head_cases,
}


# ---- the plan queries ------------------------------------------------------------------------------------------------
FORM_NAMES = {0: "tiled", 1: "stream_k", 2: "latency"}


def form_1x1(pkg, M, Cin, Kout, cus=CUS):
    """The form the 1x1 planner gives a GEMM (M, Cin, Kout), by name."""
    if pkg.small_plan_1x1_full(M, Cin, Kout, cus)[0]:
        return "latency"
    v = [ctypes.c_int() for _ in range(5)]
    rc = pkg.lib().wino_conv1x1_plan(M, Cin, Kout, cus, *[ctypes.byref(x) for x in v])
    if rc:
        raise pkg.WinoError(f"wino_conv1x1_plan rc={rc}")
    return "stream_k" if v[4].value else "tiled"


def plan_3x3(pkg, N, H, W, C, K, cus=CUS):
    """(form, detail) of the Winograd 3x3: 'latency' with (split, col_tiles) or 'throughput' with (grid, tail)."""
    use, _, split, ct, _ = pkg.small_plan_3x3_full(N, C, K, cus, H=H, W=W)
    if use:
        return "latency", {"split": split, "ct": ct}
    grid, rounds, tail, it = ctypes.c_int(), ctypes.c_int(), ctypes.c_long(), ctypes.c_int()
    rc = pkg.lib().wino_conv3x3_plan(N, H, W, C, K, cus, ctypes.byref(grid), ctypes.byref(rounds), ctypes.byref(tail),
                                     ctypes.byref(it))
    if rc:
        raise pkg.WinoError(f"wino_conv3x3_plan rc={rc}")
    return "throughput", {"grid": grid.value, "tail": tail.value}


def plan_form(pkg, case, cus=CUS):
    """The form(s) the plan queries give the case (under the knobs currently set): a dict whose 'form' names the
    automatic form, plus whatever the case's forced form is checked against.  Raises WinoError on an illegal shape."""
    s, e = case.shape, case.entry
    if e in ("conv3x3_bn_add_relu", "basic_block"):
        K = s["K"] if e == "conv3x3_bn_add_relu" else s["C"]
        form, d = plan_3x3(pkg, s["N"], s["H"], s["W"], s["C"], K, cus)
        return {"form": form, **d}
    if e in ("conv3x3_s2_bn_relu", "conv3x3_s2_proj", "basic_block_s2"):
        form = FORM_NAMES[pkg.conv3x3_s2_plan(s["N"], s["Hin"], s["Win"], s["C"], s["K"], cus)]
        M = s["N"] * _s2(s["Hin"]) * _s2(s["Win"])
        d = {"form": form, "small": pkg.small_plan_1x1_full(M, 9 * s["C"], s["K"], cus)[1:4]}
        if e == "basic_block_s2":
            d["form_3x3"] = plan_3x3(pkg, s["N"], _s2(s["Hin"]), _s2(s["Win"]), s["K"], s["K"], cus)[0]
        return d
    if e == "proj_block":
        first, tail = pkg.proj_tail_plan(s["N"], s["Hin"], s["Win"], s["Cin"], s["Cm"], s["C4"], s["stride"], cus)
        st = s["stride"]
        H, W = (s["Hin"] - 1) // st + 1, (s["Win"] - 1) // st + 1
        return {"form": f"{FORM_NAMES[first]}/{FORM_NAMES[tail]}", "first": FORM_NAMES[first],
                "tail": FORM_NAMES[tail], "form_3x3": plan_3x3(pkg, s["N"], H, W, s["Cm"], s["Cm"], cus)[0]}
    if e == "proj_block_v15":
        first = form_1x1(pkg, s["N"] * s["Hin"] * s["Win"], s["Cin"], s["Cm"], cus)
        mid = FORM_NAMES[pkg.conv3x3_s2_plan(s["N"], s["Hin"], s["Win"], s["Cm"], s["Cm"], cus)]
        tail = FORM_NAMES[pkg.proj_tail_plan(s["N"], s["Hin"], s["Win"], s["Cin"], s["Cm"], s["C4"], 2, cus)[1]]
        return {"form": f"{first}/{mid}/{tail}", "first": first, "mid": mid, "tail": tail}
    if e == "stem":
        return {"form": {1: "big", 2: "small"}[pkg.stem_plan(s["N"], s["H"], s["W"], s["K"], cus)]}
    if e == "avgpool_fc":
        return {"form": form_1x1(pkg, s["N"], s["C"], head_cols(s["classes"]), cus)}
    if e == "conv3x3_dilated_bn_relu":
        form = FORM_NAMES[pkg.conv3x3_dilated_plan(s["N"], s["H"], s["W"], s["C"], s["K"], s["d"], cus)]
        return {"form": form, **sk_ranges(pkg, s["N"] * s["H"] * s["W"], 9 * s["C"], s["K"], s["C"] // 32, cus)}
    if e == "dilated_block":
        M = s["N"] * s["H"] * s["W"]
        first = form_1x1(pkg, M, s["Cin"], s["Cm"], cus)
        mid = FORM_NAMES[pkg.conv3x3_dilated_plan(s["N"], s["H"], s["W"], s["Cm"], s["Cm"], s["d"], cus)]
        if s["proj"]:
            tail = FORM_NAMES[pkg.proj_tail_plan(s["N"], s["H"], s["W"], s["Cin"], s["Cm"], s["C4"], 1, cus)[1]]
        else:
            tail = form_1x1(pkg, M, s["Cm"], s["C4"], cus)
        return {"form": f"{first}/{mid}/{tail}", "first": first, "mid": mid, "tail": tail}
    if e == "conv1x1_cat_bn":
        form = FORM_NAMES[pkg.conv1x1_cat_plan(s["N"], s["H"], s["W"], s["S"], s["Cs"], s["Kout"], cus)]
        return {"form": form, **sk_ranges(pkg, s["N"] * s["H"] * s["W"], s["S"] * s["Cs"], s["Kout"], s["Cs"] // 32, cus)}
    if e == "aspp":   # the join names the form; every other launch must be one the library plans
        for d in s["rates"]:
            pkg.conv3x3_dilated_plan(s["N"], s["H"], s["W"], s["Cin"], s["Cb"], d, cus)
        form_1x1(pkg, s["N"] * s["H"] * s["W"], s["Cin"], s["Cb"], cus)
        return {"form": FORM_NAMES[pkg.conv1x1_cat_plan(s["N"], s["H"], s["W"], 4, s["Cb"], s["Kout"], cus)]}
    if e == "conv3x3_grouped_bn_relu":
        return grouped_form(pkg, s["N"], s["Hin"], s["Win"], s["C"], s["groups"], s["stride"])
    if e == "grouped_block":   # the first 1x1 at the full input, the grouped 3x3 at the stride, the last 1x1 / the tail
        H, W = grouped_out(s["Hin"], s["Win"], s["stride"])
        first = form_1x1(pkg, s["N"] * s["Hin"] * s["Win"], s["Cin"], s["Cm"], cus)
        mid = grouped_form(pkg, s["N"], s["Hin"], s["Win"], s["Cm"], s["groups"], s["stride"])
        if s["proj"]:
            tail = FORM_NAMES[pkg.proj_tail_plan(s["N"], s["Hin"], s["Win"], s["Cin"], s["Cm"], s["C4"], s["stride"], cus)[1]]
        else:
            tail = form_1x1(pkg, s["N"] * H * W, s["Cm"], s["C4"], cus)
        return {"form": f"{first}/{mid['form']}/{tail}", "first": first, "mid": mid, "tail": tail}
    if e == "fpn_level":   # the lateral 1x1 (the top-down read does not alter its plan), then the Winograd 3x3 Cf -> Cf
        M = s["N"] * s["H"] * s["W"]
        lat = form_1x1(pkg, M, s["Cin"], s["Cf"], cus)
        out, d = plan_3x3(pkg, s["N"], s["H"], s["W"], s["Cf"], s["Cf"], cus)
        return {"form": f"{lat}/{out}", "lateral": lat, "small": pkg.small_plan_1x1_full(M, s["Cin"], s["Cf"], cus)[1:4],
                "grid_1x1": sk_ranges(pkg, M, s["Cin"], s["Cf"], 1, cus)["grid"], "out": {"form": out, **d}}
    if e == "resize_bilinear":
        form = pkg.resize_bilinear_plan(s["h"], s["w"], s["C"], s["ld"], s["Ho"], s["Wo"], s["outputs"] != "labels",
                                        s["outputs"] != "out")
        return {"form": {STAGED: "staged", DIRECT: "direct"}[form]}
    raise KeyError(e)


def check_forced(case, plan) -> str | None:
    """None when the plan takes the case's forced form, else what differs."""
    kn, f = case.knobs, case.form
    if kn is None:
        return None
    e = case.entry
    if e == "conv3x3_bn_add_relu":
        if f.startswith("big"):
            if plan["form"] != "throughput" or plan["grid"] != kn["WINO_SK_GRID"]:
                return f"want the throughput kernel at grid {kn['WINO_SK_GRID']}, plan {plan}"
            if (plan["tail"] > 0) != (f == "big_tail"):
                return f"want {'a' if f == 'big_tail' else 'no'} stream-K tail, plan {plan}"
            return None
        want = {"form": "latency", "split": kn["WINO_SMALL_SPLIT"], "ct": kn["WINO_SMALL_CT"]}
        return None if plan == want else f"want {want}, plan {plan}"
    if e in ("conv3x3_s2_bn_relu", "conv3x3_s2_proj"):
        want = f.split("_")[0]
        want = {"latency": "latency", "tiled": "tiled"}.get(want, "stream_k")
        if plan["form"] != want:
            return f"want {want}, plan {plan}"
        if want == "latency":
            ksrc = (kn["WINO_1X1_SMALL_KS"], kn["WINO_1X1_SMALL_RT"], kn["WINO_1X1_SMALL_CT"])
            if tuple(plan["small"]) != ksrc:
                return f"want latency (ks, rt, ct) = {ksrc}, plan {plan}"
        return None
    if e == "proj_block":
        want = {"latency": "latency", "tiled": "tiled"}.get(f.split("_")[0], "stream_k")
        return None if (plan["first"], plan["tail"]) == (want, want) else f"want {want} for both, plan {plan}"
    if e == "proj_block_v15":
        ok = (plan["first"], plan["mid"], plan["tail"]) == (f, f, f)
        return None if ok else f"want {f} for all three launches, plan {plan}"
    if e == "stem":
        return None if plan["form"] == f else f"want {f}, plan {plan}"
    if e == "avgpool_fc":
        return None if plan["form"] == f else f"want {f}, plan {plan}"
    if e in ("conv3x3_dilated_bn_relu", "conv1x1_cat_bn"):
        want = "tiled" if f == "tiled" else "stream_k"
        if plan["form"] != want:
            return f"want {want}, plan {plan}"
        if "WINO_1X1_SK_GRID" in kn and not 0 < plan["grid"] <= kn["WINO_1X1_SK_GRID"]:
            return f"want a stream-K grid of at most {kn['WINO_1X1_SK_GRID']}, plan {plan}"
        return None
    if e == "dilated_block":
        ok = (plan["first"], plan["mid"], plan["tail"]) == (f, f, f)
        return None if ok else f"want {f} for all three launches, plan {plan}"
    if e == "grouped_block":   # (the grouped 3x3 has one form per shape: nothing to force)
        return None if (plan["first"], plan["tail"]) == (f, f) else f"want {f} for both 1x1 launches, plan {plan}"
    if e == "fpn_level":
        lat, out = f.split("+")
        if lat == "tiled" and plan["lateral"] != "tiled":
            return f"want a tiled lateral, plan {plan}"
        if lat.startswith("sk") and not (plan["lateral"] == "stream_k" and 0 < plan["grid_1x1"] <= kn["WINO_1X1_SK_GRID"]):
            return f"want a stream-K lateral of at most {kn['WINO_1X1_SK_GRID']} workgroups, plan {plan}"
        if lat.startswith("latency"):
            ksrc = (kn["WINO_1X1_SMALL_KS"], kn["WINO_1X1_SMALL_RT"], kn["WINO_1X1_SMALL_CT"])
            if plan["lateral"] != "latency" or tuple(plan["small"]) != ksrc:
                return f"want a latency lateral with (ks, rt, ct) = {ksrc}, plan {plan}"
        o = plan["out"]
        if out.startswith("big"):
            if o["form"] != "throughput" or o["grid"] != kn["WINO_SK_GRID"] or (o["tail"] > 0) != (out == "big_tail"):
                return f"want the 3x3 throughput kernel at grid {kn['WINO_SK_GRID']} ({out}), plan {plan}"
        if out.startswith("small"):
            want = {"form": "latency", "split": kn["WINO_SMALL_SPLIT"], "ct": kn["WINO_SMALL_CT"]}
            if o != want:
                return f"want the 3x3 as {want}, plan {plan}"
        return None
    raise KeyError(e)


def sizes(pkg, case) -> dict:
    """The pack / workspace size queries of the case's entry point (0 marks a shape the library refuses)."""
    L, s, e = pkg.lib(), case.shape, case.entry
    if e == "conv3x3_bn_add_relu":
        return {"U": L.wino_filter_f2_elems(s["C"], s["K"])}
    if e == "basic_block":
        return {"U": L.wino_filter_f2_elems(s["C"], s["C"]),
                "workspace": L.wino_basic_block_workspace_bytes_hw(s["N"], s["H"], s["W"], s["C"])}
    if e == "conv3x3_s2_bn_relu":
        return {"packed": L.wino_s2_proj_elems(s["C"], s["K"])}   # (the plain layer takes w.permute(2, 3, 1, 0))
    if e == "conv3x3_s2_proj":
        return {"packed": L.wino_s2_proj_elems(s["C"], s["K"])}
    if e == "basic_block_s2":
        return {"packed": L.wino_s2_proj_elems(s["C"], s["K"]), "U2": L.wino_filter_f2_elems(s["K"], s["K"]),
                "workspace": L.wino_basic_block_s2_workspace_bytes_hw(s["N"], s["Hin"], s["Win"], s["K"])}
    if e == "proj_block":
        st = s["stride"]
        H, W = (s["Hin"] - 1) // st + 1, (s["Win"] - 1) // st + 1
        return {"tail": L.wino_proj_tail_elems(s["Cm"], s["Cin"], s["C4"]),
                "U2": L.wino_filter_f2_elems(s["Cm"], s["Cm"]),
                "workspace": L.wino_proj_block_workspace_bytes_hw(s["N"], H, W, s["Cm"])}
    if e == "proj_block_v15":
        return {"tail": L.wino_proj_tail_elems(s["Cm"], s["Cin"], s["C4"]),
                "workspace": L.wino_proj_block_v15_workspace_bytes_hw(s["N"], s["Hin"], s["Win"], s["Cm"])}
    if e == "stem":
        return {"packed": L.wino_stem_filter_elems(s["K"])}
    if e == "avgpool_fc":
        return {"packed": L.wino_head_elems(s["C"], s["classes"]),
                "workspace": L.wino_head_workspace_bytes(s["N"], s["C"], s["classes"])}
    if e == "dilated_block":
        q = L.wino_proj_block_workspace_bytes_hw if s["proj"] else L.wino_residual_block_workspace_bytes_hw
        d = {"workspace": q(s["N"], s["H"], s["W"], s["Cm"])}
        if s["proj"]:
            d["tail"] = L.wino_proj_tail_elems(s["Cm"], s["Cin"], s["C4"])
        return d
    if e == "conv3x3_grouped_bn_relu":
        return {"packed": L.wino_conv3x3_grouped_filter_elems(s["C"], s["groups"])}
    if e == "grouped_block":
        d = {"wg": L.wino_conv3x3_grouped_filter_elems(s["Cm"], s["groups"]), "workspace": grouped_block_workspace(pkg, case)[1]}
        if s["proj"]:
            d["tail"] = L.wino_proj_tail_elems(s["Cm"], s["Cin"], s["C4"])
        return d
    if e == "aspp":
        return {"workspace": pkg.aspp_workspace_bytes(s["N"], s["H"], s["W"], s["Cin"], s["Cb"], s["Kout"])}
    if e == "fpn_level":
        return {"U": L.wino_filter_f2_elems(s["Cf"], s["Cf"])}
    if e in ("conv3x3_dilated_bn_relu", "conv1x1_cat_bn", "resize_bilinear"):
        return {}   # (no pack or workspace query of their own)
    raise KeyError(e)


def grouped_block_workspace(pkg, case):
    """(the dense block's size query that sizes the grouped block's workspace, its answer)."""
    s, L = case.shape, pkg.lib()
    H, W = grouped_out(s["Hin"], s["Win"], s["stride"])
    if not s["proj"]:
        query, args = "wino_residual_block_workspace_bytes_hw", (s["N"], s["Hin"], s["Win"], s["Cm"])
    elif s["stride"] == 1:
        query, args = "wino_proj_block_workspace_bytes_hw", (s["N"], H, W, s["Cm"])
    else:
        query, args = "wino_proj_block_v15_workspace_bytes_hw", (s["N"], s["Hin"], s["Win"], s["Cm"])
    return query, getattr(L, query)(*args)


def sk_ranges(pkg, M, Cin, Kout, unit, cus=CUS) -> dict:
    """The stream-K ranges of the GEMM (M, Cin, Kout) under the knobs currently set, as centre_tap_split reads them off
    wino_conv1x1_plan: the grid, and how many range boundaries fall strictly inside a unit of `unit` k-steps (a tap of
    the dilated layer, a source of the concat layer) and how many exactly between two units of one tile.  Zeros for
    whole tiles."""
    v = [ctypes.c_int() for _ in range(5)]
    rc = pkg.lib().wino_conv1x1_plan(M, Cin, Kout, cus, *[ctypes.byref(x) for x in v])
    if rc:
        raise pkg.WinoError(f"wino_conv1x1_plan rc={rc}")
    grid, row_tiles, col_blocks, k_steps, sk = (x.value for x in v)
    if not sk:
        return {"grid": 0, "inside": 0, "between": 0}
    R, T = grid // col_blocks, row_tiles * k_steps
    pos = [(r * T // R) % k_steps for r in range(1, R)]
    return {"grid": grid, "inside": sum(1 for p in pos if p % unit), "between": sum(1 for p in pos if p and p % unit == 0)}


def centre_tap_split(pkg, case, cus=CUS) -> bool:
    """Whether the stream-K launch of a stride-2 case (under the knobs currently set) has a range boundary strictly
    inside the centre tap's k-range [4C, 5C) -- where the fused layer's shortcut workgroups start and stop."""
    s = case.shape
    M, C = s["N"] * _s2(s["Hin"]) * _s2(s["Win"]), s["C"]
    v = [ctypes.c_int() for _ in range(5)]
    if pkg.lib().wino_conv1x1_plan(M, 9 * C, s["K"], cus, *[ctypes.byref(x) for x in v]):
        return False
    grid, row_tiles, col_blocks, k_steps, sk = (x.value for x in v)
    if not sk or pkg.small_plan_1x1_full(M, 9 * C, s["K"], cus)[0]:
        return False
    R, T = grid // col_blocks, row_tiles * k_steps
    lo, hi = 4 * C // 32, 5 * C // 32
    return any(lo < (r * T // R) % k_steps < hi for r in range(1, R))
