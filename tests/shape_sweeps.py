"""Seeded random-shape generators for the ResNet entry points, shared by tests/test_shape_sweeps_host.py (every case is
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

MAX_MACS = 2e9
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


GENERATORS = {
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
    raise KeyError(e)


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
