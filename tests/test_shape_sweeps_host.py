"""Host-side checks (no GPU) of the seeded shape sweeps in tests/shape_sweeps.py that tests/test_gpu_shape_sweeps.py
runs: every drawn case is one the library accepts, in the form it was drawn for (so a GPU sweep never skips a shape or
turns it into a WinoError), and the draws of each entry point reach the corners they exist for.  A generator edit that
loses a corner fails here and names it.  For the segmentation entries the conditions their GPU sweeps lean on are proven
here on the fp64 references of the very tensors the sweeps draw: ASPP's pooled branch carries weight in every image of
every case, and the label gap rule leaves out at most 1 % of any resize case's pixels."""
import numpy as np
import pytest

import resize_cases as RC
import shape_sweeps as S
import sweep_cases as SC
from cases import TIGHT

ENTRIES = sorted(S.GENERATORS)


def _with_knobs(knobs, case, fn):
    """fn() with the case's forced knobs set (the planner reads them), unset again afterwards."""
    for k, v in (case.knobs or {}).items():
        knobs.set(k, v)
    try:
        return fn()
    finally:
        for k in case.knobs or {}:
            knobs.unset(k)


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_drawn_case_is_legal(entry, pkg, knobs):
    cases = S.GENERATORS[entry]()
    assert 12 <= len(cases) <= 40, f"{entry}: {len(cases)} cases"
    assert cases == S.GENERATORS[entry](), f"{entry}: the generator is not deterministic"
    for c in cases:
        assert c.entry == entry
        assert S.macs(c) <= S.MAX_MACS, f"{c.tag()}: fp64 reference of {S.macs(c):.2e} multiply-adds"
        plan = _with_knobs(knobs, c, lambda: S.plan_form(pkg, c))
        bad = S.check_forced(c, plan)
        assert bad is None, f"{c.tag()}: the planner does not take the forced form: {bad}"
        for name, n in S.sizes(pkg, c).items():
            assert n > 0, f"{c.tag()}: size query {name} is 0 (a shape the library refuses)"
    if entry in SC.SEEDS:   # the segmentation entries: all references of a sweep together stay in seconds
        total = sum(S.macs(c) for c in cases)
        assert total < S.MAX_SUM_MACS, f"{entry}: {total:.2e} multiply-adds in all"


def _map_hw(c):
    """The (output) map the case's kernel walks, and the input map."""
    s = c.shape
    if c.entry in ("conv3x3_s2_bn_relu", "conv3x3_s2_proj", "basic_block_s2", "proj_block_v15"):
        return (S._s2(s["Hin"]), S._s2(s["Win"])), (s["Hin"], s["Win"])
    if c.entry in ("proj_block", "conv3x3_grouped_bn_relu", "grouped_block"):
        st = s["stride"]
        return ((s["Hin"] - 1) // st + 1, (s["Win"] - 1) // st + 1), (s["Hin"], s["Win"])
    if c.entry == "stem":
        return S.stem_out(s["H"], s["W"]), (s["H"], s["W"])
    if c.entry == "resize_bilinear":
        return (s["Ho"], s["Wo"]), (s["h"], s["w"])
    return (s["H"], s["W"]), (s["H"], s["W"])


def _channels(c):
    """(input channel counts, output channel counts) of the case."""
    s = c.shape
    return {
        "conv3x3_bn_add_relu": ([s.get("C")], [s.get("K")]),
        "basic_block": ([s.get("C")], [s.get("C")]),
        "proj_block": ([s.get("Cin")], [s.get("Cm"), s.get("C4")]),
        "proj_block_v15": ([s.get("Cin")], [s.get("Cm"), s.get("C4")]),
        "stem": ([], [s.get("K")]),
        "avgpool_fc": ([s.get("C")], []),
        "dilated_block": ([s.get("Cin")], [s.get("Cm"), s.get("C4")]),
        "conv1x1_cat_bn": ([s.get("Cs")], [s.get("Kout")]),
        "aspp": ([s.get("Cin")], [s.get("Cb"), s.get("Kout")]),
        "resize_bilinear": ([], []),
        "conv3x3_grouped_bn_relu": ([s.get("C")], [s.get("C")]),
        "grouped_block": ([s.get("Cin")], [s.get("Cm"), s.get("C4")]),
        "fpn_level": ([s.get("Cin")], [s.get("Cf")]),
    }.get(c.entry, ([s.get("C")], [s.get("K")]))


# the automatic forms the planner picks for each entry point, by launch ('a/b' forms are split at '/')
AUTO_FORMS = {
    "conv3x3_bn_add_relu": [{"latency", "throughput"}],
    "basic_block": [{"latency", "throughput"}],
    "conv3x3_s2_bn_relu": [{"latency", "tiled", "stream_k"}],
    "conv3x3_s2_proj": [{"latency", "tiled", "stream_k"}],
    "basic_block_s2": [{"latency", "tiled", "stream_k"}],
    "proj_block": [{"latency", "tiled", "stream_k"}, {"latency", "tiled", "stream_k"}],
    "proj_block_v15": [{"latency", "tiled", "stream_k"}] * 3,
    "stem": [{"big", "small"}],
    "avgpool_fc": [{"latency", "stream_k"}],
    "conv3x3_dilated_bn_relu": [{"tiled", "stream_k"}],
    "dilated_block": [{"latency"}, {"tiled", "stream_k"}, {"latency", "tiled"}],
    "conv1x1_cat_bn": [{"tiled", "stream_k"}],
    "aspp": [{"tiled", "stream_k"}],          # (the join's form)
    "resize_bilinear": [{"staged", "direct"}],
    # all twelve instantiations of the one kernel body
    "conv3x3_grouped_bn_relu": [{f"s{st}_tw{tw}_kc{kc}" for st in (1, 2) for tw in (8, 16) for kc in (16, 32, 64)}],
    "grouped_block": [{"latency"}, set(), {"latency", "tiled"}],   # (the middle launch: _grouped_block_corners)
    "fpn_level": [{"latency", "tiled", "stream_k"}, {"latency", "throughput"}],
}
FORCED_FORMS = {
    "conv3x3_bn_add_relu": {"big_tail", "big_whole", "small"},
    "basic_block": set(),
    "conv3x3_s2_bn_relu": set(S.S2_FORMS),
    "conv3x3_s2_proj": set(S.S2_FORMS),
    "basic_block_s2": set(),
    "proj_block": set(S.PROJ_FORMS),
    "proj_block_v15": set(S.V15_FORMS),
    "stem": {"big", "small"},
    "avgpool_fc": set(S.HEAD_FORMS),
    "conv3x3_dilated_bn_relu": set(S.DIL_FORMS),
    "dilated_block": set(S.BLOCK_FORMS),
    "conv1x1_cat_bn": set(S.DIL_FORMS),
    "aspp": set(),
    "resize_bilinear": set(),
    "conv3x3_grouped_bn_relu": set(),
    "grouped_block": set(S.GBLOCK_FORMS),
    "fpn_level": {f"{lat}+{out}" for lat, out in S.fpn_forms()},
}
FLAGS = {
    "conv3x3_bn_add_relu": ("relu", "in_place", "nonneg"),
    "basic_block": ("in_place", "nonneg"),
    "conv3x3_s2_bn_relu": ("relu", "nonneg"),
    "conv3x3_s2_proj": ("nonneg",),
    "basic_block_s2": ("nonneg",),
    "proj_block": ("nonneg",),
    "proj_block_v15": ("nonneg",),
    "stem": ("padded",),
    "avgpool_fc": ("padded",),
    "conv3x3_dilated_bn_relu": ("relu", "nonneg"),
    "dilated_block": ("nonneg",),
    "conv1x1_cat_bn": ("relu", "a_padded", "c_padded", "nonneg"),
    "aspp": ("nonneg",),
    "resize_bilinear": ("in_padded",),
    "conv3x3_grouped_bn_relu": ("relu", "nonneg"),
    "grouped_block": ("nonneg",),
    "fpn_level": ("top", "c_padded", "nonneg"),
}


def _dil_windows(c):
    """(some tile's window is clipped at neither end, the whole tensor lies inside one tile's window) of a dilated case:
    a tile's window reaches d (W + 3) padded pixels before its first row's centre pixel and behind its last row's."""
    N, H, W, d = c.N, c.H, c.W, c.d
    Wp, M = W + 2, N * H * W
    img = (H + 2) * Wp
    total, reach = N * img, d * (W + 3)

    def ppix(m):
        n, r = divmod(m, H * W)
        y, x = divmod(r, W)
        return n * img + (1 + y) * Wp + 1 + x

    tiles = [(ppix(t), ppix(min(t + 111, M - 1))) for t in range(0, M, 112)]
    neither = any(a > reach and total - 1 - b > reach for a, b in tiles)
    whole = len(tiles) == 1 and tiles[0][0] <= reach and total - 1 - tiles[0][1] <= reach
    return neither, whole


def _sk(pkg, knobs, c, key):
    """A count of plan_form's stream-K ranges of a forced-grid case (0 for every other case)."""
    if not (c.knobs and "WINO_1X1_SK_GRID" in c.knobs):
        return 0
    return _with_knobs(knobs, c, lambda: S.plan_form(pkg, c))[key]


CLASS_NAMES = ["d < min(H, W)", "W <= d < H", "H <= d < W", "d >= max(H, W)"]


def _dilated_corners(cases, pkg, knobs):
    got = {f"a dilation with {CLASS_NAMES[k]}": any(S.dil_class(c.H, c.W, c.d) == k for c in cases) for k in range(4)}
    got["d = 1"] = any(c.d == 1 for c in cases)
    got["the largest dilation a wide map (W >= 2000, H <= 3, C = 32) takes"] = any(
        c.W >= 2000 and c.H <= 3 and c.C == 32 and c.d == S.largest_dilation(pkg, c.N, c.H, c.W, c.C, c.K) for c in cases)
    got["H = 1 with W > d"] = any(c.H == 1 and c.W > c.d for c in cases)
    got["W = 1 with H > d"] = any(c.W == 1 and c.H > c.d for c in cases)
    got["a tile over three images (H*W < 38, N >= 3)"] = any(c.H * c.W < 38 and c.N >= 3 for c in cases)
    got["C = 32"] = any(c.C == 32 for c in cases)
    got["C / 32 odd and > 1"] = any(c.C // 32 > 1 and (c.C // 32) % 2 for c in cases)
    got["C >= 512"] = any(c.C >= 512 for c in cases)
    got["K = 320"] = any(c.K == 320 for c in cases)
    got["a forced stream-K range boundary strictly inside a tap"] = any(_sk(pkg, knobs, c, "inside") for c in cases)
    got["a forced stream-K range boundary exactly on a tap boundary"] = any(_sk(pkg, knobs, c, "between") for c in cases)
    windows = [_dil_windows(c) for c in cases]
    got["a tile's window clipped at neither end"] = any(w[0] for w in windows)
    got["the whole tensor inside one window"] = any(w[1] for w in windows)
    return got


def _block_corners(cases):
    got = {}
    for proj in (False, True):
        kind = "proj" if proj else "residual"
        mine = [c for c in cases if c.proj == proj]
        got[f"the {kind} block"] = bool(mine)
        got[f"three reach classes of d for the {kind} block"] = len({S.dil_class(c.H, c.W, c.d) for c in mine}) >= 3
        assert all(c.proj or c.Cin == c.C4 for c in mine)
    got["Cm = 64"] = any(c.Cm == 64 for c in cases)
    got["Cm % 128 != 0 and > 64"] = any(c.Cm % 128 and c.Cm > 64 for c in cases)
    got["C4 % 128 != 0"] = any(c.C4 % 128 for c in cases)
    return got


def _cat_corners(cases, pkg, knobs):
    got = {f"S = {n}": any(c.S == n for c in cases) for n in (2, 3, 5, 8)}

    def source(c):
        p = 2 if c.flags["a_padded"] else 0
        return c.N * (c.H + p) * (c.W + p) * c.Cs

    assert all(c.gap % 4 == 0 for c in cases)
    got["a gap of 0"] = any(c.gap == 0 for c in cases)
    got["a gap of 4 floats"] = any(c.gap == 4 for c in cases)
    got["a gap larger than a source"] = any(c.gap > source(c) for c in cases)
    got["Cs = 32"] = any(c.Cs == 32 for c in cases)
    got["Cs / 32 odd and > 1"] = any(c.Cs // 32 > 1 and (c.Cs // 32) % 2 for c in cases)
    got["Cs = 256"] = any(c.Cs == 256 for c in cases)
    got["M % 112 == 0"] = any((c.N * c.H * c.W) % 112 == 0 for c in cases)
    got["M % 112 != 0"] = any((c.N * c.H * c.W) % 112 for c in cases)
    got["H*W = 1 with N >= 8"] = any(c.H * c.W == 1 and c.N >= 8 for c in cases)
    got["1 < H*W < 112 with N >= 3"] = any(1 < c.H * c.W < 112 and c.N >= 3 for c in cases)
    got["a forced stream-K range boundary strictly inside a source"] = any(_sk(pkg, knobs, c, "inside") for c in cases)
    got["a forced stream-K range boundary exactly at a source boundary"] = any(_sk(pkg, knobs, c, "between") for c in cases)
    return got


def _aspp_corners(cases):
    past = lambda c: [d >= max(c.H, c.W) for d in c.rates]
    return {
        "ascending rates": any(c.rates[0] < c.rates[1] < c.rates[2] for c in cases),
        "non-ascending rates": any(c.rates[0] > c.rates[1] or c.rates[1] > c.rates[2] for c in cases),
        "two equal rates": any(len(set(c.rates)) == 2 for c in cases),
        "a rate >= the map on one branch only": any(sum(past(c)) == 1 for c in cases),
        "all three rates >= the map": any(all(past(c)) for c in cases),
        "H*W = 1": any(c.H * c.W == 1 for c in cases),
        "N >= 3": any(c.N >= 3 for c in cases),
        "Cin, Cb and Kout pairwise different": any(len({c.Cin, c.Cb, c.Kout}) == 3 for c in cases),
        "Cb = 64": any(c.Cb == 64 for c in cases),
        "Cb % 128 != 0 and > 64": any(c.Cb % 128 and c.Cb > 64 for c in cases),
    }


def _resize_corners(cases, pkg):
    form = {id(c): S.plan_form(pkg, c)["form"] for c in cases}
    down = lambda a, b: a > b          # an axis shrinks
    far = lambda a, b: a > 4 * b       # ... by more than 4x
    lds = any(c.C == c.ld == RC.smallest_direct_channels(pkg, c.h, c.w, c.Ho, c.Wo) and not far(c.h, c.Ho)
              and not far(c.w, c.Wo) and form[id(c)] == "direct" for c in cases if c.C >= 64)
    got = {
        "a non-integer up-scale on both axes": any(c.Ho > c.h and c.Wo > c.w and c.Ho % c.h and c.Wo % c.w for c in cases),
        "up on one axis and down on the other": any((c.Ho > c.h and down(c.w, c.Wo)) or (c.Wo > c.w and down(c.h, c.Ho))
                                                    for c in cases),
        "the identity": any((c.h, c.w) == (c.Ho, c.Wo) for c in cases),
        "a down-scale in (1, 4] (staged)": any(form[id(c)] == "staged" and (down(c.h, c.Ho) or down(c.w, c.Wo)) for c in cases),
        "a down-scale > 4 on exactly one axis (direct)": any(form[id(c)] == "direct" and far(c.h, c.Ho) != far(c.w, c.Wo)
                                                             for c in cases),
        "h = 1 or w = 1": any(1 in (c.h, c.w) for c in cases),
        "Ho = 1 or Wo = 1": any(1 in (c.Ho, c.Wo) for c in cases),
        "Wo < 4": any(c.Wo < 4 for c in cases),
        "two x-segments of an odd Wo in (256, 520]": any(256 < c.Wo <= 520 and c.Wo % 2 and form[id(c)] == "staged"
                                                         for c in cases),
        "Ho % 8 != 0 with Ho > 8": any(c.Ho % 8 and c.Ho > 8 for c in cases),
        "Wo > 256 in the direct form": any(c.Wo > 256 and form[id(c)] == "direct" for c in cases),
        "C = 1": any(c.C == 1 for c in cases),
        "C % 4 != 0": any(c.C % 4 for c in cases),
        "C == ld": any(c.C == c.ld for c in cases),
        "ld >= C + 8": any(c.ld >= c.C + 8 for c in cases),
        "direct because no block fits in LDS": lds,
        "N >= 3": any(c.N >= 3 for c in cases),
    }
    for r in (1, 2, 3):
        got[f"Wo % 4 = {r}"] = any(c.Wo % 4 == r for c in cases)
    for use in ("out", "labels", "both"):
        got[f"outputs: {use}"] = any(c.outputs == use for c in cases)
    return got


def _grouped_corners(cases, pkg):
    """The corners of the grouped layer's draws, every one read off wino_conv3x3_grouped_plan's answers."""
    rows = []
    for c in cases:
        p = S.plan_form(pkg, c)
        H, W = S.grouped_out(c.Hin, c.Win, c.stride)
        rows.append((c, p, H, W, S.GROUPED_TILE_H[(c.stride, p["tw"])], c.C // c.groups))
        assert p["tiles_x"] == -(-W // p["tw"]) and p["tiles_y"] == -(-H // rows[-1][4]), c.tag()
        assert p["kc"] == max(16, c.C // c.groups), c.tag()
    got = {}
    for tw in (8, 16):
        mine = [r for r in rows if r[1]["tw"] == tw]
        for Cg in (4, 8, 16):
            got[f"Cg = {Cg} at TW = {tw}"] = any(cg == Cg for *_, cg in mine)
        got[f"TW = {tw}: a clipped last x-tile"] = any(W % tw for _, _, _, W, _, _ in mine)
        got[f"TW = {tw}: a full last x-tile behind another"] = any(W % tw == 0 and p["tiles_x"] >= 2 for _, p, _, W, _, _ in mine)
        for st in (1, 2):
            pair = [r for r in mine if r[0].stride == st]
            got[f"stride {st}, TW = {tw}: two tiles down and across"] = any(p["tiles_x"] >= 2 and p["tiles_y"] >= 2
                                                                            for _, p, *_ in pair)
            got[f"stride {st}, TW = {tw}: a clipped last y-tile"] = any(H % oh for _, _, H, _, oh, _ in pair)
            got[f"stride {st}, TW = {tw}: a full last y-tile behind another"] = any(H % oh == 0 and p["tiles_y"] >= 2
                                                                                    for _, p, H, _, oh, _ in pair)
    s2 = [c for c in cases if c.stride == 2]
    for axis in ("Hin", "Win"):
        got[f"stride 2 with {axis} even"] = any(c.shape[axis] % 2 == 0 for c in s2)
        got[f"stride 2 with {axis} odd"] = any(c.shape[axis] % 2 for c in s2)
    got["an output with H = 1"] = any(H == 1 for _, _, H, _, _, _ in rows)
    got["an output with W = 1"] = any(W == 1 for _, _, _, W, _, _ in rows)
    got["Hin = 2 at stride 2"] = any(c.Hin == 2 for c in s2)
    got["C = 64 with groups = 1"] = any(c.C == 64 and c.groups == 1 for c in cases)
    got["C = 64"] = any(c.C == 64 for c in cases)
    got["C >= 192"] = any(c.C >= 192 for c in cases)
    got["N >= 3"] = any(c.N >= 3 for c in cases)
    return got


def _grouped_block_corners(cases, pkg):
    mids = [S.plan_form(pkg, c)["mid"] for c in cases]
    got = {"the residual block": any(not c.proj for c in cases)}
    assert all(c.proj or (c.Cin == c.C4 and c.stride == 1) for c in cases)
    for st in (1, 2):
        got[f"the projection block at stride {st}"] = any(c.proj and c.stride == st for c in cases)
    for Cg in S.GROUPED_CGS:
        got[f"Cg = {Cg}"] = any(c.Cm // c.groups == Cg for c in cases)
    for tw in (8, 16):
        got[f"the middle launch at TW = {tw}"] = any(m["tw"] == tw for m in mids)
    for kc in (16, 32, 64):
        got[f"the middle launch at KC = {kc}"] = any(m["kc"] == kc for m in mids)
    got["Cm = 64"] = any(c.Cm == 64 for c in cases)
    got["Cm % 128 != 0 and > 64"] = any(c.Cm % 128 and c.Cm > 64 for c in cases)
    got["C4 % 128 != 0"] = any(c.C4 % 128 for c in cases)
    got["Cin, Cm and C4 pairwise different"] = any(len({c.Cin, c.Cm, c.C4}) == 3 for c in cases)
    return got


def _fpn_corners(cases):
    """Every lateral form of forms_1x1.FORMS and every 3x3 form beside one, every channel count, the coarse map's last
    row and column read by one fine row / column alone, under each flag pair."""
    got = {f"Cin = {v}": any(c.Cin == v for c in cases) for v in S.FPN_CIN}
    got.update({f"Cf = {v}": any(c.Cf == v for c in cases) for v in S.FPN_CF})
    forced = [c.form.split("+") for c in cases if c.form]
    for lat in S.fpn_lateral_forms():
        got[f"lateral form {lat}"] = any(f[0] == lat for f in forced) or (lat == "auto" and any(not c.form for c in cases))
    for out in S.FPN_OUT_FORMS:
        got[f"3x3 form {out}"] = any(f[1] == out for f in forced) or (out == "auto" and any(not c.form for c in cases))
    got["an odd H and an odd W with a top"] = any(c.H % 2 and c.W % 2 and c.flags["top"] for c in cases)
    got["an even H or W with a top"] = any((c.H % 2 == 0 or c.W % 2 == 0) and c.flags["top"] for c in cases)
    for top in (False, True):
        for pad in (False, True):
            got[f"top={top} c_padded={pad}"] = any(c.flags["top"] == top and c.flags["c_padded"] == pad for c in cases)
    got["N = 1"] = any(c.N == 1 for c in cases)
    got["N = 6"] = any(c.N == 6 for c in cases)
    got["H or W above 32"] = any(max(c.H, c.W) > 32 for c in cases)
    drawn = [c for c in cases if c.shape not in S.FPN_AUTO]
    assert len(drawn) == len(cases) - len(S.FPN_AUTO)
    assert all(1 <= c.N <= 6 and 1 <= c.H <= 40 and 1 <= c.W <= 40 and S.macs(c) <= S.FPN_MACS for c in drawn)
    return got


def _corners(entry, cases, pkg, knobs):
    """{corner: reached} for the entry point's draws."""
    maps = [_map_hw(c) for c in cases]
    cin = [x for c in cases for x in _channels(c)[0]]
    cout = [x for c in cases for x in _channels(c)[1]]
    got = {
        "a map with H or W = 1": any(1 in out or 1 in inp for out, inp in maps),
        "an odd x odd map": any(out[0] % 2 and out[1] % 2 for out, _ in maps),
    }
    if entry not in ("basic_block", "conv3x3_grouped_bn_relu"):    # (their C is a multiple of 64 by contract)
        if cin:
            got["C % 64 != 0"] = any(x % 64 for x in cin)
    if cout:
        got["K % 128 != 0"] = any(x % 128 for x in cout)
    if entry == "conv3x3_bn_add_relu":
        got["K = 192"] = any(c.K == 192 for c in cases)
        got["C % 16 != 0"] = any(c.C % 16 for c in cases)
        got["a latency split S > 1"] = any(c.knobs and c.knobs.get("WINO_SMALL_SPLIT", 1) > 1 for c in cases)
        for ct in (1, 2, 4):
            got[f"latency block width ct = {ct}"] = any(c.knobs and c.knobs.get("WINO_SMALL_CT") == ct for c in cases)
    if entry == "basic_block":
        got["C = 192"] = any(c.C == 192 for c in cases)
    if entry == "stem":
        got["K > 128"] = any(c.K > 128 for c in cases)
    if entry == "avgpool_fc":
        got["classes % 64 != 0"] = any(c.classes % 64 for c in cases)
        got["classes % 64 == 0"] = any(c.classes % 64 == 0 for c in cases)
        got["C > 2048"] = any(c.C > 2048 for c in cases)
    if entry == "proj_block":
        got["stride 1"] = any(c.stride == 1 for c in cases)
        got["stride 2"] = any(c.stride == 2 for c in cases)
    if entry == "conv3x3_dilated_bn_relu":
        got.update(_dilated_corners(cases, pkg, knobs))
    if entry == "dilated_block":
        got.update(_block_corners(cases))
    if entry == "conv1x1_cat_bn":
        got.update(_cat_corners(cases, pkg, knobs))
    if entry == "aspp":
        got.update(_aspp_corners(cases))
    if entry == "resize_bilinear":
        got.update(_resize_corners(cases, pkg))
    if entry == "conv3x3_grouped_bn_relu":
        got.update(_grouped_corners(cases, pkg))
    if entry == "grouped_block":
        got.update(_grouped_block_corners(cases, pkg))
    if entry == "fpn_level":
        got.update(_fpn_corners(cases))
    if entry == "conv3x3_s2_proj":
        got["a stream-K range boundary inside the centre tap"] = any(
            c.knobs and _with_knobs(knobs, c, lambda: S.centre_tap_split(pkg, c)) for c in cases)
    for flag in FLAGS[entry]:
        got[f"{flag} on"] = any(c.flags.get(flag) for c in cases)
        got[f"{flag} off"] = any(not c.flags.get(flag) for c in cases)
    # every automatic form of every launch, as the plan query names it
    autos = [S.plan_form(pkg, c)["form"].split("/") for c in cases if c.knobs is None]
    for i, forms in enumerate(AUTO_FORMS[entry]):
        for f in sorted(forms):
            got[f"automatic form {f} (launch {i})"] = any(a[i] == f for a in autos)
    for f in sorted(FORCED_FORMS[entry]):
        got[f"forced form {f}"] = any(c.form == f for c in cases)
    return got


@pytest.mark.parametrize("entry", ENTRIES)
def test_draws_cover_the_corners(entry, pkg, knobs):
    got = _corners(entry, S.GENERATORS[entry](), pkg, knobs)
    missing = sorted(k for k, v in got.items() if not v)
    assert not missing, f"{entry}: the draws miss {missing}"


def _host_sweep(pkg, case, seed):
    """The tensors the GPU sweep draws for the case, on the host."""
    import torch
    return SC.Sweep(torch, "cpu", case, pkg, seed)


def test_aspp_pooled_branch_matters_in_every_case(pkg):
    """A dropped or misplaced per-image bias cannot pass the sweep: in every image of every drawn case the reference
    without the pooled branch is more than 100 x TIGHT (relative to max|full|) away from the full one."""
    for i, c in enumerate(S.GENERATORS["aspp"]()):
        P = SC.AsppProblem(_host_sweep(pkg, c, SC.SEEDS["aspp"] + i), c)
        full, without = P.reference(True), P.reference(False)
        share = [float(np.abs(full[n] - without[n]).max() / np.abs(full).max()) for n in range(c.N)]
        assert min(share) > 100 * TIGHT, f"{c.tag()}: pooled share per image {share}"
        assert (full > 0).mean() > 0.05 and (full == 0).any(), f"{c.tag()}: the final ReLU sees one side only"


def test_resize_label_rule_leaves_out_at_most_one_percent(pkg):
    """The gap rule of resize_cases.check_labels on the reference of every drawn case: the GPU sweep's label check
    covers at least 99 % of each case's pixels."""
    worst = 0.0
    for i, c in enumerate(S.GENERATORS["resize_bilinear"]()):
        src = SC.resize_src(_host_sweep(pkg, c, SC.SEEDS["resize_bilinear"] + i), c)
        want = RC.resize_reference(src.numpy(), c.Ho, c.Wo, c.C, c.flags["in_padded"])
        assert want.shape == (c.N, c.C, c.Ho, c.Wo) and np.isfinite(want).all(), c.tag()   # no NaN column or ring is read
        left = 1.0 - RC.decided(want, TIGHT * np.abs(want).max()).mean()
        worst = max(worst, left)
        assert left <= 0.01, f"{c.tag()}: the gap rule leaves out {left:.3%} of the pixels"
    print(f"resize sweep: the gap rule leaves out at most {worst:.4%} of a case's pixels")
