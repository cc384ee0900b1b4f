"""Host-side checks (no GPU) of the seeded shape sweeps in tests/shape_sweeps.py that tests/test_gpu_shape_sweeps.py
runs: every drawn case is one the library accepts, in the form it was drawn for (so a GPU sweep never skips a shape or
turns it into a WinoError), and the draws of each entry point reach the corners they exist for.  A generator edit that
loses a corner fails here and names it."""
import pytest

import shape_sweeps as S

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


def _map_hw(c):
    """The (output) map the case's kernel walks, and the input map."""
    s = c.shape
    if c.entry in ("conv3x3_s2_bn_relu", "conv3x3_s2_proj", "basic_block_s2", "proj_block_v15"):
        return (S._s2(s["Hin"]), S._s2(s["Win"])), (s["Hin"], s["Win"])
    if c.entry == "proj_block":
        st = s["stride"]
        return ((s["Hin"] - 1) // st + 1, (s["Win"] - 1) // st + 1), (s["Hin"], s["Win"])
    if c.entry == "stem":
        return S.stem_out(s["H"], s["W"]), (s["H"], s["W"])
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
}


def _corners(entry, cases, pkg, knobs):
    """{corner: reached} for the entry point's draws."""
    maps = [_map_hw(c) for c in cases]
    cin = [x for c in cases for x in _channels(c)[0]]
    cout = [x for c in cases for x in _channels(c)[1]]
    got = {
        "a map with H or W = 1": any(1 in out or 1 in inp for out, inp in maps),
        "an odd x odd map": any(out[0] % 2 and out[1] % 2 for out, _ in maps),
    }
    if entry != "basic_block":    # (its C is a multiple of 64 by contract)
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
