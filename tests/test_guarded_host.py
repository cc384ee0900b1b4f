"""The guarded arena of tests/guarded.py on CPU tensors: a clean round trip passes, a planted write at either end of
either guard or into an input is reported with its tensor, side and offset, the placements are what `align` says, and
the guard sizes obey the rule stated in the module."""
import pytest
import torch

import guarded as G


def _arena(align=256):
    return G.Arena(torch, "cpu", align=align)


def _slot(arena, t):
    return next(s for s in arena.slots if s.tensor.data_ptr() == t.data_ptr())


def test_clean_round_trip_passes():
    for align in G.ALIGNS:
        a = _arena(align)
        x = a.input(torch.rand(2, 5, 7, 16))
        nanring = torch.rand(3, 4, 4, 8)
        nanring[:, 0] = float("nan")                       # NaN inside a master compares bit for bit
        r = a.input(nanring)
        out, ws = a.output(2, 5, 7, 16), a.workspace(1001)
        assert ws.numel() == 251 and bool(torch.isnan(out).all()) and bool(torch.isnan(ws).all())
        out.copy_(x * 2)
        ws.fill_(3.0)
        a.check("clean")
        assert torch.equal(out, x * 2) and torch.equal(r[:, 1:], nanring[:, 1:])


def test_views_are_contiguous_placed_and_shaped():
    for align, rem in ((256, 0), (16, 16)):
        a = _arena(align)
        ts = [a.input(torch.rand(3, 9, 11, 40)), a.output(3, 9, 11, 40), a.output(7), a.input(torch.rand(64)),
              a.workspace(4096, align=align)]
        for t, shape in zip(ts, [(3, 9, 11, 40), (3, 9, 11, 40), (7,), (64,), (1024,)]):
            assert t.is_contiguous() and tuple(t.shape) == shape and t.dtype == torch.float32
            assert t.data_ptr() % 256 == rem, (align, t.data_ptr() % 256)
    a = _arena(16)
    assert a.workspace(4096).data_ptr() % 256 == 0, "workspaces stay at 256 unless a test asks otherwise"
    with pytest.raises(ValueError):
        a.output(4, align=6)


def test_guards_are_filled_as_stated():
    a = _arena()
    x, out = a.input(torch.rand(2, 64)), a.output(2, 64)
    sx, so = _slot(a, x), _slot(a, out)
    for g in (sx.front(), sx.back()):
        assert bool(torch.isnan(g).all()) and bool((g.view(torch.int32) == G.NAN_BITS).all())
    for g in (so.front(), so.back()):
        assert bool(torch.isnan(g).all()), "the sentinel is a NaN: a guard that leaks into arithmetic shows"
        assert bool((g.view(torch.int32) == G.SENTINEL).all())
    assert (G.SENTINEL >> 22) == 0x1FF and G.SENTINEL != G.NAN_BITS     # quiet NaN with a payload


@pytest.mark.parametrize("kind", ["input", "output", "workspace"])
@pytest.mark.parametrize("align", G.ALIGNS)
def test_planted_writes_are_reported_with_side_and_offset(kind, align):
    def fresh():
        a = _arena(align)
        other = a.output(3, 8)                              # a bystander that must not be named
        t = {"input": lambda: a.input(torch.rand(2, 6, 6, 8), name="victim"),
             "output": lambda: a.output(2, 6, 6, 8, name="victim"),
             "workspace": lambda: a.workspace(2 * 6 * 6 * 8 * 4, align=align, name="victim")}[kind]()
        return a, t, _slot(a, t)

    for side, at_far_end in (("back", False), ("back", True), ("front", False), ("front", True)):
        a, t, s = fresh()
        g = s.back() if side == "back" else s.front()
        glen = g.numel() * 4
        assert glen >= G.GUARD_MIN
        if side == "back":
            idx, off, unit = (g.numel() - 1, glen - 4, "past the end") if at_far_end else (0, 0, "past the end")
        else:
            idx, off, unit = (0, glen, "before the start") if at_far_end else (g.numel() - 1, 4, "before the start")
        g[idx] = 1.0
        with pytest.raises(G.GuardError) as e:
            a.check("case-7")
        msg = str(e.value)
        text = f"4 bytes written starting {off} bytes {unit}"
        assert msg.startswith("case-7: victim") and f"{side} guard" in msg and text in msg, msg
        assert "output0" not in msg, msg
    # the same through raw addresses: one float right behind and right before the tensor
    a, t, s = fresh()
    flat = s.buf
    flat[s.start + s.numel] = 0.0
    flat[s.start - 1] = 0.0
    with pytest.raises(G.GuardError) as e:
        a.check("raw")
    assert "0 bytes past the end" in str(e.value) and "4 bytes before the start" in str(e.value)
    # a write that restores the very bit pattern is no write; any other NaN is one
    a, t, s = fresh()
    s.back().view(torch.int32)[5] = s.fill
    a.check("same bits")
    s.back().view(torch.int32)[5] = s.fill ^ 1
    with pytest.raises(G.GuardError, match="starting 20 bytes past the end"):
        a.check("other nan")


def test_a_span_is_reported_from_first_to_last_dirty_byte():
    a = _arena()
    out = a.output(4, 64, name="out")
    _slot(a, out).back()[:64] = 0.0
    with pytest.raises(G.GuardError, match=r"out \(output, \(4, 64\)\): back guard: 256 bytes written starting 0 bytes "
                                           r"past the end \(last dirty byte 255 past the end\); 64 dirty words"):
        a.check("span")


def test_a_written_input_is_reported_unless_in_place():
    a = _arena()
    m = torch.rand(2, 3, 3, 8)
    x = a.input(m, name="weights")
    x.view(-1)[10] += 1.0
    with pytest.raises(G.GuardError) as e:
        a.check("ro")
    assert "weights" in str(e.value) and "read-only operand written" in str(e.value)
    assert "first at byte 40" in str(e.value) and "last at byte 43" in str(e.value)
    a = _arena()
    x = a.input(m, name="buf", in_place=True)
    x.mul_(2.0)
    a.check("in place")
    _slot(a, x).back()[0] = 0.0                              # its guards are still watched
    with pytest.raises(G.GuardError, match="buf"):
        a.check("in place")
    assert torch.equal(m, _slot(a, x).master), "the master is a copy of what the caller gave"


def test_guard_sizes_obey_the_rule():
    KiB, MiB, GiB = 1 << 10, 1 << 20, 1 << 30
    assert (G.GUARD_MIN, G.GUARD_MAX) == (64 * KiB, 64 * MiB)
    assert G.guard_bytes(64 * 4, 1) == 64 * KiB                       # a tiny tensor: the floor
    assert G.guard_bytes(1 * GiB, 1) == 64 * MiB                      # one 1 GiB image: the cap
    assert G.guard_bytes(1 * GiB, 64) == 16 * MiB                     # one image of 64
    assert G.guard_bytes(1 * GiB, 1 << 20) == 64 * KiB                # small images: the floor again
    img = 58 * 58 * 256 * 4
    g = G.guard_bytes(7 * img, 7)
    assert img <= g < img + 256 and g % 256 == 0                      # at least one image, whole 256-byte units
    assert G.guard_bytes(0, 0) == 64 * KiB
    # and the arena applies it: both guards of a carved tensor are at least that long
    a = _arena(16)
    t = a.output(3, 40, 40, 64)
    s = _slot(a, t)
    need = G.guard_bytes(t.numel() * 4, 3)
    assert need >= 40 * 40 * 64 * 4 > G.GUARD_MIN
    assert s.back().numel() * 4 == need and need <= s.front().numel() * 4 < need + 256


def test_workspace_runs_are_counted_once_and_only_when_clean():
    before = G.WORKSPACE_RUNS.copy()
    a = _arena()
    ws = a.workspace(512, query=("query_a", "query_b"))
    a.workspace(512)
    _slot(a, ws).back()[3] = 0.0
    with pytest.raises(G.GuardError):
        a.check("dirty")
    assert G.WORKSPACE_RUNS == before, "a failed check counts nothing"
    _slot(a, ws).back().view(torch.int32)[3] = G.SENTINEL
    a.check("clean")
    a.check("again")
    assert G.WORKSPACE_RUNS["query_a"] - before["query_a"] == 1 and G.WORKSPACE_RUNS["query_b"] - before["query_b"] == 1
    assert set(G.WORKSPACE_RUNS) - set(before) <= {"query_a", "query_b"}
