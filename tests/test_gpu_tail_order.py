"""The order of a range in the fused 3x3 kernel and the finish from registers ("Hand-off").

A workgroup whose tail range lies inside one item runs its whole-item rounds first and its tail segment last; a partial
segment that would draw its ticket at once peeks at the item's counter first and, when every other segment has already
drawn, finishes the item from its registers instead of publishing its slab.  The shapes below are the smallest that hold
every case; the comment on each says which.  tests/test_tail_order_host.py checks the cut itself without a GPU.

Every launch writes into a NaN-filled output.  The result is compared with the shared fp64 reference of layer_refs at the
suite's TIGHT and with the automatic grid's result at 2e-6 x max|ref| (the bound the existing stream-K tests hold the
decompositions to); its ring is zero; no ticket counter is left set; wino_stream_check is clean; a second, identical
launch agrees bit for bit."""
import ctypes

import numpy as np
import pytest

import layer_refs as LR
from cases import TIGHT
from gpu_support import torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu

# (kind, (N, H, W, C, K), forced grid, the cut the planner makes of it: (whole-item rounds, k-groups, sk_q, sk_rem))
# The cut is asserted from the plan queries in every case, so the comments cannot drift from the launches.
CASES = [
    # 14 items, kp = 2: one whole round and a tail of 6; ranges of 12 over items of 16: ranges 0 and 3 of each k-group
    # lie inside one item (whole-first, they finish from registers), 1 and 2 straddle, and the middle item lies between
    # the two straddlers (nseg = 2: the later of them finishes it after a peek)
    ("plain", (8, 14, 14, 128, 128), 8, (1, 2, 12, 0)),
    # kp = 1 with unequal ranges (8 or 9 iterations) behind one whole round: 5 whole-first ranges, 4 straddlers
    ("plain", (8, 14, 14, 128, 128), 9, (1, 1, 8, 8)),
    # TWO whole rounds in front of the tail segment, unequal ranges (5 or 6), kp = 2: every range is whole-first
    ("plain", (8, 14, 14, 128, 128), 6, (2, 2, 5, 1)),
    # no tail, kp = 1 (the grid divides the items: two whole rounds) and kp = 2 (one whole item each)
    ("plain", (8, 14, 14, 128, 128), 7, (2, 1, 0, 0)),
    ("plain", (8, 14, 14, 128, 128), 14, (1, 2, 0, 0)),
    # ranges of 2 or 3 over one 16-iteration tail item per k-group: six one-segment ranges inside ONE item, all
    # whole-first, all of them peek, the counter lets one through
    ("plain", (8, 14, 14, 128, 128), 12, (1, 2, 2, 4)),
    # the same with ranges of 6 or 7: four whole-first ranges and a straddler per k-group
    ("plain", (8, 14, 14, 128, 128), 10, (1, 2, 6, 2)),
    # ALL TAIL (no whole round: nothing to run first, whole-first is off, every range's last segment peeks and several
    # peekers share an item): equal ranges of 14 over items of 16, kp = 2: six straddlers per k-group ...
    ("plain", (8, 14, 14, 128, 128), 16, (0, 2, 14, 0)),
    # ... unequal ranges (11 or 12), kp = 2 ...
    ("plain", (8, 14, 14, 128, 128), 20, (0, 2, 11, 2)),
    # ... and one item-major list (kp = 1), unequal ranges (14 or 15)
    ("plain", (8, 14, 14, 128, 128), 15, (0, 1, 14, 14)),
    # items of 8 chunks, 15 items on 8 workgroups, kp = 1: ranges of 7 leave segments of one iteration, and ranges 0 and
    # 7 are whole-first with their segment at the start / at the end of its item
    ("plain", (19, 14, 14, 64, 64), 8, (1, 1, 7, 0)),
    # ... and kp = 1 with unequal ranges (5 or 6) on that shape: 6 whole-first ranges, 3 straddlers
    ("plain", (19, 14, 14, 64, 64), 9, (1, 1, 5, 3)),
    # the any-feature-map build: 28 x 28, 14 items again
    ("plain", (2, 28, 28, 128, 128), 8, (1, 2, 12, 0)),
    # the residual and the pooled entry points
    ("res", (8, 14, 14, 128, 128), 8, (1, 2, 12, 0)),
    ("pool", (8, 14, 14, 128, 128), 8, (1, 2, 12, 0)),
    # a grid beyond the CU count, whole round + tail with unequal ranges (392 items on 300 workgroups, kp = 2, ranges of
    # 2 or 3): the workgroups past the first wave of residents start late, so peeks fail and succeed in an order of
    # their own
    ("plain", (256, 14, 14, 64, 128), 300, (1, 2, 2, 68)),
]
# the images the fp64 reference is computed for (all of them where the batch is small)
REF_IMAGES = {256: [0, 197, 230, 255]}

_layers = {}


def _interior(t):
    return t[:, 1:-1, 1:-1, :]


def _ring_is_zero(torch, t):
    inner = torch.zeros_like(t, dtype=torch.bool)
    _interior(inner)[...] = True
    return bool((t[~inner] == 0).all())


def _cut(pkg, shape):
    """(whole-item rounds, k-groups, sk_q, sk_rem) of the launch the planner makes of `shape` under the knobs in force,
    and its grid: from wino_conv3x3_plan and wino_conv3x3_plan_groups."""
    N, H, W, C, K = shape
    i = [ctypes.c_int() for _ in range(7)]
    tail = ctypes.c_long()
    L = pkg.lib()
    assert L.wino_conv3x3_plan(N, H, W, C, K, 256, ctypes.byref(i[0]), ctypes.byref(i[1]), ctypes.byref(tail), ctypes.byref(i[2])) == 0
    assert L.wino_conv3x3_plan_groups(N, H, W, C, K, 256, *(ctypes.byref(v) for v in i[3:7])) == 0
    grid, rounds, kp = i[0].value, i[1].value, i[3].value
    Tg, Gp = tail.value // kp, grid // kp
    return grid, (rounds, kp, Tg // Gp, Tg % Gp)


def _layer(kind, shape, pkg, torch_dev, knobs):
    """Operands, launcher, the fp64 reference and the automatic grid's result, computed once per layer."""
    key = (kind, shape)
    if key in _layers:
        return _layers[key]
    torch, dev = torch_dev
    N, H, W, C, K = shape
    g = torch.Generator(device="cpu").manual_seed(sum(shape) + len(kind))
    x = LR.ring(torch.rand(N, H, W, C, generator=g) - 0.5)
    w = (torch.rand(K, C, 3, 3, generator=g) - 0.5) / np.sqrt(9 * C) * 4
    b, s = torch.rand(K, generator=g) - 0.5, torch.rand(K, generator=g) + 0.5
    res = LR.ring(torch.rand(N, H, W, K, generator=g) - 0.5, float("nan"))   # the residual's ring is never read
    idx = REF_IMAGES.get(N, list(range(N)))
    xt, bt, st, rt = (a.contiguous().to(dev) for a in (x, b, s, res))
    U = pkg.filter_transform_f2(w.to(dev))
    if kind == "plain":
        out_shape = (N, H + 2, W + 2, K)
        run = lambda out: pkg.conv3x3_bn_relu(xt, U, bt, st, out=out)   # noqa: E731
        want = LR.conv3x3(LR.interior(x[idx]), w, (b, s), True)
    elif kind == "res":
        out_shape = (N, H + 2, W + 2, K)
        run = lambda out: pkg.conv3x3_bn_add_relu(xt, U, bt, st, rt, out=out)   # noqa: E731
        want = LR.conv3x3(LR.interior(x[idx]), w, (b, s), True, residual=LR.interior(res[idx]))
    else:
        out_shape = (N, H // 2 + 2, W // 2 + 2, K)
        run = lambda out: pkg.conv3x3_bn_relu_pool(xt, U, bt, st, out=out)   # noqa: E731
        want = LR.conv3x3(LR.interior(x[idx]), w, (b, s), True, pool=True)
    knobs.unset("WINO_SK_GRID")
    auto = torch.full(out_shape, float("nan"), device=dev)
    run(auto)
    assert pkg.tickets_in_use() == 0
    _layers[key] = (run, out_shape, idx, want, auto)
    return _layers[key]


def _checked_launches(pkg, torch_dev, run, out_shape, idx, want, auto, tag):
    torch, dev = torch_dev
    outs = []
    for rep in range(2):
        out = torch.full(out_shape, float("nan"), device=dev)
        run(out)
        assert pkg.tickets_in_use() == 0, f"{tag}, launch {rep}: an item was left unfinished"
        pkg.stream_check()
        assert _ring_is_zero(torch, out), f"{tag}, launch {rep}: the ring is not zero"
        outs.append(out)
    a = outs[0]
    assert not bool(torch.isnan(a).any()), f"{tag}: outputs never written"
    assert torch.equal(a, outs[1]), f"{tag}: not reproducible"
    err_ref = LR.rel(_interior(a[idx]), want)
    err_auto = float((a - auto).abs().max()) / float(auto.abs().max())
    print(f"{tag}: vs fp64 reference {err_ref:.2e}, vs automatic grid {err_auto:.2e}")
    assert err_ref < TIGHT
    assert err_auto < 2e-6
    return a


@pytest.mark.parametrize("kind,shape,grid,cut", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_whole_first_ranges_and_the_finish_from_registers(kind, shape, grid, cut, pkg, torch_dev, knobs):
    knobs.set("WINO_3X3_ALGO", "big")
    run, out_shape, idx, want, auto = _layer(kind, shape, pkg, torch_dev, knobs)
    knobs.set("WINO_SK_GRID", str(grid))
    assert _cut(pkg, shape) == (grid, cut)
    _checked_launches(pkg, torch_dev, run, out_shape, idx, want, auto, f"{kind} {shape} grid {grid}")


def test_with_a_competing_stream(pkg, torch_dev, knobs):
    """A second stream's launches hold CUs, so part of the workgroups start late: peeks that usually succeed fail, the
    ticket path finishes those items, and nothing may show -- results bitwise those of the undisturbed launch, counters
    back at zero.  The headline shape (256 channels, N = 128, the automatic grid of 256: 128 whole-first workgroups) and
    the small case with both kinds of range."""
    torch, dev = torch_dev
    knobs.set("WINO_3X3_ALGO", "big")
    g = torch.Generator(device="cpu").manual_seed(23)
    mk = lambda *s: (torch.rand(*s, generator=g) - 0.5).to(dev)   # noqa: E731
    xs, ws, vs = mk(64, 16, 16, 128), mk(128, 128, 3, 3), mk(128)
    Us = pkg.filter_transform_f2(ws)
    side = torch.cuda.Stream()
    for shape, grid, reps in (((128, 14, 14, 256, 256), None, 12), ((8, 14, 14, 128, 128), 8, 12),
                              ((8, 14, 14, 128, 128), 16, 12)):   # (the last: all tail, every last segment peeks)
        N, H, W, C, K = shape
        knobs.unset("WINO_SK_GRID")
        x, w, s, b = mk(N, H + 2, W + 2, C), mk(K, C, 3, 3), mk(K), mk(K)
        U = pkg.filter_transform_f2(w)
        if grid:
            knobs.set("WINO_SK_GRID", str(grid))
        ref = pkg.conv3x3_bn_relu(x, U, b, s).clone()
        want = LR.conv3x3(x[:2].cpu(), w.cpu(), (b.cpu(), s.cpu()), True, padding=0)   # (x brings its ring along)
        assert LR.rel(_interior(ref[:2]), want) < TIGHT
        torch.cuda.synchronize()
        for rep in range(reps):
            with torch.cuda.stream(side):
                for _ in range(3):
                    pkg.conv3x3_bn_relu(xs, Us, vs, vs)
            outs = [pkg.conv3x3_bn_relu(x, U, b, s, out=torch.full_like(ref, float("nan"))) for _ in range(4)]
            for o in outs:
                assert torch.equal(o, ref), (shape, rep)
        torch.cuda.synchronize()
        assert pkg.tickets_in_use() == 0
        pkg.stream_check()
        with torch.cuda.stream(side):
            assert pkg.tickets_in_use() == 0


@pytest.mark.parametrize("value", [2, 9])
def test_a_preset_counter_is_reported_by_the_error_word(value, pkg, torch_dev, knobs):
    """The fail-fast contract where segments peek.  Grid 8 of the 14-item shape: items 8 .. 13 are the tail, two segments
    each (nseg = 2).  ONLY their counters are preset, to nseg or more: a peeking wave finds its counter out of range at
    first sight, and so does every ticket drawn on it.  The kernel says so on the host-visible error word, which is all
    the next launch looks at: it is refused (WINO_E_STATE) before anything has called wino_stream_check.
    wino_stream_reset_scratch() then recovers bitwise results.  (A peek that fails is always followed by a drawn
    ticket, which reports the same counter on the same word: the two stores cannot be told apart from outside.)"""
    torch, dev = torch_dev
    knobs.set("WINO_3X3_ALGO", "big")
    shape = (8, 14, 14, 128, 128)
    run, out_shape, idx, want, auto = _layer("plain", shape, pkg, torch_dev, knobs)
    knobs.set("WINO_SK_GRID", "8")
    assert _cut(pkg, shape) == (8, (1, 2, 12, 0))
    with torch.cuda.stream(torch.cuda.Stream()):
        ref = _checked_launches(pkg, torch_dev, run, out_shape, idx, want, auto, f"clean, before {value}").clone()
        for i in range(8 * 8, 14 * 8):   # a counter per (tail item, wave)
            pkg.poison_ticket(i, value)
        run(torch.full(out_shape, float("nan"), device=dev))   # its result is not to be trusted, and it must say so
        torch.cuda.current_stream().synchronize()
        with pytest.raises(pkg.WinoError, match="rc=-4"):
            run(torch.full(out_shape, float("nan"), device=dev))
        with pytest.raises(pkg.WinoError, match="rc=-4"):
            pkg.stream_check()
        pkg.stream_reset_scratch()
        pkg.stream_check()
        assert pkg.tickets_in_use() == 0
        for _ in range(2):
            out = torch.full(out_shape, float("nan"), device=dev)
            run(out)
            assert torch.equal(out, ref)
            assert pkg.tickets_in_use() == 0
    torch.cuda.synchronize()
