"""Host-side checks of the size limits that decide whether a shape reaches the kernels -- no GPU needed.

The Winograd 3x3's filter matrix U [16][C][K] is read through one buffer descriptor (a 32-bit size and 32-bit byte
offsets), so every entry point that takes that layer refuses C * K >= 2^26 (16 C K floats >= 4 GiB) with WINO_E_SHAPE,
before any device call: the fake, aligned, non-overlapping addresses below are never dereferenced.  The shapes that
tests/test_gpu_large_tensors.py runs (tensors past 2 and 4 GiB, the largest accepted filter) must still plan."""
import ctypes

import pytest

E_SHAPE = -2
GIB = 1 << 30
CUS = 256

# the first refused shape (U exactly 4 GiB: every read out of range), two that wrap the descriptor's size, and the
# largest accepted one (C * K = 66 584 576 < 2^26)
REFUSED = [(8192, 8192), (4104, 16384), (8192, 8256)]
LAST_ACCEPTED = (8192, 8128)


def _p(k):
    return ctypes.c_void_p(k * GIB)


def _ints(n, ctype=ctypes.c_int):
    return [ctype(0) for _ in range(n)]


def _plan(L, N, H, W, C, K):
    grid, rounds, ipi = _ints(3)
    tail = ctypes.c_long(0)
    return L.wino_conv3x3_plan(N, H, W, C, K, CUS, ctypes.byref(grid), ctypes.byref(rounds), ctypes.byref(tail),
                               ctypes.byref(ipi))


def _small_plan2(L, N, H, W, C, K):
    v = _ints(5)
    return L.wino_conv3x3_small_plan2(N, H, W, C, K, CUS, *[ctypes.byref(x) for x in v]), v


def _entry_points(L, C, K):
    """(name, call) for every entry point of the Winograd 3x3 layer itself, C -> K at N = 1, 14 x 14."""
    N, H = 1, 14
    v4 = _ints(4)
    return [
        ("wino_conv3x3_plan", lambda: _plan(L, N, H, H, C, K)),
        ("wino_conv3x3_small_plan2", lambda: _small_plan2(L, N, H, H, C, K)[0]),
        ("wino_conv3x3_small_plan",
         lambda: L.wino_conv3x3_small_plan(N, H, H, C, K, CUS, *[ctypes.byref(x) for x in v4])),
        ("wino_conv3x3_plan_groups",
         lambda: L.wino_conv3x3_plan_groups(N, H, H, C, K, CUS, *[ctypes.byref(x) for x in v4])),
        ("wino_conv3x3_prepare_hw", lambda: L.wino_conv3x3_prepare_hw(N, H, H, C, K, None)),
        ("wino_conv3x3_prepare", lambda: L.wino_conv3x3_prepare(N, C, K, None)),
        ("wino_conv3x3_bn_relu_hw",
         lambda: L.wino_conv3x3_bn_relu_hw(_p(1), _p(2), _p(3), _p(4), _p(8), N, H, H, C, K, 1, None)),
        ("wino_conv3x3_bn_relu", lambda: L.wino_conv3x3_bn_relu(_p(1), _p(2), _p(3), _p(4), _p(8), N, C, K, 1, None)),
        ("wino_conv3x3_bn_add_relu_hw",
         lambda: L.wino_conv3x3_bn_add_relu_hw(_p(1), _p(2), _p(3), _p(4), _p(12), _p(8), N, H, H, C, K, 1, None)),
    ]


def _square_entry_points(L, C):
    """Entry points whose 3x3 is C -> C: the basic block, the bottleneck blocks' middle layer, the downsampling
    block's second conv (K = C there)."""
    N, H = 1, 14
    ws = 64 * GIB   # more than any workspace at N = 1
    return [
        ("wino_basic_block_hw",
         lambda: L.wino_basic_block_hw(_p(1), _p(2), _p(3), _p(4), _p(5), _p(6), _p(7), _p(8), N, H, H, C, _p(16), ws,
                                       None)),
        ("wino_basic_block_prepare_hw", lambda: L.wino_basic_block_prepare_hw(N, H, H, C, None)),
        ("wino_basic_block_s2_prepare_hw", lambda: L.wino_basic_block_s2_prepare_hw(N, 2 * H, 2 * H, 64, C, None)),
        ("wino_basic_block_s2_hw",
         lambda: L.wino_basic_block_s2_hw(_p(1), _p(2), _p(3), _p(4), _p(5), _p(8), N, 2 * H, 2 * H, 64, C, _p(16), ws,
                                          None)),
        ("wino_residual_block_prepare_hw", lambda: L.wino_residual_block_prepare_hw(N, H, H, 64, C, None)),
        ("wino_residual_block_prepare", lambda: L.wino_residual_block_prepare(N, 64, C, None)),
        ("wino_residual_block_hw",
         lambda: L.wino_residual_block_hw(_p(1), _p(2), _p(3), _p(4), _p(5), _p(6), _p(7), _p(9), _p(10), _p(11),
                                          _p(12), N, H, H, 64, C, _p(16), ws, None)),
        ("wino_proj_block_prepare_hw", lambda: L.wino_proj_block_prepare_hw(N, H, H, 64, C, 64, 1, None)),
        ("wino_proj_block_hw",
         lambda: L.wino_proj_block_hw(_p(1), _p(2), _p(3), _p(4), _p(5), _p(6), _p(7), _p(9), _p(12), N, H, H, 64, C, 64,
                                      1, _p(16), ws, None)),
    ]


@pytest.mark.parametrize("C,K", REFUSED)
def test_every_3x3_entry_point_refuses_a_4gib_filter(C, K, pkg):
    L = pkg.lib()
    for name, call in _entry_points(L, C, K):
        assert call() == E_SHAPE, name
        assert b"filter matrix" in L.wino_last_error_string(), name


def test_square_entry_points_refuse_a_4gib_filter(pkg):
    """C = K = 8192 through every block: each refuses before its first launch (the 1x1 layers around the 3x3
    would take these shapes)."""
    L = pkg.lib()
    for name, call in _square_entry_points(L, 8192):
        assert call() == E_SHAPE, name
        assert b"filter matrix" in L.wino_last_error_string(), name


def test_the_last_accepted_filter_still_plans(pkg):
    """C = 8192, K = 8128: U is 3.97 GiB, the largest the descriptor spans; both kernels' plans are returned."""
    L = pkg.lib()
    C, K = LAST_ACCEPTED
    assert 16 * C * K * 4 < (1 << 32) <= 16 * C * (K + 64) * 4
    assert _plan(L, 1, 4, 4, C, K) == 0
    assert _plan(L, 1, 14, 14, C, K) == 0
    assert _small_plan2(L, 1, 4, 4, C, K)[0] == 0


def test_filter_transform_is_not_bounded(pkg):
    """U itself is built with 64-bit indices: its size query and index map take the refused shapes."""
    L = pkg.lib()
    for C, K in REFUSED:
        assert L.wino_filter_f2_elems(C, K) == 16 * C * K
        # the last 8-channel x 64-out-channel chunk holds the last 8192 floats
        assert 16 * C * K - 8192 <= L.wino_filter_f2_index(C, K, 15, C - 1, K - 1) < 16 * C * K


# ------------------------------------------------------------------ the shapes of tests/test_gpu_large_tensors.py
def _limit(H, W, C, K):
    return ((1 << 32) - 1) // ((H + 2) * (W + 2) * max(C, K) * 4)


def test_large_3x3_batches_plan_per_launch(pkg):
    """56x56x64 at N = 5100 goes out as 4928 + 172 images; each launch plans, and the whole batch is refused by the
    one-launch query (the launcher splits it)."""
    L = pkg.lib()
    N, H, C = 5100, 56, 64
    step = _limit(H, H, C, C)
    step -= step % 64
    assert step == 4928
    assert _plan(L, step, H, H, C, C) == 0
    assert _plan(L, N - step, H, H, C, C) == 0
    assert _plan(L, N, H, H, C, C) == E_SHAPE
    # the residual block's middle layer (N = 1400, 56x56, Cm = 64) and the v1 projection block's at both strides
    assert _plan(L, 1400, 56, 56, 64, 64) == 0
    assert _plan(L, 1400, 28, 28, 128, 128) == 0
    assert _plan(L, 1400, 56, 56, 128, 128) == 0
    # the downsampling block's second conv (5100 images of 28x28x128: one launch)
    assert _plan(L, 5100, 28, 28, 128, 128) == 0


def test_large_1x1_and_stride2_shapes_plan(pkg):
    L = pkg.lib()
    v5 = _ints(5)
    # chained 1x1 at 56x56, 256 -> 256, 1400 images (4.5 GB in, 4.8 GB padded)
    assert L.wino_conv1x1_plan(1400 * 56 * 56, 256, 256, CUS, *[ctypes.byref(x) for x in v5]) == 0
    # the residual block's two 1x1 layers
    assert L.wino_conv1x1_plan(1400 * 56 * 56, 256, 64, CUS, *[ctypes.byref(x) for x in v5]) == 0
    assert L.wino_conv1x1_plan(1400 * 56 * 56, 64, 256, CUS, *[ctypes.byref(x) for x in v5]) == 0
    form = ctypes.c_int(-1)
    # the stride-2 3x3 at conv3, 128 -> 128, 5200 images (8.9 GB in); the fused downsampling layer 64 -> 128
    assert L.wino_conv3x3_s2_plan(5200, 56, 56, 128, 128, CUS, ctypes.byref(form)) == 0
    assert L.wino_conv3x3_s2_plan(5100, 56, 56, 64, 128, CUS, ctypes.byref(form)) == 0
    first, tail = ctypes.c_int(-1), ctypes.c_int(-1)
    for stride in (1, 2):
        assert L.wino_proj_tail_plan(1400, 56, 56, 256, 128, 512, stride, CUS, ctypes.byref(first),
                                     ctypes.byref(tail)) == 0, stride
    # the v1.5 block's stride-2 3x3 (128 -> 128 from the 56x56 map)
    assert L.wino_conv3x3_s2_plan(1400, 56, 56, 128, 128, CUS, ctypes.byref(form)) == 0
