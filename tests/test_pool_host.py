"""Host-side checks of the three VGG entry points -- wino_conv3x3_bn_relu_pool_hw, wino_image_pack_hw,
wino_avgpool7_flatten_hw -- with no GPU: the symbols are exported and declared, and every argument, shape and overlap
rejection fires before any device query (the addresses are fake and never dereferenced; this machine has no device,
so a call that got past its checks would come back WINO_E_HIP, which no assertion here accepts)."""
import ctypes
import os

from conftest import ROOT

E_SHAPE, E_ARG = -2, -3
NEW = ["wino_conv3x3_bn_relu_pool_hw", "wino_image_pack_hw", "wino_avgpool7_flatten_hw"]
GIB = 1 << 30


def _p(addr):
    return ctypes.c_void_p(addr)


def test_new_symbols_exported_and_declared(pkg):
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "winograd_mi355x.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name + "(" in hdr, name
        assert name in pkg.ABI_SYMBOLS, name
        assert hdr.index(name) < hdr.index("#define WINO_ABI_VERSION"), name   # in the "Added since" list
    assert L.wino_abi_version() == 1
    for name in ("conv3x3_bn_relu_pool", "image_pack", "avgpool7_flatten", "VGG"):
        assert callable(getattr(pkg, name)), name


def _pool(L, inp, U, out, N=2, H=14, W=14, C=64, K=64, relu=1, bias=_p(64), scale=_p(128)):
    return L.wino_conv3x3_bn_relu_pool_hw(inp, U, bias, scale, out, N, H, W, C, K, relu, None)


def test_pooled_layer_rejections(pkg):
    L = pkg.lib()
    inp, U, out = _p(1 * GIB), _p(2 * GIB), _p(3 * GIB)
    args = [inp, U, _p(64), _p(128), out]
    for i in range(5):                      # NULL anywhere
        a = list(args)
        a[i] = None
        assert L.wino_conv3x3_bn_relu_pool_hw(*a, 2, 14, 14, 64, 64, 1, None) == E_ARG, i
    for i in (0, 1, 4):                     # 16-byte alignment of in, U, out
        a = list(args)
        a[i] = _p(a[i].value + 4)
        assert L.wino_conv3x3_bn_relu_pool_hw(*a, 2, 14, 14, 64, 64, 1, None) == E_ARG, i
    assert _pool(L, inp, U, out, K=96) == E_SHAPE
    assert _pool(L, inp, U, out, K=32) == E_SHAPE
    assert _pool(L, inp, U, out, C=60) == E_SHAPE
    assert _pool(L, inp, U, out, C=4) == E_SHAPE
    assert _pool(L, inp, U, out, H=1) == E_SHAPE          # no 2x2 window
    assert _pool(L, inp, U, out, W=1) == E_SHAPE
    assert _pool(L, inp, U, out, H=0) == E_SHAPE
    assert _pool(L, inp, U, out, W=4095) == E_SHAPE
    assert _pool(L, inp, U, out, N=0) == E_SHAPE
    # overlaps: in is 2 x 16 x 16 x 64 floats = 128 KiB, the pooled out 2 x 9 x 9 x 64 floats = 41472 bytes
    T_in, T_out = 2 * 16 * 16 * 64 * 4, 2 * 9 * 9 * 64 * 4
    assert _pool(L, inp, U, inp) == E_ARG                                # out IS in
    assert _pool(L, inp, U, _p(1 * GIB + T_in - 16)) == E_ARG            # out starts inside in
    assert _pool(L, inp, U, _p(1 * GIB - T_out + 16)) == E_ARG           # out ends inside in
    # (that tensors which merely touch pass is covered on a GPU: past the checks the entry point launches)


def _pack(L, x, out, N=2, Cin=3, H=32, W=32, Cpad=16):
    return L.wino_image_pack_hw(x, out, N, Cin, H, W, Cpad, None)


def test_image_pack_rejections(pkg):
    L = pkg.lib()
    x, out = _p(1 * GIB), _p(2 * GIB)
    assert _pack(L, None, out) == E_ARG
    assert _pack(L, x, None) == E_ARG
    assert _pack(L, _p(1 * GIB + 4), out) == E_ARG
    assert _pack(L, x, _p(2 * GIB + 8)) == E_ARG
    assert _pack(L, x, out, Cin=17) == E_SHAPE            # Cin > Cpad
    assert _pack(L, x, out, Cin=9, Cpad=8) == E_SHAPE
    assert _pack(L, x, out, Cin=0) == E_SHAPE
    assert _pack(L, x, out, Cpad=12) == E_SHAPE           # Cpad % 8
    assert _pack(L, x, out, Cpad=0) == E_SHAPE
    assert _pack(L, x, out, H=0) == E_SHAPE
    assert _pack(L, x, out, W=0) == E_SHAPE
    assert _pack(L, x, out, N=0) == E_SHAPE
    assert _pack(L, x, out, H=40000, W=40000) == E_SHAPE  # one image beyond 32-bit offsets
    T_x, T_out = 2 * 3 * 32 * 32 * 4, 2 * 34 * 34 * 16 * 4
    assert _pack(L, x, x) == E_ARG
    assert _pack(L, x, _p(1 * GIB + T_x - 16)) == E_ARG
    assert _pack(L, x, _p(1 * GIB - T_out + 16)) == E_ARG


def _flat(L, feat, out, N=2, H=7, W=7, C=64, padded=1):
    return L.wino_avgpool7_flatten_hw(feat, out, N, H, W, C, padded, None)


def test_avgpool7_flatten_rejections(pkg):
    L = pkg.lib()
    feat, out = _p(1 * GIB), _p(2 * GIB)
    assert _flat(L, None, out) == E_ARG
    assert _flat(L, feat, None) == E_ARG
    assert _flat(L, _p(1 * GIB + 4), out) == E_ARG
    assert _flat(L, feat, _p(2 * GIB + 4)) == E_ARG
    assert _flat(L, feat, out, C=6) == E_SHAPE            # C % 4
    assert _flat(L, feat, out, C=0) == E_SHAPE
    assert _flat(L, feat, out, H=0) == E_SHAPE
    assert _flat(L, feat, out, W=0) == E_SHAPE
    assert _flat(L, feat, out, N=0) == E_SHAPE
    assert _flat(L, feat, out, padded=2) == E_SHAPE
    T_feat, T_out = 2 * 9 * 9 * 64 * 4, 2 * 49 * 64 * 4
    assert _flat(L, feat, feat) == E_ARG
    assert _flat(L, feat, _p(1 * GIB + T_feat - 16)) == E_ARG
    assert _flat(L, feat, _p(1 * GIB - T_out + 16)) == E_ARG
    # unpadded: the input is 2 x 7 x 7 x 64 floats; an out that starts 16 bytes before its end overlaps its last unit
    assert _flat(L, feat, _p(1 * GIB + 2 * 7 * 7 * 64 * 4 - 16), padded=0) == E_ARG
