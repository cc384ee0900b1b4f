"""The depthwise 3x3 layer's plan query (wino_dwconv3x3_plan), no GPU needed: the tiles cover the output, the channel
block falls to 16 exactly when the 64-channel grid is below the device's CU count, and illegal shapes get the layer's
error codes."""
import pytest

CUS = 256


def _grid(pkg, knobs, N, Hin, Win, C, stride, cb):
    knobs.set("WINO_DW_CB", cb)
    got, th, tw, ty, tx = pkg.dwconv3x3_plan(N, Hin, Win, C, stride, CUS)
    knobs.unset("WINO_DW_CB")
    assert got == cb
    return N * ty * tx * -(-C // cb)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("N,Hin,Win,C", [(1, 7, 7, 960), (1, 14, 14, 576), (32, 7, 7, 960), (1, 112, 112, 32), (1, 1, 1, 4),
                                         (3, 9, 17, 132), (1, 33, 8, 64), (2, 28, 28, 192), (1, 56, 57, 20)])
def test_plan_geometry(N, Hin, Win, C, stride, pkg, knobs):
    cb, th, tw, ty, tx = pkg.dwconv3x3_plan(N, Hin, Win, C, stride, CUS)
    H, W = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    assert (ty - 1) * th < H <= ty * th and (tx - 1) * tw < W <= tx * tw
    grid64 = _grid(pkg, knobs, N, Hin, Win, C, stride, 64)
    assert cb == (16 if grid64 < CUS else 64), (cb, grid64)
    assert _grid(pkg, knobs, N, Hin, Win, C, stride, 16) >= grid64


@pytest.mark.parametrize("dims,rc", [((-1, 7, 7, 64, 1), -2), ((1, 0, 7, 64, 1), -2), ((1, 7, 0, 64, 1), -2),
                                     ((1, 7, 7, 6, 1), -2), ((1, 7, 7, 0, 1), -2), ((1, 7, 7, 64, 3), -3),
                                     ((1, 7, 7, 64, 0), -3), ((1, 1 << 15, 1 << 15, 4, 1), -2),
                                     ((1 << 20, 1 << 10, 1 << 10, 64, 1), -2)])
def test_plan_refusals(dims, rc, pkg):
    with pytest.raises(pkg.WinoError, match=f"rc={rc}"):
        pkg.dwconv3x3_plan(*dims, CUS)
    assert pkg.dwconv3x3_plan(0, 7, 7, 64, 1, CUS)[0] == 16   # N = 0 is a legal, empty launch
