"""MobileNetV3's tables and the K x K depthwise plan query, no GPU needed.  The parameter counts of expected_keys(arch,
1000), running statistics aside, are torchvision's documented ones; the kernel-size, SE and activation columns of the
block tables are torchvision's (and the paper's, Tables 1 and 2)."""
import importlib
import math

import pytest

KERNELS = {"large": "333555333333555", "small": "33355555555"}
SE = {"large": "000111000011111", "small": "10011111111"}
HS = {"large": "000000111111111", "small": "00011111111"}


@pytest.mark.parametrize("arch,params", [("large", 5483032), ("small", 2542856)])
def test_tables_and_parameter_count(arch, params, pkg):
    M = importlib.import_module("cuda_winograd_amd.mobilenet_v3")
    exp = M.expected_keys(arch, 1000)
    assert sum(math.prod(s) for k, s in exp.items() if "running_" not in k) == params
    rows = M.BLOCKS[arch]
    assert "".join(str(r[1]) for r in rows) == KERNELS[arch]
    assert "".join(str(int(r[4])) for r in rows) == SE[arch]
    assert "".join(str(int(r[5] == "HS")) for r in rows) == HS[arch]
    assert M.squeeze_channels(72) == 24 and M.squeeze_channels(16) == 8 and M.squeeze_channels(960) == 240


@pytest.mark.parametrize("dims,rc", [((1, 7, 7, 64, 4, 1), -3), ((1, 7, 7, 64, 7, 1), -3), ((1, 7, 7, 64, 5, 3), -3),
                                     ((1, 7, 7, 6, 5, 1), -2), ((1, 0, 7, 64, 5, 1), -2), ((-1, 7, 7, 64, 3, 1), -2),
                                     ((1, 1 << 15, 1 << 15, 4, 5, 1), -2)])
def test_plan_refusals(dims, rc, pkg):
    with pytest.raises(pkg.WinoError, match=f"rc={rc}"):
        pkg.dwconv_plan(*dims, 256)
    cb, th, tw, ty, tx = pkg.dwconv_plan(32, 14, 14, 672, 5, 2, 256)
    assert (cb, th, tw, ty, tx) == (64, 4, 8, 2, 1)
    assert pkg.dwconv_plan(1, 14, 14, 672, 5, 2, 256)[:3] == (16, 8, 8)
