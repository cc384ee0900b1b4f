"""Build budget of the depthwise 3x3 kernel, no GPU needed.  depthwise.hip compiles exactly the four instantiations of its
one body (stride x channel block): no VGPR or SGPR spill, no scratch, no MFMA.  Each one's static LDS is its input patch,
(s (TH-1) + 3)(s (TW-1) + 3) CB floats with the tile sizes the plan query names, within the 64 KiB a workgroup may
declare statically; 128 VGPRs or fewer keep four waves per SIMD."""
from build_report import assert_no_spill_scratch_or_mfma, compile_report, template_args

STATIC_LDS_LIMIT = 64 << 10


def test_depthwise_kernels_build_budget(pkg, knobs):
    k = compile_report("depthwise.hip")
    assert_no_spill_scratch_or_mfma(k)
    by = {tuple(template_args(name, "dw_kernel")): v for name, v in k.items()}
    assert sorted(by) == [(1, 16), (1, 64), (2, 16), (2, 64)], sorted(k)
    for (stride, cb), v in by.items():
        knobs.set("WINO_DW_CB", cb)
        got_cb, th, tw, _, _ = pkg.dwconv3x3_plan(1, 40, 40, 64, stride)
        assert got_cb == cb
        patch = (stride * (th - 1) + 3) * (stride * (tw - 1) + 3) * cb * 4
        assert v["static_lds"] == patch <= STATIC_LDS_LIMIT, (stride, cb, v)
        assert v["vgprs"] <= 128 and v["occupancy"] >= 4, (stride, cb, v)
