"""Build budget of roi_align.hip, no GPU needed: its kernel (one instantiation per sampling 1..4) compiles without a VGPR
or SGPR spill, at four waves per SIMD or more, with no MFMA, no static LDS and no scratch."""
from build_report import assert_no_spill_scratch_or_mfma, compile_report


def test_roi_align_kernel_build_budget():
    k = compile_report("roi_align.hip")
    assert len(k) == 4 and all("roi_align_kernel" in n for n in k), sorted(k)
    assert_no_spill_scratch_or_mfma(k)
    for name, v in sorted(k.items()):
        assert v["occupancy"] >= 4, (name, v)
        assert v["static_lds"] == 0, (name, v)
