"""Build budget of mask_paste.hip, no GPU needed: its one kernel compiles without a spill, at four waves per SIMD or
more, without a matrix instruction, and with no more than 64 KB of static LDS (it declares the 16 KB probability map of
the largest mask, (62 + 2)^2 floats)."""
from build_report import compile_report

LDS_LIMIT = 64 << 10


def test_mask_paste_kernel_build_budget():
    k = compile_report("mask_paste.hip")
    assert len(k) == 1 and any("mask_paste_kernel" in n for n in k), sorted(k)
    for name, v in k.items():
        print(name, v)
        assert v["spill"] == 0 and v["sgpr_spill"] == 0, (name, v)
        assert v["occupancy"] >= 4, (name, v)
        assert v["static_lds"] == 64 * 64 * 4 <= LDS_LIMIT, (name, v)
        assert v["mfma"] == 0, (name, v)
