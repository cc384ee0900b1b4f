"""Build budget of keypoints.hip, no GPU needed: its one kernel compiles without a spill, at four waves per SIMD or more
(the bar mask_paste.hip holds), without a matrix instruction, and with no more than 64 KB of static LDS (it declares the
16 KB plane of the largest map, 64 x 64 floats, the 4 KB low map of DECONV_ROWS, and a row per wave)."""
from build_report import compile_report

LDS_LIMIT = 64 << 10


def test_keypoints_kernel_build_budget():
    k = compile_report("keypoints.hip")
    assert len(k) == 1 and any("keypoints_kernel" in n for n in k), sorted(k)
    for name, v in k.items():
        print(name, v)
        assert v["spill"] == 0 and v["sgpr_spill"] == 0, (name, v)
        assert v["occupancy"] >= 4, (name, v)
        assert 64 * 64 * 4 + 32 * 32 * 4 <= v["static_lds"] <= LDS_LIMIT, (name, v)
        assert v["mfma"] == 0, (name, v)
