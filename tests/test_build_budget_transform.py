"""Build budget of image_transform.hip, no GPU needed: its two kernels (the fp32 and the uint8 instantiation of the one
direct-gather form) compile without a spill, at four waves per SIMD or more, with no more than 64 KB of static LDS (the
uint8 one holds its 4 x 256-float table there, the fp32 one nothing to speak of) and without a matrix instruction."""
from build_report import compile_report

LDS_LIMIT = 64 << 10


def test_transform_kernels_build_budget():
    k = compile_report("image_transform.hip")
    assert len(k) == 2 and all("image_transform_kernel" in n for n in k), sorted(k)
    for name, v in k.items():
        print(name, v)
        assert v["spill"] == 0 and v["sgpr_spill"] == 0, (name, v)
        assert v["scratch"] == 0, (name, v)            # the by-value descriptors are read from the kernel arguments
        assert v["occupancy"] >= 4, (name, v)
        assert v["static_lds"] <= LDS_LIMIT, (name, v)
        assert v["mfma"] == 0, (name, v)
    lds = sorted(v["static_lds"] for v in k.values())
    assert lds[1] == 4 * 256 * 4 and lds[0] <= 16, lds
