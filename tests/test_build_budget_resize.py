"""Build budget of resize.hip, no GPU needed: its two kernels (the staged and the direct form) compile without a spill,
at four waves per SIMD or more, and with no more than 64 KB of static LDS (the staged form's is dynamic: the launch
asks for what the plan computed, at most 64 KB, so that two workgroups fit on a CU)."""
import os

from build_report import compile_report

LDS_LIMIT = 64 << 10


def test_resize_kernels_build_budget():
    k = compile_report("resize.hip")
    assert len(k) == 2 and any("resize_staged_kernel" in n for n in k) and any("resize_direct_kernel" in n for n in k), sorted(k)
    for name, v in k.items():
        print(name, v)
        assert v["spill"] == 0 and v["sgpr_spill"] == 0, (name, v)
        assert v["occupancy"] >= 4, (name, v)
        assert v["static_lds"] <= LDS_LIMIT, (name, v)
        assert v["mfma"] == 0, (name, v)


def test_dynamic_lds_request_is_bounded_by_the_plan():
    """The launch's dynamic LDS is the plan's figure, and the plan accepts no candidate above the limit."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "cuda-winograd_amd", "csrc", "resize.hip")).read()
    assert "constexpr int LDS_LIMIT = 64 << 10;" in src
    assert "if (b > LDS_LIMIT) continue;" in src and "(size_t)p.lds_bytes" in src
