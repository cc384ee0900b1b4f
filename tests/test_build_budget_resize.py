"""Build budget of resize.hip, no GPU needed: its two kernels (the staged and the direct form) compile without a spill,
at four waves per SIMD or more, and with no more than 64 KB of static LDS (the staged form's is dynamic: the launch
asks for what the plan computed, at most 64 KB, so that two workgroups fit on a CU)."""
import os
import re

from build_report import compile_report

LDS_LIMIT = 64 << 10


def test_resize_kernels_build_budget(tmp_path):
    k = compile_report("resize.hip", tmp_path)
    assert len(k) == 2 and any("resize_staged_kernel" in n for n in k) and any("resize_direct_kernel" in n for n in k), sorted(k)
    isa = [f for f in os.listdir(tmp_path) if f.endswith(".s") and "gfx950" in f]
    assert len(isa) == 1, isa
    text = (tmp_path / isa[0]).read_text()
    for name, v in k.items():
        m = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\b.*?\.amdhsa_group_segment_fixed_size (\d+)", text, flags=re.S)
        assert m, name
        v["static_lds"] = int(m.group(1))
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
