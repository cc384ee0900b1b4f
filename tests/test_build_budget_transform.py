"""Build budget of image_transform.hip, no GPU needed: its two kernels (the fp32 and the uint8 instantiation of the one
direct-gather form) compile without a spill, at four waves per SIMD or more, with no more than 64 KB of static LDS (the
uint8 one holds its 4 x 256-float table there, the fp32 one nothing to speak of) and without a matrix instruction."""
import os
import re

from build_report import compile_report

LDS_LIMIT = 64 << 10


def test_transform_kernels_build_budget(tmp_path):
    k = compile_report("image_transform.hip", tmp_path)
    assert len(k) == 2 and all("image_transform_kernel" in n for n in k), sorted(k)
    isa = [f for f in os.listdir(tmp_path) if f.endswith(".s") and "gfx950" in f]
    assert len(isa) == 1, isa
    text = (tmp_path / isa[0]).read_text()
    for name, v in k.items():
        m = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\b.*?\.amdhsa_group_segment_fixed_size (\d+)", text, flags=re.S)
        assert m, name
        v["static_lds"] = int(m.group(1))
        m = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\b.*?\.amdhsa_private_segment_fixed_size (\d+)", text, flags=re.S)
        assert m, name
        v["scratch"] = int(m.group(1))
        print(name, v)
        assert v["spill"] == 0 and v["sgpr_spill"] == 0, (name, v)
        assert v["scratch"] == 0, (name, v)            # the by-value descriptors are read from the kernel arguments
        assert v["occupancy"] >= 4, (name, v)
        assert v["static_lds"] <= LDS_LIMIT, (name, v)
        assert v["mfma"] == 0, (name, v)
    lds = sorted(v["static_lds"] for v in k.values())
    assert lds[1] == 4 * 256 * 4 and lds[0] <= 16, lds
