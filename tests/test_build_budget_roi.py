"""Build budget of roi_align.hip, no GPU needed: its kernel (one instantiation per sampling 1..4) compiles without a VGPR
or SGPR spill, at four waves per SIMD or more, with no MFMA, no static LDS and no scratch."""
import os
import re

from build_report import compile_report


def test_roi_align_kernel_build_budget(tmp_path):
    k = compile_report("roi_align.hip", tmp_path)
    assert len(k) == 4 and all("roi_align_kernel" in n for n in k), sorted(k)
    isa = [f for f in os.listdir(tmp_path) if f.endswith(".s") and "gfx950" in f]
    assert len(isa) == 1, isa
    text = (tmp_path / isa[0]).read_text()
    for name, v in sorted(k.items()):
        body = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\b(.*?)\.end_amdhsa_kernel", text, flags=re.S)
        assert body, name
        v["static_lds"] = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body.group(1)).group(1))
        v["scratch"] = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body.group(1)).group(1))
        print(name, v)
        assert v["spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0, (name, v)
        assert v["occupancy"] >= 4, (name, v)
        assert v["mfma"] == 0, (name, v)
        assert v["static_lds"] == 0, (name, v)
