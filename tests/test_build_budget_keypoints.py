"""Build budget of keypoints.hip, no GPU needed: its one kernel compiles without a spill, at four waves per SIMD or more
(the bar mask_paste.hip holds), without a matrix instruction, and with no more than 64 KB of static LDS (it declares the
16 KB plane of the largest map, 64 x 64 floats, the 4 KB low map of DECONV_ROWS, and a row per wave)."""
import os
import re

from build_report import compile_report

LDS_LIMIT = 64 << 10


def test_keypoints_kernel_build_budget(tmp_path):
    k = compile_report("keypoints.hip", tmp_path)
    assert len(k) == 1 and any("keypoints_kernel" in n for n in k), sorted(k)
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
        assert 64 * 64 * 4 + 32 * 32 * 4 <= v["static_lds"] <= LDS_LIMIT, (name, v)
        assert v["mfma"] == 0, (name, v)
