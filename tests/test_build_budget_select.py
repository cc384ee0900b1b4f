"""Build budget of select.hip, no GPU needed: exactly its five kernels compile without a VGPR or SGPR spill, without
scratch and without an MFMA; the sort kernel's static LDS is the 64 KiB of keys DESIGN.md section 3.2p declares (plus its
one counter) and within the CU's 160 KiB; the histogram pass, and the count and gather passes with it, run at four waves
per SIMD or more."""
import os
import re

from build_report import compile_report

KERNELS = ["select_zero_kernel", "select_hist_kernel", "select_count_kernel", "select_gather_kernel", "select_sort_kernel"]
SORT_KEYS_BYTES = 8192 * 8      # 8192 composite keys of 8 bytes


def test_select_kernels_build_budget(tmp_path):
    k = compile_report("select.hip", tmp_path)
    by = {want: [n for n in k if want in n] for want in KERNELS}
    assert all(len(v) == 1 for v in by.values()) and len(k) == len(KERNELS), sorted(k)
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
        assert v["mfma"] == 0, (name, v)
        if name == by["select_sort_kernel"][0]:
            assert SORT_KEYS_BYTES <= v["static_lds"] <= SORT_KEYS_BYTES + 16 <= 160 << 10, (name, v)
        else:
            assert v["occupancy"] >= 4, (name, v)
            assert v["static_lds"] <= 16 << 10, (name, v)
