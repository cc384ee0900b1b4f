"""Build budget of RetinaNet's kernels, no GPU needed.  select_map.hip compiles exactly the four map-form kernels of
select_kernel.h and the shared zero kernel, retina.hip exactly its one decode kernel: no VGPR or SGPR spill, no scratch,
no MFMA.  The map form of the sort kernel keeps the 64 KiB of keys of DESIGN.md section 3.2p; the three passes over the
scores keep four waves per SIMD or more, as the flat form's do -- the index-to-address arithmetic costs no occupancy."""
import os
import re

from build_report import compile_report

MAP_KERNELS = ["select_zero_kernel", "select_hist_kernel", "select_count_kernel", "select_gather_kernel", "select_sort_kernel"]
SORT_KEYS_BYTES = 8192 * 8


def _report(src, tmp_path):
    k = compile_report(src, tmp_path)
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
    return k


def test_select_map_kernels_build_budget(tmp_path):
    k = _report("select_map.hip", tmp_path)
    by = {want: [n for n in k if want in n] for want in MAP_KERNELS}
    assert all(len(v) == 1 for v in by.values()) and len(k) == len(MAP_KERNELS), sorted(k)
    for want, (name,) in by.items():
        if want != "select_zero_kernel":
            assert "ILb1E" in name, f"{name}: not the map form"
        v = k[name]
        if want == "select_sort_kernel":
            assert SORT_KEYS_BYTES <= v["static_lds"] <= SORT_KEYS_BYTES + 16 <= 160 << 10, (name, v)
        else:
            assert v["occupancy"] >= 4, (name, v)
            assert v["static_lds"] <= 16 << 10, (name, v)


def test_retina_decode_kernel_build_budget(tmp_path):
    k = _report("retina.hip", tmp_path)
    assert len(k) == 1 and "retina_decode_kernel" in next(iter(k)), sorted(k)
    v = next(iter(k.values()))
    assert v["static_lds"] == 0 and v["occupancy"] >= 4 and v["vgprs"] <= 64, v
