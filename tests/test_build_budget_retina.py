"""Build budget of RetinaNet's kernels, no GPU needed.  select_map.hip compiles exactly the four map-form kernels of
select_kernel.h and the shared zero kernel, retina.hip exactly its one decode kernel: no VGPR or SGPR spill, no scratch,
no MFMA.  The map form of the sort kernel keeps the 64 KiB of keys of DESIGN.md section 3.2p; the three passes over the
scores keep four waves per SIMD or more, as the flat form's do -- the index-to-address arithmetic costs no occupancy."""
from build_report import assert_no_spill_scratch_or_mfma, compile_report, only

MAP_KERNELS = ["select_zero_kernel", "select_hist_kernel", "select_count_kernel", "select_gather_kernel", "select_sort_kernel"]
SORT_KEYS_BYTES = 8192 * 8


def test_select_map_kernels_build_budget():
    k = compile_report("select_map.hip")
    assert_no_spill_scratch_or_mfma(k)
    for want, v in only(k, MAP_KERNELS).items():
        name = v["name"]
        if want != "select_zero_kernel":
            assert "ILb1E" in name, f"{name}: not the map form"
        if want == "select_sort_kernel":
            assert SORT_KEYS_BYTES <= v["static_lds"] <= SORT_KEYS_BYTES + 16 <= 160 << 10, (name, v)
        else:
            assert v["occupancy"] >= 4, (name, v)
            assert v["static_lds"] <= 16 << 10, (name, v)


def test_retina_decode_kernel_build_budget():
    k = compile_report("retina.hip")
    assert_no_spill_scratch_or_mfma(k)
    assert len(k) == 1 and "retina_decode_kernel" in next(iter(k)), sorted(k)
    v = next(iter(k.values()))
    assert v["static_lds"] == 0 and v["occupancy"] >= 4 and v["vgprs"] <= 64, v
