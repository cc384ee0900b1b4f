"""Build budget of select.hip, no GPU needed: exactly its five kernels compile without a VGPR or SGPR spill, without
scratch and without an MFMA; the sort kernel's static LDS is the 64 KiB of keys DESIGN.md section 3.2p declares (plus its
one counter) and within the CU's 160 KiB; the histogram pass, and the count and gather passes with it, run at four waves
per SIMD or more."""
from build_report import assert_no_spill_scratch_or_mfma, compile_report, only

KERNELS = ["select_zero_kernel", "select_hist_kernel", "select_count_kernel", "select_gather_kernel", "select_sort_kernel"]
SORT_KEYS_BYTES = 8192 * 8      # 8192 composite keys of 8 bytes


def test_select_kernels_build_budget():
    k = compile_report("select.hip")
    by = only(k, KERNELS)
    assert_no_spill_scratch_or_mfma(k)
    for want, v in by.items():
        if want == "select_sort_kernel":
            assert SORT_KEYS_BYTES <= v["static_lds"] <= SORT_KEYS_BYTES + 16 <= 160 << 10, (want, v)
        else:
            assert v["occupancy"] >= 4, (want, v)
            assert v["static_lds"] <= 16 << 10, (want, v)
