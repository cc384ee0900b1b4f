"""Build budget of boxes.hip, no GPU needed: exactly its three kernels (the scan in its four widths) compile without a
VGPR or SGPR spill, without scratch and without an MFMA; the decode and mask kernels at four waves per SIMD or more; the
scan's static LDS within 64 KiB."""
from build_report import assert_no_spill_scratch_or_mfma, compile_report, template_args

SCAN_WIDTHS = [64, 128, 256, 512]


def test_boxes_kernels_build_budget():
    k = compile_report("boxes.hip")
    decode = [n for n in k if "box_decode_kernel" in n]
    mask = [n for n in k if "nms_mask_kernel" in n]
    scan = [n for n in k if "nms_scan_kernel" in n]
    assert len(decode) == 1 and len(mask) == 1 and len(k) == 2 + len(scan), sorted(k)
    assert sorted(template_args(n, "nms_scan_kernel")[0] for n in scan) == SCAN_WIDTHS, sorted(scan)
    assert_no_spill_scratch_or_mfma(k)
    for name, v in sorted(k.items()):
        if name in scan:
            assert 0 < v["static_lds"] <= 64 << 10, (name, v)
        else:
            assert v["occupancy"] >= 4, (name, v)
