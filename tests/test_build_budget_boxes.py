"""Build budget of boxes.hip, no GPU needed: exactly its three kernels (the scan in its four widths) compile without a
VGPR or SGPR spill, without scratch and without an MFMA; the decode and mask kernels at four waves per SIMD or more; the
scan's static LDS within 64 KiB."""
import os
import re

from build_report import compile_report, template_args

SCAN_WIDTHS = [64, 128, 256, 512]


def test_boxes_kernels_build_budget(tmp_path):
    k = compile_report("boxes.hip", tmp_path)
    decode = [n for n in k if "box_decode_kernel" in n]
    mask = [n for n in k if "nms_mask_kernel" in n]
    scan = [n for n in k if "nms_scan_kernel" in n]
    assert len(decode) == 1 and len(mask) == 1 and len(k) == 2 + len(scan), sorted(k)
    assert sorted(template_args(n, "nms_scan_kernel")[0] for n in scan) == SCAN_WIDTHS, sorted(scan)
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
        if name in scan:
            assert 0 < v["static_lds"] <= 64 << 10, (name, v)
        else:
            assert v["occupancy"] >= 4, (name, v)
