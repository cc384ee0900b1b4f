"""Build budget of the GroupNorm and FCOS kernels, no GPU needed.  groupnorm.hip compiles exactly its three kernels (the
whole form, and the split form's statistics and apply), fcos.hip exactly its score-map and decode kernels: no VGPR or SGPR
spill, no scratch, no MFMA.  The streaming kernels (statistics, apply, score) keep four waves per SIMD or more and at
most 16 KiB of static LDS; the whole-form kernel's LDS is the one array it declares, 12 floats per thread of its 1024
(three per group slot, four slots); the decode kernel has no LDS and at most 64 VGPRs, like RetinaNet's."""
import os
import re

from build_report import compile_report

GN_KERNELS = ["gn_whole_kernel", "gn_stats_kernel", "gn_apply_kernel"]
FCOS_KERNELS = ["fcos_score_kernel", "fcos_decode_kernel"]
WHOLE_LDS_BYTES = 12 * 1024 * 4


def _report(src, tmp_path, wanted):
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
    by = {want: [n for n in k if want in n] for want in wanted}
    assert all(len(v) == 1 for v in by.values()) and len(k) == len(wanted), sorted(k)
    return {want: k[name] for want, (name,) in by.items()}


def test_groupnorm_kernels_build_budget(tmp_path):
    k = _report("groupnorm.hip", tmp_path, GN_KERNELS)
    for name in ("gn_stats_kernel", "gn_apply_kernel"):
        assert k[name]["occupancy"] >= 4 and k[name]["static_lds"] <= 16 << 10, (name, k[name])
    assert k["gn_apply_kernel"]["static_lds"] == 0, k["gn_apply_kernel"]
    # 1024 threads are 4 waves per SIMD: the register budget of the launch bound is 128
    assert k["gn_whole_kernel"]["static_lds"] == WHOLE_LDS_BYTES and k["gn_whole_kernel"]["vgprs"] <= 128, k["gn_whole_kernel"]


def test_fcos_kernels_build_budget(tmp_path):
    k = _report("fcos.hip", tmp_path, FCOS_KERNELS)
    assert k["fcos_score_kernel"]["occupancy"] >= 4 and k["fcos_score_kernel"]["static_lds"] == 0, k["fcos_score_kernel"]
    v = k["fcos_decode_kernel"]
    assert v["static_lds"] == 0 and v["occupancy"] >= 4 and v["vgprs"] <= 64, v
