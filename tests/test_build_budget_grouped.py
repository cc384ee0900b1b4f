"""Register budget of the grouped 3x3 kernel (conv3x3_grouped.hip), with the report of build_report.py: the file
compiles the pack kernel and the twelve instantiations of the one kernel body -- stride {1, 2} x tile width {8, 16} x
contraction width {16, 32, 64} -- and none spills a VGPR or an SGPR; bottleneck.hip, which composes every bottleneck
block (the grouped ones among them) as host code over existing launches, instantiates no kernel at all."""
from build_report import compile_report, template_args


def test_grouped_kernel_spills_nothing(tmp_path):
    k = compile_report("conv3x3_grouped.hip", tmp_path)
    conv = {n: tuple(template_args(n, "conv3x3_grouped_kernel")) for n in k if "conv3x3_grouped_kernel" in n}
    assert sorted(conv.values()) == [(s, tw, kc) for s in (1, 2) for tw in (8, 16) for kc in (16, 32, 64)], conv
    assert len(k) == len(conv) + 1 and any("grouped_pack_kernel" in n for n in k), sorted(k)
    for name, v in k.items():
        assert v["spill"] == 0 and v["sgpr_spill"] == 0 and v["spill_code_in_mfma_blocks"] == 0, (name, v)
    for name, (s, tw, kc) in conv.items():
        v = k[name]
        # nine taps x kc / 4 MFMAs x row tiles (4 at stride 1, 2 at stride 2), fully unrolled
        assert v["mfma"] == 9 * (kc // 4) * (4 if s == 1 else 2), (name, v)
        # two workgroups a CU at least: one stages its patch under the other's MFMAs
        assert v["occupancy"] >= 2, (name, v)


def test_grouped_blocks_instantiate_no_kernel(tmp_path):
    assert compile_report("bottleneck.hip", tmp_path) == {}
