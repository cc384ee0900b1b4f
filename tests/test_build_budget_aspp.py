"""Build budget of aspp.hip, no GPU needed: it instantiates the tiled 1x1 kernel in operand form A_CAT (6) -- four
kernels, {4, 8 waves} x {plain, stream-K}, no latency kernel -- within the budgets tests/test_build_budget_dilated.py
holds the A_DIL kernels to, and no other translation unit instantiates that form."""
import os

from build_report import CSRC, compile_report, template_args

A_CAT = 6


def test_aspp_kernels_build_budget(tmp_path):
    k = compile_report("aspp.hip", tmp_path)
    assert len(k) == 4, sorted(k)
    args = sorted(template_args(n, "conv1x1_bn_kernel") for n in k)
    # <BK, NW, ABLATE, SK, RES, AF>
    assert args == [[32, 4, 0, 0, 0, A_CAT], [32, 4, 0, 1, 0, A_CAT], [32, 8, 0, 0, 0, A_CAT], [32, 8, 0, 1, 0, A_CAT]], args
    for name, v in k.items():
        print(name, v)
        eight = template_args(name, "conv1x1_bn_kernel")[1] == 8
        budget, waves = (128, 4) if eight else (168, 3)
        assert v["vgprs"] <= budget and v["occupancy"] >= waves and v["spill"] <= 8, (name, v)
        assert v["mfma"] >= 56 and v["spill_code_in_mfma_blocks"] == 0 and v["sgpr_spill"] <= 40, (name, v)


def test_no_other_file_instantiates_the_concat_form():
    """A template is instantiated where it is named: aspp.hip is the only translation unit that names the form, so the
    others compile exactly the kernels they had."""
    hips = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    assert "aspp.hip" in hips and "A_CAT" in open(os.path.join(CSRC, "aspp.hip")).read()
    for f in hips:
        if f == "aspp.hip":
            continue
        assert "A_CAT" not in open(os.path.join(CSRC, f)).read(), f
