"""Register budgets of the 1x1 kernels with the upsampled residual (WINO_RESIDUAL_UP2), which fpn.hip instantiates --
no GPU needed.  They are held to what tests/test_build_budget.py holds the same-size-residual kernels to: the tiled
kernel 128 VGPRs / 4 waves per SIMD (8-wave workgroups) or 168 / 3 (4-wave), no scratch at all here, spill code nowhere
beside MFMAs and at most 40 SGPRs parked in VGPR lanes; the latency kernel no spill of either kind."""
from build_report import compile_report, template_args

RES_UP2, A_PLAIN = 2, 0


def test_fpn_kernels_build_budget(tmp_path):
    k = compile_report("fpn.hip", tmp_path)
    tiled = {n: template_args(n, "conv1x1_bn_kernel") for n in k if "conv1x1_bn_kernel" in n}
    small = {n: template_args(n, "conv1x1_small_kernel") for n in k if "conv1x1_small_kernel" in n}
    assert len(k) == len(tiled) + len(small), sorted(k)          # the file instantiates nothing else
    # BK = 32, {4, 8 waves}, the product build, {plain, stream-K}, the upsampled residual, the plain operand form
    assert sorted(tiled.values()) == [[32, nw, 0, sk, RES_UP2, A_PLAIN] for nw in (4, 8) for sk in (0, 1)], tiled
    # KS {1, 2, 4} x RT {1, 2} x CT {1, 2, 4}, UP2, the plain operand form
    assert sorted(small.values()) == [[ks, rt, ct, 1, A_PLAIN] for ks in (1, 2, 4) for rt in (1, 2) for ct in (1, 2, 4)]
    for name, (_, nw, _, _, _, _) in tiled.items():
        v = k[name]
        budget, waves = (128, 4) if nw == 8 else (168, 3)
        assert v["vgprs"] <= budget and v["occupancy"] >= waves and v["spill"] == 0, (name, v)
        assert v["mfma"] >= 56 and v["spill_code_in_mfma_blocks"] == 0 and v["sgpr_spill"] <= 40, (name, v)
    for name in small:
        v = k[name]
        assert v["spill"] == 0 and v["sgpr_spill"] == 0 and v["spill_code_in_mfma_blocks"] == 0, (name, v)
        assert v["mfma"] >= 4, (name, v)


def test_the_other_files_instantiate_no_up2_kernel(tmp_path):
    """conv1x1.hip hands WINO_RESIDUAL_UP2 launches to fpn.hip and keeps exactly its kernels: no instantiation there
    carries the upsampled residual."""
    k = compile_report("conv1x1.hip", tmp_path)
    tiled = [template_args(n, "conv1x1_bn_kernel") for n in k if "conv1x1_bn_kernel" in n]
    small = [template_args(n, "conv1x1_small_kernel") for n in k if "conv1x1_small_kernel" in n]
    assert len(tiled) == 8 and len(small) == 18
    assert sorted({a[4] for a in tiled}) == [0, 1] and {a[3] for a in small} == {0}
