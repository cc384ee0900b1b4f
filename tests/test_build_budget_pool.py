"""Register budgets of the pooled 3x3 kernels (conv3x3_pool.hip), with the report of build_report.py: the file
instantiates the two 3x3 kernel templates with the pooled epilogue only (EPI = 2), every throughput instantiation
within the plain kernel's budget -- at most 256 VGPRs, two waves per SIMD, no VGPR spill, 128 MFMAs, no spill code in
a block with MFMAs, at most 80 SGPR spills -- and every latency instantiation without a spill of either kind; and the
plain file still holds no instantiation of another epilogue."""
from build_report import compile_report, template_args

EPI_POOL = 2


def _of(kernels, family):
    return {n: template_args(n, family) for n in kernels if template_args(n, family) is not None}


def test_pool_file_compiles_the_pooled_kernels_only_within_budget(tmp_path):
    k = compile_report("conv3x3_pool.hip", tmp_path)
    fused = _of(k, "wino_f2_fused_kernel")
    small = _of(k, "wino_f2_small_kernel")
    assert len(k) == len(fused) + len(small), sorted(k)        # nothing else
    # throughput: <ABLATE = 0, GEN, TAIL, EPI = 2>, GEN x TAIL
    assert sorted(tuple(a) for a in fused.values()) == [(0, g, t, EPI_POOL) for g in (0, 1) for t in (0, 1)], fused
    # latency: <CT, GEN = 1, DIAG = 0, EPI = 2>: the general form for every feature map, 14x14 included
    assert sorted(tuple(a) for a in small.values()) == [(ct, 1, 0, EPI_POOL) for ct in (1, 2, 4)], small
    for name in fused:
        v = k[name]
        assert "Li16E" not in name, name
        assert v["vgprs"] <= 256 and v["occupancy"] >= 2 and v["spill"] == 0, (name, v)
        assert v["mfma"] == 128 and v["spill_code_in_mfma_blocks"] == 0 and v["sgpr_spill"] <= 80, (name, v)
    for name in small:
        v = k[name]
        assert v["spill"] == 0 and v["sgpr_spill"] == 0 and v["spill_code_in_mfma_blocks"] == 0, (name, v)
        assert v["mfma"] >= 32, (name, v)


def test_vgg_ops_file_spills_nothing(tmp_path):
    k = compile_report("vgg_ops.hip", tmp_path)
    assert sorted(n for n in k) and all("image_pack_kernel" in n or "avgpool7_flatten_kernel" in n for n in k), sorted(k)
    assert len(k) == 2, sorted(k)
    for name, v in k.items():
        assert v["spill"] == 0 and v["sgpr_spill"] == 0, (name, v)
