"""Build budget of the depthwise K x K kernel and the squeeze-excite kernels, no GPU needed.  depthwise_ex.hip compiles
exactly the instantiations DESIGN.md section 3.2v lists, K x stride x channel block x pool: no VGPR or SGPR spill, no
scratch, no MFMA.  Each one's static LDS is its input patch, (s (TH-1) + K)(s (TW-1) + K) CB floats with the tile the plan
query names, plus, for K = 5, the copy of the 25 taps the kernel reads them from; it stays within the 64 KiB a workgroup
may declare statically.  128 VGPRs or fewer allow four waves per SIMD."""
import itertools

from build_report import assert_no_spill_scratch_or_mfma, compile_report, template_args

STATIC_LDS_LIMIT = 64 << 10


def test_depthwise_ex_kernels_build_budget(pkg, knobs):
    k = compile_report("depthwise_ex.hip")
    assert_no_spill_scratch_or_mfma(k)
    by = {tuple(template_args(name, "dwx_kernel")): v for name, v in k.items()}
    assert sorted(by) == sorted(itertools.product((3, 5), (1, 2), (16, 64), (0, 1))), sorted(k)
    for (K, stride, cb, pool), v in by.items():
        knobs.set("WINO_DW_CB", cb)
        got_cb, th, tw, _, _ = pkg.dwconv_plan(1, 40, 40, 64, K, stride)
        assert got_cb == cb
        lds = (stride * (th - 1) + K) * (stride * (tw - 1) + K) * cb * 4 + (25 * cb * 4 if K == 5 else 0)
        assert v["static_lds"] == lds <= STATIC_LDS_LIMIT, (K, stride, cb, pool, v)
        assert v["vgprs"] <= 128, (K, stride, cb, pool, v)


def test_se_kernels_build_budget():
    k = compile_report("se.hip")
    assert_no_spill_scratch_or_mfma(k)
    assert len(k) == 2 and all(v["static_lds"] <= STATIC_LDS_LIMIT for v in k.values()), sorted(k)
