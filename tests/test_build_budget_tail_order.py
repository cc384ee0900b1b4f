"""Build-time budget of the fused 3x3 kernel's hand-off (no GPU needed): the order of a range and the finish from
registers ("Hand-off") live in the prologue, the event code and the epilogue.  Every
instantiation with a stream-K tail -- the plain, the residual and the pooled epilogue, the 14x14 and the any-feature-map
form, the stamped diagnostic build -- must stay at two waves per SIMD (at most 256 VGPRs) without a VGPR spill and
without spill code of any kind in a block that holds MFMAs; the gather from registers holds one 8 x 16-byte temporary
beside the wave's own part.  The innermost loop keeps the instruction and branch counts test_build_budget_loop.py pins:
the order is settled once, in the prologue, and costs the loop nothing."""
import pytest

from build_report import compile_report, template_args
from test_build_budget_loop import innermost_mfma_loop, loop_counts   # the loop finder and its counters, as pinned there

SOURCES = ["wino_f2_fused.hip", "conv3x3_res.hip", "conv3x3_pool.hip"]


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    out = {}
    for src in SOURCES:
        tmp = tmp_path_factory.mktemp(src.replace(".", "_"))
        kernels = {n: v for n, v in compile_report(src, tmp).items() if "wino_f2_fused_kernel" in n}
        isa = [f for f in tmp.iterdir() if f.name.endswith(".s") and "gfx950" in f.name]
        assert len(isa) == 1, isa
        text = isa[0].read_text()
        for name, v in kernels.items():
            i = text.index(name + ":")
            v["body"] = text[i:text.index(".Lfunc_end", i)].splitlines()
            out[(src, tuple(template_args(name, "wino_f2_fused_kernel")))] = v
    return out


def test_every_instantiation_is_there(reports):
    keys = sorted(k[1] for k in reports)
    # (ABLATE, GEN, TAIL, EPI): the stamped plain build, and {14x14, any map} x {tail, whole items} per epilogue form
    assert keys == sorted([(16, 0, 1, 0)] + [(0, g, t, e) for g in (0, 1) for t in (0, 1) for e in (0, 1, 2)]), keys


def test_registers_and_spills(reports):
    for key, v in reports.items():
        print(key, {k: v[k] for k in ("vgprs", "spill", "sgpr_spill", "occupancy", "spill_code_in_mfma_blocks")})
        assert v["vgprs"] <= 256 and v["occupancy"] >= 2, key
        assert v["spill"] == 0, key
        assert v["spill_code_in_mfma_blocks"] == 0, key
        assert v["mfma"] == 128, key


def test_the_order_costs_the_loop_nothing(reports):
    for key, v in reports.items():
        c = loop_counts(innermost_mfma_loop(v["body"]))
        print(key, c)
        assert c["mfma"] == 128 and c["lds_dma"] == 16, (key, c)
        assert c["instructions"] <= 450 and c["branches"] <= 4, (key, c)
        assert c["readlane"] == 0 and c["s_load"] == 0 and c["tile_decode"] == 0, (key, c)
