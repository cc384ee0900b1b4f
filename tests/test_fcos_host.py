"""Host-side tests of the GroupNorm and FCOS kernels' references, cases, plan and limits; no GPU.  The fp64 GroupNorm
reference against torch.nn.functional.group_norm in fp64; the decode references against the coder's formula; the claim
that the `offset` case separates fp32 E[x^2] - E[x]^2 from centred fp32 arithmetic at cases.TIGHT; the plan and workspace
queries; every refusal the entry points make before they look at a pointer."""
import numpy as np
import pytest
import torch

import fcos_cases as fc
import groupnorm_cases as gc
import retina_cases as rc
from cases import TIGHT


@pytest.mark.parametrize("kind", gc.KINDS)
def test_groupnorm_reference_is_torch_in_fp64(kind):
    for (N, h, w, C, G) in ((2, 7, 11, 64, 32), (1, 2, 3, 128, 1), (3, 1, 1, 64, 64), (1, 13, 21, 256, 32)):
        if kind == "scales" and h * w * (C // G) == 1:
            # a group of one value of magnitude 1e3 has variance 0: torch applies x * a + (beta - mean * a) with
            # a = gamma / sqrt(eps), and the two terms of 3e5 cancel to 5e-11 in fp64; the reference gives beta exactly
            h, w = 1, 2
        x, gamma, beta = gc.case(kind, N, h, w, C, G)
        xd = torch.from_numpy(x).double()
        if kind == "offset":
            # GroupNorm does not see a shift of a whole group, and float32 - 64 is exact in fp64: torch gets the centred
            # values, because its own fp64 statistics lose (mean / std)^2 = 4096 ulps at the offset (1.6e-12 here)
            xd = xd - 64.0 * torch.where((torch.arange(C) // (C // G)) % 2 == 0, 1.0, -1.0).double()
        for relu in (True, False):
            want = torch.nn.functional.group_norm(xd.permute(0, 3, 1, 2), G,
                                                  torch.from_numpy(gamma).double(), torch.from_numpy(beta).double(), gc.EPS)
            want = (want.relu() if relu else want).permute(0, 2, 3, 1).numpy()
            got = gc.reference(x, gamma, beta, G, relu=relu)
            assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0)


def test_groupnorm_reference_nan_and_inf_as_torch():
    x, gamma, beta = gc.case("plain", 2, 3, 5, 64, 32)
    for bad in (np.nan, np.inf):
        hurt = x.copy()
        hurt[1, 2, 4, 7] = bad
        got = gc.reference(hurt, gamma, beta, 32)
        want = torch.nn.functional.group_norm(torch.from_numpy(hurt).double().permute(0, 3, 1, 2), 32,
                                              torch.from_numpy(gamma).double(), torch.from_numpy(beta).double(), gc.EPS)
        want = want.permute(0, 2, 3, 1).numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.isnan(got[1, :, :, 6:8]).all() and np.isnan(got).sum() == 3 * 5 * 2


def _fp32_groupnorm(x, gamma, beta, G, centred, chunk=64):
    """GroupNorm in fp32 numpy: statistics from E[x^2] - E[x]^2, or from per-chunk (count, mean, M2) merged in chunk order
    by Chan's formula and a centred apply."""
    f = np.float32
    N, h, w, C = x.shape
    g = x.reshape(N, h * w, G, C // G).transpose(0, 2, 1, 3).reshape(N, G, -1).astype(f)
    if centred:
        n, mean, m2 = f(0), np.zeros((N, G), f), np.zeros((N, G), f)
        for s in range(0, g.shape[2], chunk):
            part = g[:, :, s:s + chunk]
            nb, mb = f(part.shape[2]), part.mean(axis=2, dtype=f)
            m2b = ((part - mb[..., None]) ** 2).sum(axis=2, dtype=f)
            tot = n + nb
            d, r = mb - mean, nb / tot
            mean, m2, n = mean + d * r, (m2 + m2b) + (d * d) * (n * r), tot
        var = m2 / n
    else:
        mean = g.mean(axis=2, dtype=f)
        var = (g * g).mean(axis=2, dtype=f) - mean * mean
    rstd = (f(1) / np.sqrt(var + f(gc.EPS))).astype(f)
    y = (g - mean[..., None]) * rstd[..., None]
    y = y.reshape(N, G, h * w, C // G).transpose(0, 2, 1, 3).reshape(N, h, w, C) * gamma + beta
    return np.where(y < 0, f(0), y)


@pytest.mark.parametrize("h,w,cpg", [(7, 11, 2), (25, 42, 8)])
def test_the_offset_case_separates_the_two_formulas(h, w, cpg):
    C = 64
    x, gamma, beta = gc.case("offset", 1, h, w, C, C // cpg)
    want = gc.reference(x, gamma, beta, C // cpg)
    naive = gc.rel_err(_fp32_groupnorm(x, gamma, beta, C // cpg, centred=False), want)
    centred = gc.rel_err(_fp32_groupnorm(x, gamma, beta, C // cpg, centred=True), want)
    print(f"{h}x{w}x{cpg}: E[x^2] - E[x]^2 {naive:.2e}, centred {centred:.2e}")
    assert centred < TIGHT / 2 and naive > 5 * TIGHT          # room on both sides of the bar


def test_cases_claims():
    x, gamma, beta = gc.case("constant", 2, 7, 11, 64, 32)
    want = gc.reference(x, gamma, beta, 32)
    assert np.abs(want[..., :2] - np.maximum(beta[:2], 0)).max() < 1e-12
    x, gamma, beta = gc.case("gamma0", 2, 7, 11, 64, 32)
    assert np.array_equal(gc.reference(x, gamma, beta, 32), np.broadcast_to(np.maximum(beta.astype(np.float64), 0), x.shape))
    x, _, _ = gc.case("scales", 1, 7, 11, 64, 32)
    assert np.abs(x[..., :2]).max() < 1e-2 and np.abs(x[..., 2:4]).max() > 1e2
    x, _, _ = gc.case("offset", 1, 13, 21, 64, 32)
    assert abs(abs(x[..., :2].mean()) / x[..., :2].std() - 64) < 8
    assert len(gc.sweep_specs()) == gc.SWEEP_COUNT
    for s in gc.sweep_specs():
        assert s["C"] % 64 == 0 and s["C"] % s["G"] == 0 and (s["C"] // s["G"]) & (s["C"] // s["G"] - 1) == 0
    assert {s["form"] for s in gc.sweep_specs()} == {None, "whole", "split"}


def test_groupnorm_plan_and_workspace(pkg, knobs):
    knobs.unset("WINO_GN_FORM")
    # FCOS's levels at C = 256, G = 32: whichever form, chunks and workspace agree with it
    for N in (1, 2):
        for h, w in ((100, 168), (50, 84), (25, 42), (13, 21), (7, 11)):
            form, chunks = pkg.groupnorm_plan(N, h, w, 256, 32)
            need = pkg.groupnorm_workspace_bytes(N, h, w, 256, 32)
            if form == "whole":
                assert chunks == 1 and need == 0
            else:
                assert 1 <= chunks <= 128 and need == N * min(h * w, 128) * 4 * 32 * 4
    assert pkg.groupnorm_plan(1, 7, 11, 256, 32)[0] == "whole" and pkg.groupnorm_plan(1, 100, 168, 256, 32)[0] == "split"
    knobs.set("WINO_GN_FORM", "split")
    for cus in (1, 64, 256, 304):
        form, chunks = pkg.groupnorm_plan(1, 37, 29, 64, 32, cus)
        assert form == "split" and chunks >= 1
    form, chunks = pkg.groupnorm_plan(1, 37, 29, 64, 32, 256)
    assert chunks > 1 and (37 * 29) % chunks != 0
    assert pkg.groupnorm_plan(2, 1, 1, 64, 32) == ("split", 1)
    assert pkg.groupnorm_workspace_bytes(2, 1, 1, 64, 32) == 2 * 1 * 4 * 32 * 4
    knobs.set("WINO_GN_FORM", "whole")
    assert pkg.groupnorm_plan(1, 100, 168, 256, 32) == ("whole", 1) and pkg.groupnorm_workspace_bytes(1, 100, 168, 256, 32) == 0
    for bad in ((1, 0, 5, 64, 32), (1, 5, 5, 32, 32), (1, 5, 5, 96, 32), (1, 5, 5, 192, 1), (1, 5, 5, 64, 3), (-1, 5, 5, 64, 32)):
        with pytest.raises(pkg.WinoError, match="rc=-2"):
            pkg.groupnorm_plan(*bad)
        with pytest.raises(pkg.WinoError, match="rc=-2"):
            pkg.groupnorm_workspace_bytes(*bad)
    with pytest.raises(pkg.WinoError, match="rc=-2"):
        pkg.groupnorm_plan(1, 5, 5, 64, 32, cus=0)


def test_shape_refusals_come_before_any_pointer(pkg):
    L = pkg.lib()
    for dims in ((1, 0, 5, 64, 32), (1, 5, 5, 96, 32), (1, 5, 5, 64, 5), (1, 5, 5, 128, 1 << 8), (1, 1 << 20, 1 << 14, 64, 32)):
        assert L.wino_groupnorm_relu_hw(None, None, None, None, *dims, 1e-5, 1, None, 0, None) == -2, dims
        assert b"groupnorm_relu" in L.wino_last_error_string()
    assert L.wino_groupnorm_relu_hw(None, None, None, None, 0, 5, 5, 64, 32, 1e-5, 1, None, 0, None) == 0
    assert L.wino_fcos_score_map_hw(None, None, 1, 3, 5, 65, 64, 64, 4, None) == -2
    assert L.wino_fcos_score_map_hw(None, None, 0, 3, 5, 5, 64, 64, 4, None) == 0
    assert L.wino_fcos_decode_hw(None, 2, 5, 5, 0, None, 3, 5, 2, 1, 5, None, 8, 8, None, None, None, None) == -2   # 4 A > ld_r
    assert b"fcos_decode" in L.wino_last_error_string()
    assert L.wino_fcos_decode_hw(None, 2, 0, 5, 0, None, 3, 5, 64, 1, 5, None, 8, 8, None, None, None, None) == 0
    assert L.wino_fcos_decode_hw(None, 2, 5, 5, 0, None, 3, 5, 64, 1, 5, None, 8, 8, None, None, None, None) == -3  # NULL
    assert L.wino_retina_decode_hw(None, 2, 5, 5, 1, None, 3, 5, 64, 1, 5, None, 8, 8, None, 4.0, None, None, None) == -2
    assert b"retina_decode" in L.wino_last_error_string()


def test_decode_references_are_the_coders_formula():
    c = rc.decode_level(7, 11, 1, 5)
    got64, got32 = fc.decode_fp64(c), fc.decode_fp32(c)
    assert got32.dtype == np.float32 and np.abs(got32 - got64).max() / np.abs(got64).max() < 1e-6
    gh, gw, sy, sx = c.grid
    for n, y, x in ((0, 0, 0), (1, 3, 7), (1, 6, 10)):
        anchor = c.base[0].astype(np.float64) + np.array([x * sx, y * sy, x * sx, y * sy])
        want = fc.coder_formula(anchor, c.deltas[n, y, x, 0], c.image_hw[n])
        assert np.abs(got64[n, y * c.w + x] - want).max() < 1e-12
    assert (c.deltas < 0).any() and (got64[..., 2] >= got64[..., 0]).all()


def test_score_reference_is_torchs_formula():
    c = fc.score_level(3, 5, 5)
    want = torch.sqrt(torch.sigmoid(torch.from_numpy(c.logits).double()) * torch.sigmoid(torch.from_numpy(c.ctr).double())[..., None])
    assert np.abs(fc.score_reference(c.logits, c.ctr) - want.numpy()).max() < 1e-14
    assert np.isnan(c.cls_map()[:, 0]).all() and np.isnan(c.reg_map()[..., :fc.CTR_COL]).all()


# ---- the FCOS head's reference and state dict ------------------------------------------------------------------------------
def test_head_reference_is_the_torch_module_tree():
    import fcos_reference as fr
    C, classes = 64, 5
    sd = fr.head_state_dict(C, classes, seed=3)
    head = fr.torch_head(C, classes).double()
    head.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    g = torch.Generator().manual_seed(4)
    feats = {name: torch.randn(2, h, w, C, generator=g) for name, (h, w) in zip(fr.LEVELS, fr.LEVEL_HW)}
    with torch.no_grad():
        for name, (cls, reg, ctr) in zip(fr.LEVELS, fr.head_reference(sd, feats)):
            want = head(feats[name].double().permute(0, 3, 1, 2))
            for got, w in zip((cls, reg, ctr[..., None]), want):
                assert (got - w.permute(0, 2, 3, 1)).abs().max() <= 1e-12 * max(float(w.abs().max()), 1.0)


def test_fcos_head_state_dict_validation(pkg):
    import importlib

    import fcos_reference as fr
    det = importlib.import_module("cuda_winograd_amd.detection")
    sd = fr.head_state_dict(64, 5, seed=3)
    assert det.validate_fcos_head_state_dict(sd, 64) == 5
    assert set(det.expected_fcos_head_keys(64, 5)) == set(sd)
    for key in ("classification_head.conv.4.weight", "regression_head.conv.10.bias", "regression_head.bbox_ctrness.weight",
                "classification_head.conv.9.bias"):
        with pytest.raises(pkg.WinoError, match="state dict"):
            det.validate_fcos_head_state_dict({k: v for k, v in sd.items() if k != key}, 64)
    with pytest.raises(pkg.WinoError, match="state dict"):
        det.validate_fcos_head_state_dict({**sd, "classification_head.conv.2.weight": torch.zeros(1)}, 64)
    with pytest.raises(pkg.WinoError, match="state dict"):
        det.validate_fcos_head_state_dict({**sd, "classification_head.conv.1.weight": torch.zeros(32)}, 64)
    with pytest.raises(pkg.WinoError, match="state dict"):
        det.validate_fcos_head_state_dict({**sd, "regression_head.bbox_reg.weight": torch.zeros(5, 64, 3, 3)}, 64)
    with pytest.raises(pkg.WinoError, match="multiple of 64"):
        det.validate_fcos_head_state_dict(fr.head_state_dict(96, 5), 96)
    assert det.score_threshold(0.2) == float(np.nextafter(np.float32(0.2), np.float32(1)))
    assert np.float32(det.score_threshold(0.2)) > np.float32(0.2)
    with pytest.raises(pkg.WinoError, match="score_thresh"):
        det.score_threshold(1.0)


def test_fcos_selection_and_decode_references():
    import fcos_reference as fr
    scores = np.array([[0.1, 0.5, 0.21, 0.9, 0.2, 0.3]])
    idx, count, tm, gap = fr.level_select_reference(scores, 3, 0.2)
    assert idx.tolist() == [[3, 1, 5]] and count.tolist() == [3] and tm == 0.0 and abs(gap - 0.09) < 1e-12
    idx, count, _, _ = fr.level_select_reference(scores[:, :3], 5, 0.2)
    assert idx.tolist() == [[1, 2, -1]] and count.tolist() == [2]
    c = rc.decode_level(7, 11, 1, 5)
    boxes, labels = fr.decode_selected_reference(c.deltas[:, :, :, 0, :], c.idx, c.base, c.grid, c.image_hw, c.K)
    want_boxes, want_labels = c.gather(fc.decode_fp64(c))
    assert np.array_equal(labels, want_labels) and np.abs(boxes - want_boxes).max() < 1e-12
