"""Host-side checks of the multi-launch entry points -- no GPU needed: every block refuses a NULL or misaligned tensor,
a workspace inside x or out, and a shape that only a later layer refuses, before its first device query.  The addresses
are fake and never dereferenced: a call that got past the checks would return WINO_E_HIP on a machine without a GPU."""
import ctypes

import pytest

E_SHAPE, E_ARG = -2, -3
GIB = 1 << 30
F = 4   # bytes per float


class Block:
    """One entry point `fn(pointers..., shape..., workspace, workspace_bytes, stream)`.  `kinds` lists its pointer
    arguments in order: a 16-byte-aligned tensor ("t"), a BN vector ("v": 4-byte alignment only); the workspace comes
    after the shape.  Each pointer gets its own GiB-spaced address; x_bytes / out_bytes are the sizes of x and out."""

    def __init__(self, fn, kinds, shape, ws_need, x_bytes, out_bytes):
        self.fn, self.kinds, self.shape = fn, dict(kinds, ws="t"), shape
        self.ws_need, self.bytes = ws_need, {"x": x_bytes, "out": out_bytes}
        self.addr = {name: (i + 1) * GIB for i, name in enumerate(self.kinds)}

    def call(self, L, shape=None, **override):
        a = dict(self.addr, **override)
        p = [None if a[n] is None else ctypes.c_void_p(a[n]) for n in self.kinds]
        return getattr(L, self.fn)(*p[:-1], *(shape or self.shape), p[-1], self.ws_need, None)


def _blocks(L):
    N, H, C4, Cm = 1, 14, 256, 64
    act = N * H * H * C4 * F
    res = {"x": "t", "w1": "t", "b1": "v", "s1": "v", "U2": "t", "b2": "v", "s2": "v", "w3": "t", "b3": "v", "s3": "v",
           "out": "t"}
    res_ws = L.wino_residual_block_workspace_bytes_hw(N, H, H, Cm)
    Hin, Cin, Ho = 28, 64, 14
    proj = {"x": "t", "w1": "t", "b1": "v", "s1": "v", "U2": "t", "b2": "v", "s2": "v", "tail": "t", "out": "t"}
    x_proj, out_proj = N * Hin * Hin * Cin * F, N * Ho * Ho * C4 * F
    Cg, groups = 128, 32    # the grouped blocks' middle width
    gres = {("wg" if k == "U2" else k): v for k, v in res.items()}
    gproj = {("wg" if k == "U2" else k): v for k, v in proj.items()}
    C, K = 64, 128
    bb = {"x": "t", "U1": "t", "b1": "v", "s1": "v", "U2": "t", "b2": "v", "s2": "v", "out": "t"}
    bb_act = 2 * (H + 2) * (H + 2) * C * F
    s2 = {"x": "t", "packed": "t", "U2": "t", "b2": "v", "s2": "v", "out": "t"}
    Cf, classes = 512, 1000
    head = {"x": "t", "packed": "t", "out": "t"}   # x: feat
    return {
        "wino_residual_block_hw": Block("wino_residual_block_hw", res, (N, H, H, C4, Cm), res_ws, act, act),
        "wino_residual_block": Block("wino_residual_block", res, (N, C4, Cm), res_ws, act, act),
        "wino_proj_block_hw": Block("wino_proj_block_hw", proj, (N, Hin, Hin, Cin, Cm, C4, 2),
                                    L.wino_proj_block_workspace_bytes_hw(N, Ho, Ho, Cm), x_proj, out_proj),
        "wino_proj_block_v15_hw": Block("wino_proj_block_v15_hw", proj, (N, Hin, Hin, Cin, Cm, C4),
                                        L.wino_proj_block_v15_workspace_bytes_hw(N, Hin, Hin, Cm), x_proj, out_proj),
        "wino_grouped_residual_block_hw": Block("wino_grouped_residual_block_hw", gres, (N, H, H, C4, Cg, groups),
                                                L.wino_residual_block_workspace_bytes_hw(N, H, H, Cg), act, act),
        "wino_grouped_proj_block_hw": Block("wino_grouped_proj_block_hw", gproj, (N, Hin, Hin, Cin, Cg, C4, groups, 2),
                                            L.wino_proj_block_v15_workspace_bytes_hw(N, Hin, Hin, Cg), x_proj, out_proj),
        "wino_basic_block_hw": Block("wino_basic_block_hw", bb, (2, H, H, C),
                                     L.wino_basic_block_workspace_bytes_hw(2, H, H, C), bb_act, bb_act),
        "wino_basic_block_s2_hw": Block("wino_basic_block_s2_hw", s2, (2, Hin, Hin, C, K),
                                        L.wino_basic_block_s2_workspace_bytes_hw(2, Hin, Hin, K),
                                        2 * (Hin + 2) * (Hin + 2) * C * F, 2 * (Ho + 2) * (Ho + 2) * K * F),
        "wino_avgpool_fc_hw": Block("wino_avgpool_fc_hw", head, (2, 7, 7, Cf, classes, 1),
                                    L.wino_head_workspace_bytes(2, Cf, classes), 2 * 9 * 9 * Cf * F, 2 * classes * F),
    }


@pytest.mark.parametrize("name", ["wino_residual_block_hw", "wino_residual_block", "wino_proj_block_hw",
                                  "wino_proj_block_v15_hw", "wino_grouped_residual_block_hw",
                                  "wino_grouped_proj_block_hw", "wino_basic_block_hw", "wino_basic_block_s2_hw",
                                  "wino_avgpool_fc_hw"])
def test_blocks_refuse_before_their_first_launch(name, pkg):
    L = pkg.lib()
    b = _blocks(L)[name]
    for arg, kind in b.kinds.items():
        assert b.call(L, **{arg: None}) == E_ARG, arg                 # each pointer NULL in turn
        if kind == "t":                                               # each 16-byte-aligned tensor moved by 4 bytes
            assert b.call(L, **{arg: b.addr[arg] + 4}) == E_ARG, arg
            assert "16-byte aligned" in L.wino_last_error_string().decode(), arg
    for arg in ("x", "out"):                                          # a workspace inside x, inside out
        assert b.bytes[arg] > 256
        assert b.call(L, ws=b.addr[arg] + 256) == E_ARG, arg
        assert "overlap" in L.wino_last_error_string().decode(), arg
    if name.startswith("wino_residual_block"):
        # C4 = 96: legal for the first 1x1 (Cin % 32 == 0), refused by the last one (Kout % 64 == 0)
        shape = (1, 14, 14, 96, 64) if name.endswith("_hw") else (1, 96, 64)
        assert b.call(L, shape) == E_SHAPE
