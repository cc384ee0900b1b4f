"""Host-side checks of the stride-2 3x3 layer (wino_conv3x3_s2_*) and the v1.5 projection block (wino_proj_block_v15_*)
-- no GPU needed: the new C-ABI symbols, the workspace size, every argument and shape rejection (each fires before
the GPU is touched: on a machine without one, anything later fails with WINO_E_HIP instead), the plan's routing as
the plain 1x1 GEMM of shape (N*H*W, 9C, K), and the build budget of conv3x3_s2.hip, which instantiates the 1x1 kernel
templates in operand form A_TAPS only."""
import ctypes
import os

from build_report import compile_report, template_args
from conftest import ROOT

E_SHAPE, E_ARG = -2, -3
A_TAPS = 3
# the 3x3 of ResNet-50's v1.5 stage-entry blocks: (Hin, C = K)
STAGES = {"conv3": (56, 128), "conv4": (28, 256), "conv5": (14, 512)}
NEW = ["wino_conv3x3_s2_bn_relu_hw", "wino_conv3x3_s2_prepare_hw", "wino_conv3x3_s2_plan",
       "wino_proj_block_v15_workspace_bytes_hw", "wino_proj_block_v15_hw", "wino_proj_block_v15_prepare_hw"]


def test_new_symbols_exported_and_declared(pkg):
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "winograd_mi355x.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name + "(" in hdr, name
        assert name in pkg.ABI_SYMBOLS, name
    assert "is not supported: F(2x2,3x3) has no stride-2 form" not in hdr
    assert L.wino_abi_version() == 1


def test_workspace_sizes(pkg):
    L = pkg.lib()
    # t1 at the input resolution, t2 at the output's, both padded, Cm channels
    assert L.wino_proj_block_v15_workspace_bytes_hw(2, 56, 56, 128) == 2 * (58 * 58 + 30 * 30) * 128 * 4
    assert L.wino_proj_block_v15_workspace_bytes_hw(1, 15, 9, 64) == (17 * 11 + 10 * 7) * 64 * 4
    assert L.wino_proj_block_v15_workspace_bytes_hw(0, 56, 56, 128) == 0


def _plan(pkg, N, Hin, Win, C, K, cus=256):
    f = ctypes.c_int(-1)
    rc = pkg.lib().wino_conv3x3_s2_plan(N, Hin, Win, C, K, cus, ctypes.byref(f))
    return rc, f.value


def test_layer_rejections(pkg):
    L = pkg.lib()
    assert _plan(pkg, 2, 28, 28, 256, 256)[0] == 0
    assert _plan(pkg, 2, 28, 28, 48, 256)[0] == E_SHAPE            # C % 32
    assert _plan(pkg, 2, 28, 28, 256, 96)[0] == E_SHAPE            # K % 64
    assert _plan(pkg, 0, 28, 28, 256, 256)[0] == E_SHAPE           # no image
    assert _plan(pkg, 2, 0, 28, 256, 256)[0] == E_SHAPE
    assert _plan(pkg, 2, 28, 28, 256, 256, cus=0)[0] == E_ARG
    assert L.wino_conv3x3_s2_plan(2, 28, 28, 256, 256, 256, None) == E_ARG
    # the 32-bit limits: M = N*H*W < 2^31; a tile's window over the padded input (111 rows up to 4 (Win+2) pixels
    # apart, plus the taps' reach); B = 9 C K floats; the ring pass's 16-byte units
    assert _plan(pkg, 1 << 22, 56, 56, 64, 64)[0] == E_SHAPE       # M = 3.3e9
    assert _plan(pkg, 1, 1, 8186, 512, 64)[0] == E_SHAPE           # window: (111 * 4 * 8188 + ...) * 512 * 4 bytes
    assert _plan(pkg, 1, 1, 8186, 256, 64)[0] == 0                 # ... half the channels fit
    assert _plan(pkg, 1, 7, 7, 4096, 32768)[0] == E_SHAPE          # B: 9 * 4096 * 32768 * 4 bytes
    assert _plan(pkg, 1 << 20, 1, 1, 32, 4096)[0] == E_SHAPE       # ring: 2^20 images * 8 pixels * 1024 units
    assert _plan(pkg, 1 << 18, 1, 1, 32, 4096)[0] == 0
    assert _plan(pkg, 1, 3, 8200, 32, 64)[0] == E_SHAPE            # output 4100 wide: more than 4094
    # the entry points refuse bad arguments before they touch the GPU
    w, bad = ctypes.c_void_p(256), ctypes.c_void_p(260)
    args = [w] * 5
    for i in range(5):
        a = list(args)
        a[i] = None
        assert L.wino_conv3x3_s2_bn_relu_hw(*a, 1, 14, 14, 64, 64, 1, None) == E_ARG, i
    for i in (0, 1, 4):   # in, w_taps, out move 16 bytes per lane
        a = list(args)
        a[i] = bad
        assert L.wino_conv3x3_s2_bn_relu_hw(*a, 1, 14, 14, 64, 64, 1, None) == E_ARG, i
    assert L.wino_conv3x3_s2_bn_relu_hw(*args, 1, 14, 14, 48, 64, 1, None) == E_SHAPE
    assert L.wino_conv3x3_s2_bn_relu_hw(*args, 1, 14, 14, 64, 96, 1, None) == E_SHAPE
    assert L.wino_conv3x3_s2_bn_relu_hw(*args, 1 << 22, 56, 56, 64, 64, 1, None) == E_SHAPE
    assert L.wino_conv3x3_s2_bn_relu_hw(*args, 1, 1, 8186, 512, 64, 1, None) == E_SHAPE
    assert L.wino_conv3x3_s2_bn_relu_hw(*args, 1, 7, 7, 4096, 32768, 1, None) == E_SHAPE
    assert L.wino_conv3x3_s2_bn_relu_hw(*args, 1 << 20, 1, 1, 32, 4096, 1, None) == E_SHAPE
    assert L.wino_conv3x3_s2_prepare_hw(1, 14, 14, 48, 64, None) == E_SHAPE
    assert "C % 32" in L.wino_last_error_string().decode()


def test_block_rejections(pkg):
    L = pkg.lib()
    w, bad = ctypes.c_void_p(256), ctypes.c_void_p(260)
    args = [w] * 9
    ws = 1 << 30
    run = lambda a, *shape, ws_ptr=w, ws_bytes=ws: L.wino_proj_block_v15_hw(*a, *shape, ws_ptr, ws_bytes, None)
    ok = (1, 14, 14, 64, 64, 128)
    assert run(args, 1, 14, 14, 48, 64, 128) == E_SHAPE                 # Cin % 32
    assert run(args, 1, 14, 14, 64, 96, 128) == E_SHAPE                 # Cm % 64
    assert run(args, 1, 14, 14, 64, 64, 96) == E_SHAPE                  # C4 % 64
    assert run(args, 0, 14, 14, 64, 64, 128) == E_SHAPE
    assert run(args, 1 << 22, 28, 28, 64, 64, 256) == E_SHAPE           # the first 1x1's N*Hin*Win rows (N*H*W fits)
    assert run(args, 1, 4100, 2, 64, 64, 64) == E_SHAPE                 # the first 1x1's 4100 x 2 map
    assert run(args, 1, 2, 4094, 32, 640, 64) == E_SHAPE                # the 3x3's window over t1
    assert run(args, 1, 7, 7, 64, 32768, 64) == E_SHAPE                 # the 3x3's B: 9 Cm^2 floats
    for i in range(9):
        a = list(args)
        a[i] = None
        assert run(a, *ok) == E_ARG, i
    for i in (0, 1, 4, 7, 8):   # x, w1, w2_taps, tail, out
        a = list(args)
        a[i] = bad
        assert run(a, *ok) == E_ARG, i
    assert run(args, *ok, ws_ptr=bad) == E_ARG                          # misaligned workspace
    assert run(args, *ok, ws_ptr=None) == E_ARG
    need = L.wino_proj_block_v15_workspace_bytes_hw(1, 14, 14, 64)
    assert run(args, *ok, ws_bytes=need - 4) == E_ARG                   # workspace too small
    assert "workspace" in L.wino_last_error_string().decode()
    assert L.wino_proj_block_v15_prepare_hw(1, 14, 14, 48, 64, 128, None) == E_SHAPE


def _form_1x1(pkg, M, K, Kout):
    if pkg.small_plan_1x1(M, K, Kout, cus=256)[0]:
        return pkg.FORM_LATENCY
    v = [ctypes.c_int() for _ in range(5)]
    assert pkg.lib().wino_conv1x1_plan(M, K, Kout, 256, *[ctypes.byref(x) for x in v]) == 0
    return pkg.FORM_STREAM_K if v[4].value else pkg.FORM_TILED


# the forms the tap-form plan takes at N = 1, 2, 8, 16, 32, 128 on 256 CUs: the fastest measured form family at each
# point (profiles/proj_block_v15/policy.json)
ROUTES = {"conv3": "LLSTTT", "conv4": "LLLSSS", "conv5": "LLLSSS"}
N_ROUTED = (1, 2, 8, 16, 32, 128)


def test_plan_routes_as_measured(pkg, knobs):
    """The layer is planned as the 1x1 GEMM (N*H*W, 9C, K) with the latency-or-tiled choice re-priced for the tap form
    (conv3x3_s2.hip plan_s2): the latency form up to 8 images (conv3: 2), the tiled kernel beyond.  Where the plain
    1x1 models would route conv5 at 8 images to stream-K, the tap form takes the latency form; everywhere else the
    route is that of the plain GEMM.  Forced WINO_1X1_* knobs are reported as such."""
    for k in ("WINO_1X1_ALGO", "WINO_1X1_SMALL_KS", "WINO_1X1_SK", "WINO_1X1_SK_GRID"):
        knobs.unset(k)
    code = {"L": pkg.FORM_LATENCY, "S": pkg.FORM_STREAM_K, "T": pkg.FORM_TILED}
    for stage, (Hin, C) in STAGES.items():
        H = (Hin - 1) // 2 + 1
        for N, want in zip(N_ROUTED, ROUTES[stage]):
            assert _plan(pkg, N, Hin, Hin, C, C) == (0, code[want]), (stage, N)
            if (stage, N) != ("conv5", 8):
                assert code[want] == _form_1x1(pkg, N * H * H, 9 * C, C), (stage, N)
    assert _form_1x1(pkg, 8 * 7 * 7, 9 * 512, 512) == pkg.FORM_STREAM_K   # (what the plain models pick there)
    shape = (2, 28, 28, 256, 256)
    knobs.set("WINO_1X1_ALGO", "small")
    assert pkg.conv3x3_s2_plan(*shape) == pkg.FORM_LATENCY
    knobs.set("WINO_1X1_ALGO", "big")
    knobs.set("WINO_1X1_SK", 0)
    assert pkg.conv3x3_s2_plan(*shape) == pkg.FORM_TILED
    knobs.set("WINO_1X1_SK", 1)
    assert pkg.conv3x3_s2_plan(*shape) == pkg.FORM_STREAM_K


def test_tap_form_kernels_build_budget(tmp_path):
    """conv3x3_s2.hip instantiates the 1x1 kernel templates in form A_TAPS (3) only -- 4 tiled kernels ({4, 8 waves} x
    {plain, stream-K}) and 18 latency kernels (KS x RT x CT) -- within the budgets of the other forms
    (test_proj_block_host.py): the tiled kernel 128 VGPRs / 4 waves (8-wave) or 168 / 3 (4-wave), a few spills outside
    the loops at most; the latency kernels no spill at all; no spill code beside MFMAs."""
    k = compile_report("conv3x3_s2.hip", tmp_path)
    tiled = {n: v for n, v in k.items() if "conv1x1_bn_kernel" in n}
    small = {n: v for n, v in k.items() if "conv1x1_small_kernel" in n}
    assert len(tiled) == 4, sorted(tiled)
    assert len(small) == 18, sorted(small)
    assert set(k) == set(tiled) | set(small), sorted(k)
    assert all(template_args(n, "conv1x1_bn_kernel")[-1] == A_TAPS for n in tiled), sorted(tiled)
    assert all(template_args(n, "conv1x1_small_kernel")[-1] == A_TAPS for n in small), sorted(small)
    for name, v in tiled.items():
        eight = "ILi32ELi8E" in name
        assert eight or "ILi32ELi4E" in name, name
        budget, waves = (128, 4) if eight else (168, 3)
        assert v["vgprs"] <= budget and v["occupancy"] >= waves and v["spill"] <= 8, (name, v)
        assert v["mfma"] >= 56 and v["spill_code_in_mfma_blocks"] == 0 and v["sgpr_spill"] <= 40, (name, v)
    for name, v in small.items():
        assert v["spill"] == 0 and v["sgpr_spill"] == 0 and v["spill_code_in_mfma_blocks"] == 0, (name, v)


def test_tap_offset_is_scalar_in_the_k_loop(tmp_path):
    """The tiled kernel's A offset of a k-step is one wave-uniform scalar in every operand form.  Computed on the VALU,
    it has to reach the LDS-DMA's soffset through a readfirstlane loop around every A piece (v_readfirstlane,
    v_cmp_eq, s_and_saveexec, ..., s_cbranch_execnz) inside the MFMA loop.  None of that, and no per-lane multiply,
    may sit in a basic block with MFMAs of the tap-form kernels."""
    import re
    import shutil
    import subprocess
    from build_report import CSRC
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    asm = tmp_path / "s2.s"
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                          "-I" + CSRC, "--cuda-device-only", "-S", os.path.join(CSRC, "conv3x3_s2.hip"), "-o", str(asm)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    text = asm.read_text()
    names = re.findall(r"^(_ZN4wino7gemm1x117conv1x1_bn_kernel\w+):", text, re.M)
    assert len(names) == 4, names
    for name in names:
        i = text.index("\n" + name + ":") + 1
        body = text[i:text.index(".Lfunc_end", i)]
        hot = [b for b in re.split(r"\n(?=\.LBB\d+_\d+:)", body) if "v_mfma" in b]
        assert hot, name
        for op in ("v_readfirstlane", "s_and_saveexec", "v_mul_lo_u32"):
            assert sum(b.count(op) for b in hot) == 0, (name, op)
