"""cuda-winograd_amd -- MI355X-native fused Winograd conv(+BN+ReLU) and 1x1-conv GEMM.

Python side of the drop-in boundary: a ctypes binding of the C-ABI declared in
``include/winograd_mi355x.h`` (the same shared library the C ``./Test`` driver
links; the binding is ``_abi.py``), plus thin operator wrappers that take torch tensors.  PyTorch is only
plumbing here (device memory, streams, ``torch.distributed``); every compute
call goes to the hand-written HIP kernels in ``csrc/``.  There is NO CPU or
eager fallback: if the library is missing or no GPU is visible, calls raise.

The directory name contains a hyphen, so import it through
``__graft_entry__.load_package()`` (registers it as ``cuda_winograd_amd``).
"""
from __future__ import annotations

import ctypes
from ctypes import c_int, c_long, c_void_p

import torch  # imported first on purpose: the library then binds to torch's HIP runtime

from ._abi import (ABI_SYMBOLS, LIB_PATH, SIGNATURES, CpuBaselineResult, DriverResult, WinoError,  # noqa: F401
                   _check, lib)


def _dev(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise WinoError(f"{name} must be a CUDA(HIP) tensor -- this framework has no CPU path")
    if t.dtype != torch.float32:
        raise WinoError(f"{name} must be float32, got {t.dtype}")
    return t.contiguous()


def _stream() -> c_void_p:
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def tickets_in_use() -> int:
    """Diagnostic (tests): non-zero stream-K ticket counters of the current stream's scratch after a
    synchronise.  Every launch must leave 0."""
    n = c_long(0)
    _check(lib().wino_debug_tickets_in_use(_stream(), ctypes.byref(n)), "wino_debug_tickets_in_use")
    return int(n.value)


def stream_check() -> None:
    """Waits for the current stream; raises WinoError (WINO_E_STATE) when its library-owned scratch cannot
    be trusted (an earlier launch failed, or a kernel found a ticket counter that was not zero at launch)."""
    _check(lib().wino_stream_check(_stream()), "wino_stream_check")


def stream_reset_scratch() -> None:
    """Recovery: zero the current stream's ticket counters and clear its error state."""
    _check(lib().wino_stream_reset_scratch(_stream()), "wino_stream_reset_scratch")


def poison_ticket(index: int, value: int) -> None:
    """Test hook: overwrite one ticket counter of the current stream's scratch."""
    _check(lib().wino_debug_poison_ticket(_stream(), int(index), int(value)), "wino_debug_poison_ticket")


def last_clock_ghz(kernel: int = 0):
    """The clock the chip held inside the MOST RECENT launch of a product kernel (0 = fused 3x3, 1 = 1x1 GEMM)
    on the current device: (GHz, shader cycles, microseconds) between workgroup 0's entry and exit stamps,
    or None when no launch has stamped yet.  Synchronises the current stream."""
    st = (ctypes.c_ulonglong * 4)()
    _check(lib().wino_diag_last_clock(int(kernel), _stream(), st), "wino_diag_last_clock")
    cyc, ticks = st[2] - st[0], st[3] - st[1]
    if st[1] == 0 or ticks <= 0 or cyc <= 0:
        return None
    return cyc / ticks * 0.1, int(cyc), ticks / 100.0


def _plan_query(name: str, n: int, *args):
    """A host-side plan query of the library: `args`, then n int out-parameters, returned as a tuple."""
    v = [c_int(0) for _ in range(n)]
    _check(getattr(lib(), name)(*args, *[ctypes.byref(x) for x in v]), name)
    return tuple(int(x.value) for x in v)


def small_plan_3x3(N: int, C: int, K: int, cus: int = 256, H: int = 14, W: int = 14):
    """(use, point_rows, split, workgroups) of the 3x3 latency kernel for this shape (host-side)."""
    return _plan_query("wino_conv3x3_small_plan", 4, N, H, W, C, K, cus)


def small_plan_3x3_full(N: int, C: int, K: int, cus: int = 256, H: int = 14, W: int = 14):
    """(use, point_rows, split, col_tiles, workgroups) of the 3x3 latency kernel (host-side)."""
    return _plan_query("wino_conv3x3_small_plan2", 5, N, H, W, C, K, cus)


def small_plan_1x1(M: int, Cin: int, Kout: int, cus: int = 256):
    """(use, k_split, workgroups) of the 1x1 latency form for a plain layer of this shape (host-side)."""
    return _plan_query("wino_conv1x1_small_plan", 3, M, Cin, Kout, cus)


def small_plan_1x1_full(M: int, Cin: int, Kout: int, cus: int = 256):
    """(use, k_split, row_tiles, col_tiles, workgroups) of the 1x1 latency form (host-side)."""
    return _plan_query("wino_conv1x1_small_plan2", 5, M, Cin, Kout, cus)


def _on_current_device(*tensors) -> None:
    """The library launches on the CURRENT device's stream: every tensor must live there."""
    cur = torch.cuda.current_device()
    for t in tensors:
        if t is not None and t.device.index != cur:
            raise WinoError(f"tensor on cuda:{t.device.index} but the current device is cuda:{cur}: "
                            "wrap the call in torch.cuda.device(...)")


def _out(t: torch.Tensor, shape, name: str) -> torch.Tensor:
    """A caller-supplied output / workspace: written by the kernel as is, so it must be exactly what
    the kernel assumes (a wrong-sized or strided buffer would be an out-of-bounds GPU write)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise WinoError(f"{name} must be a float32 CUDA(HIP) tensor")
    if not t.is_contiguous():
        raise WinoError(f"{name} must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise WinoError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _output(t, shape, device, name: str = "out") -> torch.Tensor:
    """The caller's output checked by _out, or a new one of `shape` on `device`."""
    if t is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    return _out(t, shape, name)


def _workspace(t, need: int, device) -> torch.Tensor:
    """The caller's workspace, checked by _out and against `need` bytes, or a new one of `need` bytes."""
    if t is None:
        return torch.empty((need + 3) // 4, dtype=torch.float32, device=device)
    _out(t, None, "workspace")
    if t.numel() * 4 < need:
        raise WinoError(f"workspace too small: {t.numel() * 4} bytes, need {need}")
    return t


def _prepare(name: str, *dims) -> None:
    """A *_prepare entry point of the library: the shape as ints, then the current stream."""
    _check(getattr(lib(), name)(*(int(d) for d in dims), _stream()), name)


def _ws_args(ws: torch.Tensor):
    """(pointer, bytes): how every entry point takes a workspace."""
    return ws.data_ptr(), ws.numel() * 4


def _bn_vecs(*pairs):
    """Folded BN (bias, scale) pairs -> their vectors in the C argument order, each checked by _dev."""
    return [_dev(v, "bn") for pair in pairs for v in pair]


def _out_hw(h: int, w: int, stride: int):
    """The output grid of a centred (pad = kernel // 2) convolution or pool of this stride."""
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def _operands_3x3(inp, U, bn_bias, bn_scale, min_hp: int = 3, what: str = "inp must be [N][H+2][W+2][C]"):
    """The opening of the Winograd 3x3 layers: the four operands checked by _dev, the padded input's rank and minimum
    extent, and U / the BN vectors against C, K.  Returns (x, U, bias, scale, N, Hp, Wp, C, K)."""
    x = _dev(inp, "inp")
    U = _dev(U, "U")
    b, s = _dev(bn_bias, "bn_bias"), _dev(bn_scale, "bn_scale")
    shape = x.shape   # (read once: every .shape builds a new torch.Size, and this is the launch path)
    if len(shape) != 4 or shape[1] < min_hp or shape[2] < min_hp:
        raise WinoError(what)
    N, Hp, Wp, C, K = int(shape[0]), int(shape[1]), int(shape[2]), int(shape[3]), int(b.numel())
    if U.numel() != 16 * C * K or s.numel() != K:
        raise WinoError("U / bn vectors do not match C, K")
    return x, U, b, s, N, Hp, Wp, C, K


# --------------------------------------------------------------------------- operators
def filter_transform_f2(w_kcrs: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """[K][C][3][3] taps -> packed F(2x2,3x3) filter buffer (opaque layout, 16*C*K floats; `out`: the caller's)."""
    w = _dev(w_kcrs, "w_kcrs")
    K, C = int(w.shape[0]), int(w.shape[1])
    if tuple(w.shape[2:]) != (3, 3):
        raise WinoError("w_kcrs must be [K][C][3][3]")
    U = _output(out, (lib().wino_filter_f2_elems(C, K),), w.device)
    _check(lib().wino_filter_transform_f2(w.data_ptr(), U.data_ptr(), C, K, _stream()),
           "wino_filter_transform_f2")
    return U


def filter_import_f4(u36: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """The reference's weight_winograd_C_K.bin tensor [36][C][K] -> packed F(2x2) buffer."""
    u = _dev(u36, "u36")
    if u.dim() != 3 or u.shape[0] != 36:
        raise WinoError("u36 must be [36][C][K]")
    C, K = int(u.shape[1]), int(u.shape[2])
    U = _output(out, (lib().wino_filter_f2_elems(C, K),), u.device)
    _check(lib().wino_filter_import_f4(u.data_ptr(), U.data_ptr(), C, K, _stream()),
           "wino_filter_import_f4")
    return U


def conv3x3_bn_relu(inp: torch.Tensor, U: torch.Tensor, bn_bias: torch.Tensor,
                    bn_scale: torch.Tensor, relu: bool = True,
                    out: torch.Tensor | None = None) -> torch.Tensor:
    """inp [N][H+2][W+2][C] -> out [N][H+2][W+2][K] (interior H x W, zero ring).  One HIP launch.
    [N][16][16][C] is the reference's 14x14 stage (wino_conv3x3_bn_relu); any other even H, W goes
    through wino_conv3x3_bn_relu_hw."""
    x, U, b, s, N, Hp, Wp, C, K = _operands_3x3(inp, U, bn_bias, bn_scale)
    out = _output(out, (N, Hp, Wp, K), x.device)
    _on_current_device(x, U, b, s, out)
    if Hp == 16 and Wp == 16:
        _check(lib().wino_conv3x3_bn_relu(x.data_ptr(), U.data_ptr(), b.data_ptr(), s.data_ptr(),
                                          out.data_ptr(), N, C, K, int(relu), _stream()),
               "wino_conv3x3_bn_relu")
    else:
        _check(lib().wino_conv3x3_bn_relu_hw(x.data_ptr(), U.data_ptr(), b.data_ptr(), s.data_ptr(),
                                             out.data_ptr(), N, Hp - 2, Wp - 2, C, K, int(relu), _stream()),
               "wino_conv3x3_bn_relu_hw")
    return out


def conv3x3_f4_bn_relu(inp: torch.Tensor, u36: torch.Tensor, bn_bias: torch.Tensor, bn_scale: torch.Tensor,
                       relu: bool = True, out: torch.Tensor | None = None, workspace=None) -> torch.Tensor:
    """F(4x4,3x3) compatibility path: the reference's three stages on its own weight_winograd tensor
    u36 [36][C][K], consumed as is.  inp [N][16][16][C] -> out [N][16][16][K]."""
    x, u = _dev(inp, "inp"), _dev(u36, "u36")
    b, s = _dev(bn_bias, "bn_bias"), _dev(bn_scale, "bn_scale")
    if x.dim() != 4 or tuple(x.shape[1:3]) != (16, 16) or u.dim() != 3 or u.shape[0] != 36:
        raise WinoError("inp must be [N][16][16][C], u36 [36][C][K]")
    N, C, K = int(x.shape[0]), int(x.shape[3]), int(u.shape[2])
    if int(u.shape[1]) != C or b.numel() != K or s.numel() != K:
        raise WinoError("u36 / bn vectors do not match C, K")
    out = _output(out, (N, 16, 16, K), x.device)
    ws = _workspace(workspace, lib().wino_conv3x3_f4_workspace_bytes(N, C, K), x.device)
    _on_current_device(x, u, b, s, out, ws)
    _check(lib().wino_conv3x3_f4_bn_relu(x.data_ptr(), u.data_ptr(), b.data_ptr(), s.data_ptr(), out.data_ptr(),
                                         N, C, K, int(relu), *_ws_args(ws), _stream()),
           "wino_conv3x3_f4_bn_relu")
    return out


def conv3x3_prepare(N: int, C: int, K: int, H: int = 14, W: int = 14) -> None:
    """Allocate the library-owned stream-K scratch of conv3x3_bn_relu for this shape on the current
    device and stream ahead of time (needed before capturing the call into a HIP graph)."""
    _prepare("wino_conv3x3_prepare_hw", N, H, W, C, K)


def conv3x3_direct(inp, w_kcrs, bn_bias, bn_scale, relu: bool = True, out=None) -> torch.Tensor:
    """Comparator: direct 3x3 conv + BN + ReLU on the GPU (not the product path); any H, W."""
    x, w = _dev(inp, "inp"), _dev(w_kcrs, "w_kcrs")
    b, s = _dev(bn_bias, "bn_bias"), _dev(bn_scale, "bn_scale")
    N, Hp, Wp, C, K = int(x.shape[0]), int(x.shape[1]), int(x.shape[2]), int(x.shape[3]), int(w.shape[0])
    out = _output(out, (N, Hp, Wp, K), x.device)
    _check(lib().wino_conv3x3_direct_hw(x.data_ptr(), w.data_ptr(), b.data_ptr(), s.data_ptr(),
                                        out.data_ptr(), N, Hp - 2, Wp - 2, C, K, int(relu), _stream()),
           "wino_conv3x3_direct_hw")
    return out


def conv1x1_bn(A: torch.Tensor, B: torch.Tensor, bn_bias: torch.Tensor, bn_scale: torch.Tensor,
               relu: bool, out: torch.Tensor | None = None) -> torch.Tensor:
    """A [M][Cin] @ B [Cin][Kout] -> scale*(.)+bias (+ReLU), [M][Kout].  One HIP launch."""
    a, bm = _dev(A, "A"), _dev(B, "B")
    b, s = _dev(bn_bias, "bn_bias"), _dev(bn_scale, "bn_scale")
    if a.dim() != 2 or bm.dim() != 2 or a.shape[1] != bm.shape[0]:
        raise WinoError("A must be [M][Cin], B [Cin][Kout]")
    M, Cin, Kout = int(a.shape[0]), int(a.shape[1]), int(bm.shape[1])
    if b.numel() != Kout or s.numel() != Kout:
        raise WinoError("bn vectors do not match Kout")
    out = _output(out, (M, Kout), a.device)
    _on_current_device(a, bm, b, s, out)
    _check(lib().wino_conv1x1_bn(a.data_ptr(), bm.data_ptr(), b.data_ptr(), s.data_ptr(),
                                 out.data_ptr(), M, Cin, Kout, int(relu), _stream()),
           "wino_conv1x1_bn")
    return out


RELU, A_PADDED, C_PADDED, ADD_RESIDUAL = 1, 2, 4, 8  # WINO_* flag bits of wino_conv1x1_bn_ex
RESIDUAL_UP2 = 16  # WINO_RESIDUAL_UP2: with ADD_RESIDUAL, the residual is the padded coarser map (conv1x1_bn_ex)


def _up_hw(h: int, w: int):
    """The coarser map under an H x W one in a pyramid of stride-2 stages: ((H+1)//2, (W+1)//2)."""
    return (h + 1) // 2, (w + 1) // 2


def residual_block_prepare(N: int, C4: int, Cm: int, H: int = 14, W: int = 14) -> None:
    """Allocate the scratch of residual_block's three launches for the current stream (before graph capture)."""
    _prepare("wino_residual_block_prepare_hw", N, H, W, C4, Cm)


def conv3x3_clock_ghz(inp, U, bn_bias, bn_scale, out) -> float:
    """Diagnostic: one launch of the 3x3 throughput kernel's stamped build (14x14 only); returns the
    median over workgroups of the in-kernel clock, d(s_memtime) / d(s_memrealtime) * 0.1 GHz."""
    x, U = _dev(inp, "inp"), _dev(U, "U")
    b, s = _dev(bn_bias, "bn_bias"), _dev(bn_scale, "bn_scale")
    N, C, K = int(x.shape[0]), int(x.shape[3]), int(b.numel())
    _out(out, (N, 16, 16, K), "out")
    _on_current_device(x, U, b, s, out)
    stamps = torch.zeros(4 * 2048, dtype=torch.int64, device=x.device)
    wgs = c_int(0)
    _check(lib().wino_diag_conv3x3_clock(x.data_ptr(), U.data_ptr(), b.data_ptr(), s.data_ptr(), out.data_ptr(),
                                         N, C, K, stamps.data_ptr(), ctypes.byref(wgs), _stream()),
           "wino_diag_conv3x3_clock")
    st = stamps[:4 * wgs.value].view(-1, 4).cpu()      # {cycles, 100 MHz ticks} at start and at end
    cyc, ticks = (st[:, 2] - st[:, 0]).double(), (st[:, 3] - st[:, 1]).double()
    ok = (ticks > 0) & (st[:, 1] != 0)
    if not bool(ok.any()):
        raise WinoError("clock probe returned no stamps")
    return float((cyc[ok] / ticks[ok]).median()) * 0.1


def conv1x1_prepare(M: int, Cin: int, Kout: int) -> None:
    """Allocate the 1x1 layer's stream-K scratch for the current stream (before graph capture)."""
    _prepare("wino_conv1x1_prepare", M, Cin, Kout)


def conv1x1_bn_ex(A, B, bn_bias, bn_scale, flags: int, residual=None, out=None, hw=None) -> torch.Tensor:
    """Chaining form of the 1x1 layer: A and/or C may be the padded [N][H+2][W+2][.] tensors of the
    3x3 layer (flags A_PADDED / C_PADDED), a residual [M][Kout] may be added before the ReLU.
    The feature-map size comes from the padded A, else from a 4-D unpadded A [N][H][W][Cin], else
    from `hw`, else it is the reference's 14 x 14 (wino_conv1x1_bn_ex); anything but 14 x 14 goes
    through wino_conv1x1_bn_ex_hw.
    With RESIDUAL_UP2 (beside ADD_RESIDUAL) the residual is the padded coarser map [N][Hc+2][Wc+2][Kout],
    Hc = (H+1)//2, Wc = (W+1)//2, and output pixel (y, x) adds its pixel (y >> 1, x >> 1): the sum with
    F.interpolate(residual, size=(H, W), mode="nearest") without the upsampled tensor (an FPN's top-down step)."""
    a, bm = _dev(A, "A"), _dev(B, "B")
    b, s = _dev(bn_bias, "bn_bias"), _dev(bn_scale, "bn_scale")
    Cin, Kout = int(bm.shape[0]), int(bm.shape[1])
    H = W = None
    if flags & A_PADDED:
        if a.dim() != 4 or int(a.shape[3]) != Cin or a.shape[1] < 3 or a.shape[2] < 3:
            raise WinoError("A_PADDED: A must be [N][H+2][W+2][Cin]")
        H, W = int(a.shape[1]) - 2, int(a.shape[2]) - 2
        N = int(a.shape[0])
        M = N * H * W
    else:
        if a.dim() == 4:
            H, W = int(a.shape[1]), int(a.shape[2])
        a = a.reshape(-1, Cin)
        M = int(a.shape[0])
    if hw is not None:
        if H is not None and (H, W) != tuple(hw):
            raise WinoError(f"hw={tuple(hw)} contradicts A's {H}x{W}")
        H, W = int(hw[0]), int(hw[1])
    if H is None:
        H = W = 14
    padded = bool(flags & (A_PADDED | C_PADDED))
    if padded and M % (H * W):
        raise WinoError(f"padded layouts need M = N*{H}*{W}, got M={M}")
    r = _dev(residual, "residual") if residual is not None else None
    up2 = bool(flags & RESIDUAL_UP2)
    if up2:
        if not flags & ADD_RESIDUAL or r is None:
            raise WinoError("RESIDUAL_UP2 needs ADD_RESIDUAL and a residual")
        if M % (H * W):
            raise WinoError(f"RESIDUAL_UP2 needs M = N*{H}*{W}, got M={M}")
        Hc, Wc = _up_hw(H, W)
        if tuple(r.shape) != (M // (H * W), Hc + 2, Wc + 2, Kout):
            raise WinoError(f"RESIDUAL_UP2: residual must be the padded coarser map "
                            f"{(M // (H * W), Hc + 2, Wc + 2, Kout)}, got {tuple(r.shape)}")
    elif r is not None and r.numel() != M * Kout:
        raise WinoError(f"residual must hold M*Kout = {M * Kout} values, got {r.numel()}")
    shape = (M // (H * W), H + 2, W + 2, Kout) if flags & C_PADDED else (M, Kout)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=a.device)
    elif out.numel() != M * Kout or flags & C_PADDED:
        _out(out, shape, "out")
    else:
        _out(out, None, "out")   # unpadded: any contiguous view of M*Kout values ([M][Kout] or [N][H][W][Kout])
    _on_current_device(a, bm, b, s, r, out)
    args = (a.data_ptr(), bm.data_ptr(), b.data_ptr(), s.data_ptr(), r.data_ptr() if r is not None else None,
            out.data_ptr())
    if up2 or (padded and (H, W) != (14, 14)):
        _check(lib().wino_conv1x1_bn_ex_hw(*args, M // (H * W), H, W, Cin, Kout, int(flags), _stream()),
               "wino_conv1x1_bn_ex_hw")
    else:
        _check(lib().wino_conv1x1_bn_ex(*args, M, Cin, Kout, int(flags), _stream()), "wino_conv1x1_bn_ex")
    return out


def _bottleneck(entry, x, w1, bn1, mid, w2, bn2, last, bn3, out, workspace, stride=1, groups=None, dilation=None):
    """The one body of the seven bottleneck wrappers: operands checked against each other, workspace and output made or
    checked, then `entry(x, w1, bn1, w2, bn2, last[, bn3], out, N, Hin, Win, Cin, Cm[, C4][, groups][, stride],
    workspace, stream)`.  `mid` names what w2 is packed for: "U2" (filter_transform_f2: Winograd, a stride sits on the
    first 1x1), "w2_taps" (filter_pack_s2: the 3x3 as an implicit GEMM -- at stride 2, or, with `dilation`, at stride 1
    with that dilation; neither entry point takes a stride argument) or "wg" (filter_pack_grouped: `stride` on the
    3x3).  `dilation` is passed last among the dimensions.  `last` is w3 with its bn3 (identity shortcut: C4 = Cin) or, bn3
    None, the packed tail of a projection block."""
    identity = bn3 is not None
    x = _dev(x, "x")
    if x.dim() != 4:
        raise WinoError("x must be [N][H][W][C4]" if identity else "x must be [N][Hin][Win][Cin]")
    N, Hin, Win, Cin = (int(v) for v in x.shape)
    w1, w2, last = _dev(w1, "w1"), _dev(w2, mid), _dev(last, "w3" if identity else "tail")
    Cm = int(w1.shape[1]) if w1.dim() == 2 else 0
    if identity:
        C4 = Cin
        if w1.dim() != 2 or int(w1.shape[0]) != C4 or last.dim() != 2 or tuple(last.shape) != (Cm, C4):
            raise WinoError("w1 must be [C4][Cm], w3 [Cm][C4]")
    elif w1.dim() != 2 or int(w1.shape[0]) != Cin:
        raise WinoError("w1 must be [Cin][Cm]")
    if mid == "U2":
        if w2.numel() != 16 * Cm * Cm:
            raise WinoError(f"U2 must be a {Cm} -> {Cm} filter from filter_transform_f2 (16*Cm*Cm values)")
    elif mid == "w2_taps":
        if w2.dim() != 4 or tuple(w2.shape) != (3, 3, Cm, Cm):
            raise WinoError(f"w2_taps must be [3][3][{Cm}][{Cm}]: pack it with filter_pack_s2")
    else:
        groups = _groups_of(w2, Cm, groups, "wg")
    if not identity:
        if last.numel() % (Cm + Cin + 2):
            raise WinoError("tail does not match Cm / Cin: pack it with proj_tail_pack")
        C4 = last.numel() // (Cm + Cin + 2)
        if int(stride) not in (1, 2):
            raise WinoError(f"stride must be 1 or 2, got {stride}")
    H, W = _out_hw(Hin, Win, int(stride))
    vecs = _bn_vecs(bn1, bn2, bn3) if identity else _bn_vecs(bn1, bn2)
    if any(v.numel() != c for v, c in zip(vecs, (Cm, Cm, Cm, Cm, C4, C4))):
        raise WinoError("bn1 / bn2 vectors must have Cm values" + (", bn3's C4" if identity else ""))
    if identity:
        need = lib().wino_residual_block_workspace_bytes_hw(N, H, W, Cm)
    elif mid == "U2" or int(stride) == 1:   # t1 and t2 both on the output grid
        need = lib().wino_proj_block_workspace_bytes_hw(N, H, W, Cm)
    else:
        need = lib().wino_proj_block_v15_workspace_bytes_hw(N, Hin, Win, Cm)
    workspace = _workspace(workspace, need, x.device)
    out = _output(out, (N, H, W, C4), x.device)
    _on_current_device(x, w1, w2, last, out, workspace, *vecs)
    dims = (N, Hin, Win, Cin, Cm) if identity else (N, Hin, Win, Cin, Cm, C4)
    if mid == "wg":
        dims += (groups,)
    if not identity and mid != "w2_taps":   # (the v1.5 and the dilated projection blocks take no stride argument)
        dims += (int(stride),)
    if dilation is not None:
        dims += (int(dilation),)
    if entry == "wino_residual_block_hw" and (H, W) == (14, 14):   # the reference's stage has an entry point of its own
        entry, dims = "wino_residual_block", (N, C4, Cm)
    _check(getattr(lib(), entry)(x.data_ptr(), w1.data_ptr(), vecs[0].data_ptr(), vecs[1].data_ptr(), w2.data_ptr(),
                                 vecs[2].data_ptr(), vecs[3].data_ptr(), last.data_ptr(),
                                 *(v.data_ptr() for v in vecs[4:]), out.data_ptr(), *dims, *_ws_args(workspace),
                                 _stream()), entry)
    return out


def residual_block(x, w1, bn1, U2, bn2, w3, bn3, out=None, workspace=None) -> torch.Tensor:
    """ResNet bottleneck: x [N][H][W][C4] -> same shape (the reference's stage is 14 x 14:
    wino_residual_block; other sizes: wino_residual_block_hw).  bnX = (bias, scale) folded BN
    vectors; w1 [C4][Cm], w3 [Cm][C4]; U2 from filter_transform_f2 (Cm -> Cm)."""
    return _bottleneck("wino_residual_block_hw", x, w1, bn1, "U2", U2, bn2, w3, bn3, out, workspace)


FORM_TILED, FORM_STREAM_K, FORM_LATENCY = 0, 1, 2   # WINO_1X1_FORM_*


def proj_tail_pack(w3, bn3, wp, bnp, out=None) -> torch.Tensor:
    """The projection block's fused last layer: w3 [Cm][C4], wp [Cin][C4] and their folded BNs (bias, scale) packed
    into one opaque buffer (wino_proj_tail_pack) -- the analogue of filter_transform_f2 for U2."""
    w3, wp = _dev(w3, "w3"), _dev(wp, "wp")
    vecs = _bn_vecs(bn3, bnp)
    Cm, C4, Cin = int(w3.shape[0]), int(w3.shape[1]), int(wp.shape[0])
    if w3.dim() != 2 or wp.dim() != 2 or int(wp.shape[1]) != C4 or any(v.numel() != C4 for v in vecs):
        raise WinoError("w3 must be [Cm][C4], wp [Cin][C4], the BN vectors [C4]")
    n = lib().wino_proj_tail_elems(Cm, Cin, C4)
    if n == 0:
        raise WinoError(f"bad projection tail shape Cm={Cm} Cin={Cin} C4={C4}")
    packed = _output(out, (n,), w3.device)
    _on_current_device(w3, wp, packed, *vecs)
    _check(lib().wino_proj_tail_pack(w3.data_ptr(), vecs[0].data_ptr(), vecs[1].data_ptr(), wp.data_ptr(),
                                     vecs[2].data_ptr(), vecs[3].data_ptr(), packed.data_ptr(), Cm, Cin, C4, _stream()),
           "wino_proj_tail_pack")
    return packed


def proj_block_prepare(N: int, Hin: int, Win: int, Cin: int, Cm: int, C4: int, stride: int) -> None:
    """Allocate the scratch of proj_block's three launches for the current stream (before graph capture)."""
    _prepare("wino_proj_block_prepare_hw", N, Hin, Win, Cin, Cm, C4, stride)


def proj_tail_plan(N: int, Hin: int, Win: int, Cin: int, Cm: int, C4: int, stride: int, cus: int = 256):
    """(first, tail): the FORM_* each of the projection block's two 1x1 launches takes (host-side)."""
    return _plan_query("wino_proj_tail_plan", 2, N, Hin, Win, Cin, Cm, C4, stride, cus)


def proj_block(x, w1, bn1, U2, bn2, tail, stride: int, out=None, workspace=None) -> torch.Tensor:
    """ResNet projection bottleneck (a stage's first block, v1 placement): x [N][Hin][Win][Cin] ->
    [N][H][W][C4], H = (Hin-1)//stride + 1.  bnX = (bias, scale) folded BN vectors; w1 [Cin][Cm]; U2 from
    filter_transform_f2 (Cm -> Cm); tail from proj_tail_pack (w3, bn3, wp, bnp)."""
    return _bottleneck("wino_proj_block_hw", x, w1, bn1, "U2", U2, bn2, tail, None, out, workspace, stride)


def filter_pack_s2(w_kcrs: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """[K][C][3][3] taps -> the stride-2 3x3 layer's [3][3][C][K] filter (w.permute(2, 3, 1, 0)), the analogue of
    filter_transform_f2 for conv3x3_s2_bn_relu."""
    w = _dev(w_kcrs, "w_kcrs")
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise WinoError("w_kcrs must be [K][C][3][3]")
    taps = w.permute(2, 3, 1, 0)
    if out is None:
        return taps.contiguous()
    return _out(out, taps.shape, "out").copy_(taps)


def conv3x3_s2_bn_relu(inp: torch.Tensor, w_taps: torch.Tensor, bn_bias: torch.Tensor, bn_scale: torch.Tensor,
                       relu: bool = True, out: torch.Tensor | None = None) -> torch.Tensor:
    """Stride-2, pad-1 3x3 conv + folded BN (+ReLU): inp [N][Hin+2][Win+2][C] (zero ring) -> out [N][H+2][W+2][K]
    (interior H x W = (Hin-1)//2 + 1 x (Win-1)//2 + 1, zero ring).  w_taps [3][3][C][K] from filter_pack_s2.  One launch."""
    x, w = _dev(inp, "inp"), _dev(w_taps, "w_taps")
    b, s = _dev(bn_bias, "bn_bias"), _dev(bn_scale, "bn_scale")
    if x.dim() != 4 or x.shape[1] < 3 or x.shape[2] < 3:
        raise WinoError("inp must be [N][Hin+2][Win+2][C]")
    N, Hin, Win, C = int(x.shape[0]), int(x.shape[1]) - 2, int(x.shape[2]) - 2, int(x.shape[3])
    if w.dim() != 4 or tuple(w.shape[:3]) != (3, 3, C):
        raise WinoError(f"w_taps must be [3][3][{C}][K]: pack it with filter_pack_s2")
    K = int(w.shape[3])
    if b.numel() != K or s.numel() != K:
        raise WinoError("bn vectors do not match K")
    H, W = _out_hw(Hin, Win, 2)
    out = _output(out, (N, H + 2, W + 2, K), x.device)
    _on_current_device(x, w, b, s, out)
    _check(lib().wino_conv3x3_s2_bn_relu_hw(x.data_ptr(), w.data_ptr(), b.data_ptr(), s.data_ptr(), out.data_ptr(),
                                            N, Hin, Win, C, K, int(relu), _stream()), "wino_conv3x3_s2_bn_relu_hw")
    return out


def conv3x3_s2_prepare(N: int, Hin: int, Win: int, C: int, K: int) -> None:
    """Allocate the stride-2 3x3 layer's stream-K scratch for the current stream (before graph capture)."""
    _prepare("wino_conv3x3_s2_prepare_hw", N, Hin, Win, C, K)


def conv3x3_s2_plan(N: int, Hin: int, Win: int, C: int, K: int, cus: int = 256) -> int:
    """The FORM_* the stride-2 3x3 layer takes on a device with `cus` CUs (host-side)."""
    return _plan_query("wino_conv3x3_s2_plan", 1, int(N), int(Hin), int(Win), int(C), int(K), int(cus))[0]


def proj_block_v15_prepare(N: int, Hin: int, Win: int, Cin: int, Cm: int, C4: int) -> None:
    """Allocate the scratch of proj_block_v15's three launches for the current stream (before graph capture)."""
    _prepare("wino_proj_block_v15_prepare_hw", N, Hin, Win, Cin, Cm, C4)


def proj_block_v15(x, w1, bn1, w2_taps, bn2, tail, out=None, workspace=None) -> torch.Tensor:
    """ResNet projection bottleneck, v1.5 placement (torchvision's: the stride 2 on the 3x3): x [N][Hin][Win][Cin] ->
    [N][H][W][C4], H = (Hin-1)//2 + 1.  bnX = (bias, scale) folded BN vectors; w1 [Cin][Cm]; w2_taps [3][3][Cm][Cm]
    from filter_pack_s2; tail from proj_tail_pack (w3, bn3, wp, bnp)."""
    return _bottleneck("wino_proj_block_v15_hw", x, w1, bn1, "w2_taps", w2_taps, bn2, tail, None, out, workspace, 2)


def conv3x3_dilated_bn_relu(inp: torch.Tensor, w_taps: torch.Tensor, bn_bias: torch.Tensor, bn_scale: torch.Tensor,
                            dilation: int, relu: bool = True, out: torch.Tensor | None = None) -> torch.Tensor:
    """Stride-1 3x3 conv with dilation = padding = `dilation` + folded BN (+ReLU): inp [N][H+2][W+2][C] with a zero ring
    of width one (whatever the dilation) -> out [N][H+2][W+2][K], zero ring.  w_taps [3][3][C][K] from filter_pack_s2.
    One launch of the tiled 1x1 GEMM kernel in its dilated-tap operand form."""
    x, w = _dev(inp, "inp"), _dev(w_taps, "w_taps")
    b, s = _dev(bn_bias, "bn_bias"), _dev(bn_scale, "bn_scale")
    if x.dim() != 4 or x.shape[1] < 3 or x.shape[2] < 3:
        raise WinoError("inp must be [N][H+2][W+2][C]")
    N, H, W, C = int(x.shape[0]), int(x.shape[1]) - 2, int(x.shape[2]) - 2, int(x.shape[3])
    if w.dim() != 4 or tuple(w.shape[:3]) != (3, 3, C):
        raise WinoError(f"w_taps must be [3][3][{C}][K]: pack it with filter_pack_s2")
    K = int(w.shape[3])
    if b.numel() != K or s.numel() != K:
        raise WinoError("bn vectors do not match K")
    out = _output(out, (N, H + 2, W + 2, K), x.device)
    _on_current_device(x, w, b, s, out)
    _check(lib().wino_conv3x3_dilated_bn_relu_hw(x.data_ptr(), w.data_ptr(), b.data_ptr(), s.data_ptr(),
                                                 out.data_ptr(), N, H, W, C, K, int(dilation), int(relu), _stream()),
           "wino_conv3x3_dilated_bn_relu_hw")
    return out


def conv3x3_dilated_prepare(N: int, H: int, W: int, C: int, K: int, dilation: int) -> None:
    """Allocate the dilated 3x3 layer's stream-K scratch for the current stream (before graph capture)."""
    _prepare("wino_conv3x3_dilated_prepare_hw", N, H, W, C, K, dilation)


def conv3x3_dilated_plan(N: int, H: int, W: int, C: int, K: int, dilation: int, cus: int = 256) -> int:
    """The FORM_* the dilated 3x3 layer takes on a device with `cus` CUs (host-side): FORM_TILED or FORM_STREAM_K."""
    return _plan_query("wino_conv3x3_dilated_plan", 1, int(N), int(H), int(W), int(C), int(K), int(dilation),
                       int(cus))[0]


def dilated_residual_block_prepare(N: int, H: int, W: int, C4: int, Cm: int, dilation: int) -> None:
    """Allocate the scratch of dilated_residual_block's three launches for the current stream (before graph capture)."""
    _prepare("wino_dilated_residual_block_prepare_hw", N, H, W, C4, Cm, dilation)


def dilated_residual_block(x, w1, bn1, w2_taps, bn2, w3, bn3, dilation: int, out=None, workspace=None) -> torch.Tensor:
    """Identity bottleneck of a dilated stage: residual_block with the dilated 3x3 in the middle.  x [N][H][W][C4] ->
    same shape; w1 [C4][Cm], w3 [Cm][C4]; w2_taps [3][3][Cm][Cm] from filter_pack_s2; bnX = (bias, scale)."""
    return _bottleneck("wino_dilated_residual_block_hw", x, w1, bn1, "w2_taps", w2_taps, bn2, w3, bn3, out, workspace,
                       dilation=dilation)


def dilated_proj_block_prepare(N: int, H: int, W: int, Cin: int, Cm: int, C4: int, dilation: int) -> None:
    """Allocate the scratch of dilated_proj_block's three launches for the current stream (before graph capture)."""
    _prepare("wino_dilated_proj_block_prepare_hw", N, H, W, Cin, Cm, C4, dilation)


def dilated_proj_block(x, w1, bn1, w2_taps, bn2, tail, dilation: int, out=None, workspace=None) -> torch.Tensor:
    """Projection bottleneck of a dilated stage (stride 1, the dilated 3x3 in the middle): x [N][H][W][Cin] ->
    [N][H][W][C4].  w1 [Cin][Cm]; w2_taps [3][3][Cm][Cm] from filter_pack_s2; tail from proj_tail_pack (stride 1)."""
    return _bottleneck("wino_dilated_proj_block_hw", x, w1, bn1, "w2_taps", w2_taps, bn2, tail, None, out, workspace, 1,
                       dilation=dilation)


def _cat_sources(srcs):
    """The concat layer's sources: one [S][N][h][w][Cs] tensor, or S tensors [N][h][w][Cs] of one shape at equally spaced,
    ascending addresses of one allocation (views of a buffer: what lies between them is never read).  Returns (first,
    spacing in floats, S, (N, h, w, Cs), the tensors kept alive)."""
    if isinstance(srcs, torch.Tensor):
        t = _dev(srcs, "srcs")
        if t.dim() != 5:
            raise WinoError("srcs must be [S][N][H][W][Cs] or a sequence of [N][H][W][Cs] tensors")
        S = int(t.shape[0])
        return t, t.numel() // max(S, 1), S, tuple(int(v) for v in t.shape[1:]), (t,)
    views = [_out(v, None, "srcs[i]") for v in srcs]
    if len(views) < 2 or any(v.dim() != 4 or v.shape != views[0].shape for v in views):
        raise WinoError("srcs must be at least two [N][H][W][Cs] tensors of one shape")
    step = views[1].data_ptr() - views[0].data_ptr()
    if step <= 0 or step % 4 or any(b.data_ptr() - a.data_ptr() != step for a, b in zip(views, views[1:])):
        raise WinoError("srcs must lie at equally spaced, ascending addresses")
    return views[0], step // 4, len(views), tuple(int(v) for v in views[0].shape), tuple(views)


def conv1x1_cat_bn(srcs, w: torch.Tensor, bias_per_image: torch.Tensor, bn_scale: torch.Tensor, flags: int = 0,
                   out: torch.Tensor | None = None) -> torch.Tensor:
    """The 1x1 layer behind a channel concatenation that is never made: out = act(bn_scale * (cat(srcs, channels) . w) +
    bias_per_image[n]).  srcs: see _cat_sources ([N][H+2][W+2][Cs] each with A_PADDED); w [S*Cs][Kout]; bias_per_image
    [N][Kout], one bias row per image; flags: RELU | A_PADDED | C_PADDED.  Returns [N][H][W][Kout], or the padded
    [N][H+2][W+2][Kout] with a zero ring (C_PADDED).  One launch of the tiled 1x1 GEMM kernel in its concat operand form."""
    first, stride, S, (N, h, wd, Cs), keep = _cat_sources(srcs)
    p = 2 if flags & A_PADDED else 0
    if h <= p or wd <= p:
        raise WinoError("A_PADDED: the sources must be [N][H+2][W+2][Cs]")
    H, W = h - p, wd - p
    bm, b, sc = _dev(w, "w"), _dev(bias_per_image, "bias_per_image"), _dev(bn_scale, "bn_scale")
    if bm.dim() != 2 or int(bm.shape[0]) != S * Cs:
        raise WinoError(f"w must be [S*Cs][Kout] = [{S * Cs}][Kout]")
    Kout = int(bm.shape[1])
    if tuple(b.shape) != (N, Kout) or sc.numel() != Kout:
        raise WinoError(f"bias_per_image must be [{N}][{Kout}], bn_scale [{Kout}]")
    out = _output(out, (N, H + 2, W + 2, Kout) if flags & C_PADDED else (N, H, W, Kout), first.device)
    _on_current_device(*keep, bm, b, sc, out)
    _check(lib().wino_conv1x1_cat_bn_hw(first.data_ptr(), stride, bm.data_ptr(), b.data_ptr(), sc.data_ptr(),
                                        out.data_ptr(), N, H, W, S, Cs, Kout, int(flags), _stream()),
           "wino_conv1x1_cat_bn_hw")
    return out


def conv1x1_cat_prepare(N: int, H: int, W: int, sources: int, Cs: int, Kout: int) -> None:
    """Allocate the concat layer's stream-K scratch for the current stream (before graph capture)."""
    _prepare("wino_conv1x1_cat_prepare_hw", N, H, W, sources, Cs, Kout)


def conv1x1_cat_plan(N: int, H: int, W: int, sources: int, Cs: int, Kout: int, cus: int = 256) -> int:
    """The FORM_* the concat layer takes on a device with `cus` CUs (host-side): FORM_TILED or FORM_STREAM_K."""
    return _plan_query("wino_conv1x1_cat_plan", 1, int(N), int(H), int(W), int(sources), int(Cs), int(Kout), int(cus))[0]


def aspp_workspace_bytes(N: int, H: int, W: int, Cin: int, Cb: int, Kout: int) -> int:
    """Bytes of aspp's workspace, the formula of winograd_mi355x.h (wino_aspp_hw refuses less): the pooled vector
    [N][Cin], its branch [N][Cb] and the per-image bias [N][Kout], each rounded up to 256 bytes, and the four spatial
    branches' unpadded [N][H][W][Cb] slots."""
    N, H, W, Cin, Cb, Kout = int(N), int(H), int(W), int(Cin), int(Cb), int(Kout)
    if min(N, H, W, Cin, Cb, Kout) < 1:
        return 0
    r256 = lambda b: (b + 255) // 256 * 256
    return r256(4 * N * Cin) + r256(4 * N * Cb) + r256(4 * N * Kout) + 4 * (4 * N * H * W * Cb)


def aspp_prepare(N: int, H: int, W: int, Cin: int, Cb: int, Kout: int, rates) -> None:
    """Allocate the scratch of aspp's eight launches for the current stream (before graph capture)."""
    d1, d2, d3 = (int(r) for r in rates)
    _prepare("wino_aspp_prepare_hw", N, H, W, Cin, Cb, Kout, d1, d2, d3)


def aspp(inp, w0, bn0, w_taps, bn_taps, rates, w_pool, bn_pool, w_proj, bn_proj, out=None, workspace=None) -> torch.Tensor:
    """Atrous spatial pyramid pooling (torchvision's DeepLabV3 ASPP, dropout aside): inp [N][H+2][W+2][Cin] with a zero
    ring -> relu(bn(cat(five branches) . w_proj)) as the padded [N][H+2][W+2][Kout].  w0, w_pool [Cin][Cb]; w_taps: three
    [3][3][Cin][Cb] from filter_pack_s2 with their `rates`; w_proj [5*Cb][Kout], the pooled branch's rows last; bnX =
    (bias, scale), bn_taps three such pairs.  The concatenated tensor and the broadcast pooled branch never exist: see
    conv1x1_cat_bn."""
    x = _dev(inp, "inp")
    if x.dim() != 4 or x.shape[1] < 3 or x.shape[2] < 3:
        raise WinoError("inp must be [N][H+2][W+2][Cin]")
    N, H, W, Cin = int(x.shape[0]), int(x.shape[1]) - 2, int(x.shape[2]) - 2, int(x.shape[3])
    w0, w_pool, w_proj = _dev(w0, "w0"), _dev(w_pool, "w_pool"), _dev(w_proj, "w_proj")
    if w0.dim() != 2 or int(w0.shape[0]) != Cin or w_pool.shape != w0.shape:
        raise WinoError("w0 and w_pool must be [Cin][Cb]")
    Cb = int(w0.shape[1])
    taps = [_dev(t, "w_taps[i]") for t in w_taps]
    if len(taps) != 3 or len(bn_taps) != 3 or len(rates) != 3:
        raise WinoError("aspp takes three dilated branches: three w_taps, bn_taps and rates")
    if any(tuple(t.shape) != (3, 3, Cin, Cb) for t in taps):
        raise WinoError(f"every w_taps must be [3][3][{Cin}][{Cb}]: pack it with filter_pack_s2")
    if w_proj.dim() != 2 or int(w_proj.shape[0]) != 5 * Cb:
        raise WinoError(f"w_proj must be [5*Cb][Kout] = [{5 * Cb}][Kout]")
    Kout = int(w_proj.shape[1])
    vecs = _bn_vecs(bn0, *bn_taps, bn_pool, bn_proj)
    if any(v.numel() != c for v, c in zip(vecs, [Cb] * 10 + [Kout] * 2)):
        raise WinoError("the branches' bn vectors must have Cb values, bn_proj's Kout")
    workspace = _workspace(workspace, aspp_workspace_bytes(N, H, W, Cin, Cb, Kout), x.device)
    out = _output(out, (N, H + 2, W + 2, Kout), x.device)
    _on_current_device(x, w0, w_pool, w_proj, out, workspace, *taps, *vecs)
    v = [t.data_ptr() for t in vecs]
    _check(lib().wino_aspp_hw(x.data_ptr(), w0.data_ptr(), v[0], v[1], taps[0].data_ptr(), v[2], v[3], taps[1].data_ptr(),
                              v[4], v[5], taps[2].data_ptr(), v[6], v[7], w_pool.data_ptr(), v[8], v[9],
                              w_proj.data_ptr(), v[10], v[11], out.data_ptr(), N, H, W, Cin, Cb, Kout,
                              *(int(r) for r in rates), *_ws_args(workspace), _stream()), "wino_aspp_hw")
    return out


RESIZE_FORM_STAGED, RESIZE_FORM_DIRECT = 1, 2   # WINO_RESIZE_FORM_*


def resize_bilinear_plan(h: int, w: int, C: int, ld: int, Ho: int, Wo: int, want_out: bool = True,
                         want_labels: bool = False) -> int:
    """The RESIZE_FORM_* resize_bilinear takes for this shape (host-side, a function of the shape alone)."""
    return _plan_query("wino_resize_bilinear_plan", 1, int(h), int(w), int(C), int(ld), int(Ho), int(Wo),
                       int(bool(want_out)), int(bool(want_labels)))[0]


def resize_bilinear(src, Ho: int, Wo: int, C=None, in_padded: bool = False, out=None, labels=None,
                    want_out: bool = True, want_labels: bool = False):
    """torch's F.interpolate(mode="bilinear", align_corners=False) of class scores, and / or their argmax over the
    classes, in one HIP launch with exact integer source coordinates.  src [N][h][w][ld] or, in_padded, [N][h+2][w+2][ld]
    (the ring is not read); the first C of the ld columns are the classes (default: all).  Returns (out, labels): out
    [N][C][Ho][Wo] float32 (NCHW) or None, labels [N][Ho][Wo] int32 or None.  A given `out` / `labels` tensor is written
    and implies want_out / want_labels."""
    x = _dev(src, "src")
    if x.dim() != 4:
        raise WinoError("src must be [N][h][w][ld]")
    p = 2 if in_padded else 0
    N, h, w, ld = int(x.shape[0]), int(x.shape[1]) - p, int(x.shape[2]) - p, int(x.shape[3])
    if h < 1 or w < 1:
        raise WinoError("src has no interior")
    C = ld if C is None else int(C)
    Ho, Wo = int(Ho), int(Wo)
    want_out, want_labels = bool(want_out) or out is not None, bool(want_labels) or labels is not None
    if not want_out and not want_labels:
        raise WinoError("resize_bilinear: neither out nor labels is wanted")
    if min(N, Ho, Wo, C) < 1:
        raise WinoError(f"resize_bilinear: bad shape N={N} C={C} Ho={Ho} Wo={Wo}")
    if want_out:
        out = _output(out, (N, C, Ho, Wo), x.device)
    if want_labels:
        if labels is None:
            labels = torch.empty((N, Ho, Wo), dtype=torch.int32, device=x.device)
        elif (not isinstance(labels, torch.Tensor) or not labels.is_cuda or labels.dtype != torch.int32
              or not labels.is_contiguous() or tuple(labels.shape) != (N, Ho, Wo)):
            raise WinoError(f"labels must be a contiguous int32 CUDA(HIP) tensor of shape {(N, Ho, Wo)}")
    _on_current_device(x, out, labels)
    _check(lib().wino_resize_bilinear_hw(x.data_ptr(), out.data_ptr() if want_out else None,
                                         labels.data_ptr() if want_labels else None, N, h, w, C, ld,
                                         int(bool(in_padded)), Ho, Wo, _stream()), "wino_resize_bilinear_hw")
    return (out if want_out else None), (labels if want_labels else None)


IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)   # torchvision's detectors' defaults
TRANSFORM_MAX_IMAGES = 32                                                     # WINO_TRANSFORM_MAX_IMAGES
IMAGE_DTYPES = {torch.float32: 0, torch.uint8: 1}                             # WINO_IMAGE_F32, WINO_IMAGE_U8


def transform_size(h: int, w: int, min_size: int = 800, max_size: int = 1333):
    """(ho, wo): the size torchvision's GeneralizedRCNNTransform resizes an h x w image to (host-side, torch's fp32
    scale factor and floor bit for bit)."""
    return _plan_query("wino_transform_size", 2, int(h), int(w), int(min_size), int(max_size))


def batch_hw(sizes, size_divisible: int = 32):
    """(Hb, Wb) of the batch that holds images of `sizes` [(h, w)]: the per-axis maximum, rounded up to a multiple of
    size_divisible (torchvision's batch_images)."""
    sizes, d = [(int(h), int(w)) for h, w in sizes], int(size_divisible)
    if not sizes or d < 1:
        raise WinoError(f"batch_hw: {len(sizes)} sizes, size_divisible={d} (need at least one size and size_divisible >= 1)")
    return tuple((max(s[k] for s in sizes) + d - 1) // d * d for k in (0, 1))


def image_transform(images, out_sizes, Hb: int, Wb: int, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None) -> torch.Tensor:
    """torchvision's GeneralizedRCNNTransform at test time in one HIP launch per 32 images: every image [C][h][w] of the
    list (all float32 in [0, 1], or all uint8, taken as byte / 255) is normalised with mean / std [C], resized to its
    (ho, wo) of `out_sizes` (bilinear, align_corners=False, exact integer source coordinates) and written into the top-left
    corner of its planes of out [N][C][Hb][Wb] float32; the rest of every plane is written 0.  No scratch: capturable
    into a graph without a prepare."""
    images = list(images)
    if not images:
        raise WinoError("image_transform: no images")
    for k, t in enumerate(images):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise WinoError(f"images[{k}] must be a CUDA(HIP) tensor -- this framework has no CPU path")
        if t.dtype not in IMAGE_DTYPES or t.dtype != images[0].dtype:
            raise WinoError(f"images[{k}] is {t.dtype}: the images must be all float32 or all uint8")
        if t.dim() != 3 or t.shape[0] != images[0].shape[0] or min(t.shape) < 1:
            raise WinoError(f"images[{k}] must be [C][h][w] with the C of images[0], got {tuple(t.shape)}")
    imgs = [t.contiguous() for t in images]
    N, C = len(imgs), int(imgs[0].shape[0])
    out_sizes = [(int(h), int(w)) for h, w in out_sizes]
    mean, std = [float(v) for v in mean], [float(v) for v in std]
    if len(out_sizes) != N or len(mean) != C or len(std) != C:
        raise WinoError(f"image_transform: {N} images of {C} channels, {len(out_sizes)} out_sizes, {len(mean)} means, "
                        f"{len(std)} stds")
    Hb, Wb = int(Hb), int(Wb)
    if Hb < 1 or Wb < 1:
        raise WinoError(f"image_transform: bad batch Hb={Hb} Wb={Wb}")
    out = _output(out, (N, C, Hb, Wb), imgs[0].device)
    _on_current_device(*imgs, out)
    ptrs = (c_void_p * N)(*[t.data_ptr() for t in imgs])
    hw = (c_int * (2 * N))(*[int(t.shape[d]) for t in imgs for d in (1, 2)])
    ohw = (c_int * (2 * N))(*[v for s in out_sizes for v in s])
    _check(lib().wino_image_transform_hw(ptrs, hw, ohw, N, C, IMAGE_DTYPES[imgs[0].dtype], (ctypes.c_float * C)(*mean),
                                         (ctypes.c_float * C)(*std), out.data_ptr(), Hb, Wb, _stream()),
           "wino_image_transform_hw")
    return out


def roi_align(levels, rois, P: int, scales, sampling: int = 2, in_padded: bool = False, out_padded: bool = False,
              canonical_scale: float = 224.0, canonical_level: int = 4, out=None) -> torch.Tensor:
    """torchvision's roi_align(aligned=False) over 1 to 4 pyramid levels with MultiScaleRoIAlign's level assignment, one
    HIP launch for all boxes.  levels: a tensor or a list of 1..4 tensors, finest first, each [N][h][w][C] or, in_padded,
    [N][h+2][w+2][C] (the ring is not read); rois [R][5] = (batch index, x1, y1, x2, y2) in image pixels; scales: one
    spatial_scale per level (several levels: 2^-(k0+l)).  Returns [R][P][P][C], or out_padded [R][P+2][P+2][C] with a zero
    ring (the Winograd layer's input at N = R).  No scratch: capturable into a graph without a prepare."""
    maps = [levels] if isinstance(levels, torch.Tensor) else list(levels)
    if not 1 <= len(maps) <= 4:
        raise WinoError(f"roi_align takes 1 to 4 level maps, got {len(maps)}")
    maps = [_dev(m, f"levels[{i}]") for i, m in enumerate(maps)]
    p = 2 if in_padded else 0
    if any(m.dim() != 4 or m.shape[1] <= p or m.shape[2] <= p for m in maps):
        raise WinoError("every level map must be [N][h][w][C]" + (" with a ring (in_padded)" if in_padded else ""))
    N, C = int(maps[0].shape[0]), int(maps[0].shape[3])
    if any(int(m.shape[0]) != N or int(m.shape[3]) != C for m in maps):
        raise WinoError("the level maps must agree in N and C")
    scales = [float(scales)] if isinstance(scales, (int, float)) else [float(v) for v in scales]
    if len(scales) != len(maps):
        raise WinoError(f"{len(maps)} level maps but {len(scales)} scales")
    r = _dev(rois, "rois")
    if r.dim() != 2 or int(r.shape[1]) != 5:
        raise WinoError("rois must be [R][5]: (batch index, x1, y1, x2, y2)")
    R, P, q = int(r.shape[0]), int(P), 2 if out_padded else 0
    if P < 1:
        raise WinoError(f"roi_align: bad P={P}")
    out = _output(out, (R, P + q, P + q, C), r.device)
    _on_current_device(*maps, r, out)
    hw = (c_int * (2 * len(maps)))(*[int(m.shape[d]) - p for m in maps for d in (1, 2)])
    sc = (ctypes.c_float * len(maps))(*scales)
    ptrs = [m.data_ptr() for m in maps] + [None] * (4 - len(maps))
    _check(lib().wino_roi_align_hw(*ptrs, hw, sc, len(maps), N, C, int(bool(in_padded)), r.data_ptr() or None, R, P,
                                   int(sampling), float(canonical_scale), int(canonical_level), out.data_ptr() or None,
                                   int(bool(out_padded)), _stream()), "wino_roi_align_hw")
    return out


def roi_align_launches(R: int, P: int, out_padded: bool = False) -> int:
    """How many kernel launches roi_align splits R boxes into (host-side): one until R (P + 2 out_padded)^2 passes 2^31, or
    the developer knob WINO_ROI_LAUNCH_TASKS."""
    n = c_long(0)
    _check(lib().wino_roi_align_launches(int(R), int(P), int(bool(out_padded)), ctypes.byref(n)), "wino_roi_align_launches")
    return int(n.value)


def boxes_to_rois(boxes) -> torch.Tensor:
    """torchvision's convert_to_roi_format: a list of per-image [L_i][4] box tensors -> [K][5] with the image index in
    front, by torch ops on the device (no host synchronisation); a [K][5] tensor passes through."""
    if isinstance(boxes, torch.Tensor):
        return boxes
    ids = torch.cat([torch.full((int(b.shape[0]), 1), float(i), dtype=b.dtype, device=b.device)
                     for i, b in enumerate(boxes)])
    return torch.cat([ids, torch.cat(list(boxes))], dim=1)


def infer_roi_scales(maps, image_size, in_padded: bool = False):
    """torchvision's MultiScaleRoIAlign.infer_scale: per level 2^round(log2(h_l / H_img)), the same along both axes."""
    import math
    p = 2 if in_padded else 0
    scales = []
    for m in maps:
        per_axis = [2.0 ** round(math.log2((int(m.shape[d]) - p) / float(size))) for d, size in zip((1, 2), image_size)]
        if per_axis[0] != per_axis[1]:
            raise WinoError(f"level map {tuple(m.shape)}: the two axes give different scales {per_axis} for image "
                            f"{tuple(image_size)}")
        scales.append(per_axis[0])
    return scales


def multiscale_roi_align(features, boxes, image_size, P: int, sampling: int = 2, in_padded: bool = False,
                         out_padded: bool = False, canonical_scale: float = 224.0, canonical_level: int = 4,
                         out=None) -> torch.Tensor:
    """torchvision's MultiScaleRoIAlign (aligned=False) on NHWC level maps.  features: a dict as ResNetFPN returns it (its
    "pool" entry is left out, as torchvision's detectors do), or a list / one tensor, finest first; with in_padded the
    padded tensors of ResNetFPN(..., padded=True).  boxes: Tensor[K, 5], or a list of per-image Tensor[L_i, 4].
    image_size: (H, W) of the network's input, from which the scales are inferred.  See roi_align for the result."""
    if isinstance(features, dict):
        maps = [v for k, v in features.items() if k != "pool"]
    else:
        maps = [features] if isinstance(features, torch.Tensor) else list(features)
    scales = infer_roi_scales(maps, image_size, in_padded)
    return roi_align(maps, boxes_to_rois(boxes), P, scales, sampling, in_padded, out_padded, canonical_scale,
                     canonical_level, out)


BBOX_XFORM_CLIP = 4.135166556742356   # log(1000 / 16): torchvision's BoxCoder.bbox_xform_clip


def _int32(t, shape, device, name: str) -> torch.Tensor:
    """The caller's int32 output checked like _out, or a new one of `shape` on `device`."""
    if t is None:
        return torch.empty(shape, dtype=torch.int32, device=device)
    if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous()
            or tuple(t.shape) != tuple(shape)):
        raise WinoError(f"{name} must be a contiguous int32 CUDA(HIP) tensor of shape {tuple(shape)}")
    return t


def box_decode(head, anchors, image_hw, A: int, weights=(1.0, 1.0, 1.0, 1.0), grid=None, delta_col: int = 0,
               score_col=None, out_boxes=None, out_scores=None, out_offset: int = 0, clamp: float = BBOX_XFORM_CLIP):
    """torchvision's BoxCoder.decode_single + clip_boxes_to_image in one HIP launch, on a GEMM output read in place.
    head [...][ld] float32 with N * rows_per_image rows: anchor a of a row has its deltas at columns delta_col + 4a .. + 3
    and, with score_col given, its raw score at column score_col + a.  image_hw [N][2] float32 (H, W) per image.
    grid=(h, w, stride_y, stride_x): anchors is [A][4] base anchors and row (n, y, x) of the h x w level takes base[a]
    shifted by (x stride_x, y stride_y), torchvision's AnchorGenerator; grid=None: anchors is [rows][4], one box per row
    for every a (the second stage, a = class).  Returns (boxes [N][total][4], scores [N][total] or None); this call
    writes [:, out_offset : out_offset + rows_per_image * A] of them, in the order (row, a).  Given out_boxes /
    out_scores may be wider than that (a level's slice of all levels' proposals); new ones are exactly that wide.
    No scratch: capturable into a graph without a prepare."""
    h = _dev(head, "head")
    hw = _dev(image_hw, "image_hw")
    anc = _dev(anchors, "anchors")
    A, off = int(A), int(out_offset)
    if h.dim() < 2 or hw.dim() != 2 or int(hw.shape[1]) != 2:
        raise WinoError("head must be [...][ld] and image_hw [N][2]")
    ld, N = int(h.shape[-1]), int(hw.shape[0])
    rows = h.numel() // ld if ld else 0
    if N < 1 or A < 1 or rows % N or off < 0:
        raise WinoError(f"box_decode: {rows} rows for N={N} images, A={A}, out_offset={off}")
    rpi = rows // N
    if grid is None:
        gh = gw = sy = sx = 0
        want = (rows, 4)
    else:
        gh, gw, sy, sx = (int(v) for v in grid)
        want = (A, 4)
        if gh * gw != rpi:
            raise WinoError(f"box_decode: grid {gh}x{gw} but {rpi} rows per image")
    if tuple(anc.shape) != want:
        raise WinoError(f"anchors must have shape {want}, got {tuple(anc.shape)}")
    wx, wy, ww, wh = (float(v) for v in weights)
    per_image = rpi * A

    def slot(t, tail, name):
        if t is None:
            if off:
                raise WinoError(f"out_offset={off} needs {name}")
            return torch.empty((N, per_image) + tail, dtype=torch.float32, device=h.device)
        _out(t, None, name)
        if t.dim() != 2 + len(tail) or int(t.shape[0]) != N or tuple(t.shape[2:]) != tail or int(t.shape[1]) < off + per_image:
            raise WinoError(f"{name} must be [{N}][total >= {off + per_image}]{list(tail)}, got {tuple(t.shape)}")
        return t

    boxes = slot(out_boxes, (4,), "out_boxes")
    scores = None if score_col is None else slot(out_scores, (), "out_scores")
    _on_current_device(h, hw, anc, boxes, scores)
    _check(lib().wino_box_decode_hw(h.data_ptr() or None, N, rpi, ld, A, int(delta_col),
                                    -1 if score_col is None else int(score_col), anc.data_ptr() or None, gh, gw, sy, sx,
                                    hw.data_ptr(), wx, wy, ww, wh, float(clamp), boxes.data_ptr() or None,
                                    int(boxes.shape[1]), off, None if scores is None else (scores.data_ptr() or None),
                                    0 if scores is None else int(scores.shape[1]), off, _stream()), "wino_box_decode_hw")
    return boxes, scores


def nms_workspace_bytes(S: int, R: int) -> int:
    """Bytes of batched_nms's workspace, the formula of winograd_mi355x.h (wino_batched_nms_hw refuses less): the
    suppression bit matrix, R rows of ceil(R / 64) 64-bit words per segment."""
    S, R = int(S), int(R)
    if S < 1 or R < 1:
        return 0
    return S * R * ((R + 63) // 64) * 8


def batched_nms(boxes, scores=None, groups=None, iou_thresh: float = 0.5, min_size: float = 0.0,
                score_thresh: float = float("-inf"), max_out=None, rois_out=False, workspace=None, keep=None, count=None):
    """Greedy NMS over S independent segments of R boxes in two HIP launches, never leaving the device, with fixed-size
    outputs.  boxes [S][R][4] float32, already in priority order (the caller sorts; ties are the caller's too); scores
    [S][R] float32 or None; groups [S][R] int32 or None (boxes of different groups never suppress each other).  A box is
    a candidate when both sides are >= min_size and its score >= score_thresh; the first max_out (default R) candidates
    that no kept box of their group overlaps by IoU > iou_thresh are kept.  Returns (keep [S][max_out] int32: the kept
    indices ascending, then -1; count [S] int32[; rois [S][max_out][5] = (segment, box), padding rows (-1, 0, 0, 0, 0):
    roi_align's input]).  rois_out: True, or the tensor to write.  workspace: nms_workspace_bytes(S, R) bytes.  No
    scratch of the library's: capturable into a graph without a prepare."""
    b = _dev(boxes, "boxes")
    if b.dim() != 3 or int(b.shape[2]) != 4:
        raise WinoError("boxes must be [S][R][4]")
    S, R = int(b.shape[0]), int(b.shape[1])
    sc = None if scores is None else _dev(scores, "scores")
    if sc is not None and tuple(sc.shape) != (S, R):
        raise WinoError(f"scores must be [{S}][{R}]")
    g = None if groups is None else _int32(groups, (S, R), b.device, "groups")
    max_out = max(R, 1) if max_out is None else int(max_out)
    if max_out < 1:
        raise WinoError(f"batched_nms: max_out={max_out}")
    keep = _int32(keep, (S, max_out), b.device, "keep")
    count = _int32(count, (S,), b.device, "count")
    rois = None
    if rois_out is not False and rois_out is not None:
        rois = _output(None if rois_out is True else rois_out, (S, max_out, 5), b.device, "rois_out")
    ws = _workspace(workspace, nms_workspace_bytes(S, R), b.device)
    _on_current_device(b, sc, g, keep, count, rois, ws)
    if R == 0 and rois is not None and S > 0:   # the library launches nothing: every row is a padding row
        rois.zero_()
        rois[:, :, 0] = -1.0
    ptr = lambda t: None if t is None else (t.data_ptr() or None)
    _check(lib().wino_batched_nms_hw(ptr(b), ptr(sc), ptr(g), S, R, float(iou_thresh), float(min_size),
                                     float(score_thresh), max_out, ptr(keep), ptr(count), ptr(rois), ptr(ws),
                                     ws.numel() * 4, _stream()), "wino_batched_nms_hw")
    return (keep, count) if rois is None else (keep, count, rois)


SELECT_MAX_K = 8192   # the keys one workgroup of select.hip sorts in LDS: the most a part can keep


def _select_parts(k, n, off, stride=None):
    """(k, n, off) as equally long lists of ints: each an int (one part) or a sequence; n defaults to the rest of the
    row behind off, off to 0."""
    ks = [int(v) for v in k] if isinstance(k, (list, tuple)) else [int(k)]
    parts = len(ks)

    def seq(v, name, default):
        if v is None:
            return default
        v = [int(x) for x in v] if isinstance(v, (list, tuple)) else [int(v)]
        if len(v) != parts:
            raise WinoError(f"select: {name} has {len(v)} entries for {parts} parts")
        return v

    offs = seq(off, "off", [0] * parts)
    if n is None and stride is None:
        raise WinoError("select: n is needed")
    ns = seq(n, "n", None if stride is None else [int(stride) - o for o in offs])
    return ks, ns, offs


def select_workspace_bytes(N: int, n, k) -> int:
    """Bytes of select_topk's workspace for N images whose parts have n[p] scores and keep k[p] (ints or sequences), the
    formula of winograd_mi355x.h (wino_select_topk_hw refuses less): per part longer than 8192 scores three histograms
    and a list length, one word per chunk of 2048 scores and k[p] 64-bit keys, each region rounded up to 16 bytes.  0 when
    every n[p] <= 8192.  Host only; raises WinoError outside the entry point's limits."""
    ks, ns, _ = _select_parts(k, n, None)
    N = int(N)
    if N < 0 or not 1 <= len(ks) <= 8 or min(ns) < 0 or min(ks) < 1 or max(ks) > SELECT_MAX_K:
        raise WinoError(f"select: unsupported shape N={N} n={ns} k={ks} (need N >= 0, 1 <= parts <= 8, n[p] >= 0, "
                        f"1 <= k[p] <= {SELECT_MAX_K})")
    long_parts = [(n_p, k_p) for n_p, k_p in zip(ns, ks) if n_p > SELECT_MAX_K]
    round16 = lambda b: (b + 15) // 16 * 16
    header, chunk = 3 * 2048 + 4, 2048   # select.hip's SEL_HDR words per long segment and SEL_CHUNK scores per workgroup
    return (round16(N * len(long_parts) * header * 4) + round16(N * sum((n_p + chunk - 1) // chunk for n_p, _ in long_parts) * 4)
            + round16(N * sum(k_p for _, k_p in long_parts) * 8))


def select_topk(scores, k, n=None, off=None, score_thresh=None, boxes=None, out_idx=None, out_vals=None, out_count=None,
                out_boxes=None, workspace=None):
    """Segmented top-k and sort on the device (select.hip), with fixed-size outputs and an order that is a function of the
    inputs: torch.sort(descending=True, stable=True) truncated to k (NaN first, -0.0 == +0.0, ties to the lower index).
    scores [N][stride] float32.  k, n, off: ints, or sequences for several parts; part p of every image reads n[p] scores
    from column off[p] (default: one part over the whole row) and keeps the best min(k[p], candidates), where with
    score_thresh given only scores >= score_thresh are candidates.  Part p writes k[p] rows behind those of the parts
    before it.  Returns (idx [N][sum k] int32: column indices within the row, -1 past the kept count; vals [N][sum k]: the
    scores' own bits, 0.0 past it; count [N][parts] int32[; boxes [N][sum k][4]: with boxes [N][stride][4] given, the kept
    scores' rows, zeros past the count]).  Given outputs may be wider than sum k; what lies behind is not written.
    workspace: select_workspace_bytes(N, n, k) bytes.  No scratch of the library's: capturable into a graph without a
    prepare."""
    sc = _dev(scores, "scores")
    if sc.dim() != 2:
        raise WinoError("scores must be [N][stride]")
    N, stride = int(sc.shape[0]), int(sc.shape[1])
    ks, ns, offs = _select_parts(k, n, off, stride)
    parts, ksum = len(ks), sum(ks)
    bx = None
    if boxes is not None:
        bx = _dev(boxes, "boxes")
        if bx.dim() != 3 or int(bx.shape[0]) != N or int(bx.shape[2]) != 4:
            raise WinoError(f"boxes must be [{N}][stride][4]")

    def slot(t, tail, dtype, name):
        if t is None:
            return torch.empty((N, ksum) + tail, dtype=dtype, device=sc.device)
        if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous()
                or t.dim() != 2 + len(tail) or int(t.shape[0]) != N or tuple(t.shape[2:]) != tail or int(t.shape[1]) < ksum):
            raise WinoError(f"{name} must be a contiguous {dtype} CUDA(HIP) tensor [{N}][>= {ksum}]{list(tail)}")
        return t

    idx = slot(out_idx, (), torch.int32, "out_idx")
    vals = slot(out_vals, (), torch.float32, "out_vals")
    count = _int32(out_count, (N, parts), sc.device, "out_count")
    ob = None if bx is None else slot(out_boxes, (4,), torch.float32, "out_boxes")
    out_stride = int(idx.shape[1])
    if int(vals.shape[1]) != out_stride or (ob is not None and int(ob.shape[1]) != out_stride):
        raise WinoError("select_topk: out_idx, out_vals and out_boxes must have the same row length")
    ws = _workspace(workspace, select_workspace_bytes(N, ns, ks), sc.device)
    _on_current_device(sc, bx, idx, vals, count, ob, ws)
    ptr = lambda t: None if t is None else (t.data_ptr() or None)
    _check(lib().wino_select_topk_hw(ptr(sc), N, stride, parts, (c_long * parts)(*offs), (c_int * parts)(*ns),
                                     (c_int * parts)(*ks), 0 if score_thresh is None else 1,
                                     0.0 if score_thresh is None else float(score_thresh), ptr(idx), ptr(vals), ptr(count),
                                     out_stride, ptr(bx), 0 if bx is None else int(bx.shape[1]), ptr(ob), ptr(ws),
                                     ws.numel() * 4, _stream()), "wino_select_topk_hw")
    return (idx, vals, count) if ob is None else (idx, vals, count, ob)


SELECT_MAX_N = (1 << 31) - 1   # the longest segment: an index must fit idx's int32


def select_map_workspace_bytes(N: int, h: int, w: int, cols: int, k: int) -> int:
    """Bytes of select_topk_map's workspace for N maps of h x w pixels with `cols` scores each: select_workspace_bytes
    for the one part n = h * w * cols, the formula of winograd_mi355x.h.  Host only; raises WinoError outside the
    entry point's limits, a segment longer than 2^31 - 1 scores among them."""
    N, h, w, cols, k = int(N), int(h), int(w), int(cols), int(k)
    if h < 1 or w < 1 or cols < 1:
        raise WinoError(f"select_topk_map: unsupported shape h={h} w={w} cols={cols} (need h, w, cols >= 1)")
    n = h * w * cols
    if n > SELECT_MAX_N:
        raise WinoError(f"select_topk_map: a segment of h w cols = {h} x {w} x {cols} scores is longer than 2^31 - 1")
    return select_workspace_bytes(N, n, k)


def select_topk_map(scores_map, cols: int, k: int, score_thresh=None, out_idx=None, out_vals=None, out_count=None,
                    out_offset: int = 0, workspace=None):
    """select_topk on a padded NHWC map, in place (select.hip).  scores_map [N][h+2][w+2][ld] float32, what a 3x3 layer
    writes; image i's segment is its h * w * cols scores map[i][1 + y][1 + x][c], c < cols <= ld, and the index of one is
    (y * w + x) * cols + c: with cols = A * K and channel a * K + k, torchvision's (N, HWA, K) flattening.  The ring and
    the pad columns have no index and are never read as candidates.  Order, NaN and +-0 rules, score_thresh (>=) and
    k <= 8192 are select_topk's.  Returns (idx [N][total] int32, vals [N][total], count [N] int32); this call writes
    [:, out_offset : out_offset + k] of idx and vals (a level's slice of one buffer for all levels; new ones are exactly k
    wide).  workspace: select_map_workspace_bytes(N, h, w, cols, k) bytes.  No scratch of the library's: capturable into
    a graph without a prepare."""
    m = _dev(scores_map, "scores_map")
    if m.dim() != 4 or int(m.shape[1]) < 3 or int(m.shape[2]) < 3:
        raise WinoError("scores_map must be [N][h+2][w+2][ld]")
    N, h, w, ld = int(m.shape[0]), int(m.shape[1]) - 2, int(m.shape[2]) - 2, int(m.shape[3])
    cols, k, off = int(cols), int(k), int(out_offset)
    if not 1 <= cols <= ld or off < 0:
        raise WinoError(f"select_topk_map: cols={cols} of ld={ld}, out_offset={off}")
    need = select_map_workspace_bytes(N, h, w, cols, k)

    def slot(t, dtype, name):
        if t is None:
            if off:
                raise WinoError(f"out_offset={off} needs {name}")
            return torch.empty((N, k), dtype=dtype, device=m.device)
        if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or t.dim() != 2
                or int(t.shape[0]) != N or int(t.shape[1]) < off + k):
            raise WinoError(f"{name} must be a contiguous {dtype} CUDA(HIP) tensor [{N}][>= {off + k}]")
        return t

    idx = slot(out_idx, torch.int32, "out_idx")
    vals = slot(out_vals, torch.float32, "out_vals")
    count = _int32(out_count, (N,), m.device, "out_count")
    if int(vals.shape[1]) != int(idx.shape[1]):
        raise WinoError("select_topk_map: out_idx and out_vals must have the same row length")
    ws = _workspace(workspace, need, m.device)
    _on_current_device(m, idx, vals, count, ws)
    ptr = lambda t: None if t is None else (t.data_ptr() or None)
    _check(lib().wino_select_topk_map_hw(ptr(m), N, h, w, cols, ld, k, 0 if score_thresh is None else 1,
                                         0.0 if score_thresh is None else float(score_thresh), ptr(idx), ptr(vals),
                                         ptr(count), int(idx.shape[1]), off, ptr(ws), ws.numel() * 4, _stream()),
           "wino_select_topk_map_hw")
    return idx, vals, count


def _decode_rows(entry: str, idx, reg_map, base, image_hw, grid, K, k, out_boxes, out_labels, out_offset, clamp=None):
    """retina_decode's and fcos_decode's checks and launch: entry point wino_`entry`_hw, messages under `entry`; `clamp` is
    passed on only where it is given (the FCOS entry point takes none)."""
    ix = idx
    if not isinstance(ix, torch.Tensor) or not ix.is_cuda or ix.dtype != torch.int32 or not ix.is_contiguous() or ix.dim() != 2:
        raise WinoError("idx must be a contiguous int32 CUDA(HIP) tensor [N][total]")
    reg, anc, hw = _dev(reg_map, "reg_map"), _dev(base, "base"), _dev(image_hw, "image_hw")
    N, total, off = int(ix.shape[0]), int(ix.shape[1]), int(out_offset)
    gh, gw, sy, sx = (int(v) for v in grid)
    if reg.dim() != 4 or tuple(reg.shape[:3]) != (N, gh + 2, gw + 2) or tuple(hw.shape) != (N, 2):
        raise WinoError(f"reg_map must be [{N}][{gh + 2}][{gw + 2}][ld_r] and image_hw [{N}][2]")
    if anc.dim() != 2 or int(anc.shape[1]) != 4:
        raise WinoError("base must be [A][4]")
    k = total - off if k is None else int(k)
    if off < 0 or k < 0 or off + k > total:
        raise WinoError(f"{entry}: rows {off} .. {off + k} of {total}")
    boxes = _output(out_boxes, (N, total, 4), ix.device, "out_boxes")
    labels = _int32(out_labels, (N, total), ix.device, "out_labels")
    _on_current_device(ix, reg, anc, hw, boxes, labels)
    ptr = lambda t: t.data_ptr() or None
    _check(getattr(lib(), f"wino_{entry}_hw")(ptr(ix), N, k, total, off, ptr(reg), gh, gw, int(reg.shape[3]), int(anc.shape[0]),
                                              int(K), ptr(anc), sy, sx, ptr(hw), *(() if clamp is None else (float(clamp),)),
                                              ptr(boxes), ptr(labels), _stream()), f"wino_{entry}_hw")
    return boxes, labels


def retina_decode(idx, reg_map, base, image_hw, grid, K: int, k=None, out_boxes=None, out_labels=None, out_offset: int = 0,
                  clamp: float = BBOX_XFORM_CLIP):
    """RetinaNet's decode of the selected anchors only, in one HIP launch (retina.hip).  idx [N][total] int32 as
    select_topk_map writes it with cols = A * K; this call reads rows [:, out_offset : out_offset + k] (k defaults to the
    rest of the row): anchor = idx // K, label = idx % K.  reg_map [N][h+2][w+2][ld_r] float32, the regression head's
    padded output with the deltas of anchor a at columns 4a .. 4a + 3; base [A][4]; image_hw [N][2];
    grid = (h, w, stride_y, stride_x).  The box is box_decode's in grid mode at the same anchor, bit for bit (weights
    (1, 1, 1, 1), clamp, clipped to the image).  Returns (boxes [N][total][4], labels [N][total] int32), of which the
    same rows are written; rows with idx < 0 get a zero box and label -1.  No scratch: capturable without a prepare."""
    return _decode_rows("retina_decode", idx, reg_map, base, image_hw, grid, K, k, out_boxes, out_labels, out_offset, clamp)


GN_FORMS = {1: "whole", 2: "split"}   # WINO_GN_FORM_*


def groupnorm_plan(N: int, h: int, w: int, C: int, groups: int, cus: int = 256):
    """(form, chunks) of groupnorm_relu for N maps of h x w pixels and C channels in `groups` groups on a device of `cus`
    CUs: form "whole" (one launch, chunks = 1) or "split" (statistics per chunk of pixels, then apply).  Host only;
    WINO_GN_FORM = whole | split (read at the library's first use, or by wino_debug_reload_knobs) forces a form.  Raises WinoError outside the layer's limits."""
    form, chunks = _plan_query("wino_groupnorm_plan", 2, int(N), int(h), int(w), int(C), int(groups), int(cus))
    return GN_FORMS[form], chunks


def groupnorm_workspace_bytes(N: int, h: int, w: int, C: int, groups: int) -> int:
    """Bytes of groupnorm_relu's workspace: 0 for the whole form, N * min(h w, 128) * 4 * groups * 4 for the split form
    (enough on any device): the formula of winograd_mi355x.h.  Host only; raises WinoError outside the layer's limits."""
    form, _ = groupnorm_plan(N, h, w, C, groups)
    return 0 if form == "whole" else int(N) * min(int(h) * int(w), 128) * 4 * int(groups) * 4


def groupnorm_relu(x, gamma, beta, groups: int, eps: float = 1e-5, relu: bool = True, out=None, workspace=None):
    """torch's F.group_norm(x, groups, gamma, beta, eps), then ReLU when `relu`, on a padded NHWC map (groupnorm.hip).
    x [N][h+2][w+2][C] float32, what a 3x3 layer writes; gamma, beta [C].  Statistics per (image, group) over the h * w *
    (C / groups) interior values, biased variance; only the interior of `out` is written (a new `out` starts as zeros, so
    its ring is the padding the next 3x3 reads).  out=x normalises in place.  C a multiple of 64, C / groups a power of
    two.  workspace: groupnorm_workspace_bytes(...) bytes.  One launch or two (groupnorm_plan); deterministic; no scratch
    of the library's: capturable into a graph without a prepare."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 4 \
            or int(x.shape[1]) < 3 or int(x.shape[2]) < 3:
        raise WinoError("x must be a contiguous float32 CUDA(HIP) tensor [N][h+2][w+2][C]")
    N, h, w, C = int(x.shape[0]), int(x.shape[1]) - 2, int(x.shape[2]) - 2, int(x.shape[3])
    g, b = _dev(gamma, "gamma"), _dev(beta, "beta")
    if tuple(g.shape) != (C,) or tuple(b.shape) != (C,):
        raise WinoError(f"gamma and beta must be [{C}]")
    need = groupnorm_workspace_bytes(N, h, w, C, groups)
    o = torch.zeros_like(x) if out is None else _out(out, x.shape, "out")
    ws = _workspace(workspace, need, x.device) if need or workspace is not None else None
    _on_current_device(x, g, b, o, ws)
    ptr = lambda t: None if t is None else (t.data_ptr() or None)
    _check(lib().wino_groupnorm_relu_hw(ptr(x), ptr(g), ptr(b), ptr(o), N, h, w, C, int(groups), float(eps), 1 if relu else 0,
                                        ptr(ws), 0 if ws is None else ws.numel() * 4, _stream()), "wino_groupnorm_relu_hw")
    return o


def fcos_score_map(cls_map, reg_map, K: int, ctr_col: int = 4):
    """FCOS's score of every location, in place on the class-logit map, in one HIP launch (fcos.hip).  cls_map
    [N][h+2][w+2][ld_c] float32: interior columns < K become sqrt(sigmoid(logit) * sigmoid(ctr)) with ctr = column ctr_col
    of the same pixel of reg_map [N][h+2][w+2][ld_r].  Rings and pad columns are neither read nor written.  Returns
    cls_map.  No scratch: capturable without a prepare."""
    for t, name in ((cls_map, "cls_map"), (reg_map, "reg_map")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 4:
            raise WinoError(f"{name} must be a contiguous float32 CUDA(HIP) tensor [N][h+2][w+2][ld]")
    if tuple(cls_map.shape[:3]) != tuple(reg_map.shape[:3]) or int(cls_map.shape[1]) < 3 or int(cls_map.shape[2]) < 3:
        raise WinoError("cls_map and reg_map must be [N][h+2][w+2][ld] maps of one level")
    N, h, w = int(cls_map.shape[0]), int(cls_map.shape[1]) - 2, int(cls_map.shape[2]) - 2
    _on_current_device(cls_map, reg_map)
    _check(lib().wino_fcos_score_map_hw(cls_map.data_ptr() or None, reg_map.data_ptr() or None, N, h, w, int(K),
                                        int(cls_map.shape[3]), int(reg_map.shape[3]), int(ctr_col), _stream()),
           "wino_fcos_score_map_hw")
    return cls_map


def fcos_decode(idx, reg_map, base, image_hw, grid, K: int, k=None, out_boxes=None, out_labels=None, out_offset: int = 0):
    """FCOS's decode of the selected locations only, in one HIP launch (fcos.hip): retina_decode's operands, rows and
    outputs, with the anchor-free box of torchvision's BoxLinearCoder(normalize_by_size=True): (l, t, r, b) = relu of
    columns 4a .. 4a + 3 of reg_map, box = (cx - l w, cy - t h, cx + r w, cy + b h) of the shifted base anchor, clipped to
    the image.  Rows with idx < 0 get a zero box and label -1.  No scratch: capturable without a prepare."""
    return _decode_rows("fcos_decode", idx, reg_map, base, image_hw, grid, K, k, out_boxes, out_labels, out_offset)


MASK_LAYOUTS = {"planes": 0, "gemm_rows": 1}   # WINO_MASK_LAYOUT_*
MASK_MAX_M = 62


def _uint8(t, shape, device, name: str) -> torch.Tensor:
    """The caller's uint8 output checked like _out, or a new one of `shape` on `device`."""
    if t is None:
        return torch.empty(shape, dtype=torch.uint8, device=device)
    if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous()
            or tuple(t.shape) != tuple(shape)):
        raise WinoError(f"{name} must be a contiguous uint8 CUDA(HIP) tensor of shape {tuple(shape)}")
    return t


def paste_masks(logits, labels, boxes, image_hw, H: int, W: int, M=None, classes=None, layout: str = "planes",
                out=None, binary=None, want_out: bool = True, want_binary: bool = False, threshold: float = 0.5):
    """torchvision's maskrcnn_inference + paste_masks_in_image (padding 1) for all detections in one HIP launch: detection
    r = n D + d takes the mask of class labels[r] out of `logits`, applies the sigmoid and pastes it, resized to its box
    grown by (M + 2) / M, into plane (n, d).  logits, read in place: layout "planes" [R][classes][M][M] (M and classes
    from the shape), or "gemm_rows" [R (M/2)^2 4][ld], the mask head's logits GEMM output (MaskHead's raw form; M must be
    given, classes defaults to ld).  labels [N][D] (or [R]) int32: a label outside [0, classes), such as a padding row's
    -1, gives a zero plane.  boxes [N][D][4] (or [R][4]) float32; image_hw [N][2] float32 (H, W) per image, beyond which
    the plane is zero.  Returns (out, binary): out [N][D][H][W] float32 or None, binary [N][D][H][W] uint8 = out >
    threshold or None.  A given `out` / `binary` tensor is written and implies want_out / want_binary.  No scratch:
    capturable into a graph without a prepare."""
    if layout not in MASK_LAYOUTS:
        raise WinoError(f"paste_masks: layout must be one of {sorted(MASK_LAYOUTS)}, got {layout!r}")
    H, W, threshold = int(H), int(W), float(threshold)
    if H < 1 or W < 1 or H * W >= 1 << 31:
        raise WinoError(f"paste_masks: bad plane H={H} W={W} (need H, W >= 1, H W < 2^31)")
    if threshold != threshold:
        raise WinoError("paste_masks: threshold is NaN")
    want_out, want_binary = bool(want_out) or out is not None, bool(want_binary) or binary is not None
    if not want_out and not want_binary:
        raise WinoError("paste_masks: neither out nor binary is wanted")
    lg = _dev(logits, "logits")
    hw = _dev(image_hw, "image_hw")
    bx = _dev(boxes, "boxes")
    if hw.dim() != 2 or int(hw.shape[1]) != 2:
        raise WinoError("image_hw must be [N][2]")
    N = int(hw.shape[0])
    if bx.dim() not in (2, 3) or int(bx.shape[-1]) != 4:
        raise WinoError("boxes must be [N][D][4] or [N D][4]")
    R = bx.numel() // 4
    if N < 1 or R % N:
        raise WinoError(f"paste_masks: {R} boxes for N={N} images")
    D = R // N
    if not isinstance(labels, torch.Tensor):
        raise WinoError("labels must be an int32 CUDA(HIP) tensor")
    lb = _int32(labels, tuple(labels.shape), bx.device, "labels")
    if lb.numel() != R:
        raise WinoError(f"labels must hold {R} int32, one per box, got {tuple(lb.shape)}")
    if layout == "planes":
        if lg.dim() != 4 or int(lg.shape[0]) != R or int(lg.shape[2]) != int(lg.shape[3]):
            raise WinoError(f"logits must be [{R}][classes][M][M] in the planes layout, got {tuple(lg.shape)}")
        ld = cls = int(lg.shape[1])
        m = int(lg.shape[2])
        if (M is not None and int(M) != m) or (classes is not None and int(classes) != cls):
            raise WinoError(f"paste_masks: M={M} classes={classes} but logits is {tuple(lg.shape)}")
    else:
        if M is None:
            raise WinoError("paste_masks: the gemm_rows layout needs M")
        m = int(M)
        if lg.dim() != 2 or m < 2 or m % 2 or int(lg.shape[0]) != R * m * m:
            raise WinoError(f"logits must be [{R} * M * M][ld] with M even in the gemm_rows layout, got {tuple(lg.shape)} "
                            f"for M={m}")
        ld = int(lg.shape[1])
        cls = ld if classes is None else int(classes)
    if not 1 <= m <= MASK_MAX_M or not 1 <= cls <= ld:
        raise WinoError(f"paste_masks: need 1 <= M <= {MASK_MAX_M} and 1 <= classes <= ld, got M={m} classes={cls} ld={ld}")
    if want_out:
        out = _output(out, (N, D, H, W), bx.device)
    if want_binary:
        binary = _uint8(binary, (N, D, H, W), bx.device, "binary")
    _on_current_device(lg, lb, bx, hw, out, binary)
    ptr = lambda t: None if t is None else (t.data_ptr() or None)
    _check(lib().wino_mask_paste_hw(ptr(lg), MASK_LAYOUTS[layout], ptr(lb), ptr(bx), ptr(hw), N, D, cls, m, ld, H, W,
                                    threshold, ptr(out) if want_out else None, ptr(binary) if want_binary else None,
                                    _stream()), "wino_mask_paste_hw")
    return (out if want_out else None), (binary if want_binary else None)


KP_LAYOUTS = {"planes": 0, "deconv_rows": 1}   # WINO_KP_LAYOUT_*
KP_MAX_M = 64
KP_MAX_SIDE = 16384


def heatmaps_to_keypoints(maps, rois, K=None, M=None, layout: str = "planes", bias=None, ld=None, max_side: int = 16384,
                          out=None, scores_out=None):
    """torchvision's heatmaps_to_keypoints for all detections in one HIP launch: heatmap plane (r, k) is resized to the box
    of detection r with torch's bicubic (exact integer source coordinates), and the argmax becomes keypoint k of that
    detection.  maps, read in place: layout "planes" [R][K][M][M] (K and M from the shape), or "deconv_rows" [R (M/4)^2][ld],
    the partial products of ConvTranspose2d(C, K, 4, 2, 1) as KeypointHead's raw form leaves them (K and M must be given,
    ld is read off the shape, bias [K] is required; the kernel gathers them, adds the bias and upsamples x2).  rois
    [R][5] (or [N][D][5]) float32 (n, x1, y1, x2, y2): a padding row, !(n >= 0), gives zeros; a box that is not finite or
    larger than max_side gives NaN and reads no map.  Returns (keypoints [R][K][3] (or [N][D][K][3]) = (x, y, 1) in image
    coordinates, scores [R][K] = the heatmap value there); `out` / `scores_out` are written when given.  No scratch:
    capturable into a graph without a prepare."""
    if layout not in KP_LAYOUTS:
        raise WinoError(f"heatmaps_to_keypoints: layout must be one of {sorted(KP_LAYOUTS)}, got {layout!r}")
    max_side = int(max_side)
    if not 1 <= max_side <= KP_MAX_SIDE:
        raise WinoError(f"heatmaps_to_keypoints: need 1 <= max_side <= {KP_MAX_SIDE}, got {max_side}")
    mp = _dev(maps, "maps")
    ro = _dev(rois, "rois")
    if ro.dim() not in (2, 3) or int(ro.shape[-1]) != 5:
        raise WinoError("rois must be [R][5] or [N][D][5]")
    R = ro.numel() // 5
    if layout == "planes":
        if mp.dim() != 4 or int(mp.shape[0]) != R or int(mp.shape[2]) != int(mp.shape[3]):
            raise WinoError(f"maps must be [{R}][K][M][M] in the planes layout, got {tuple(mp.shape)}")
        k, m = int(mp.shape[1]), int(mp.shape[2])
        if (K is not None and int(K) != k) or (M is not None and int(M) != m):
            raise WinoError(f"heatmaps_to_keypoints: K={K} M={M} but maps is {tuple(mp.shape)}")
        if bias is not None:
            raise WinoError("heatmaps_to_keypoints: the planes layout takes no bias")
        if not 1 <= m <= KP_MAX_M or k < 1:
            raise WinoError(f"heatmaps_to_keypoints: need 1 <= M <= {KP_MAX_M} and K >= 1, got M={m} K={k}")
        lead, b = 0, None
    else:
        if K is None or M is None:
            raise WinoError("heatmaps_to_keypoints: the deconv_rows layout needs K and M")
        k, m = int(K), int(M)
        if k < 1 or m < 4 or m % 4 or m > KP_MAX_M:
            raise WinoError(f"heatmaps_to_keypoints: the deconv_rows layout needs K >= 1 and M = 4 P <= {KP_MAX_M}, got "
                            f"K={k} M={m}")
        if mp.dim() != 2 or int(mp.shape[0]) != R * (m // 4) ** 2:
            raise WinoError(f"maps must be [{R} * (M/4)^2][ld] in the deconv_rows layout, got {tuple(mp.shape)} for M={m}")
        lead = int(mp.shape[1])
        if (ld is not None and int(ld) != lead) or lead < 16 * k:
            raise WinoError(f"heatmaps_to_keypoints: ld={ld} K={k} but maps is {tuple(mp.shape)} (need 16 K <= ld)")
        if bias is None:
            raise WinoError("heatmaps_to_keypoints: the deconv_rows layout needs bias")
        b = _dev(bias, "bias")
        if tuple(b.shape) != (k,):
            raise WinoError(f"bias must be [{k}], got {tuple(b.shape)}")
    front = tuple(ro.shape[:-1])
    out = _output(out, front + (k, 3), ro.device)
    scores_out = _output(scores_out, front + (k,), ro.device, "scores_out")
    _on_current_device(mp, ro, b, out, scores_out)
    ptr = lambda t: None if t is None else (t.data_ptr() or None)
    _check(lib().wino_keypoints_hw(ptr(mp), KP_LAYOUTS[layout], ptr(b), ptr(ro), R, k, m, lead, max_side, ptr(out),
                                   ptr(scores_out), _stream()), "wino_keypoints_hw")
    return out, scores_out


def _groups_of(packed: torch.Tensor, C: int, groups: int, name: str) -> int:
    """`groups` checked against C and against a buffer from filter_pack_grouped (a wrong-sized one would be read out of
    bounds by the kernel)."""
    groups = int(groups)
    n = lib().wino_conv3x3_grouped_filter_elems(C, groups)
    if n == 0:
        raise WinoError(f"grouped 3x3: unsupported C={C} groups={groups} "
                        "(need C % 64 == 0 and C / groups in {4, 8, 16, 32, 64})")
    if packed.dim() != 1 or packed.numel() != n:
        raise WinoError(f"{name} does not match C={C} groups={groups}: pack it with filter_pack_grouped")
    return groups


def filter_pack_grouped(w: torch.Tensor, groups: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """torch's grouped 3x3 weight [C][C/groups][3][3] -> the grouped layer's packed filter (opaque layout,
    wino_conv3x3_grouped_filter_elems floats), the analogue of filter_transform_f2 for conv3x3_grouped_bn_relu."""
    w = _dev(w, "w")
    groups = int(groups)
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or groups < 1 or int(w.shape[0]) != int(w.shape[1]) * groups:
        raise WinoError("w must be [C][C/groups][3][3]")
    C = int(w.shape[0])
    n = lib().wino_conv3x3_grouped_filter_elems(C, groups)
    if n == 0:
        raise WinoError(f"grouped 3x3: unsupported C={C} groups={groups} "
                        "(need C % 64 == 0 and C / groups in {4, 8, 16, 32, 64})")
    packed = _output(out, (n,), w.device)
    _on_current_device(w, packed)
    _check(lib().wino_conv3x3_grouped_filter_pack(w.data_ptr(), packed.data_ptr(), C, groups, _stream()),
           "wino_conv3x3_grouped_filter_pack")
    return packed


def conv3x3_grouped_bn_relu(inp: torch.Tensor, packed: torch.Tensor, bn_bias: torch.Tensor, bn_scale: torch.Tensor,
                            groups: int, stride: int = 1, relu: bool = True,
                            out: torch.Tensor | None = None) -> torch.Tensor:
    """Grouped 3x3 conv (stride 1 or 2, pad 1) + folded BN (+ReLU): inp [N][Hin+2][Win+2][C] (zero ring) ->
    out [N][H+2][W+2][C] (interior H x W = (Hin-1)//stride + 1 x (Win-1)//stride + 1, zero ring).  packed from
    filter_pack_grouped(w, groups).  One HIP launch."""
    x, packed = _dev(inp, "inp"), _dev(packed, "packed")
    b, s = _dev(bn_bias, "bn_bias"), _dev(bn_scale, "bn_scale")
    if x.dim() != 4 or x.shape[1] < 3 or x.shape[2] < 3:
        raise WinoError("inp must be [N][Hin+2][Win+2][C]")
    N, Hin, Win, C = int(x.shape[0]), int(x.shape[1]) - 2, int(x.shape[2]) - 2, int(x.shape[3])
    groups = _groups_of(packed, C, groups, "packed")
    if b.numel() != C or s.numel() != C:
        raise WinoError("bn vectors do not match C")
    if int(stride) not in (1, 2):
        raise WinoError(f"stride must be 1 or 2, got {stride}")
    H, W = _out_hw(Hin, Win, int(stride))
    out = _output(out, (N, H + 2, W + 2, C), x.device)
    _on_current_device(x, packed, b, s, out)
    _check(lib().wino_conv3x3_grouped_bn_relu_hw(x.data_ptr(), packed.data_ptr(), b.data_ptr(), s.data_ptr(),
                                                 out.data_ptr(), N, Hin, Win, C, groups, int(stride), int(relu),
                                                 _stream()), "wino_conv3x3_grouped_bn_relu_hw")
    return out


def conv3x3_grouped_plan(N: int, Hin: int, Win: int, C: int, groups: int, stride: int = 1):
    """(tile_w, kc, tiles_y, tiles_x) of conv3x3_grouped_bn_relu's launch for this shape (host-side): the tile width
    and contraction width of the kernel instantiation, and the tiles of one image."""
    return _plan_query("wino_conv3x3_grouped_plan", 4, int(N), int(Hin), int(Win), int(C), int(groups), int(stride))


def grouped_residual_block_prepare(N: int, H: int, W: int, C4: int, Cm: int, groups: int) -> None:
    """Allocate the scratch of grouped_residual_block's two 1x1 launches for the current stream (before graph capture)."""
    _prepare("wino_grouped_residual_block_prepare_hw", N, H, W, C4, Cm, groups)


def grouped_residual_block(x, w1, bn1, wg, bn2, w3, bn3, groups: int, out=None, workspace=None) -> torch.Tensor:
    """ResNeXt identity bottleneck: residual_block with the grouped 3x3 in the middle.  x [N][H][W][C4] -> same shape;
    w1 [C4][Cm], w3 [Cm][C4]; wg from filter_pack_grouped (Cm channels in `groups` groups); bnX = (bias, scale)."""
    return _bottleneck("wino_grouped_residual_block_hw", x, w1, bn1, "wg", wg, bn2, w3, bn3, out, workspace,
                       groups=groups)


def grouped_proj_block_workspace_bytes(N: int, Hin: int, Win: int, Cm: int, stride: int) -> int:
    """The workspace of grouped_proj_block: its intermediates are the dense projection blocks', so are the sizes."""
    if int(stride) == 1:
        return lib().wino_proj_block_workspace_bytes_hw(N, Hin, Win, Cm)
    return lib().wino_proj_block_v15_workspace_bytes_hw(N, Hin, Win, Cm)


def grouped_proj_block_prepare(N: int, Hin: int, Win: int, Cin: int, Cm: int, C4: int, groups: int, stride: int) -> None:
    """Allocate the scratch of grouped_proj_block's two 1x1 launches for the current stream (before graph capture)."""
    _prepare("wino_grouped_proj_block_prepare_hw", N, Hin, Win, Cin, Cm, C4, groups, stride)


def grouped_proj_block(x, w1, bn1, wg, bn2, tail, groups: int, stride: int, out=None, workspace=None) -> torch.Tensor:
    """ResNeXt projection bottleneck (a stage's first block, torchvision's placement): x [N][Hin][Win][Cin] ->
    [N][H][W][C4], H = (Hin-1)//stride + 1.  The first 1x1 runs at Hin x Win, the grouped 3x3 at `stride`; w1 [Cin][Cm];
    wg from filter_pack_grouped; tail from proj_tail_pack (w3, bn3, wp, bnp); bnX = (bias, scale)."""
    return _bottleneck("wino_grouped_proj_block_hw", x, w1, bn1, "wg", wg, bn2, tail, None, out, workspace, stride,
                       groups)


def conv3x3_bn_add_relu(inp: torch.Tensor, U: torch.Tensor, bn_bias: torch.Tensor, bn_scale: torch.Tensor,
                        residual: torch.Tensor, relu: bool = True, out: torch.Tensor | None = None) -> torch.Tensor:
    """out = act(bn_scale * conv3x3(inp, U) + bn_bias + residual): the second 3x3 of a ResNet basic block, one HIP
    launch.  inp [N][H+2][W+2][C]; residual and out [N][H+2][W+2][K] (out's ring written 0, residual's ring not read).
    out may be residual itself (in place); the ReLU follows the add."""
    x, U, b, s, N, Hp, Wp, C, K = _operands_3x3(inp, U, bn_bias, bn_scale)
    r = _out(residual, (N, Hp, Wp, K), "residual")
    out = _output(out, (N, Hp, Wp, K), x.device)
    _on_current_device(x, U, b, s, r, out)
    _check(lib().wino_conv3x3_bn_add_relu_hw(x.data_ptr(), U.data_ptr(), b.data_ptr(), s.data_ptr(), r.data_ptr(),
                                             out.data_ptr(), N, Hp - 2, Wp - 2, C, K, int(relu), _stream()),
           "wino_conv3x3_bn_add_relu_hw")
    return out


def basic_block_prepare(N: int, H: int, W: int, C: int) -> None:
    """Allocate the scratch of basic_block's two launches for the current stream (before graph capture)."""
    _prepare("wino_basic_block_prepare_hw", N, H, W, C)


def basic_block(x, U1, bn1, U2, bn2, out=None, workspace=None) -> torch.Tensor:
    """ResNet basic block (ResNet-18 / -34), identity shortcut: out = relu(bn2(conv3x3(relu(bn1(conv3x3(x, U1))), U2))
    + x).  x [N][H+2][W+2][C] with a zero ring -> out, the same layout (its ring written 0: the next block's x).
    U1, U2 from filter_transform_f2 (C -> C); bnX = (bias, scale) folded BN vectors.  Two HIP launches; out may be x
    (in place)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] < 3 or x.shape[2] < 3:
        raise WinoError("x must be [N][H+2][W+2][C]")
    N, Hp, Wp, C = (int(v) for v in x.shape)
    for name, u in (("U1", U1), ("U2", U2)):   # (shape first: a C -> K filter is refused before any device check)
        if not isinstance(u, torch.Tensor) or u.numel() != 16 * C * C:
            raise WinoError(f"{name} must be a {C} -> {C} filter from filter_transform_f2 (16*C*C values): "
                            "the basic block keeps its channel count")
    x, U1, U2 = _dev(x, "x"), _dev(U1, "U1"), _dev(U2, "U2")
    vecs = _bn_vecs(bn1, bn2)
    if any(v.numel() != C for v in vecs):
        raise WinoError("bn1 / bn2 vectors must have C values")
    workspace = _workspace(workspace, lib().wino_basic_block_workspace_bytes_hw(N, Hp - 2, Wp - 2, C), x.device)
    out = _output(out, (N, Hp, Wp, C), x.device)
    _on_current_device(x, U1, U2, out, workspace, *vecs)
    _check(lib().wino_basic_block_hw(x.data_ptr(), U1.data_ptr(), vecs[0].data_ptr(), vecs[1].data_ptr(),
                                     U2.data_ptr(), vecs[2].data_ptr(), vecs[3].data_ptr(), out.data_ptr(),
                                     N, Hp - 2, Wp - 2, C, *_ws_args(workspace), _stream()),
           "wino_basic_block_hw")
    return out


def s2_proj_pack(w_taps, bn1, wd, bnd, out=None) -> torch.Tensor:
    """The downsampling basic block's first layer: w_taps [3][3][C][K] (filter_pack_s2), its BN bn1 = (bias, scale),
    the shortcut wd [C][K] (torch's [K][C][1][1] weight as w.view(K, C).t()) and its BN bnd = (bias, scale), packed
    into one opaque buffer (wino_s2_proj_pack).  The scales are not folded into the filters."""
    w, wd = _dev(w_taps, "w_taps"), _dev(wd, "wd")
    if w.dim() != 4 or tuple(w.shape[:2]) != (3, 3):
        raise WinoError("w_taps must be [3][3][C][K]: pack it with filter_pack_s2")
    C, K = int(w.shape[2]), int(w.shape[3])
    if wd.dim() != 2 or tuple(wd.shape) != (C, K):
        raise WinoError(f"wd must be [{C}][{K}]")
    vecs = _bn_vecs(bn1, bnd)
    if any(v.numel() != K for v in vecs):
        raise WinoError("bn1 / bnd vectors must have K values")
    n = lib().wino_s2_proj_elems(C, K)
    if n == 0:
        raise WinoError(f"bad shape C={C} K={K}")
    packed = _output(out, (n,), w.device)
    _on_current_device(w, wd, packed, *vecs)
    _check(lib().wino_s2_proj_pack(w.data_ptr(), vecs[0].data_ptr(), vecs[1].data_ptr(), wd.data_ptr(),
                                   vecs[2].data_ptr(), vecs[3].data_ptr(), packed.data_ptr(), C, K, _stream()),
           "wino_s2_proj_pack")
    return packed


def _s2_proj_ck(x: torch.Tensor, packed: torch.Tensor):
    """(N, Hin, Win, C, K) of a padded x [N][Hin+2][Win+2][C] and a buffer from s2_proj_pack."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] < 3 or x.shape[2] < 3:
        raise WinoError("x must be [N][Hin+2][Win+2][C]")
    N, Hin, Win, C = int(x.shape[0]), int(x.shape[1]) - 2, int(x.shape[2]) - 2, int(x.shape[3])
    if not isinstance(packed, torch.Tensor) or packed.dim() != 1 or packed.numel() % (10 * C + 4):
        raise WinoError(f"packed does not match C={C}: pack it with s2_proj_pack")
    return N, Hin, Win, C, packed.numel() // (10 * C + 4)


def conv3x3_s2_proj(x, packed, t1=None, sc=None):
    """The downsampling basic block's first layer, one HIP launch: t1 = relu(bn1(conv3x3_s2(x))) and the shortcut
    sc = bnd(conv1x1_s2(x, wd)).  x [N][Hin+2][Win+2][C] with a zero ring; t1 and sc [N][H+2][W+2][K],
    H = (Hin-1)//2 + 1: t1 exactly as conv3x3_s2_bn_relu writes it (ring 0), sc's interior written and its ring not
    touched.  packed from s2_proj_pack.  Returns (t1, sc)."""
    N, Hin, Win, C, K = _s2_proj_ck(x, packed)
    x, packed = _dev(x, "x"), _dev(packed, "packed")
    H, W = _out_hw(Hin, Win, 2)
    shape = (N, H + 2, W + 2, K)
    t1 = _output(t1, shape, x.device, "t1")
    sc = _output(sc, shape, x.device, "sc")
    _on_current_device(x, packed, t1, sc)
    _check(lib().wino_conv3x3_s2_proj_bn_relu_hw(x.data_ptr(), packed.data_ptr(), t1.data_ptr(), sc.data_ptr(), N, Hin,
                                                 Win, C, K, _stream()), "wino_conv3x3_s2_proj_bn_relu_hw")
    return t1, sc


def basic_block_s2_prepare(N: int, Hin: int, Win: int, C: int, K: int) -> None:
    """Allocate the scratch of basic_block_s2's two launches for the current stream (before graph capture)."""
    _prepare("wino_basic_block_s2_prepare_hw", N, Hin, Win, C, K)


def basic_block_s2(x, packed, U2, bn2, out=None, workspace=None) -> torch.Tensor:
    """ResNet-18 / -34 downsampling basic block (torchvision's BasicBlock with `downsample`): out =
    relu(bn2(conv3x3(relu(bn1(conv3x3_s2(x))), U2)) + bnd(conv1x1_s2(x, wd))).  x [N][Hin+2][Win+2][C] with a zero
    ring -> out [N][H+2][W+2][K], H = (Hin-1)//2 + 1, its ring written 0 (the next identity basic_block's x).
    packed from s2_proj_pack (w_taps, bn1, wd, bnd); U2 from filter_transform_f2 (K -> K); bn2 = (bias, scale).
    Two HIP launches."""
    N, Hin, Win, C, K = _s2_proj_ck(x, packed)
    if not isinstance(U2, torch.Tensor) or U2.numel() != 16 * K * K:
        raise WinoError(f"U2 must be a {K} -> {K} filter from filter_transform_f2 (16*K*K values)")
    x, packed, U2 = _dev(x, "x"), _dev(packed, "packed"), _dev(U2, "U2")
    vecs = _bn_vecs(bn2)
    if len(vecs) != 2 or any(v.numel() != K for v in vecs):
        raise WinoError("bn2 must be (bias, scale) with K values each")
    H, W = _out_hw(Hin, Win, 2)
    workspace = _workspace(workspace, lib().wino_basic_block_s2_workspace_bytes_hw(N, Hin, Win, K), x.device)
    out = _output(out, (N, H + 2, W + 2, K), x.device)
    _on_current_device(x, packed, U2, out, workspace, *vecs)
    _check(lib().wino_basic_block_s2_hw(x.data_ptr(), packed.data_ptr(), U2.data_ptr(), vecs[0].data_ptr(),
                                        vecs[1].data_ptr(), out.data_ptr(), N, Hin, Win, C, K, *_ws_args(workspace),
                                        _stream()), "wino_basic_block_s2_hw")
    return out


STEM_FORM_BIG, STEM_FORM_SMALL = 1, 2   # WINO_STEM_FORM_*


def stem_out_hw(H: int, W: int):
    """The stem's pooled grid: conv 7x7 stride 2 pad 3, then max-pool 3x3 stride 2 pad 1 (224 -> 112 -> 56)."""
    return _out_hw(*_out_hw(int(H), int(W), 2), 2)


def stem_filter_pack(w, bn, out=None) -> torch.Tensor:
    """The stem's conv filter, torch's w [K][3][7][7], and its BN bn = (bias, scale) packed into one opaque buffer
    (wino_stem_filter_pack).  The scale is not folded into the filter."""
    w = _dev(w, "w")
    if w.dim() != 4 or tuple(w.shape[1:]) != (3, 7, 7):
        raise WinoError("w must be [K][3][7][7]")
    K = int(w.shape[0])
    vecs = _bn_vecs(bn)
    if len(vecs) != 2 or any(v.numel() != K for v in vecs):
        raise WinoError("bn must be (bias, scale) with K values each")
    n = lib().wino_stem_filter_elems(K)
    if n == 0:
        raise WinoError(f"stem: unsupported K={K} (need K % 64 == 0)")
    packed = _output(out, (n,), w.device)
    _on_current_device(w, packed, *vecs)
    _check(lib().wino_stem_filter_pack(w.data_ptr(), vecs[0].data_ptr(), vecs[1].data_ptr(), packed.data_ptr(), K,
                                       _stream()), "wino_stem_filter_pack")
    return packed


def stem_plan(N: int, H: int, W: int, K: int = 64, cus: int = 256) -> int:
    """The STEM_FORM_* the stem takes for this shape on a device with `cus` CUs (host-side)."""
    return _plan_query("wino_stem_plan", 1, int(N), int(H), int(W), int(K), int(cus))[0]


def stem(x, packed, out_padded: bool = False, out=None) -> torch.Tensor:
    """ResNet stem, one HIP launch: maxpool3x3_s2_p1(relu(bn(conv7x7_s2_p3(x)))).  x [N][3][H][W] (NCHW) ->
    out [N][Hp][Wp][K] (channels-last; proj_block's and residual_block's x) or, out_padded, [N][Hp+2][Wp+2][K] with a
    zero ring (basic_block's x).  packed from stem_filter_pack."""
    x, packed = _dev(x, "x"), _dev(packed, "packed")
    if x.dim() != 4 or int(x.shape[1]) != 3:
        raise WinoError("x must be [N][3][H][W]")
    N, H, W = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
    if packed.dim() != 1 or packed.numel() % 150:
        raise WinoError("packed does not hold a stem filter: pack it with stem_filter_pack")
    K = packed.numel() // 150
    Hp, Wp = stem_out_hw(H, W)
    p = 2 if out_padded else 0
    shape = (N, Hp + p, Wp + p, K)
    out = _output(out, shape, x.device)
    _on_current_device(x, packed, out)
    _check(lib().wino_stem_hw(x.data_ptr(), packed.data_ptr(), out.data_ptr(), N, H, W, K, int(bool(out_padded)),
                              _stream()), "wino_stem_hw")
    return out


def head_pack(wfc, bfc, out=None) -> torch.Tensor:
    """The classifier head's FC layer, torch's weight [classes][C] and bias [classes], packed into one opaque buffer
    (wino_head_pack; the class count padded to a multiple of 64 inside)."""
    w, b = _dev(wfc, "wfc"), _dev(bfc, "bfc")
    if w.dim() != 2 or b.dim() != 1 or int(b.shape[0]) != int(w.shape[0]):
        raise WinoError("wfc must be [classes][C], bfc [classes]")
    classes, C = int(w.shape[0]), int(w.shape[1])
    n = lib().wino_head_elems(C, classes)
    if n == 0:
        raise WinoError(f"head: unsupported C={C} classes={classes} (need C % 32 == 0)")
    packed = _output(out, (n,), w.device)
    _on_current_device(w, b, packed)
    _check(lib().wino_head_pack(w.data_ptr(), b.data_ptr(), packed.data_ptr(), C, classes, _stream()), "wino_head_pack")
    return packed


def head_prepare(N: int, C: int, classes: int) -> None:
    """Allocate the head GEMM's stream-K scratch for the current stream (before graph capture)."""
    _prepare("wino_head_prepare", N, C, classes)


def avgpool_fc(feat, packed, classes: int, in_padded: bool = False, out=None, workspace=None) -> torch.Tensor:
    """Classifier head: logits [N][classes] = mean_hw(feat) . Wfc^T + b.  feat [N][H][W][C] or, in_padded,
    [N][H+2][W+2][C] (the ring is not read); packed from head_pack(Wfc, b) with the same `classes`."""
    f, packed = _dev(feat, "feat"), _dev(packed, "packed")
    if f.dim() != 4:
        raise WinoError("feat must be [N][H][W][C]")
    p = 2 if in_padded else 0
    N, H, W, C = int(f.shape[0]), int(f.shape[1]) - p, int(f.shape[2]) - p, int(f.shape[3])
    if H < 1 or W < 1:
        raise WinoError("feat has no interior")
    classes = int(classes)
    n = lib().wino_head_elems(C, classes)
    if n == 0 or packed.numel() != n:
        raise WinoError(f"packed does not match C={C} classes={classes}: pack it with head_pack")
    workspace = _workspace(workspace, lib().wino_head_workspace_bytes(N, C, classes), f.device)
    out = _output(out, (N, classes), f.device)
    _on_current_device(f, packed, out, workspace)
    _check(lib().wino_avgpool_fc_hw(f.data_ptr(), packed.data_ptr(), out.data_ptr(), N, H, W, C, classes,
                                    int(bool(in_padded)), *_ws_args(workspace), _stream()),
           "wino_avgpool_fc_hw")
    return out


def conv3x3_bn_relu_pool(inp: torch.Tensor, U: torch.Tensor, bn_bias: torch.Tensor, bn_scale: torch.Tensor,
                         relu: bool = True, out: torch.Tensor | None = None) -> torch.Tensor:
    """The 3x3 layer with MaxPool2d(2, 2) fused into its epilogue, one HIP launch: inp [N][H+2][W+2][C] ->
    out [N][H//2+2][W//2+2][K] = maxpool2x2_s2(act(scale*conv3x3(inp) + bias)) with a zero ring.  The launch takes the
    plan of conv3x3_bn_relu at the same shape (conv3x3_prepare reserves its scratch).  H, W >= 2."""
    x, U, b, s, N, Hp, Wp, C, K = _operands_3x3(inp, U, bn_bias, bn_scale, 4,
                                                "inp must be [N][H+2][W+2][C] with H, W >= 2")
    H, W = Hp - 2, Wp - 2
    out = _output(out, (N, H // 2 + 2, W // 2 + 2, K), x.device)
    _on_current_device(x, U, b, s, out)
    _check(lib().wino_conv3x3_bn_relu_pool_hw(x.data_ptr(), U.data_ptr(), b.data_ptr(), s.data_ptr(), out.data_ptr(),
                                              N, H, W, C, K, int(relu), _stream()), "wino_conv3x3_bn_relu_pool_hw")
    return out


def image_pack(x, Cpad: int = 16, out=None) -> torch.Tensor:
    """x [N][Cin][H][W] (NCHW) -> out [N][H+2][W+2][Cpad]: the first 3x3 layer's input, channels Cin .. Cpad-1 and the
    ring written 0.  1 <= Cin <= Cpad, Cpad % 8 == 0.  One HIP launch."""
    x = _dev(x, "x")
    if x.dim() != 4:
        raise WinoError("x must be [N][Cin][H][W]")
    N, Cin, H, W = (int(v) for v in x.shape)
    Cpad = int(Cpad)
    out = _output(out, (N, H + 2, W + 2, Cpad), x.device)
    _on_current_device(x, out)
    _check(lib().wino_image_pack_hw(x.data_ptr(), out.data_ptr(), N, Cin, H, W, Cpad, _stream()), "wino_image_pack_hw")
    return out


def avgpool7_flatten(feat, in_padded: bool = False, out=None) -> torch.Tensor:
    """torch's AdaptiveAvgPool2d((7, 7)) + flatten, channels innermost: feat [N][H][W][C] or, in_padded,
    [N][H+2][W+2][C] (the ring is not read) -> out [N][49*C] in (h, w, c) order.  C % 4 == 0.  One HIP launch."""
    f = _dev(feat, "feat")
    if f.dim() != 4:
        raise WinoError("feat must be [N][H][W][C]")
    p = 2 if in_padded else 0
    N, H, W, C = int(f.shape[0]), int(f.shape[1]) - p, int(f.shape[2]) - p, int(f.shape[3])
    if H < 1 or W < 1:
        raise WinoError("feat has no interior")
    out = _output(out, (N, 49 * C), f.device)
    _on_current_device(f, out)
    _check(lib().wino_avgpool7_flatten_hw(f.data_ptr(), out.data_ptr(), N, H, W, C, int(bool(in_padded)), _stream()),
           "wino_avgpool7_flatten_hw")
    return out


def fpn_level_prepare(N: int, H: int, W: int, Cin: int, Cf: int) -> None:
    """Allocate the scratch of fpn_level's two launches for the current stream (before graph capture)."""
    _prepare("wino_fpn_level_prepare_hw", N, H, W, Cin, Cf)


def fpn_level(c, w_lat, b_lat, U_out, b_out, top=None, c_padded: bool = False, ones=None, inner=None, out=None):
    """One level of a Feature Pyramid Network, two HIP launches: inner = conv1x1(c, w_lat) + b_lat
    [+ nearest_upsample(top)], P = conv3x3(inner, U_out) + b_out.  c [N][H][W][Cin], or [N][H+2][W+2][Cin] with
    c_padded (ResNet-18 / -34's stage outputs); w_lat [Cin][Cf]; U_out from filter_transform_f2 (Cf -> Cf); top: the
    coarser level's inner, padded [N][(H+1)//2+2][(W+1)//2+2][Cf], or None on the coarsest level; ones: a vector of Cf
    ones (made here when left out: keep one when capturing).  Returns (inner, P), both padded [N][H+2][W+2][Cf] with
    zero rings."""
    c, w_lat, U_out = _dev(c, "c"), _dev(w_lat, "w_lat"), _dev(U_out, "U_out")
    b_lat, b_out = _dev(b_lat, "b_lat"), _dev(b_out, "b_out")
    p = 2 if c_padded else 0
    if c.dim() != 4 or c.shape[1] <= p or c.shape[2] <= p:
        raise WinoError("c must be [N][H+2][W+2][Cin]" if c_padded else "c must be [N][H][W][Cin]")
    N, H, W, Cin = int(c.shape[0]), int(c.shape[1]) - p, int(c.shape[2]) - p, int(c.shape[3])
    if w_lat.dim() != 2 or int(w_lat.shape[0]) != Cin:
        raise WinoError("w_lat must be [Cin][Cf]")
    Cf = int(w_lat.shape[1])
    if U_out.numel() != 16 * Cf * Cf:
        raise WinoError(f"U_out must be a {Cf} -> {Cf} filter from filter_transform_f2 (16*Cf*Cf values)")
    if b_lat.numel() != Cf or b_out.numel() != Cf:
        raise WinoError("b_lat / b_out must have Cf values")
    ones = torch.ones(Cf, dtype=torch.float32, device=c.device) if ones is None else _dev(ones, "ones")
    if ones.numel() != Cf:
        raise WinoError("ones must have Cf values")
    if top is not None:
        Hc, Wc = _up_hw(H, W)
        top = _out(top, (N, Hc + 2, Wc + 2, Cf), "top")
    inner = _output(inner, (N, H + 2, W + 2, Cf), c.device, "inner")
    out = _output(out, (N, H + 2, W + 2, Cf), c.device)
    _on_current_device(c, w_lat, b_lat, U_out, b_out, ones, top, inner, out)
    _check(lib().wino_fpn_level_hw(c.data_ptr(), w_lat.data_ptr(), b_lat.data_ptr(), ones.data_ptr(),
                                   top.data_ptr() if top is not None else None, inner.data_ptr(), U_out.data_ptr(),
                                   b_out.data_ptr(), ones.data_ptr(), out.data_ptr(), N, H, W, Cin, Cf,
                                   int(bool(c_padded)), _stream()), "wino_fpn_level_hw")
    return inner, out


def conv1x1_direct(A, B, bn_bias, bn_scale, relu: bool, out=None) -> torch.Tensor:
    a, bm = _dev(A, "A"), _dev(B, "B")
    b, s = _dev(bn_bias, "bn_bias"), _dev(bn_scale, "bn_scale")
    M, Cin, Kout = int(a.shape[0]), int(a.shape[1]), int(bm.shape[1])
    out = _output(out, (M, Kout), a.device)
    _check(lib().wino_conv1x1_direct(a.data_ptr(), bm.data_ptr(), b.data_ptr(), s.data_ptr(),
                                     out.data_ptr(), M, Cin, Kout, int(relu), _stream()),
           "wino_conv1x1_direct")
    return out


# ---------------------------------------------------------------- batch split (multi-GPU)
def shard_range(N: int, rank: int, world: int) -> tuple[int, int]:
    """Contiguous image range [n0, n1) of `rank` when N images are split over `world` GPUs.
    The path has no exchange step: every image is independent, weights are replicated, so
    there is no collective on the data path."""
    if world < 1 or not (0 <= rank < world):
        raise ValueError("bad rank/world")
    return (N * rank) // world, (N * (rank + 1)) // world


from .resnet import ResNet  # noqa: E402  (whole networks on the operators above)
from .vgg import VGG  # noqa: E402
from .fpn import ResNetFPN  # noqa: E402
from .segmentation import FCN, DeepLabV3  # noqa: E402
from .detection import BoxHead, MaskHead, KeypointHead, RPN, FasterRCNN, MaskRCNN, KeypointRCNN  # noqa: E402
from .detection import RetinaNetHead, RetinaNet  # noqa: E402
from .detection import FCOSHead, FCOS  # noqa: E402
