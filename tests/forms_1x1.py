"""The launch forms of the 1x1 kernels that the GPU tests force: the knob sets by name, the context manager that sets
and unsets them, the stream-K grid arithmetic of conv1x1.hip, and the question whether the plan takes a form for a GEMM.
Shared by tests/test_gpu_fpn.py and tests/test_gpu_nonfinite.py."""
import contextlib

import shape_sweeps as S

TILED = {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 0}
FORMS = {"auto": {}, "tiled": TILED}
FORMS.update({f"sk{g}": {"WINO_1X1_ALGO": "big", "WINO_1X1_SK": 1, "WINO_1X1_SK_GRID": g} for g in (8, 24)})
FORMS.update({f"latency_ks{ks}_rt{rt}_ct{ct}": {"WINO_1X1_ALGO": "small", "WINO_1X1_SMALL_KS": ks,
                                                 "WINO_1X1_SMALL_RT": rt, "WINO_1X1_SMALL_CT": ct}
              for ks in (1, 2, 4) for rt in (1, 2) for ct in (1, 2, 4)})


@contextlib.contextmanager
def knobs_set(knobs, kv):
    for k, v in (kv or {}).items():
        knobs.set(k, v)
    try:
        yield
    finally:
        for k in kv or {}:
            knobs.unset(k)


def sk_plan(M, Cin, Kout, grid):
    """(legal, cuts a tile) of the stream-K form with WINO_1X1_SK_GRID = grid, as sk1_grid in conv1x1.hip decides."""
    four = Kout <= 128 or Cin <= 128 or Kout % 128 != 0
    nblk, nk, nmb = Kout // (64 if four else 128), Cin // 32, (M + 111) // 112
    step = 8
    while step % nblk:
        step += 8
    g = min(grid, nmb * nblk * nk)
    g -= g % step
    if g < step:
        return False, False
    ranges, units = g // nblk, nmb * nk
    return True, any((units * r // ranges) % nk for r in range(1, ranges))


def takes(pkg, form, M, Cin, Kout):
    """Does the plan, under the knobs of `form` (set by the caller), take that form for this GEMM?  The forms a shape
    cannot take -- a K split its Cin does not divide, a grid with more ranges than k-steps -- are skipped by the
    caller; that each form runs somewhere is test_every_form_runs_somewhere's."""
    kv = FORMS[form]
    if form.startswith("latency"):
        use, ks, rt, ct, _ = pkg.small_plan_1x1_full(M, Cin, Kout, S.CUS)
        return bool(use) and (ks, rt, ct) == (kv["WINO_1X1_SMALL_KS"], kv["WINO_1X1_SMALL_RT"], kv["WINO_1X1_SMALL_CT"])
    planned = S.form_1x1(pkg, M, Cin, Kout)
    if form.startswith("sk"):
        legal, _ = sk_plan(M, Cin, Kout, kv["WINO_1X1_SK_GRID"])
        assert (planned == "stream_k") == legal, (form, M, Cin, Kout, planned)
        return legal
    if form == "tiled":
        assert planned == "tiled"
    return True
