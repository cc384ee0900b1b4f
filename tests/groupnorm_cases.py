"""GroupNorm's fp64 reference, its case classes and its guarded-arena run, shared by tests/test_fcos_host.py,
tests/test_gpu_groupnorm.py and tests/test_gpu_groupnorm_large.py.  Nothing here needs a GPU to import.

The cases (interior [N][h][w][C] float32, gamma [C], beta [C]):
  plain     zero-mean unit-variance values
  offset    every (image, group) sample is standardised and moved to a mean of 64 of its standard deviations (sign by
            group): E[x^2] - E[x]^2 in fp32 is off by 1.8e-4 to 5.4e-4 in the tests' metric here, centred fp32 arithmetic
            by less than 1e-5 (tests/test_fcos_host.py measures both); TIGHT = 2e-5 lies between
  scales    groups of magnitude 1e-3 next to groups of 1e3: a group-index slip normalises with the wrong statistics
  constant  group 0 of every image is all 0.5: variance exactly 0, so the output there is relu(beta)
  gamma0    gamma is zero: the output is relu(beta) everywhere
"""
import functools

import numpy as np

KINDS = ("plain", "offset", "scales", "constant", "gamma0")
MAPS = ((1, 1), (1, 2), (2, 3), (7, 11), (13, 21), (37, 29))
CHANNELS = (64, 128, 256)
EPS = 1e-5
FORMS = ("whole", "split")


def cpgs(C):
    return (1, 2, 4, 8, 16, C)


def reference(x, gamma, beta, G, eps=EPS, relu=True):
    """torch's F.group_norm (+ ReLU) in fp64 on an NHWC interior [N][h][w][C]; NaN and Inf behave as in torch."""
    x = np.asarray(x, dtype=np.float64)
    N, h, w, C = x.shape
    g = x.reshape(N, h * w, G, C // G)
    with np.errstate(invalid="ignore", over="ignore"):
        mean = g.mean(axis=(1, 3), keepdims=True)
        var = ((g - mean) ** 2).mean(axis=(1, 3), keepdims=True)
        y = ((g - mean) / np.sqrt(var + eps)).reshape(N, h, w, C) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
        if relu:
            y = np.where(y < 0, 0.0, y)          # NaN fails the compare and stays
    return y


def rel_err(got, want):
    """The project's metric: max |got - want| / max |want|."""
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


@functools.lru_cache(maxsize=None)
def case(kind, N, h, w, C, G, seed=0):
    """(x [N][h][w][C], gamma [C], beta [C]) float32 of a case class."""
    rng = np.random.RandomState(1000 * seed + 7 * C + G + 31 * h + w)
    cpg = C // G
    x = rng.standard_normal((N, h, w, C))
    gamma = rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)
    beta = rng.uniform(-1.0, 1.0, C)
    group = np.arange(C) // cpg
    if kind == "offset":
        # 64 of the group's OWN standard deviations: every (image, group) sample is standardised first, since a group of
        # two or six values drawn from N(0, 1) can have a deviation of 0.01, and its mean near 64 is then thousands of
        # deviations away, where the fp32 ulp of the mean itself (3.8e-6) is all the error there is
        g = x.reshape(N, h * w, G, cpg)
        if h * w * cpg > 1:
            g = (g - g.mean(axis=(1, 3), keepdims=True)) / g.std(axis=(1, 3), keepdims=True)
        x = g.reshape(N, h, w, C) + 64.0 * np.where(group % 2 == 0, 1.0, -1.0)
    elif kind == "scales":
        x = x * np.where(group % 2 == 0, 1e-3, 1e3)
    elif kind == "constant":
        x[..., group == 0] = 0.5
    elif kind == "gamma0":
        gamma = np.zeros(C)
    elif kind != "plain":
        raise KeyError(kind)
    return x.astype(np.float32), gamma.astype(np.float32), beta.astype(np.float32)


def padded(x, ring=np.nan):
    """[N][h][w][C] -> float32 [N][h+2][w+2][C] with `ring` around the interior."""
    N, h, w, C = x.shape
    m = np.full((N, h + 2, w + 2, C), ring, dtype=np.float32)
    m[:, 1:-1, 1:-1, :] = x
    return m


def ring_of(m):
    """The ring's words of a padded map, as int32."""
    mask = np.ones(m.shape[1:3], dtype=bool)
    mask[1:-1, 1:-1] = False
    return np.ascontiguousarray(m[:, mask, :]).view(np.int32)


def run_groupnorm(pkg, dev, x, gamma, beta, G, relu=True, in_place=False, eps=EPS, aligns=None, tag=""):
    """groupnorm_relu on the guarded arena at each of `aligns`, twice each into a NaN-filled output and workspace (in
    place: into a fresh copy of the input), all runs bitwise equal.  The input's ring holds NaN; the ring of the output
    keeps the bits it had.  The workspace is exactly what groupnorm_workspace_bytes reports.  Returns the interior
    [N][h][w][C] as numpy."""
    import torch

    import guarded
    N, h, w, C = x.shape
    master = torch.from_numpy(padded(x))
    need = pkg.groupnorm_workspace_bytes(N, h, w, C, G)
    first = None
    for align in (guarded.ALIGNS if aligns is None else aligns):
        arena = guarded.Arena(torch, dev, align)
        xt = arena.input(master, name="x", in_place=in_place)
        gt = arena.input(torch.from_numpy(gamma), name="gamma")
        bt = arena.input(torch.from_numpy(beta), name="beta")
        out = xt if in_place else arena.output(N, h + 2, w + 2, C, name="out")
        ws = arena.workspace(need, name="workspace", query="groupnorm_workspace_bytes") if need else None
        for _ in range(2):
            if in_place:
                xt.copy_(master)
            else:
                out.fill_(float("nan"))
            if ws is not None:
                ws.fill_(float("nan"))
            got = pkg.groupnorm_relu(xt, gt, bt, G, eps, relu, out=out, workspace=ws)
            assert got is out
            arena.check(f"groupnorm_relu {tag} align={align}")
            o = out.cpu().numpy()
            assert (ring_of(o) == np.int32(guarded.NAN_BITS)).all(), f"{tag}: the ring of out was written"
            cur = o[:, 1:-1, 1:-1, :].copy()
            if first is None:
                first = cur
            assert np.array_equal(cur.view(np.int32), first.view(np.int32)), f"{tag}: not bitwise reproducible (align {align})"
    return first


SWEEP_COUNT = 24


@functools.lru_cache(maxsize=None)
def sweep_specs():
    """SWEEP_COUNT seeded legal layouts: N 1..3, h x w up to 40 x 40, C a multiple of 64 up to 320 (so channel blocks
    that are not the whole of C), any legal cpg, a kind, a form or the planner's choice, ReLU and in-place coins."""
    rng = np.random.RandomState(20261)
    specs = []
    for index in range(SWEEP_COUNT):
        C = 64 * int(rng.randint(1, 6))
        pow2 = C & -C
        cpg = int(rng.choice([1 << s for s in range(pow2.bit_length())]))
        specs.append(dict(index=index, N=int(rng.randint(1, 4)), h=int(rng.randint(1, 41)), w=int(rng.randint(1, 41)), C=C,
                          G=C // cpg, kind=KINDS[rng.randint(len(KINDS))], form=(None, "whole", "split")[rng.randint(3)],
                          relu=bool(rng.randint(2)), in_place=bool(rng.randint(2))))
    return specs
