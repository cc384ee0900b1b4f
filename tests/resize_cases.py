"""The bilinear resize tests' helper: the fp64 reference written from the layer's integer coordinate rule (per axis:
num = max((2d+1) in - out, 0), i0 = num // (2 out), i1 = min(i0 + 1, in - 1), lambda = (num - i0 2 out) / (2 out); value
(1-ly)((1-lx) a + lx b) + ly((1-lx) c + lx d), every tap multiplied), its labels, the gap rule the label tests share,
the shapes the host and the GPU tests both name, and a case class with seeded inputs and prefilled outputs.  Nothing
here needs a GPU to import."""
import numpy as np

STAGED, DIRECT = 1, 2

# (N, h, w, Ho, Wo, C, ld)
STAGED_SHAPES = [
    (2, 9, 9, 65, 65, 21, 64),
    (2, 7, 11, 49, 81, 21, 64),      # odd Wo: rows start off 16 bytes
    (3, 5, 3, 33, 49, 5, 8),
    (1, 9, 9, 9, 9, 4, 4),           # identity size: bitwise the input
    (1, 1, 1, 7, 3, 1, 4),
    (1, 12, 10, 5, 7, 64, 64),       # mild down-scale
]
DIRECT_SMALL = (2, 64, 48, 2, 3, 8, 8)   # strong down-scale
EXACT_WIDTHS = [(3001, 7919), (4099, 4100), (1031, 8209)]
WORKLOAD = (65, 65, 21, 64, 520, 520)    # h, w, C, ld, Ho, Wo


def smallest_direct_channels(pkg, h=6, w=6, Ho=13, Wo=11, limit=1 << 16):
    """The smallest C = ld, a multiple of 4, at which the plan answers DIRECT for (h, w) -> (Ho, Wo): read off the plan,
    never guessed."""
    for C in range(4, limit, 4):
        if pkg.resize_bilinear_plan(h, w, C, C, Ho, Wo) == DIRECT:
            return C
    raise AssertionError("the plan never answers DIRECT")


def axis_coords(n_in, n_out, idx=None):
    """(i0, i1, lambda) of the outputs `idx` (default: all) of an axis, exact: int64 and float64 of an exact ratio."""
    d = np.arange(n_out, dtype=np.int64) if idx is None else np.asarray(idx, dtype=np.int64)
    num = np.maximum((2 * d + 1) * n_in - n_out, 0)
    i0 = num // (2 * n_out)
    i1 = np.minimum(i0 + 1, n_in - 1)
    lam = (num - i0 * 2 * n_out).astype(np.float64) / float(2 * n_out)
    return i0, i1, lam


def resize_reference(src, Ho, Wo, C=None, in_padded=False, rows=None):
    """fp64: src [N][h(+2)][w(+2)][ld] -> [N][C][Ho][Wo] (or, with `rows`, those output rows only)."""
    src = np.asarray(src)
    p = 1 if in_padded else 0
    h, w = src.shape[1] - 2 * p, src.shape[2] - 2 * p
    C = src.shape[3] if C is None else C
    x = src[:, p:p + h, p:p + w, :C].astype(np.float64).transpose(0, 3, 1, 2)
    y0, y1, ly = axis_coords(h, Ho, rows)
    x0, x1, lx = axis_coords(w, Wo)
    ly, lx = ly[:, None], lx[None, :]
    with np.errstate(invalid="ignore"):
        top = (1 - lx) * x[:, :, y0][:, :, :, x0] + lx * x[:, :, y0][:, :, :, x1]
        bot = (1 - lx) * x[:, :, y1][:, :, :, x0] + lx * x[:, :, y1][:, :, :, x1]
        return (1 - ly) * top + ly * bot


def labels_of(want):
    """argmax over the classes as torch.argmax gives it: the lowest index of the maximum, a NaN above everything and the
    first NaN winning (numpy's rule too)."""
    return np.argmax(want, axis=1).astype(np.int32)


def decided(want, gap):
    """The pixels [N][Ho][Wo] whose top two classes are at least `gap` apart in the reference (all, with one class)."""
    if want.shape[1] < 2:
        return np.ones(want.shape[:1] + want.shape[2:], bool)
    top = np.partition(want, -2, axis=1)[:, -2:]
    return (top[:, 1] - top[:, 0]) >= gap


def check_labels(got, want, tol, what=""):
    """The gap rule: labels equal the reference's on every pixel decided by tol * max|want|; at most 1 % are left out.
    Returns the share left out."""
    mask = decided(want, tol * np.abs(want).max())
    left = 1.0 - mask.mean()
    print(f"{what}: labels: {left:.4%} of the pixels left out by the gap rule")
    assert left <= 0.01, (what, left)
    ref = labels_of(want)
    bad = (np.asarray(got) != ref) & mask
    assert not bad.any(), (what, int(bad.sum()))
    return left


class ResizeCase:
    """One call's tensors: seeded src uniform in (-0.5, 0.5) in all ld columns (a NaN ring with in_padded), outputs
    prefilled with NaN / -1, the library's run and the fp64 reference."""

    def __init__(self, pkg, torch_dev, N, h, w, Ho, Wo, C, ld, seed=0, in_padded=False):
        self.torch, self.dev = torch_dev
        self.pkg = pkg
        torch = self.torch
        g = torch.Generator(device="cpu").manual_seed(seed)
        x = torch.rand(N, h, w, ld, generator=g) - 0.5
        if in_padded:
            full = torch.full((N, h + 2, w + 2, ld), float("nan"))
            full[:, 1:-1, 1:-1, :] = x
            x = full
        self.src = x
        self.N, self.h, self.w, self.Ho, self.Wo, self.C, self.ld, self.in_padded = N, h, w, Ho, Wo, C, ld, in_padded
        self._want = None

    def form(self):
        return self.pkg.resize_bilinear_plan(self.h, self.w, self.C, self.ld, self.Ho, self.Wo)

    def run(self, want_out=True, want_labels=False, src=None, out=None, labels=None):
        """(out, labels) as numpy arrays (None where not wanted), into prefilled tensors unless given."""
        torch = self.torch
        x = (self.src if src is None else src).to(self.dev)
        if want_out and out is None:
            out = torch.full((self.N, self.C, self.Ho, self.Wo), float("nan"), device=self.dev)
        if want_labels and labels is None:
            labels = torch.full((self.N, self.Ho, self.Wo), -1, dtype=torch.int32, device=self.dev)
        o, l = self.pkg.resize_bilinear(x, self.Ho, self.Wo, C=self.C, in_padded=self.in_padded, out=out, labels=labels,
                                        want_out=want_out, want_labels=want_labels)
        torch.cuda.synchronize()
        assert (o is None) == (not want_out) and (l is None) == (not want_labels)
        return (o.cpu().numpy() if want_out else None), (l.cpu().numpy() if want_labels else None)

    def reference(self, src=None):
        if src is not None:
            return resize_reference(src.numpy(), self.Ho, self.Wo, self.C, self.in_padded)
        if self._want is None:
            self._want = resize_reference(self.src.numpy(), self.Ho, self.Wo, self.C, self.in_padded)
            self._want.setflags(write=False)
        return self._want
