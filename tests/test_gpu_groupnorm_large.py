"""groupnorm_relu on one map past 4 GiB (N = 1, 2048 x 2048, C = 256: 4.3 GB, offsets past 2^32 bytes and a count of
2^25 values per group), in place.  The input is a_c + S * (+1 or -1 by the parity of y + x): a group's mean is the mean
of its channels' a_c and its variance var(a_c) + S^2 (up to the fp32 rounding of a_c +- S, 6e-8), so the expected output
of any row is a closed form.
Checked on sampled rows, the first and the last included; the ring holds NaN and keeps it."""
import numpy as np
import pytest
import torch

from cases import TIGHT
from gpu_support import torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu

H = W = 2048
C, G, S, EPS = 256, 32, 0.75, 1e-5
ROWS = (0, 1, 777, 1024, 2046, 2047)


def test_groupnorm_past_4_gib(pkg, torch_dev):
    _, dev = torch_dev
    rng = np.random.RandomState(5)
    a = rng.uniform(-2, 2, C).astype(np.float32)
    gamma = (rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    beta = rng.uniform(-1, 1, C).astype(np.float32)
    x = torch.full((1, H + 2, W + 2, C), float("nan"), device=dev)
    assert x.numel() * 4 > 1 << 32
    yy, xx = torch.arange(H, device=dev)[:, None], torch.arange(W, device=dev)[None, :]
    sign = (1.0 - 2.0 * ((yy + xx) % 2)).to(torch.float32)
    interior = x[0, 1:-1, 1:-1, :]
    interior.copy_(torch.from_numpy(a).to(dev)[None, None, :].expand(H, W, C))
    interior.add_(sign[:, :, None] * S)
    del sign
    form, chunks = pkg.groupnorm_plan(1, H, W, C, G, torch.cuda.get_device_properties(0).multi_processor_count)
    assert form == "split" and chunks > 1
    ws = torch.full((pkg.groupnorm_workspace_bytes(1, H, W, C, G) // 4,), float("nan"), device=dev)
    out = pkg.groupnorm_relu(x, torch.from_numpy(gamma).to(dev), torch.from_numpy(beta).to(dev), G, EPS, out=x, workspace=ws)
    torch.cuda.synchronize()
    assert out is x
    a64 = a.astype(np.float64).reshape(G, C // G)
    mean = np.repeat(a64.mean(axis=1), C // G)
    rstd = np.repeat(1.0 / np.sqrt(a64.var(axis=1) + S * S + EPS), C // G)
    worst = 0.0
    for y in ROWS:
        got = x[0, y + 1].cpu().numpy()
        assert np.isnan(got[0]).all() and np.isnan(got[-1]).all(), "the ring was written"
        sgn = 1.0 - 2.0 * ((y + np.arange(W)) % 2)
        val = (a.astype(np.float64)[None, :] + (S * sgn)[:, None]).astype(np.float32).astype(np.float64)
        want = np.maximum((val - mean) * rstd * gamma + beta, 0.0)
        worst = max(worst, np.abs(got[1:-1] - want).max() / np.abs(want).max())
    print(f"2048 x 2048 x 256 in place, {chunks} chunks: rel err {worst:.2e}")
    assert worst < TIGHT
    assert bool(torch.isnan(x[0, 0]).all()) and bool(torch.isnan(x[0, -1]).all())
