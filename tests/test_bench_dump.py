"""bench.py --dump-outputs: the output of the last timed step as float32 .npy files, under a size cap,
identical from run to run; and --steps is the number of timed steps the result line reports."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import bench


def test_dump_outputs_writes_small_outputs_whole(tmp_path):
    t = torch.rand(3, 5, 7, generator=torch.Generator().manual_seed(0))
    info = bench.dump_outputs(str(tmp_path), {"out": t})
    a = np.load(tmp_path / "out.npy")
    assert a.dtype == np.float32 and np.array_equal(a, t.numpy())
    assert info["out"] == {"shape": [3, 5, 7], "full_shape": [3, 5, 7], "sample": None}


def test_dump_outputs_samples_large_outputs_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 3000)
    t = torch.arange(40 * 25, dtype=torch.float32).reshape(40, 25)   # 4000 bytes, rows of 100 bytes
    info = bench.dump_outputs(str(tmp_path / "a"), {"out": t})
    bench.dump_outputs(str(tmp_path / "b"), {"out": t})
    a, b = np.load(tmp_path / "a" / "out.npy"), np.load(tmp_path / "b" / "out.npy")
    assert a.shape == (30, 25) and a.nbytes <= 3000 and np.array_equal(a, b)
    rows = a[:, 0] / 25                                     # each kept row is a whole row of t, in order
    assert np.array_equal(a, t.numpy()[rows.astype(int)]) and (np.diff(rows) > 0).all()
    assert info["out"]["full_shape"] == [40, 25] and info["out"]["sample"].startswith("30 of 40")


def test_dump_cap_is_below_64_mb():
    assert bench.DUMP_BYTES + 4096 <= 64 * 10 ** 6


def _run_bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--warmup", "2", "--preheat-ms", "0",
           "--no-cpu-baseline", "--dump-outputs", str(out_dir)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_bench_dump_is_the_layer_output_and_repeats(tmp_path, O):
    """A small 3x3 layer: the dump is the conv + BN + ReLU of bench.py's seeded inputs (rebuilt here in the
    order bench.py draws them), two runs write the same bytes, and the line reports the steps asked for."""
    N, C, K = 2, 128, 128
    js = [_run_bench(tmp_path / f"d{i}", "--layer", "conv3x3_128", "--batch", str(N), "--steps", "7") for i in range(2)]
    for j in js:
        assert j["steps"] == 7 and j["trials"] == 1 and len(j["trials_us"]) == 1 and j["ms_per_step"] > 0
        assert j["dumped_outputs"]["arrays"]["out"]["sample"] is None
    a, b = np.load(tmp_path / "d0" / "out.npy"), np.load(tmp_path / "d1" / "out.npy")
    assert a.dtype == np.float32 and a.shape == (N, 16, 16, K) and np.array_equal(a, b)
    g = torch.Generator(device="cpu").manual_seed(1234)
    rnd = lambda *shape: ((torch.rand(*shape, generator=g) - 0.5)).numpy()
    scale, bias = rnd(K), rnd(K)
    x, w = rnd(N, 16, 16, C), rnd(K, C, 3, 3)
    assert O.rel_error(a, O.conv3x3_bn_relu_direct(x, w, scale, bias)) < 1e-3


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_bench_dump_of_a_large_output_is_a_capped_repeatable_sample(tmp_path):
    """The bottleneck block's output at N = 128 (103 MB) is cut to a seeded sample of images under the cap."""
    js = [_run_bench(tmp_path / f"d{i}", "--layer", "residual_block", "--steps", "3") for i in range(2)]
    info = js[0]["dumped_outputs"]["arrays"]["out"]
    assert info["full_shape"] == [128, 14, 14, 1024] and info["sample"] is not None
    a, b = np.load(tmp_path / "d0" / "out.npy"), np.load(tmp_path / "d1" / "out.npy")
    assert a.shape == tuple(info["shape"]) and a.nbytes <= bench.DUMP_BYTES and np.array_equal(a, b)
    assert np.isfinite(a).all() and (a != 0).any()
