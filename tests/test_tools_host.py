"""tools/benchlib.py and tools/torch_nets.py on the CPU: the torch comparator every "against torch" figure in profiles/
is a ratio to computes the networks the test suite's fp64 references compute, the interleaved-trials loop keeps the
setups out of the timed windows, and every tool parses its documented command lines without importing another tool.

The comparator runs on the CPU with the tools' own state dicts (seed 1) at a [2][3][64][64] input (seed 2); the figure
is max |got - want| / max |want|.  The bar is 1e-5: about 15 times the fp32 rounding of the ResNets below, a hundred
times tighter than NET_TOL, and far below any structural error (a wrong stride, a missing ReLU or a swapped BN shows
at 1e-1).  Measured with the comparator classes the tools had before this module:
  resnet18 3.2e-7, resnet50 5.5e-7, resnext50_32x4d 4.9e-7, wide_resnet50_2 6.7e-7,
  fcn_resnet50 2.3e-6, deeplabv3_resnet50 1.2e-6, resnet50-fpn 2.1e-6 / 1.9e-6 / 1.7e-6 / 1.2e-6 / 1.4e-6 (levels 0..3
  and the pool), vgg16 (at [1][3][64][64]) 1.4e-6.
The last four are above 1e-6 -- their fp32 sums are longer (2048 x 9 terms in the heads, 25088 in VGG's first fc) -- so
each of them is held to ten times its own figure instead."""
import importlib
import os
import re
import sys

import pytest
import torch

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)
import benchlib  # noqa: E402
import torch_nets  # noqa: E402

import deeplab_reference  # noqa: E402
import fpn_reference  # noqa: E402
import reference_nets  # noqa: E402
import segmentation_reference  # noqa: E402

BAR = 1e-5
TOOL_NAMES = sorted(f[:-3] for f in os.listdir(TOOLS) if f.endswith("_bench.py"))
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def R(pkg):
    return importlib.import_module("cuda_winograd_amd.resnet")


@pytest.fixture(scope="module")
def x():
    return torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(2)) * 2 - 1


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _err(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


def _check(name, err, bar):
    print(f"{name}: {err:.2e} (bar {bar:.1e})")
    assert err < bar, f"{name}: {err:.2e}"


# ---- the comparator against the fp64 references ----------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ["resnet18", "resnet50", "resnext50_32x4d", "wide_resnet50_2"])
def test_classifier_matches_reference(R, x, arch):
    sd = torch_nets.random_state_dict(R, arch, seed=1)
    body = torch_nets.TorchResNetBody(R, sd, arch, CPU)
    want, _ = reference_nets.reference_forward(torch, sd, x)
    _check(arch, _err(torch_nets.classifier_head(body, body(_cl(x))), want), BAR)


def test_fcn_matches_reference(R, x):
    sd = torch_nets.fcn_state_dict(R, "resnet50", seed=1)
    body = torch_nets.TorchResNetBody(R, sd, "resnet50", CPU, prefix="backbone.", dilate=(False, True, True))
    want = segmentation_reference.fcn_reference_forward(torch, sd, x)
    _check("fcn_resnet50", _err(torch_nets.fcn_head(body, body(_cl(x)), x.shape[-2:]), want), 10 * 2.30e-6)


def test_deeplab_matches_reference(R, x):
    sd = torch_nets.deeplab_state_dict(R, "resnet50", seed=1)
    body = torch_nets.TorchResNetBody(R, sd, "resnet50", CPU, prefix="backbone.", dilate=(False, True, True))
    want = deeplab_reference.deeplab_reference_forward(torch, sd, x)
    _check("deeplabv3_resnet50", _err(torch_nets.deeplab_head(body, body(_cl(x)), x.shape[-2:]), want), 10 * 1.16e-6)


def test_fpn_matches_reference(R, x):
    sd, plain = torch_nets.fpn_state_dict(R, "resnet50", seed=1)
    body = torch_nets.TorchResNetBody(R, sd, "resnet50", CPU, prefix="body.")
    got = torch_nets.fpn_head(body, body(_cl(x)))
    want = fpn_reference.fpn_reference_forward(torch, sd, plain, x)
    before = {"0": 2.09e-6, "1": 1.86e-6, "2": 1.72e-6, "3": 1.17e-6, "pool": 1.36e-6}
    assert len(got) == len(want) == 5
    for level, g in zip(before, got):
        _check(f"resnet50-fpn level {level}", _err(g, want[level].permute(0, 3, 1, 2)), 10 * before[level])


def test_vgg_matches_reference(pkg, x):
    V = importlib.import_module("cuda_winograd_amd.vgg")
    sd = torch_nets.vgg_state_dict(V, "vgg16", torch.Generator().manual_seed(16))   # the seed vgg_bench draws it with
    want, _ = reference_nets.vgg_reference_forward(torch, V, sd, "vgg16", x[:1])
    _check("vgg16", _err(torch_nets.torch_vgg(sd, V, "vgg16", CPU)(_cl(x[:1])), want), 10 * 1.44e-6)


# ---- the interleaved-trials loop -------------------------------------------------------------------------------------------
def test_interleaved_keeps_setups_outside_the_timed_window(monkeypatch):
    log, clock = [], iter(range(1, 1000))

    def fake_time_us(fn, reps):
        log.append("window open")
        for _ in range(reps):
            fn()
        log.append("window shut")
        return float(next(clock))

    monkeypatch.setattr(benchlib, "time_us", fake_time_us)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)
    variants = {k: (lambda k=k: log.append("run " + k)) for k in ("a", "b")}
    setups = {"a": lambda: log.append("setup a")}
    trials, reps = 5, 2
    med, times = benchlib.interleaved(variants, trials, reps, setups, after={"b": lambda: log.append("after b")})
    warm_up = ["setup a"] + ["run a"] * 3 + ["run b"] * 3
    one_round = ["setup a", "window open", "run a", "run a", "window shut",
                 "window open", "run b", "run b", "window shut", "after b"]
    assert log == warm_up + one_round * trials
    assert times == {"a": [1.0, 3.0, 5.0, 7.0, 9.0], "b": [2.0, 4.0, 6.0, 8.0, 10.0]}
    assert med == {"a": 5.0, "b": 6.0}


# ---- every tool's command line ---------------------------------------------------------------------------------------------
def _documented_command_lines(name, doc):
    """[(mode or None, {option: default text})] off the usage lines of a tool's docstring:
    `python tools/<name>.py [mode] [out] [--option default] ...`, continued on lines that open with a bracket."""
    found, lines = [], doc.splitlines()
    for i, line in enumerate(lines):
        m = re.search(rf"python tools/{name}\.py( \w+)?( \S+\.json| \[)", line)
        if not m:
            continue
        text = line[m.start():]
        for more in lines[i + 1:]:
            if not more.strip().startswith("["):
                break
            text += " " + more.strip()
        found.append((m.group(1).strip() if m.group(1) else None, dict(re.findall(r"\[--(\w+) ([^\]\s]+)\]", text))))
    return found


@pytest.mark.parametrize("name", TOOL_NAMES)
def test_tool_parses_its_documented_command_lines(name, capsys):
    for other in [m for m in sys.modules if m.endswith("_bench")]:
        del sys.modules[other]
    tool = importlib.import_module(name)
    assert [m for m in sys.modules if m.endswith("_bench")] == [name], "a tool imports another tool"
    extra = getattr(tool, "EXTRA", ())
    with pytest.raises(SystemExit) as stop:
        benchlib.parse(tool.MODES, extra, ["--help"])
    assert stop.value.code == 0 and "--reps" in capsys.readouterr().out
    documented = _documented_command_lines(name, tool.__doc__)
    assert {mode for mode, _ in documented} == set(tool.MODES), "the usage text and the mode table name different modes"
    for mode, options in documented:
        a = benchlib.parse(tool.MODES, extra, [mode] if mode else [])
        assert a.mode == mode and a.out is None
        assert {k: str(getattr(a, k)) for k in options} == options, f"{name} {mode}: defaults differ from the usage text"
