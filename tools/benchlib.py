"""What the tools/*_bench.py developer tools share: the repository root on sys.path and the package loader, the one
event timer, the one interleaved-trials loop, the one graph-capture sequence, the eager / graph / torch variants of a
whole network with their three ratios, and the command line and JSON output of a tool.  A tool imports this module and
torch_nets and nothing else from tools/."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

load_package = ge.load_package
FLOP_PER_CLK = 256 * 4 * 64   # CUs x SIMDs x f32 MFMA FLOP per clock per SIMD
FORM_NAMES = {0: "tiled", 1: "stream_k", 2: "latency"}   # the 1x1 family's plan forms


def package_module(name):
    """cuda_winograd_amd.<name>, the package loaded first."""
    load_package()
    return importlib.import_module("cuda_winograd_amd." + name)


def tests_module(name):
    """tests/<name>.py: the test suite's own cases and references, for a tool that measures against them."""
    tests = os.path.join(ROOT, "tests")
    if tests not in sys.path:
        sys.path.insert(0, tests)
    return importlib.import_module(name)


def ints(csv):
    return [int(v) for v in csv.split(",")]


# ---- timing ------------------------------------------------------------------------------------------------------------
def time_us(fn, reps):
    """us per call: two events around `reps` calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def interleaved(variants, trials, reps, setups=None, preheat_s=0.0, after=None):
    """Warm every variant up, then `trials` rounds of every variant in turn: (median us per call of each, all times).
    The warm-up is three calls of each (plans, scratch, torch's algorithm choice), or with `preheat_s` that many seconds
    of rounds of five calls each.  setups[k] runs before variant k's warm-up and before each of its timed windows,
    after[k] after each of its windows: both outside the timed repetitions."""
    setups, after = setups or {}, after or {}
    nothing = lambda: None
    t0 = time.time()
    while True:
        for k, fn in variants.items():
            setups.get(k, nothing)()
            for _ in range(5 if preheat_s else 3):
                fn()
        torch.cuda.synchronize()
        if time.time() - t0 >= preheat_s:
            break
    times = {k: [] for k in variants}
    for _ in range(trials):
        for k, fn in variants.items():
            setups.get(k, nothing)()
            times[k].append(time_us(fn, reps))
            after.get(k, nothing)()
    return {k: statistics.median(v) for k, v in times.items()}, times


# ---- graphs ------------------------------------------------------------------------------------------------------------
def captured(fn, prepare=None):
    """fn as a CUDAGraph: on a side stream that waits for the current one, prepare() and one eager fn() (the library's
    scratch is per stream), then the capture.  Returns (graph, what the eager call returned)."""
    sg = torch.cuda.Stream()
    sg.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(sg):
        if prepare:
            prepare()
        first = fn()
    sg.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=sg):
        fn()
    torch.cuda.synchronize()
    return graph, first


def repeated(fn, reps):
    """`reps` calls of fn as one call: what a graph of `reps` launches captures."""
    def run():
        for _ in range(reps):
            fn()
    return run


def net_variants(model_call, graph, torch_call):
    """A whole network three ways: one Python call per block, one graph replay, torch eager."""
    return {"eager": model_call, "graph": graph.replay, "torch": torch_call}


def net_ratios(med):
    return {"graph_over_eager": med["graph"] / med["eager"], "graph_over_torch": med["graph"] / med["torch"],
            "eager_over_torch": med["eager"] / med["torch"]}


# ---- command line and output ---------------------------------------------------------------------------------------------
def parse(modes, extra=(), argv=None):
    """The command line of a tool: [mode] [out] and one --option per key of the mode tables.  modes: {mode: {"fn": ...,
    option: default, ...}}, or {None: {...}} for a tool without modes; an option left out takes its mode's default (and
    stays None in a mode whose table does not name it), its type is its defaults' type.  A mode whose table is a list
    of other modes ("all") runs those, each with its own defaults: see sections.  extra: (flag, add_argument keywords)
    pairs."""
    ap = argparse.ArgumentParser()
    if None not in modes:
        ap.add_argument("mode", choices=list(modes))
    ap.add_argument("out", nargs="?", default=None)
    options = {}
    for table in modes.values():
        if isinstance(table, dict):
            options.update({k: type(v) for k, v in table.items() if k != "fn"})
    for k, t in options.items():
        ap.add_argument("--" + k, type=t, default=None)
    for flag, kw in extra:
        ap.add_argument(flag, **kw)
    a = ap.parse_args(argv)
    a.mode = getattr(a, "mode", None)
    return with_defaults(a, modes[a.mode])


def with_defaults(a, table):
    """A copy of the parsed options with the table's defaults where the command line gave none."""
    b = argparse.Namespace(**vars(a))
    for k, v in (table.items() if isinstance(table, dict) else ()):
        if getattr(b, k, None) is None:
            setattr(b, k, v)
    return b


def sections(a, modes, *args):
    """{mode: section} of a's mode, or of each mode that a's mode lists: fn(options, *args) makes the rows."""
    out = {}
    for mode in (modes[a.mode] if isinstance(modes[a.mode], list) else [a.mode]):
        b = with_defaults(a, modes[mode])
        out[mode] = section(b, b.fn(b, *args))
    return out


def header(tool, **fields):
    return {"tool": tool, "device": torch.cuda.get_device_name(0), **fields}


def section(a, rows):
    return {"trials": a.trials, "reps": a.reps, "rows": rows}


def main_rows(tool, modes):
    """main() of a tool whose modes return rows for {"tool", "device", "trials", "reps", "rows"}, or nothing (a trace
    mode: nothing is written)."""
    a = parse(modes)
    rows = a.fn(a, load_package(), torch.device("cuda:0"))
    if rows is not None:
        write_json(a.out, header(f"{tool} {a.mode}", **section(a, rows)))


def write_json(path, doc, merge=False):
    """doc into path (nothing without a path); merge: over the file's present content, whose other keys stay."""
    if not path:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    if merge and os.path.exists(path):
        with open(path) as f:
            doc = {**json.load(f), **doc}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
