"""What the GPU test modules share: the module-scoped fixtures (imported by name into each test module that uses
them, `from gpu_support import torch_dev  # noqa: F401`, so each module still gets its own instance), the torch
relative-error measure of the network tests, and the scenarios several layers' tests repeat step for step: the
fail-fast contract of the ticket counters, and a block or a whole network captured into a graph."""
import importlib

import pytest

import layer_refs


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch, torch.device("cuda:0")


@pytest.fixture(scope="module")
def R(pkg):
    return importlib.import_module("cuda_winograd_amd.resnet")


@pytest.fixture(scope="module")
def V(pkg):
    return importlib.import_module("cuda_winograd_amd.vgg")


def rel(torch, got, want):
    """layer_refs.rel: max |got - want| / max |want| against an fp64 CPU tensor, shapes equal, both sides finite."""
    return layer_refs.rel(got, want)


def _clone(r):
    return tuple(t.clone() for t in r) if isinstance(r, tuple) else r.clone()


def dirty_ticket_scenario(pkg, torch, launch, n_tickets, same=None, check=None, also_refused=(), after=None, reruns=2):
    """The fail-fast contract of a stream's ticket counters, on a stream of its own.  `launch()` runs the layer and
    returns its output (or a tuple of outputs); the first `n_tickets` counters are the ones it draws on.  A counter
    left non-zero (as by a launch that died mid-way) is reported by the launch that meets it, every launch on the
    stream then fails with WINO_E_STATE (rc=-4), `launch` and each of `also_refused` alike, and
    wino_stream_reset_scratch() recovers: `reruns` further launches are `same(got, ref)` (torch.equal unless given) as
    the clean first one, which `check(ref)` compared with its oracle.  `after()` runs last, on the recovered stream."""
    same = same or torch.equal
    with torch.cuda.stream(torch.cuda.Stream()):
        ref = _clone(launch())
        if check:
            check(ref)
        assert pkg.tickets_in_use() == 0
        pkg.stream_check()
        # every counter the launch draws on is left one too high, as by a launch that never finished
        for i in range(n_tickets):
            pkg.poison_ticket(i, 1)
        launch()   # computes with dirty counters: its result is not to be trusted, and it must say so
        with pytest.raises(pkg.WinoError, match="rc=-4"):
            pkg.stream_check()
        for refused in (launch, *also_refused):
            with pytest.raises(pkg.WinoError, match="rc=-4"):
                refused()
        pkg.stream_reset_scratch()
        pkg.stream_check()
        assert pkg.tickets_in_use() == 0
        for _ in range(reruns):
            assert same(launch(), ref)
        if after:
            after()
        assert pkg.tickets_in_use() == 0
    torch.cuda.synchronize()


def graph_replay_scenario(pkg, torch_dev, run, prepare, workspace_bytes, rounds=2):
    """A block captured into one graph.  `run(out=, workspace=)` launches it (into fresh tensors when they are left
    out); `prepare()` allocates every launch's scratch on the capture stream beforehand (an allocation inside a
    capture is an error).  `rounds` replays into a zeroed `out` are bitwise the eager result, and no ticket stays held
    on the capture stream or the current one.  Returns the eager result for the caller's oracle check."""
    torch, dev = torch_dev
    eager = run().clone()
    out = torch.zeros_like(eager)
    ws = torch.empty(workspace_bytes // 4, device=dev)
    sg = torch.cuda.Stream()
    with torch.cuda.stream(sg):
        prepare()
    sg.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=sg):
        run(out=out, workspace=ws)
    for _ in range(rounds):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    with torch.cuda.stream(sg):
        assert pkg.tickets_in_use() == 0
    assert pkg.tickets_in_use() == 0
    return eager


def network_graph_scenario(pkg, torch, model, x, rounds=2):
    """A whole network captured into one graph: prepared and run eagerly on the capture stream, captured there, then
    `rounds` replays into a NaN-filled output are bitwise the eager logits and no ticket stays held.  Returns
    (eager logits, the graph); the graph holds the model's tensors, so the caller deletes it when done."""
    N, _, H, W = x.shape
    sg = torch.cuda.Stream()
    with torch.cuda.stream(sg):
        model.prepare(N, H, W)
        eager = model(x).clone()
    sg.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=sg):
        out = model(x)
    for _ in range(rounds):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    with torch.cuda.stream(sg):
        assert pkg.tickets_in_use() == 0
    return eager, graph
