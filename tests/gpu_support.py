"""What the GPU test modules share: the module-scoped fixtures (imported by name into each test module that uses
them, `from gpu_support import torch_dev  # noqa: F401`, so each module still gets its own instance), the torch
relative-error measure of the network tests, the scenarios several layers' tests repeat step for step (the fail-fast
contract of the ticket counters, a block or a whole network captured into a graph), and the guarded-arena runs of box
decoding and batched NMS that tests/test_gpu_boxes.py and tests/test_gpu_box_sweep.py both use."""
import importlib

import numpy as np
import pytest

import guarded
import layer_refs

NAN = float("nan")


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


def same_bits(a, b):
    """Two tensors (or arrays), wherever they live, have one shape, one dtype and the same bytes."""
    import torch
    a, b = (torch.as_tensor(t).detach().cpu().contiguous() for t in (a, b))
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool((a.reshape(-1).view(torch.uint8) == b.reshape(-1).view(torch.uint8)).all())


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


# ---- box decoding and batched NMS on the guarded arena --------------------------------------------------------------------
def as_f32(a: np.ndarray):
    """An int32 array as the float32 master the arena holds (same bits)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).view(torch.float32)


def bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def run_decode(pkg, dev, c, head=None, offset=0, extra=0, aligns=guarded.ALIGNS, tag=""):
    """The kernel on case `c` (or on another `head`), into [N][offset + boxes + extra] outputs; returns this launch's
    slice of (boxes, scores) on the CPU.  What lies outside the slice keeps its NaN fill.  A case without a score column
    goes through the C entry point itself with a scores buffer passed alongside, which must keep its NaN fill whole."""
    import torch
    per, first = c.rpi * c.A, None
    total = offset + per + extra
    for align in aligns:
        arena = guarded.Arena(torch, dev, align)
        h = arena.input(torch.from_numpy(c.head if head is None else head), name="head")
        anc = arena.input(torch.from_numpy(c.anchors), name="anchors")
        hw = arena.input(torch.from_numpy(c.image_hw), name="image_hw")
        ob, os_ = arena.output(c.N, total, 4, name="boxes"), arena.output(c.N, total, name="scores")
        for _ in range(2):
            ob.fill_(NAN), os_.fill_(NAN)
            if c.score_col is None:
                gh, gw, sy, sx = c.grid or (0, 0, 0, 0)
                p = lambda t: t.data_ptr() or None
                pkg._check(pkg.lib().wino_box_decode_hw(p(h), c.N, c.rpi, c.ld, c.A, c.delta_col, -1, p(anc), gh, gw, sy, sx,
                                                        p(hw), *c.weights, c.clamp, p(ob), total, offset, p(os_), total, offset,
                                                        pkg._stream()), "wino_box_decode_hw")
            else:
                got = pkg.box_decode(h, anc, hw, c.A, c.weights, c.grid, c.delta_col, c.score_col, ob, os_, offset, c.clamp)
                assert got[0] is ob and got[1] is os_
            arena.check(f"box_decode {tag} align={align}")
            b, s = ob.cpu(), os_.cpu()
            outside = torch.ones(total, dtype=torch.bool)
            outside[offset:offset + per] = False
            if c.score_col is None:
                outside_scores = torch.ones(total, dtype=torch.bool)
            else:
                outside_scores = outside
            assert bool(torch.isnan(b[:, outside]).all()) and bool(torch.isnan(s[:, outside_scores]).all()), \
                "wrote outside its slice"
            cur = (b[:, offset:offset + per].contiguous(), s[:, offset:offset + per].contiguous())
            if first is None:
                first = cur
            assert torch.equal(bits(cur[0]), bits(first[0])) and torch.equal(bits(cur[1]), bits(first[1])), \
                f"{tag}: not bitwise reproducible (align {align})"
    return first[0].numpy(), (None if c.score_col is None else first[1].numpy())


def run_nms(pkg, dev, boxes, scores, groups, max_out, params, rois=True, aligns=guarded.ALIGNS, tag="", repeats=2):
    """The two kernels on numpy operands, on the guarded arena at each of `aligns`: a first call, then (repeats = 2) a
    second one into NaN-filled outputs and a NaN-filled workspace, bitwise the first.  Returns (keep, count, rois) as
    numpy arrays."""
    import torch
    S, R = boxes.shape[:2]
    first = None
    for align in aligns:
        arena = guarded.Arena(torch, dev, align)
        b = arena.input(torch.from_numpy(boxes), name="boxes")
        sc = None if scores is None else arena.input(torch.from_numpy(scores), name="scores")
        g = None if groups is None else arena.input(as_f32(groups), name="groups").view(torch.int32)
        keep = arena.output(S, max_out, name="keep").view(torch.int32)
        count = arena.output(S, name="count").view(torch.int32)
        ro = arena.output(S, max_out, 5, name="rois") if rois else False
        ws = arena.workspace(pkg.nms_workspace_bytes(S, R), name="workspace")
        for _ in range(repeats):
            keep.view(torch.float32).fill_(NAN), count.view(torch.float32).fill_(NAN), ws.fill_(NAN)
            if rois:
                ro.fill_(NAN)
            got = pkg.batched_nms(b, sc, g, max_out=max_out, rois_out=ro, workspace=ws, keep=keep, count=count, **params)
            assert got[0] is keep and got[1] is count and (not rois or got[2] is ro)
            arena.check(f"batched_nms {tag} S={S} R={R} max_out={max_out} align={align}")
            cur = (keep.cpu().numpy(), count.cpu().numpy(), ro.cpu().numpy() if rois else None)
            if first is None:
                first = cur
            for x, y in zip(cur, first):
                assert x is None or np.array_equal(x.view(np.int32), y.view(np.int32)), f"{tag}: not bitwise reproducible"
    return first
