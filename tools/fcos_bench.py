"""Developer tool (GPU box): the GroupNorm + ReLU kernel and FCOS's score-map and decode kernels at FCOS's five levels.
usage: python tools/fcos_bench.py [profiles/fcos/bench.json] [--trials 7] [--reps 20] [--det_trials 5] [--det_reps 5]
  fcos_resnet50_fpn at 800 x 1344: levels 100 x 168, 50 x 84, 25 x 42, 13 x 21, 7 x 11, C = 256, GroupNorm(32, 256), 91
  classes, N = 1 and 2.  Every figure is us per call inside one graph of `reps` calls, so that launch gaps count the way
  they do in a captured network:
    groupnorm   groupnorm_relu in place, forced whole, forced split and as planned; torch's F.group_norm + relu_ on the
                same values (channels-last interior); a device copy of the padded map, the time of reading and writing it once
    score       fcos_score_map in place on the class-logit map
    decode      fcos_decode of 1000 selected locations
    detector    FCOS-ResNet50-FPN and RetinaNet-ResNet50-FPN with random weights at N = 1 and 2 (us per forward, events
                around `det_reps` calls): eager, from one graph, the backbone alone, the head alone from a graph, and for
                FCOS the head's convolutions alone (the same graph without its 40 GroupNorm calls)
(median of the trials; every trial is kept in the JSON: their spread is the run-to-run noise)"""
import os

import benchlib
import torch

IMAGE = (800, 1344)
LEVEL_HW = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
STRIDES = [8, 16, 32, 64, 128]
C, G, K, TOPK = 256, 32, 91, 1000


def graph_of(fn, reps):
    return benchlib.captured(benchlib.repeated(fn, reps))[0]


def per_call(graphs, a):
    med, times = benchlib.interleaved({k: g.replay for k, g in graphs.items()}, a.trials, 1)
    return {k: v / a.reps for k, v in med.items()}, {k: [t / a.reps for t in v] for k, v in times.items()}


def force(pkg, form):
    if form:
        os.environ["WINO_GN_FORM"] = form
    else:
        os.environ.pop("WINO_GN_FORM", None)
    pkg.lib().wino_debug_reload_knobs()


def groupnorm_rows(a, pkg, dev):
    g = torch.Generator().manual_seed(11)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(dev), (torch.rand(C, generator=g) - 0.5).to(dev)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = []
    for N in (1, 2):
        for h, w in LEVEL_HW:
            x = torch.zeros(N, h + 2, w + 2, C)
            x[:, 1:-1, 1:-1] = torch.randn(N, h, w, C, generator=g)
            x = x.to(dev)
            y = torch.empty_like(x)
            xt = x[:, 1:-1, 1:-1].permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
            graphs, plans, held = {}, {}, []
            for name, form in (("whole", "whole"), ("split", "split"), ("planned", None)):
                force(pkg, form)
                plans[name] = pkg.groupnorm_plan(N, h, w, C, G, cus)
                ws = torch.empty(pkg.groupnorm_workspace_bytes(N, h, w, C, G) // 4 + 4, device=dev)
                buf = x.clone()
                # a graph does not own the tensors its launches name, and the next capture empties the allocator's cache:
                # a map or workspace dropped here would be unmapped under the replays
                held += [buf, ws]
                graphs[name] = graph_of(lambda buf=buf, ws=ws: pkg.groupnorm_relu(buf, gamma, beta, G, out=buf, workspace=ws),
                                        a.reps)
            force(pkg, None)
            graphs["torch"] = graph_of(lambda: torch.nn.functional.group_norm(xt, G, gamma, beta, 1e-5).relu_(), a.reps)
            graphs["copy"] = graph_of(lambda: y.copy_(x), a.reps)
            med, times = per_call(graphs, a)
            del graphs, held
            rows.append({"N": N, "h": h, "w": w, "map_bytes": x.numel() * 4, "planned_form": plans["planned"][0],
                         "split_chunks": plans["split"][1], **{f"{k}_us": v for k, v in med.items()},
                         **{f"{k}_trials_us": v for k, v in times.items()}})
            print(f"groupnorm N={N} {h:3d}x{w:3d}: whole {med['whole']:7.2f}  split {med['split']:7.2f} ({plans['split'][1]} chunks)  "
                  f"planned {med['planned']:7.2f} ({plans['planned'][0]})  torch {med['torch']:7.2f}  copy {med['copy']:7.2f} us",
                  flush=True)
    return rows


def kernel_rows(a, pkg, dev):
    g = torch.Generator().manual_seed(12)
    rows = []
    for N in (1, 2):
        for (h, w), stride in zip(LEVEL_HW, STRIDES):
            cls = torch.randn(N, h + 2, w + 2, 128, generator=g).to(dev)
            reg = torch.randn(N, h + 2, w + 2, 64, generator=g).to(dev)
            k = min(TOPK, h * w * K)
            idx = torch.stack([torch.randperm(h * w * K, generator=g)[:k] for _ in range(N)]).to(torch.int32).to(dev)
            base = torch.tensor([[-4.0, -4.0, 4.0, 4.0]], device=dev) * (stride / 8)
            hw = torch.tensor([IMAGE] * N, dtype=torch.float32, device=dev)
            boxes, labels = torch.empty(N, k, 4, device=dev), torch.empty(N, k, dtype=torch.int32, device=dev)
            graphs = {"score": graph_of(lambda: pkg.fcos_score_map(cls, reg, K, 4), a.reps),
                      "decode": graph_of(lambda: pkg.fcos_decode(idx, reg, base, hw, (h, w, stride, stride), K, out_boxes=boxes,
                                                                 out_labels=labels), a.reps)}
            med, times = per_call(graphs, a)
            del graphs
            rows.append({"N": N, "h": h, "w": w, "k": k, **{f"{n}_us": v for n, v in med.items()},
                         **{f"{n}_trials_us": v for n, v in times.items()}})
            print(f"N={N} {h:3d}x{w:3d}: score map {med['score']:7.2f} us   decode of {k} {med['decode']:7.2f} us", flush=True)
    return rows


def detector_rows(a, pkg, dev):
    R = benchlib.package_module("resnet")
    fp, rr, fr = (benchlib.tests_module(n) for n in ("fpn_p6p7_reference", "retinanet_reference", "fcos_reference"))
    fpn_sd, _ = fp.p6p7_random_state_dict(torch, R, "resnet50", C, seed=1)
    backbone = {"backbone." + k: v for k, v in fpn_sd.items()}
    heads = {"fcos": (pkg.FCOS, fr.head_state_dict(C, K, seed=2)), "retinanet": (pkg.RetinaNet, rr.head_state_dict(C, 9, K, seed=2))}
    rows = []
    for N in (1, 2):
        x = torch.rand((N, 3, *IMAGE), device=dev) - 0.5
        for name, (cls, head_sd) in heads.items():
            m = cls.from_state_dict({**backbone, **{"head." + k: v for k, v in head_sd.items()}}, "resnet50", device=dev)
            # one prepare, then every graph on the stream it reserved the scratch on: a second prepare would free the
            # tensors an earlier graph holds
            sg = torch.cuda.Stream()
            sg.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(sg):
                m.prepare(N, *IMAGE)
                count = m(x)["count"].tolist()
                maps = [t.clone() for t in (m.backbone(x, padded=True)[k] for k in ("0", "1", "2", "p6", "p7"))]
                m.head(maps)
            sg.synchronize()

            def capture(fn):
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=sg):
                    fn()
                torch.cuda.synchronize()
                return graph

            graph, head_graph = capture(lambda: m(x)), capture(lambda: m.head(maps))
            calls = {"eager": lambda: m(x), "graph": graph.replay, "backbone": lambda: m.backbone(x, padded=True),
                     "head_graph": head_graph.replay}
            if name == "fcos":
                gn = pkg.groupnorm_relu
                try:                                     # the head's graph once more, its GroupNorm calls left out
                    pkg.groupnorm_relu = lambda t, *args, **kw: t
                    convs_graph = capture(lambda: m.head(maps))
                    calls["head_convs_graph"] = convs_graph.replay
                finally:
                    pkg.groupnorm_relu = gn
            med, times = benchlib.interleaved(calls, a.det_trials, a.det_reps)
            torch.cuda.synchronize()
            rows.append({"model": name, "N": N, "H": IMAGE[0], "W": IMAGE[1], "classes": K, "count": count,
                         **{f"{k}_us": v for k, v in med.items()}, **{f"{k}_trials_us": v for k, v in times.items()}})
            print(f"{name:9s} N={N}: " + "  ".join(f"{k} {v:9.1f}" for k, v in med.items()) + " us", flush=True)
            del graph, head_graph, calls, m
    return rows


MODES = {None: dict(trials=7, reps=20, det_trials=5, det_reps=5)}


def main():
    a = benchlib.parse(MODES)
    pkg = benchlib.load_package()
    dev = torch.device("cuda:0")
    result = benchlib.header("tools/fcos_bench.py", trials=a.trials, reps=a.reps,
                             workload={"image": IMAGE, "levels": LEVEL_HW, "channels": C, "groups": G, "classes": K, "topk": TOPK})
    result["groupnorm"] = groupnorm_rows(a, pkg, dev)
    result["kernels"] = kernel_rows(a, pkg, dev)
    result["detector"] = detector_rows(a, pkg, dev)
    benchlib.write_json(a.out, result)


if __name__ == "__main__":
    main()
