"""Developer tool (GPU box): the bilinear resize and label-map launch, and the segmentation networks' output stage.
usage: python tools/resize_bench.py layer [out.json] [--ns 1,8] [--trials 7] [--reps 20]
         the launch (wino_resize_bilinear_hw) at 65x65x21 (ld 64) -> 520x520 and 33x33x21 -> 260x260 in its three uses --
         out only, labels only, both -- interleaved in every trial with what it replaces:
           torch_out     F.interpolate(bilinear, align_corners=False) on the permuted view of the scores
           torch_labels  that, followed by .argmax(1)
         each variant twice: called eagerly (events around `reps` calls: Python's and the launch's host time count), and
         as `reps` calls captured into one graph (replays: what the stream executes); beside each time the store-bound
         floor: bytes written / 6.29 TB/s (the measured copy rate)
       python tools/resize_bench.py net [out.json] [--ns 1,8] [--trials 5] [--reps 3] [--size 520]
         FCN-ResNet50 and DeepLabV3-ResNet50 forwards to a label map, one-graph replay each, interleaved:
           torch   resize="torch", then torch's .argmax(1)
           kernel  labels=True, out=False: only the label map is written
       python tools/resize_bench.py all profiles/resize/bench.json
         both, each in a child process of its own under its own time limit, into one file
(median of the trials, events around `reps` calls)"""
import json
import os
import subprocess
import sys
import tempfile

import benchlib
import torch
import torch.nn.functional as F
import torch_nets

COPY_TBS = 6.29          # the measured device copy rate the floors are taken at
POINTS = [(65, 520), (33, 260)]
C, LD = 21, 64
FORMS = {1: "staged", 2: "direct"}
STEP_LIMIT_S = {"layer": 240, "net": 420}


def layer(a, pkg, dev):
    rows = []
    for h, Ho in POINTS:
        for N in benchlib.ints(a.ns):
            g = torch.Generator().manual_seed(N + h)
            scores = (torch.rand(N, h, h, LD, generator=g) - 0.5).to(dev)
            out = torch.empty(N, C, Ho, Ho, device=dev)
            labels = torch.empty(N, Ho, Ho, dtype=torch.int32, device=dev)
            view = scores[..., :C].permute(0, 3, 1, 2)
            t_out = lambda: F.interpolate(view, size=(Ho, Ho), mode="bilinear", align_corners=False)
            variants = {
                "out": lambda: pkg.resize_bilinear(scores, Ho, Ho, C=C, out=out),
                "labels": lambda: pkg.resize_bilinear(scores, Ho, Ho, C=C, labels=labels, want_out=False),
                "both": lambda: pkg.resize_bilinear(scores, Ho, Ho, C=C, out=out, labels=labels),
                "torch_out": t_out,
                "torch_labels": lambda: t_out().argmax(1),
            }
            ref = t_out()
            diff = float((variants["out"]()[0] - ref).abs().max() / ref.abs().max())
            agree = float((variants["labels"]()[1] == ref.argmax(1)).float().mean())
            med, times = benchlib.interleaved(variants, a.trials, a.reps)
            graphs = {k: benchlib.captured(benchlib.repeated(fn, a.reps))[0] for k, fn in variants.items()}
            gmed, gtimes = benchlib.interleaved({k: gph.replay for k, gph in graphs.items()}, a.trials, 3)
            gmed = {k: v / a.reps for k, v in gmed.items()}
            gtimes = {k: [t / a.reps for t in v] for k, v in gtimes.items()}
            del graphs
            out_b, lab_b = 4.0 * N * C * Ho * Ho, 4.0 * N * Ho * Ho
            floor = {"out": out_b / COPY_TBS / 1e6, "labels": lab_b / COPY_TBS / 1e6, "both": (out_b + lab_b) / COPY_TBS / 1e6}
            form = FORMS[pkg.resize_bilinear_plan(h, h, C, LD, Ho, Ho)]
            ratios = lambda m: {"out_over_torch_out": m["out"] / m["torch_out"],
                                "labels_over_torch_labels": m["labels"] / m["torch_labels"],
                                "both_over_torch_labels": m["both"] / m["torch_labels"]}
            rows.append({"N": N, "h": h, "Ho": Ho, "C": C, "ld": LD, "form": form, "store_floor_us": floor,
                         "eager": dict(median_us=med, trials_us=times, **ratios(med)),
                         "graph": dict(median_us=gmed, trials_us=gtimes, **ratios(gmed)),
                         "rel_diff_to_torch_fp32": diff, "labels_equal_torch": agree})
            for how, m in (("eager", med), ("graph", gmed)):
                r = ratios(m)
                print(f"resize N={N} {h}->{Ho} ({form}) {how}  out {m['out']:7.1f} us (floor {floor['out']:5.1f})  labels "
                      f"{m['labels']:7.1f} (floor {floor['labels']:4.1f})  both {m['both']:7.1f} (floor {floor['both']:5.1f})  | "
                      f"torch out {m['torch_out']:7.1f}  torch out+argmax {m['torch_labels']:7.1f}  | out/torch "
                      f"{r['out_over_torch_out']:.3f}  labels/torch {r['labels_over_torch_labels']:.3f}  both/torch "
                      f"{r['both_over_torch_labels']:.3f}", flush=True)
            print(f"    (rel diff to torch fp32 {diff:.1e}, labels equal {agree:.5f})", flush=True)
            del scores, out, labels, ref
            torch.cuda.empty_cache()
    return rows


def net(a, pkg, dev):
    R = benchlib.package_module("resnet")
    rows = []
    S = a.size
    for name, cls, make in (("fcn_resnet50", pkg.FCN, torch_nets.fcn_state_dict),
                            ("deeplabv3_resnet50", pkg.DeepLabV3, torch_nets.deeplab_state_dict)):
        model = cls.from_state_dict(make(R, "resnet50"), "resnet50")
        for N in benchlib.ints(a.ns):
            x, _ = torch_nets.image_batch(N, S, S, dev)
            runs = {"torch": lambda: model(x, resize="torch")["out"].argmax(1),
                    "kernel": lambda: model(x, labels=True, out=False)["labels"]}
            graphs, results = {}, {}
            for k, fn in runs.items():   # prepare allocates the activations: once, before the first capture
                graphs[k], results[k] = benchlib.captured(fn, None if graphs else lambda: model.prepare(N, S, S))
            agree = float((results["torch"] == results["kernel"]).float().mean())
            med, times = benchlib.interleaved({k: gph.replay for k, gph in graphs.items()}, a.trials, a.reps)
            rows.append({"arch": name, "N": N, "size": S, "median_us": med, "trials_us": times,
                         "labels_equal_torch": agree, "kernel_over_torch": med["kernel"] / med["torch"],
                         "saved_us": med["torch"] - med["kernel"]})
            print(f"{name} N={N} {S}x{S}  graph, torch resize + argmax {med['torch']:9.1f} us  graph, labels=True out=False "
                  f"{med['kernel']:9.1f} us  kernel/torch {rows[-1]['kernel_over_torch']:.3f}  (labels equal {agree:.5f})",
                  flush=True)
            del graphs, results, x
            torch.cuda.empty_cache()
        del model
        torch.cuda.empty_cache()
    return rows


MODES = {"layer": dict(fn=layer, ns="1,8", trials=7, reps=20),
         "net": dict(fn=net, ns="1,8", size=520, trials=5, reps=3),
         "all": ["layer", "net"]}


def run_all(a):
    """Each step in a fresh child process under its own time limit; the first that fails ends the run."""
    result = {"tool": "tools/resize_bench.py all"}
    with tempfile.TemporaryDirectory() as tmp:
        for mode in MODES["all"]:
            part = os.path.join(tmp, mode + ".json")
            cmd = [sys.executable, os.path.abspath(__file__), mode, part]
            cmd += (["--ns", a.ns] if a.ns else []) + (["--size", str(a.size)] if a.size else [])
            subprocess.run(cmd, check=True, timeout=STEP_LIMIT_S[mode])
            with open(part) as f:
                got = json.load(f)
            result["device"] = got["device"]
            result[mode] = got[mode]
    return result


def main():
    a = benchlib.parse(MODES)
    if a.mode == "all":
        result = run_all(a)
    else:
        result = benchlib.header(f"tools/resize_bench.py {a.mode}")
        result.update(benchlib.sections(a, MODES, benchlib.load_package(), torch.device("cuda:0")))
    benchlib.write_json(a.out, result)


if __name__ == "__main__":
    main()
