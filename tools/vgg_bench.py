"""Developer tool (GPU box): the pooled 3x3 layer at VGG-16's five pooled shapes, and a whole VGG-16 forward.
usage: python tools/vgg_bench.py [out.json] [--ns 128,1] [--trials 7] [--reps 20] [--skip-net]
         in one process, the variants interleaved in every trial (median of the trials, events around `reps` calls):
         (a) the pooled layer (wino_conv3x3_bn_relu_pool_hw) against the plain layer of the same shape alone, and
             against the plain layer followed by torch's max_pool2d on its interior;
         (b) VGG-16 (random weights) eager and replayed from one graph, against torch eager on channels-last tensors
             (F.conv2d + bias + relu + max_pool2d + linear).
       The default output is profiles/vgg/bench.json."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

MARGIN = 1.02   # the pooled launch may not be slower than the plain launch alone beyond the box-to-box scatter
SHAPES = [(224, 64, 64), (112, 128, 128), (56, 256, 256), (28, 512, 512), (14, 512, 512)]   # (H, C, K)


def _time(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def _interleaved(variants, trials, reps):
    for fn in variants.values():   # warm-up: plans, scratch, torch's algorithm choice
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(trials):
        for k, fn in variants.items():
            times[k].append(_time(fn, reps))
    return {k: statistics.median(v) for k, v in times.items()}, times


def layers(a, pkg, dev):
    rows = []
    for N in (int(v) for v in a.ns.split(",")):
        for H, C, K in SHAPES:
            g = torch.Generator(device=dev).manual_seed(N + H)
            x = torch.rand(N, H + 2, H + 2, C, device=dev, generator=g).sub_(0.5)
            for r in (x[:, 0], x[:, -1], x[:, :, 0], x[:, :, -1]):
                r.zero_()
            w = (torch.rand(K, C, 3, 3, device=dev, generator=g) - 0.5) / (9 * C) ** 0.5 * 2
            b, s = torch.rand(K, device=dev, generator=g) - 0.5, torch.rand(K, device=dev, generator=g) + 0.5
            U = pkg.filter_transform_f2(w)
            full = torch.empty(N, H + 2, H + 2, K, device=dev)
            small = torch.empty(N, H // 2 + 2, H // 2 + 2, K, device=dev)
            pkg.conv3x3_prepare(N, C, K, H, H)

            def plain():
                pkg.conv3x3_bn_relu(x, U, b, s, out=full)

            def plain_then_pool():
                pkg.conv3x3_bn_relu(x, U, b, s, out=full)
                F.max_pool2d(full[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2), 2, 2)

            def pooled():
                pkg.conv3x3_bn_relu_pool(x, U, b, s, out=small)

            med, times = _interleaved({"plain": plain, "plain_then_pool": plain_then_pool, "pooled": pooled},
                                      a.trials, a.reps)
            row = {"N": N, "H": H, "C": C, "K": K, "median_us": med, "trials_us": times,
                   "pooled_over_plain": med["pooled"] / med["plain"],
                   "within_margin": med["pooled"] <= MARGIN * med["plain"],
                   "pooled_over_plain_then_pool": med["pooled"] / med["plain_then_pool"]}
            rows.append(row)
            print(f"N={N:4d} {H}x{H} {C}->{K}: pooled {med['pooled']:9.1f} us  plain {med['plain']:9.1f} us "
                  f"({row['pooled_over_plain']:.3f})  plain+max_pool2d {med['plain_then_pool']:9.1f} us "
                  f"({row['pooled_over_plain_then_pool']:.3f})"
                  + ("" if row["within_margin"] else f"   SLOWER THAN THE PLAIN LAUNCH BY MORE THAN {MARGIN - 1:.0%}"),
                  flush=True)
            del x, full, small
            torch.cuda.empty_cache()
    return rows


def network(a, pkg, dev):
    V = importlib.import_module("cuda_winograd_amd.vgg")
    g = torch.Generator().manual_seed(16)
    sd = {}
    for k, shape in V.expected_keys("vgg16", 1000, 4096).items():
        fan = shape[1] * (9 if len(shape) == 4 else 1) if len(shape) > 1 else 1
        sd[k] = torch.randn(shape, generator=g) * (2.0 / fan) ** 0.5 if len(shape) > 1 else torch.zeros(shape)
    model = pkg.VGG.from_state_dict(sd, "vgg16")
    convs = [(sd[f"features.{i}.weight"].to(dev).contiguous(memory_format=torch.channels_last),
              sd[f"features.{i}.bias"].to(dev), pool) for i, _, _, pool in V.conv_layers("vgg16")]
    fcs = [(sd[f"classifier.{i}.weight"].to(dev), sd[f"classifier.{i}.bias"].to(dev)) for i in (0, 3, 6)]
    rows = []
    for N in (int(v) for v in a.ns.split(",")):
        x = (torch.rand(N, 3, 224, 224, generator=g) * 2 - 1).to(dev)
        x_cl = x.contiguous(memory_format=torch.channels_last)
        sg = torch.cuda.Stream()
        with torch.cuda.stream(sg):
            model.prepare(N, 224, 224)
            model(x)
        sg.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=sg):
            model(x)

        def torch_eager():
            t = x_cl
            for w, b, pool in convs:
                t = torch.relu(F.conv2d(t, w, b, padding=1))
                if pool:
                    t = F.max_pool2d(t, 2, 2)
            t = F.adaptive_avg_pool2d(t, (7, 7)).flatten(1)
            for i, (w, b) in enumerate(fcs):
                t = F.linear(t, w, b)
                if i < 2:
                    t = torch.relu(t)
            return t

        med, times = _interleaved({"eager": lambda: model(x), "graph": graph.replay, "torch": torch_eager},
                                  a.trials, max(1, a.reps // 4))
        rows.append({"arch": "vgg16", "N": N, "median_us": med, "trials_us": times,
                     "tflops_eager": model.flops() * N / med["eager"] / 1e6})
        print(f"vgg16 N={N:4d}: eager {med['eager']:10.1f} us  graph {med['graph']:10.1f} us  "
              f"torch {med['torch']:10.1f} us", flush=True)
        del graph
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "vgg", "bench.json"))
    ap.add_argument("--ns", default="128,1")
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-net", action="store_true")
    a = ap.parse_args()
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    res = {"tool": "tools/vgg_bench.py", "device": torch.cuda.get_device_name(0), "trials": a.trials, "reps": a.reps,
           "layers": layers(a, pkg, dev)}
    if not a.skip_net:
        res["network"] = network(a, pkg, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    slow = [r for r in res["layers"] if not r["within_margin"]]
    if slow:
        print(f"{len(slow)} pooled shape(s) slower than the plain launch beyond the margin", flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
