"""Developer tool (GPU box): the pooled 3x3 layer at VGG-16's five pooled shapes, and a whole VGG-16 forward.
usage: python tools/vgg_bench.py [out.json] [--ns 128,1] [--trials 7] [--reps 20] [--skip-net]
         in one process, the variants interleaved in every trial (median of the trials, events around `reps` calls):
         (a) the pooled layer (wino_conv3x3_bn_relu_pool_hw) against the plain layer of the same shape alone, and
             against the plain layer followed by torch's max_pool2d on its interior;
         (b) VGG-16 (random weights) eager and replayed from one graph, against torch eager on channels-last tensors
             (F.conv2d + bias + relu + max_pool2d + linear).
       The default output is profiles/vgg/bench.json."""
import os
import sys

import benchlib
import torch
import torch.nn.functional as F
import torch_nets

MARGIN = 1.02   # the pooled launch may not be slower than the plain launch alone beyond the box-to-box scatter
SHAPES = [(224, 64, 64), (112, 128, 128), (56, 256, 256), (28, 512, 512), (14, 512, 512)]   # (H, C, K)


def layers(a, pkg, dev):
    rows = []
    for N in benchlib.ints(a.ns):
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

            med, times = benchlib.interleaved({"plain": plain, "plain_then_pool": plain_then_pool, "pooled": pooled},
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
    V = benchlib.package_module("vgg")
    g = torch.Generator().manual_seed(16)
    sd = torch_nets.vgg_state_dict(V, "vgg16", g)
    model = pkg.VGG.from_state_dict(sd, "vgg16")
    torch_eager = torch_nets.torch_vgg(sd, V, "vgg16", dev)
    rows = []
    for N in benchlib.ints(a.ns):
        x = (torch.rand(N, 3, 224, 224, generator=g) * 2 - 1).to(dev)
        x_cl = x.contiguous(memory_format=torch.channels_last)
        graph, _ = benchlib.captured(lambda: model(x), lambda: model.prepare(N, 224, 224))
        med, times = benchlib.interleaved(benchlib.net_variants(lambda: model(x), graph, lambda: torch_eager(x_cl)),
                                          a.trials, max(1, a.reps // 4))
        rows.append({"arch": "vgg16", "N": N, "median_us": med, "trials_us": times,
                     "tflops_eager": model.flops() * N / med["eager"] / 1e6})
        print(f"vgg16 N={N:4d}: eager {med['eager']:10.1f} us  graph {med['graph']:10.1f} us  "
              f"torch {med['torch']:10.1f} us", flush=True)
        del graph
        torch.cuda.empty_cache()
    return rows


MODES = {None: dict(ns="128,1", trials=7, reps=20)}
EXTRA = [("--skip-net", dict(action="store_true"))]


def main():
    a = benchlib.parse(MODES, EXTRA)
    pkg = benchlib.load_package()
    dev = torch.device("cuda:0")
    res = benchlib.header("tools/vgg_bench.py", trials=a.trials, reps=a.reps, layers=layers(a, pkg, dev))
    if not a.skip_net:
        res["network"] = network(a, pkg, dev)
    benchlib.write_json(a.out or os.path.join(benchlib.ROOT, "profiles", "vgg", "bench.json"), res)
    slow = [r for r in res["layers"] if not r["within_margin"]]
    if slow:
        print(f"{len(slow)} pooled shape(s) slower than the plain launch beyond the margin", flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
