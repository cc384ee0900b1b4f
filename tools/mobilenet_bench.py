"""Developer tool (GPU box): the depthwise 3x3 layer at MobileNetV2's distinct points, and a whole MobileNetV2 forward.
usage: python tools/mobilenet_bench.py [out.json] [--ns 1,32] [--trials 7] [--reps 20] [--skip-net]
         in one process, the variants interleaved in every trial (median of the trials; a layer variant is one graph of
         `reps` launches, a network variant is timed by events around `reps` // 4 calls):
         (a) the depthwise layer (act relu6, in_cap 6) at the kernel's real (padded to 64) channel count under the plan's
             channel block and under each block forced (WINO_DW_CB), against torch's F.conv2d(groups=C) on channels-last
             tensors followed by the BN affine and clamp, and against a plain copy of the input map, the kernel's floor
             of 4 N C (Hin Win + H W) bytes;
         (b) mobilenet_v2 at 224 x 224 (random weights) eager and replayed from one graph, against torch eager on
             channels-last tensors.
       The default output is profiles/mobilenet/bench.json."""
import os

import benchlib
import torch
import torch.nn.functional as F
import torch_nets

# (Hin, C of the network, stride): every distinct depthwise layer of mobilenet_v2 at 224 x 224
POINTS = [(112, 32, 1), (112, 96, 2), (56, 144, 1), (56, 144, 2), (28, 192, 1), (28, 192, 2), (14, 384, 1), (14, 576, 1),
          (14, 576, 2), (7, 960, 1)]


def layers(a, pkg, dev):
    rows, L = [], pkg.lib()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count

    def force(cb):
        def setup():
            if cb:
                os.environ["WINO_DW_CB"] = str(cb)
            else:
                os.environ.pop("WINO_DW_CB", None)
            L.wino_debug_reload_knobs()
        return setup

    for N in benchlib.ints(a.ns):
        for Hin, c, stride in POINTS:
            C, H = -(-c // 64) * 64, (Hin - 1) // stride + 1
            g = torch.Generator(device=dev).manual_seed(N + Hin + C)
            x = torch.randn(N, Hin + 2, Hin + 2, C, device=dev, generator=g).mul_(6 / 0.84)
            for r in (x[:, 0], x[:, -1], x[:, :, 0], x[:, :, -1]):
                r.zero_()
            w = torch.randn(C, 1, 3, 3, device=dev, generator=g) / 3
            b, s = torch.rand(C, device=dev, generator=g) - 0.5, torch.rand(C, device=dev, generator=g) + 0.5
            taps = w[:, 0].permute(1, 2, 0).contiguous()
            out = torch.empty(N, H + 2, H + 2, C, device=dev)
            x_cl = x[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).clamp(max=6.0).contiguous(memory_format=torch.channels_last)
            w_cl = w.contiguous(memory_format=torch.channels_last)
            s4, b4 = s[None, :, None, None], b[None, :, None, None]
            src = torch.empty(N * C * (Hin * Hin + H * H) // 2, device=dev)   # the copy moves the layer's bytes
            dst = torch.empty_like(src)

            def ours():
                pkg.dwconv3x3_bn_act(x, taps, b, s, stride, "relu6", 6.0, out=out)

            def torch_dw():
                (F.conv2d(x_cl, w_cl, stride=stride, padding=1, groups=C) * s4 + b4).clamp_(0, 6)

            # each variant is one graph of `reps` launches (the launcher reads the knob when it is captured): a replay
            # times the kernels, not the Python wrapper, which at the small points costs more than the kernel
            graphs = {}
            for k, fn, cb in (("plan", ours, 0), ("cb64", ours, 64), ("cb16", ours, 16), ("torch", torch_dw, 0),
                              ("copy", lambda: dst.copy_(src), 0)):
                force(cb)()
                graphs[k] = benchlib.captured(benchlib.repeated(fn, a.reps))[0]
            force(0)()
            med, times = benchlib.interleaved({k: g.replay for k, g in graphs.items()}, a.trials, 1)
            med = {k: v / a.reps for k, v in med.items()}
            times = {k: [t / a.reps for t in v] for k, v in times.items()}
            cb = pkg.dwconv3x3_plan(N, Hin, Hin, C, stride, cus)[0]
            best = 64 if med["cb64"] <= med["cb16"] else 16
            row = {"N": N, "Hin": Hin, "C": C, "stride": stride, "plan_cb": cb, "faster_cb": best, "median_us": med,
                   "trials_us": times, "over_copy": med["plan"] / med["copy"], "over_torch": med["plan"] / med["torch"],
                   "gb_s": 4e-3 * N * C * (Hin * Hin + H * H) / med["plan"]}
            rows.append(row)
            print(f"N={N:3d} {Hin}x{Hin}x{C} s{stride}: plan(cb{cb}) {med['plan']:8.1f} us  cb64 {med['cb64']:8.1f}  cb16 "
                  f"{med['cb16']:8.1f}  torch {med['torch']:8.1f} ({row['over_torch']:.2f})  copy {med['copy']:8.1f} "
                  f"({row['over_copy']:.2f})  {row['gb_s']:.0f} GB/s" + ("" if best == cb else "   PLAN IS NOT THE FASTER BLOCK"),
                  flush=True)
            del graphs, x, out, x_cl, src, dst
            torch.cuda.empty_cache()
    return rows


def network(a, pkg, dev):
    M = benchlib.package_module("mobilenet")
    sd = torch_nets.mobilenet_state_dict(M, 1.0)
    model = pkg.MobileNetV2.from_state_dict(sd)
    torch_eager = torch_nets.torch_mobilenet(sd, M, 1.0, dev)
    rows = []
    for N in benchlib.ints(a.ns):
        x, x_cl = torch_nets.image_batch(N, 224, 224, dev)
        graph, _ = benchlib.captured(lambda: model(x), lambda: model.prepare(N, 224, 224))
        med, times = benchlib.interleaved(benchlib.net_variants(lambda: model(x), graph, lambda: torch_eager(x_cl)),
                                          a.trials, max(1, a.reps // 4))
        rows.append({"arch": "mobilenet_v2", "N": N, "median_us": med, "trials_us": times, **benchlib.net_ratios(med)})
        print(f"mobilenet_v2 N={N:4d}: eager {med['eager']:10.1f} us  graph {med['graph']:10.1f} us  "
              f"torch {med['torch']:10.1f} us", flush=True)
        del graph
        torch.cuda.empty_cache()
    return rows


MODES = {None: dict(ns="1,32", trials=7, reps=20)}
EXTRA = [("--skip-net", dict(action="store_true"))]


def main():
    a = benchlib.parse(MODES, EXTRA)
    pkg = benchlib.load_package()
    dev = torch.device("cuda:0")
    res = benchlib.header("tools/mobilenet_bench.py", trials=a.trials, reps=a.reps, layers=layers(a, pkg, dev))
    if not a.skip_net:
        res["network"] = network(a, pkg, dev)
    benchlib.write_json(a.out or os.path.join(benchlib.ROOT, "profiles", "mobilenet", "bench.json"), res)


if __name__ == "__main__":
    main()
