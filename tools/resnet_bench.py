"""Developer tool (GPU box): the ResNet stem and whole ResNet forwards.
usage: python tools/resnet_bench.py stem [out.json] [--ns 1,32,128] [--trials 7] [--reps 20]
         in one process, the variants interleaved in every trial (median of the trials, events around `reps` calls):
         the fused stem (wino_stem_hw, automatic form, and each forced form) against torch's composition on the same
         card: F.conv2d on channels-last fp32, BN as scale and bias, ReLU, F.max_pool2d(3, 2, 1).  Reports the
         executed-MFMA fraction: executed MFMA FLOPs / (time x 65536 FLOP/clk x clock), at the clock a 1x1 GEMM
         launch stamps right after the stem's repetitions, and at the 2.4 GHz peak clock
       python tools/resnet_bench.py net [out.json] [--archs resnet18,resnet50] [--ns 1,32,128] [--trials 5] [--reps 5]
         whole forwards at 224x224, three ways interleaved: eager (one Python call per block), the same forward
         captured once in a torch.cuda.graph and replayed, and torch eager on channels-last fp32 with the same weights
       python tools/resnet_bench.py trace [--archs resnet18] [--ns 1] [--reps 20]
         eager forwards back to back -- run it under `rocprofv3 --kernel-trace --stats -- python ...` to see every
         launch of a forward, the stem's among them"""
import os

import benchlib
import torch
import torch.nn.functional as F
import torch_nets
from benchlib import FLOP_PER_CLK


def _stem_executed_flop(N, H, W, K, form):
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    tp, kc, rows = (8, 64, 19 * 16) if form == 1 else (4, 16, 6 * 16)
    wgs = N * -(-Hp // tp) * -(-Wp // tp) * (K // kc)
    return wgs * rows * kc * 148 * 2.0, N * Hc * Wc * K * 147 * 2.0


def stem(a, pkg, dev):
    rows = []
    L = pkg.lib()
    for N in benchlib.ints(a.ns):
        H = W = 224
        K = 64
        g = torch.Generator().manual_seed(N)
        x = (torch.rand(N, 3, H, W, generator=g) * 2 - 1).to(dev)
        w = ((torch.rand(K, 3, 7, 7, generator=g) - 0.5) * 0.3).to(dev)
        bias, scale = (torch.rand(K, generator=g) - 0.5).to(dev), (torch.rand(K, generator=g) + 0.5).to(dev)
        packed = pkg.stem_filter_pack(w, (bias, scale))
        out = torch.empty(N, 56, 56, K, device=dev)
        x_cl = x.contiguous(memory_format=torch.channels_last)
        w_cl = w.contiguous(memory_format=torch.channels_last)
        sc, bs = scale[None, :, None, None], bias[None, :, None, None]
        # a 1x1 GEMM launch long enough to stamp the clock the card holds under this load
        A = torch.rand(N * 3136, 64, device=dev)
        B = torch.rand(64, 256, device=dev)
        ob, os_ = torch.zeros(256, device=dev), torch.ones(256, device=dev)

        def form_knob(form):
            def setup():
                if form:
                    os.environ["WINO_STEM_FORM"] = str(form)
                else:
                    os.environ.pop("WINO_STEM_FORM", None)
                L.wino_debug_reload_knobs()
            return setup

        def run_stem():
            pkg.stem(x, packed, out=out)

        def torch_stem():
            y = F.conv2d(x_cl, w_cl, stride=2, padding=3)
            return F.max_pool2d(torch.relu(y * sc + bs), 3, 2, 1)

        variants = {"stem_auto": run_stem, "stem_big": run_stem, "stem_small": run_stem, "torch": torch_stem}
        setups = {"stem_auto": form_knob(0), "stem_big": form_knob(1), "stem_small": form_knob(2),
                  "torch": form_knob(0)}
        med, times = benchlib.interleaved(variants, a.trials, a.reps, setups)
        form_knob(0)()
        run_stem()
        pkg.conv1x1_bn(A, B, ob, os_, False)
        clk = pkg.last_clock_ghz(1)
        clock = clk[0] if clk else 2.4
        form = pkg.stem_plan(N, H, W, K)
        row = {"N": N, "H": H, "W": W, "K": K, "auto_form": form, "median_us": med, "trials_us": times,
               "stem_over_torch": med["stem_auto"] / med["torch"], "clock_ghz_1x1_stamp": clock}
        for name, f in (("big", 1), ("small", 2)):
            exe, alg = _stem_executed_flop(N, H, W, K, f)
            t = med[f"stem_{name}"] * 1e-6
            row[f"{name}_executed_gflop"] = exe / 1e9
            row[f"{name}_mfma_fraction"] = exe / (t * FLOP_PER_CLK * clock * 1e9)
            row[f"{name}_mfma_fraction_at_2.4ghz"] = exe / (t * FLOP_PER_CLK * 2.4e9)
            row[f"{name}_algorithmic_tflops"] = alg / t / 1e12
        rows.append(row)
        af = "big" if form == 1 else "small"
        print(f"stem N={N:4d} auto={af:5s} {med['stem_auto']:8.1f} us  big {med['stem_big']:8.1f}  small "
              f"{med['stem_small']:8.1f}  torch {med['torch']:8.1f}  /torch {row['stem_over_torch']:.3f}  "
              f"mfma frac ({af}) {row[af + '_mfma_fraction']:.3f} at {clock:.2f} GHz", flush=True)
        del x, out, x_cl, A
        torch.cuda.empty_cache()
    return rows


def net(a, pkg, dev):
    R = benchlib.package_module("resnet")
    rows = []
    for arch in a.archs.split(","):
        sd = torch_nets.random_state_dict(R, arch, seed=1)
        model = pkg.ResNet.from_state_dict(sd, arch)
        body = torch_nets.TorchResNetBody(R, sd, arch, dev)
        for N in benchlib.ints(a.ns):
            x, x_cl = torch_nets.image_batch(N, 224, 224, dev)
            graph, _ = benchlib.captured(lambda: model(x), lambda: model.prepare(N, 224, 224))
            variants = benchlib.net_variants(lambda: model(x), graph,
                                             lambda: torch_nets.classifier_head(body, body(x_cl)))
            med, times = benchlib.interleaved(variants, a.trials, a.reps)
            gflop = model.flops() * N / 1e9
            row = {"arch": arch, "N": N, "median_us": med, "trials_us": times, "gflop": gflop, **benchlib.net_ratios(med)}
            rows.append(row)
            print(f"{arch:9s} N={N:4d}  eager {med['eager']:9.1f} us  graph {med['graph']:9.1f} us  torch "
                  f"{med['torch']:9.1f} us  graph/eager {row['graph_over_eager']:.3f}  graph/torch "
                  f"{row['graph_over_torch']:.3f}  ({gflop / med['graph'] * 1e3:.1f} TF/s algorithmic, replayed)", flush=True)
            del graph, x, x_cl
            torch.cuda.empty_cache()
        del model, body
    return rows


def trace(a, pkg, dev):
    R = benchlib.package_module("resnet")
    for arch in a.archs.split(","):
        model = pkg.ResNet.from_state_dict(torch_nets.random_state_dict(R, arch, seed=1), arch)
        for N in benchlib.ints(a.ns):
            x = (torch.rand(N, 3, 224, 224) * 2 - 1).to(dev)
            for _ in range(a.reps):
                model(x)
            torch.cuda.synchronize()
            print(f"{arch} N={N}: {a.reps} eager forwards", flush=True)


MODES = {"stem": dict(fn=stem, ns="1,32,128", trials=7, reps=20),
         "net": dict(fn=net, archs="resnet18,resnet50", ns="1,32,128", trials=5, reps=5),
         "trace": dict(fn=trace, archs="resnet18", ns="1", reps=20)}


def main():
    benchlib.main_rows("tools/resnet_bench.py", MODES)


if __name__ == "__main__":
    main()

