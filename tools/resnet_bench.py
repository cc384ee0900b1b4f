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
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

FLOP_PER_CLK = 256 * 4 * 64   # CUs x SIMDs x f32 MFMA FLOP per clock per SIMD


def _time(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def _interleaved(variants, trials, reps, setups=None):
    setups = setups or {}
    for k, fn in variants.items():   # warm-up: plans, scratch, torch's algorithm choice
        setups.get(k, lambda: None)()
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(trials):
        for k, fn in variants.items():
            setups.get(k, lambda: None)()   # outside the timed repetitions
            times[k].append(_time(fn, reps))
    return {k: statistics.median(v) for k, v in times.items()}, times


def _stem_executed_flop(N, H, W, K, form):
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    tp, kc, rows = (8, 64, 19 * 16) if form == 1 else (4, 16, 6 * 16)
    wgs = N * -(-Hp // tp) * -(-Wp // tp) * (K // kc)
    return wgs * rows * kc * 148 * 2.0, N * Hc * Wc * K * 147 * 2.0


def stem(a, pkg, dev):
    rows = []
    L = pkg.lib()
    for N in (int(v) for v in a.ns.split(",")):
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
        med, times = _interleaved(variants, a.trials, a.reps, setups)
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


def random_state_dict(R, arch, seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in R.expected_keys(arch, 1000).items():
        if k.endswith(".weight") and len(shape) == 4:
            sd[k] = torch.randn(shape, generator=g) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
        elif k.endswith("running_var"):
            sd[k] = torch.rand(shape, generator=g) + 0.5
        elif k == "fc.weight":
            sd[k] = torch.randn(shape, generator=g) * (1.0 / shape[1]) ** 0.5
        elif k.endswith(".weight"):
            sd[k] = (torch.rand(shape, generator=g) + 0.5) * (0.2 if k.endswith(("bn3.weight",)) or
                                                               (k.endswith("bn2.weight") and "layer" in k and
                                                                not R.ARCHS[arch][0]) else 1.0)
        else:
            sd[k] = (torch.rand(shape, generator=g) - 0.5) * 0.2
    return sd


class TorchNet:
    """torch eager on channels-last fp32 with the same weights: conv, BN as scale and bias, ReLU, add."""

    def __init__(self, R, sd, arch, dev, eps=1e-5):
        self.bottleneck, self.blocks = R.ARCHS[arch]
        self.w = {k: v.to(dev).contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v.to(dev)
                  for k, v in sd.items()}
        self.bn = {}
        for k in sd:
            if k.endswith("running_var"):
                p = k[: -len(".running_var")]
                s = sd[p + ".weight"] / torch.sqrt(sd[k] + eps)
                self.bn[p] = (s.to(dev)[None, :, None, None], (sd[p + ".bias"] - sd[p + ".running_mean"] * s)
                              .to(dev)[None, :, None, None])

    def _cb(self, t, conv, bn, stride=1, pad=0, relu=True):
        s, b = self.bn[bn]
        y = F.conv2d(t, self.w[conv], stride=stride, padding=pad) * s + b
        return torch.relu(y) if relu else y

    def __call__(self, x):
        t = F.max_pool2d(self._cb(x, "conv1.weight", "bn1", 2, 3), 3, 2, 1)
        for L, nb in enumerate(self.blocks, 1):
            for b in range(nb):
                p = f"layer{L}.{b}"
                st = 2 if (b == 0 and L > 1) else 1
                if self.bottleneck:
                    y = self._cb(t, p + ".conv1.weight", p + ".bn1")
                    y = self._cb(y, p + ".conv2.weight", p + ".bn2", st, 1)
                    y = self._cb(y, p + ".conv3.weight", p + ".bn3", relu=False)
                else:
                    y = self._cb(t, p + ".conv1.weight", p + ".bn1", st, 1)
                    y = self._cb(y, p + ".conv2.weight", p + ".bn2", 1, 1, relu=False)
                sc = t
                if p + ".downsample.0.weight" in self.w:
                    sc = self._cb(t, p + ".downsample.0.weight", p + ".downsample.1", st, relu=False)
                t = torch.relu(y + sc)
        return F.linear(t.mean(dim=(2, 3)), self.w["fc.weight"], self.w["fc.bias"])


def net(a, pkg, dev):
    import importlib
    R = importlib.import_module("cuda_winograd_amd.resnet")
    rows = []
    for arch in a.archs.split(","):
        sd = random_state_dict(R, arch, seed=1)
        model = pkg.ResNet.from_state_dict(sd, arch)
        tnet = TorchNet(R, sd, arch, dev)
        for N in (int(v) for v in a.ns.split(",")):
            x = (torch.rand(N, 3, 224, 224, generator=torch.Generator().manual_seed(N)) * 2 - 1).to(dev)
            x_cl = x.contiguous(memory_format=torch.channels_last)
            sg = torch.cuda.Stream()
            sg.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(sg):
                model.prepare(N, 224, 224)
                model(x)
            sg.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=sg):
                model(x)
            torch.cuda.synchronize()
            variants = {"eager": lambda: model(x), "graph": graph.replay, "torch": lambda: tnet(x_cl)}
            med, times = _interleaved(variants, a.trials, a.reps)
            gflop = model.flops() * N / 1e9
            row = {"arch": arch, "N": N, "median_us": med, "trials_us": times, "gflop": gflop,
                   "graph_over_eager": med["graph"] / med["eager"], "graph_over_torch": med["graph"] / med["torch"],
                   "eager_over_torch": med["eager"] / med["torch"]}
            rows.append(row)
            print(f"{arch:9s} N={N:4d}  eager {med['eager']:9.1f} us  graph {med['graph']:9.1f} us  torch "
                  f"{med['torch']:9.1f} us  graph/eager {row['graph_over_eager']:.3f}  graph/torch "
                  f"{row['graph_over_torch']:.3f}  ({gflop / med['graph'] * 1e3:.1f} TF/s algorithmic, replayed)", flush=True)
            del graph, x, x_cl
            torch.cuda.empty_cache()
        del model, tnet
    return rows


def trace(a, pkg, dev):
    import importlib
    R = importlib.import_module("cuda_winograd_amd.resnet")
    for arch in a.archs.split(","):
        model = pkg.ResNet.from_state_dict(random_state_dict(R, arch, seed=1), arch)
        for N in (int(v) for v in a.ns.split(",")):
            x = (torch.rand(N, 3, 224, 224) * 2 - 1).to(dev)
            for _ in range(a.reps):
                model(x)
            torch.cuda.synchronize()
            print(f"{arch} N={N}: {a.reps} eager forwards", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["stem", "net", "trace"])
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--ns", default=None)
    ap.add_argument("--archs", default=None)
    ap.add_argument("--trials", type=int, default=None)
    ap.add_argument("--reps", type=int, default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    if a.mode == "stem":
        a.ns, a.trials, a.reps = a.ns or "1,32,128", a.trials or 7, a.reps or 20
        rows = stem(a, pkg, dev)
    elif a.mode == "net":
        a.ns, a.archs = a.ns or "1,32,128", a.archs or "resnet18,resnet50"
        a.trials, a.reps = a.trials or 5, a.reps or 5
        rows = net(a, pkg, dev)
    else:
        a.ns, a.archs, a.reps = a.ns or "1", a.archs or "resnet18", a.reps or 20
        trace(a, pkg, dev)
        return
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": f"tools/resnet_bench.py {a.mode}", "device": torch.cuda.get_device_name(0),
                       "trials": a.trials, "reps": a.reps, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
