"""Developer tool (GPU box): the dilated 3x3 layer and a whole FCN-ResNet50 forward.
usage: python tools/dilated_bench.py layer [out.json] [--ns 1,8] [--trials 7] [--reps 20]
         the dilated layer (wino_conv3x3_dilated_bn_relu_hw) at the three (map, channels, dilation) points of
         FCN-ResNet50's layer3 / layer4 at a 520x520 input, in one process, interleaved in every trial with
           torch     F.conv2d(padding=d, dilation=d) on channels-last fp32 with BN as scale and bias and the ReLU
           winograd  the Winograd layer at the same shape (dilation 1): the price of having no Winograd form
           taps      the stride-2 layer (operand form A_TAPS) at the same GEMM shape (M, 9C, K): a 129x129 input, the
                     same K loop with scalar tap offsets; its planned form is reported beside the dilated layer's
         (median of the trials, events around `reps` calls)
       python tools/dilated_bench.py net [out.json] [--ns 1,8] [--trials 5] [--reps 3] [--size 520]
         whole FCN-ResNet50 forwards, three ways interleaved: eager, one torch.cuda.graph replay, and torch eager on
         channels-last fp32 with the same weights
       python tools/dilated_bench.py all profiles/dilated/bench.json
         both, into one file"""
import argparse
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import __graft_entry__ as ge  # noqa: E402
from resnet_bench import _interleaved, random_state_dict  # noqa: E402

# FCN-ResNet50's dilated 3x3 layers at 520x520: (name, H = W, C = K, dilation)
POINTS = [("layer3", 65, 256, 2), ("layer4.0", 65, 512, 2), ("layer4", 65, 512, 4)]
FORM_NAMES = {0: "tiled", 1: "stream_k", 2: "latency"}
DILATE = (False, True, True)


def layer(a, pkg, dev):
    rows = []
    for N in (int(v) for v in a.ns.split(",")):
        for name, H, C, d in POINTS:
            g = torch.Generator().manual_seed(H + C + d)
            x = torch.zeros(N, H + 2, H + 2, C)
            x[:, 1:-1, 1:-1, :] = torch.rand(N, H, H, C, generator=g) - 0.5
            x = x.to(dev)
            w = ((torch.rand(C, C, 3, 3, generator=g) - 0.5) * (4.0 / (9 * C) ** 0.5)).to(dev)
            bias, scale = (torch.rand(C, generator=g) - 0.5).to(dev), (torch.rand(C, generator=g) + 0.5).to(dev)
            taps, U = pkg.filter_pack_s2(w), pkg.filter_transform_f2(w)
            out = torch.empty(N, H + 2, H + 2, C, device=dev)
            out_w, out_t = torch.empty_like(out), torch.empty_like(out)
            Hin = 2 * H - 1                                        # the stride-2 layer with an H x H output
            x2 = torch.zeros(N, Hin + 2, Hin + 2, C, device=dev)
            x2[:, 1:-1, 1:-1, :] = torch.rand(N, Hin, Hin, C, device=dev) - 0.5
            x_cl = x[:, 1:-1, 1:-1, :].contiguous().permute(0, 3, 1, 2)
            w_cl = w.contiguous(memory_format=torch.channels_last)
            sc, bs = scale[None, :, None, None], bias[None, :, None, None]
            variants = {
                "dilated": lambda: pkg.conv3x3_dilated_bn_relu(x, taps, bias, scale, d, out=out),
                "torch": lambda: torch.relu(F.conv2d(x_cl, w_cl, padding=d, dilation=d) * sc + bs),
                "winograd": lambda: pkg.conv3x3_bn_relu(x, U, bias, scale, out=out_w),
                "taps": lambda: pkg.conv3x3_s2_bn_relu(x2, taps, bias, scale, out=out_t),
            }
            med, times = _interleaved(variants, a.trials, a.reps)
            forms = {"dilated": FORM_NAMES[pkg.conv3x3_dilated_plan(N, H, H, C, C, d)],
                     "taps": FORM_NAMES[pkg.conv3x3_s2_plan(N, Hin, Hin, C, C)]}
            flop = 2.0 * N * H * H * 9 * C * C
            rows.append({"point": name, "N": N, "H": H, "C": C, "dilation": d, "median_us": med, "trials_us": times,
                         "forms": forms, "dilated_over_torch": med["dilated"] / med["torch"],
                         "dilated_over_winograd": med["dilated"] / med["winograd"],
                         "dilated_over_taps": med["dilated"] / med["taps"],
                         "algorithmic_tflops": flop / med["dilated"] / 1e6})
            r = rows[-1]
            print(f"{name:9s} N={N:2d} {H}x{H} C={C:4d} d={d}  dilated {med['dilated']:8.1f} us ({forms['dilated']})  torch "
                  f"{med['torch']:8.1f}  winograd {med['winograd']:8.1f}  taps {med['taps']:8.1f} ({forms['taps']})  "
                  f"/torch {r['dilated_over_torch']:.3f}  /winograd {r['dilated_over_winograd']:.3f}  /taps "
                  f"{r['dilated_over_taps']:.3f}  {r['algorithmic_tflops']:.1f} TF/s", flush=True)
            del x, x2, out, out_w, out_t, x_cl
            torch.cuda.empty_cache()
    return rows


class TorchFCN:
    """torch eager on channels-last fp32 with the same weights: conv, BN as scale and bias, ReLU, add, the FCN head and
    the bilinear resize."""

    def __init__(self, R, sd, arch, dev, eps=1e-5):
        self.blocks = R.ARCHS[arch][1]
        self.w = {k: v.to(dev).contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v.to(dev)
                  for k, v in sd.items() if v.dim() > 0}
        self.bn = {}
        for k in sd:
            if k.endswith("running_var"):
                p = k[: -len(".running_var")]
                s = sd[p + ".weight"] / torch.sqrt(sd[k] + eps)
                self.bn[p] = (s.to(dev)[None, :, None, None], (sd[p + ".bias"] - sd[p + ".running_mean"] * s)
                              .to(dev)[None, :, None, None])

    def _cb(self, t, conv, bn, stride=1, pad=0, dil=1, relu=True):
        s, b = self.bn[bn]
        y = F.conv2d(t, self.w[conv], stride=stride, padding=pad, dilation=dil) * s + b
        return torch.relu(y) if relu else y

    def __call__(self, x):
        q = "backbone."
        t = F.max_pool2d(self._cb(x, q + "conv1.weight", q + "bn1", 2, 3), 3, 2, 1)
        plan = importlib.import_module("cuda_winograd_amd.resnet").dilated_block_plan(DILATE, self.blocks)
        for L, stage in enumerate(plan, 1):
            for b, (kind, d) in enumerate(stage):
                p = f"{q}layer{L}.{b}"
                st = 2 if kind == "proj_v15" else 1
                y = self._cb(t, p + ".conv1.weight", p + ".bn1")
                y = self._cb(y, p + ".conv2.weight", p + ".bn2", st, d, d)
                y = self._cb(y, p + ".conv3.weight", p + ".bn3", relu=False)
                sc = self._cb(t, p + ".downsample.0.weight", p + ".downsample.1", st, relu=False) if b == 0 else t
                t = torch.relu(y + sc)
        t = self._cb(t, "classifier.0.weight", "classifier.1", 1, 1)
        t = F.conv2d(t, self.w["classifier.4.weight"], self.w["classifier.4.bias"])
        return F.interpolate(t, size=x.shape[-2:], mode="bilinear", align_corners=False)


def fcn_state_dict(R, arch, classes=21, seed=1):
    g = torch.Generator().manual_seed(seed + 100)
    sd = {"backbone." + k: v for k, v in random_state_dict(R, arch, seed).items() if not k.startswith("fc.")}
    sd["classifier.0.weight"] = torch.randn(512, 2048, 3, 3, generator=g) * (2.0 / (2048 * 9)) ** 0.5
    sd["classifier.1.weight"] = torch.rand(512, generator=g) + 0.5
    sd["classifier.1.bias"] = (torch.rand(512, generator=g) - 0.5) * 0.2
    sd["classifier.1.running_mean"] = (torch.rand(512, generator=g) - 0.5) * 0.2
    sd["classifier.1.running_var"] = torch.rand(512, generator=g) + 0.5
    sd["classifier.4.weight"] = torch.randn(classes, 512, 1, 1, generator=g) * (1.0 / 512) ** 0.5
    sd["classifier.4.bias"] = torch.rand(classes, generator=g) - 0.5
    return sd


def net(a, pkg, dev):
    R = importlib.import_module("cuda_winograd_amd.resnet")
    sd = fcn_state_dict(R, "resnet50")
    model = pkg.FCN.from_state_dict(sd, "resnet50")
    tnet = TorchFCN(R, sd, "resnet50", dev)
    rows = []
    S = a.size
    for N in (int(v) for v in a.ns.split(",")):
        x = (torch.rand(N, 3, S, S, generator=torch.Generator().manual_seed(N)) * 2 - 1).to(dev)
        x_cl = x.contiguous(memory_format=torch.channels_last)
        sg = torch.cuda.Stream()
        sg.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(sg):
            model.prepare(N, S, S)
            mine = model(x)["out"]
        sg.synchronize()
        ref = tnet(x_cl)
        diff = float((mine - ref).abs().max() / ref.abs().max())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=sg):
            model(x)
        torch.cuda.synchronize()
        variants = {"eager": lambda: model(x), "graph": graph.replay, "torch": lambda: tnet(x_cl)}
        med, times = _interleaved(variants, a.trials, a.reps)
        rows.append({"arch": "fcn_resnet50", "N": N, "size": S, "median_us": med, "trials_us": times,
                     "rel_diff_to_torch_fp32": diff, "graph_over_eager": med["graph"] / med["eager"],
                     "graph_over_torch": med["graph"] / med["torch"], "eager_over_torch": med["eager"] / med["torch"]})
        print(f"fcn_resnet50 N={N:2d} {S}x{S}  eager {med['eager']:9.1f} us  graph {med['graph']:9.1f} us  torch "
              f"{med['torch']:9.1f} us  graph/torch {rows[-1]['graph_over_torch']:.3f}  eager/torch "
              f"{rows[-1]['eager_over_torch']:.3f}  (max rel diff to torch fp32 {diff:.1e})", flush=True)
        del graph, x, x_cl, mine, ref
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["layer", "net", "all"])
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--ns", default="1,8")
    ap.add_argument("--size", type=int, default=520)
    ap.add_argument("--trials", type=int, default=None)
    ap.add_argument("--reps", type=int, default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    result = {"tool": f"tools/dilated_bench.py {a.mode}", "device": torch.cuda.get_device_name(0)}
    trials, reps = a.trials, a.reps
    if a.mode in ("layer", "all"):
        a.trials, a.reps = trials or 7, reps or 20
        result["layer"] = {"trials": a.trials, "reps": a.reps, "rows": layer(a, pkg, dev)}
    if a.mode in ("net", "all"):
        a.trials, a.reps = trials or 5, reps or 3
        result["net"] = {"trials": a.trials, "reps": a.reps, "rows": net(a, pkg, dev)}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
