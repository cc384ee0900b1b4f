"""Developer tool (GPU box): the FPN's top-down sum in the 1x1 epilogue, and whole ResNet-FPN backbones.
usage: python tools/fpn_bench.py lateral [out.json] [--n 2] [--hw 800,1344] [--trials 7] [--reps 20]
         ResNet-50-FPN's three top-down points (laterals 1024 / 512 / 256 -> 256 on the conv4 / conv3 / conv2 maps of an
         800 x 1344 input), in one process, the variants interleaved in every trial (median of the trials, events around
         `reps` calls):
         fused     the lateral with WINO_RESIDUAL_UP2: the coarser inner map added in the epilogue
         plain     the lateral alone (WINO_C_PADDED), no sum: what the fused launch is expected to cost
         composed  the best the library offered before: the plain lateral, then torch's F.interpolate(nearest) of the
                   coarser map and an in-place add on the interior view
         same_size the lateral with a same-size residual (WINO_ADD_RESIDUAL alone, a [N*H*W][256] tensor): the same
                   staged epilogue reading four times the residual bytes -- what of fused - plain is the epilogue's
       python tools/fpn_bench.py net [out.json] [--archs resnet50,resnet18] [--n 2] [--hw 800,1344] [--trials 5] [--reps 5]
         backbone + FPN three ways interleaved: eager, the same forward captured once in a torch.cuda.graph and
         replayed, and a torch fp32 channels-last composition with the same weights (conv, BN as scale and bias,
         F.interpolate, F.max_pool2d(1, 2))
Results under profiles/fpn/ (bench.json holds both modes' rows)."""
import argparse
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import __graft_entry__ as ge  # noqa: E402
from resnet_bench import TorchNet, _interleaved, random_state_dict  # noqa: E402

CF = 256


def lateral(a, pkg, dev):
    R = importlib.import_module("cuda_winograd_amd.resnet")
    N, (H0, W0) = a.n, a.hw
    stages = R.stage_shapes("resnet50", H0, W0)[1:]            # (name, C, h, w) of conv2..conv5
    rows = []
    for lvl in (2, 1, 0):
        _, Cin, H, W = stages[lvl]
        _, _, Hc, Wc = stages[lvl + 1]
        assert (Hc, Wc) == ((H + 1) // 2, (W + 1) // 2)
        g = torch.Generator().manual_seed(lvl)
        c = (torch.rand(N, H, W, Cin, generator=g) - 0.5).to(dev)
        wl = ((torch.rand(Cin, CF, generator=g) - 0.5) / Cin ** 0.5 * 4).to(dev)
        bl, ones = (torch.rand(CF, generator=g) - 0.5).to(dev), torch.ones(CF, device=dev)
        top = torch.zeros(N, Hc + 2, Wc + 2, CF)
        top[:, 1:-1, 1:-1, :] = torch.rand(N, Hc, Wc, CF, generator=g) - 0.5
        top = top.to(dev)
        inner = torch.empty(N, H + 2, W + 2, CF, device=dev)
        top_nchw = top[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2)   # (channels-last strides: no copy)
        interior = inner[:, 1:-1, 1:-1, :]
        res_same = (torch.rand(N * H * W, CF, generator=g) - 0.5).to(dev)
        pkg.conv1x1_prepare(N * H * W, Cin, CF)
        UP = pkg.C_PADDED | pkg.ADD_RESIDUAL | pkg.RESIDUAL_UP2

        def fused():
            pkg.conv1x1_bn_ex(c, wl, bl, ones, UP, residual=top, out=inner)

        def plain():
            pkg.conv1x1_bn_ex(c, wl, bl, ones, pkg.C_PADDED, out=inner)

        def composed():
            plain()
            interior.add_(F.interpolate(top_nchw, size=(H, W), mode="nearest").permute(0, 2, 3, 1))

        def same_size():
            pkg.conv1x1_bn_ex(c, wl, bl, ones, pkg.C_PADDED | pkg.ADD_RESIDUAL, residual=res_same, out=inner, hw=(H, W))

        fused()
        want = inner.clone()
        composed()
        torch.cuda.synchronize()
        assert float((inner - want).abs().max()) < 1e-5, "the fused launch and the composition disagree"
        med, times = _interleaved({"fused": fused, "plain": plain, "composed": composed, "same_size": same_size},
                                  a.trials, a.reps)
        row = {"level": lvl, "N": N, "H": H, "W": W, "Cin": Cin, "Cf": CF, "median_us": med, "trials_us": times,
               "fused_over_plain": med["fused"] / med["plain"], "fused_over_composed": med["fused"] / med["composed"],
               "same_size_over_plain": med["same_size"] / med["plain"]}
        rows.append(row)
        print(f"level {lvl} {H:3d}x{W:3d} {Cin:4d}->{CF}  fused {med['fused']:8.1f} us  plain {med['plain']:8.1f}  "
              f"composed {med['composed']:8.1f}  same-size {med['same_size']:8.1f}  fused/plain {row['fused_over_plain']:.3f}  fused/composed "
              f"{row['fused_over_composed']:.3f}", flush=True)
        del c, top, inner, want, res_same
        torch.cuda.empty_cache()
    return rows


def fpn_state_dict(R, arch, seed=1):
    body = random_state_dict(R, arch, seed=seed)
    sd = {"body." + k: v for k, v in body.items() if not k.startswith("fc.")}
    g = torch.Generator().manual_seed(seed + 1)
    for i, (_, c, _, _) in enumerate(R.stage_shapes(arch, 64, 64)[1:]):
        sd[f"fpn.inner_blocks.{i}.0.weight"] = torch.randn(CF, c, 1, 1, generator=g) * (1.0 / c) ** 0.5
        sd[f"fpn.inner_blocks.{i}.0.bias"] = (torch.rand(CF, generator=g) - 0.5) * 0.2
        sd[f"fpn.layer_blocks.{i}.0.weight"] = torch.randn(CF, CF, 3, 3, generator=g) * (1.0 / (9 * CF)) ** 0.5
        sd[f"fpn.layer_blocks.{i}.0.bias"] = (torch.rand(CF, generator=g) - 0.5) * 0.2
    return sd, body


class TorchFPN(TorchNet):
    """torch eager on channels-last fp32 with the same weights: the body of resnet_bench.TorchNet, then
    torchvision's FeaturePyramidNetwork and LastLevelMaxPool written out."""

    def __init__(self, R, sd, body, arch, dev):
        super().__init__(R, body, arch, dev)
        self.f = {k: v.to(dev).contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v.to(dev)
                  for k, v in sd.items() if k.startswith("fpn.")}

    def __call__(self, x):
        t = F.max_pool2d(self._cb(x, "conv1.weight", "bn1", 2, 3), 3, 2, 1)
        c = []
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
            c.append(t)
        f = self.f
        last = F.conv2d(c[3], f["fpn.inner_blocks.3.0.weight"], f["fpn.inner_blocks.3.0.bias"])
        out = [None, None, None, F.conv2d(last, f["fpn.layer_blocks.3.0.weight"], f["fpn.layer_blocks.3.0.bias"], padding=1)]
        for i in (2, 1, 0):
            lat = F.conv2d(c[i], f[f"fpn.inner_blocks.{i}.0.weight"], f[f"fpn.inner_blocks.{i}.0.bias"])
            last = lat + F.interpolate(last, size=lat.shape[-2:], mode="nearest")
            out[i] = F.conv2d(last, f[f"fpn.layer_blocks.{i}.0.weight"], f[f"fpn.layer_blocks.{i}.0.bias"], padding=1)
        return out + [F.max_pool2d(out[3], 1, 2, 0)]


def net(a, pkg, dev):
    R = importlib.import_module("cuda_winograd_amd.resnet")
    N, (H, W) = a.n, a.hw
    rows = []
    for arch in a.archs.split(","):
        sd, body = fpn_state_dict(R, arch)
        model = pkg.ResNetFPN.from_state_dict(sd, arch, out_channels=CF)
        tnet = TorchFPN(R, sd, body, arch, dev)
        x = (torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(N)) * 2 - 1).to(dev)
        x_cl = x.contiguous(memory_format=torch.channels_last)
        sg = torch.cuda.Stream()
        sg.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(sg):
            model.prepare(N, H, W)
            got = model(x)
        sg.synchronize()
        want = tnet(x_cl)
        errs = {k: float((got[k].permute(0, 3, 1, 2) - w).abs().max() / w.abs().max())
                for k, w in zip(("0", "1", "2", "3", "pool"), want)}
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=sg):
            model(x)
        torch.cuda.synchronize()
        med, times = _interleaved({"eager": lambda: model(x), "graph": graph.replay, "torch": lambda: tnet(x_cl)},
                                  a.trials, a.reps)
        row = {"arch": arch, "N": N, "H": H, "W": W, "median_us": med, "trials_us": times,
               "max_rel_diff_vs_torch_fp32": errs, "graph_over_eager": med["graph"] / med["eager"],
               "graph_over_torch": med["graph"] / med["torch"], "eager_over_torch": med["eager"] / med["torch"]}
        rows.append(row)
        print(f"{arch:9s}-fpn N={N} {H}x{W}  eager {med['eager']:9.1f} us  graph {med['graph']:9.1f} us  torch "
              f"{med['torch']:9.1f} us  graph/torch {row['graph_over_torch']:.3f}  max rel diff vs torch "
              f"{max(errs.values()):.1e}", flush=True)
        del graph, model, tnet, x, x_cl, got, want
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["lateral", "net"])
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--n", type=int, default=2)
    ap.add_argument("--hw", default="800,1344")
    ap.add_argument("--archs", default="resnet50,resnet18")
    ap.add_argument("--trials", type=int, default=None)
    ap.add_argument("--reps", type=int, default=None)
    a = ap.parse_args()
    a.hw = tuple(int(v) for v in a.hw.split(","))
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    if a.mode == "lateral":
        a.trials, a.reps = a.trials or 7, a.reps or 20
        rows = lateral(a, pkg, dev)
    else:
        a.trials, a.reps = a.trials or 5, a.reps or 5
        rows = net(a, pkg, dev)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        doc = {}
        if os.path.exists(a.out):   # one file for both modes: the other mode's rows stay
            with open(a.out) as f:
                doc = json.load(f)
        doc.update({"tool": "tools/fpn_bench.py", "device": torch.cuda.get_device_name(0),
                    a.mode: {"trials": a.trials, "reps": a.reps, "rows": rows}})
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
