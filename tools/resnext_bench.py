"""Developer tool (GPU box): the grouped 3x3 layer and whole ResNeXt / Wide-ResNet forwards.
usage: python tools/resnext_bench.py layer [out.json] [--ns 128,1] [--trials 7] [--reps 20]
         the grouped layer (wino_conv3x3_grouped_bn_relu_hw) at the seven (shape, stride) points of ResNeXt-50 32x4d's
         3x3 layers, in one process, interleaved in every trial with torch's F.conv2d(groups=32) on channels-last fp32
         with BN as scale and bias and the ReLU (median of the trials, events around `reps` calls).  Reports the
         layer's two floors: the HBM time of reading and writing the activation once at 6.3 TB/s, and the executed-MFMA
         time (max(Cg, 16) / Cg times the useful work, tiles counted whole) at 65536 FLOP/clk and 2.4 GHz
       python tools/resnext_bench.py net [out.json] [--archs resnext50_32x4d,wide_resnet50_2] [--ns 128,1] [--trials 5]
                                         [--reps 3]
         whole forwards at 224x224, three ways interleaved: eager, one torch.cuda.graph replay, and torch eager on
         channels-last fp32 with the same weights
       python tools/resnext_bench.py trace [--ns 128] [--reps 10]
         the seven layer points back to back -- run it under `rocprofv3 --kernel-trace --stats -- python ...`"""
import benchlib
import torch
import torch.nn.functional as F
import torch_nets
from benchlib import FLOP_PER_CLK

HBM_BYTES_PER_S = 6.3e12
PEAK_CLOCK_HZ = 2.4e9
GROUPS = 32
# ResNeXt-50 32x4d's 3x3 layers: (name, Hin, C, stride); Cg = C / 32 = 4, 8, 16, 32
POINTS = [("conv2", 56, 128, 1), ("conv3.0", 56, 256, 2), ("conv3", 28, 256, 1), ("conv4.0", 28, 512, 2),
          ("conv4", 14, 512, 1), ("conv5.0", 14, 1024, 2), ("conv5", 7, 1024, 1)]


def _floors(N, Hin, C, stride):
    """(HBM seconds, executed-MFMA seconds, algorithmic FLOPs) of one layer call."""
    H = (Hin - 1) // stride + 1
    Cg = C // GROUPS
    hbm = 4.0 * N * C * ((Hin + 2) ** 2 + (H + 2) ** 2) / HBM_BYTES_PER_S
    tw = 8 if -(-H // 8) * 8 < -(-H // 16) * 16 else 16            # the kernel's tile: conv3x3_grouped.hip
    oh = (4 if stride == 1 else 2) * (16 // tw)
    pixels = N * -(-H // oh) * oh * -(-H // tw) * tw                # whole tiles
    executed = 2.0 * pixels * C * 9 * max(Cg, 16)
    return hbm, executed / (FLOP_PER_CLK * PEAK_CLOCK_HZ), 2.0 * N * H * H * C * 9 * Cg


def _layer_tensors(pkg, dev, N, Hin, C, stride):
    g = torch.Generator().manual_seed(Hin + C)
    H = (Hin - 1) // stride + 1
    Cg = C // GROUPS
    x = torch.zeros(N, Hin + 2, Hin + 2, C)
    x[:, 1:-1, 1:-1, :] = torch.rand(N, Hin, Hin, C, generator=g) - 0.5
    w = ((torch.rand(C, Cg, 3, 3, generator=g) - 0.5) * (4.0 / (9 * Cg) ** 0.5)).to(dev)
    bias, scale = (torch.rand(C, generator=g) - 0.5).to(dev), (torch.rand(C, generator=g) + 0.5).to(dev)
    x = x.to(dev)
    return x, w, bias, scale, pkg.filter_pack_grouped(w, GROUPS), torch.empty(N, H + 2, H + 2, C, device=dev)


def layer(a, pkg, dev):
    rows = []
    for N in benchlib.ints(a.ns):
        for name, Hin, C, stride in POINTS:
            x, w, bias, scale, packed, out = _layer_tensors(pkg, dev, N, Hin, C, stride)
            # torch: the unpadded map as a channels-last NCHW view, pad = 1 inside the conv
            x_cl = x[:, 1:-1, 1:-1, :].contiguous().permute(0, 3, 1, 2)
            w_cl = w.contiguous(memory_format=torch.channels_last)
            sc, bs = scale[None, :, None, None], bias[None, :, None, None]

            def mine():
                pkg.conv3x3_grouped_bn_relu(x, packed, bias, scale, GROUPS, stride=stride, out=out)

            def torch_layer():
                return torch.relu(F.conv2d(x_cl, w_cl, stride=stride, padding=1, groups=GROUPS) * sc + bs)

            med, times = benchlib.interleaved({"grouped": mine, "torch": torch_layer}, a.trials, a.reps)
            hbm, mfma, alg = _floors(N, Hin, C, stride)
            t = med["grouped"] * 1e-6
            rows.append({"point": name, "N": N, "Hin": Hin, "C": C, "Cg": C // GROUPS, "stride": stride,
                         "median_us": med, "trials_us": times, "grouped_over_torch": med["grouped"] / med["torch"],
                         "hbm_floor_us": hbm * 1e6, "mfma_floor_us": mfma * 1e6, "hbm_fraction": hbm / t,
                         "mfma_fraction_at_2.4ghz": mfma / t, "algorithmic_tflops": alg / t / 1e12})
            print(f"{name:8s} N={N:4d} {Hin:3d}x{Hin:<3d} C={C:5d} Cg={C // GROUPS:3d} s={stride}  grouped "
                  f"{med['grouped']:9.1f} us  torch {med['torch']:9.1f} us  /torch {rows[-1]['grouped_over_torch']:.3f}  "
                  f"floors: hbm {hbm * 1e6:7.1f} us ({hbm / t:.2f})  mfma {mfma * 1e6:7.1f} us ({mfma / t:.2f})", flush=True)
            del x, out, x_cl
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
            rows.append({"arch": arch, "N": N, "median_us": med, "trials_us": times, "gflop": gflop,
                         **benchlib.net_ratios(med)})
            print(f"{arch:16s} N={N:4d}  eager {med['eager']:9.1f} us  graph {med['graph']:9.1f} us  torch "
                  f"{med['torch']:9.1f} us  graph/torch {rows[-1]['graph_over_torch']:.3f}  eager/torch "
                  f"{rows[-1]['eager_over_torch']:.3f}  ({gflop / med['graph'] * 1e3:.1f} TF/s algorithmic, replayed)", flush=True)
            del graph, x, x_cl
            torch.cuda.empty_cache()
        del model, body
    return rows


def trace(a, pkg, dev):
    for N in benchlib.ints(a.ns):
        for name, Hin, C, stride in POINTS:
            x, w, bias, scale, packed, out = _layer_tensors(pkg, dev, N, Hin, C, stride)
            for _ in range(a.reps):
                pkg.conv3x3_grouped_bn_relu(x, packed, bias, scale, GROUPS, stride=stride, out=out)
            torch.cuda.synchronize()
            print(f"{name} N={N}: {a.reps} launches", flush=True)


MODES = {"layer": dict(fn=layer, ns="128,1", trials=7, reps=20),
         "net": dict(fn=net, archs="resnext50_32x4d,wide_resnet50_2", ns="128,1", trials=5, reps=3),
         "trace": dict(fn=trace, ns="128", reps=10)}


def main():
    benchlib.main_rows("tools/resnext_bench.py", MODES)


if __name__ == "__main__":
    main()
