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
import benchlib
import torch
import torch.nn.functional as F
import torch_nets
from benchlib import FORM_NAMES

# FCN-ResNet50's dilated 3x3 layers at 520x520: (name, H = W, C = K, dilation)
POINTS = [("layer3", 65, 256, 2), ("layer4.0", 65, 512, 2), ("layer4", 65, 512, 4)]


def layer(a, pkg, dev):
    rows = []
    for N in benchlib.ints(a.ns):
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
            med, times = benchlib.interleaved(variants, a.trials, a.reps)
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


def net(a, pkg, dev):
    R = benchlib.package_module("resnet")
    sd = torch_nets.fcn_state_dict(R, "resnet50")
    model = pkg.FCN.from_state_dict(sd, "resnet50")
    body = torch_nets.TorchResNetBody(R, sd, "resnet50", dev, prefix="backbone.", dilate=torch_nets.SEGMENTATION_DILATE)
    rows = []
    S = a.size
    for N in benchlib.ints(a.ns):
        x, x_cl = torch_nets.image_batch(N, S, S, dev)
        tnet = lambda: torch_nets.fcn_head(body, body(x_cl), (S, S))
        graph, first = benchlib.captured(lambda: model(x), lambda: model.prepare(N, S, S))
        mine, ref = first["out"], tnet()
        diff = float((mine - ref).abs().max() / ref.abs().max())
        med, times = benchlib.interleaved(benchlib.net_variants(lambda: model(x), graph, tnet), a.trials, a.reps)
        rows.append({"arch": "fcn_resnet50", "N": N, "size": S, "median_us": med, "trials_us": times,
                     "rel_diff_to_torch_fp32": diff, **benchlib.net_ratios(med)})
        print(f"fcn_resnet50 N={N:2d} {S}x{S}  eager {med['eager']:9.1f} us  graph {med['graph']:9.1f} us  torch "
              f"{med['torch']:9.1f} us  graph/torch {rows[-1]['graph_over_torch']:.3f}  eager/torch "
              f"{rows[-1]['eager_over_torch']:.3f}  (max rel diff to torch fp32 {diff:.1e})", flush=True)
        del graph, x, x_cl, first, mine, ref
        torch.cuda.empty_cache()
    return rows


MODES = {"layer": dict(fn=layer, ns="1,8", trials=7, reps=20),
         "net": dict(fn=net, ns="1,8", size=520, trials=5, reps=3),
         "all": ["layer", "net"]}


def main():
    a = benchlib.parse(MODES)
    result = benchlib.header(f"tools/dilated_bench.py {a.mode}")
    result.update(benchlib.sections(a, MODES, benchlib.load_package(), torch.device("cuda:0")))
    benchlib.write_json(a.out, result)


if __name__ == "__main__":
    main()
