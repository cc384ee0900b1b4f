"""Developer tool (GPU box): the concat projection, the ASPP module and a whole DeepLabV3-ResNet50 forward.
usage: python tools/aspp_bench.py cat [out.json] [--ns 1,8] [--trials 7] [--reps 20]
         the concat layer (wino_conv1x1_cat_bn_hw, operand form A_CAT) at DeepLabV3's join -- four 65x65x256 sources to
         256 channels, the per-image bias, ReLU, padded output -- in one process, interleaved in every trial with
           cat_plain  torch.cat of the four maps, then the plain 1x1 layer on the copy (bias of image 0: the plain
                      layer has one bias row), the composition the form replaces
           plain      that plain 1x1 alone on a ready-made copy: the GEMM without the cat
         (median of the trials, events around `reps` calls)
       python tools/aspp_bench.py module [out.json] [--ns 1,8] [--trials 5] [--reps 5]
         the ASPP module (wino_aspp_hw, 2048 -> 5 x 256 -> 256 at 65x65, rates 12, 24, 36) against a torch fp32
         composition on channels-last tensors (conv2d, adaptive_avg_pool2d, expand, cat, conv2d, BN as scale and bias)
       python tools/aspp_bench.py net [out.json] [--ns 1,8] [--trials 5] [--reps 3] [--size 520]
         whole DeepLabV3-ResNet50 forwards, three ways interleaved: eager, one torch.cuda.graph replay, and torch eager
         on channels-last fp32 with the same weights
       python tools/aspp_bench.py parts [out.json] [--ns 1,8] [--trials 5] [--reps 10]
         the module's launches one by one at the same point, through the layers' own wrappers: branch 0, the three dilated
         branches (into padded outputs: the module's skip the ring pass), the join, and the average pool with a 1x1 of N
         rows behind it (avgpool_fc: the module runs the same pool and two such 1x1 layers)
       python tools/aspp_bench.py all profiles/aspp/bench.json
         cat, module and net, into one file"""
import benchlib
import torch
import torch.nn.functional as F
import torch_nets
from benchlib import FORM_NAMES

H = 65                  # layer4's map at a 520x520 input
CIN, CB, RATES = torch_nets.ASPP_CIN, torch_nets.ASPP_CB, torch_nets.ASPP_RATES   # 2048 -> 256, rates 12, 24, 36
RELU, A_PADDED, C_PADDED = 1, 2, 4


def cat(a, pkg, dev):
    rows = []
    S, K = 4, CB
    for N in benchlib.ints(a.ns):
        g = torch.Generator().manual_seed(N)
        srcs = (torch.rand(S, N, H, H, CB, generator=g) - 0.5).to(dev)
        w = ((torch.rand(S * CB, K, generator=g) - 0.5) * (4.0 / (S * CB) ** 0.5)).to(dev)
        bias, scale = (torch.rand(N, K, generator=g) - 0.5).to(dev), (torch.rand(K, generator=g) + 0.5).to(dev)
        out, out_p = torch.empty(N, H + 2, H + 2, K, device=dev), torch.empty(N, H + 2, H + 2, K, device=dev)
        copy = torch.cat(list(srcs), dim=-1)
        pkg.conv1x1_cat_prepare(N, H, H, S, CB, K)
        pkg.conv1x1_prepare(N * H * H, S * CB, K)
        plain = lambda t: pkg.conv1x1_bn_ex(t, w, bias[0], scale, RELU | C_PADDED, out=out_p)
        variants = {
            "cat_form": lambda: pkg.conv1x1_cat_bn(srcs, w, bias, scale, RELU | C_PADDED, out=out),
            "cat_plain": lambda: plain(torch.cat(list(srcs), dim=-1)),
            "plain": lambda: plain(copy),
        }
        med, times = benchlib.interleaved(variants, a.trials, a.reps)
        form = FORM_NAMES[pkg.conv1x1_cat_plan(N, H, H, S, CB, K)]
        rows.append({"N": N, "H": H, "sources": S, "Cs": CB, "Kout": K, "form": form, "median_us": med, "trials_us": times,
                     "cat_form_over_cat_plain": med["cat_form"] / med["cat_plain"],
                     "cat_form_over_plain": med["cat_form"] / med["plain"]})
        r = rows[-1]
        print(f"join N={N:2d} {H}x{H} {S}x{CB}->{K}  cat form {med['cat_form']:8.1f} us ({form})  cat+plain "
              f"{med['cat_plain']:8.1f}  plain alone {med['plain']:8.1f}  /cat+plain {r['cat_form_over_cat_plain']:.3f}  "
              f"/plain {r['cat_form_over_plain']:.3f}", flush=True)
        del srcs, copy, out, out_p
        torch.cuda.empty_cache()
    return rows


def module(a, pkg, dev):
    rows = []
    for N in benchlib.ints(a.ns):
        g = torch.Generator().manual_seed(N + 7)
        r = lambda *s: torch.rand(*s, generator=g) - 0.5
        x = torch.zeros(N, H + 2, H + 2, CIN)
        x[:, 1:-1, 1:-1, :] = r(N, H, H, CIN)
        x = x.to(dev)
        w0, w_pool = (r(CIN, CB) * (4.0 / CIN ** 0.5)).to(dev), (r(CIN, CB) * (4.0 / CIN ** 0.5)).to(dev)
        ws = [(r(CB, CIN, 3, 3) * (4.0 / (9 * CIN) ** 0.5)).to(dev) for _ in range(3)]
        w_proj = (r(5 * CB, CB) * (4.0 / (5 * CB) ** 0.5)).to(dev)
        bn = [(r(CB).to(dev), (r(CB) + 1.0).to(dev)) for _ in range(6)]
        taps = [pkg.filter_pack_s2(w) for w in ws]
        out = torch.empty(N, H + 2, H + 2, CB, device=dev)
        wsp = torch.empty(pkg.aspp_workspace_bytes(N, H, H, CIN, CB, CB) // 4, device=dev)
        pkg.aspp_prepare(N, H, H, CIN, CB, CB, RATES)
        x_cl = x[:, 1:-1, 1:-1, :].contiguous().permute(0, 3, 1, 2)
        cl = lambda t: t.contiguous(memory_format=torch.channels_last)
        mat = lambda m: cl(m.t().contiguous()[:, :, None, None])
        tw0, twp, twproj, tws = mat(w0), mat(w_pool), mat(w_proj), [cl(w) for w in ws]
        act = lambda t, p: torch.relu(t * p[1][None, :, None, None] + p[0][None, :, None, None])

        def torch_aspp():
            b = [act(F.conv2d(x_cl, tw0), bn[0])]
            for w, p, d in zip(tws, bn[1:4], RATES):
                b.append(act(F.conv2d(x_cl, w, padding=d, dilation=d), p))
            pooled = act(F.conv2d(F.adaptive_avg_pool2d(x_cl, 1), twp), bn[4])
            b.append(pooled.expand(-1, -1, H, H))
            return act(F.conv2d(torch.cat(b, dim=1), twproj), bn[5])

        mine = lambda: pkg.aspp(x, w0, bn[0], taps, bn[1:4], RATES, w_pool, bn[4], w_proj, bn[5], out=out, workspace=wsp)
        ref = torch_aspp().permute(0, 2, 3, 1)
        diff = float((mine()[:, 1:-1, 1:-1, :] - ref).abs().max() / ref.abs().max())
        med, times = benchlib.interleaved({"aspp": mine, "torch": torch_aspp}, a.trials, a.reps)
        flop = 2.0 * N * H * H * CB * (CIN * 28 + 4 * CB)
        rows.append({"N": N, "H": H, "Cin": CIN, "Cb": CB, "rates": RATES, "median_us": med, "trials_us": times,
                     "rel_diff_to_torch_fp32": diff, "aspp_over_torch": med["aspp"] / med["torch"],
                     "algorithmic_tflops": flop / med["aspp"] / 1e6})
        print(f"aspp N={N:2d} {H}x{H} {CIN}->5x{CB}->{CB}  module {med['aspp']:9.1f} us  torch {med['torch']:9.1f} us  "
              f"/torch {rows[-1]['aspp_over_torch']:.3f}  {rows[-1]['algorithmic_tflops']:.1f} TF/s  (max rel diff {diff:.1e})",
              flush=True)
        del x, x_cl, out, wsp, ref
        torch.cuda.empty_cache()
    return rows


def parts(a, pkg, dev):
    rows = []
    for N in benchlib.ints(a.ns):
        g = torch.Generator().manual_seed(N + 11)
        r = lambda *s: torch.rand(*s, generator=g) - 0.5
        x = torch.zeros(N, H + 2, H + 2, CIN)
        x[:, 1:-1, 1:-1, :] = r(N, H, H, CIN)
        x = x.to(dev)
        w0 = (r(CIN, CB) * (4.0 / CIN ** 0.5)).to(dev)
        taps = pkg.filter_pack_s2((r(CB, CIN, 3, 3) * (4.0 / (9 * CIN) ** 0.5)).to(dev))
        b, s = r(CB).to(dev), (r(CB) + 1.0).to(dev)
        o_un, o_p = torch.empty(N, H, H, CB, device=dev), torch.empty(N, H + 2, H + 2, CB, device=dev)
        srcs, w_proj = r(4, N, H, H, CB).to(dev), (r(4 * CB, CB) * (4.0 / (4 * CB) ** 0.5)).to(dev)
        bias = r(N, CB).to(dev)
        head, logits = pkg.head_pack((r(CB, CIN) * 0.1).to(dev), r(CB).to(dev)), torch.empty(N, CB, device=dev)
        pkg.head_prepare(N, CIN, CB)
        pkg.conv1x1_cat_prepare(N, H, H, 4, CB, CB)
        for d in RATES:
            pkg.conv3x3_dilated_prepare(N, H, H, CIN, CB, d)
        variants = {"branch0": lambda: pkg.conv1x1_bn_ex(x, w0, b, s, RELU | A_PADDED, out=o_un)}
        for d in RATES:
            variants[f"dilated_{d}"] = lambda d=d: pkg.conv3x3_dilated_bn_relu(x, taps, b, s, d, out=o_p)
        variants["join"] = lambda: pkg.conv1x1_cat_bn(srcs, w_proj, bias, s, RELU | C_PADDED, out=o_p)
        variants["avgpool_fc"] = lambda: pkg.avgpool_fc(x, head, CB, in_padded=True, out=logits)
        med, times = benchlib.interleaved(variants, a.trials, a.reps)
        rows.append({"N": N, "H": H, "Cin": CIN, "Cb": CB, "median_us": med, "trials_us": times, "sum_us": sum(med.values())})
        print(f"parts N={N:2d}  " + "  ".join(f"{k} {v:.1f}" for k, v in med.items()) + f"  sum {sum(med.values()):.1f} us",
              flush=True)
        del x, o_un, o_p, srcs
        torch.cuda.empty_cache()
    return rows


def net(a, pkg, dev):
    R = benchlib.package_module("resnet")
    sd = torch_nets.deeplab_state_dict(R, "resnet50")
    model = pkg.DeepLabV3.from_state_dict(sd, "resnet50")
    body = torch_nets.TorchResNetBody(R, sd, "resnet50", dev, prefix="backbone.", dilate=torch_nets.SEGMENTATION_DILATE)
    rows = []
    S = a.size
    for N in benchlib.ints(a.ns):
        x, x_cl = torch_nets.image_batch(N, S, S, dev)
        tnet = lambda: torch_nets.deeplab_head(body, body(x_cl), (S, S))
        graph, first = benchlib.captured(lambda: model(x), lambda: model.prepare(N, S, S))
        mine, ref = first["out"], tnet()
        diff = float((mine - ref).abs().max() / ref.abs().max())
        med, times = benchlib.interleaved(benchlib.net_variants(lambda: model(x), graph, tnet), a.trials, a.reps)
        rows.append({"arch": "deeplabv3_resnet50", "N": N, "size": S, "median_us": med, "trials_us": times,
                     "rel_diff_to_torch_fp32": diff, **benchlib.net_ratios(med)})
        print(f"deeplabv3_resnet50 N={N:2d} {S}x{S}  eager {med['eager']:9.1f} us  graph {med['graph']:9.1f} us  torch "
              f"{med['torch']:9.1f} us  graph/torch {rows[-1]['graph_over_torch']:.3f}  eager/torch "
              f"{rows[-1]['eager_over_torch']:.3f}  (max rel diff to torch fp32 {diff:.1e})", flush=True)
        del graph, x, x_cl, first, mine, ref
        torch.cuda.empty_cache()
    return rows


MODES = {"cat": dict(fn=cat, ns="1,8", trials=7, reps=20),
         "module": dict(fn=module, ns="1,8", trials=5, reps=5),
         "net": dict(fn=net, ns="1,8", size=520, trials=5, reps=3),
         "parts": dict(fn=parts, ns="1,8", trials=5, reps=10),
         "all": ["cat", "module", "net"]}


def main():
    a = benchlib.parse(MODES)
    result = benchlib.header(f"tools/aspp_bench.py {a.mode}")
    result.update(benchlib.sections(a, MODES, benchlib.load_package(), torch.device("cuda:0")))
    benchlib.write_json(a.out, result)


if __name__ == "__main__":
    main()
