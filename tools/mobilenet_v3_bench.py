"""Developer tool (GPU box): the depthwise K x K layer at MobileNetV3-Large's points, the new 3x3 entry against the old one,
fc_act at the SE and head shapes, and whole MobileNetV3 forwards.
usage: python tools/mobilenet_v3_bench.py [out.json] [--ns 1,32] [--trials 7] [--reps 20] [--skip-net]
         in one process, the variants interleaved in every trial (median of the trials; a layer variant is one graph of
         `reps` launches, a network variant is timed by events around `reps` // 4 calls):
         (a) dwconv_bn_act (in_act = act = hardswish) at every distinct depthwise point of mobilenet_v3_large at 224 x 224,
             channels padded to 64, under the plan's channel block and under each block forced (WINO_DW_CB), against
             torch's F.conv2d(groups=C) on channels-last tensors + BN affine + hardswish, and against a plain copy of the
             layer's bytes, 4 N C (Hin Win + H W);
         (b) the K = 3 points of mobilenet_v2 (DESIGN.md section 3.2u's table) through dwconv_bn_act(act relu6, no pool)
             against dwconv3x3_bn_act, the unchanged depthwise.hip, in the same run;
         (c) fc_act at the SE and classifier shapes of mobilenet_v3_large against torch.addmm;
         (d) mobilenet_v3_large and _small at 224 x 224 (random weights) eager and replayed from one graph, against torch
             eager on channels-last fp32 tensors.
       The default output is profiles/mobilenet_v3/bench.json."""
import os

import benchlib
import torch
import torch.nn.functional as F

# (Hin, expanded channels, kernel, stride): every distinct depthwise layer of mobilenet_v3_large at 224 x 224
POINTS = [(112, 16, 3, 1), (112, 64, 3, 2), (56, 72, 3, 1), (56, 72, 5, 2), (28, 120, 5, 1), (28, 240, 3, 2), (14, 200, 3, 1),
          (14, 184, 3, 1), (14, 480, 3, 1), (14, 672, 3, 1), (14, 672, 5, 2), (7, 960, 5, 1)]
# (Hin, C of the network, stride): mobilenet_v2's ten depthwise points, the table of DESIGN.md section 3.2u
V2_POINTS = [(112, 32, 1), (112, 96, 2), (56, 144, 1), (56, 144, 2), (28, 192, 1), (28, 192, 2), (14, 384, 1), (14, 576, 1),
             (14, 576, 2), (7, 960, 1)]
# (C, J, act): the SE pairs of mobilenet_v3_large (expanded -> squeeze -> expanded) and its classifier
FC_POINTS = [(72, 24, "relu"), (24, 72, "hardsigmoid"), (120, 32, "relu"), (480, 120, "relu"), (672, 168, "relu"),
             (168, 672, "hardsigmoid"), (960, 240, "relu"), (240, 960, "hardsigmoid"), (960, 1280, "hardswish"),
             (1280, 1000, "none")]


def _pad(c):
    return -(-c // 64) * 64


def _force(L, cb):
    if cb:
        os.environ["WINO_DW_CB"] = str(cb)
    else:
        os.environ.pop("WINO_DW_CB", None)
    L.wino_debug_reload_knobs()


def _layer(N, Hin, C, K, dev, std=3.0):
    g = torch.Generator(device=dev).manual_seed(N + Hin + C + K)
    x = torch.randn(N, Hin + 2, Hin + 2, C, device=dev, generator=g).mul_(std)
    for r in (x[:, 0], x[:, -1], x[:, :, 0], x[:, :, -1]):
        r.zero_()
    w = torch.randn(C, 1, K, K, device=dev, generator=g) / K
    b, s = torch.rand(C, device=dev, generator=g) - 0.5, torch.rand(C, device=dev, generator=g) + 0.5
    return x, w, w[:, 0].permute(1, 2, 0).contiguous(), b, s


def _timed(a, graphs):
    med, times = benchlib.interleaved({k: g.replay for k, g in graphs.items()}, a.trials, 1)
    return {k: v / a.reps for k, v in med.items()}, {k: [t / a.reps for t in v] for k, v in times.items()}


def layers(a, pkg, dev):
    rows, L = [], pkg.lib()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    for N in benchlib.ints(a.ns):
        for Hin, c, K, stride in POINTS:
            C, H = _pad(c), (Hin - 1) // stride + 1
            x, w, taps, b, s = _layer(N, Hin, C, K, dev)
            out = torch.empty(N, H + 2, H + 2, C, device=dev)
            x_cl = x[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
            w_cl = w.contiguous(memory_format=torch.channels_last)
            s4, b4 = s[None, :, None, None], b[None, :, None, None]
            src = torch.empty(N * C * (Hin * Hin + H * H) // 2, device=dev)   # the copy moves the layer's bytes
            dst = torch.empty_like(src)

            def ours():
                pkg.dwconv_bn_act(x, taps, b, s, stride, "hardswish", "hardswish", out=out)

            def torch_dw():
                F.hardswish(F.conv2d(F.hardswish(x_cl), w_cl, stride=stride, padding=K // 2, groups=C) * s4 + b4)

            graphs = {}
            for k, fn, cb in (("plan", ours, 0), ("cb64", ours, 64), ("cb16", ours, 16), ("torch", torch_dw, 0),
                              ("copy", lambda: dst.copy_(src), 0)):
                _force(L, cb)
                graphs[k] = benchlib.captured(benchlib.repeated(fn, a.reps))[0]
            _force(L, 0)
            med, times = _timed(a, graphs)
            cb = pkg.dwconv_plan(N, Hin, Hin, C, K, stride, cus)[0]
            best = 64 if med["cb64"] <= med["cb16"] else 16
            rows.append({"N": N, "Hin": Hin, "C": C, "K": K, "stride": stride, "plan_cb": cb, "faster_cb": best,
                         "median_us": med, "trials_us": times, "over_copy": med["plan"] / med["copy"],
                         "over_torch": med["plan"] / med["torch"]})
            print(f"N={N:3d} {Hin}x{Hin}x{C} k{K} s{stride}: plan(cb{cb}) {med['plan']:8.1f} us  cb64 {med['cb64']:8.1f}  cb16 "
                  f"{med['cb16']:8.1f}  torch {med['torch']:8.1f} ({rows[-1]['over_torch']:.2f})  copy {med['copy']:8.1f} "
                  f"({rows[-1]['over_copy']:.2f})" + ("" if best == cb else "   PLAN IS NOT THE FASTER BLOCK"), flush=True)
            del graphs, x, out, x_cl, src, dst
            torch.cuda.empty_cache()
    return rows


def old_entry(a, pkg, dev):
    rows = []
    for N in benchlib.ints(a.ns):
        for Hin, c, stride in V2_POINTS:
            C, H = _pad(c), (Hin - 1) // stride + 1
            x, _, taps, b, s = _layer(N, Hin, C, 3, dev, 6 / 0.84)
            out = torch.empty(N, H + 2, H + 2, C, device=dev)
            graphs = {"new": benchlib.captured(benchlib.repeated(
                          lambda: pkg.dwconv_bn_act(x, taps, b, s, stride, "relu6", out=out), a.reps))[0],
                      "old": benchlib.captured(benchlib.repeated(
                          lambda: pkg.dwconv3x3_bn_act(x, taps, b, s, stride, "relu6", None, out=out), a.reps))[0]}
            med, times = _timed(a, graphs)
            rows.append({"N": N, "Hin": Hin, "C": C, "stride": stride, "median_us": med, "trials_us": times,
                         "new_over_old": med["new"] / med["old"]})
            print(f"N={N:3d} {Hin}x{Hin}x{C} k3 s{stride}: new {med['new']:8.1f} us  old {med['old']:8.1f} "
                  f"({rows[-1]['new_over_old']:.2f})", flush=True)
            del graphs, x, out
            torch.cuda.empty_cache()
    return rows


def fcs(a, pkg, dev):
    rows = []
    for N in benchlib.ints(a.ns):
        for C, J, act in FC_POINTS:
            g = torch.Generator(device=dev).manual_seed(C + J)
            x, W, b = (torch.randn(*sh, device=dev, generator=g) for sh in ((N, C), (J, C), (J,)))
            out, Wt = torch.empty(N, J, device=dev), W.t().contiguous()
            graphs = {"ours": benchlib.captured(benchlib.repeated(lambda: pkg.fc_act(x, W, b, act, out=out), a.reps))[0],
                      "torch": benchlib.captured(benchlib.repeated(lambda: torch.addmm(b, x, Wt), a.reps))[0]}
            med, times = _timed(a, graphs)
            rows.append({"N": N, "C": C, "J": J, "act": act, "median_us": med, "trials_us": times,
                         "over_torch": med["ours"] / med["torch"]})
            print(f"N={N:3d} fc {C}->{J} {act}: ours {med['ours']:7.1f} us  addmm {med['torch']:7.1f} "
                  f"({rows[-1]['over_torch']:.2f})", flush=True)
    return rows


def state_dict(M, arch, classes=1000, seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in M.expected_keys(arch, classes).items():
        if len(shape) > 1:
            sd[k] = torch.randn(shape, generator=g) * (2.0 / (shape[1] * shape[-1] * shape[-2] if len(shape) == 4 else shape[1])) ** 0.5
        elif k.endswith((".running_var", ".1.weight")):
            sd[k] = torch.rand(shape, generator=g) + 0.5
        else:
            sd[k] = (torch.rand(shape, generator=g) - 0.5) * 0.2
    return sd


def torch_v3(sd, M, arch, dev, eps=1e-3):
    """mobilenet_v3 as a function of the channels-last input: F.conv2d, BN as scale and bias, the activations, SE with
    mean and two 1x1 convolutions, the residual add, mean and two linears."""
    w = {k: v.to(dev).contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v.to(dev) for k, v in sd.items()}
    bn = {}
    for k in sd:
        if k.endswith("running_var"):
            p = k[: -len(".running_var")]
            s = sd[p + ".weight"] / torch.sqrt(sd[k] + eps)
            bn[p] = (s.to(dev)[None, :, None, None], (sd[p + ".bias"] - sd[p + ".running_mean"] * s).to(dev)[None, :, None, None])
    acts = {"RE": F.relu_, "HS": F.hardswish, None: lambda t: t}
    rows = M.BLOCKS[arch]

    def cba(t, p, act, stride=1, pad=0):
        s, b = bn[p + ".1"]
        wt = w[p + ".0.weight"]
        return acts[act](F.conv2d(t, wt, stride=stride, padding=pad, groups=t.shape[1] // wt.shape[1]) * s + b)

    def forward(x_cl):
        t = cba(x_cl, "features.0", "HS", 2, 1)
        for i, (cin, k, hid, cout, se, act, st) in enumerate(rows, 1):
            p, j, y = f"features.{i}.block", 0, t
            if hid != cin:
                y, j = cba(y, f"{p}.0", act), 1
            y = cba(y, f"{p}.{j}", act, st, k // 2)
            j += 1
            if se:
                q = F.relu_(F.conv2d(y.mean(dim=(2, 3), keepdim=True), w[f"{p}.{j}.fc1.weight"], w[f"{p}.{j}.fc1.bias"]))
                y = y * F.hardsigmoid(F.conv2d(q, w[f"{p}.{j}.fc2.weight"], w[f"{p}.{j}.fc2.bias"]))
                j += 1
            y = cba(y, f"{p}.{j}", None)
            t = t + y if st == 1 and cin == cout else y
        t = cba(t, f"features.{len(rows) + 1}", "HS").mean(dim=(2, 3))
        t = F.hardswish(F.linear(t, w["classifier.0.weight"], w["classifier.0.bias"]))
        return F.linear(t, w["classifier.3.weight"], w["classifier.3.bias"])
    return forward


def network(a, pkg, dev):
    M = benchlib.package_module("mobilenet_v3")
    rows = []
    for arch in ("large", "small"):
        sd = state_dict(M, arch)
        model = pkg.MobileNetV3.from_state_dict(sd, arch)
        torch_eager = torch_v3(sd, M, arch, dev)
        for N in benchlib.ints(a.ns):
            x = torch.rand(N, 3, 224, 224, device=dev) * 2 - 1
            x_cl = x.contiguous(memory_format=torch.channels_last)
            graph, _ = benchlib.captured(lambda: model(x), lambda: model.prepare(N, 224, 224))
            med, times = benchlib.interleaved(benchlib.net_variants(lambda: model(x), graph, lambda: torch_eager(x_cl)),
                                              a.trials, max(1, a.reps // 4))
            rows.append({"arch": f"mobilenet_v3_{arch}", "N": N, "median_us": med, "trials_us": times, **benchlib.net_ratios(med)})
            print(f"mobilenet_v3_{arch} N={N:4d}: eager {med['eager']:10.1f} us  graph {med['graph']:10.1f} us  "
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
    res = benchlib.header("tools/mobilenet_v3_bench.py", trials=a.trials, reps=a.reps, layers=layers(a, pkg, dev),
                          old_entry=old_entry(a, pkg, dev), fc_act=fcs(a, pkg, dev))
    if not a.skip_net:
        res["network"] = network(a, pkg, dev)
    benchlib.write_json(a.out or os.path.join(benchlib.ROOT, "profiles", "mobilenet_v3", "bench.json"), res)


if __name__ == "__main__":
    main()
