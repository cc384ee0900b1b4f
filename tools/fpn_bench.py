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
import benchlib
import torch
import torch.nn.functional as F
import torch_nets

CF = torch_nets.FPN_CHANNELS


def lateral(a, pkg, dev):
    R = benchlib.package_module("resnet")
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
        med, times = benchlib.interleaved({"fused": fused, "plain": plain, "composed": composed, "same_size": same_size},
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


def net(a, pkg, dev):
    R = benchlib.package_module("resnet")
    N, (H, W) = a.n, a.hw
    rows = []
    for arch in a.archs.split(","):
        sd, _ = torch_nets.fpn_state_dict(R, arch)
        model = pkg.ResNetFPN.from_state_dict(sd, arch, out_channels=CF)
        body = torch_nets.TorchResNetBody(R, sd, arch, dev, prefix="body.")
        x, x_cl = torch_nets.image_batch(N, H, W, dev)
        tnet = lambda: torch_nets.fpn_head(body, body(x_cl))
        graph, got = benchlib.captured(lambda: model(x), lambda: model.prepare(N, H, W))
        want = tnet()
        errs = {k: float((got[k].permute(0, 3, 1, 2) - w).abs().max() / w.abs().max())
                for k, w in zip(("0", "1", "2", "3", "pool"), want)}
        med, times = benchlib.interleaved(benchlib.net_variants(lambda: model(x), graph, tnet), a.trials, a.reps)
        row = {"arch": arch, "N": N, "H": H, "W": W, "median_us": med, "trials_us": times,
               "max_rel_diff_vs_torch_fp32": errs, **benchlib.net_ratios(med)}
        rows.append(row)
        print(f"{arch:9s}-fpn N={N} {H}x{W}  eager {med['eager']:9.1f} us  graph {med['graph']:9.1f} us  torch "
              f"{med['torch']:9.1f} us  graph/torch {row['graph_over_torch']:.3f}  max rel diff vs torch "
              f"{max(errs.values()):.1e}", flush=True)
        del graph, model, body, x, x_cl, got, want
        torch.cuda.empty_cache()
    return rows


MODES = {"lateral": dict(fn=lateral, n=2, hw="800,1344", trials=7, reps=20),
         "net": dict(fn=net, archs="resnet50,resnet18", n=2, hw="800,1344", trials=5, reps=5)}


def main():
    a = benchlib.parse(MODES)
    a.hw = tuple(benchlib.ints(a.hw))
    rows = a.fn(a, benchlib.load_package(), torch.device("cuda:0"))
    # one file for both modes: the other mode's rows stay
    benchlib.write_json(a.out, benchlib.header("tools/fpn_bench.py", **{a.mode: benchlib.section(a, rows)}), merge=True)


if __name__ == "__main__":
    main()
