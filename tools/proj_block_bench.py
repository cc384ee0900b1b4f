"""Developer tool (GPU box): the projection bottleneck block, fused (wino_proj_block_hw: strided 1x1, 3x3, fused tail)
against the best composition the library allowed before it (a torch strided copy of x, the projection 1x1 written
to memory, then the identity block's three launches with the shortcut added as WINO_ADD_RESIDUAL), interleaved.
usage: python tools/proj_block_bench.py [out.json] [--ns 1,16,128] [--trials 5] [--reps 50]
Per (stage, N): 0.4 s of preheat, then `trials` rounds; in every round each variant runs `reps` blocks between two
events.  Reported: the median round per variant (us per block), the ratio, and the chip clock the last 3x3 launch
of each variant ran at (wino_diag_last_clock).
--v15: the v1.5 block (wino_proj_block_v15_hw: 1x1, stride-2 3x3, fused tail) at conv3/4/5 against the same block with
the stride-2 3x3 done by torch -- F.conv2d(stride=2, padding=1) on channels-last tensors, BN and ReLU in torch -- and
the tail as the library's shortcut 1x1 + last 1x1 with WINO_ADD_RESIDUAL (the fused tail has no entry point of its
own); in the same rounds the stride-2 3x3 alone, library against torch."""
import statistics

import benchlib
import torch

STAGES = {   # ResNet-50's stage-entry blocks: (Hin, Cin, Cm, C4, stride)
    "conv2": (56, 64, 64, 256, 1),
    "conv3": (56, 256, 128, 512, 2),
    "conv4": (28, 512, 256, 1024, 2),
    "conv5": (14, 1024, 512, 2048, 2),
}
PREHEAT_S = 0.4


def main_v1(a, pkg, dev):
    rows = []
    for stage, (Hin, Cin, Cm, C4, s) in STAGES.items():
        for N in benchlib.ints(a.ns):
            g = torch.Generator(device="cpu").manual_seed(N)
            r = lambda *shape, sc=1.0: ((torch.rand(*shape, generator=g) - 0.5) * sc).to(dev)
            x = r(N, Hin, Hin, Cin)
            w1, wp = r(Cin, Cm, sc=4 / Cin ** 0.5), r(Cin, C4, sc=2 / Cin ** 0.5)
            w2, w3 = r(Cm, Cm, 3, 3, sc=4 / (9 * Cm) ** 0.5), r(Cm, C4, sc=4 / Cm ** 0.5)
            bn = [(r(c), r(c) + 1.0) for c in (Cm, Cm, C4, C4)]
            U2 = pkg.filter_transform_f2(w2)
            tail = pkg.proj_tail_pack(w3, bn[2], wp, bn[3])
            H = (Hin - 1) // s + 1
            out = torch.empty(N, H, H, C4, device=dev)
            ws = torch.empty(pkg.lib().wino_proj_block_workspace_bytes_hw(N, H, H, Cm) // 4, device=dev)
            short = torch.empty(N * H * H, C4, device=dev)
            t1p = torch.empty(N, H + 2, H + 2, Cm, device=dev)
            t2p = torch.empty_like(t1p)
            out2 = torch.empty(N * H * H, C4, device=dev)

            def fused():
                pkg.proj_block(x, w1, bn[0], U2, bn[1], tail, s, out=out, workspace=ws)

            def composed():
                xs = x[:, ::s, ::s, :].contiguous() if s > 1 else x
                pkg.conv1x1_bn_ex(xs, wp, bn[3][0], bn[3][1], 0, out=short)
                pkg.conv1x1_bn_ex(xs, w1, bn[0][0], bn[0][1], pkg.RELU | pkg.C_PADDED, out=t1p)
                pkg.conv3x3_bn_relu(t1p, U2, bn[1][0], bn[1][1], out=t2p)
                pkg.conv1x1_bn_ex(t2p, w3, bn[2][0], bn[2][1], pkg.RELU | pkg.A_PADDED | pkg.ADD_RESIDUAL,
                                  residual=short, out=out2)

            fns = {"fused": fused, "composed": composed}
            fused(); composed(); torch.cuda.synchronize()
            rel = float((out.reshape(-1, C4) - out2).abs().max() / out2.abs().max().clamp_min(1e-30))
            clocks = {k: [] for k in fns}   # the chip clock of each round's last 3x3 launch, read after its window
            stamp = lambda k: clocks[k].append((pkg.last_clock_ghz(0) or [None])[0])
            med, times = benchlib.interleaved(fns, a.trials, a.reps, preheat_s=PREHEAT_S,
                                              after={k: (lambda k=k: stamp(k)) for k in fns})
            row = {"stage": stage, "N": N, "Hin": Hin, "Cin": Cin, "Cm": Cm, "C4": C4, "stride": s,
                   "forms_first_tail": pkg.proj_tail_plan(N, Hin, Hin, Cin, Cm, C4, s),
                   "fused_us": med["fused"], "composed_us": med["composed"],
                   "fused_trials_us": times["fused"], "composed_trials_us": times["composed"],
                   "clock_ghz_fused": statistics.median([c for c in clocks["fused"] if c] or [0.0]),
                   "clock_ghz_composed": statistics.median([c for c in clocks["composed"] if c] or [0.0]),
                   "rel_diff_fused_vs_composed": rel}
            row["speedup"] = row["composed_us"] / row["fused_us"]
            rows.append(row)
            print(f"{stage} N={N:4d}  fused {row['fused_us']:9.1f} us  composed {row['composed_us']:9.1f} us  "
                  f"x{row['speedup']:.3f}  clk {row['clock_ghz_fused']:.2f}/{row['clock_ghz_composed']:.2f} GHz  "
                  f"forms {row['forms_first_tail']}  rel {rel:.1e}", flush=True)
            del x, out, ws, short, t1p, t2p, out2
            torch.cuda.empty_cache()
    return rows


def main_v15(a, pkg, dev):
    F = torch.nn.functional
    rows = []
    for stage in ("conv3", "conv4", "conv5"):
        Hin, Cin, Cm, C4, _ = STAGES[stage]
        H = (Hin - 1) // 2 + 1
        for N in benchlib.ints(a.ns):
            g = torch.Generator(device="cpu").manual_seed(N)
            r = lambda *shape, sc=1.0: ((torch.rand(*shape, generator=g) - 0.5) * sc).to(dev)
            x = r(N, Hin, Hin, Cin)
            w1, wp = r(Cin, Cm, sc=4 / Cin ** 0.5), r(Cin, C4, sc=2 / Cin ** 0.5)
            w2, w3 = r(Cm, Cm, 3, 3, sc=4 / (9 * Cm) ** 0.5), r(Cm, C4, sc=4 / Cm ** 0.5)
            bn = [(r(c), r(c) + 1.0) for c in (Cm, Cm, C4, C4)]
            taps = pkg.filter_pack_s2(w2)
            w2_cl = w2.contiguous(memory_format=torch.channels_last)
            tail = pkg.proj_tail_pack(w3, bn[2], wp, bn[3])
            out = torch.empty(N, H, H, C4, device=dev)
            ws = torch.empty(pkg.lib().wino_proj_block_v15_workspace_bytes_hw(N, Hin, Hin, Cm) // 4, device=dev)
            t1p = torch.zeros(N, Hin + 2, Hin + 2, Cm, device=dev)
            t2p = torch.zeros(N, H + 2, H + 2, Cm, device=dev)
            t2l = torch.empty_like(t2p)
            short = torch.empty(N * H * H, C4, device=dev)
            out2 = torch.empty(N * H * H, C4, device=dev)
            sc2, bi2 = bn[1][1][None, :, None, None], bn[1][0][None, :, None, None]

            def torch_s2():   # channels-last NCHW views of the padded NHWC tensors
                y = F.conv2d(t1p[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2), w2_cl, stride=2, padding=1)
                t2p[:, 1:-1, 1:-1, :] = torch.relu(y * sc2 + bi2).permute(0, 2, 3, 1)

            def fused():
                pkg.proj_block_v15(x, w1, bn[0], taps, bn[1], tail, out=out, workspace=ws)

            def composed():
                pkg.conv1x1_bn_ex(x, w1, bn[0][0], bn[0][1], pkg.RELU | pkg.C_PADDED, out=t1p)
                torch_s2()
                pkg.conv1x1_bn_ex(x[:, ::2, ::2, :].contiguous(), wp, bn[3][0], bn[3][1], 0, out=short)
                pkg.conv1x1_bn_ex(t2p, w3, bn[2][0], bn[2][1], pkg.RELU | pkg.A_PADDED | pkg.ADD_RESIDUAL,
                                  residual=short, out=out2)

            def layer():
                pkg.conv3x3_s2_bn_relu(t1p, taps, bn[1][0], bn[1][1], out=t2l)

            fns = {"fused": fused, "composed": composed, "layer": layer, "torch_layer": torch_s2}
            fused(); composed(); layer(); torch.cuda.synchronize()
            rel = float((out.reshape(-1, C4) - out2).abs().max() / out2.abs().max().clamp_min(1e-30))
            rel_layer = float((t2l - t2p).abs().max() / t2p.abs().max().clamp_min(1e-30))
            med, trials = benchlib.interleaved(fns, a.trials, a.reps, preheat_s=PREHEAT_S)
            row = {"stage": stage, "N": N, "Hin": Hin, "Cin": Cin, "Cm": Cm, "C4": C4,
                   "form_3x3": pkg.conv3x3_s2_plan(N, Hin, Hin, Cm, Cm),
                   "fused_us": med["fused"], "composed_torch_3x3_us": med["composed"],
                   "s2_layer_us": med["layer"], "torch_s2_layer_us": med["torch_layer"],
                   "trials_us": trials, "rel_diff_fused_vs_composed": rel, "rel_diff_layer_vs_torch": rel_layer}
            row["speedup_block"] = row["composed_torch_3x3_us"] / row["fused_us"]
            row["speedup_layer"] = row["torch_s2_layer_us"] / row["s2_layer_us"]
            rows.append(row)
            print(f"{stage} N={N:4d}  v1.5 block {med['fused']:9.1f} us  with torch 3x3 {med['composed']:9.1f} us  "
                  f"x{row['speedup_block']:.3f}   3x3 s2 {med['layer']:8.1f} us  torch {med['torch_layer']:8.1f} us  "
                  f"x{row['speedup_layer']:.3f}  form {row['form_3x3']}  rel {rel:.1e} / {rel_layer:.1e}", flush=True)
            del x, out, ws, t1p, t2p, t2l, short, out2
            torch.cuda.empty_cache()
    return rows


MODES = {None: dict(ns="1,16,128", trials=5, reps=50)}
EXTRA = [("--v15", dict(action="store_true"))]


def main():
    a = benchlib.parse(MODES, EXTRA)
    rows = (main_v15 if a.v15 else main_v1)(a, benchlib.load_package(), torch.device("cuda:0"))
    tool = "tools/proj_block_bench.py" + (" --v15" if a.v15 else "")
    benchlib.write_json(a.out, benchlib.header(tool, **benchlib.section(a, rows)))


if __name__ == "__main__":
    main()
