"""Developer tool (GPU box): Mask R-CNN's mask selection and paste at the detection workload's point.
usage: python tools/mask_bench.py paste profiles/mask/paste.json [--trials 9] [--reps 5]
       python tools/mask_bench.py detector profiles/mask/detector.json [--trials 5] [--reps 3]
  paste     wino_mask_paste_hw at N = 2, D = 100, 800 x 1344, M = 28, 91 classes, on the mask head's own GEMM output
            ([R 784][128], the gemm_rows layout): the fp32 planes (860 MB), the uint8 planes (215 MB) and both, each
            interleaved with `zero_()` of the same tensor, the fill every paste time is reported as a ratio to.  The boxes
            have sides log-uniform in 16 .. 400 pixels inside the image; `window_fraction` is the share of the planes'
            pixels that lie inside a window (the rest is written as zeros without reading a logit)
  detector  Mask R-CNN-ResNet50-FPN (1024-wide box head, 91 classes, random weights) beside Faster R-CNN on the same
            weights, eager and as one-graph replay
(median of the trials, events around `reps` calls)"""
import benchlib
import numpy as np
import torch
import torch_nets

IMAGE, N, D, M, CLASSES, LD = (800, 1344), 2, 100, 28, 91, 128


def paste_rows(a, pkg, dev):
    mc = benchlib.tests_module("mask_cases")
    H, W = IMAGE
    rng = np.random.RandomState(3)
    R = N * D
    side = np.exp(rng.uniform(np.log(16.0), np.log(400.0), size=(R, 2)))
    c = rng.uniform(0, 1, size=(R, 2)) * ([W, H] - side) + side / 2
    boxes = np.concatenate([c - side / 2, c + side / 2], axis=1).astype(np.float32)
    labels = rng.randint(1, CLASSES, size=R).astype(np.int32)
    hw = np.array([[float(H), float(W)]] * N, dtype=np.float32)
    inside = 0
    bi, _ = mc.box_integers(boxes, M, np.float32)
    for r in range(R):
        x0, x1e, y0, y1e, _, _ = mc.window(bi[r], H, W)
        inside += max(x1e - x0, 0) * max(y1e - y0, 0)
    t = lambda v: torch.from_numpy(v).to(dev)
    logits = (torch.randn(R * M * M, LD, generator=torch.Generator().manual_seed(4)) * 2).to(dev)
    lb, bx, ihw = t(labels), t(boxes), t(hw)
    out = torch.empty(N, D, H, W, device=dev)
    binary = torch.empty(N, D, H, W, dtype=torch.uint8, device=dev)
    run = lambda **kw: pkg.paste_masks(logits, lb, bx, ihw, H, W, M=M, classes=CLASSES, layout="gemm_rows", want_out=False, **kw)
    calls = {"fill fp32": out.zero_, "paste fp32": lambda: run(out=out), "fill uint8": binary.zero_,
             "paste uint8": lambda: run(binary=binary), "fill both": lambda: (out.zero_(), binary.zero_()),
             "paste both": lambda: run(out=out, binary=binary)}
    med, times = benchlib.interleaved(calls, a.trials, a.reps)
    rows = []
    for kind, nbytes in (("fp32", out.numel() * 4), ("uint8", binary.numel()), ("both", out.numel() * 5)):
        fill, paste = med["fill " + kind], med["paste " + kind]
        rows.append({"output": kind, "bytes": nbytes, "fill_us": fill, "paste_us": paste, "paste_over_fill": paste / fill,
                     "paste_gbs": nbytes / paste / 1e3, "fill_gbs": nbytes / fill / 1e3,
                     "trials_fill_us": times["fill " + kind], "trials_paste_us": times["paste " + kind]})
        r = rows[-1]
        print(f"{kind:6s} {nbytes / 1e6:7.1f} MB  paste {paste:8.1f} us ({r['paste_gbs']:6.0f} GB/s)  fill {fill:8.1f} us "
              f"({r['fill_gbs']:6.0f} GB/s)  paste / fill {r['paste_over_fill']:.2f}", flush=True)
    rows.append({"workload": {"N": N, "D": D, "image": IMAGE, "M": M, "classes": CLASSES, "ld": LD},
                 "window_fraction": inside / float(R * H * W), "logits_bytes_selected": R * (M * M) * 4,
                 "logits_bytes_tensor": logits.numel() * 4})
    return rows


def detector_rows(a, pkg, dev):
    """Mask R-CNN and Faster R-CNN on the same weights, eager and as one-graph replay (one model per variant: a graph
    holds its model's tensors)."""
    R, rc = benchlib.package_module("resnet"), benchlib.tests_module("roi_cases")
    C, An = torch_nets.FPN_CHANNELS, 3
    sd = {"backbone." + k: v for k, v in torch_nets.fpn_state_dict(R, "resnet50")[0].items()}
    g = torch.Generator().manual_seed(7)
    rn = lambda *s: torch.randn(*s, generator=g)
    sd.update({"rpn.head.conv.0.0.weight": rn(C, C, 3, 3) * (2.0 / (9 * C)) ** 0.5, "rpn.head.conv.0.0.bias": rn(C) * 0.1,
               "rpn.head.cls_logits.weight": rn(An, C, 1, 1) * (4.0 / C) ** 0.5, "rpn.head.cls_logits.bias": rn(An) * 0.1,
               "rpn.head.bbox_pred.weight": rn(4 * An, C, 1, 1) * (0.5 / C) ** 0.5, "rpn.head.bbox_pred.bias": rn(4 * An) * 0.05})
    sd.update({"roi_heads." + k: v for k, v in rc.box_head_state_dict(C, 7, 1024, CLASSES, seed=7).items()})
    full = dict(sd)
    full.update({"roi_heads." + k: v for k, v in rc.mask_head_state_dict(C, CLASSES, seed=7).items()})
    x = (torch.rand(N, 3, *IMAGE, generator=g) - 0.5).to(dev)
    make = {"faster r-cnn": lambda: pkg.FasterRCNN.from_state_dict(sd, "resnet50"),
            "mask r-cnn": lambda: pkg.MaskRCNN.from_state_dict(full, "resnet50")}
    rows = []
    for k, build in make.items():
        eager, held = build(), build()
        eager.prepare(N, *IMAGE)
        eager(x)
        torch.cuda.synchronize()
        med, times = benchlib.interleaved({"eager": lambda: eager(x)}, a.trials, a.reps)
        graph = benchlib.captured(lambda: held(x), prepare=lambda: (held.prepare(N, *IMAGE), held(x)))[0]
        gmed, gtimes = benchlib.interleaved({"graph": graph.replay}, a.trials, a.reps)
        out = eager(x)
        torch.cuda.synchronize()
        rows.append({"what": k, "eager_us": med["eager"], "graph_us": gmed["graph"], "detections": out["count"].tolist(),
                     "trials_eager_us": times["eager"], "trials_graph_us": gtimes["graph"]})
        print(f"{k:12s} eager {med['eager']:9.1f} us   graph {gmed['graph']:9.1f} us   detections {rows[-1]['detections']}",
              flush=True)
        del graph, eager, held
    rows.append({"mask_branch_graph_us": rows[1]["graph_us"] - rows[0]["graph_us"]})
    return rows


MODES = {"paste": dict(fn=paste_rows, trials=9, reps=5), "detector": dict(fn=detector_rows, trials=5, reps=3)}

if __name__ == "__main__":
    benchlib.main_rows("tools/mask_bench.py", MODES)
