"""Developer tool (GPU box): the R-CNN image transform at the detection workload's point.
usage: python tools/transform_bench.py transform profiles/transform/transform.json [--trials 9] [--reps 20]
       python tools/transform_bench.py detector profiles/transform/detector.json [--trials 5] [--reps 3]
  transform  wino_image_transform_hw on a 480 x 640 and a 427 x 640 image (resized to 800 x 1066 and 799 x 1199) into the
             2 x 3 x 800 x 1216 batch, from float32 and from uint8 images, interleaved with (a) torch's composition -- per
             image normalise, interpolate(scale_factor, recompute_scale_factor=True), copy into a zeroed batch -- and (b)
             `zero_()` of the batch tensor, the store floor the launch's time is reported as a ratio to; the launch
             and the fill are timed a second time as graphs of `reps` calls, which leaves the host's share out
  detector   Faster and Mask R-CNN-ResNet50-FPN (1024-wide box head, 91 classes, random weights): `predict` on the two
             images beside `forward` on the ready batch, each as one-graph replay
(median of the trials, events around `reps` calls)"""
import benchlib
import torch
import torch_nets

SHAPES, CLASSES = [(480, 640), (427, 640)], 91
MIN_SIZE, MAX_SIZE = 800, 1333


def torch_transform(imgs, scales, batch, mean, std):
    """torchvision's GeneralizedRCNNTransform with torch ops, into `batch`."""
    batch.zero_()
    for i, (t, s) in enumerate(zip(imgs, scales)):
        x = t.float() / 255.0 if t.dtype == torch.uint8 else t
        x = (x - mean) / std
        x = torch.nn.functional.interpolate(x[None], scale_factor=s, mode="bilinear", recompute_scale_factor=True,
                                            align_corners=False)[0]
        batch[i, :, :x.shape[1], :x.shape[2]].copy_(x)
    return batch


def workload(pkg, dev):
    tc = benchlib.tests_module("transform_cases")
    sizes = [pkg.transform_size(h, w, MIN_SIZE, MAX_SIZE) for h, w in SHAPES]
    Hb, Wb = pkg.batch_hw(sizes)
    scales = []
    for h, w in SHAPES:
        mn, mx = torch.tensor(float(min(h, w))), torch.tensor(float(max(h, w)))
        scales.append(torch.min(MIN_SIZE / mn, MAX_SIZE / mx).item())
    imgs = {"f32": [t.to(dev) for t in tc.images(SHAPES, 3, torch.float32, seed=1)],
            "u8": [t.to(dev) for t in tc.images(SHAPES, 3, torch.uint8, seed=1)]}
    return sizes, (Hb, Wb), scales, imgs


def transform_rows(a, pkg, dev):
    sizes, (Hb, Wb), scales, imgs = workload(pkg, dev)
    mean = torch.tensor(pkg.IMAGENET_MEAN, device=dev)[:, None, None]
    std = torch.tensor(pkg.IMAGENET_STD, device=dev)[:, None, None]
    batch, ref = torch.empty(len(SHAPES), 3, Hb, Wb, device=dev), torch.empty(len(SHAPES), 3, Hb, Wb, device=dev)
    run = lambda k: pkg.image_transform(imgs[k], sizes, Hb, Wb, out=batch)
    calls = {"fill": batch.zero_, "transform f32": lambda: run("f32"), "transform u8": lambda: run("u8"),
             "torch f32": lambda: torch_transform(imgs["f32"], scales, ref, mean, std),
             "torch u8": lambda: torch_transform(imgs["u8"], scales, ref, mean, std)}
    med, times = benchlib.interleaved(calls, a.trials, a.reps)
    # the same launches without the host's share: `reps` calls captured into one graph, one replay per timed call
    graphs = {k: benchlib.captured(benchlib.repeated(calls[k], a.reps))[0] for k in ("fill", "transform f32", "transform u8")}
    gmed, gtimes = benchlib.interleaved({k: g.replay for k, g in graphs.items()}, a.trials, 1)
    gmed = {k: v / a.reps for k, v in gmed.items()}
    out_bytes = batch.numel() * 4
    rows = []
    for k, px in (("f32", 4), ("u8", 1)):
        in_bytes = sum(3 * h * w * px for h, w in SHAPES)
        run(k), torch_transform(imgs[k], scales, ref, mean, std)
        torch.cuda.synchronize()
        assert [tuple(int(v) for v in pkg.transform_size(h, w)) for h, w in SHAPES] == sizes
        diff = float((batch - ref).abs().max() / ref.abs().max())
        t, tt = med["transform " + k], med["torch " + k]
        rows.append({"images": k, "in_bytes": in_bytes, "out_bytes": out_bytes, "transform_us": t, "torch_us": tt,
                     "fill_us": med["fill"], "transform_over_fill": t / med["fill"], "torch_over_transform": tt / t,
                     "store_gbs": out_bytes / t / 1e3, "fill_gbs": out_bytes / med["fill"] / 1e3,
                     "graph_transform_us": gmed["transform " + k], "graph_fill_us": gmed["fill"],
                     "graph_transform_over_fill": gmed["transform " + k] / gmed["fill"],
                     "graph_store_gbs": out_bytes / gmed["transform " + k] / 1e3,
                     "trials_graph_transform_us": [v / a.reps for v in gtimes["transform " + k]],
                     "trials_graph_fill_us": [v / a.reps for v in gtimes["fill"]],
                     "max_diff_to_torch_over_max": diff, "trials_transform_us": times["transform " + k],
                     "trials_torch_us": times["torch " + k], "trials_fill_us": times["fill"]})
        r = rows[-1]
        print(f"{k:4s} transform {t:7.1f} us ({r['store_gbs']:5.0f} GB/s stored)  fill {med['fill']:7.1f} us  transform / fill "
              f"{r['transform_over_fill']:.2f}  torch {tt:8.1f} us ({r['torch_over_transform']:.1f}x)  against torch {diff:.1e}\n"
              f"     from a graph of {a.reps}: transform {r['graph_transform_us']:7.1f} us ({r['graph_store_gbs']:5.0f} GB/s stored)  fill "
              f"{r['graph_fill_us']:7.1f} us  transform / fill {r['graph_transform_over_fill']:.2f}", flush=True)
    del graphs
    rows.append({"workload": {"shapes": SHAPES, "sizes": sizes, "batch": [len(SHAPES), 3, Hb, Wb],
                              "min_size": MIN_SIZE, "max_size": MAX_SIZE}})
    return rows


def detector_rows(a, pkg, dev):
    """predict on the two images beside forward on the ready batch, each from one graph (one model per graph: a graph
    holds its model's tensors)."""
    R, rc = benchlib.package_module("resnet"), benchlib.tests_module("roi_cases")
    sizes, (Hb, Wb), _, imgs = workload(pkg, dev)
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
    make = {"faster r-cnn": lambda: pkg.FasterRCNN.from_state_dict(sd, "resnet50"),
            "mask r-cnn": lambda: pkg.MaskRCNN.from_state_dict(full, "resnet50")}
    x = pkg.image_transform(imgs["f32"], sizes, Hb, Wb)
    hw = torch.tensor(sizes, dtype=torch.float32, device=dev)
    rows = []
    for k, build in make.items():
        fwd, prd = build(), build()
        gf = benchlib.captured(lambda: fwd(x, hw), prepare=lambda: fwd.prepare(len(SHAPES), Hb, Wb))[0]
        gp, out = benchlib.captured(lambda: prd.predict(imgs["f32"]), prepare=lambda: prd.prepare_images(SHAPES))
        med, times = benchlib.interleaved({"forward": gf.replay, "predict": gp.replay}, a.trials, a.reps)
        rows.append({"what": k, "forward_graph_us": med["forward"], "predict_graph_us": med["predict"],
                     "predict_minus_forward_us": med["predict"] - med["forward"], "detections": out["count"].tolist(),
                     "trials_forward_us": times["forward"], "trials_predict_us": times["predict"]})
        print(f"{k:12s} forward {med['forward']:9.1f} us   predict {med['predict']:9.1f} us   detections "
              f"{rows[-1]['detections']}", flush=True)
        del gf, gp, fwd, prd
    return rows


MODES = {"transform": dict(fn=transform_rows, trials=9, reps=20), "detector": dict(fn=detector_rows, trials=5, reps=3)}

if __name__ == "__main__":
    benchlib.main_rows("tools/transform_bench.py", MODES)
