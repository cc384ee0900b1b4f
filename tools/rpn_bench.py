"""Developer tool (GPU box): box decoding and batched NMS at the detection workload's point.
usage: python tools/rpn_bench.py [profiles/detect/bench.json] [--trials 7] [--reps 10]
  ResNet-50-FPN at N = 2, 800 x 1344: five levels (200x336 .. 13x21, A = 3 anchors, the RPN head's 64-column GEMM output)
  and 4819 proposals per image after the per-level top-k (1000 from each of the four finer levels, 819 from the last):
    decode   wino_box_decode_hw per level and for all five, writing each level's slice of one [N][total] buffer, against
             two byte floors over the HBM rate bench.py's roofline uses: the columns it needs, and the whole rows it touches
    nms      wino_batched_nms_hw at S = 2, R = 4819, IoU 0.7, groups = level, max_out = 1000, and with max_out = R (the
             walk then reaches the last box).  The mask kernel alone is estimated by a call at max_out = 1 (the scan then
             stops after its first block), the scan as the rest
    torch    what torchvision's op does, as a torch composition: the same IoU bit matrix built on the device, copied to
             the host, scanned there.  The scan here is a numpy loop, slower than torchvision's C++ one, so the three parts
             are reported apart; the copy with its synchronisation is what no graph can hold
    detector the first stage (RPN head, decode, filter_proposals) on a held pyramid and the whole FasterRCNN (resnet50,
             1024-wide box head, 91 classes, random weights), eager and as one-graph replay
(median of the trials, events around `reps` calls; the host parts by wall clock)"""
import time

import benchlib
import numpy as np
import torch
import torch_nets

HBM_GBS = 8000.0                        # bench.py's HBM_PEAK_GBS
IMAGE, N, A, LD = (800, 1344), 2, 3, 64
LEVEL_HW = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
PRE_NMS, POST_NMS, IOU = 1000, 1000, 0.7


def decode_rows(a, pkg, dev):
    bc = benchlib.tests_module("box_cases")
    g = torch.Generator().manual_seed(1)
    sizes = (32, 64, 128, 256, 512)
    total = sum(h * w * A for h, w in LEVEL_HW)
    boxes, scores = torch.empty(N, total, 4, device=dev), torch.empty(N, total, device=dev)
    image_hw = torch.tensor([[float(IMAGE[0]), float(IMAGE[1])]] * N, device=dev)
    calls, rows, off = {}, [], 0
    for (h, w), size in zip(LEVEL_HW, sizes):
        head = ((torch.rand(N * h * w, LD, generator=g) - 0.5) * 0.5).to(dev)
        base = bc.base_anchors((size,), (0.5, 1.0, 2.0)).to(dev)
        grid = (h, w, IMAGE[0] // h, IMAGE[1] // w)
        calls[f"{h}x{w}"] = (lambda head=head, base=base, grid=grid, off=off:
                             pkg.box_decode(head, base, image_hw, A, grid=grid, delta_col=A, score_col=0, out_boxes=boxes,
                                            out_scores=scores, out_offset=off))
        off += h * w * A
    calls["all levels"] = lambda: [fn() for k, fn in list(calls.items())[:len(LEVEL_HW)]]
    med, times = benchlib.interleaved(calls, a.trials, a.reps)
    graphs = {k: benchlib.captured(benchlib.repeated(fn, a.reps))[0] for k, fn in calls.items()}
    gmed, _ = benchlib.interleaved({k: gr.replay for k, gr in graphs.items()}, a.trials, 3)
    del graphs
    for k in calls:
        n_rows = N * sum(h * w for h, w in LEVEL_HW) if k == "all levels" else N * int(k.split("x")[0]) * int(k.split("x")[1])
        used = n_rows * (5 * A * 4 + A * 20)
        touched = n_rows * (LD * 4 + A * 20)
        rows.append({"level": k, "boxes": n_rows * A, "eager_us": med[k], "graph_us": gmed[k] / a.reps,
                     "floor_used_columns_us": used / HBM_GBS / 1e3, "floor_whole_rows_us": touched / HBM_GBS / 1e3})
        r = rows[-1]
        print(f"decode {k:10s} {r['boxes']:7d} boxes  graph {r['graph_us']:7.1f} us  eager {r['eager_us']:7.1f} us  floors "
              f"{r['floor_used_columns_us']:.2f} / {r['floor_whole_rows_us']:.2f} us", flush=True)
    return rows


def torch_mask(boxes, groups, nb):
    """The suppression bit matrix of one segment with torch ops on the device: [R][nb] int64 words."""
    R = boxes.shape[0]
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    lt, rb = torch.max(boxes[:, None, :2], boxes[None, :, :2]), torch.min(boxes[:, None, 2:], boxes[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    hit = (inter / (area[:, None] + area[None, :] - inter) > IOU) & (groups[:, None] == groups[None, :])
    hit = torch.triu(hit, diagonal=1)
    hit = torch.nn.functional.pad(hit, (0, nb * 64 - R)).view(R, nb, 64).long()
    return (hit << torch.arange(64, device=boxes.device)).sum(dim=2)


def host_scan(mask, cand, max_out):
    """torchvision's host loop over the bit matrix (numpy words)."""
    removed = np.zeros(mask.shape[1], dtype=np.uint64)
    keep = []
    for i in range(mask.shape[0]):
        if cand[i] and not (int(removed[i >> 6]) >> (i & 63)) & 1:
            keep.append(i)
            if len(keep) >= max_out:
                break
            removed |= mask[i]
    return keep


def nms_rows(a, pkg, dev):
    bc = benchlib.tests_module("box_cases")
    R = 4 * PRE_NMS + LEVEL_HW[-1][0] * LEVEL_HW[-1][1] * A
    case = bc.NmsCase(R, N, seed=5, n_groups=5)
    b, sc, g = (torch.from_numpy(v).to(dev) for v in (case.boxes, case.scores, case.groups))
    p = dict(iou_thresh=IOU, min_size=1e-3, score_thresh=0.0)
    want = bc.batched_nms_reference(case.boxes, case.scores, case.groups, max_out=POST_NMS, **p)
    ws = torch.empty(pkg.nms_workspace_bytes(N, R) // 4, device=dev)
    keep, count = torch.empty(N, POST_NMS, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    rois = torch.empty(N, POST_NMS, 5, device=dev)
    keep1 = torch.empty(N, 1, dtype=torch.int32, device=dev)
    calls = {"nms": lambda: pkg.batched_nms(b, sc, g, max_out=POST_NMS, rois_out=rois, workspace=ws, keep=keep, count=count, **p),
             "mask + one block": lambda: pkg.batched_nms(b, sc, g, max_out=1, workspace=ws, keep=keep1, count=count, **p)}
    keep_all = torch.empty(N, R, dtype=torch.int32, device=dev)
    calls["nms, full walk"] = lambda: pkg.batched_nms(b, sc, g, max_out=R, workspace=ws, keep=keep_all, count=count, **p)
    calls["nms"]()
    torch.cuda.synchronize()
    same = bool(np.array_equal(keep.cpu().numpy(), want[0]) and np.array_equal(count.cpu().numpy(), want[1]))
    nb = (R + 63) // 64
    calls["torch mask (device)"] = lambda: [torch_mask(b[s], g[s], nb) for s in range(N)]
    med, times = benchlib.interleaved(calls, a.trials, a.reps)
    graphs = {k: benchlib.captured(benchlib.repeated(fn, a.reps))[0] for k, fn in list(calls.items())[:3]}
    gmed, _ = benchlib.interleaved({k: gr.replay for k, gr in graphs.items()}, a.trials, 3)
    gmed = {k: v / a.reps for k, v in gmed.items()}
    del graphs
    masks = calls["torch mask (device)"]()
    torch.cuda.synchronize()
    copy_s, scan_s = [], []
    for _ in range(a.trials):
        t0 = time.perf_counter()
        host = [m.cpu().numpy().view(np.uint64) for m in masks]          # (synchronises)
        t1 = time.perf_counter()
        kept = [host_scan(host[s], (case.scores[s] >= 0.0) & ((case.boxes[s, :, 2] - case.boxes[s, :, 0]) >= 1e-3)
                          & ((case.boxes[s, :, 3] - case.boxes[s, :, 1]) >= 1e-3), POST_NMS) for s in range(N)]
        t2 = time.perf_counter()
        copy_s.append(t1 - t0), scan_s.append(t2 - t1)
    same_host = all(kept[s] == [v for v in want[0][s].tolist() if v >= 0] for s in range(N))
    row = {"S": N, "R": R, "max_out": POST_NMS, "kept": want[1].tolist(), "kernel_equals_fp64_walk": same,
           "host_scan_equals_fp64_walk": same_host, "workspace_bytes": pkg.nms_workspace_bytes(N, R),
           "nms_eager_us": med["nms"], "nms_graph_us": gmed["nms"], "mask_plus_one_block_graph_us": gmed["mask + one block"],
           "scan_estimate_us": gmed["nms"] - gmed["mask + one block"], "full_walk_graph_us": gmed["nms, full walk"],
           "full_walk_kept": bc.batched_nms_reference(case.boxes, case.scores, case.groups, **p)[1].tolist(), "torch_mask_device_us": med["torch mask (device)"],
           "torch_mask_copy_to_host_us": float(np.median(copy_s)) * 1e6, "numpy_host_scan_us": float(np.median(scan_s)) * 1e6}
    for k, v in row.items():
        print(f"nms {k}: {v}", flush=True)
    return [row]


def detector_rows(a, pkg, dev):
    """The first stage on a held pyramid, and the whole detector, eager and as one-graph replay (one model each: a graph
    holds its model's tensors)."""
    R, rc = benchlib.package_module("resnet"), benchlib.tests_module("roi_cases")
    C, An = torch_nets.FPN_CHANNELS, A
    sd = {"backbone." + k: v for k, v in torch_nets.fpn_state_dict(R, "resnet50")[0].items()}
    g = torch.Generator().manual_seed(7)
    rn = lambda *s: torch.randn(*s, generator=g)
    sd.update({"rpn.head.conv.0.0.weight": rn(C, C, 3, 3) * (2.0 / (9 * C)) ** 0.5, "rpn.head.conv.0.0.bias": rn(C) * 0.1,
               "rpn.head.cls_logits.weight": rn(An, C, 1, 1) * (4.0 / C) ** 0.5, "rpn.head.cls_logits.bias": rn(An) * 0.1,
               "rpn.head.bbox_pred.weight": rn(4 * An, C, 1, 1) * (0.5 / C) ** 0.5, "rpn.head.bbox_pred.bias": rn(4 * An) * 0.05})
    sd.update({"roi_heads." + k: v for k, v in rc.box_head_state_dict(C, 7, 1024, 91, seed=7).items()})
    x = (torch.rand(N, 3, *IMAGE, generator=g) - 0.5).to(dev)
    models = [pkg.FasterRCNN.from_state_dict(sd, "resnet50") for _ in range(2)]
    for m in models:
        m.prepare(N, *IMAGE)
        m(x)
    torch.cuda.synchronize()
    pyramid = lambda m: {**{str(i): t for i, t in enumerate(m.backbone._p)}, "pool": m.backbone._p[3][:, 1:-1:2, 1:-1:2, :]}
    first = lambda m: m.rpn(pyramid(m), m._full_hw, IMAGE)
    calls = {"first stage": lambda: first(models[0]), "detector": lambda: models[1](x)}
    med, times = benchlib.interleaved(calls, a.trials, a.reps)
    graphs = {}
    for (k, fn), m in zip(calls.items(), models):
        graphs[k] = benchlib.captured(fn, prepare=lambda m=m: (m.prepare(N, *IMAGE), m(x)))[0]
    gmed, gtimes = benchlib.interleaved({k: gr.replay for k, gr in graphs.items()}, a.trials, a.reps)
    out = models[1](x)
    torch.cuda.synchronize()
    rows = [{"what": k, "eager_us": med[k], "graph_us": gmed[k], "trials_eager_us": times[k], "trials_graph_us": gtimes[k]}
            for k in calls]
    rows[0]["proposals"], rows[1]["detections"] = models[0].rpn._count.tolist(), out["count"].tolist()
    for r in rows:
        print(f"{r['what']:12s} eager {r['eager_us']:9.1f} us   graph {r['graph_us']:9.1f} us", flush=True)
    del graphs
    return rows


MODES = {None: dict(trials=7, reps=10)}


def main():
    a = benchlib.parse(MODES)
    pkg = benchlib.load_package()
    dev = torch.device("cuda:0")
    result = benchlib.header("tools/rpn_bench.py", trials=a.trials, reps=a.reps,
                             workload={"N": N, "image": IMAGE, "levels": LEVEL_HW, "anchors": A, "pre_nms_top_n": PRE_NMS,
                                       "post_nms_top_n": POST_NMS, "iou": IOU}, hbm_gbs=HBM_GBS)
    result["decode"] = decode_rows(a, pkg, dev)
    result["nms"] = nms_rows(a, pkg, dev)
    result["detector"] = detector_rows(a, pkg, dev)
    benchlib.write_json(a.out, result)


if __name__ == "__main__":
    main()
