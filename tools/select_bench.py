"""Developer tool (GPU box): the detectors' select step, torch's topk / sort / gather against select_topk.
usage: python tools/select_bench.py [profiles/select/bench.json] [--trials 7] [--reps 10]
  ResNet-50-FPN at N = 2, 800 x 1344, each row on the torch path and on the kernel path, interleaved in one process, eager
  and as one-graph replay:
    rpn select    filter_proposals' selecting and ordering on held logits and boxes: five levels (201600 .. 819 scores per
                  image) to 1000 each, K = 4819, then the stable sort of the K and the boxes in that order
    post select   postprocess_detections' select on held scores and boxes: M = 1000 x 90 = 90000 scores per image, k = 8192
    first stage   RPN head, decode, filter_proposals and NMS on a held pyramid
    detector      the whole FasterRCNN (resnet50, 1024-wide box head, 91 classes, random weights)
  The two select rows also give the byte floor of reading the scores once at the HBM rate bench.py's roofline uses, and
  whether the two paths returned the same indices on this input.
(median of the trials, events around `reps` calls; every trial is kept in the JSON: their spread is the run-to-run noise)"""
import benchlib
import torch
import torch_nets

HBM_GBS = 8000.0                        # bench.py's HBM_PEAK_GBS
IMAGE, N, A = (800, 1344), 2, 3
LEVEL_HW = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
PRE_NMS = 1000
POST_M, POST_K = 1000 * 90, 8192


def both_ways(a, calls, floor_bytes=None, prepare=None, **fields):
    """calls: {"torch": fn, "kernel": fn}.  One row: eager and graph medians, every trial, the kernel path over torch's.
    prepare[k] runs on the capture stream before variant k's capture (the library's scratch is per stream)."""
    med, times = benchlib.interleaved(calls, a.trials, a.reps)
    graphs = {k: benchlib.captured(fn, (prepare or {}).get(k))[0] for k, fn in calls.items()}
    gmed, gtimes = benchlib.interleaved({k: g.replay for k, g in graphs.items()}, a.trials, a.reps)
    del graphs
    row = dict(fields)
    for k in calls:
        row.update({f"{k}_eager_us": med[k], f"{k}_graph_us": gmed[k], f"{k}_trials_eager_us": times[k],
                    f"{k}_trials_graph_us": gtimes[k]})
    row["kernel_over_torch_eager"] = med["kernel"] / med["torch"]
    row["kernel_over_torch_graph"] = gmed["kernel"] / gmed["torch"]
    if floor_bytes is not None:
        row["floor_read_scores_once_us"] = floor_bytes / HBM_GBS / 1e3
    print(f"{row['what']:12s} torch eager {med['torch']:9.1f} graph {gmed['torch']:9.1f} us   kernel eager "
          f"{med['kernel']:9.1f} graph {gmed['kernel']:9.1f} us   kernel / torch (graph) {row['kernel_over_torch_graph']:.2f}"
          + (f"   floor {row['floor_read_scores_once_us']:.2f} us" if floor_bytes is not None else ""), flush=True)
    return row


def select_rows(a, pkg, dev):
    g = torch.Generator().manual_seed(3)
    ns = [h * w * A for h, w in LEVEL_HW]
    ks = [min(PRE_NMS, n) for n in ns]
    offs = [sum(ns[:l]) for l in range(len(ns))]
    total, K = sum(ns), sum(ks)
    logits = torch.randn(N, total, generator=g).to(dev)
    boxes = torch.rand(N, total, 4, generator=g).to(dev)
    i32, f32 = torch.int32, torch.float32
    o = dict(idx=torch.empty(N, K, dtype=i32, device=dev), logit=torch.empty(N, K, device=dev),
             count=torch.empty(N, len(ks), dtype=i32, device=dev), boxes=torch.empty(N, K, 4, device=dev),
             ws=torch.empty(pkg.select_workspace_bytes(N, ns, ks) // 4 + 1, dtype=f32, device=dev),
             order=torch.empty(N, K, dtype=i32, device=dev), slogit=torch.empty(N, K, device=dev),
             count2=torch.empty(N, 1, dtype=i32, device=dev), sboxes=torch.empty(N, K, 4, device=dev))

    def rpn_torch():
        idx = torch.cat([logits[:, off:off + n].topk(k, dim=1, sorted=True).indices + off for n, k, off in zip(ns, ks, offs)],
                        dim=1)
        slogit, order = torch.sort(logits.gather(1, idx), dim=1, descending=True, stable=True)
        sidx = idx.gather(1, order)
        return sidx, slogit, boxes.gather(1, sidx[:, :, None].expand(-1, -1, 4)).contiguous()

    def rpn_kernel():
        idx, logit, _, b = pkg.select_topk(logits, ks, ns, offs, boxes=boxes, out_idx=o["idx"], out_vals=o["logit"],
                                           out_count=o["count"], out_boxes=o["boxes"], workspace=o["ws"])
        order, slogit, _, sb = pkg.select_topk(logit, K, boxes=b, out_idx=o["order"], out_vals=o["slogit"],
                                               out_count=o["count2"], out_boxes=o["sboxes"])
        return idx.long().gather(1, order.long()), slogit, sb

    want, got = rpn_torch(), rpn_kernel()
    torch.cuda.synchronize()
    same = all(torch.equal(x, y) for x, y in zip(want, got))
    rows = [both_ways(a, {"torch": rpn_torch, "kernel": rpn_kernel}, N * total * 4, what="rpn select", scores=[N, total],
                      levels=ns, k=ks, same_result=same)]
    scores = torch.rand(N, POST_M, generator=g).to(dev)
    scores[:, POST_M // 2:] = 0.0                      # the padding proposals' exact zeros
    pboxes = torch.rand(N, POST_M, 4, generator=g).to(dev)
    p = dict(idx=torch.empty(N, POST_K, dtype=i32, device=dev), vals=torch.empty(N, POST_K, device=dev),
             count=torch.empty(N, 1, dtype=i32, device=dev), boxes=torch.empty(N, POST_K, 4, device=dev),
             ws=torch.empty(pkg.select_workspace_bytes(N, POST_M, POST_K) // 4 + 1, dtype=f32, device=dev))

    def post_torch():
        top = scores.topk(POST_K, dim=1, sorted=True)
        return top.indices, top.values.contiguous(), pboxes.gather(1, top.indices[:, :, None].expand(-1, -1, 4)).contiguous()

    def post_kernel():
        idx, vals, _, b = pkg.select_topk(scores, POST_K, boxes=pboxes, out_idx=p["idx"], out_vals=p["vals"],
                                          out_count=p["count"], out_boxes=p["boxes"], workspace=p["ws"])
        return idx.long(), vals, b

    want, got = post_torch(), post_kernel()
    torch.cuda.synchronize()
    live = want[1] != 0
    same = bool(torch.equal(want[1], got[1]) and torch.equal(want[0][live], got[0][live]))
    rows.append(both_ways(a, {"torch": post_torch, "kernel": post_kernel}, N * POST_M * 4, what="post select",
                          scores=[N, POST_M], k=POST_K, same_result_on_nonzero_scores=same))
    return rows


def detector_rows(a, pkg, dev):
    """The first stage on a held pyramid and the whole detector (one model per variant: a graph holds its model's
    tensors)."""
    R, rc = benchlib.package_module("resnet"), benchlib.tests_module("roi_cases")
    C = torch_nets.FPN_CHANNELS
    sd = {"backbone." + k: v for k, v in torch_nets.fpn_state_dict(R, "resnet50")[0].items()}
    g = torch.Generator().manual_seed(7)
    rn = lambda *s: torch.randn(*s, generator=g)
    sd.update({"rpn.head.conv.0.0.weight": rn(C, C, 3, 3) * (2.0 / (9 * C)) ** 0.5, "rpn.head.conv.0.0.bias": rn(C) * 0.1,
               "rpn.head.cls_logits.weight": rn(A, C, 1, 1) * (4.0 / C) ** 0.5, "rpn.head.cls_logits.bias": rn(A) * 0.1,
               "rpn.head.bbox_pred.weight": rn(4 * A, C, 1, 1) * (0.5 / C) ** 0.5, "rpn.head.bbox_pred.bias": rn(4 * A) * 0.05})
    sd.update({"roi_heads." + k: v for k, v in rc.box_head_state_dict(C, 7, 1024, 91, seed=7).items()})
    x = (torch.rand(N, 3, *IMAGE, generator=g) - 0.5).to(dev)
    pyramid = lambda m: {**{str(i): t for i, t in enumerate(m.backbone._p)}, "pool": m.backbone._p[3][:, 1:-1:2, 1:-1:2, :]}
    rows = []
    for what in ("first stage", "detector"):
        models = {k: pkg.FasterRCNN.from_state_dict(sd, "resnet50", select=k) for k in ("torch", "kernel")}
        outs = {}
        for k, m in models.items():
            m.prepare(N, *IMAGE)
            outs[k] = {name: t.clone() for name, t in m(x).items()}
        torch.cuda.synchronize()
        same = all(torch.equal(outs["torch"][name], outs["kernel"][name]) for name in outs["torch"])
        if what == "first stage":
            calls = {k: (lambda m=m: m.rpn(pyramid(m), m._full_hw, IMAGE)) for k, m in models.items()}
        else:
            calls = {k: (lambda m=m: m(x)) for k, m in models.items()}
        prepare = {k: (lambda m=m: (m.prepare(N, *IMAGE), m(x))) for k, m in models.items()}
        rows.append(both_ways(a, calls, prepare=prepare, what=what, same_detections=same, detections=outs["kernel"]["count"].tolist()))
        del models, calls
    return rows


MODES = {None: dict(trials=7, reps=10)}


def main():
    a = benchlib.parse(MODES)
    pkg = benchlib.load_package()
    dev = torch.device("cuda:0")
    result = benchlib.header("tools/select_bench.py", trials=a.trials, reps=a.reps,
                             workload={"N": N, "image": IMAGE, "levels": LEVEL_HW, "anchors": A, "pre_nms_top_n": PRE_NMS,
                                       "post_scores": POST_M, "post_k": POST_K}, hbm_gbs=HBM_GBS)
    result["select"] = select_rows(a, pkg, dev)
    result["detector"] = detector_rows(a, pkg, dev)
    benchlib.write_json(a.out, result)


if __name__ == "__main__":
    main()
