"""Developer tool (GPU box): what RetinaNet's two kernels and the composed detector cost, at torchvision's point (N = 2,
800 x 1344, 91 classes, A = 9: P3 = 100 x 168, P5 = 25 x 42, cols = 819 of ld = 832).
usage: python tools/retinanet_bench.py select profiles/retinanet/select.json [--N 2] [--trials 7] [--reps 20]
       python tools/retinanet_bench.py decode profiles/retinanet/decode.json [--N 2] [--trials 7] [--reps 50]
       python tools/retinanet_bench.py detector profiles/retinanet/detector.json [--N 2] [--H 800] [--W 1344] [--trials 5]
       [--reps 5]

  select    per level (i) select_topk_map on the padded class map in place; (ii) a contiguous copy of the real columns
            followed by select_topk; (iii) torch: sigmoid, > thresh, topk on the flat copy's values (the copy not timed)
  decode    retina_decode of the 1000 selected anchors against box_decode of the whole level plus a gather
  detector  RetinaNet-ResNet50-FPN with random weights, eager and from one graph; the head alone, eager
(median of the trials, events around `reps` calls)"""
import benchlib as bl
import torch

LEVELS = {"P3": (100, 168, 8), "P5": (25, 42, 32)}
A, K, TOPK, THRESH = 9, 91, 1000, -2.9444


def _select(a, pkg, dev):
    rows, N, cols, ld = [], a.N, A * K, 832
    for name, (h, w, _) in LEVELS.items():
        m = torch.zeros((N, h + 2, w + 2, ld), device=dev)
        m[:, 1:-1, 1:-1, :cols] = torch.randn((N, h, w, cols), device=dev) * 1.5 - 4.0
        n = h * w * cols
        idx, vals = torch.empty((N, TOPK), dtype=torch.int32, device=dev), torch.empty((N, TOPK), device=dev)
        count, count2 = torch.empty((N,), dtype=torch.int32, device=dev), torch.empty((N, 1), dtype=torch.int32, device=dev)
        ws = torch.empty(pkg.select_map_workspace_bytes(N, h, w, cols, TOPK) // 4 + 4, device=dev)
        flat = torch.empty((N, n), device=dev)

        def in_place():
            pkg.select_topk_map(m, cols, TOPK, THRESH, idx, vals, count, 0, ws)

        def copy_then_select():
            flat.view(N, h, w, cols).copy_(m[:, 1:-1, 1:-1, :cols])
            pkg.select_topk(flat, TOPK, score_thresh=THRESH, out_idx=idx, out_vals=vals, out_count=count2, workspace=ws)

        def torch_ops():
            s = torch.sigmoid(flat)
            torch.where(s > 0.05, s, torch.zeros_like(s)).topk(TOPK, dim=1)

        copy_then_select()
        med, _ = bl.interleaved({"map": in_place, "copy_select": copy_then_select, "torch": torch_ops}, a.trials, a.reps)
        rows.append(dict(level=name, N=N, h=h, w=w, cols=cols, ld=ld, n=n, k=TOPK, map_bytes=m.numel() * 4, **med))
        print(rows[-1])
    return rows


def _decode(a, pkg, dev):
    rows, N = [], a.N
    D = bl.package_module("detection")
    for (name, (h, w, stride)), sizes in zip(LEVELS.items(), (D.RETINA_SIZES[0], D.RETINA_SIZES[2])):
        reg = torch.randn((N, h + 2, w + 2, 64), device=dev) * 0.3
        base = D.base_anchors(sizes, D.ANCHOR_RATIOS).to(dev)
        hw = torch.tensor([[800.0, 1344.0]] * N, device=dev)
        idx = torch.randint(0, h * w * A * K, (N, TOPK), dtype=torch.int32, device=dev)
        boxes, labels = torch.empty((N, TOPK, 4), device=dev), torch.empty((N, TOPK), dtype=torch.int32, device=dev)
        head = reg[:, 1:-1, 1:-1, :].reshape(N * h * w, 64).contiguous()
        level = torch.empty((N, h * w * A, 4), device=dev)
        grid = (h, w, stride, stride)

        def selected():
            pkg.retina_decode(idx, reg, base, hw, grid, K, TOPK, boxes, labels)

        def whole_level():
            pkg.box_decode(head, base, hw, A, grid=grid, out_boxes=level)
            level.gather(1, (idx // K).long()[:, :, None].expand(-1, -1, 4))

        med, _ = bl.interleaved({"retina_decode": selected, "box_decode_gather": whole_level}, a.trials, a.reps)
        rows.append(dict(level=name, N=N, anchors=h * w * A, k=TOPK, **med))
        print(rows[-1])
    return rows


def _detector(a, pkg, dev):
    R = bl.package_module("resnet")
    fr, rr = bl.tests_module("fpn_p6p7_reference"), bl.tests_module("retinanet_reference")
    fpn_sd, _ = fr.p6p7_random_state_dict(torch, R, "resnet50", 256, seed=1)
    sd = {"backbone." + k: v for k, v in fpn_sd.items()}
    sd.update({"head." + k: v for k, v in rr.head_state_dict(256, A, K, seed=2).items()})
    m = pkg.RetinaNet.from_state_dict(sd, "resnet50", device=dev)
    x = torch.rand((a.N, 3, a.H, a.W), device=dev) - 0.5
    m.prepare(a.N, a.H, a.W)
    m(x)
    feats = m.backbone(x, padded=True)
    maps = [feats[k] for k in ("0", "1", "2", "p6", "p7")]
    graph, _ = bl.captured(lambda: m(x), lambda: m.prepare(a.N, a.H, a.W))
    med, _ = bl.interleaved({"eager": lambda: m(x), "graph": graph.replay, "backbone": lambda: m.backbone(x, padded=True),
                             "head": lambda: m.head(maps)}, a.trials, a.reps)
    torch.cuda.synchronize()
    row = dict(N=a.N, H=a.H, W=a.W, classes=K, count=m(x)["count"].tolist(), **med)
    print(row)
    return [row]


MODES = {"select": dict(fn=_select, N=2, trials=7, reps=20), "decode": dict(fn=_decode, N=2, trials=7, reps=50),
         "detector": dict(fn=_detector, N=2, H=800, W=1344, trials=5, reps=5)}

if __name__ == "__main__":
    bl.main_rows("retinanet_bench", MODES)
