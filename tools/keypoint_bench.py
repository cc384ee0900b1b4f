"""Developer tool (GPU box): Keypoint R-CNN's output stage, its head and the whole detector at the detection workload's point.
usage: python tools/keypoint_bench.py kernel profiles/keypoint/kernel.json [--trials 5] [--reps 2]
       python tools/keypoint_bench.py head profiles/keypoint/head.json [--trials 7] [--reps 3]
       python tools/keypoint_bench.py detector profiles/keypoint/detector.json [--trials 5] [--reps 3]
  kernel    wino_keypoints_hw at N = 2, D = 100, K = 17, M = 56 in both layouts (planes [R][17][56][56]; deconv_rows, the
            head's own GEMM output [R 196][320]) on two box sets: `detections`, sides log-uniform in 16 .. 400 pixels
            inside an 800 x 1344 image, and `whole_image`, the worst case, every box the whole image (about 1 M outputs per
            plane in one workgroup).  Beside it torchvision's heatmaps_to_keypoints, transcribed with its host reads, on
            the same device tensors
  head      KeypointHead at R = 200, P = 14 (256 -> 8 x 512 -> 17 keypoints), launch by launch, and the whole forward
  detector  Keypoint R-CNN-ResNet50-FPN (1024-wide box head, 2 classes, 17 keypoints, random weights, the class
            scores held at 0.5 so that detections survive) beside Faster R-CNN on the same weights, eager and as
            one-graph replay
(median of the trials, events around `reps` calls)"""
import benchlib
import numpy as np
import torch
import torch_nets

IMAGE, N, D, K, P = (800, 1344), 2, 100, 17, 14
M = 4 * P


def torchvision_loop(maps, rois):
    """torchvision's heatmaps_to_keypoints on device tensors, with its per-detection host reads."""
    F = torch.nn.functional
    offset_x, offset_y = rois[:, 0], rois[:, 1]
    widths = (rois[:, 2] - rois[:, 0]).clamp(min=1)
    heights = (rois[:, 3] - rois[:, 1]).clamp(min=1)
    widths_ceil, heights_ceil = widths.ceil(), heights.ceil()
    num_keypoints = maps.shape[1]
    xy_preds = torch.zeros((len(rois), 3, num_keypoints), dtype=torch.float32, device=maps.device)
    end_scores = torch.zeros((len(rois), num_keypoints), dtype=torch.float32, device=maps.device)
    for i in range(len(rois)):
        roi_map_width = int(widths_ceil[i].item())
        roi_map_height = int(heights_ceil[i].item())
        width_correction = widths[i] / roi_map_width
        height_correction = heights[i] / roi_map_height
        roi_map = F.interpolate(maps[i][:, None], size=(roi_map_height, roi_map_width), mode="bicubic",
                                align_corners=False)[:, 0]
        w = roi_map.shape[2]
        pos = roi_map.reshape(num_keypoints, -1).argmax(dim=1)
        x_int = pos % w
        y_int = torch.div(pos - x_int, w, rounding_mode="floor")
        x = (x_int.float() + 0.5) * width_correction
        y = (y_int.float() + 0.5) * height_correction
        xy_preds[i, 0, :] = x + offset_x[i]
        xy_preds[i, 1, :] = y + offset_y[i]
        xy_preds[i, 2, :] = 1
        end_scores[i, :] = roi_map[torch.arange(num_keypoints, device=maps.device), y_int, x_int]
    return xy_preds.permute(0, 2, 1), end_scores


def kernel_rows(a, pkg, dev):
    H, W = IMAGE
    R, ld = N * D, (16 * K + 63) // 64 * 64
    rng = np.random.RandomState(3)
    side = np.exp(rng.uniform(np.log(16.0), np.log(400.0), size=(R, 2)))
    c = rng.uniform(0, 1, size=(R, 2)) * ([W, H] - side) + side / 2
    idx = np.repeat(np.arange(N, dtype=np.float64), D)[:, None]
    sets = {"detections": np.concatenate([idx, c - side / 2, c + side / 2], axis=1).astype(np.float32),
            "whole_image": np.concatenate([idx, np.tile([0.0, 0.0, W, H], (R, 1))], axis=1).astype(np.float32)}
    g = torch.Generator().manual_seed(4)
    rows_t = (torch.randn(R * P * P, ld, generator=g) * 0.5).to(dev)
    bias = torch.randn(K, generator=g).to(dev)
    # the planes the rows stand for, composed in torch as KeypointHead(raw=False) does
    F = torch.nn.functional
    cols = rows_t[:, :16 * K].view(R, P, P, 4, 4, K).permute(0, 5, 3, 4, 1, 2).reshape(R, 16 * K, P * P)
    low = F.fold(cols, (2 * P, 2 * P), kernel_size=4, stride=2, padding=1) + bias.view(1, K, 1, 1)
    planes = F.interpolate(low, scale_factor=2, mode="bilinear", align_corners=False).contiguous()
    kp, sc = torch.empty(R, K, 3, device=dev), torch.empty(R, K, device=dev)
    out = []
    for name, rois_np in sets.items():
        rois = torch.from_numpy(rois_np).to(dev)
        boxes = rois[:, 1:].contiguous()
        calls = {"planes": lambda: pkg.heatmaps_to_keypoints(planes, rois, max_side=max(IMAGE), out=kp, scores_out=sc),
                 "deconv_rows": lambda: pkg.heatmaps_to_keypoints(rows_t, rois, K=K, M=M, layout="deconv_rows", bias=bias,
                                                                  max_side=max(IMAGE), out=kp, scores_out=sc),
                 "torchvision loop": lambda: torchvision_loop(planes, boxes)}
        med, times = benchlib.interleaved(calls, a.trials, a.reps)
        # how often the two agree (torch's fp32 source coordinate and summation order differ: ties may fall elsewhere)
        got = pkg.heatmaps_to_keypoints(planes, rois, max_side=max(IMAGE))
        want = torchvision_loop(planes, boxes)
        torch.cuda.synchronize()
        same = float((got[0] == want[0]).all(dim=2).float().mean())
        pixels = float(np.ceil(np.maximum(rois_np[:, 3] - rois_np[:, 1], 1)) @ np.ceil(np.maximum(rois_np[:, 4] - rois_np[:, 2], 1)))
        out.append({"boxes": name, "planes_us": med["planes"], "deconv_rows_us": med["deconv_rows"],
                    "torchvision_loop_us": med["torchvision loop"], "loop_over_kernel": med["torchvision loop"] / med["deconv_rows"],
                    "resized_outputs_per_keypoint": pixels, "same_keypoints_as_loop": same,
                    "trials_us": {k: v for k, v in times.items()}})
        r = out[-1]
        print(f"{name:12s} planes {r['planes_us']:9.1f} us  deconv_rows {r['deconv_rows_us']:9.1f} us  torchvision loop "
              f"{r['torchvision_loop_us']:11.1f} us  ({r['loop_over_kernel']:.0f}x)  same keypoints {same:.4f}", flush=True)
    out.append({"workload": {"N": N, "D": D, "K": K, "M": M, "ld": ld, "image": IMAGE}})
    return out


def head_state_dict(C, seed=7):
    kc = benchlib.tests_module("keypoint_cases")
    return kc.keypoint_head_state_dict(C, [512] * 8, K, seed=seed)


def head_rows(a, pkg, dev):
    C, R = torch_nets.FPN_CHANNELS, N * D
    head = pkg.KeypointHead.from_state_dict(head_state_dict(C), C, dev)
    head.prepare(R, P)
    x = torch.zeros(R, P + 2, P + 2, C, device=dev)
    x[:, 1:-1, 1:-1] = torch.rand(R, P, P, C, device=dev) - 0.5
    head(x, raw=True)
    torch.cuda.synchronize()
    calls, src = {}, x
    for i, ((U, bias), dst, w) in enumerate(zip(head.convs, head._acts, head.widths)):
        calls[f"conv3x3 {i} ({int(src.shape[3])} -> {w})"] = (
            lambda s=src, U=U, b=bias, d=dst, w=w: pkg.conv3x3_bn_relu(s, U, b, head._ones[:w], relu=True, out=d))
        src = dst
    calls[f"deconv GEMM ({head.widths[-1]} -> {head.ld})"] = (
        lambda s=src: pkg.conv1x1_bn_ex(s, head.wd, head._zeros, head._ones[:head.ld], pkg.A_PADDED, out=head._rows))
    calls["whole forward (raw)"] = lambda: head(x, raw=True)
    calls["whole forward (logits composed in torch)"] = lambda: head(x)
    med, times = benchlib.interleaved(calls, a.trials, a.reps)
    rows = [{"launch": k, "us": med[k], "trials_us": times[k]} for k in calls]
    for r in rows:
        print(f"{r['launch']:45s} {r['us']:9.1f} us", flush=True)
    rows.append({"workload": {"R": R, "P": P, "in_channels": C, "widths": head.widths, "K": K, "ld": head.ld},
                 "sum_of_launches_us": sum(med[k] for k in list(calls)[:9])})
    return rows


def detector_rows(a, pkg, dev):
    """Keypoint R-CNN and Faster R-CNN on the same weights, eager and as one-graph replay (one model per variant: a graph
    holds its model's tensors)."""
    R, rc = benchlib.package_module("resnet"), benchlib.tests_module("roi_cases")
    C, An, classes = torch_nets.FPN_CHANNELS, 3, 2
    sd = {"backbone." + k: v for k, v in torch_nets.fpn_state_dict(R, "resnet50")[0].items()}
    g = torch.Generator().manual_seed(7)
    rn = lambda *s: torch.randn(*s, generator=g)
    sd.update({"rpn.head.conv.0.0.weight": rn(C, C, 3, 3) * (2.0 / (9 * C)) ** 0.5, "rpn.head.conv.0.0.bias": rn(C) * 0.1,
               "rpn.head.cls_logits.weight": rn(An, C, 1, 1) * (4.0 / C) ** 0.5, "rpn.head.cls_logits.bias": rn(An) * 0.1,
               "rpn.head.bbox_pred.weight": rn(4 * An, C, 1, 1) * (0.5 / C) ** 0.5, "rpn.head.bbox_pred.bias": rn(4 * An) * 0.05})
    sd.update({"roi_heads." + k: v for k, v in rc.box_head_state_dict(C, 7, 1024, classes, seed=7).items()})
    # two classes on random weights score every proposal alike, all person or none: a zero cls_score scores them all 0.5,
    # so that the keypoint branch has detections to work on whatever the seed
    sd["roi_heads.box_predictor.cls_score.weight"] = sd["roi_heads.box_predictor.cls_score.weight"] * 0
    sd["roi_heads.box_predictor.cls_score.bias"] = sd["roi_heads.box_predictor.cls_score.bias"] * 0
    full = dict(sd)
    full.update({"roi_heads." + k: v for k, v in head_state_dict(C).items()})
    x = (torch.rand(N, 3, *IMAGE, generator=g) - 0.5).to(dev)
    make = {"faster r-cnn": lambda: pkg.FasterRCNN.from_state_dict(sd, "resnet50"),
            "keypoint r-cnn": lambda: pkg.KeypointRCNN.from_state_dict(full, "resnet50")}
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
        print(f"{k:14s} eager {med['eager']:9.1f} us   graph {gmed['graph']:9.1f} us   detections {rows[-1]['detections']}",
              flush=True)
        del graph, eager, held
    rows.append({"keypoint_branch_graph_us": rows[1]["graph_us"] - rows[0]["graph_us"]})
    return rows


MODES = {"kernel": dict(fn=kernel_rows, trials=5, reps=2), "head": dict(fn=head_rows, trials=7, reps=3),
         "detector": dict(fn=detector_rows, trials=5, reps=3)}

if __name__ == "__main__":
    benchlib.main_rows("tools/keypoint_bench.py", MODES)
