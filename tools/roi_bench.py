"""Developer tool (GPU box): multi-scale RoIAlign and the R-CNN heads at the detection workload's points.
usage: python tools/roi_bench.py [profiles/roi/bench.json] [--trials 7] [--reps 10]
  The pyramid of ResNet-50-FPN at N = 2, 800 x 1344 (200x336 / 100x168 / 50x84 / 25x42, C = 256, padded as ResNetFPN
  writes it), boxes log-uniform in size so that all four levels are hit:
    kernel   wino_roi_align_hw at R = 2000, P = 7 unpadded (the box branch) and R = 200, P = 14 padded (the mask branch),
             against the store-bound floor -- output bytes over the HBM rate bench.py's roofline uses -- and against a
             torch composition of the same arithmetic (index gathers + weighted sum), eager and as one-graph replay
    heads    BoxHead (1024-wide, 91 classes) at R = 2000 and MaskHead (91 classes) at R = 200, launch by launch, and the
             whole forward eager against one-graph replay
    error    the torch-fp32 restatement against fp64 at the 200 x 336 level (why no tight claim is made for full-size maps)
(median of the trials, events around `reps` calls)"""
import benchlib
import torch

HBM_GBS = 8000.0                        # bench.py's HBM_PEAK_GBS
IMAGE, N, C = (800, 1344), 2, 256
LEVEL_HW = [(200, 336), (100, 168), (50, 84), (25, 42)]
SCALES = [1 / 4, 1 / 8, 1 / 16, 1 / 32]
POINTS = [("box branch", 2000, 7, False), ("mask branch", 200, 14, True)]


def make_boxes(R, seed, dev):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(R, 5, generator=g, dtype=torch.float64)
    size = 16.0 * (800.0 / 16.0) ** u[:, 0]                    # sqrt(area), log-uniform
    aspect = torch.exp(1.4 * u[:, 1] - 0.7)
    w, h = (size * aspect.sqrt()).clamp(max=IMAGE[1]), (size / aspect.sqrt()).clamp(max=IMAGE[0])
    x1, y1 = (IMAGE[1] - w) * u[:, 2], (IMAGE[0] - h) * u[:, 3]
    n = (u[:, 4] * N).floor()
    return torch.stack([n, x1, y1, x1 + w, y1 + h], dim=1).float().to(dev)


def torch_roi_align(maps, rois, P, S, sels):
    """The same arithmetic as a torch composition on the device: per level, index gathers of the four taps and a
    weighted sum (fp32).  maps unpadded [N][h][w][C]; sels[l]: the indices of level l's boxes (found beforehand, so that
    the composition has static shapes and can be captured into a graph)."""
    out = torch.zeros(rois.shape[0], P, P, maps[0].shape[3], device=rois.device)
    for l, m in enumerate(maps):
        sel = sels[l]
        if sel.numel() == 0:
            continue
        b = rois[sel]
        h, w = m.shape[1], m.shape[2]
        sx, sy, ex, ey = (b[:, i] * SCALES[l] for i in (1, 2, 3, 4))
        bw, bh = (ex - sx).clamp(min=1) / P, (ey - sy).clamp(min=1) / P
        p = torch.arange(P, device=b.device, dtype=torch.float32)[None, :, None]
        i = (torch.arange(S, device=b.device, dtype=torch.float32) + 0.5)[None, None, :]
        ys = (sy[:, None, None] + p * bh[:, None, None] + i * bh[:, None, None] / S).flatten(1)   # [R][P*S]
        xs = (sx[:, None, None] + p * bw[:, None, None] + i * bw[:, None, None] / S).flatten(1)

        def taps(v, size):
            ok = (v >= -1) & (v <= size)
            c = torch.where(ok, v.clamp(min=0), torch.zeros_like(v))
            lo = c.floor().long()
            edge = lo >= size - 1
            lo = torch.where(edge, torch.full_like(lo, size - 1), lo)
            hi = torch.where(edge, lo, lo + 1)
            frac = torch.where(edge, torch.zeros_like(c), c - lo.float())
            return lo, hi, frac * ok, (1 - frac) * ok

        ylo, yhi, ly, hy = taps(ys, h)
        xlo, xhi, lx, hx = taps(xs, w)
        img = b[:, 0].long()[:, None, None]
        acc = 0
        for yi, wy in ((ylo, hy), (yhi, ly)):
            for xi, wx in ((xlo, hx), (xhi, lx)):
                v = m[img, yi[:, :, None], xi[:, None, :]]                                   # [R][P*S][P*S][C]
                acc = acc + (wy[:, :, None] * wx[:, None, :])[..., None] * v
        R_l = sel.numel()
        out[sel] = acc.view(R_l, P, S, P, S, -1).sum(dim=(2, 4)) / (S * S)
    return out


def kernel_rows(a, pkg, dev):
    rc = benchlib.tests_module("roi_cases")
    rows = []
    g = torch.Generator().manual_seed(1)
    padded = [torch.zeros(N, h + 2, w + 2, C) for h, w in LEVEL_HW]
    for p in padded:
        p[:, 1:-1, 1:-1, :] = torch.rand(N, p.shape[1] - 2, p.shape[2] - 2, C, generator=g) - 0.5
    padded = [p.to(dev) for p in padded]
    plain = [p[:, 1:-1, 1:-1, :].contiguous() for p in padded]
    for name, R, P, out_padded in POINTS:
        rois = make_boxes(R, R, dev)
        levels = rc.threshold_levels(rois.cpu(), SCALES, 224.0, 4).to(dev)
        q = 2 if out_padded else 0
        out = torch.empty(R, P + q, P + q, C, device=dev)
        kern = lambda: pkg.roi_align(padded, rois, P, SCALES, 2, True, out_padded, out=out)
        sels = [torch.nonzero(levels == l).flatten() for l in range(4)]
        comp = lambda: torch_roi_align(plain, rois, P, 2, sels)
        got = kern()
        got = got[:, 1:-1, 1:-1, :] if out_padded else got
        ref = comp()
        diff = float((got - ref).abs().max() / ref.abs().max())
        variants = {"kernel": kern, "torch": comp}
        med, times = benchlib.interleaved(variants, a.trials, a.reps)
        graphs = {k: benchlib.captured(benchlib.repeated(fn, a.reps))[0] for k, fn in variants.items()}
        gmed, gtimes = benchlib.interleaved({k: gr.replay for k, gr in graphs.items()}, a.trials, 3)
        gmed = {k: v / a.reps for k, v in gmed.items()}
        del graphs
        floor = out.numel() * 4.0 / HBM_GBS / 1e3     # us
        rows.append({"point": name, "R": R, "P": P, "out_padded": out_padded, "levels_hit": torch.bincount(levels, minlength=4).tolist(),
                     "store_floor_us": floor, "eager_us": med, "graph_us": gmed, "trials_eager_us": times,
                     "trials_graph_us": {k: [t / a.reps for t in v] for k, v in gtimes.items()},
                     "kernel_over_floor": gmed["kernel"] / floor, "kernel_over_torch": gmed["kernel"] / gmed["torch"],
                     "rel_diff_to_torch_fp32": diff})
        print(f"roi_align {name}: R={R} P={P} padded={out_padded}  levels {rows[-1]['levels_hit']}  kernel {gmed['kernel']:.1f} us "
              f"graph / {med['kernel']:.1f} eager (floor {floor:.1f}: {rows[-1]['kernel_over_floor']:.2f}x)  torch {gmed['torch']:.1f} "
              f"graph / {med['torch']:.1f} eager  kernel/torch {rows[-1]['kernel_over_torch']:.4f}  (rel diff {diff:.1e})", flush=True)
        del out, ref, got
        torch.cuda.empty_cache()
    return rows


def head_rows(a, pkg, dev):
    rc = benchlib.tests_module("roi_cases")
    rows = []
    classes, rep = 91, 1024
    box = pkg.BoxHead.from_state_dict(rc.box_head_state_dict(C, 7, rep, classes), in_channels=C, P=7)
    mask = pkg.MaskHead.from_state_dict(rc.mask_head_state_dict(C, classes), in_channels=C)
    g = torch.Generator().manual_seed(2)
    p7 = (torch.rand(2000, 7, 7, C, generator=g) - 0.5).to(dev)
    p14 = torch.zeros(200, 16, 16, C)
    p14[:, 1:-1, 1:-1, :] = torch.rand(200, 14, 14, C, generator=g) - 0.5
    p14 = p14.to(dev)
    box.prepare(2000)
    mask.prepare(200, 14)
    ones, kp, kl, R, Rm, P = box._ones, int(box.wp.shape[1]), int(mask.wl.shape[1]), 2000, 200, 14
    launches = {
        "box.fc6": lambda: pkg.conv1x1_bn(p7.view(R, -1), box.w6, box.b6, ones[:rep], True, out=box._h6),
        "box.fc7": lambda: pkg.conv1x1_bn(box._h6, box.w7, box.b7, ones[:rep], True, out=box._h7),
        "box.predictor": lambda: pkg.conv1x1_bn(box._h7, box.wp, box.bp, ones[:kp], False, out=box._scores),
        "mask.conv3x3": lambda: pkg.conv3x3_bn_relu(p14, *mask.convs[0], mask._ones[:C], relu=True, out=mask._a),
        "mask.deconv": lambda: pkg.conv1x1_bn_ex(mask._a, mask.wd, mask.bd, mask._ones[:4 * C], pkg.A_PADDED | pkg.RELU,
                                                 out=mask._up, hw=(P, P)),
        "mask.logits": lambda: pkg.conv1x1_bn(mask._up.view(Rm * P * P * 4, C), mask.wl, mask.bl, mask._ones[:kl], False,
                                              out=mask._scores),
        "box head": lambda: box(p7),
        "mask head": lambda: mask(p14),
    }
    med, times = benchlib.interleaved(launches, a.trials, a.reps)
    graphs = {k: benchlib.captured(benchlib.repeated(fn, a.reps))[0] for k, fn in launches.items()}
    gmed, _ = benchlib.interleaved({k: gr.replay for k, gr in graphs.items()}, a.trials, 3)
    gmed = {k: v / a.reps for k, v in gmed.items()}
    del graphs
    for k in launches:
        rows.append({"what": k, "eager_us": med[k], "graph_us": gmed[k]})
        print(f"{k:14s} eager {med[k]:8.1f} us   graph {gmed[k]:8.1f} us", flush=True)
    return rows


def restatement_error():
    """torch fp32 against fp64 at the workload's finest level, 200 x 336, on the CPU (C = 8 is enough: the error is
    in the coordinates and weights)."""
    rc = benchlib.tests_module("roi_cases")
    g = torch.Generator().manual_seed(3)
    fmap = torch.rand(N, 200, 336, 8, generator=g) - 0.5
    rois = make_boxes(300, 3, "cpu")
    rois = rois[rc.threshold_levels(rois, SCALES, 224.0, 4) == 0]
    zeros = torch.zeros(rois.shape[0], dtype=torch.int64)
    res = {}
    for P in (7, 14):
        want = rc.roi_align_reference([fmap], rois, P, (0.25,), 2, zeros)
        got = rc.roi_align_reference([fmap], rois, P, (0.25,), 2, zeros, dtype=torch.float32)
        res[f"P={P}"] = rc.rel_err(got, want)
        print(f"fp32 restatement at 200x336, {rois.shape[0]} boxes, P={P}: {res[f'P={P}']:.2e}", flush=True)
    return res


MODES = {None: dict(trials=7, reps=10)}


def main():
    a = benchlib.parse(MODES)
    pkg = benchlib.load_package()
    dev = torch.device("cuda:0")
    result = benchlib.header("tools/roi_bench.py", trials=a.trials, reps=a.reps,
                             workload={"N": N, "image": IMAGE, "C": C, "levels": LEVEL_HW}, hbm_gbs=HBM_GBS)
    result["kernel"] = kernel_rows(a, pkg, dev)
    result["heads"] = head_rows(a, pkg, dev)
    result["fp32_restatement_rel_err_200x336"] = restatement_error()
    benchlib.write_json(a.out, result)


if __name__ == "__main__":
    main()
