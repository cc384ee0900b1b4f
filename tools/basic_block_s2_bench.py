"""Developer tool (GPU box): the fused stride-2 3x3 + shortcut layer and the downsampling basic block at ResNet-18/34's
downsampling shapes.
usage: python tools/basic_block_s2_bench.py bench [out.json] [--ns 1,8,32,128] [--trials 7] [--reps 20]
         in one process, the variants interleaved in every trial (median of the trials, events around `reps` calls):
         (a) the fused layer (wino_conv3x3_s2_proj_bn_relu_hw) against the plain stride-2 3x3 alone, and against the
             plain stride-2 3x3 plus a separate shortcut 1x1 (conv1x1_bn_ex with WINO_C_PADDED on
             x[:, 1:-1:2, 1:-1:2] made contiguous);
         (b) the block (wino_basic_block_s2_hw) against that three-launch library composition, then the residual 3x3
             in place -- the contiguous copy of the strided x included, as a user has to make it;
         (c) the block against torch: F.conv2d on channels-last fp32, BN as scale and bias, add and ReLU
       python tools/basic_block_s2_bench.py trace [--ns 128] [--reps 20]
         the fused layer, the plain stride-2 3x3 and the block back to back -- run it under
         `rocprofv3 --kernel-trace --stats -- python ...` to compare the kernels' own times in one trace"""
import benchlib
import torch
import torch.nn.functional as F

STAGES = {"conv3": (56, 64, 128), "conv4": (28, 128, 256), "conv5": (14, 256, 512)}   # (Hin, C, K)


class _Case:
    def __init__(self, pkg, N, Hin, C, K, dev):
        g = torch.Generator(device="cpu").manual_seed(N * Hin + C)
        x = torch.zeros(N, Hin + 2, Hin + 2, C)
        x[:, 1:-1, 1:-1, :] = torch.rand(N, Hin, Hin, C, generator=g) - 0.5
        self.x = x.to(dev)
        H = (Hin - 1) // 2 + 1
        rnd = lambda *s, fan: ((torch.rand(*s, generator=g) - 0.5) / fan ** 0.5 * 2).to(dev)
        self.w1, self.w2, self.wd = rnd(K, C, 3, 3, fan=9 * C), rnd(K, K, 3, 3, fan=9 * K), rnd(K, C, fan=C)
        self.bn = [((torch.rand(K, generator=g) - 0.5).to(dev), (torch.rand(K, generator=g) + 0.5).to(dev))
                   for _ in range(3)]   # bn1, bnd, bn2
        self.taps = pkg.filter_pack_s2(self.w1)
        self.wd_ck = self.wd.t().contiguous()
        self.packed = pkg.s2_proj_pack(self.taps, self.bn[0], self.wd_ck, self.bn[1])
        self.U2 = pkg.filter_transform_f2(self.w2)
        self.t1 = torch.empty(N, H + 2, H + 2, K, device=dev)
        self.out = torch.empty_like(self.t1)
        self.ws = torch.empty(pkg.lib().wino_basic_block_s2_workspace_bytes_hw(N, Hin, Hin, K) // 4, device=dev)
        self.xs = torch.empty(N, H, H, C, device=dev)
        self.x_cl = self.x[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
        self.pkg, self.N, self.Hin, self.H, self.C, self.K = pkg, N, Hin, H, C, K

    # (a)
    def fused_layer(self):
        self.pkg.conv3x3_s2_proj(self.x, self.packed, t1=self.t1, sc=self.out)

    def plain_layer(self):
        b, s = self.bn[0]
        self.pkg.conv3x3_s2_bn_relu(self.x, self.taps, b, s, out=self.t1)

    def shortcut(self):
        self.xs.copy_(self.x[:, 1:-1:2, 1:-1:2, :])
        b, s = self.bn[1]
        self.pkg.conv1x1_bn_ex(self.xs, self.wd_ck, b, s, self.pkg.C_PADDED, out=self.out, hw=(self.H, self.H))

    def plain_and_shortcut(self):
        self.plain_layer()
        self.shortcut()

    # (b)
    def block(self):
        self.pkg.basic_block_s2(self.x, self.packed, self.U2, self.bn[2], out=self.out, workspace=self.ws)

    def composed(self):
        self.plain_and_shortcut()
        b, s = self.bn[2]
        self.pkg.conv3x3_bn_add_relu(self.t1, self.U2, b, s, self.out, out=self.out)

    # (c)
    def torch_block(self):
        (b1, s1), (bd, sd), (b2, s2) = self.bn
        c = lambda v: v[None, :, None, None]
        y = torch.relu(F.conv2d(self.x_cl, self.w1, stride=2, padding=1) * c(s1) + c(b1))
        y = F.conv2d(y, self.w2, padding=1) * c(s2) + c(b2)
        sc = F.conv2d(self.x_cl, self.wd[:, :, None, None], stride=2) * c(sd) + c(bd)
        return torch.relu(y + sc)


def bench(a, pkg, dev):
    rows = []
    for stage, (Hin, C, K) in STAGES.items():
        for N in benchlib.ints(a.ns):
            c = _Case(pkg, N, Hin, C, K, dev)
            pkg.basic_block_s2_prepare(N, Hin, Hin, C, K)
            variants = {"fused_layer": c.fused_layer, "plain_layer": c.plain_layer,
                        "plain_and_shortcut": c.plain_and_shortcut, "block": c.block, "composed": c.composed,
                        "torch": c.torch_block}
            med, times = benchlib.interleaved(variants, a.trials, a.reps)
            row = {"stage": stage, "Hin": Hin, "C": C, "K": K, "N": N, "median_us": med, "trials_us": times,
                   "fused_over_plain": med["fused_layer"] / med["plain_layer"],
                   "fused_over_plain_and_shortcut": med["fused_layer"] / med["plain_and_shortcut"],
                   "block_over_composed": med["block"] / med["composed"],
                   "block_over_torch": med["block"] / med["torch"]}
            rows.append(row)
            print(f"{stage} N={N:4d}  fused {med['fused_layer']:8.1f} us: /plain {row['fused_over_plain']:.3f} "
                  f"/plain+sc {row['fused_over_plain_and_shortcut']:.3f}  block {med['block']:8.1f} us: "
                  f"/composed {row['block_over_composed']:.3f} /torch {row['block_over_torch']:.3f}", flush=True)
            del c
            torch.cuda.empty_cache()
    return rows


def trace(a, pkg, dev):
    for stage, (Hin, C, K) in STAGES.items():
        for N in benchlib.ints(a.ns):
            c = _Case(pkg, N, Hin, C, K, dev)
            for fn in (c.fused_layer, c.plain_layer, c.shortcut, c.block):
                for _ in range(a.reps):
                    fn()
            torch.cuda.synchronize()
            print(f"{stage} N={N}: {a.reps} x (fused layer, plain stride-2 layer, shortcut 1x1, block)", flush=True)


MODES = {"bench": dict(fn=bench, ns="1,8,32,128", trials=7, reps=20),
         "trace": dict(fn=trace, ns="128", reps=20)}


def main():
    benchlib.main_rows("tools/basic_block_s2_bench.py", MODES)


if __name__ == "__main__":
    main()
