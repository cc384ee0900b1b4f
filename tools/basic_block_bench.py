"""Developer tool (GPU box): the residual 3x3 layer and the ResNet basic block at ResNet-18/34's stage shapes.
usage: python tools/basic_block_bench.py bench [out.json] [--ns 1,8,32,128] [--trials 7] [--reps 20]
         in one process, the variants interleaved in every trial (median of the trials, events around `reps` calls):
         (a) the residual layer (wino_conv3x3_bn_add_relu_hw) against the plain layer of the same shape;
         (b) the block (wino_basic_block_hw) against the hand composition: two library launches, then torch's add and
             ReLU over the interior views of the two padded tensors;
         (c) the block against torch: F.conv2d on channels-last fp32, BN as scale and bias, add and ReLU
       python tools/basic_block_bench.py trace [--ns 128] [--reps 20]
         the residual and the plain layer back to back, then the block -- run it under
         `rocprofv3 --kernel-trace --stats -- python ...` to compare the kernels' own times in one trace"""
import benchlib
import torch
import torch.nn.functional as F

STAGES = {"conv2": (56, 64), "conv3": (28, 128), "conv4": (14, 256), "conv5": (7, 512)}   # (H, C)


class _Case:
    def __init__(self, pkg, N, H, C, dev):
        g = torch.Generator(device="cpu").manual_seed(N * H + C)
        x = torch.zeros(N, H + 2, H + 2, C)
        x[:, 1:-1, 1:-1, :] = torch.rand(N, H, H, C, generator=g) - 0.5
        self.x = x.to(dev)
        self.w = [((torch.rand(C, C, 3, 3, generator=g) - 0.5) / (9 * C) ** 0.5 * 2).to(dev) for _ in range(2)]
        self.bn = [((torch.rand(C, generator=g) - 0.5).to(dev), (torch.rand(C, generator=g) + 0.5).to(dev))
                   for _ in range(2)]
        self.U = [pkg.filter_transform_f2(w) for w in self.w]
        self.t1 = self.x.clone()
        self.t2 = torch.empty_like(self.x)
        self.out = torch.empty_like(self.x)
        self.ws = torch.empty(pkg.lib().wino_basic_block_workspace_bytes_hw(N, H, H, C) // 4, device=dev)
        self.x_cl = self.x[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
        self.pkg, self.N, self.H, self.C = pkg, N, H, C

    # (a)
    def plain_layer(self):
        b, s = self.bn[1]
        self.pkg.conv3x3_bn_relu(self.t1, self.U[1], b, s, out=self.out)

    def res_layer(self):
        b, s = self.bn[1]
        self.pkg.conv3x3_bn_add_relu(self.t1, self.U[1], b, s, self.x, out=self.out)

    # (b)
    def block(self):
        self.pkg.basic_block(self.x, self.U[0], self.bn[0], self.U[1], self.bn[1], out=self.out, workspace=self.ws)

    def composed(self):
        (b1, s1), (b2, s2) = self.bn
        self.pkg.conv3x3_bn_relu(self.x, self.U[0], b1, s1, out=self.t1)
        self.pkg.conv3x3_bn_relu(self.t1, self.U[1], b2, s2, relu=False, out=self.t2)
        o = self.out[:, 1:-1, 1:-1, :]
        torch.add(self.t2[:, 1:-1, 1:-1, :], self.x[:, 1:-1, 1:-1, :], out=o)
        o.relu_()

    # (c)
    def torch_block(self):
        (b1, s1), (b2, s2) = self.bn
        y = F.conv2d(self.x_cl, self.w[0], padding=1)
        y = torch.relu(y * s1[None, :, None, None] + b1[None, :, None, None])
        y = F.conv2d(y, self.w[1], padding=1)
        return torch.relu(y * s2[None, :, None, None] + b2[None, :, None, None] + self.x_cl)


def bench(a, pkg, dev):
    rows = []
    for stage, (H, C) in STAGES.items():
        for N in benchlib.ints(a.ns):
            c = _Case(pkg, N, H, C, dev)
            pkg.basic_block_prepare(N, H, H, C)
            variants = {"plain_layer": c.plain_layer, "res_layer": c.res_layer, "block": c.block,
                        "composed": c.composed, "torch": c.torch_block}
            med, times = benchlib.interleaved(variants, a.trials, a.reps)
            row = {"stage": stage, "H": H, "C": C, "N": N, "median_us": med, "trials_us": times,
                   "res_over_plain": med["res_layer"] / med["plain_layer"],
                   "block_over_composed": med["block"] / med["composed"],
                   "block_over_torch": med["block"] / med["torch"]}
            rows.append(row)
            print(f"{stage} N={N:4d}  res/plain {med['res_layer']:8.1f}/{med['plain_layer']:8.1f} us "
                  f"({row['res_over_plain']:.3f})  block/composed {med['block']:8.1f}/{med['composed']:8.1f} us "
                  f"({row['block_over_composed']:.3f})  torch {med['torch']:8.1f} us ({row['block_over_torch']:.3f})",
                  flush=True)
            del c
            torch.cuda.empty_cache()
    return rows


def trace(a, pkg, dev):
    for stage, (H, C) in STAGES.items():
        for N in benchlib.ints(a.ns):
            c = _Case(pkg, N, H, C, dev)
            for fn in (c.res_layer, c.plain_layer, c.block):
                for _ in range(a.reps):
                    fn()
            torch.cuda.synchronize()
            print(f"{stage} N={N}: {a.reps} x (residual layer, plain layer, block)", flush=True)


MODES = {"bench": dict(fn=bench, ns="1,8,32,128", trials=7, reps=20),
         "trace": dict(fn=trace, ns="128", reps=20)}


def main():
    benchlib.main_rows("tools/basic_block_bench.py", MODES)


if __name__ == "__main__":
    main()
