"""Developer tool (GPU box): the stride-2 3x3 layer (wino_conv3x3_s2_bn_relu_hw, the 1x1 kernels in tap form).
usage: python tools/conv3x3_s2_bench.py trace [--ns 128] [--reps 20]
         the tap layer and the plain 1x1 GEMM of the same shape (M = N*H*W, 9C, K; random A) back to back at the
         conv3/4/5 shapes -- run it under `rocprofv3 --kernel-trace --stats -- python ...` and compare the two kernels'
         times in one trace; prints the in-kernel clock of the last plain GEMM launch
       python tools/conv3x3_s2_bench.py policy [out.json] [--ns 1,2,8,16,32,128] [--trials 5] [--reps 30]
         the automatic plan against every forced form (latency KS x RT x CT, tiled, stream-K) at the conv3/4/5 shapes,
         interleaved rounds between events; reports each form's median and automatic / best forced"""
import os

import benchlib
import torch

STAGES = {"conv3": (56, 128), "conv4": (28, 256), "conv5": (14, 512)}   # (Hin, C = K)
KNOBS = ("WINO_1X1_ALGO", "WINO_1X1_SMALL_KS", "WINO_1X1_SMALL_RT", "WINO_1X1_SMALL_CT", "WINO_1X1_SK", "WINO_1X1_SK_GRID")


def _set(pkg, **kv):
    for k in KNOBS:
        os.environ.pop(k, None)
    for k, v in kv.items():
        os.environ[k] = str(v)
    pkg.lib().wino_debug_reload_knobs()


def _layer(N, Hin, C, K, dev):
    g = torch.Generator(device="cpu").manual_seed(N * Hin + C)
    x = torch.zeros(N, Hin + 2, Hin + 2, C)
    x[:, 1:-1, 1:-1, :] = torch.rand(N, Hin, Hin, C, generator=g) - 0.5
    w = (torch.rand(K, C, 3, 3, generator=g) - 0.5) / (9 * C) ** 0.5
    b, s = torch.rand(K, generator=g) - 0.5, torch.rand(K, generator=g) + 0.5
    return x.to(dev), w.to(dev), b.to(dev), s.to(dev)


def trace(a, pkg, dev):
    for stage, (Hin, C) in STAGES.items():
        for N in benchlib.ints(a.ns):
            H = (Hin - 1) // 2 + 1
            x, w, b, s = _layer(N, Hin, C, C, dev)
            taps = pkg.filter_pack_s2(w)
            M = N * H * H
            A = torch.rand(M, 9 * C, device=dev) - 0.5
            Bm = taps.reshape(9 * C, C)
            out = torch.empty(N, H + 2, H + 2, C, device=dev)
            out1 = torch.empty(M, C, device=dev)
            for _ in range(a.reps):
                pkg.conv3x3_s2_bn_relu(x, taps, b, s, out=out)
            for _ in range(a.reps):
                pkg.conv1x1_bn_ex(A, Bm, b, s, pkg.RELU, out=out1)
            # (wino_diag_last_clock reads conv1x1.hip's stamp slot: the plain GEMM's; the tap kernels stamp their own copy)
            c_gemm = pkg.last_clock_ghz(1)
            torch.cuda.synchronize()
            print(f"{stage} N={N}: M={M} K={9 * C} Kout={C} form {pkg.conv3x3_s2_plan(N, Hin, Hin, C, C)}  "
                  f"clock of the last gemm {c_gemm[0] if c_gemm else 0:.2f} GHz", flush=True)


def _forms(C, K):
    forms = {"auto": {}}
    for ks in (1, 2, 4):
        for rt in (1, 2):
            for ct in (1, 2, 4):
                if (9 * C) % (16 * ks) == 0 and K % ((4 // ks) * ct * 16) == 0 and (9 * C) // ks >= 64:
                    forms[f"lat_ks{ks}_rt{rt}_ct{ct}"] = dict(WINO_1X1_ALGO="small", WINO_1X1_SMALL_KS=ks,
                                                             WINO_1X1_SMALL_RT=rt, WINO_1X1_SMALL_CT=ct)
    forms["tiled"] = dict(WINO_1X1_ALGO="big", WINO_1X1_SK=0)
    forms["stream_k"] = dict(WINO_1X1_ALGO="big", WINO_1X1_SK=1)
    return forms


def policy(a, pkg, dev):
    rows = []
    for stage, (Hin, C) in STAGES.items():
        for N in benchlib.ints(a.ns):
            H = (Hin - 1) // 2 + 1
            x, w, b, s = _layer(N, Hin, C, C, dev)
            taps = pkg.filter_pack_s2(w)
            out = torch.empty(N, H + 2, H + 2, C, device=dev)
            forms = _forms(C, C)
            plans = {}
            for name, kv in forms.items():
                _set(pkg, **kv)
                plans[name] = pkg.conv3x3_s2_plan(N, Hin, Hin, C, C)
                pkg.conv3x3_s2_prepare(N, Hin, Hin, C, C)
            run = lambda: pkg.conv3x3_s2_bn_relu(x, taps, b, s, out=out)
            med, times = benchlib.interleaved({k: run for k in forms}, a.trials, a.reps, preheat_s=0.3,
                                              setups={k: (lambda kv=kv: _set(pkg, **kv)) for k, kv in forms.items()})
            best = min((v, k) for k, v in med.items() if k != "auto")
            row = {"stage": stage, "N": N, "auto_form": plans["auto"], "auto_us": med["auto"], "best_forced": best[1],
                   "best_forced_us": best[0], "auto_over_best": med["auto"] / best[0], "median_us": med,
                   "trials_us": times}
            rows.append(row)
            print(f"{stage} N={N:4d} auto {med['auto']:8.1f} us (form {plans['auto']})  best forced {best[1]} "
                  f"{best[0]:8.1f} us  ratio {row['auto_over_best']:.3f}", flush=True)
            _set(pkg)
    return rows


MODES = {"trace": dict(fn=trace, ns="128", reps=20),
         "policy": dict(fn=policy, ns="1,2,8,16,32,128", trials=5, reps=30)}


def main():
    benchlib.main_rows("tools/conv3x3_s2_bench.py", MODES)


if __name__ == "__main__":
    main()
