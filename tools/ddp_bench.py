#!/usr/bin/env python3
"""Time the distributed-DP client pass in ONE process on one GPU (numbers of different runs are never compared).

At the iresnet100 parameter count (65 156 160 fp32), for a client among K = 8 (7 pair masks + 1 self mask = 8 streams):

    secagg_mask k=8       fedfr_secagg_mask: encode + masks (the pass distributed DP replaces)
    secagg_mask_dp k=8    fedfr_secagg_mask_dp: clip factor from the device, encode, sum of squares, discrete Gaussian noise, masks
    secagg_mask_dp k=0    the same without masks: encode + noise
    dgauss_fill           the sampler alone (block layout, 64 B per lane: not the layout of the pass)
    fedopt_sqnorm k=1     the norm pass that precedes mask_dp

All rows are timed in interleaved rounds (row A, B, C, ..., A, B, C, ...), every launch between its own pair of HIP events after --warmup
rounds; each row reports the MEAN of --reps launches with its standard deviation, minimum and maximum, and the noise values per second.
No GPU: an error.
usage: python tools/ddp_bench.py [--n N] [--sigma S] [--reps 20] [--warmup 3] [--limit 240] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import signal
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IRESNET100_PARAMS = 65156160


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=IRESNET100_PARAMS)
    ap.add_argument("--sigma", type=float, default=29308.59, help="sigma_int (default: z = 1, C = 1, f = 16, T = 5)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds after which the process gives up")
    ap.add_argument("--out", default=None, help="also write the JSON result line to this file")
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: (sys.stderr.write("ddp_bench: time limit of %d s reached\n" % a.limit), os._exit(3)))
    signal.alarm(a.limit)

    import numpy as np
    import torch
    from fedfr_amd import _C
    from fedfr_amd.server import ServerOptimizer
    if not torch.cuda.is_available():
        sys.exit("ddp_bench: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    n = a.n
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(n, generator=g, device=dev) - 0.5
    xi = x + 0.01 * (torch.rand(n, generator=g, device=dev) - 0.5)
    y = torch.empty(n, dtype=torch.int32, device=dev)
    counters = torch.zeros(3, dtype=torch.int32, device=dev)
    sqnorm = torch.zeros(1, dtype=torch.int64, device=dev)
    st = _C.stream()
    rng = np.random.default_rng(1)
    keys = (C.c_uint * (8 * 32))(*[int(v) for v in rng.integers(0, 2 ** 32, 8 * 32)])
    nonces = (C.c_uint * (3 * 32))(*[int(v) for v in rng.integers(0, 2 ** 32, 3 * 32)])
    signs = (C.c_int * 32)(*[1 if s % 3 else -1 for s in range(32)])
    limit = (2 ** 31 - 1) // 8 - 37 * (int(a.sigma) + 1)
    clipper = ServerOptimizer("AVGM", clip_norm=1.0)
    factor = clipper.coefficients(x, [xi], [1.0])

    def mask(k):
        _C.call("fedfr_secagg_mask", y.data_ptr(), x.data_ptr(), xi.data_ptr(), float(2.0 ** 16), limit, keys, nonces, signs, k, n, counters.data_ptr(), st)

    def mask_dp(k):
        _C.call("fedfr_secagg_mask_dp", y.data_ptr(), x.data_ptr(), xi.data_ptr(), factor.data_ptr(), 16, limit, 12345, 1, 0, a.sigma, keys, nonces, signs, k, n,
                counters.data_ptr(), sqnorm.data_ptr(), st)

    def fill():
        _C.call("fedfr_dgauss_fill", y.data_ptr(), n, 12345, 1, 7, 0, a.sigma, counters.data_ptr() + 8, st)

    def sqnorm_pass():
        clipper.coefficients(x, [xi], [1.0])

    group = [("secagg_mask k=8", lambda: mask(8), 0), ("secagg_mask_dp k=8", lambda: mask_dp(8), n), ("secagg_mask_dp k=0", lambda: mask_dp(0), n),
             ("dgauss_fill", fill, n), ("fedopt_sqnorm k=1", sqnorm_pass, 0)]
    for _ in range(a.warmup):
        for _, fn, _ in group:
            fn()
    torch.cuda.synchronize()
    ev = {name: [] for name, _, _ in group}
    for _ in range(a.reps):
        for name, fn, _ in group:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            ev[name].append((e0, e1))
    torch.cuda.synchronize()
    res = {}
    for name, _, draws in group:
        ms = np.array([e0.elapsed_time(e1) for e0, e1 in ev[name]])
        res[name] = {"ms_mean": float(ms.mean()), "ms_std": float(ms.std(ddof=1)) if ms.size > 1 else 0.0, "ms_min": float(ms.min()), "ms_max": float(ms.max()),
                     "giga_draws_per_s": draws / ms.mean() / 1e6}
        print("%-20s %.3f ms mean (std %.3f, min %.3f, max %.3f)%s"
              % (name, ms.mean(), res[name]["ms_std"], ms.min(), ms.max(), "  %.1f G noise values/s" % res[name]["giga_draws_per_s"] if draws else ""))
    exhausted = int(counters[2].item())
    assert exhausted == 0, "the sampler exhausted its attempts on %d elements" % exhausted
    line = json.dumps({"n": n, "sigma": a.sigma, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "kernels": res})
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    signal.alarm(0)


if __name__ == "__main__":
    main()
