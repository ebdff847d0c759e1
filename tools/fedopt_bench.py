#!/usr/bin/env python3
"""Time the server-optimiser kernels against fedfr_fedavg_multi, their yardstick, in ONE process on one GPU.

At the iresnet100 parameter count (65 156 160 fp32) and k = 8 client states: fedfr_fedavg_multi, fedfr_fedopt_sqnorm and fedfr_fedopt_multi
for FedAvgM and FedAdam, each timed with HIP events over --reps launches after --warmup (every launch its own event pair; median and
min reported), and the achieved GB/s against the bytes the algorithm needs:

    fedavg_multi   (k + 1) n 4 B                      k states read, the aggregate written
    sqnorm         (k + 1) n 4 B                      x and k states read (+ 8 k grid B of partials)
    AVGM           (k + 2) n 4 B read + 2 n 4 B written      x, m, k states -> x', m'
    ADAM           (k + 3) n 4 B read + 3 n 4 B written      x, m, v, k states -> x', m', v'

All four are one-pass streaming kernels with the same access pattern, so fedavg_multi's GB/s FROM THE SAME RUN is what the others are
compared with.  The states total (k + 5) n 4 B = 3.4 GB: far beyond the caches, every launch reads HBM.  No GPU: an error, not a fallback.
usage: python tools/fedopt_bench.py [--n N] [--k K] [--reps 20] [--warmup 3] [--limit 120]
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
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds after which the process gives up")
    a = ap.parse_args()
    if not 1 <= a.k <= 8:
        ap.error("--k must be 1..8 (one pass)")
    signal.signal(signal.SIGALRM, lambda *_: (sys.stderr.write("fedopt_bench: time limit of %d s reached\n" % a.limit), os._exit(3)))
    signal.alarm(a.limit)

    import numpy as np
    import torch
    from fedfr_amd import _C
    if not torch.cuda.is_available():
        sys.exit("fedopt_bench: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    n, k = a.n, a.k
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(n, generator=g, device=dev) - 0.5
    xs = [x + 0.01 * (torch.rand(n, generator=g, device=dev) - 0.5) for _ in range(k)]
    m = 0.01 * (torch.rand(n, generator=g, device=dev) - 0.5)
    v = torch.full((n,), 1e-6, device=dev) + 1e-4 * torch.rand(n, generator=g, device=dev)
    out = torch.empty_like(x)
    ptrs = (C.c_void_p * k)(*[t.data_ptr() for t in xs])
    wv = (C.c_float * k)(*[float(np.float32(1.0 / k))] * k)
    lib = _C.lib()
    ws = torch.empty(lib.fedfr_fedopt_sqnorm_workspace_bytes(k, n) // 8, dtype=torch.float64, device=dev)
    sq = torch.empty(k, dtype=torch.float64, device=dev)
    coef = torch.empty(k, dtype=torch.float32, device=dev)
    st = _C.stream()
    f = np.float32
    hyp = [float(t) for t in (f(1.0), f(0.9), f(1) - f(0.9), f(0.99), f(1) - f(0.99), f(1e-3))]

    def fedavg():
        _C.call("fedfr_fedavg_multi", out.data_ptr(), ptrs, wv, k, n, 0, st)

    def sqnorm():
        _C.call("fedfr_fedopt_sqnorm", x.data_ptr(), ptrs, wv, k, n, 1.0, sq.data_ptr(), coef.data_ptr(), ws.data_ptr(), ws.numel() * 8, st)

    def opt(kind):
        def run():      # m, v keep evolving across launches: the work per launch does not depend on their values
            _C.call("fedfr_fedopt_multi", kind, out.data_ptr(), x.data_ptr(), ptrs, coef.data_ptr(), k, n, m.data_ptr(), v.data_ptr(), None, 1, 1,
                    *hyp, st)
        return run

    cases = [("fedavg_multi", fedavg, (k + 1) * n * 4), ("fedopt_sqnorm", sqnorm, (k + 1) * n * 4 + 8 * k * (ws.numel() // k)),
             ("fedopt_multi AVGM", opt(0), (k + 2) * n * 4 + 2 * n * 4), ("fedopt_multi ADAM", opt(2), (k + 3) * n * 4 + 3 * n * 4)]
    sqnorm()                                   # coef for the optimiser launches
    res = {}
    for name, fn, nbytes in cases:
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        med = ms[len(ms) // 2]
        res[name] = {"bytes": nbytes, "ms_median": med, "ms_min": ms[0], "ms_max": ms[-1], "gbps_median": nbytes / med / 1e6}
        print("%-18s n=%d k=%d  %.3f ms median (min %.3f, max %.3f)  %.0f GB/s of %.1f MB" % (name, n, k, med, ms[0], ms[-1], nbytes / med / 1e6, nbytes / 1e6))
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(sq).all())
    base = res["fedavg_multi"]["gbps_median"]
    for name in res:
        res[name]["vs_fedavg_multi"] = res[name]["gbps_median"] / base
    print(json.dumps({"n": n, "k": k, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "kernels": res}))
    signal.alarm(0)


if __name__ == "__main__":
    main()
