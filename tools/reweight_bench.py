#!/usr/bin/env python3
"""Time the reweighted-aggregation kernels against fedfr_fedavg_multi, their yardstick, in ONE process on one GPU.

At the iresnet100 parameter count (65 156 160 fp32) and k = 8 client states: fedfr_fedavg_multi, the distance-only pass and one weighted
step of fedfr_reweight_step (out of place and in place, each with the fedfr_reweight_weights launch behind it, as a round issues them), and
a whole round of R = 3 steps of each rule through server.ReweightedAggregator.aggregate (4 passes, 4 weights launches and the one blocking
copy).  The cases are INTERLEAVED: every repetition runs each case once between its own pair of HIP events, so a drift of the clock or of
a neighbour's load falls on all of them alike; median, min and max over --reps repetitions after --warmup, and the achieved GB/s against
the bytes the algorithm needs:

    fedavg_multi        (k + 1) n 4 B      k states read, the aggregate written
    distance-only pass  (k + 1) n 4 B      z and k states read (+ 8 k grid B of partials)
    weighted step       (k + 2) n 4 B      z and k states read, z' written
    round, R steps      (k + 1) n 4 B + R (k + 2) n 4 B

The states total (k + 3) n 4 B = 2.9 GB: far beyond the caches, every launch reads HBM.  No GPU: an error, not a fallback.
usage: python tools/reweight_bench.py [--n N] [--k K] [--iters 3] [--reps 20] [--warmup 3] [--limit 240]
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
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds after which the process gives up")
    a = ap.parse_args()
    if not 1 <= a.k <= 8:
        ap.error("--k must be 1..8 (fedfr_fedavg_multi, the yardstick, takes no more in one pass)")
    signal.signal(signal.SIGALRM, lambda *_: (sys.stderr.write("reweight_bench: time limit of %d s reached\n" % a.limit), os._exit(3)))
    signal.alarm(a.limit)

    import numpy as np
    import torch
    from fedfr_amd import _C, ops, server
    if not torch.cuda.is_available():
        sys.exit("reweight_bench: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    n, k, R = a.n, a.k, a.iters
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(n, generator=g, device=dev) - 0.5
    xs = [x + 0.01 * (i + 1) * (torch.rand(n, generator=g, device=dev) - 0.5) for i in range(k)]
    out, zin = torch.empty_like(x), x.clone()
    ptrs = (C.c_void_p * k)(*[t.data_ptr() for t in xs])
    wv = (C.c_float * k)(*[float(np.float32(1.0 / k))] * k)
    alpha = [1.0 / k] * k
    ws = torch.empty(ops.reweight_workspace_bytes(k, n) // 8, dtype=torch.float64, device=dev)
    grid = ws.numel() // k
    hd, hb, info = torch.zeros(2 * k, dtype=torch.float64, device=dev), torch.zeros(k, dtype=torch.float32, device=dev), torch.zeros(4, dtype=torch.float64, device=dev)
    st = _C.stream()
    aggs = {kind: server.ReweightedAggregator(kind, iters=R) for kind in ("GeoMedian", "CenteredClip")}

    def fedavg():
        _C.call("fedfr_fedavg_multi", out.data_ptr(), ptrs, wv, k, n, 0, st)

    def dist_only():
        ops.reweight_step(None, x, xs, None, ws)
        ops.reweight_weights("GeoMedian", alpha, 1e-6, 0, 1, k, n, ws, hd, hb, info)

    def step_to(dst, z):
        def run():      # hb holds the weights of the distance-only pass; an in-place centre keeps evolving: the work per launch does not depend on its values
            ops.reweight_step(dst, z, xs, hb, ws)
            ops.reweight_weights("GeoMedian", alpha, 1e-6, 1, 1, k, n, ws, hd, hb, info)
        return run

    def round_of(kind):
        return lambda: aggs[kind].aggregate(x, xs, alpha)

    one, part = n * 4, 8 * k * grid
    cases = [("fedavg_multi", fedavg, (k + 1) * one), ("reweight distance-only", dist_only, (k + 1) * one + part),
             ("reweight step", step_to(out, x), (k + 2) * one + part), ("reweight step in place", step_to(zin, zin), (k + 2) * one + part),
             ("GeoMedian round R=%d" % R, round_of("GeoMedian"), (k + 1) * one + R * (k + 2) * one),
             ("CenteredClip round R=%d" % R, round_of("CenteredClip"), (k + 1) * one + R * (k + 2) * one)]
    dist_only()                                # weights for the step launches
    for _ in range(a.warmup):
        for _, fn, _ in cases:
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in cases}
    for _ in range(a.reps):                    # interleaved: one repetition of every case after another
        ev = []
        for name, fn, _ in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            ev.append((name, e0, e1))
        torch.cuda.synchronize()
        for name, e0, e1 in ev:
            ms[name].append(e0.elapsed_time(e1))
    res = {}
    for name, _, nbytes in cases:
        v = sorted(ms[name])
        med = v[len(v) // 2]
        res[name] = {"bytes": nbytes, "ms_median": med, "ms_min": v[0], "ms_max": v[-1], "gbps_median": nbytes / med / 1e6}
        print("%-26s n=%d k=%d  %.3f ms median (min %.3f, max %.3f)  %.0f GB/s of %.1f MB" % (name, n, k, med, v[0], v[-1], nbytes / med / 1e6, nbytes / 1e6))
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(zin).all()) and all(np.all(np.isfinite(g_.last_dist)) for g_ in aggs.values())
    base = res["fedavg_multi"]["ms_median"]
    for name in res:
        res[name]["time_vs_fedavg_multi"] = res[name]["ms_median"] / base
    print(json.dumps({"n": n, "k": k, "iters": R, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "kernels": res}))
    signal.alarm(0)


if __name__ == "__main__":
    main()
