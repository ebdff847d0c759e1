#!/usr/bin/env python3
"""Time the robust-aggregation kernels against fedfr_fedavg_multi, their yardstick, in ONE process on one GPU.

At the iresnet100 parameter count (65 156 160 fp32) and k = 4, 8, 10, 16 client states: fedfr_fedavg_multi (chained over groups of 8 for
k > 8, as FedPavg calls it), fedfr_robust_trimmed_mean at the median's trim and at b = floor(0.1 k), and fedfr_robust_pairdist, each timed
with HIP events over --reps launches after --warmup (every launch its own event pair; median and min reported), and the achieved GB/s
against the bytes the ALGORITHM needs:

    fedavg_multi    (k + 1) n 4 B                k states read, the aggregate written (k > 8: + the aggregate re-read and re-written per further group)
    trimmed_mean    (k + 1) n 4 B                k states read, the aggregate written
    pairdist        k n 4 B                      k states read once (+ the partials); the kernel's tiling READS `traffic multiple` x that for k > 8

All are one-pass streaming kernels, so fedavg_multi's GB/s FROM THE SAME RUN is the achievable rate the others are compared with:
``vs_fedavg_multi`` is algorithm bytes per second over fedavg_multi's; for the pair kernel ``vs_fedavg_multi_moved`` also counts the bytes
its tiling actually moves.  The states total up to 16 n 4 B = 4.2 GB: far beyond the caches, every launch reads HBM.  No GPU: an error.
usage: python tools/robust_bench.py [--n N] [--ks 4,8,10,16] [--reps 20] [--warmup 3] [--limit 240] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import signal
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IRESNET100_PARAMS = 65156160


def pair_reads(k):
    """client states read by fedfr_robust_pairdist's launches (k <= 13: one launch; else groups of 8: one diagonal launch per group of >= 2,
    one cross launch per pair of groups)"""
    if k <= 13:
        return k
    sizes = [min(8, k - g) for g in range(0, k, 8)]
    return sum(s for s in sizes if s >= 2) + sum(sizes[a] + sizes[b] for a in range(len(sizes)) for b in range(a + 1, len(sizes)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=IRESNET100_PARAMS)
    ap.add_argument("--ks", default="4,8,10,16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds after which the process gives up")
    ap.add_argument("--out", default=None, help="also write the JSON result line to this file")
    a = ap.parse_args()
    ks = [int(t) for t in a.ks.split(",")]
    if not all(2 <= k <= 32 for k in ks):
        ap.error("--ks must be 2..32")
    signal.signal(signal.SIGALRM, lambda *_: (sys.stderr.write("robust_bench: time limit of %d s reached\n" % a.limit), os._exit(3)))
    signal.alarm(a.limit)

    import numpy as np
    import torch
    from fedfr_amd import _C
    if not torch.cuda.is_available():
        sys.exit("robust_bench: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    n, kmax = a.n, max(ks)
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(n, generator=g, device=dev) - 0.5
    xs = [x + 0.01 * (i + 1) * (torch.rand(n, generator=g, device=dev) - 0.5) for i in range(kmax)]
    del x
    out = torch.empty(n, device=dev)
    lib = _C.lib()
    st = _C.stream()
    res = {}
    for k in ks:
        ptrs = (C.c_void_p * k)(*[t.data_ptr() for t in xs[:k]])
        slices = [xs[c:min(c + 8, k)] for c in range(0, k, 8)]
        groups = [((C.c_void_p * len(sl))(*[t.data_ptr() for t in sl]), len(sl)) for sl in slices]
        wv = (C.c_float * 8)(*[float(np.float32(1.0 / k))] * 8)
        ws = torch.empty(lib.fedfr_robust_pairdist_workspace_bytes(k, n) // 8, dtype=torch.float64, device=dev)
        dist = torch.empty(k * k, dtype=torch.float64, device=dev)

        def fedavg():
            for gi, (p, kk) in enumerate(groups):
                _C.call("fedfr_fedavg_multi", out.data_ptr(), p, wv, kk, n, 1 if gi else 0, st)

        def trimmed(b):
            def run():
                _C.call("fedfr_robust_trimmed_mean", out.data_ptr(), ptrs, k, b, n, st)
            return run

        def pairs():
            _C.call("fedfr_robust_pairdist", ptrs, k, n, dist.data_ptr(), ws.data_ptr(), ws.numel() * 8, st)

        mult = pair_reads(k) / k
        cases = [("fedavg_multi", fedavg, (k + 1 + 2 * (len(groups) - 1)) * n * 4, None),
                 ("trimmed_mean b=%d (median)" % ((k - 1) // 2), trimmed((k - 1) // 2), (k + 1) * n * 4, None),
                 ("trimmed_mean b=%d" % (k // 10), trimmed(k // 10), (k + 1) * n * 4, None),
                 ("pairdist", pairs, k * n * 4 + ws.numel() * 8, pair_reads(k) * n * 4 + ws.numel() * 8)]
        rk = {}
        for name, fn, nbytes, moved in cases:
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
            rk[name] = {"bytes": nbytes, "ms_median": med, "ms_min": ms[0], "ms_max": ms[-1], "gbps_median": nbytes / med / 1e6}
            if moved is not None:
                rk[name].update({"bytes_moved": moved, "traffic_multiple": mult, "gbps_moved_median": moved / med / 1e6})
            print("k=%-2d %-28s %.3f ms median (min %.3f, max %.3f)  %.0f GB/s of %.1f MB%s" % (
                k, name, med, ms[0], ms[-1], nbytes / med / 1e6, nbytes / 1e6,
                "" if moved is None else "  (moved: %.0f GB/s of %.1f MB, x%.2f)" % (moved / med / 1e6, moved / 1e6, mult)))
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dist).all())
        base = rk["fedavg_multi"]["gbps_median"]
        for name in rk:
            rk[name]["vs_fedavg_multi"] = rk[name]["gbps_median"] / base
            if "gbps_moved_median" in rk[name]:
                rk[name]["vs_fedavg_multi_moved"] = rk[name]["gbps_moved_median"] / base
        res[str(k)] = rk
        del ws, dist
    line = json.dumps({"n": n, "ks": ks, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "kernels": res})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    signal.alarm(0)


if __name__ == "__main__":
    main()
