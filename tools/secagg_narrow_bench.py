#!/usr/bin/env python3
"""Time the narrow secure-aggregation kernels beside the 32-bit ones in ONE process on one GPU (numbers of different runs are never compared).

At the iresnet100 parameter count (65 156 160 fp32) and K = 8 participants (a client generates 7 pair masks + 1 self mask = 8 streams; the
server, with no dropout, removes the 8 self masks):

    mask32 k=S            fedfr_secagg_mask with S streams, S in 0, 8
    mask8 / mask16 k=S    fedfr_secagg_mask_narrow at 8 / 16 bits with S streams, S in 0, 8 (k=0: rotation, rounding and packing alone)
    aggregate32 / aggregate8 / aggregate16 ku=8 k=S   the aggregates over 8 uploads with S recovery streams, S in 0, 8 (first = last = 1, x added)
    rht_fill              the rotation alone (reads n floats, writes n_pad)

All rows are timed in interleaved rounds (row A, B, C, ..., A, B, C, ...), every launch between its own pair of HIP events after --warmup
rounds; each row is the median of --reps rounds (min and max reported too), with the GB/s against the bytes the ALGORITHM needs

    mask                  4 n 2 + n b / 8          x and x_i read, the words written
    aggregate             ku n b / 8 + 4 n 2       every upload and x read, out written

No GPU: an error.
usage: python tools/secagg_narrow_bench.py [--n N] [--reps 20] [--warmup 3] [--limit 240] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import signal
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IRESNET100_PARAMS = 65156160
K = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=IRESNET100_PARAMS)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds after which the process gives up")
    ap.add_argument("--out", default=None, help="also write the JSON result line to this file")
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: (sys.stderr.write("secagg_narrow_bench: time limit of %d s reached\n" % a.limit), os._exit(3)))
    signal.alarm(a.limit)

    import numpy as np
    import torch
    from fedfr_amd import _C
    if not torch.cuda.is_available():
        sys.exit("secagg_narrow_bench: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    n = a.n
    npad = int(_C.lib().fedfr_rht_padded_count(n))
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(n, generator=g, device=dev) - 0.5
    xi = x + 0.01 * (torch.rand(n, generator=g, device=dev) - 0.5)
    nw = max(n, npad * 16 // 32)                                   # words of the largest upload: n at 32 bits, n_pad / 2 at 16 (more than n for a small n)
    y = torch.empty(nw, dtype=torch.int32, device=dev)
    ys = [torch.randint(-2 ** 31, 2 ** 31 - 1, (nw,), generator=g, device=dev, dtype=torch.int32) for _ in range(8)]
    out = torch.empty(npad, device=dev)
    counters = torch.zeros(2, dtype=torch.int32, device=dev)
    st = _C.stream()
    rng = np.random.default_rng(1)
    keys = (C.c_uint * (8 * 32))(*[int(v) for v in rng.integers(0, 2 ** 32, 8 * 32)])
    nonces = (C.c_uint * (3 * 32))(*[int(v) for v in rng.integers(0, 2 ** 32, 3 * 32)])
    signs = (C.c_int * 32)(*[1 if s % 3 else -1 for s in range(32)])
    yptrs = (C.c_void_p * 8)(*[t.data_ptr() for t in ys])          # (a narrow upload is the front of the same buffer)
    frac = {32: 24, 16: 16, 8: 10}
    res = {}

    def coef(bits):
        return float(np.float32(1.0 / K) * np.float32(2.0 ** frac[bits]))

    def mask(bits, k):
        if bits == 32:
            _C.call("fedfr_secagg_mask", y.data_ptr(), x.data_ptr(), xi.data_ptr(), coef(32), (2 ** 31 - 1) // K, keys, nonces, signs, k, n,
                    counters.data_ptr(), st)
        else:
            _C.call("fedfr_secagg_mask_narrow", y.data_ptr(), x.data_ptr(), xi.data_ptr(), coef(bits), K, bits, 5, 7, 1, keys, nonces, signs, k, 0, n,
                    counters.data_ptr(), st)

    def aggregate(bits, k):
        if bits == 32:
            _C.call("fedfr_secagg_aggregate", out.data_ptr(), x.data_ptr(), None, yptrs, 8, keys, nonces, signs, k, frac[32], 1.0, n, 1, 1, st)
        else:
            _C.call("fedfr_secagg_aggregate_narrow", out.data_ptr(), x.data_ptr(), None, yptrs, 8, bits, 5, 1, keys, nonces, signs, k, 0, frac[bits], 1.0, n,
                    1, 1, st)

    def rht():
        _C.call("fedfr_rht_fill", out.data_ptr(), x.data_ptr(), n, 5, 1, 0, st)

    group = []
    for k in (0, K):
        for bits in (32, 16, 8):
            group.append(("mask%d k=%d" % (bits, k), (lambda bits=bits, k=k: mask(bits, k)), 8 * n + n * bits // 8, k))
    for k in (0, K):
        for bits in (32, 16, 8):
            group.append(("aggregate%d ku=8 k=%d" % (bits, k), (lambda bits=bits, k=k: aggregate(bits, k)), 8 * n * bits // 8 + 8 * n, k))
    group.append(("rht_fill", rht, 8 * n, 0))
    for _ in range(a.warmup):
        for _, fn, _, _ in group:
            fn()
    torch.cuda.synchronize()
    ev = {name: [] for name, _, _, _ in group}
    for _ in range(a.reps):
        for name, fn, _, _ in group:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            ev[name].append((e0, e1))
    torch.cuda.synchronize()
    for name, _, nbytes, k in group:
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev[name])
        med = ms[len(ms) // 2]
        res[name] = {"bytes": nbytes, "streams": k, "ms_median": med, "ms_min": ms[0], "ms_max": ms[-1], "gbps_median": nbytes / med / 1e6}
        print("%-24s %.3f ms median (min %.3f, max %.3f)  %5.0f GB/s of %.1f MB" % (name, med, ms[0], ms[-1], nbytes / med / 1e6, nbytes / 1e6))
    assert bool(torch.isfinite(out[:n]).all())
    line = json.dumps({"n": n, "participants": K, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "kernels": res})
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    signal.alarm(0)


if __name__ == "__main__":
    main()
