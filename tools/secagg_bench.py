#!/usr/bin/env python3
"""Time the secure-aggregation kernels in ONE process on one GPU (numbers of different runs are never compared).

At the iresnet100 parameter count (65 156 160 fp32):

    mask k=K          fedfr_secagg_mask with K streams, K in 0, 1, 3, 7, 31 (a client among 8 generates 7 pair masks + 1 self mask)
    aggregate ku=8 k=K   fedfr_secagg_aggregate over 8 uploads with K recovery streams, K in 0, 7 (first = last = 1, x added)
    delta_quantize    fedfr_delta_quantize (8 bits, no error feedback): the nearest sibling of mask k=0 (reads x and x_i, writes codes)
    chacha20_fill     the generator alone

All rows are timed in interleaved rounds (row A, B, C, ..., A, B, C, ...), every launch between its own pair of HIP events after --warmup
rounds; each row is the median of --reps rounds (min and max reported too), with the GB/s against the bytes the ALGORITHM needs

    mask              4 n (2 + 1)         x and x_i read, y written
    aggregate         4 n (ku + 2)        every upload and x read, out written
    delta_quantize    4 n 2 + n + n / 32  x and x_i read, one code byte per element and one scale byte per 32 written
    chacha20_fill     4 n

beside the copy rate the microarchitecture guide measured (6.29 TB/s), and the integer lane-operations per second against the VALU peak
(256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz = 78.6 T lane-ops/s) with the op count of one ChaCha20 block: 80 quarter rounds x 12 operations
+ 16 additions = 976 lane-operations for 16 words, 61 per word and stream (the encoding, the signed accumulation and the address
arithmetic are not counted).  No GPU: an error.
usage: python tools/secagg_bench.py [--n N] [--reps 20] [--warmup 3] [--limit 240] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import signal
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IRESNET100_PARAMS = 65156160
COPY_GBPS = 6290.0                     # the guide's measured copy rate
VALU_PEAK = 256 * 4 * 32 * 2.4e9       # lane-operations per second
OPS_PER_WORD = 976 / 16.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=IRESNET100_PARAMS)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds after which the process gives up")
    ap.add_argument("--out", default=None, help="also write the JSON result line to this file")
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: (sys.stderr.write("secagg_bench: time limit of %d s reached\n" % a.limit), os._exit(3)))
    signal.alarm(a.limit)

    import numpy as np
    import torch
    from fedfr_amd import _C
    if not torch.cuda.is_available():
        sys.exit("secagg_bench: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    n = a.n
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(n, generator=g, device=dev) - 0.5
    xi = x + 0.01 * (torch.rand(n, generator=g, device=dev) - 0.5)
    y = torch.empty(n, dtype=torch.int32, device=dev)
    ys = [torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, device=dev, dtype=torch.int32) for _ in range(8)]
    out = torch.empty(n, device=dev)
    codes = torch.empty(int(_C.lib().fedfr_delta_code_bytes(8, n)), dtype=torch.uint8, device=dev)
    scales = torch.empty(int(_C.lib().fedfr_delta_scale_bytes(n)), dtype=torch.uint8, device=dev)
    counters = torch.zeros(2, dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    st = _C.stream()
    rng = np.random.default_rng(1)
    keys = (C.c_uint * (8 * 32))(*[int(v) for v in rng.integers(0, 2 ** 32, 8 * 32)])
    nonces = (C.c_uint * (3 * 32))(*[int(v) for v in rng.integers(0, 2 ** 32, 3 * 32)])
    signs = (C.c_int * 32)(*[1 if s % 3 else -1 for s in range(32)])
    yptrs = (C.c_void_p * 8)(*[t.data_ptr() for t in ys])
    coef, limit = float(np.float32(0.125) * np.float32(2.0 ** 24)), (2 ** 31 - 1) // 8
    res = {}

    def mask(k):
        _C.call("fedfr_secagg_mask", y.data_ptr(), x.data_ptr(), xi.data_ptr(), coef, limit, keys, nonces, signs, k, n, counters.data_ptr(), st)

    def aggregate(k):
        _C.call("fedfr_secagg_aggregate", out.data_ptr(), x.data_ptr(), None, yptrs, 8, keys, nonces, signs, k, 24, 1.0, n, 1, 1, st)

    def quantize():
        _C.call("fedfr_delta_quantize", x.data_ptr(), xi.data_ptr(), None, codes.data_ptr(), scales.data_ptr(), 8, n, bad.data_ptr(), st)

    def fill():
        _C.call("fedfr_chacha20_fill", y.data_ptr(), n, keys, 0, nonces, st)

    group = [("mask k=%d" % k, (lambda k=k: mask(k)), 12 * n, k) for k in (0, 1, 3, 7, 31)]
    group += [("aggregate ku=8 k=%d" % k, (lambda k=k: aggregate(k)), 40 * n, k) for k in (0, 7)]
    group += [("delta_quantize 8 bit", quantize, 8 * n + n + n // 32, 0), ("chacha20_fill", fill, 4 * n, 1)]
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
        ops = OPS_PER_WORD * k * n
        res[name] = {"bytes": nbytes, "streams": k, "ms_median": med, "ms_min": ms[0], "ms_max": ms[-1], "gbps_median": nbytes / med / 1e6,
                     "share_of_copy_rate": nbytes / med / 1e6 / COPY_GBPS, "lane_ops": ops, "tera_lane_ops_per_s": ops / med / 1e9,
                     "share_of_valu_peak": ops / (med * 1e-3) / VALU_PEAK}
        print("%-22s %.3f ms median (min %.3f, max %.3f)  %5.0f GB/s of %.1f MB (%.2f of the copy rate)  %5.1f T lane-ops/s (%.2f of the VALU peak)"
              % (name, med, ms[0], ms[-1], nbytes / med / 1e6, nbytes / 1e6, res[name]["share_of_copy_rate"], res[name]["tera_lane_ops_per_s"],
                 res[name]["share_of_valu_peak"]))
    assert bool(torch.isfinite(out).all())
    line = json.dumps({"n": n, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "kernels": res})
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    signal.alarm(0)


if __name__ == "__main__":
    main()
