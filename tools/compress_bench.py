#!/usr/bin/env python3
"""Time the compressed-upload kernels against fedfr_fedavg_multi, their yardstick, in ONE process on one GPU.

At the iresnet100 parameter count (65 156 160 fp32), k = 8 clients, both code widths: fedfr_fedavg_multi over 8 fp32 states,
fedfr_delta_quantize (with the residual: the error-feedback form) and fedfr_delta_aggregate over 8 uploads with base = x, each timed
with HIP events over --reps launches after --warmup (every launch its own event pair; median, min and max reported), and the achieved
GB/s against the bytes the ALGORITHM needs:

    fedavg_multi    (k + 1) n 4 B                      k states read, the aggregate written
    quantize        n (16 + bits / 8 + 1 / 32) B       x, x_i and e read, e' written, codes and scale bytes written
    aggregate       n (8 + k (bits / 8 + 1 / 32)) B    x read, the aggregate written, k uploads read

All are one-pass streaming kernels, so fedavg_multi's GB/s FROM THE SAME RUN is the rate the others are compared with
(``vs_fedavg_multi``).  Two more figures: ``aggregate_time_vs_fedavg_multi`` (the time of aggregating 8 compressed uploads over the time
of fedavg_multi on 8 fp32 states, beside ``aggregate_bytes_vs_fedavg_multi``, the share of the bytes it moves: how much of the saved
traffic shows up as time) and ``quantize_vs_round`` (one quantise call over --round-ms, the time of one client's training round: default
the recorded 124 ms of 1 client x 8 local steps of iresnet100 at B = 128, profiles/r06_bench_r100_b128_v1.json).
Every launch moves more than the 256 MiB last-level cache holds (the smallest, the 4-bit aggregate: 0.8 GB) and the quantiser rotates
over the 8 client states, so every launch reads HBM.  No GPU: an error.
usage: python tools/compress_bench.py [--n N] [--reps 20] [--warmup 3] [--round-ms 124] [--limit 240] [--out FILE]
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
    ap.add_argument("--round-ms", type=float, default=124.0, help="one client's training round, for quantize_vs_round")
    ap.add_argument("--limit", type=int, default=240, help="seconds after which the process gives up")
    ap.add_argument("--out", default=None, help="also write the JSON result line to this file")
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: (sys.stderr.write("compress_bench: time limit of %d s reached\n" % a.limit), os._exit(3)))
    signal.alarm(a.limit)

    import numpy as np
    import torch
    from fedfr_amd import _C
    if not torch.cuda.is_available():
        sys.exit("compress_bench: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    n = a.n
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(n, generator=g, device=dev) - 0.5
    xs = [x + 0.01 * (i + 1) * (torch.rand(n, generator=g, device=dev) - 0.5) for i in range(K)]
    out = torch.empty(n, device=dev)
    lib = _C.lib()
    st = _C.stream()
    wv = (C.c_float * K)(*[float(np.float32(1.0 / K))] * K)
    res = {}
    turn = [0]

    def timed(name, fn, nbytes):
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
        print("%-22s %.3f ms median (min %.3f, max %.3f)  %.0f GB/s of %.1f MB" % (name, med, ms[0], ms[-1], nbytes / med / 1e6, nbytes / 1e6))

    ptrs = (C.c_void_p * K)(*[t.data_ptr() for t in xs])
    timed("fedavg_multi k=8", lambda: _C.call("fedfr_fedavg_multi", out.data_ptr(), ptrs, wv, K, n, 0, st), (K + 1) * n * 4)
    assert bool(torch.isfinite(out).all())
    for bits in (8, 4):
        nc, ns = int(lib.fedfr_delta_code_bytes(bits, n)), int(lib.fedfr_delta_scale_bytes(n))
        codes = [torch.empty(nc, dtype=torch.uint8, device=dev) for _ in range(K)]
        scales = [torch.empty(ns, dtype=torch.uint8, device=dev) for _ in range(K)]
        resid = [torch.zeros(n, device=dev) for _ in range(K)]
        bad = torch.zeros(1, dtype=torch.int32, device=dev)

        def quantize():
            i = turn[0] % K                                 # another client every launch: its state, residual and upload
            turn[0] += 1
            _C.call("fedfr_delta_quantize", x.data_ptr(), xs[i].data_ptr(), resid[i].data_ptr(), codes[i].data_ptr(), scales[i].data_ptr(), bits, n,
                    bad.data_ptr(), st)

        for i in range(K):                                  # every upload filled before the aggregate reads it
            turn[0] = i
            quantize()
        timed("quantize %d bits" % bits, quantize, n * 16 + nc + ns)
        cp = (C.c_void_p * K)(*[t.data_ptr() for t in codes])
        sp = (C.c_void_p * K)(*[t.data_ptr() for t in scales])
        timed("aggregate %d bits k=8" % bits, lambda: _C.call("fedfr_delta_aggregate", out.data_ptr(), x.data_ptr(), cp, sp, wv, K, bits, n, 0, st),
              n * 8 + K * (nc + ns))
        assert int(bad.item()) == 0 and bool(torch.isfinite(out).all())
        # the aggregate of the uploads is within sum w_i scale_i of the fp32 mean (every dq_i is within one scale of the delta it encodes)
        mean = sum(t.double() for t in xs) / K
        res["aggregate %d bits k=8" % bits]["max_abs_error_vs_fp32_mean"] = float((out.double() - mean).abs().max())
        del codes, scales, resid, mean
    base = res["fedavg_multi k=8"]
    for name, r in res.items():
        r["vs_fedavg_multi"] = r["gbps_median"] / base["gbps_median"]
    for bits in (8, 4):
        ag, qu = res["aggregate %d bits k=8" % bits], res["quantize %d bits" % bits]
        ag["aggregate_time_vs_fedavg_multi"] = ag["ms_median"] / base["ms_median"]
        ag["aggregate_bytes_vs_fedavg_multi"] = ag["bytes"] / base["bytes"]
        qu["quantize_vs_round"] = qu["ms_median"] / a.round_ms
        print("%d bits: aggregate takes %.2f of fedavg_multi's time for %.2f of its bytes; quantising one state is %.4f of a %.0f ms round"
              % (bits, ag["aggregate_time_vs_fedavg_multi"], ag["aggregate_bytes_vs_fedavg_multi"], qu["quantize_vs_round"], a.round_ms))
    line = json.dumps({"n": n, "k": K, "reps": a.reps, "warmup": a.warmup, "round_ms": a.round_ms, "device": torch.cuda.get_device_name(0), "kernels": res})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    signal.alarm(0)


if __name__ == "__main__":
    main()
