#!/usr/bin/env python3
"""Time the top-k upload kernels against their yardsticks in ONE process on one GPU (numbers of different runs are never compared).

At the iresnet100 parameter count (65 156 160 fp32), k = 8 clients, each row the median of --reps launches timed with HIP events after
--warmup (every launch its own event pair; min and max reported too), and the achieved GB/s against the bytes the ALGORITHM needs:

    sparsify        n (16 + 4 P) + 8 keep B      x, x_i and e read and v written by the first pass; P = 4 later passes read v (two digit
                                                 histograms, the count pass, the emit pass); keep (index, value) pairs written
    sparse aggregate  8 n + 8 sum keep B         x read, the aggregate written, every entry counted once (the kernel loads 256 entries per
                                                 upload and tile and keeps the in-tile ones: the re-reads are not counted)
    quantize 8 bits, aggregate 8 bits k=8, fedavg_multi k=8: as tools/compress_bench.py counts them

Rows: sparsify at ratio 0.01 and 0.001 on sine-like deltas (uniform noise scaled by a slowly varying envelope, a few octaves wide) and at
0.01 on a single-exponent input (every |v| in one octave: the top-digit histogram then has 8 hot bins); sparse aggregate of 8 uploads at
ratio 0.01 and 0.001.  ``vs_<yardstick>`` = the row's GB/s over the yardstick's GB/s FROM THE SAME RUN; sparsify is compared with
``quantize 8 bits`` (``time_vs_quantize_at_equal_bytes``: its time over what its bytes would take at the quantiser's rate), the aggregate
with ``aggregate 8 bits k=8`` and ``fedavg_multi k=8``.  The sparsify launches rotate over the 8 client states, so every launch reads HBM.
No GPU: an error.
usage: python tools/sparse_bench.py [--n N] [--reps 20] [--warmup 3] [--limit 240] [--out FILE]
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
LATER_PASSES = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=IRESNET100_PARAMS)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds after which the process gives up")
    ap.add_argument("--out", default=None, help="also write the JSON result line to this file")
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: (sys.stderr.write("sparse_bench: time limit of %d s reached\n" % a.limit), os._exit(3)))
    signal.alarm(a.limit)

    import numpy as np
    import torch
    from fedfr_amd import _C, compress
    if not torch.cuda.is_available():
        sys.exit("sparse_bench: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    n = a.n
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(n, generator=g, device=dev) - 0.5
    env = 0.05 + torch.sin(torch.arange(n, device=dev, dtype=torch.float32) * 0.0113) ** 2
    xs = [x + 0.01 * (i + 1) * env * (torch.rand(n, generator=g, device=dev) - 0.5) for i in range(K)]
    del env
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
        print("%-28s %.3f ms median (min %.3f, max %.3f)  %.0f GB/s of %.1f MB" % (name, med, ms[0], ms[-1], nbytes / med / 1e6, nbytes / 1e6))

    # ---- the yardsticks
    ptrs = (C.c_void_p * K)(*[t.data_ptr() for t in xs])
    timed("fedavg_multi k=8", lambda: _C.call("fedfr_fedavg_multi", out.data_ptr(), ptrs, wv, K, n, 0, st), (K + 1) * n * 4)
    nc, ns = int(lib.fedfr_delta_code_bytes(8, n)), int(lib.fedfr_delta_scale_bytes(n))
    codes = [torch.empty(nc, dtype=torch.uint8, device=dev) for _ in range(K)]
    scales = [torch.empty(ns, dtype=torch.uint8, device=dev) for _ in range(K)]
    resid = [torch.zeros(n, device=dev) for _ in range(K)]
    bad = torch.zeros(1, dtype=torch.int32, device=dev)

    def quantize():
        i = turn[0] % K                                     # another client every launch: its state, residual and upload
        turn[0] += 1
        _C.call("fedfr_delta_quantize", x.data_ptr(), xs[i].data_ptr(), resid[i].data_ptr(), codes[i].data_ptr(), scales[i].data_ptr(), 8, n,
                bad.data_ptr(), st)

    for i in range(K):
        turn[0] = i
        quantize()
    timed("quantize 8 bits", quantize, n * 16 + nc + ns)
    cp = (C.c_void_p * K)(*[t.data_ptr() for t in codes])
    sp = (C.c_void_p * K)(*[t.data_ptr() for t in scales])
    timed("aggregate 8 bits k=8", lambda: _C.call("fedfr_delta_aggregate", out.data_ptr(), x.data_ptr(), cp, sp, wv, K, 8, n, 0, st), n * 8 + K * (nc + ns))
    assert int(bad.item()) == 0 and bool(torch.isfinite(out).all())
    del codes, scales

    # ---- sparsify
    ws = torch.empty(int(lib.fedfr_topk_workspace_bytes(n, 1)), dtype=torch.uint8, device=dev)
    ups = {}

    def sparsify_rows(tag, states, ratios):
        for ratio in ratios:
            keep = compress.keep_count(n, ratio)
            idx = [torch.empty(keep, dtype=torch.int32, device=dev) for _ in range(K)]
            val = [torch.empty(keep, device=dev) for _ in range(K)]
            for r in resid:
                r.zero_()

            def sparsify():
                i = turn[0] % K
                turn[0] += 1
                _C.call("fedfr_topk_sparsify", x.data_ptr(), states[i].data_ptr(), resid[i].data_ptr(), n, keep, idx[i].data_ptr(), val[i].data_ptr(),
                        bad.data_ptr(), ws.data_ptr(), st)

            for i in range(K):                              # every upload filled before the aggregate reads it
                turn[0] = i
                sparsify()
            name = "sparsify ratio %g%s" % (ratio, tag)
            timed(name, sparsify, n * (16 + 4 * LATER_PASSES) + 8 * keep)
            res[name]["keep"] = keep
            torch.cuda.synchronize()
            assert int(bad.item()) == 0
            for i in range(K):                              # a valid upload: strictly ascending indices below n
                assert bool((idx[i][1:] > idx[i][:-1]).all()) and 0 <= int(idx[i][0]) and int(idx[i][-1]) < n
            ups[name] = (keep, idx, val)

    sparsify_rows("", xs, (0.01, 0.001))
    one_exp = [x + (0.0078125 + 0.0078125 * torch.rand(n, generator=g, device=dev)) * (1.0 if i % 2 else -1.0) for i in range(K)]      # |x_i - x| in [2^-7, 2^-6)
    sparsify_rows(" one exponent", one_exp, (0.01,))
    del one_exp

    # ---- sparse aggregate
    for ratio in (0.01, 0.001):
        keep, idx, val = ups["sparsify ratio %g" % ratio]
        ip = (C.c_void_p * K)(*[t.data_ptr() for t in idx])
        vp = (C.c_void_p * K)(*[t.data_ptr() for t in val])
        keeps = (C.c_size_t * K)(*([keep] * K))
        name = "sparse aggregate ratio %g k=8" % ratio
        timed(name, lambda: _C.call("fedfr_sparse_aggregate", out.data_ptr(), x.data_ptr(), ip, vp, keeps, wv, K, n, 0, st), 8 * n + 8 * K * keep)
        res[name]["keep"] = keep
        assert bool(torch.isfinite(out).all())
        ref = x.clone()                                     # the same sum by index_add (another order of additions: compared loosely)
        for i in range(K):
            ref.index_add_(0, idx[i].long(), val[i] * float(wv[i]))
        res[name]["max_abs_diff_vs_index_add"] = float((out - ref).abs().max())
        assert res[name]["max_abs_diff_vs_index_add"] < 1e-6
        del ref

    for name, r in res.items():
        for y in ("fedavg_multi k=8", "quantize 8 bits", "aggregate 8 bits k=8"):
            r["vs_" + y.split(" k=")[0].replace(" ", "_")] = r["gbps_median"] / res[y]["gbps_median"]
        if name.startswith("sparsify"):
            r["time_vs_quantize_at_equal_bytes"] = r["ms_median"] / (r["bytes"] / res["quantize 8 bits"]["gbps_median"] / 1e6)
            r["time_vs_quantize"] = r["ms_median"] / res["quantize 8 bits"]["ms_median"]
        if name.startswith("sparse aggregate"):
            r["time_vs_aggregate_8_bits"] = r["ms_median"] / res["aggregate 8 bits k=8"]["ms_median"]
            r["time_vs_fedavg_multi"] = r["ms_median"] / res["fedavg_multi k=8"]["ms_median"]
    sine, hot = res["sparsify ratio 0.01"], res["sparsify ratio 0.01 one exponent"]
    print("sparsify: %.2f of the quantiser's byte rate; one exponent takes %.2f of the sine row's time"
          % (sine["vs_quantize_8_bits"], hot["ms_median"] / sine["ms_median"]))
    line = json.dumps({"n": n, "k": K, "reps": a.reps, "warmup": a.warmup, "later_passes": LATER_PASSES, "device": torch.cuda.get_device_name(0), "kernels": res})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    signal.alarm(0)


if __name__ == "__main__":
    main()
