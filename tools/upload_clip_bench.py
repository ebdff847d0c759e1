#!/usr/bin/env python3
"""Time the clip and the Gaussian mechanism on compressed and top-k uploads against their yardsticks, in ONE process on one GPU.

At the iresnet100 parameter count (65 156 160), k = 8 uploads, HIP events around every launch, mean and standard deviation over --reps
launches after --warmup:

    the norm passes      fedfr_delta_sqnorm (8 and 4 bits) and fedfr_sparse_sqnorm (--ratio of the parameters kept)
                         next to fedfr_fedopt_sqnorm k=8, the clip of fp32 states               bytes: k (n bits / 8 + n / 32) | k keep 8 | (k + 1) n 4
    noise off            fedfr_delta_aggregate_dp / fedfr_sparse_aggregate_dp with noise_std = 0
                         next to fedfr_delta_aggregate / fedfr_sparse_aggregate (same uploads, base = x)      expected: the same time within the spread
    noise on             the same with noise_std > 0, minus noise off: what drawing n Gaussians inside the pass costs,
                         next to fedfr_dp_multi (noise on) minus fedfr_fedopt_multi, the same difference on fp32 states (kind AVGM, k = 8)

Every launch takes the NEXT of several sets of 8 uploads (as many sets as it takes to hold 600 MB, at least two), so no launch finds its
uploads in the 256 MiB last-level cache: every launch reads HBM.  ``ms_mean`` / ``ms_std`` per kernel, ``gbps`` against the bytes the
ALGORITHM needs, and the comparisons as ratios and differences with the spread beside them.  No GPU: an error.
usage: python tools/upload_clip_bench.py [--n N] [--ratio 0.01] [--reps 20] [--warmup 3] [--limit 300] [--out FILE]
"""
import argparse
import ctypes as C
import json
import math
import os
import signal
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IRESNET100_PARAMS = 65156160
K = 8
ROTATE_BYTES = 600e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=IRESNET100_PARAMS)
    ap.add_argument("--ratio", type=float, default=0.01, help="share of the parameters a top-k upload keeps")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds after which the process gives up")
    ap.add_argument("--out", default=None, help="also write the JSON result line to this file")
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: (sys.stderr.write("upload_clip_bench: time limit of %d s reached\n" % a.limit), os._exit(3)))
    signal.alarm(a.limit)

    import numpy as np
    import torch
    from fedfr_amd import _C
    if not torch.cuda.is_available():
        sys.exit("upload_clip_bench: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    n = a.n
    lib, st = _C.lib(), _C.stream()
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(n, generator=g, device=dev) - 0.5
    out = torch.empty(n, device=dev)
    wv = (C.c_float * K)(*[float(np.float32(1.0 / K))] * K)
    sq = torch.empty(K, dtype=torch.float64, device=dev)
    coef = torch.full((K,), 1.0 / K, dtype=torch.float32, device=dev)
    viol = torch.zeros(K, dtype=torch.int32, device=dev)
    res = {}

    def vp(ts):
        return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])

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
        ms = [e0.elapsed_time(e1) for e0, e1 in ev]
        mean = sum(ms) / len(ms)
        std = math.sqrt(sum((t - mean) ** 2 for t in ms) / max(len(ms) - 1, 1))
        res[name] = {"bytes": nbytes, "ms_mean": mean, "ms_std": std, "ms_min": min(ms), "ms_max": max(ms), "gbps": nbytes / mean / 1e6}
        print("%-34s %8.3f ms +- %.3f (min %.3f, max %.3f)  %6.0f GB/s of %.1f MB" % (name, mean, std, min(ms), max(ms), nbytes / mean / 1e6, nbytes / 1e6))

    def rotating(sets):
        turn = [0]

        def nxt():
            turn[0] += 1
            return sets[turn[0] % len(sets)]
        return nxt

    # ---- fp32 states: the yardsticks ------------------------------------------------------------------------------------------------------
    xs = [x + 0.01 * (i + 1) * (torch.rand(n, generator=g, device=dev) - 0.5) for i in range(K)]
    ptrs = vp(xs)
    wsp_bytes = max(int(lib.fedfr_fedopt_sqnorm_workspace_bytes(K, n)), int(lib.fedfr_upload_sqnorm_workspace_bytes(K, n)))
    wsp = torch.empty(wsp_bytes // 8, dtype=torch.float64, device=dev)
    timed("fedopt_sqnorm k=8", lambda: _C.call("fedfr_fedopt_sqnorm", x.data_ptr(), ptrs, wv, K, n, 1.0, sq.data_ptr(), coef.data_ptr(), wsp.data_ptr(),
                                               wsp_bytes, st), (K + 1) * n * 4)
    coef.fill_(1.0 / K)
    m = torch.zeros(n, device=dev)
    hyper = (1.0, 0.9, float(np.float32(1) - np.float32(0.9)), 0.99, float(np.float32(1) - np.float32(0.99)), 1e-3)
    noise = (0.01, 1234, 5, 0, 0)
    timed("fedopt_multi AVGM k=8", lambda: _C.call("fedfr_fedopt_multi", 0, out.data_ptr(), x.data_ptr(), ptrs, coef.data_ptr(), K, n, m.data_ptr(), None, None,
                                                   1, 1, *hyper, st), (K + 3) * n * 4)
    timed("dp_multi AVGM k=8 noise on", lambda: _C.call("fedfr_dp_multi", 0, out.data_ptr(), x.data_ptr(), ptrs, coef.data_ptr(), K, n, m.data_ptr(), None, None,
                                                        1, 1, *hyper, *noise, st), (K + 3) * n * 4)
    del m

    # ---- compressed uploads ---------------------------------------------------------------------------------------------------------------
    for bits in (8, 4):
        nc, ns = int(lib.fedfr_delta_code_bytes(bits, n)), int(lib.fedfr_delta_scale_bytes(n))
        nsets = max(2, int(math.ceil(ROTATE_BYTES / (K * (nc + ns)))))
        sets = []
        for s in range(nsets):
            codes = [torch.empty(nc, dtype=torch.uint8, device=dev) for _ in range(K)]
            scales = [torch.empty(ns, dtype=torch.uint8, device=dev) for _ in range(K)]
            for i in range(K):
                _C.call("fedfr_delta_quantize", x.data_ptr(), xs[(i + s) % K].data_ptr(), None, codes[i].data_ptr(), scales[i].data_ptr(), bits, n, None, st)
            sets.append((vp(codes), vp(scales), codes, scales))
        nxt = rotating(sets)
        up = K * (nc + ns)

        def norm():
            cp, sp = nxt()[:2]
            _C.call("fedfr_delta_sqnorm", cp, sp, wv, K, bits, n, 1.0, sq.data_ptr(), coef.data_ptr(), wsp.data_ptr(), wsp_bytes, st)

        def agg():
            cp, sp = nxt()[:2]
            _C.call("fedfr_delta_aggregate", out.data_ptr(), x.data_ptr(), cp, sp, wv, K, bits, n, 0, st)

        def agg_dp(std):
            cp, sp = nxt()[:2]
            _C.call("fedfr_delta_aggregate_dp", out.data_ptr(), x.data_ptr(), cp, sp, coef.data_ptr(), K, bits, n, 0, 1, std, *noise[1:], st)

        timed("delta_sqnorm %d bits k=8" % bits, norm, up)
        assert bool(torch.isfinite(sq).all()) and bool((coef <= 1.0 / K).all())
        timed("delta_aggregate %d bits k=8" % bits, agg, n * 8 + up)
        timed("delta_aggregate_dp %d bits noise off" % bits, lambda: agg_dp(0.0), n * 8 + up)
        timed("delta_aggregate_dp %d bits noise on" % bits, lambda: agg_dp(noise[0]), n * 8 + up)
        assert bool(torch.isfinite(out).all())
        del sets, nxt
    del xs, ptrs

    # ---- top-k uploads --------------------------------------------------------------------------------------------------------------------
    keep = min(n, max(1, int(math.ceil(a.ratio * n))))
    stride = n // keep
    nsets = max(2, int(math.ceil(ROTATE_BYTES / (K * keep * 8))))
    sets = []
    for s in range(nsets):
        idx = [(torch.arange(keep, device=dev, dtype=torch.int64) * stride + torch.randint(0, stride, (keep,), generator=g, device=dev)).to(torch.int32)
               for _ in range(K)]
        val = [0.02 * (torch.rand(keep, generator=g, device=dev) - 0.5) for _ in range(K)]
        sets.append((vp(idx), vp(val), idx, val))
    nxt = rotating(sets)
    keeps = (C.c_size_t * K)(*([keep] * K))
    up = K * keep * 8

    def snorm():
        ip, vl = nxt()[:2]
        _C.call("fedfr_sparse_sqnorm", ip, vl, keeps, wv, K, n, 1.0, sq.data_ptr(), coef.data_ptr(), viol.data_ptr(), wsp.data_ptr(), wsp_bytes, st)

    def sagg():
        ip, vl = nxt()[:2]
        _C.call("fedfr_sparse_aggregate", out.data_ptr(), x.data_ptr(), ip, vl, keeps, wv, K, n, 0, st)

    def sagg_dp(std):
        ip, vl = nxt()[:2]
        _C.call("fedfr_sparse_aggregate_dp", out.data_ptr(), x.data_ptr(), ip, vl, keeps, coef.data_ptr(), K, n, 0, 1, std, *noise[1:], st)

    timed("sparse_sqnorm k=8", snorm, up)
    assert int(viol.abs().sum()) == 0 and bool(torch.isfinite(sq).all())
    timed("sparse_aggregate k=8", sagg, n * 8 + up)
    timed("sparse_aggregate_dp noise off", lambda: sagg_dp(0.0), n * 8 + up)
    timed("sparse_aggregate_dp noise on", lambda: sagg_dp(noise[0]), n * 8 + up)
    assert bool(torch.isfinite(out).all())

    # ---- the comparisons ------------------------------------------------------------------------------------------------------------------
    def spread(*names):
        return math.sqrt(sum(res[k]["ms_std"] ** 2 for k in names))

    cmp_ = {}
    ref = res["fedopt_sqnorm k=8"]
    for name in ("delta_sqnorm 8 bits k=8", "delta_sqnorm 4 bits k=8", "sparse_sqnorm k=8"):
        cmp_[name + " vs fedopt_sqnorm"] = {"time": res[name]["ms_mean"] / ref["ms_mean"], "bytes": res[name]["bytes"] / ref["bytes"],
                                            "bytes_per_upload": res[name]["bytes"] / K / (n * 4.0)}
    fp32_noise = res["dp_multi AVGM k=8 noise on"]["ms_mean"] - res["fedopt_multi AVGM k=8"]["ms_mean"]
    cmp_["noise on fp32 states (dp_multi - fedopt_multi)"] = {"ms": fp32_noise, "spread_ms": spread("dp_multi AVGM k=8 noise on", "fedopt_multi AVGM k=8")}
    for fam, old in (("delta_aggregate_dp 8 bits", "delta_aggregate 8 bits k=8"), ("delta_aggregate_dp 4 bits", "delta_aggregate 4 bits k=8"),
                     ("sparse_aggregate_dp", "sparse_aggregate k=8")):
        off, on = fam + " noise off", fam + " noise on"
        cmp_[off + " - " + old] = {"ms": res[off]["ms_mean"] - res[old]["ms_mean"], "spread_ms": spread(off, old)}
        cmp_[on + " - noise off"] = {"ms": res[on]["ms_mean"] - res[off]["ms_mean"], "spread_ms": spread(on, off)}
    for name, r in cmp_.items():
        print("%-66s %s" % (name, "  ".join("%s %.4g" % kv for kv in r.items())))
    line = json.dumps({"n": n, "k": K, "keep": keep, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "kernels": res,
                       "comparisons": cmp_})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    signal.alarm(0)


if __name__ == "__main__":
    main()
