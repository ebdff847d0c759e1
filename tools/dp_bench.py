#!/usr/bin/env python3
"""Time the differential-privacy step against its alternatives in ONE process on one GPU (numbers of different runs are never compared).

At the iresnet100 parameter count (65 156 160 fp32), for k = 8 and k = 1 client states and the optimiser kinds AVGM and ADAM, three routes
to the same result x' = x + step(sum_i coef_i (x_i - x) + noise_std z) on the same buffers:

    fused       fedfr_dp_multi: the noise is drawn and added inside the pass that streams the client states
    parent      fedfr_fedopt_multi: the same pass WITHOUT noise (what the fused kernel would cost if the generator were free)
    unfused     fedfr_fedopt_multi into a Delta scratch buffer (first = 1, last = 0), fedfr_gaussian_fill(accumulate = 1) on it, then
                fedfr_fedopt_multi as ServerOptimizer.apply_delta calls it (first = 0, last = 1, the one "client" x itself): three launches

plus fedfr_dp_multi of the plain kind (DP-FedAvg proper: no parent counterpart) and fedfr_gaussian_fill alone.  The routes are timed in
interleaved rounds (route A, B, C, A, B, C, ...), every launch group between its own pair of HIP events after --warmup rounds; each row is
the median of --reps rounds (min and max reported too) and the GB/s against the bytes the ALGORITHM needs:

    fused / parent   4 n (k + 2 + 2 [m] + 2 [v])     every x_i, x read, x' written, m (and v) read and written
    unfused          the parent's bytes + 4 n (2 + 2 + 1)   Delta written, read and written by the fill, read by the last pass, x read again
    plain            4 n (k + 2)
    fill             4 n (accumulate: 8 n)

The fused and the unfused route are checked against each other first (same bits: the noise is the same stream).  No GPU: an error.
usage: python tools/dp_bench.py [--n N] [--reps 20] [--warmup 3] [--limit 240] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import signal
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IRESNET100_PARAMS = 65156160
KINDS = {"AVGM": 0, "ADAM": 2, "PLAIN": 4}
SEED, ROUND, SID = 0x0123456789ABCDEF, 3, 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=IRESNET100_PARAMS)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds after which the process gives up")
    ap.add_argument("--out", default=None, help="also write the JSON result line to this file")
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: (sys.stderr.write("dp_bench: time limit of %d s reached\n" % a.limit), os._exit(3)))
    signal.alarm(a.limit)

    import numpy as np
    import torch
    from fedfr_amd import _C
    if not torch.cuda.is_available():
        sys.exit("dp_bench: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    n = a.n
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(n, generator=g, device=dev) - 0.5
    xs = [x + 0.01 * (i + 1) * (torch.rand(n, generator=g, device=dev) - 0.5) for i in range(8)]
    out, out2, scratch = torch.empty(n, device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev)
    m, v = torch.zeros(n, device=dev), torch.full((n,), 1e-6, device=dev)
    coef = torch.full((8,), 0.125, device=dev)
    one = torch.ones(1, device=dev)
    st = _C.stream()
    f = np.float32
    hyper = [float(t) for t in (f(0.01), f(0.9), f(1) - f(0.9), f(0.99), f(1) - f(0.99), f(1e-3))]
    std = 0.003
    res = {}

    def ptrs(ts):
        return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])

    def fused(kind, k, dst=out):
        _C.call("fedfr_dp_multi", KINDS[kind], dst.data_ptr(), x.data_ptr(), ptrs(xs[:k]), coef.data_ptr(), k, n, m.data_ptr(), v.data_ptr(), None, 1, 1,
                *hyper, std, SEED, ROUND, SID, 0, st)

    def parent(kind, k):
        _C.call("fedfr_fedopt_multi", KINDS[kind], out.data_ptr(), x.data_ptr(), ptrs(xs[:k]), coef.data_ptr(), k, n, m.data_ptr(), v.data_ptr(), None, 1, 1,
                *hyper, st)

    def unfused(kind, k, dst=out):
        _C.call("fedfr_fedopt_multi", KINDS[kind], None, x.data_ptr(), ptrs(xs[:k]), coef.data_ptr(), k, n, None, None, scratch.data_ptr(), 1, 0, *hyper, st)
        _C.call("fedfr_gaussian_fill", scratch.data_ptr(), n, SEED, ROUND, SID, 0, std, 1, st)
        _C.call("fedfr_fedopt_multi", KINDS[kind], dst.data_ptr(), x.data_ptr(), ptrs([x]), one.data_ptr(), 1, n, m.data_ptr(), v.data_ptr(), scratch.data_ptr(),
                0, 1, *hyper, st)

    # ---- the two routes give the same bits (from equal moments)
    for kind in ("AVGM", "ADAM"):
        m.zero_(); v.fill_(1e-6)
        fused(kind, 8, out)
        m1 = m.clone()
        m.zero_(); v.fill_(1e-6)
        unfused(kind, 8, out2)
        torch.cuda.synchronize()
        assert torch.equal(out, out2) and torch.equal(m, m1), "fused and unfused routes differ (%s)" % kind
        del m1
    m.zero_(); v.fill_(1e-6)

    def timed(group):
        """group: [(name, fn, bytes)], timed in interleaved rounds"""
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
        for name, _, nbytes in group:
            ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev[name])
            med = ms[len(ms) // 2]
            res[name] = {"bytes": nbytes, "ms_median": med, "ms_min": ms[0], "ms_max": ms[-1], "gbps_median": nbytes / med / 1e6}
            print("%-28s %.3f ms median (min %.3f, max %.3f)  %.0f GB/s of %.1f MB" % (name, med, ms[0], ms[-1], nbytes / med / 1e6, nbytes / 1e6))

    for kind in ("AVGM", "ADAM"):
        mv = 2 if kind == "AVGM" else 4
        for k in (8, 1):
            base = 4 * n * (k + 2 + mv)
            tag = "%s k=%d" % (kind, k)
            timed([("fused " + tag, lambda kind=kind, k=k: fused(kind, k), base),
                   ("parent " + tag, lambda kind=kind, k=k: parent(kind, k), base),
                   ("unfused " + tag, lambda kind=kind, k=k: unfused(kind, k), base + 4 * n * 5)])
            r = res["fused " + tag]
            r["time_vs_parent"] = r["ms_median"] / res["parent " + tag]["ms_median"]
            r["time_vs_unfused"] = r["ms_median"] / res["unfused " + tag]["ms_median"]
            print("  fused %s: %.3f of the parent's time, %.3f of the unfused route's" % (tag, r["time_vs_parent"], r["time_vs_unfused"]))
    timed([("fused PLAIN k=8", lambda: fused("PLAIN", 8), 4 * n * 10), ("fused PLAIN k=1", lambda: fused("PLAIN", 1), 4 * n * 3),
           ("gaussian_fill", lambda: _C.call("fedfr_gaussian_fill", scratch.data_ptr(), n, SEED, ROUND, SID, 0, std, 0, st), 4 * n),
           ("gaussian_fill accumulate", lambda: _C.call("fedfr_gaussian_fill", scratch.data_ptr(), n, SEED, ROUND, SID, 0, std, 1, st), 8 * n)])
    assert bool(torch.isfinite(out).all())
    line = json.dumps({"n": n, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "kernels": res})
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    signal.alarm(0)


if __name__ == "__main__":
    main()
