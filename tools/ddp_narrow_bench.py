#!/usr/bin/env python3
"""Time the distributed-DP client pass at 16-bit narrow words beside the passes it is made of, in ONE process on one GPU (numbers of
different runs are never compared).

At the iresnet100 parameter count (65 156 160 fp32) for a client among K = T = 8 (7 pair masks + 1 self mask = 8 streams), z = 1, C = 1,
f = 12, kappa = 7 (privacy.DistributedDiscreteGaussian(bits=16, wrap_sigmas=7): sigma_int = 1448.15, code_limit = 511):

    mask_narrow_dp16 k=8   fedfr_secagg_mask_narrow_dp: clip factor from the device, rotation, stochastic rounding, sum of squares, discrete
                           Gaussian noise on all n_pad coordinates mod 2^16, packing, masks
    mask_dp32 k=8          fedfr_secagg_mask_dp at the same sigma: the 32-bit pass with the sampler
    mask_narrow16 k=8      fedfr_secagg_mask_narrow at 16 bits: the narrow pass without the sampler
    mask32 k=8             fedfr_secagg_mask: the 32-bit pass without the sampler
    aggregate16 ku=8 k=8   fedfr_secagg_aggregate_narrow over 8 uploads and the 8 self masks: the server's side, unchanged by the feature

THE EXPECTATION.  The new pass should cost no more than mask_narrow16 + (mask_dp32 - mask32): the narrow pass plus the sampler's share,
three kernels the feature does not touch, measured in this run; "within" allows 15 % over that sum for run-to-run spread and for overlap
between the sampler and the memory streams that the rotation's barriers may lose.  It is reported (``expected_ms``, ``ratio``,
``within_15_percent``), not asserted.

All rows are timed in interleaved rounds (row A, B, C, ..., A, B, C, ...), every launch between its own pair of HIP events after --warmup
rounds; each row reports the median of --reps launches with mean, standard deviation, minimum and maximum, and the GB/s against the bytes
the ALGORITHM needs (x and x_i read, the words written; every upload and x read, out written).  No GPU: an error.
usage: python tools/ddp_narrow_bench.py [--n N] [--reps 20] [--warmup 3] [--limit 240] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import signal
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IRESNET100_PARAMS = 65156160
K, FRAC, KAPPA = 8, 12, 7.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=IRESNET100_PARAMS)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds after which the process gives up")
    ap.add_argument("--out", default=None, help="also write the JSON result line to this file")
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: (sys.stderr.write("ddp_narrow_bench: time limit of %d s reached\n" % a.limit), os._exit(3)))
    signal.alarm(a.limit)

    import numpy as np
    import torch
    from fedfr_amd import _C
    from fedfr_amd.privacy import DistributedDiscreteGaussian
    from fedfr_amd.server import ServerOptimizer
    if not torch.cuda.is_available():
        sys.exit("ddp_narrow_bench: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    n = a.n
    mech = DistributedDiscreteGaussian(1.0, 1.0, FRAC, K, K, n, bits=16, wrap_sigmas=KAPPA)
    npad, sigma = mech.n_pad, mech.sigma_int
    limit32 = (2 ** 31 - 1) // K - 37 * (int(sigma) + 1)
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(n, generator=g, device=dev) - 0.5
    xi = x + 0.01 * (torch.rand(n, generator=g, device=dev) - 0.5)
    nw = max(n, npad // 2)
    y = torch.empty(nw, dtype=torch.int32, device=dev)
    ys = [torch.randint(-2 ** 31, 2 ** 31 - 1, (npad // 2,), generator=g, device=dev, dtype=torch.int32) for _ in range(8)]
    out = torch.empty(npad, device=dev)
    counters = torch.zeros(3, dtype=torch.int32, device=dev)
    sqnorm = torch.zeros(1, dtype=torch.int64, device=dev)
    st = _C.stream()
    rng = np.random.default_rng(1)
    keys = (C.c_uint * (8 * 32))(*[int(v) for v in rng.integers(0, 2 ** 32, 8 * 32)])
    nonces = (C.c_uint * (3 * 32))(*[int(v) for v in rng.integers(0, 2 ** 32, 3 * 32)])
    signs = (C.c_int * 32)(*[1 if s % 3 else -1 for s in range(32)])
    yptrs = (C.c_void_p * 8)(*[t.data_ptr() for t in ys])
    factor = ServerOptimizer("AVGM", clip_norm=mech.clip_norm).coefficients(x, [xi], [1.0])
    coef = float(np.float32(factor.item()) * np.float32(2.0 ** FRAC))      # what the passes without the clip encode with: the same codes

    def narrow_dp():
        _C.call("fedfr_secagg_mask_narrow_dp", y.data_ptr(), x.data_ptr(), xi.data_ptr(), factor.data_ptr(), FRAC, mech.code_limit, 16, 5, 7, 1, 12345, 1, 0,
                sigma, keys, nonces, signs, K, 0, n, counters.data_ptr(), sqnorm.data_ptr(), st)

    def mask_dp32():
        _C.call("fedfr_secagg_mask_dp", y.data_ptr(), x.data_ptr(), xi.data_ptr(), factor.data_ptr(), FRAC, limit32, 12345, 1, 0, sigma, keys, nonces, signs, K, n,
                counters.data_ptr(), sqnorm.data_ptr(), st)

    def narrow16():
        _C.call("fedfr_secagg_mask_narrow", y.data_ptr(), x.data_ptr(), xi.data_ptr(), coef, K, 16, 5, 7, 1, keys, nonces, signs, K, 0, n, counters.data_ptr(), st)

    def mask32():
        _C.call("fedfr_secagg_mask", y.data_ptr(), x.data_ptr(), xi.data_ptr(), coef, limit32, keys, nonces, signs, K, n, counters.data_ptr(), st)

    def aggregate16():
        _C.call("fedfr_secagg_aggregate_narrow", out.data_ptr(), x.data_ptr(), None, yptrs, 8, 16, 5, 1, keys, nonces, signs, K, 0, FRAC, 0.125, n, 1, 1, st)

    group = [("mask_narrow_dp16 k=8", narrow_dp, 8 * n + 2 * npad), ("mask_dp32 k=8", mask_dp32, 12 * n), ("mask_narrow16 k=8", narrow16, 8 * n + 2 * npad),
             ("mask32 k=8", mask32, 12 * n), ("aggregate16 ku=8 k=8", aggregate16, 8 * 2 * npad + 8 * n)]
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
    for name, _, nbytes in group:
        ms = np.sort(np.array([e0.elapsed_time(e1) for e0, e1 in ev[name]]))
        med = float(ms[ms.size // 2])
        res[name] = {"bytes": nbytes, "ms_median": med, "ms_mean": float(ms.mean()), "ms_std": float(ms.std(ddof=1)) if ms.size > 1 else 0.0,
                     "ms_min": float(ms[0]), "ms_max": float(ms[-1]), "gbps_median": nbytes / med / 1e6}
        print("%-22s %.3f ms median (mean %.3f, std %.3f, min %.3f, max %.3f)  %5.0f GB/s of %.1f MB"
              % (name, med, ms.mean(), res[name]["ms_std"], ms[0], ms[-1], nbytes / med / 1e6, nbytes / 1e6))
    exhausted = int(counters[2].item())
    assert exhausted == 0, "the sampler exhausted its attempts on %d elements" % exhausted
    assert bool(torch.isfinite(out[:n]).all())
    m = {k: v["ms_median"] for k, v in res.items()}
    expected = m["mask_narrow16 k=8"] + (m["mask_dp32 k=8"] - m["mask32 k=8"])
    ratio = m["mask_narrow_dp16 k=8"] / expected
    print("expected mask_narrow16 + (mask_dp32 - mask32) = %.3f ms; mask_narrow_dp16 / expected = %.3f (%s 15 %%); %.1f G noise values/s"
          % (expected, ratio, "within" if ratio <= 1.15 else "NOT within", npad / m["mask_narrow_dp16 k=8"] / 1e6))
    line = json.dumps({"n": n, "n_pad": npad, "participants": K, "frac_bits": FRAC, "wrap_sigmas": KAPPA, "sigma_int": sigma, "code_limit": mech.code_limit,
                       "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "kernels": res, "expected_ms": expected, "ratio": ratio,
                       "within_15_percent": bool(ratio <= 1.15)})
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    signal.alarm(0)


if __name__ == "__main__":
    main()
