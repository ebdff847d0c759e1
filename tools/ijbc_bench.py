#!/usr/bin/env python3
"""IJB-C job 1:1 (fedfr_amd.eval_ijbc) at the full IJB-C shape on one MI355X, synthetic data: 469 375 images x D = 512, 23 124
templates, 15 658 489 pairs (19 557 genuine).  Times each stage with device events (median of --reps) and the whole job:
template pooling (fedfr_template_pool: GB/s of the image features read), pair scores alone (GB/s of the two gathered fp64 rows per pair,
what the Infinity Cache serves), pair scores fused with the ROC counts, and ijbc_11 end to end (host CSR + read-out included).
Prints one JSON line.  usage: python tools/ijbc_bench.py [--reps N]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from fedfr_amd import eval_ijbc


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, D, T, P, NG = 469375, 512, 23124, 15658489, 19557
    rng = np.random.default_rng(0)
    templates = np.sort(rng.integers(0, T, N))
    templates[:T] = np.arange(T)
    templates = rng.permutation(templates) + 1
    medias = templates * 10 + rng.integers(0, 3, N)
    g = torch.Generator(device=dev).manual_seed(0)
    feats = torch.randn(N, D, device=dev, generator=g)
    face = torch.rand(N, device=dev, generator=g) * 0.5 + 0.5
    p1 = torch.randint(1, T + 1, (P,), device=dev, generator=g)
    p2 = torch.randint(1, T + 1, (P,), device=dev, generator=g)
    label = torch.zeros(P, dtype=torch.int64, device=dev)
    label[torch.randperm(P, device=dev, generator=g)[:NG]] = 1
    tf, uniq = eval_ijbc.template_pool(feats, templates, medias, faceness=face)
    r = {"N": N, "D": D, "T": T, "P": P}
    r["pool_ms"] = timed(lambda: eval_ijbc.template_pool(feats, templates, medias, faceness=face), a.reps)
    # pool_ms includes the host CSR build (a lexsort of the meta lists); the kernel alone: rocprofv3 --kernel-trace --stats
    r["pool_gbps_incl_host"] = N * D * 4 / r["pool_ms"] / 1e6
    r["scores_ms"] = timed(lambda: eval_ijbc.pair_scores(tf, uniq, p1, p2), a.reps)
    r["scores_gather_gbps"] = P * 2 * D * 8 / r["scores_ms"] / 1e6
    r["scores_roc_ms"] = timed(lambda: eval_ijbc.pair_scores(tf, uniq, p1, p2, label), a.reps)
    t0 = time.perf_counter()
    res = eval_ijbc.ijbc_11(feats, templates, medias, p1, p2, label, faceness=face)
    torch.cuda.synchronize()
    r["job_11_s"] = time.perf_counter() - t0
    r["tpr"] = res["table"]
    print(json.dumps(r))


if __name__ == "__main__":
    main()
