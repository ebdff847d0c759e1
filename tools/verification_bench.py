#!/usr/bin/env python3
"""k-fold 1:1 verification at the lfw / agedb_30 size (P = 6000 pairs, D = 512, 10 folds): the fused kernel alone, kernel + host
read-out (``evaluate``'s numbers from the count tables), the reference's own formulation restated in numpy in the same process (the
per-threshold calculate_accuracy / calculate_val_far loops of calculate_roc and calculate_val on host embeddings, FAR pick by
``pick_far_threshold``), and ``eval_verification.test`` end to end for iresnet100 on 12 000 synthetic uint8 images resident on the GPU.
Prints one JSON line and writes it to --out.
usage: python tools/verification_bench.py [--pairs 6000] [--dim 512] [--reps 20] [--network iresnet100] [--batch 128] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from fedfr_amd import backbones, eval_verification as V  # noqa: E402
from verification_pairs import synthetic_pairs  # noqa: E402  (tools/)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "reps": reps}


def kernel_events(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "reps": reps}


def reference_formulation(emb, issame, nfolds):
    """evaluate() as the reference computes it: one calculate_accuracy / calculate_val_far call per fold and threshold."""
    issame = np.asarray(issame)
    e1, e2 = emb[0::2], emb[1::2]
    dist = np.sum(np.square(np.subtract(e1, e2)), 1)
    accuracy = np.zeros(nfolds)
    val, far = np.zeros(nfolds), np.zeros(nfolds)
    thr_a, thr_b = V.roc_thresholds(), V.val_thresholds()
    for f, (a, b) in enumerate(V.fold_ranges(len(dist), nfolds)):
        test = np.arange(a, b)
        train = np.concatenate([np.arange(0, a), np.arange(b, len(dist))]) if nfolds > 1 else test
        acc_train = np.array([V.calculate_accuracy(t, dist[train], issame[train])[2] for t in thr_a])
        for t in thr_a:
            V.calculate_accuracy(t, dist[test], issame[test])
        accuracy[f] = V.calculate_accuracy(thr_a[np.argmax(acc_train)], dist[test], issame[test])[2]
        far_train = np.array([V.calculate_val_far(t, dist[train], issame[train])[1] for t in thr_b])
        val[f], far[f] = V.calculate_val_far(V.pick_far_threshold(far_train, thr_b, V.FAR_TARGET), dist[test], issame[test])
    return accuracy, np.mean(val), np.std(val), np.mean(far)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=6000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--folds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--network", default="iresnet100")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "verification_bench_v1.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    P, D = a.pairs, a.dim
    emb0, emb1, issame = synthetic_pairs(P, D, 0, "blocks")
    g0, g1 = torch.from_numpy(emb0).to(dev), torch.from_numpy(emb1).to(dev)
    same = torch.from_numpy(issame).to(dev)
    out = {"device": torch.cuda.get_device_name(0), "pairs": P, "dim": D, "folds": a.folds}

    res = V.fold_counts(g0, g1, same, a.folds)
    tables = V._evaluate_counts(res, issame)
    out["kernel"] = kernel_events(lambda: V.fold_counts(g0, g1, same, a.folds), 3, a.reps)
    out["kernel_and_readout"] = timed(lambda: V._evaluate_counts(V.fold_counts(g0, g1, same, a.folds), issame), 2, a.reps)

    def host_path():
        e = g0.cpu().numpy().astype(np.float64) + g1.cpu().numpy().astype(np.float64)       # the embeddings leave the GPU first
        n = np.sqrt(np.sum(e * e, 1, keepdims=True))
        return reference_formulation(e / np.where(n == 0, 1, n), issame, a.folds)
    t = time.perf_counter()
    ref = host_path()
    out["reference_formulation_numpy"] = {"ms": (time.perf_counter() - t) * 1e3, "reps": 1}
    out["accuracy_equal"] = bool(np.array_equal(ref[0], tables[2]))
    out["accuracy_mean"] = float(np.mean(tables[2]))

    rng = np.random.default_rng(0)
    data = torch.from_numpy(rng.integers(0, 256, (2 * P, 112, 112, 3), dtype=np.uint8)).to(dev)
    m = getattr(backbones, a.network)(False, dropout=0, fp16=True).to(dev).eval()
    V.test((data, list(issame)), m, a.batch, a.folds)                   # warm-up: arenas, weight shadows
    r = timed(lambda: V.test((data, list(issame)), m, a.batch, a.folds), 0, 2)
    r.update({"network": a.network, "images": 2 * P, "batch": a.batch, "forward_passes": 2})
    out["test_end_to_end"] = r
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
