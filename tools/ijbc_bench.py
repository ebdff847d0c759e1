#!/usr/bin/env python3
"""IJB-C job 1:1 (fedfr_amd.eval_ijbc) at the full IJB-C shape on one MI355X, synthetic data: 469 375 images x D = 512, 23 124
templates, 15 658 489 pairs (19 557 genuine).  Times each stage with device events (median of --reps) and the whole job:
template pooling (fedfr_template_pool: GB/s of the image features read), pair scores alone (GB/s of the two gathered fp64 rows per pair,
what the Infinity Cache serves), pair scores fused with the ROC counts, and ijbc_11 end to end (host CSR + read-out included).
Job 1:N at the IJB-C shape (19 593 probes x 3 531 gallery templates x D = 512, K = 1 960): fedfr_ident_rank_topk (useful fp64 TF/s =
2 Q G D / t; the kernel computes the products twice, once per sweep), fedfr_ident_topk on the same features rounded to fp32 (one segment,
K = 1 024) as the same-box baseline, with --host the numpy restatement of the reference's evaluation on the host (np.partition in place of
heapq.nlargest), and ijbc_1n end to end (host CSR, gen_mask and read-out included).
Prints one JSON line.  usage: python tools/ijbc_bench.py [--reps N] [--job 1:1|1:n|both] [--host]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from fedfr_amd import eval_1n, eval_ijbc


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


def host_evaluation(query, gallery, mask, fars=(0.01, 0.1)):
    """ijbc_all.py:367-427 in numpy on the host: np.dot, a full argsort for the ranks, the thresholds by np.partition."""
    Q = query.shape[0]
    sim = np.dot(query, gallery.T)
    top = np.argsort(-sim)[:, :10]
    rank = {"top%d" % k: float(np.mean(np.any(top[:, :k] == mask[:, None], axis=1))) for k in (1, 5, 10)}
    pos = sim[np.arange(Q), mask]
    sim[np.arange(Q), mask] = -2.0
    K = int(np.ceil(Q * max(fars)))
    neg = -np.sort(np.partition(-sim.ravel(), K - 1)[:K])
    return rank, {f: float(np.sum(pos > neg[int(np.ceil(Q * f)) - 1]) / Q) for f in fars}


def job_1n(a, dev):
    Q, G, D, K = 19593, 3531, 512, 1960
    g = torch.Generator(device=dev).manual_seed(1)
    centers = torch.nn.functional.normalize(torch.randn(G, D, device=dev, generator=g, dtype=torch.float64))
    mask = torch.randint(0, G, (Q,), device=dev, generator=g)
    gallery = torch.nn.functional.normalize(centers + 0.5 * torch.randn(G, D, device=dev, generator=g, dtype=torch.float64) / D ** 0.5)
    strength = 1.0 + 7.0 * torch.rand(Q, 1, device=dev, generator=g, dtype=torch.float64)
    query = torch.nn.functional.normalize(centers[mask] + strength * torch.randn(Q, D, device=dev, generator=g, dtype=torch.float64) / D ** 0.5)
    r = {"Q": Q, "G": G, "D": D, "K": K}
    eval_ijbc.identification_rank_topk(query, gallery, mask, K)
    r["rank_topk_ms"] = timed(lambda: eval_ijbc.identification_rank_topk(query, gallery, mask, K), a.reps)
    r["rank_topk_useful_tflops"] = 2.0 * Q * G * D / r["rank_topk_ms"] / 1e9
    r["rank_topk_k1024_ms"] = timed(lambda: eval_ijbc.identification_rank_topk(query, gallery, mask, 1024), a.reps)
    q32, g32, gid = query.float(), gallery.float(), torch.arange(G, device=dev)
    eval_1n.identification_topk(q32, mask, g32, gid, [0, G], 1024)
    r["ident_topk_f32_k1024_ms"] = timed(lambda: eval_1n.identification_topk(q32, mask, g32, gid, [0, G], 1024), a.reps)
    r["ident_topk_f32_tflops"] = 2.0 * Q * G * D / r["ident_topk_f32_k1024_ms"] / 1e9
    t0 = time.perf_counter()
    rank, pr, ties = eval_ijbc.evaluation(query, gallery, mask, return_ties=True)
    r["evaluation_s"] = time.perf_counter() - t0
    r["rank"], r["pr"], r["ties"] = rank, {str(k): v for k, v in pr.items()}, ties
    if a.host:
        qh, gh, mh = query.cpu().numpy(), gallery.cpu().numpy(), mask.cpu().numpy()
        t0 = time.perf_counter()
        hrank, hpr = host_evaluation(qh, gh, mh)
        r["host_evaluation_s"] = time.perf_counter() - t0
        r["host_equal"] = bool(hrank == rank and list(hpr.values()) == list(pr.values()))
    # the whole job from image features: 469 375 images, every template with at least one image, gallery subjects = template index
    N = 469375
    rng = np.random.default_rng(1)
    T = G + Q
    templates = np.concatenate([np.arange(T), rng.integers(0, T, N - T)])
    templates = rng.permutation(templates) + 1
    medias = templates * 10 + rng.integers(0, 3, N)
    feats = torch.randn(N, D, device=dev, generator=g)
    face = torch.rand(N, device=dev, generator=g) * 0.5 + 0.5
    gal_t, gal_id = np.arange(G) + 1, np.arange(G)
    probe_t, probe_id = np.arange(G, T) + 1, rng.integers(0, G, Q)
    t0 = time.perf_counter()
    eval_ijbc.ijbc_1n(feats, templates, medias, gal_t, gal_id, probe_t, probe_id, faceness=face)
    torch.cuda.synchronize()
    r["job_1n_s"] = time.perf_counter() - t0
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--job", choices=("1:1", "1:n", "both"), default="both")
    ap.add_argument("--host", action="store_true", help="job 1:N: also time the numpy restatement of the reference's evaluation on the host")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.job == "1:n":
        print(json.dumps({"job_1n": job_1n(a, dev)}))
        return
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
    if a.job == "both":
        del feats, face, p1, p2, label, tf, res
        r["job_1n"] = job_1n(a, dev)
    print(json.dumps(r))


if __name__ == "__main__":
    main()
