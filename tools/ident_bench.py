#!/usr/bin/env python3
"""1:N identification (fedfr_amd.eval_1n, local_all.py:142-176 + the --task 1:n loop :274-297) at the reference's full local setting on one
MI355X: 160 000 queries (4 000 ids x 40 images), a 4 000-id gallery split over 40 clients, D = 512, K = ceil(160 000 * 1e-3) = 160.
One ``identification_topk`` call covers all 40 clients (the fp64-MFMA similarity GEMM, 0.66 TFLOP, with the top-K epilogue).
Prints one JSON line: ms per whole 40-client evaluation, fp64 TFLOP/s and its fraction of the 78.6 TF peak, the call's peak device
memory, and the numpy restatement of the reference's per-client step timed on a bounded sample (extrapolated to all 40 clients).
usage: python tools/ident_bench.py [--reps N]"""
import argparse
import heapq
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F

from fedfr_amd import eval_1n

FP64_PEAK_TF = 78.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-sample", type=int, default=8000, help="queries of the numpy sample (one client)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    Q, G, D, S, ipi = 160000, 4000, 512, 40, 40
    K = max(eval_1n.required_topk(Q))
    g = torch.Generator(device=dev).manual_seed(0)
    centers = F.normalize(torch.randn(G, D, device=dev, generator=g))
    qid = torch.arange(Q, device=dev) // ipi
    query = F.normalize(centers[qid] + 3.0 * torch.randn(Q, D, device=dev, generator=g) / D ** 0.5)
    gallery = F.normalize(centers + 0.5 * torch.randn(G, D, device=dev, generator=g) / D ** 0.5)
    gid = torch.arange(G, device=dev)
    per = G // S
    seg = [s * per for s in range(S + 1)]

    def run():
        pos, top, _ = eval_1n.identification_topk(query, qid, gallery, gid, seg, K)
        return pos, top

    for _ in range(3):
        run()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    run()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    # the whole evaluation as a user sees it: kernels + host read-out of all 40 clients (device->host copies included)
    t0 = time.perf_counter()
    for _ in range(3):
        pos, top = run()
        p, t = pos.cpu().numpy(), top.cpu().numpy()
        rates = [eval_1n.identification_rates(p[c * per * ipi:(c + 1) * per * ipi], t[c], Q, per, ipi)[0] for c in range(S)]
    e2e_ms = (time.perf_counter() - t0) / 3 * 1e3
    med = float(np.median(ms))
    flop = 2.0 * Q * G * D
    tf = flop / (med * 1e-3) / 1e12

    # numpy restatement of local_all.evaluation (float32 matmul, argsort of every row, heap top-K of the negatives) for one client on a
    # sample of queries: time scales with the matrix entries, extrapolated to Q queries x 40 clients
    qs = a.cpu_sample
    qn = query[:qs].cpu().numpy()
    gn = gallery[:per].cpu().numpy()
    mask = np.where(np.arange(qs) < per * ipi, np.arange(qs) // ipi, -1)
    t0 = time.perf_counter()
    sim = np.dot(qn, gn.T)
    np.argsort(-sim)
    rows = np.where(mask != -1)[0]
    pos_sims = sim[rows, mask[rows]].copy()
    sim[rows, mask[rows]] = -2.0
    neg = heapq.nlargest(max(1, math.ceil(qs * 1e-3)), sim[np.where(sim > -2.0)])
    [np.sum(pos_sims > neg[k - 1]) for k in eval_1n.required_topk(qs)]
    cpu_s = time.perf_counter() - t0
    out = {"metric": "ident_1n_local_40clients", "Q": Q, "G": G, "D": D, "clients": S, "K": K,
           "ms": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "reps": a.reps,
           "ms_with_host_readout": round(e2e_ms, 2),
           "fp64_tflops": round(tf, 2), "frac_of_fp64_peak": round(tf / FP64_PEAK_TF, 3),
           "peak_mem_bytes": int(peak), "matrix_bytes_if_materialised": Q * G * 8,
           "numpy_sample": {"queries": qs, "gallery": per, "s": round(cpu_s, 3),
                            "est_full_40_clients_s": round(cpu_s * (Q / qs) * S, 1)},
           "rate_client0": [round(float(r), 5) for r in rates[0]]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
