#!/usr/bin/env python3
"""Local 1:1 verification of all clients on one feature matrix (local_all.py:303-335): ONE eval_roc.roc_histogram_groups call against
G x (order_targets + roc_histogram), the reference's one-roc_cuda.py-run-per-client structure on the existing single-range kernel.

Default shape: N = 160 000 (40 images x 4000 identities), D = 512, G = 40 clients of 100 identities.  Both sides run in this process on
the same tensors, after a warm-up call each, timed with device events around synchronised regions; the median of --reps runs is kept.
The two results must be equal (integer counts).  Writes profiles/local_veri_bench_v1.json (--out) and prints the same JSON line.
usage: python tools/local_veri_bench.py [--n-ids 4000] [--per-id 40] [--clients 40] [--dim 512] [--reps 3] [--out PATH]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    fn()                                                     # warm-up: allocator, code object load
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return out, sorted(ms)[len(ms) // 2], ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-ids", type=int, default=4000)
    ap.add_argument("--per-id", type=int, default=40)
    ap.add_argument("--clients", type=int, default=40)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_veri_bench_v1.json"))
    args = ap.parse_args()
    from fedfr_amd import eval_roc, ops
    dev = torch.device("cuda:0")
    N, D, G = args.n_ids * args.per_id, args.dim, args.clients
    per = args.n_ids // G
    gen = torch.Generator(device=dev).manual_seed(0)
    lab = torch.arange(args.n_ids, device=dev).repeat_interleave(args.per_id)
    cen = torch.randn(args.n_ids, D, generator=gen, device=dev)
    feats, _ = ops.normalize_rows(cen[lab] + 0.7 * torch.randn(N, D, generator=gen, device=dev))
    del cen
    group = torch.where(lab < per * G, torch.div(lab, per, rounding_mode="floor"), torch.full_like(lab, -1))

    def grouped():
        return eval_roc.roc_histogram_groups(feats, lab, group, G)

    def per_client():
        out = []
        for c in range(G):
            f, l, t = eval_roc.order_targets(feats, lab, range(c * per, (c + 1) * per))
            out.append(eval_roc.roc_histogram(f, l, t))
        return torch.stack(out)

    h_new, ms_new, all_new = timed(grouped, args.reps)
    h_old, ms_old, all_old = timed(per_client, args.reps)
    equal = bool(torch.equal(h_new, h_old))
    sizes = torch.bincount(group[group >= 0], minlength=G).tolist()
    pairs_old = sum(t * (t - 1) // 2 + t * (N - t) for t in sizes)               # pairs with a target row, per client: what both count
    ung = N - sum(sizes)
    pairs_new = N * (N - 1) // 2 - ung * (ung - 1) // 2                          # dot products of the one pass
    res = {"tool": "local_veri_bench", "device": torch.cuda.get_device_name(0), "N": N, "D": D, "G": G, "reps": args.reps,
           "grouped_ms": round(ms_new, 2), "grouped_ms_all": [round(v, 2) for v in all_new],
           "per_client_ms": round(ms_old, 2), "per_client_ms_all": [round(v, 2) for v in all_old],
           "speedup": round(ms_old / ms_new, 3), "dot_products_grouped": pairs_new, "dot_products_per_client": pairs_old,
           "grouped_tflops_fp64": round(2.0 * D * pairs_new / (ms_new * 1e-3) / 1e12, 2), "results_equal": equal,
           "pairs_counted": int(h_new.sum().item())}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    if not equal:
        raise SystemExit("local_veri_bench: the grouped pass and the per-client launches disagree")


if __name__ == "__main__":
    main()
