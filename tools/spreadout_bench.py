#!/usr/bin/env python3
"""One spread-out iteration (normalise -> fused loss + gradient kernel -> normalise backward) on unit rows with planted near-duplicates:
ms, fp32 TFLOP/s of the first product (2 N^2 D / t), active 64 x 64 tiles / all tiles, peak extra device memory; the same with the tile
skip disabled (margin = -2: every tile active); and, at N = 4000, the reference's formulation (server.py:55-63) restated as plain torch ops
that materialise S, forward + backward, in the same process.  Prints one JSON line.
usage: python tools/spreadout_bench.py [--sizes 4000,85000] [--dim 512] [--reps 10]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fedfr_amd import ops  # noqa: E402


def planted(N, D, frac, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(N, D, generator=g, device=dev)
    x /= x.norm(dim=1, keepdim=True)
    n = max(2, int(N * frac))
    perm = torch.randperm(N, generator=g, device=dev)
    t = torch.linspace(0.5, 0.95, n, device=dev)[:, None]
    x[perm[:n]] = t * x[perm[n:2 * n]] + (1 - t * t).sqrt() * x[perm[:n]]
    return x.contiguous()


def timed(fn, warmup, reps):
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


def active_tiles(fn, margin, chunk=2048):
    """64 x 64 tiles of S with an off-diagonal element above the margin (torch fp32, S in row chunks)."""
    N = fn.shape[0]
    nt, hit = -(-N // 64), 0
    pad = torch.zeros(nt * 64, fn.shape[1], device=fn.device)
    pad[:N] = fn
    for r0 in range(0, nt * 64, chunk):
        s = pad[r0:r0 + chunk] @ pad.T
        k = torch.arange(s.shape[0], device=fn.device)
        s[k, k + r0] = -2.0
        hit += int((s.view(s.shape[0] // 64, 64, nt, 64) > margin).any(dim=3).any(dim=1).sum())
    return hit, nt * nt


def torch_formulation(fc, margin):
    x = fc.detach().clone().requires_grad_(True)
    fn = torch.nn.functional.normalize(x)
    s = fn @ fn.t()
    loss = (torch.relu(s.masked_select(~torch.eye(len(x), dtype=torch.bool, device=x.device)) - margin) ** 2).sum()
    loss.backward()
    return x.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4000,85000")
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--margin", type=float, default=0.4)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "dim": a.dim, "margin": a.margin, "sizes": {}}
    for N in (int(v) for v in a.sizes.split(",")):
        D = a.dim
        fc = planted(N, D, 0.001 if N > 10000 else 0.01, dev)

        def step(margin=a.margin):
            fn, inv = ops.normalize_rows(fc)
            loss, dfn, active = ops.spreadout_loss_grad(fn, margin, False)
            return ops.normalize_rows_bwd(fn, inv, dfn), active

        def kernel_only(margin=a.margin, fn=ops.normalize_rows(fc)[0]):
            return ops.spreadout_loss_grad(fn, margin, False)

        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        _, active = step()
        torch.cuda.synchronize()
        r = {"active_pairs": int(active), "peak_extra_bytes": torch.cuda.max_memory_allocated(dev) - base, "fc_bytes": N * D * 4}
        reps = a.reps if N <= 10000 else max(3, a.reps // 3)
        r["iteration"] = timed(step, 2, reps)
        r["kernel"] = timed(kernel_only, 1, reps)
        r["kernel_first_product_tflops"] = 2.0 * N * N * D / (r["kernel"]["median_ms"] * 1e-3) / 1e12
        r["kernel_all_tiles_active"] = timed(lambda: kernel_only(-2.0), 1, max(2, reps // 3))
        hit, tiles = active_tiles(ops.normalize_rows(fc)[0], a.margin)
        r["active_tiles"], r["tiles"] = hit, tiles
        if N <= 10000:
            r["torch_materialised_fwd_bwd"] = timed(lambda: torch_formulation(fc, a.margin), 2, a.reps)
        out["sizes"][str(N)] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
