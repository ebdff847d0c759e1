#!/usr/bin/env python3
"""Forward + backward time of the BottleBlock converter (D = 512, bottle_rate 4) at B = 8, 256, 1024: the fused kernels (csrc/bottle.hip,
2 + 2 launches) against the same math composed from the primitives the package had before them (ops.sgemm, ops.colsum, torch elementwise
LeakyReLU / cat / add).  HIP events in one process; the two paths alternate, ROUNDS windows of ITERS calls each after a warm-up of both;
the median window and the spread are reported.  Outputs of the two paths are compared first (same products, another summation order in the
split-K GEMMs of the composed path).  usage: python tools/bottle_bench.py [iters] [rounds]      Prints one JSON line per batch size."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from fedfr_amd import ops
from fedfr_amd.backbones import bottle

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 500
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
D, H, SLOPE = 512, 128, 0.01
dev = torch.device("cuda:0")
launches = {"n": 0}


def fused(x, P, dy):
    y, h1, h2 = bottle.bottle_forward(x, P)
    dx, grads = bottle.bottle_backward(x, P, h1, h2, dy)
    return y, dx, grads


def composed(x, P, dy):
    """every line that enqueues work counts its launches (ops.sgemm adds a slab sum when it splits K: counted by the caller below)"""
    n = 0
    h1s, h2s = [], []
    for g in range(4):
        h1 = F.leaky_relu(ops.sgemm(x, P[4 * g], trans_b=True, bias=P[4 * g + 1]), SLOPE)
        h2 = F.leaky_relu(ops.sgemm(h1, P[4 * g + 2], trans_b=True, bias=P[4 * g + 3]), SLOPE)
        h1s.append(h1), h2s.append(h2)
        n += 4
    cat = torch.cat(h2s, 1)
    y = x + ops.sgemm(cat, P[16], trans_b=True, bias=P[17])
    n += 3
    fwd = n
    grads = [None] * 18
    grads[16], grads[17] = ops.sgemm(dy, cat, trans_a=True), ops.colsum(dy)
    dcat = ops.sgemm(dy, P[16])
    dx = dy.clone()
    n += 4
    for g in range(4):
        dz2 = torch.ops.aten.leaky_relu_backward(dcat[:, g * H:(g + 1) * H], h2s[g], SLOPE, False).contiguous()
        grads[4 * g + 2], grads[4 * g + 3] = ops.sgemm(dz2, h1s[g], trans_a=True), ops.colsum(dz2)
        dz1 = torch.ops.aten.leaky_relu_backward(ops.sgemm(dz2, P[4 * g + 2]), h1s[g], SLOPE, False)
        grads[4 * g], grads[4 * g + 1] = ops.sgemm(dz1, x, trans_a=True), ops.colsum(dz1)
        dx += ops.sgemm(dz1, P[4 * g])
        n += 9
    launches["fwd"], launches["bwd"] = fwd, n - fwd
    return y, dx, grads


def window(fn, args):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn(*args)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / ITERS * 1e3          # us per forward + backward


def main():
    assert torch.cuda.is_available(), "bottle_bench needs an MI355X"
    torch.manual_seed(0)
    for B in (8, 256, 1024):
        x, dy = (torch.rand(B, D, device=dev) * 2 - 1 for _ in range(2))
        P = []
        for s in [t for _ in range(4) for t in ((H, D), (H,), (H, H), (H,))] + [(D, D), (D,)]:
            fan_in = s[1] if len(s) == 2 else P[-1].shape[1]
            P.append((torch.rand(*s, device=dev) * 2 - 1) / fan_in ** 0.5)
        a, b = fused(x, P, dy), composed(x, P, dy)
        worst = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip([a[0], a[1]] + a[2], [b[0], b[1]] + b[2]))
        assert worst < 1e-4, worst
        # the slab sums of the composed path's split-K GEMMs (K = B >= 1024 over few tiles): one more launch each
        extra = (1 if ops._auto_splits(D, D, B) > 1 else 0) + 4 * ((1 if ops._auto_splits(H, H, B) > 1 else 0) + (1 if ops._auto_splits(H, D, B) > 1 else 0))
        for _ in range(20):
            fused(x, P, dy), composed(x, P, dy)
        torch.cuda.synchronize()
        tf, tc = [], []
        for _ in range(ROUNDS):
            tf.append(window(fused, (x, P, dy)))
            tc.append(window(composed, (x, P, dy)))
        print(json.dumps({"what": "BottleBlock forward + backward", "B": B, "D": D, "iters": ITERS, "rounds": ROUNDS,
                          "fused_us": round(statistics.median(tf), 2), "fused_us_min_max": [round(min(tf), 2), round(max(tf), 2)],
                          "composed_us": round(statistics.median(tc), 2), "composed_us_min_max": [round(min(tc), 2), round(max(tc), 2)],
                          "ratio": round(statistics.median(tc) / statistics.median(tf), 2),
                          "fused_launches": [2, 2], "composed_launches": [launches["fwd"], launches["bwd"] + extra],
                          "max_rel_diff": worst}), flush=True)


if __name__ == "__main__":
    main()
