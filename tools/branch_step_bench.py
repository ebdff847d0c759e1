#!/usr/bin/env python3
"""A/B of the train_with_public_data step: the fused branch head (client.FusedBranchTrainer, csrc/branch.hip) against the autograd closure
it replaces (client.FusedHeadTrainer on client.public_head_loss: the closure Client.train_with_public_data itself builds under
FEDFR_FUSED_BRANCH=0), same process, same box, rounds interleaved A B A B ... the way
tools/ab.sh alternates builds.  iresnet100, B = 128, 100 local + 6000 public classes, BCE on, contrastive on and off, warm.

Two figures per path, both from HIP events:
  step  the whole trainer step (forward, head, backward, updates), the loss read back every step as Client.train_with_public_data does
  head  from the end of _forward to the start of _backward (the kernels of the head and whatever host gaps starve the GPU between them)
The frozen global / last-round embeddings of the contrastive term are fixed tensors: those two eval forward passes are the same launches on
both paths and are not part of the step measured here.

usage: python tools/branch_step_bench.py [arch] [rounds] [steps per round] [converter_layer] [out.json]
Prints one JSON line per (variant, path) and a verdict line; the spread of a figure is max - min of its per-round means."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from fedfr_amd import _C, backbones, client, losses  # noqa: E402
from fedfr_amd.config import config as cfg  # noqa: E402

arch = sys.argv[1] if len(sys.argv) > 1 else "iresnet100"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
conv_layer = int(sys.argv[4]) if len(sys.argv) > 4 else 1
out_path = sys.argv[5] if len(sys.argv) > 5 else None
dev = torch.device("cuda:0")
B, NL, NP, LR = 128, 100, 6000, 1e-3            # (random-init weights and two fixed random batches: the reference's 0.05 diverges)


class _Timed:
    """records a HIP event pair around the head segment of every step"""

    def _forward(self, *a, **k):
        out = super()._forward(*a, **k)
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self._head_t0 = e
        return out

    def _backward(self, *a, **k):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.head_events.append((self._head_t0, e))
        return super()._backward(*a, **k)


class TimedBranch(_Timed, client.FusedBranchTrainer):
    pass


class TimedHead(_Timed, client.FusedHeadTrainer):
    pass


def make(path, use_con):
    torch.manual_seed(100)                         # both paths start from the same random weights
    bb = getattr(backbones, arch)(False, dropout=0, fp16=True).to(dev)
    fcm = client.FC_module(512, NL, "/tmp").to(dev)
    fcm.update_with_pretrain((torch.randn(NP, 512) * 0.01).to(dev))
    bm = client.BCE_module(512, NL, conv_layer).to(dev)
    gf, lf = (torch.randn(B, 512, device=dev), torch.randn(B, 512, device=dev)) if use_con else (None, None)
    if path == "fused":
        tr = TimedBranch(bb, fcm, bm, "CosFace", 30.0, 0.4, detach=False, mu=cfg.mu if use_con else 0.0, temperature=0.5, bce_weight=10.0,
                         lr=LR, momentum=cfg.momentum, weight_decay=cfg.weight_decay)
        tr.head_events = []
        return tr, lambda x, y: tr.step(x, y, gf, lf)
    margin, bce_loss = losses.CosFace(s=30, m=0.4), losses.BCE_loss()
    tr = TimedHead(bb, list(fcm.parameters()) + list(bm.parameters()), lr=LR, momentum=cfg.momentum, weight_decay=cfg.weight_decay)
    tr.head_events = []
    head_loss = client.public_head_loss(margin, fcm, bm, bce_loss, False, None, {"global_feats": gf, "last_feats": lf} if use_con else None,
                                        0.5, cfg.mu)
    return tr, lambda x, y: tr.step(x, y, head_loss)


def main():
    torch.manual_seed(7)
    imgs = [(torch.rand(B, 3, 112, 112) * 2 - 1).to(dev) for _ in range(2)]
    labs = [torch.randint(0, NL + NP, (B,)).to(dev) for _ in range(2)]
    results = []
    for use_con in (True, False):
        runs = {p: make(p, use_con) for p in ("fused", "closure")}
        step_ms = {p: [] for p in runs}
        head_ms = {p: [] for p in runs}
        last = {}
        for p, (tr, one) in runs.items():          # warm: plans, arenas, momentum buffers, the allocator's pools
            for i in range(3):
                one(imgs[i % 2], labs[i % 2])[0].item()
            tr.head_events.clear()
        torch.cuda.synchronize()
        for r in range(rounds):
            for p, (tr, one) in runs.items():      # interleaved: fused, closure, fused, closure, ...
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(steps):
                    last[p] = one(imgs[i % 2], labs[i % 2])[0].item()
                e1.record()
                torch.cuda.synchronize()
                step_ms[p].append(e0.elapsed_time(e1) / steps)
                head_ms[p].append(sum(a.elapsed_time(b) for a, b in tr.head_events) / len(tr.head_events))
                tr.head_events.clear()
        for p, (tr, _) in runs.items():
            tr.finish()
            mean = lambda v: sum(v) / len(v)                                    # noqa: E731
            row = {"variant": "bce+contrastive" if use_con else "bce", "path": p, "arch": arch, "batch": B, "classes": NL + NP,
                   "converter_layer": conv_layer, "rounds": rounds, "steps_per_round": steps,
                   "step_ms": round(mean(step_ms[p]), 4), "step_ms_spread": round(max(step_ms[p]) - min(step_ms[p]), 4),
                   "head_ms": round(mean(head_ms[p]), 4), "head_ms_spread": round(max(head_ms[p]) - min(head_ms[p]), 4),
                   "step_ms_rounds": [round(v, 4) for v in step_ms[p]], "head_ms_rounds": [round(v, 4) for v in head_ms[p]],
                   "last_loss": last[p], "storage": str(_C.storage_dtype()).split(".")[-1]}
            results.append(row)
            print(json.dumps(row), flush=True)
        del runs
        torch.cuda.empty_cache()
    verdict = []
    for v in ("bce+contrastive", "bce"):
        f = next(r for r in results if r["variant"] == v and r["path"] == "fused")
        c = next(r for r in results if r["variant"] == v and r["path"] == "closure")
        spread = max(f["step_ms_spread"], c["step_ms_spread"])
        verdict.append({"variant": v, "step_ms_fused_minus_closure": round(f["step_ms"] - c["step_ms"], 4), "spread_ms": spread,
                        "head_ms_fused_minus_closure": round(f["head_ms"] - c["head_ms"], 4),
                        "not_slower_than_spread": f["step_ms"] - c["step_ms"] <= spread})
    print(json.dumps({"verdict": verdict}), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump({"results": results, "verdict": verdict}, fh, indent=1)


if __name__ == "__main__":
    main()
