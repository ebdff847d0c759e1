#!/usr/bin/env python3
"""Time the drift-term instantiations of the SGD kernel beside the two existing ones, SCAFFOLD's end-of-round pass, and one FusedTrainer
step with and without both terms, in ONE process on one GPU (numbers of different runs are never compared).

At the iresnet100 parameter count (65 156 160 fp32), momentum step (first = 0), with the 16-bit mirror:

    sgd_step / sgd_step_scaled                 the existing entry points (plain / guarded)
    drift plain|guarded anchor|corr|both       fedfr_sgd_step_drift, the six new instantiations
    scaffold_control corr|nocorr               fedfr_scaffold_control

All rows are timed in interleaved rounds (row A, B, C, ..., A, B, C, ...), every launch between its own pair of HIP events after --warmup
rounds; each row is the median of --reps rounds (min and max reported too), with the GB/s against the bytes the ALGORITHM needs

    SGD step              22 n (p and buf read and written, g read, the mirror written) + 4 n per drift stream + 4 n guarded (g written back)
    scaffold_control      24 n with corr (c_i, x, y, corr read; c_i, dc written), 20 n without

and the ratio of every SGD row to the plain row beside the ratio of their bytes.  --trainer adds one iresnet100 B = 128 FusedTrainer.step()
with and without anchor + corr, two trainers stepped alternately.  The loaded library is the one FEDFR_HIP_LIB_NAME selects: a build with
-DFEDFR_DRIFT_LD_ONCE=1 times the non-temporal loads of the two streams.

No GPU: an error.
usage: python tools/drift_bench.py [--n N] [--reps 20] [--warmup 3] [--trainer] [--limit 420] [--out FILE]
"""
import argparse
import json
import os
import signal
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IRESNET100_PARAMS = 65156160


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=IRESNET100_PARAMS)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trainer", action="store_true", help="also time one iresnet100 B = 128 FusedTrainer step with and without both terms")
    ap.add_argument("--limit", type=int, default=420, help="seconds after which the process gives up")
    ap.add_argument("--out", default=None, help="also write the JSON result line to this file")
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: (sys.stderr.write("drift_bench: time limit of %d s reached\n" % a.limit), os._exit(3)))
    signal.alarm(a.limit)

    import torch
    from fedfr_amd import _C
    if not torch.cuda.is_available():
        sys.exit("drift_bench: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    n = a.n
    g_ = torch.Generator(device=dev).manual_seed(1)

    def rnd(scale):
        return (torch.rand(n, generator=g_, device=dev) - 0.5) * scale

    p, grad, buf = rnd(1.0), rnd(0.01), rnd(0.01)
    anchor, corr = p + rnd(0.01), rnd(0.01)
    shadow = torch.empty(n, dtype=_C.storage_dtype(), device=dev)
    ci, dc, y = rnd(0.01), torch.empty(n, device=dev), p + rnd(0.01)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    st = _C.stream()
    hyper = (1e-3, 0.9, 5e-4, 0)
    base = (p.data_ptr(), grad.data_ptr(), buf.data_ptr(), shadow.data_ptr(), n, *hyper)

    def drift(guarded, has_a, has_c):
        _C.call("fedfr_sgd_step_drift", *base, 1.0, word.data_ptr() if guarded else None, anchor.data_ptr() if has_a else None,
                0.01 if has_a else 0.0, corr.data_ptr() if has_c else None, st)

    group = [("sgd_step", lambda: _C.call("fedfr_sgd_step", *base, st), 22),
             ("sgd_step_scaled", lambda: _C.call("fedfr_sgd_step_scaled", *base, 1.0, word.data_ptr(), st), 26)]
    for guarded in (False, True):
        for name, has_a, has_c in (("anchor", True, False), ("corr", False, True), ("both", True, True)):
            group.append(("drift %s %s" % ("guarded" if guarded else "plain", name), (lambda g=guarded, x=has_a, c=has_c: drift(g, x, c)),
                          22 + 4 * (has_a + has_c) + 4 * guarded))
    for name, cptr, per in (("corr", corr.data_ptr(), 24), ("nocorr", None, 20)):
        group.append(("scaffold_control %s" % name,
                      (lambda cptr=cptr: _C.call("fedfr_scaffold_control", ci.data_ptr(), dc.data_ptr(), anchor.data_ptr(), y.data_ptr(), cptr, 2.0, n, st)), per))
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
    for name, _, per in group:
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev[name])
        med = ms[len(ms) // 2]
        res[name] = {"bytes_per_element": per, "ms_median": med, "ms_min": ms[0], "ms_max": ms[-1], "gbps_median": per * n / med / 1e6}
    plain = res["sgd_step"]
    for name, _, per in group:
        r = res[name]
        if not name.startswith("scaffold"):
            r["ratio_to_plain"], r["byte_ratio_to_plain"] = r["ms_median"] / plain["ms_median"], per / 22.0
        print("%-28s %.3f ms median (min %.3f, max %.3f)  %5.0f GB/s of %d B/element%s" % (
            name, r["ms_median"], r["ms_min"], r["ms_max"], r["gbps_median"], per,
            "" if name.startswith("scaffold") else "  x%.3f of plain (bytes x%.3f)" % (r["ratio_to_plain"], r["byte_ratio_to_plain"])))
    assert bool(torch.isfinite(p).all()) and int(word[0]) == 0
    out = {"n": n, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "library": os.environ.get("FEDFR_HIP_LIB_NAME", "libfedfr_hip.so"), "kernels": res}
    del p, grad, buf, anchor, corr, shadow, ci, dc, y

    if a.trainer:
        from fedfr_amd import backbones, client
        B, C_ = 128, 1000
        imgs = torch.rand(B, 3, 112, 112, generator=g_, device=dev) * 2 - 1
        lab = torch.randint(0, C_, (B,), generator=g_, device=dev)
        trainers = {}
        for name in ("plain", "both"):
            torch.manual_seed(3)
            m = backbones.iresnet100(False, dropout=0, fp16=True).to(dev)
            m._ensure_device_state()
            nt = m.trainable_count()
            terms = None
            if name == "both":
                terms = client.DriftTerms(m._flat_params[:nt].clone(), 0.01, (torch.rand(nt, generator=g_, device=dev) - 0.5) * 1e-4)
            fc = torch.randn(C_, 512, device=dev) * 0.01
            trainers[name] = client.FusedTrainer(m, fc, "CosFace", 30.0, 0.4, lr=0.01, aux_slot=len(trainers), drift=terms)
        for _ in range(a.warmup):
            for tr in trainers.values():
                tr.step(imgs, lab)
        torch.cuda.synchronize()
        tev = {name: [] for name in trainers}
        for _ in range(a.reps):
            for name, tr in trainers.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                loss = tr.step(imgs, lab)
                e1.record()
                tev[name].append((e0, e1))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss))
        out["trainer"] = {"arch": "iresnet100", "batch": B}
        for name in trainers:
            ms = sorted(e0.elapsed_time(e1) for e0, e1 in tev[name])
            out["trainer"][name] = {"ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1]}
            print("FusedTrainer.step %-6s %.3f ms median (min %.3f, max %.3f)" % (name, ms[len(ms) // 2], ms[0], ms[-1]))
        for tr in trainers.values():
            tr.finish()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    signal.alarm(0)


if __name__ == "__main__":
    main()
