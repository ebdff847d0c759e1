"""Server optimisers (FedAvgM / FedAdagrad / FedAdam / FedYogi with update clipping), the part that needs no GPU: the C ABI carries the
new entry points, no instantiation of the two kernels spills, the restatement of tests/fedopt_cases.py obeys the laws the algorithms
define (and meets, alone, the fp64 bound the GPU tests hold the kernel to), and the Python surface validates its arguments."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import fedopt_cases as F
from conftest import REPO

f32, f64 = np.float32, np.float64
NEW_SYMBOLS = ("fedfr_fedopt_sqnorm_workspace_bytes", "fedfr_fedopt_sqnorm", "fedfr_fedopt_multi")


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from fedfr_amd import _C
    return _C


def test_header_ctypes_table_and_library_carry_the_fedopt_symbols(built_lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "fedfr_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fedfr_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\sT\s+(fedfr_[a-z0-9_]+)", out))
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in built_lib.SIGNATURES, s
        assert s in exported, s
    lib = built_lib.lib()
    # the workspace query is host code: [k][grid] doubles with fedavg_multi's grid rule, 0 for arguments the kernel refuses
    for n in F.SIZES:
        for k in F.KS:
            assert lib.fedfr_fedopt_sqnorm_workspace_bytes(k, n) == 8 * k * F.grid(n), (k, n)
    assert F.grid(F.SIZES[-1]) == F.GRID_CAP and F.grid(F.SIZES[-1] - 1024) == F.GRID_CAP and F.grid(4103) == 5
    assert lib.fedfr_fedopt_sqnorm_workspace_bytes(0, 100) == 0 and lib.fedfr_fedopt_sqnorm_workspace_bytes(9, 100) == 0
    assert lib.fedfr_fedopt_sqnorm_workspace_bytes(3, 0) == 0


def test_fedopt_kernels_do_not_spill(built_lib):
    """every instantiation (K = 1..8 x four kinds, K = 1..8 norms, both storage builds) is HBM-bound streaming code: no scratch"""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr.kernels(built_lib.LIB_PATH)
    bf16 = os.path.join(os.path.dirname(built_lib.LIB_PATH), "libfedfr_hip_bf16.so")
    if os.path.exists(bf16) and os.path.basename(built_lib.LIB_PATH) != "libfedfr_hip_bf16.so":
        ks.update({"bf16:" + k: v for k, v in kr.kernels(bf16).items()})
    builds = 2 if any(k.startswith("bf16:") for k in ks) else 1
    multi = {n: r for n, r in ks.items() if "fedopt_multi_kernel" in n}
    sqn = {n: r for n, r in ks.items() if "fedopt_sqnorm_kernel" in n}
    assert len(multi) == 32 * builds and len(sqn) == 8 * builds, (len(multi), len(sqn))
    bad = [(n, r) for n, r in list(multi.items()) + list(sqn.items()) if r["scratch"]]
    assert not bad, bad


# ---- laws of the restatement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", F.KS)
def test_avgm_without_momentum_is_the_weighted_mean(k):
    """beta1 = 0, lr = 1, no clip: x' = x + sum w_i (x_i - x) = the weighted mean, within (k + 3) 2^-24 (|x| + sum |w_i| |x_i - x|)"""
    n = 4103
    x, xs, m, _ = F.inputs(n, k)
    ws = F.weights(k)
    h = F.hyper(lr=1.0, beta1=0.0)
    m1, v1, x1 = F.run32("AVGM", x, xs, ws, m, None, h)
    assert v1 is None
    mean = sum(f64(w) * xi.astype(f64) for w, xi in zip(ws, xs))
    bound = (k + 3) * F.U * (np.abs(x.astype(f64)) + sum(abs(f64(w)) * np.abs(xi.astype(f64) - x.astype(f64)) for w, xi in zip(ws, xs)))
    err = np.abs(x1.astype(f64) - mean)
    print("k=%d max err/bound %.3f" % (k, float(np.max(err / bound))))
    assert np.all(err <= bound)
    assert np.array_equal(m1, F.delta32(x, xs, ws))        # 0 * m + Delta == Delta


def test_momentum_two_round_closed_form():
    """from m = 0: x_2 = x_0 + lr ((1 + beta1) Delta_1 + Delta_2), m_2 = beta1 Delta_1 + Delta_2 — the moments persist between rounds"""
    n, k = 1023, 3
    ws = F.weights(k)
    h = F.hyper(lr=0.7, beta1=0.9)
    x0, xa, _, _ = F.inputs(n, k, tag=0.0)
    m0 = np.zeros(n, f32)
    d1, _ = F.delta64(x0, xa, ws)
    m1, _, x1, _ = F.step64("AVGM", x0, m0, None, d1, h)
    _, xb, _, _ = F.inputs(n, k, tag=1.0)
    d2 = sum(f64(w) * (xi.astype(f64) - x1) for w, xi in zip(ws, xb))
    m2 = f64(h[1]) * m1 + d2
    x2 = x1 + f64(h[0]) * m2
    assert np.allclose(m2, f64(h[1]) * d1 + d2, rtol=1e-13, atol=1e-16)
    assert np.allclose(x2, x0.astype(f64) + f64(h[0]) * ((1 + f64(h[1])) * d1 + d2), rtol=1e-13, atol=1e-16)
    # the fp32 form on dyadic values (every operation exact): equality, not closeness
    xq = (np.round(x0 * 256) / 256).astype(f32)
    xsq = [(np.round(xi * 256) / 256).astype(f32) for xi in xa]
    hq = F.hyper(lr=1.0, beta1=0.5)
    one = [f32(1.0)]
    ma, _, xa1 = F.run32("AVGM", xq, xsq[:1], one, np.zeros(n, f32), None, hq)
    tgt = [(xa1 + (xsq[1] - xq)).astype(f32)]              # round 2: the client moves by Delta_2 = xsq[1] - xq from the new global
    mb, _, xb2 = F.run32("AVGM", xa1, tgt, one, ma, None, hq)
    dA, dB = xsq[0] - xq, xsq[1] - xq
    assert np.array_equal(mb, f32(0.5) * dA + dB) and np.array_equal(xb2, xq + (f32(1.5) * dA + dB))


def test_yogi_sign_rule_at_equality():
    """v' = v - (1 - beta2) D^2 sign(v - D^2): v shrinks towards D^2 from above, grows from below, and stays put AT v == D^2"""
    h = F.hyper(lr=0.01, beta1=0.9, beta2=0.75)
    x = np.zeros(3, f32)
    xs = [np.full(3, 0.5, f32)]
    v = np.array([0.25, 0.5, 0.125], f32)
    m = np.zeros(3, f32)
    m1, v1, x1 = F.run32("YOGI", x, xs, [f32(1.0)], m, v, h)
    assert v1[0] == f32(0.25) and v1[1] == f32(0.5 - 0.25 * 0.25) and v1[2] == f32(0.125 + 0.25 * 0.25)
    _, V1, _, _ = F.step64("YOGI", x, m, v, F.delta64(x, xs, [f32(1.0)])[0], h)
    assert np.array_equal(V1, v1.astype(f64))
    assert np.all(np.isfinite(x1)) and np.all(m1 == h[2] * f32(0.5))


def test_clipping_law():
    n, k = 4103, 3
    x, xs, _, _ = F.inputs(n, k)
    ws = F.weights(k)
    sq = F.sqnorm(x, xs)
    norms = np.sqrt(sq)
    clip = float(f32(0.5 * (np.sort(norms)[0] + np.sort(norms)[1])))       # between the smallest and the second smallest update norm
    c = F.clip_coef64(sq, ws, clip)
    for i in range(k):
        if norms[i] <= clip:
            assert c[i] == f64(ws[i])                                       # untouched
        else:
            assert abs(c[i] / f64(ws[i]) * norms[i] - clip) <= 4e-16 * clip   # the scaled update has norm clip, to fp64 rounding
    assert sum(norms <= clip) == 1 and sum(norms > clip) == k - 1
    assert np.array_equal(F.clip_coef(sq, ws, 0.0), np.array(ws, f32))      # clip = 0: w_i exactly
    assert np.array_equal(F.clip_coef(np.zeros(k), ws, 1.0), np.array(ws, f32))      # zero delta: w_i exactly
    assert np.array_equal(F.clip_coef(sq, ws, 1e9), np.array(ws, f32))      # nobody exceeds it


@pytest.mark.parametrize("kind", list(F.KINDS))
def test_restatement_meets_the_fp64_bound_alone(kind):
    """the float32 restatement against the fp64 evaluation on the inputs of the GPU test's fp64 comparison (same n, k, hyper-parameters)"""
    worst = 0.0
    for k in F.KS:
        for n in F.SIZES:
            x, xs, m, v = F.inputs(n, k, same_sign=True)
            ws = F.weights(k)
            h = F.hyper(lr=1.0 if kind == "AVGM" else 0.01)
            _, _, x1 = F.run32(kind, x, xs, ws, m, v, h)
            d, mag = F.delta64(x, xs, ws)
            _, _, X1, u = F.step64(kind, x, m, v, d, h)
            r = float(np.max(np.abs(x1.astype(f64) - X1) / F.fp64_bound(k, x, m, u, mag)))
            worst = max(worst, r)
            assert r <= 1.0, (kind, k, n, r)
    print("%s: worst error / bound %.3f" % (kind, worst))


# ---- Python surface ----------------------------------------------------------------------------------------------------------------------
def test_server_optimizer_state_dict_round_trip_and_names():
    from fedfr_amd import server
    opt = server.ServerOptimizer("ADAM", lr=0.03, beta1=0.8, beta2=0.95, tau=2e-3, clip_norm=1.5)
    opt.m = torch.arange(7, dtype=torch.float32) * 0.5
    opt.v = torch.arange(7, dtype=torch.float32) + 4e-6
    opt.rounds = 3
    sd = opt.state_dict()
    assert set(sd) == {"kind", "lr", "beta1", "beta2", "tau", "clip_norm", "rounds", "m", "v"}
    sd["m"][0] = 99.0                                                         # the snapshot is a copy
    assert float(opt.m[0]) == 0.0
    sd["m"][0] = 0.0
    new = server.ServerOptimizer("AVGM")
    new.load_state_dict(sd)
    assert (new.kind, new.lr, new.beta1, new.beta2, new.tau, new.clip_norm, new.rounds) == ("ADAM", 0.03, 0.8, 0.95, 2e-3, 1.5, 3)
    assert torch.equal(new.m, opt.m) and torch.equal(new.v, opt.v) and new.m.data_ptr() != sd["m"].data_ptr()
    assert new.hyper() == opt.hyper() == tuple(float(t) for t in F.hyper(0.03, 0.8, 0.95, 2e-3))
    new.reset()
    assert new.m is None and new.v is None and new.rounds == 0 and new.last_update_sqnorm is None
    fresh = server.ServerOptimizer("FedYogi")                                 # the aggr_alg spelling
    assert fresh.kind == "YOGI" and fresh.state_dict()["m"] is None
    server.ServerOptimizer("AVGM").load_state_dict(fresh.state_dict())
    for bad in ("Adam", "FedAvg", "", None, 2):
        with pytest.raises(ValueError):
            server.ServerOptimizer(bad)
    with pytest.raises(ValueError):
        new.load_state_dict(dict(sd, kind="SGD"))
    with pytest.raises(ValueError):
        server.ServerOptimizer("AVGM", clip_norm=-1.0)


def test_unknown_aggr_alg_and_cpu_states_raise():
    from fedfr_amd import server
    from fedfr_amd.client import FlatStateDict

    class Args:
        network, loss, local_epoch, output_dir, BCE_local, aggr_alg = "iresnet18", "CosFace", 1, "/tmp", False, "FedMedian"

    srv = server.Server([], None, Args, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="FedMedian"):
        srv.train()
    assert sorted(server.AGGR_ALG_KINDS) == ["FedAdagrad", "FedAdam", "FedAvgM", "FedYogi"]
    opt = server.ServerOptimizer("AVGM")
    cpu = FlatStateDict.from_flat((torch.zeros(8), torch.zeros(0), torch.zeros(0, dtype=torch.int64)), [], [])
    with pytest.raises(RuntimeError, match="GPU"):
        server.FedOpt(cpu, [cpu, cpu], [1.0, 1.0], opt)                      # FlatStateDicts, but not on the GPU
    with pytest.raises(RuntimeError, match="FlatStateDict"):
        server.FedOpt(cpu, [{"w": torch.zeros(8)}], [1.0], opt)
    with pytest.raises(ValueError, match="clip_norm"):
        server.fedavg_all_reduce(None, 1.0, 1.0, comm=object(), server_opt=server.ServerOptimizer("AVGM", clip_norm=1.0),
                                 prev_params=torch.zeros(8))
