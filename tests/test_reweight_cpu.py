"""Reweighted aggregation (GeoMedian / CenteredClip), the part that needs no GPU: the C ABI carries the three entry points, no ``reweight_``
kernel uses scratch memory, the restatements of tests/reweight_cases.py obey the laws the rules define, the rounds of the GPU tests are
conditioned (float32 restatement against the fp64 iteration) so that the check on the GPU is a condition and not a measurement, and the Python
surface validates its arguments and refuses what it cannot serve before any client trains."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import reweight_cases as W
import robust_cases as R
from conftest import REPO

f32, f64 = np.float32, np.float64
NEW_SYMBOLS = ("fedfr_reweight_workspace_bytes", "fedfr_reweight_step", "fedfr_reweight_weights")


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from fedfr_amd import _C
    return _C


def test_header_ctypes_table_and_library_carry_the_reweight_symbols(built_lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "fedfr_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fedfr_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\sT\s+(fedfr_[a-z0-9_]+)", out))
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in built_lib.SIGNATURES, s
        assert s in exported, s
    lib = built_lib.lib()
    # the workspace query is host code: [k][grid] doubles with fedavg_multi's grid rule, 0 for arguments the kernels refuse
    for n in R.SIZES:
        for k in (1, 2, 3, 8, 16, 17, 32):
            assert lib.fedfr_reweight_workspace_bytes(k, n) == 8 * k * R.grid(n), (k, n)
    for k, n in ((0, 100), (-1, 100), (33, 100), (3, 0)):
        assert lib.fedfr_reweight_workspace_bytes(k, n) == 0


def test_reweight_kernels_use_no_scratch_memory(built_lib):
    """every ``reweight_`` kernel (K = 1..32 step kernels with and without the store of the centre, the weights kernel; both storage
    builds): the states and the fp64 accumulators are registers, what is indexed at run time lives in LDS"""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr.kernels(built_lib.LIB_PATH)
    bf16 = os.path.join(os.path.dirname(built_lib.LIB_PATH), "libfedfr_hip_bf16.so")
    if os.path.exists(bf16) and os.path.basename(built_lib.LIB_PATH) != "libfedfr_hip_bf16.so":
        ks.update({"bf16:" + k: v for k, v in kr.kernels(bf16).items()})
    builds = 2 if any(k.startswith("bf16:") for k in ks) else 1
    rw = {n: r for n, r in ks.items() if "reweight_" in n}
    steps = [n for n in rw if "reweight_step_kernel" in n]
    assert len(steps) == 32 * 2 * builds, len(steps)
    assert sum("reweight_weights_kernel" in n for n in rw) == builds
    bad = [(n, r) for n, r in rw.items() if r["scratch"]]
    assert not bad, bad


# ---- laws of the restatement -------------------------------------------------------------------------------------------------------------
def _some_D(k, seed):
    rng = np.random.RandomState(seed)
    return (rng.rand(k) * 10.0 + 0.01) ** 2


@pytest.mark.parametrize("k", [1, 2, 5, 8, 17, 32])
def test_geomedian_weights_sum_to_one_and_cclip_weights_stay_below_the_prior(k):
    alpha = np.full(k, 1.0 / k)
    for seed in range(5):
        D = _some_D(k, seed)
        b, S, _, nf = W.weights64(W.GEOMEDIAN, D, alpha, 1e-6)
        assert b.dtype == f32 and nf == k and S > 0
        assert abs(float(b.astype(f64).sum()) - 1.0) <= k * 2.0 ** -24          # k roundings of at most half an ulp of a number <= 1
        for param in (0.0, 0.5, 3.0, 100.0):
            c, Sc, tau, _ = W.weights64(W.CCLIP, D, alpha, param)
            assert np.all(c <= f32(1.0 / k)) and np.all(c >= 0) and Sc == float(np.sum(c.astype(f64)))
            assert tau == (param if param else float(np.sort(np.sqrt(D))[(k - 1) // 2]))
        assert np.array_equal(W.weights64(W.CCLIP, D, alpha, 100.0)[0], np.full(k, 1.0 / k).astype(f32))      # nobody beyond tau: the plain mean


def test_non_finite_clients_get_zero_and_a_client_at_distance_zero_its_full_weight():
    alpha = np.array([0.1, 0.2, 0.3, 0.25, 0.15])
    D = np.array([4.0, np.inf, 0.0, np.nan, 1.0])
    for rule, param in ((W.GEOMEDIAN, 1e-6), (W.CCLIP, 0.0), (W.CCLIP, 0.5)):
        b, S, tau, nf = W.weights64(rule, D, alpha, param)
        assert nf == 3 and b[1] == 0 and b[3] == 0 and np.all(b[[0, 2, 4]] > 0)
        if rule == W.CCLIP:
            assert b[2] == f32(0.3)                                              # d = 0: the full prior weight
            assert tau == (0.5 if param else 1.0)                                # auto: the lower median of (2, 0, 1)
            assert b[0] == f32(0.1 * (tau / 2.0)) and b[4] == f32(0.15 * min(1.0, tau / 1.0))
        else:
            assert b[2] == f32((0.3 / 1e-6) / S) and b[2] > 0.999                # the smoothing nu: a client AT the centre takes (almost) all
    for rule, param in ((W.GEOMEDIAN, 1e-6), (W.CCLIP, 0.0)):
        b, S, tau, nf = W.weights64(rule, np.array([np.nan, np.inf, -np.inf]), [1 / 3] * 3, param)
        assert nf == 0 and not b.any() and S == 0.0
    b, _, tau, nf = W.weights64(W.CCLIP, np.array([np.nan, 9.0]), [0.5, 0.5], 0.0)      # one finite client: it is its own median
    assert nf == 1 and tau == 3.0 and b.tolist() == [0.0, 0.5]
    assert W.weights64(W.CCLIP, np.array([16.0, 9.0]), [0.5, 0.5], 0.0, tau=1.0)[2] == 1.0      # a later slot keeps the round's tau


@pytest.mark.parametrize("k", [1, 3, 8, 17])
def test_equal_clients_do_not_move_the_centre(k):
    """every client equal to z: delta = 0, beta delta = +-0, z + 0 = z bit for bit (z != -0 here), distances 0, for both rules and any R"""
    z0 = W.base(1023)
    xs = [z0] * k
    for rule, param in ((W.GEOMEDIAN, 1e-6), (W.CCLIP, 0.0), (W.CCLIP, 2.0)):
        z, Dh, Bh, _ = W.round32(z0, xs, [1.0 / k] * k, rule, 3, param)
        assert np.array_equal(R.bits(z), R.bits(z0)) and not Dh.any()
        assert np.all(Bh == f32(1.0 / k)) or rule == W.GEOMEDIAN
    zz, D = W.step32(z0, xs, np.zeros(k, dtype=f32))                             # all beta zero: nothing is added at all
    assert np.array_equal(R.bits(zz), R.bits(z0))


def test_a_skipped_client_does_not_reach_the_centre():
    n, k = 1023, 5
    xs = R.spiked(n, k)                                                          # clients 0, 1, 2: NaN, +-inf, +-1e30
    z0 = W.base(n)
    beta = np.array([0, 0, 0, 0.5, 0.25], dtype=f32)
    z, D = W.step32(z0, xs, beta)
    zh, Dh = W.step32(z0, xs[3:], beta[3:])
    assert np.array_equal(R.bits(z), R.bits(zh)) and np.all(np.isfinite(z))
    assert not np.isfinite(D[0]) and not np.isfinite(D[1]) and D[2] > 1e60 and np.array_equal(D[3:], Dh)


# ---- conditioning of the rounds the GPU runs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,f", W.ROUND_CASES)
def test_rounds_are_conditioned_and_robust(n, k, f):
    """on ``krum_inputs`` (the last f clients planted outliers, one +-1e30), R = 1, 3, 8, both rules: the float32 restatement stays within
    0.25 (R + 1)(k + 3) 2^-24 max|x| of the fp64 iteration per coordinate (a step is k multiply-adds and a subtraction on top of the previous
    centre; measured at most 0.19), so the GPU test may hold the kernels to the whole bound; and the result lies within 0.02 sqrt(n) of the
    honest clients' mean while the plain mean is off by more than 1e28"""
    xs, z0, alpha = R.krum_inputs(n, k, f), W.base(n), [1.0 / k] * k
    scale = W.honest_scale(z0, xs, k - f)
    honest = np.mean([x.astype(f64) for x in xs[:k - f]], axis=0)
    plain = np.mean([x.astype(f64) for x in xs], axis=0)
    assert np.linalg.norm(plain - honest) > 1e28
    for rule, param in ((W.GEOMEDIAN, 1e-6), (W.CCLIP, 0.0)):
        for iters in W.ROUND_ITERS:
            z, Dh, Bh, tau = W.round32(z0, xs, alpha, rule, iters, param)
            z64 = W.round64(z0, xs, alpha, rule, iters, param)
            bound = (iters + 1) * (k + 3) * W.U * scale
            err = float(np.abs(z.astype(f64) - z64).max())
            print("n=%d k=%d rule=%d R=%d: error / bound %.3f" % (n, k, rule, iters, err / bound))
            assert err <= 0.25 * bound, (rule, iters, err / bound)
            assert np.all(np.isfinite(z)) and np.linalg.norm(z.astype(f64) - honest) <= 0.02 * np.sqrt(n)
            assert np.all(np.isfinite(Dh)) and Bh.shape == (iters, k)


# ---- Python surface ----------------------------------------------------------------------------------------------------------------------
def test_reweighted_aggregator_arguments():
    from fedfr_amd import server
    assert server.REWEIGHT_ALG_KINDS == {"GeoMedian", "CenteredClip"}
    assert server.ROBUST_ALG_KINDS == {"TrimmedMean", "CoordMedian", "Krum", "MultiKrum"}
    assert not server.REWEIGHT_ALG_KINDS & server.ROBUST_ALG_KINDS and not server.REWEIGHT_ALG_KINDS & set(server.AGGR_ALG_KINDS)
    A = server.ReweightedAggregator
    a = A("GeoMedian")
    assert (a.iters, a.nu, a.tau) == (3, 1e-6, None) and a.last_dist is None and a.last_weights is None and a.last_tau is None
    c = A("CenteredClip", iters=5, tau=2.5)
    assert (c.iters, c.tau) == (5, 2.5) and A("CenteredClip", tau="auto").tau is None
    for bad in ("Krum", "FedAvg", "RFA", "", None, 3):
        with pytest.raises(ValueError):
            A(bad)
    for kw in ({"iters": 0}, {"iters": -1}, {"iters": 2.5}, {"iters": True}, {"nu": 0.0}, {"nu": -1.0}, {"nu": float("inf")}, {"nu": float("nan")},
               {"tau": 0.0}, {"tau": -2.0}, {"tau": float("inf")}, {"tau": "median"}):
        with pytest.raises(ValueError):
            A("CenteredClip", **kw)
    for k in (0, 33):
        with pytest.raises(ValueError, match="GeoMedian"):
            a.validate(k)
    a.validate(1)
    a.validate(32)
    with pytest.raises(ValueError, match="sum"):
        server.fedavg_all_reduce(None, 1.0, 1.0, comm=object(), server_opt=a, prev_params=torch.zeros(8))


def test_fedreweighted_refuses_cpu_states_and_plain_dicts():
    from fedfr_amd import server
    from fedfr_amd.client import FlatStateDict
    cpu = FlatStateDict.from_flat((torch.zeros(8), torch.zeros(0), torch.zeros(0, dtype=torch.int64)), [], [])
    for kind in ("GeoMedian", "CenteredClip"):
        agg = server.ReweightedAggregator(kind)
        with pytest.raises(RuntimeError, match="GPU"):
            server.FedReweighted(cpu, [cpu] * 5, [1.0] * 5, agg)
        with pytest.raises(RuntimeError, match="FlatStateDict"):
            server.FedReweighted(cpu, [{"w": torch.zeros(8)}] * 5, [1.0] * 5, agg)
        with pytest.raises(RuntimeError, match="FlatStateDict"):
            server.FedReweighted({"w": torch.zeros(8)}, [cpu] * 5, [1.0] * 5, agg)
        with pytest.raises(RuntimeError, match="FlatStateDict"):
            server.FedReweighted(cpu, [], [], agg)
        with pytest.raises(RuntimeError, match="weights"):
            server.FedReweighted(cpu, [cpu] * 5, [1.0] * 4, agg)
        with pytest.raises(ValueError, match="32"):
            server.FedReweighted(cpu, [cpu] * 33, [1.0] * 33, agg)


def test_server_train_refuses_before_any_client_trains():
    from fedfr_amd import server

    def world(aggr, nclients, **extra):
        class Args:
            network, loss, local_epoch, output_dir, BCE_local, aggr_alg = "iresnet18", "CosFace", 1, "/tmp", False, aggr

        for k_, v_ in extra.items():
            setattr(Args, k_, v_)

        class NeverTrains:
            cid = 0

            def __getattr__(self, name):
                raise AssertionError("a client was touched (%s): the round has started" % name)

            def __setattr__(self, name, value):
                raise AssertionError("a client was touched (%s): the round has started" % name)
        return server.Server([NeverTrains() for _ in range(nclients)], None, Args, device=torch.device("cpu"))

    with pytest.raises(ValueError, match="GeoMedian, CenteredClip|CenteredClip, GeoMedian"):
        world("RFA", 3).train()                                                  # not a name; the message lists the new ones
    for aggr in ("GeoMedian", "CenteredClip"):
        with pytest.raises(ValueError, match=aggr):
            world(aggr, 33).train()
        with pytest.raises(ValueError, match=aggr):
            world(aggr, 0).train()
        # the combinations a robust rule refuses, in the same words
        for extra, words in (({"compress_bits": 8}, "a robust rule needs whole client states"),
                             ({"topk_ratio": 0.1}, "a robust rule needs whole client states"),
                             ({"secure_aggregation": True}, "a robust rule needs whole client states, which masked uploads hide"),
                             ({"dp_noise_multiplier": 1.0, "clip_norm": 1.0}, "a robust rule provides no per-client norms to clip")):
            with pytest.raises(ValueError, match=words) as e:
                world(aggr, 5, **extra).train()
            assert "aggr_alg=%r" % aggr in str(e.value)
            ref = None
            try:
                world("CoordMedian", 5, **extra).train()
            except ValueError as r:
                ref = str(r)
            assert ref is not None and ref.replace("'CoordMedian'", repr(aggr)) == str(e.value)
        for extra in (({"rfa_iters": 0}, {"rfa_nu": 0.0}) if aggr == "GeoMedian" else ({"cclip_iters": 0}, {"cclip_tau": -1.0})):
            with pytest.raises(ValueError, match="ReweightedAggregator"):
                world(aggr, 5, **extra).train()
        srv = world(aggr, 5, prox_mu=0.01, rfa_iters=2, cclip_iters=4, cclip_tau=1.5)      # prox_mu is client-side: it combines
        with pytest.raises(AssertionError, match="the round has started"):                 # a valid rule: the round starts (and meets the stub)
            srv.train()
        assert srv.reweight_agg.kind == aggr and srv.robust_agg is None
        assert srv.reweight_agg.iters == (2 if aggr == "GeoMedian" else 4)
        assert srv.reweight_agg.tau == 1.5 and srv.reweight_agg.nu == 1e-6
