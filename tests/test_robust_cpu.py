"""Robust aggregation (trimmed mean / median, Krum / Multi-Krum), the part that needs no GPU: the C ABI carries the new entry points, no
``robust_`` kernel uses scratch memory, the restatements of tests/robust_cases.py obey the laws the rules define, the Krum inputs are
conditioned so that the selection on the GPU is a condition and not a measurement, and the Python surface validates its arguments."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import robust_cases as R
from conftest import REPO

f32, f64 = np.float32, np.float64
NEW_SYMBOLS = ("fedfr_robust_trimmed_mean", "fedfr_robust_pairdist_workspace_bytes", "fedfr_robust_pairdist", "fedfr_robust_krum_select")


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from fedfr_amd import _C
    return _C


def test_header_ctypes_table_and_library_carry_the_robust_symbols(built_lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "fedfr_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fedfr_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\sT\s+(fedfr_[a-z0-9_]+)", out))
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in built_lib.SIGNATURES, s
        assert s in exported, s
    lib = built_lib.lib()
    # the workspace query is host code: [k (k - 1) / 2][grid] doubles with fedavg_multi's grid rule, 0 for arguments the kernel refuses
    for n in R.SIZES:
        for k in R.KS_DIST:
            assert lib.fedfr_robust_pairdist_workspace_bytes(k, n) == 8 * (k * (k - 1) // 2) * R.grid(n), (k, n)
    assert R.grid(R.BIG) == R.GRID_CAP and R.grid(4103) == 5
    for k, n in ((0, 100), (1, 100), (33, 100), (3, 0)):
        assert lib.fedfr_robust_pairdist_workspace_bytes(k, n) == 0


def test_robust_kernels_use_no_scratch_memory(built_lib):
    """every ``robust_`` kernel (K = 1..32 trimmed means, the 12 + 8 pair tiles, the two single-block kernels; both storage builds): the sort is a
    compile-time network on registers and the accumulators are registers, so scratch memory would mean an array indexed at run time"""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr.kernels(built_lib.LIB_PATH)
    bf16 = os.path.join(os.path.dirname(built_lib.LIB_PATH), "libfedfr_hip_bf16.so")
    if os.path.exists(bf16) and os.path.basename(built_lib.LIB_PATH) != "libfedfr_hip_bf16.so":
        ks.update({"bf16:" + k: v for k, v in kr.kernels(bf16).items()})
    builds = 2 if any(k.startswith("bf16:") for k in ks) else 1
    rob = {n: r for n, r in ks.items() if "robust_" in n}
    tm = [n for n in rob if "robust_trimmed_mean_kernel" in n]
    pd = [n for n in rob if "robust_pairdist_kernel" in n]
    assert len(tm) == 32 * builds and len(pd) == 20 * builds, (len(tm), len(pd))
    assert sum("robust_krum_select_kernel" in n for n in rob) == builds and sum("robust_pairdist_final_kernel" in n for n in rob) == builds
    bad = [(n, r) for n, r in rob.items() if r["scratch"]]
    assert not bad, bad


def test_sorting_networks_sort(tmp_path):
    """the compile-time compare-exchange networks of csrc/robust_net.h, K = 1 .. 32, under the 0-1 principle (tools/sort_network_check.cpp:
    every 0-1 sequence to K = 16, 2^18 random ones above), compiled for the host from the very header the kernel includes"""
    import shutil
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "hipcc"
    exe = str(tmp_path / "sort_network_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", os.path.join(REPO, "fedfr_amd", "csrc"), os.path.join(REPO, "tools", "sort_network_check.cpp"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 32 and all(l.endswith("bad=0") for l in lines)
    n_ex = {int(l.split()[0][2:]): int(l.split()[1].split("=")[1]) for l in lines}
    assert (n_ex[1], n_ex[2], n_ex[8], n_ex[16], n_ex[32]) == (0, 1, 19, 63, 191)


# ---- laws of the trimmed-mean restatement ------------------------------------------------------------------------------------------------
def test_key_is_the_documented_total_order():
    v = np.array([-np.inf, -1e30, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 1e30, np.inf], dtype=f32)
    k = R.key(v)
    assert np.all(k[1:] > k[:-1])                                            # strictly ascending, -0 < +0, the infinities at the ends
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32).view(f32)
    assert np.all(R.key(nans) == 0xFFFFFFFF) and np.all(k < 0xFFFFFFFF)      # every NaN, either sign: last


@pytest.mark.parametrize("k", R.KS_TRIM)
def test_restatement_against_fp64(k):
    """within (k + 2) 2^-24 sum |kept| of the fp64 trimmed mean, on the finite inputs and every b of the GPU tests"""
    worst = 0.0
    for n in R.SIZES[:-1]:
        xs = R.inputs(n, k)
        for b in R.trims(k):
            got = R.trimmed32(xs, b)
            mean, mag = R.trimmed64(xs, b)
            bound = (k + 2) * R.U * mag
            err = np.abs(got.astype(f64) - mean)
            assert np.all(err <= bound), (k, n, b, float(np.max(err / bound)))
            worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
    print("k=%d: worst error / bound %.3f" % (k, worst))


@pytest.mark.parametrize("k", [2, 3, 5, 8, 9, 17])
def test_restatement_is_invariant_under_client_permutation(k):
    """bit for bit, the +-0 coordinates included: the order is total on bit patterns, so equal keys are equal values"""
    n = 1023
    rng = np.random.RandomState(7)
    cases = [R.inputs(n, k), R.signed_zeros(n, k)] + ([R.spiked(n, k)] if k >= 5 else [])
    for xs in cases:
        for b in R.trims(k):
            ref = R.trimmed32(xs, b)
            for _ in range(3):
                perm = rng.permutation(k)
                got = R.trimmed32([xs[i] for i in perm], b)
                assert R.same_bits_or_nan(got, ref).size == 0
    z = R.trimmed32(R.signed_zeros(n, k), 0)
    assert np.all(z == 0.0) and (k == 1 or len(set(R.bits(z).tolist())) == 2)      # both zeros occur as results


@pytest.mark.parametrize("k", [1, 2, 3, 8, 17])
def test_equal_clients_without_trimming_return_the_client(k):
    x = R.inputs(4103, 1)[0]
    q = (np.round(x * 1024) / 1024).astype(f32)             # dyadic values: every partial sum j q is exact for any k <= 32
    assert np.array_equal(R.trimmed32([q] * k, 0), q)
    for b in R.trims(k):                                    # and with trimming: the kept ones are the client as well
        assert np.array_equal(R.trimmed32([q] * k, b), q)


@pytest.mark.parametrize("k,c", [(3, 1), (5, 1), (5, 2), (9, 3), (17, 8), (32, 4)])
def test_nan_clients_up_to_the_trim_are_trimmed(k, c):
    """c <= b clients send NaN: they sort last and fall to the upper trim; the result is finite and is the restatement of the honest k - c
    clients with b dropped below and b - c above (the same kept set, so the same additions)"""
    n = 1023
    honest = list(R.inputs(n, k))[c:]
    nan = np.full(n, np.nan, dtype=f32)
    for b in sorted({c, (k - 1) // 2}):
        xs = [nan] * c + honest
        got = R.trimmed32(xs, b)
        assert np.all(np.isfinite(got))
        assert np.array_equal(R.bits(got), R.bits(R.trimmed32(honest, b, b - c)))
    over = R.trimmed32([nan] * c + honest, c - 1)           # one NaN more than the trim: it is kept, and shows
    assert np.all(np.isnan(over))


# ---- the Krum reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,f,m", R.KRUM_CASES)
def test_krum_ref_rejects_the_planted_outliers_and_the_cases_are_conditioned(n, k, f, m):
    """the last f clients of ``krum_inputs`` are outliers: never selected.  And the m-th and the (m+1)-th lowest score are at least 10^6
    distance bounds (n 2^-52, relative to the larger score: a score is a sum of k - f - 2 distances, each within that bound) apart, so the
    kernel's distances — any summation order — give the same selection: on the GPU the selection is asserted exactly."""
    xs = R.krum_inputs(n, k, f)
    D = R.pairdist64(xs)
    assert np.array_equal(D, D.T) and np.all(np.diag(D) == 0) and np.all(np.isfinite(D))
    score, sel = R.krum_ref(D, f, m)
    assert sel.sum() == m and not sel[k - f:].any()
    assert np.all(score[k - f:] > score[:k - f].max())
    gap, hi = R.score_gap(score, m)
    print("n=%d k=%d f=%d m=%d: gap / score %.3e, needed %.3e" % (n, k, f, m, gap / hi, 1e6 * n * 2.0 ** -52))
    assert gap >= 1e6 * n * 2.0 ** -52 * hi


def test_krum_ref_ties_and_non_finite_rows():
    D = np.array([[0, 1, 1, 9, 9], [1, 0, 1, 9, 9], [1, 1, 0, 9, 9], [9, 9, 9, 0, 1], [9, 9, 9, 1, 0]], dtype=f64)
    score, sel = R.krum_ref(D, 1, 1)                         # k - f - 2 = 2 neighbours: clients 0, 1, 2 tie at 2.0
    assert score.tolist() == [2.0, 2.0, 2.0, 10.0, 10.0] and sel.tolist() == [1, 0, 0, 0, 0]
    assert R.krum_ref(D, 1, 2)[1].tolist() == [1, 1, 0, 0, 0]
    E = D.copy()
    E[0, :] = E[:, 0] = np.nan                               # client 0 sent NaN: its row and column are not finite
    E[0, 0] = 0.0
    score, sel = R.krum_ref(E, 1, 4)
    assert np.isinf(score[0]) and sel.tolist() == [0, 1, 1, 1, 1]


# ---- Python surface ----------------------------------------------------------------------------------------------------------------------
def test_robust_aggregator_counts_and_errors():
    from fedfr_amd import server
    assert server.ROBUST_ALG_KINDS == {"TrimmedMean", "CoordMedian", "Krum", "MultiKrum"}
    assert sorted(server.AGGR_ALG_KINDS) == ["FedAdagrad", "FedAdam", "FedAvgM", "FedYogi"]
    assert not server.ROBUST_ALG_KINDS & set(server.AGGR_ALG_KINDS)
    A = server.RobustAggregator
    assert [A("TrimmedMean").trim_count(k) for k in (3, 9, 10, 20, 32)] == [0, 0, 1, 2, 3]      # floor(0.1 k)
    assert A("TrimmedMean", trim_ratio=0.25).trim_count(9) == 2 and A("TrimmedMean", trim=3).trim_count(9) == 3
    assert [A("CoordMedian", trim=0, trim_ratio=0.0).trim_count(k) for k in (1, 2, 3, 8, 9)] == [0, 0, 1, 3, 4]
    assert A("Krum").select_count(9) == 1 and A("MultiKrum", num_byzantine=2).select_count(9) == 7
    assert A("MultiKrum", multi_m=3).select_count(9) == 3
    a = A("Krum")
    assert a.last_selected is None and a.last_scores is None and a.last_dist is None
    for bad in ("FedMedian", "Median", "FedAvg", "FedAdam", "", None, 3):
        with pytest.raises(ValueError):
            A(bad)
    for kw in ({"trim_ratio": 0.5}, {"trim_ratio": -0.1}, {"trim": -1}, {"num_byzantine": -1}, {"multi_m": 0}):
        with pytest.raises(ValueError):
            A("TrimmedMean", **kw)
    for agg, k in ((A("TrimmedMean", trim=2), 4), (A("TrimmedMean", trim=1), 2), (A("CoordMedian"), 33), (A("TrimmedMean"), 33),
                   (A("Krum"), 4), (A("Krum", num_byzantine=3), 8), (A("MultiKrum"), 33), (A("MultiKrum", multi_m=5), 5),
                   (A("MultiKrum", num_byzantine=0, multi_m=4), 3), (A("CoordMedian"), 0)):
        with pytest.raises(ValueError, match=agg.kind):
            agg.validate(k)
    for agg, k in ((A("TrimmedMean", trim=2), 5), (A("CoordMedian"), 1), (A("CoordMedian"), 32), (A("Krum"), 5), (A("Krum", num_byzantine=0), 3),
                   (A("MultiKrum", num_byzantine=7), 32), (A("MultiKrum", multi_m=4), 5)):
        agg.validate(k)


def test_fedrobust_refuses_cpu_states_and_plain_dicts():
    from fedfr_amd import server
    from fedfr_amd.client import FlatStateDict
    cpu = FlatStateDict.from_flat((torch.zeros(8), torch.zeros(0), torch.zeros(0, dtype=torch.int64)), [], [])
    for kind in ("CoordMedian", "MultiKrum"):
        agg = server.RobustAggregator(kind)
        with pytest.raises(RuntimeError, match="GPU"):
            server.FedRobust([cpu] * 5, [1.0] * 5, agg)                       # FlatStateDicts, but not on the GPU
        with pytest.raises(RuntimeError, match="FlatStateDict"):
            server.FedRobust([{"w": torch.zeros(8)}] * 5, [1.0] * 5, agg)
        with pytest.raises(RuntimeError, match="FlatStateDict"):
            server.FedRobust([], [], agg)
        with pytest.raises(RuntimeError, match="weights"):
            server.FedRobust([cpu] * 5, [1.0] * 4, agg)
    with pytest.raises(ValueError, match="Krum"):
        server.FedRobust([cpu] * 4, [1.0] * 4, server.RobustAggregator("Krum"))              # k < 2 f + 3
    with pytest.raises(ValueError, match="TrimmedMean"):
        server.FedRobust([cpu] * 4, [1.0] * 4, server.RobustAggregator("TrimmedMean", trim=2))
    with pytest.raises(ValueError, match="32"):
        server.FedRobust([cpu] * 33, [1.0] * 33, server.RobustAggregator("CoordMedian"))
    with pytest.raises(ValueError, match="sum"):
        server.fedavg_all_reduce(None, 1.0, 1.0, comm=object(), server_opt=server.RobustAggregator("CoordMedian"), prev_params=torch.zeros(8))


def test_server_train_validates_the_rule_before_any_client_trains():
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

    with pytest.raises(ValueError, match="FedMedian"):
        world("FedMedian", 3).train()                                            # still not a name the server knows
    with pytest.raises(ValueError, match="Krum"):
        world("Krum", 4).train()                                                 # k < 2 f + 3 at the default f = 1
    with pytest.raises(ValueError, match="MultiKrum"):
        world("MultiKrum", 6, num_byzantine=2).train()
    with pytest.raises(ValueError, match="MultiKrum"):
        world("MultiKrum", 5, multi_krum_m=5).train()
    with pytest.raises(ValueError, match="TrimmedMean"):
        world("TrimmedMean", 33).train()
    with pytest.raises(ValueError, match="CoordMedian"):
        world("CoordMedian", 0).train()
    srv = world("TrimmedMean", 10, trim_ratio=0.2)
    with pytest.raises(AssertionError, match="the round has started"):                 # a valid rule: the round starts (and meets the stub)
        srv.train()
    assert srv.robust_agg.kind == "TrimmedMean" and srv.robust_agg.trim_count(10) == 2
