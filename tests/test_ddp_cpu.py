"""Distributed differential privacy, the part that needs no GPU: the sampler's restatement of tests/ddp_cases.py (which fedfr_dgauss_fill is
held to bit for bit on the GPU) against the exact probability mass function, the sum of several clients' streams, the seeds of the GPU
tests (no ambiguous decision), privacy.DistributedDiscreteGaussian by hand, the host-side argument checks of the new C entry points, no
scratch memory in the new kernels, and what Server.train refuses before any client trains."""
import ctypes as C
import functools
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

import ddp_cases as X
import dp_cases as D
import secagg_cases as S
from conftest import REPO

f32, f64, u32, i64 = np.float32, np.float64, np.uint32, np.int64
DRAWS = 1 << 20


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from fedfr_amd import _C
    return _C


@functools.lru_cache(maxsize=None)
def draws(sigma, seed=12345, rnd=3, n=DRAWS):
    out = X.sample(n, seed, rnd, X.NOISE_STREAM, 0, sigma)
    for a in out[:3]:
        a.flags.writeable = False
    return out


def six_sigma(dof):
    return dof + 6.0 * math.sqrt(2.0 * dof)


# ---- the sampler's restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma, cells", [(16.5, None), (1000.5, 50)])
def test_restated_sampler_fits_the_exact_pmf(sigma, cells):
    """chi-square of 2^20 draws against exp(-y^2 / 2 sigma^2) / Z: one cell per integer |y| <= 4 sigma and one tail cell at sigma = 16.5,
    50 equal-probability cells at sigma = 1000.5.  Fixed seeds: deterministic (129.8 on 133 and 43.4 on 49 degrees of freedom)"""
    values, attempts, ambiguous, exhausted = draws(sigma)
    assert exhausted == 0 and attempts.min() >= 1 and not ambiguous.any()
    edges, prob = X.chi2_cells(sigma, cells)
    assert abs(prob.sum() - 1.0) < 1e-12 and prob.min() * DRAWS > 5
    if cells is not None:
        assert prob.size == cells and prob.max() / prob.min() < 1.1
    stat, dof = X.chi2(values, sigma, cells)
    print("sigma=%g: chi2 %.1f on %d dof (limit %.1f), mean attempts %.3f, worst %d, std / sigma %.5f"
          % (sigma, stat, dof, six_sigma(dof), attempts.mean(), attempts.max(), values.std() / sigma))
    assert stat < six_sigma(dof)
    assert 1.25 < attempts.mean() < 1.45 and attempts.max() <= 20 and np.abs(values).max() <= X.TAIL * (math.floor(sigma) + 1)


def test_sum_of_eight_streams_has_the_variance_of_the_mechanism(K=8, sigma=40.25, n=1 << 17):
    """K clients with seeds of their own: the sum has mean 0 and variance K var(N_Z(0, sigma^2)) within 6 standard errors, the standard
    errors from the pmf's second and fourth moments (Var S^2 = K m4 + 3 K (K - 1) var^2 - K^2 var^2)"""
    var, m4 = X.pmf_moments(sigma)
    assert abs(var / sigma ** 2 - 1.0) < 1e-9                       # (the discrete variance is sigma^2 to far below that at sigma >= 16)
    total = np.zeros(n, i64)
    for c in range(K):
        values, _, _, exhausted = X.sample(n, 0xABCDEF00 + 977 * c, 7, X.NOISE_STREAM, 0, sigma)
        assert exhausted == 0
        total += values
    se_mean = math.sqrt(K * var / n)
    se_var = math.sqrt((K * m4 + 3 * K * (K - 1) * var * var - K * K * var * var) / n)
    mean, second = float(total.mean()), float(np.mean(total.astype(f64) ** 2))
    print("mean %.4f (se %.4f), E S^2 / (K sigma^2) %.5f (se %.5f)" % (mean, se_mean, second / (K * var), se_var / (K * var)))
    assert abs(mean) < 6 * se_mean and abs(second - K * var) < 6 * se_var


def test_stream_coordinates_of_the_restatement():
    """a value depends on (seed, round, stream_id, offset + e) only: a shifted window reads the same values, every coordinate matters; the
    words of attempt a of element e are the Philox block e * 64 + a"""
    sigma = 1000.5
    base = X.sample(300, 11, 3, X.NOISE_STREAM, 0, sigma)[0]
    assert np.array_equal(X.sample(200, 11, 3, X.NOISE_STREAM, 100, sigma)[0], base[100:])
    big = X.sample(64, 11, 3, X.NOISE_STREAM, X.FILL_OFFSET, sigma)[0]
    assert np.array_equal(X.sample(32, 11, 3, X.NOISE_STREAM, X.FILL_OFFSET + 32, sigma)[0], big[32:])
    for other in (X.sample(300, 12, 3, X.NOISE_STREAM, 0, sigma), X.sample(300, 11, 4, X.NOISE_STREAM, 0, sigma), X.sample(300, 11, 3, 0, 0, sigma),
                  X.sample(300, 11 | 1 << 32, 3, X.NOISE_STREAM, 0, sigma)):
        assert np.mean(other[0] == base) < 0.05
    # element 5, first attempt, by hand from the generator of tests/dp_cases.py
    w = np.stack(D.philox4x32_10((5 * 64, 0, 3, X.NOISE_STREAM), (11, 0)), axis=1)
    ok, val, _ = X.attempt(w, sigma)
    vals, att, _, _ = X.sample(6, 11, 3, X.NOISE_STREAM, 0, sigma)
    assert (att[5] == 1) == bool(ok[0]) and (not ok[0] or vals[5] == val[0])


def test_one_attempt_at_the_edges_of_its_words():
    """U1 = 2^-53 gives the largest magnitude, floor(t 53 ln 2) <= 37 t; U1 = 1 gives G = 0, which the negative branch rejects; a proposal
    at the mode is always accepted, one far out never"""
    for sigma in (16.0, 1000.5, 2.0 ** 26):
        t = math.floor(sigma) + 1
        w = np.array([[0, 0, 1, 0], [0, 1, 1, 0], [0xFFFFFFFF, 0xFFFFF800, 0, 0], [0xFFFFFFFF, 0xFFFFF801, 0, 0]], dtype=u32)
        ok, val, _ = X.attempt(w, sigma)
        assert val[0] == math.floor(-t * math.log(2.0 ** -53)) and val[1] == -val[0] and 36 * t < val[0] <= X.TAIL * t
        assert not ok[0] and not ok[1]                              # more than 35 sigma out: p is far below U2 = 2^-32
        assert val[2] == 0 and ok[2]                                # the mode with U2 = 0: accepted
        assert val[3] == 0 and not ok[3]                            # B = 1 and G = 0: rejected whatever U2 is
    assert X.as_u32(np.array([-1, 2 ** 31, -2 ** 31 - 1], i64)).tolist() == [0xFFFFFFFF, 0x80000000, 0x7FFFFFFF]
    t, s2t, c = X.params(16.5)
    assert (t, s2t, c) == (17.0, 16.5 * 16.5 / 17.0, -1.0 / (2.0 * 16.5 * 16.5))


def test_the_seeds_of_the_gpu_tests_take_no_ambiguous_decision():
    """what tests/test_ddp_gpu.py asserts again before it compares bit for bit: with these seeds no -t log(U1) lies within 64 ulp of an
    integer and no U2 within 64 ulp of p, so a last-place difference between two log / exp implementations cannot change a value"""
    for sigma in X.FILL_SIGMAS:
        for n, off, rnd in [(max(X.FILL_SIZES), 0, X.FILL_ROUND), (4100, X.FILL_OFFSET, X.FILL_ROUND), (4100, 0, X.FILL_ROUND + 1)]:
            _, attempts, ambiguous, exhausted = X.sample(n, X.FILL_SEED, rnd, X.NOISE_STREAM, off, sigma)
            assert exhausted == 0 and not ambiguous.any(), (sigma, n, off, rnd, int(ambiguous.sum()))
    _, _, ambiguous, exhausted = X.sample(S.GRID_WRAP, X.MASK_SEED, X.MASK_ROUND, X.NOISE_STREAM, 0, X.MASK_SIGMA)
    assert exhausted == 0 and not ambiguous.any()


def test_mask_dp_restatement_on_its_own_inputs():
    """the encode half: the clip factor of every kind of input, the codes' exact squared norm, the counters, and y - noise - masks = codes"""
    n = 4100
    streams = S.some_streams(3)
    for kind in X.MASK_KINDS:
        x, xi, clip, limit = X.mask_inputs(n, kind)
        factor = X.clip_factor(x, xi, clip)
        y, sq, (sat, bad, exhausted), amb = X.mask_dp_u32(x, xi, factor, X.MASK_FRAC, limit, X.MASK_SEED, X.MASK_ROUND, 0, X.MASK_SIGMA, streams)
        q, sat0, bad0 = S.encode32(x, xi, f32(factor) * f32(2.0 ** X.MASK_FRAC), limit)
        noise = X.sample(n, X.MASK_SEED, X.MASK_ROUND, X.NOISE_STREAM, 0, X.MASK_SIGMA)[0]
        with np.errstate(over="ignore"):
            assert np.array_equal(y - S.stream_sum(n, streams) - X.as_u32(noise), q.view(u32))
        assert (sat, bad, exhausted) == (sat0, bad0, 0) and not amb.any()
        assert sq == sum(int(v) ** 2 for v in q.tolist()) % 2 ** 64
        if kind == "planted":
            assert factor == 1.0 and sat >= 2 and bad >= 3
        elif kind == "binds":
            assert 0.45 < factor < 0.55 and sat == 1 and bad == 0 and abs(int(q[1])) == limit
            assert math.sqrt(sq) <= clip * 2.0 ** X.MASK_FRAC * (1 + 2.0 ** -22) + math.sqrt(n) / 2
        else:
            assert factor == 1.0 and (sat, bad) == (0, 0)
    assert X.clip_factor(np.zeros(4, f32), np.zeros(4, f32), 1.0) == 1.0                                     # a zero norm: no division
    assert X.clip_factor(np.zeros(4, f32), np.array([np.inf, 0, 0, 0], f32), 1.0) == 0.0                     # an infinite one: 0


# ---- privacy.DistributedDiscreteGaussian --------------------------------------------------------------------------------------------------
def test_mechanism_arithmetic_by_hand():
    """z = 1, C = 1, f = 16, K = 8, T = 5, n = 10^6:
         sigma_int = 65536 / sqrt(5) = 29308.590194...      delta_int = 65536 (1 + 2^-22) + 1000 / 2 = 66036.015625
         L' = (2^31 - 1) // 8 - 37 * 29309 = 268435455 - 1084433 = 267351022      z_eff = sqrt(5) * 29308.590194 / 66036.015625 = 0.99242813..."""
    from fedfr_amd.privacy import DistributedDiscreteGaussian, RDPAccountant
    m = DistributedDiscreteGaussian(1.0, 1.0, 16, 8, 5, 10 ** 6)
    assert m.sigma_int == pytest.approx(29308.590194685, rel=1e-12)
    assert m.delta_int == 66036.015625 and m.code_limit == 267351022 and isinstance(m.code_limit, int)
    assert m.z_eff == pytest.approx(65536.0 / 66036.015625, rel=1e-12) and m.z_eff == pytest.approx(0.99242813758, rel=1e-10)
    assert m.tau == 0.0
    assert m.realised_multiplier(8) == pytest.approx(math.sqrt(8 / 5) * m.z_eff, rel=1e-15) and m.realised_multiplier(5) == m.z_eff
    acc = m.accountant()
    assert isinstance(acc, RDPAccountant) and (acc.q, acc.sigma, acc.steps) == (1.0, m.z_eff, 0)
    for rounds in (1, 5, 40):
        acc.step(rounds - acc.steps)
        assert acc.epsilon(1e-5) == pytest.approx(D.epsilon_by_hand(1.0, m.z_eff, rounds, 1e-5), rel=1e-12)
    assert m.same_as(DistributedDiscreteGaussian(1.0, 1.0, 16, 8, 5, 10 ** 6)) and not m.same_as(DistributedDiscreteGaussian(1.0, 1.0, 16, 8, 6, 10 ** 6))
    # the clamp leaves room for the largest noise value beside the largest code, K times over
    assert m.participants * (m.code_limit + X.TAIL * (math.floor(m.sigma_int) + 1)) <= 2 ** 31 - 1


def test_mechanism_refusals():
    from fedfr_amd.privacy import DistributedDiscreteGaussian as M
    with pytest.raises(ValueError, match=r"L' = -\d+ is below the sensitivity.*secagg_frac_bits in 8 \.\.\. 23 would work"):
        M(1.0, 1.0, 24, 8, 5, 10 ** 6)                               # 37 sigma_int alone passes L(8)
    with pytest.raises(ValueError, match=r"sigma_int = 4\.57947 is outside.*secagg_frac_bits in 12 \.\.\. 27 would work"):
        M(0.01, 1.0, 10, 8, 5, 10 ** 6)
    with pytest.raises(ValueError, match=r"outside the sampler's range.*secagg_frac_bits in 26 \.\.\. 30 would work"):
        M(1.0, 1e-6, 16, 8, 5, 100)
    with pytest.raises(ValueError, match=r"no secagg_frac_bits in 8 \.\.\. 30 would work"):
        M(1.0, 1e-9, 16, 8, 5, 100)
    with pytest.raises(ValueError, match=r"below the sensitivity"):
        M(1e-4, 4000.0, 16, 32, 17, 10 ** 6)                         # sigma_int in range, C 2^f itself passes L(32)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="noise_multiplier"):
            M(bad, 1.0, 16, 8, 5, 100)
        with pytest.raises(ValueError, match="clip_norm"):
            M(1.0, bad, 16, 8, 5, 100)
    for bad in (7, 31, 16.0, None):
        with pytest.raises(ValueError, match="secagg_frac_bits"):
            M(1.0, 1.0, bad, 8, 5, 100)
    for K, T, n, word in ((1, 2, 100, "participants"), (33, 2, 100, "participants"), (8, 1, 100, "threshold"), (8, 9, 100, "threshold"),
                          (8, 2.0, 100, "threshold"), (8, True, 100, "threshold"), (8, 5, 0, "n must")):
        with pytest.raises(ValueError, match=word):
            M(1.0, 1.0, 16, K, T, n)

    class Loose(M):                                                  # the smoothing term, below the sampler's range (where it is not yet 0)
        SIGMA_MIN = 0.25

    with pytest.raises(ValueError, match=r"not close to one \(tau n = "):
        Loose(1.0, 2.0 ** -17 * math.sqrt(5), 16, 8, 5, 100)         # sigma_int = 0.5: tau = 10 sum_k exp(-pi^2 k / (2 (k + 1)))
    assert Loose(1.0, 2.0 ** -14 * math.sqrt(5), 16, 8, 5, 100).tau == pytest.approx(
        10 * sum(math.exp(-2 * math.pi ** 2 * 16.0 * k / (k + 1.0)) for k in range(1, 5)), rel=1e-9)      # sigma_int = 4


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_host_side_checks_of_the_new_entry_points(built_lib):
    """what the entry points refuse, they refuse on the host before any HIP call (dummy host pointers: every call fails its checks
    first); n = 0 is a successful no-op"""
    lib = built_lib.lib()
    err_arg = int(re.search(r"#define FEDFR_ERR_ARG \((-?\d+)\)", open(os.path.join(REPO, "include", "fedfr_hip.h")).read()).group(1))
    buf = (C.c_float * 64)()
    base = C.addressof(buf)
    base += -base % 16
    keys, nonces = (C.c_uint * (8 * 33))(), (C.c_uint * (3 * 33))()
    signs = (C.c_int * 33)(*[1] * 33)

    def refused(rc, *words):
        msg = lib.fedfr_last_error_string().decode()
        assert rc == err_arg and all(w in msg for w in words), (rc, msg)

    def fill(dst=base, n=8, offset=0, sigma=100.0, exhausted=base + 64):
        return lib.fedfr_dgauss_fill(dst, n, 1, 2, 3, offset, sigma, exhausted, None)

    refused(fill(dst=None), "dgauss_fill", "dst=(nil)")
    refused(fill(exhausted=None), "dgauss_fill", "exhausted=(nil)")
    refused(fill(dst=base + 4), "dgauss_fill", "aligned")
    for bad in (15.999, 2.0 ** 26 + 1, float("nan"), -100.0, float("inf")):
        refused(fill(sigma=bad), "dgauss_fill", "sigma must be in [16, 2^26]")
    refused(fill(offset=2 ** 58), "dgauss_fill", "2^58")
    refused(fill(n=2 ** 58, offset=1), "dgauss_fill", "2^58")
    assert fill(n=0) == 0 and fill(n=0, sigma=16.0) == 0 and fill(n=0, sigma=2.0 ** 26) == 0

    def mask(y=base, x=base + 64, xi=base + 128, coef=base + 192, frac_bits=24, limit=100, offset=0, sigma=100.0, keys_=keys, nonces_=nonces,
             signs_=signs, k=2, n=8, counters=None, sqnorm=None):
        return lib.fedfr_secagg_mask_dp(y, x, xi, coef, frac_bits, limit, 1, 2, offset, sigma, keys_, nonces_, signs_, k, n, counters, sqnorm, None)

    refused(mask(y=None), "secagg_mask_dp", "y=(nil)")
    refused(mask(xi=None), "secagg_mask_dp", "xi=(nil)")
    refused(mask(coef=None), "secagg_mask_dp", "clip_coef=(nil)")
    refused(mask(frac_bits=7), "secagg_mask_dp", "frac_bits=7")
    refused(mask(frac_bits=31), "secagg_mask_dp", "frac_bits=31")
    refused(mask(limit=0), "secagg_mask_dp", "code_limit=0")
    refused(mask(limit=-3), "secagg_mask_dp", "code_limit=-3")
    refused(mask(sigma=15.0), "secagg_mask_dp", "sigma=15")
    refused(mask(sigma=2.0 ** 27), "secagg_mask_dp", "sigma must be in [16, 2^26]")
    refused(mask(sigma=float("nan")), "secagg_mask_dp", "sigma=nan")
    refused(mask(offset=2 ** 58 + 1), "secagg_mask_dp", "2^58")
    refused(mask(k=33), "secagg_mask_dp", "k=33")
    refused(mask(k=-1), "secagg_mask_dp", "k=-1")
    refused(mask(keys_=None), "secagg_mask_dp", "keys=(nil)")
    refused(mask(signs_=(C.c_int * 2)(1, 0)), "secagg_mask_dp", "sign 1 is 0")
    refused(mask(y=base + 4), "secagg_mask_dp", "aligned")
    refused(mask(counters=base + 2), "secagg_mask_dp", "counters")
    refused(mask(sqnorm=base + 4), "secagg_mask_dp", "sqnorm")
    refused(mask(n=16 * 2 ** 32 + 1), "secagg_mask_dp", "overflows")
    assert mask(n=0) == 0 and mask(n=0, k=0, keys_=None, nonces_=None, signs_=None) == 0


def test_new_kernels_use_no_scratch_memory(built_lib):
    """both kernels of csrc/ddp.hip in both builds, from the code objects' metadata (tools/kernel_resources.py): no scratch; static LDS is
    the noise strip (4 KiB per wave) and, in the mask pass, the exchange buffer and four 64-bit partial sums beside it"""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr.kernels(built_lib.LIB_PATH)
    bf16 = os.path.join(os.path.dirname(built_lib.LIB_PATH), "libfedfr_hip_bf16.so")
    if os.path.exists(bf16) and os.path.basename(built_lib.LIB_PATH) != "libfedfr_hip_bf16.so":
        ks.update({"bf16:" + k: v for k, v in kr.kernels(bf16).items()})
    builds = 2 if any(k.startswith("bf16:") for k in ks) else 1
    mine = {n: r for n, r in ks.items() if "ddp_mask_kernel" in n or "dgauss_fill_kernel" in n}
    assert len(mine) == 2 * builds, sorted(mine)
    for n, r in mine.items():
        print(n, r)
        assert r["scratch"] == 0, (n, r)
        assert r["lds"] == (16384 if "dgauss_fill_kernel" in n else 2 * 16384 + 32), (n, r)


# ---- Server.train ------------------------------------------------------------------------------------------------------------------------
def test_server_train_refuses_distributed_dp_settings_before_any_client_trains():
    from fedfr_amd import server

    class NeverTrains:
        cid = 0

        def __getattr__(self, name):
            raise AssertionError("a client was touched (%s): the round has started" % name)

        def __setattr__(self, name, value):
            raise AssertionError("a client was touched (%s): the round has started" % name)

    servers = {}

    def world(aggr, nclients=3, **extra):
        Args = type("Args", (), dict(network="iresnet18", loss="CosFace", local_epoch=1, output_dir="/tmp", BCE_local=False, aggr_alg=aggr, **extra))
        srv = servers.get(nclients)
        if srv is None:
            srv = servers[nclients] = server.Server([NeverTrains() for _ in range(nclients)], None, Args, device=torch.device("cpu"))
        srv.args, srv.robust_agg, srv.server_opt, srv.dp_accountant = Args, None, None, None
        return srv

    good = dict(distributed_dp=True, secure_aggregation=True, dp_noise_multiplier=0.01, clip_norm=1.0, secagg_frac_bits=16)
    for aggr in ("FedAvg", "FedAdam"):
        # without the switch the two refusals stand, word for word
        with pytest.raises(ValueError, match=r"secure_aggregation cannot be combined with dp_noise_multiplier=1.1: distributed differential privacy is not provided"):
            world(aggr, secure_aggregation=True, dp_noise_multiplier=1.1, clip_norm=2.0).train()
        with pytest.raises(ValueError, match=r"secure_aggregation cannot be combined with clip_norm=2.0: the clip needs per-client norms"):
            world(aggr, secure_aggregation=True, clip_norm=2.0).train()
        with pytest.raises(ValueError, match=r"secure_aggregation.*dp_noise_multiplier=1.1"):
            world(aggr, secure_aggregation=True, dp_noise_multiplier=1.1, clip_norm=2.0, distributed_dp=False).train()
        # what the switch needs
        with pytest.raises(ValueError, match=r"distributed_dp needs secure_aggregation"):
            world(aggr, **dict(good, secure_aggregation=False)).train()
        with pytest.raises(ValueError, match=r"distributed_dp needs dp_noise_multiplier > 0"):
            world(aggr, **dict(good, dp_noise_multiplier=0)).train()
        with pytest.raises(ValueError, match=r"needs clip_norm > 0"):
            world(aggr, **dict(good, clip_norm=0.0)).train()
        with pytest.raises(ValueError, match=r"distributed_dp needs dp_uniform_weights on"):
            world(aggr, dp_uniform_weights=False, **good).train()
        # what stays refused
        with pytest.raises(ValueError, match=r"compress_bits=8"):
            world(aggr, compress_bits=8, **good).train()
        with pytest.raises(ValueError, match=r"topk_ratio=0.01"):
            world(aggr, topk_ratio=0.01, **good).train()
        with pytest.raises(ValueError, match=r"return_all"):
            world(aggr, return_all=True, add_pretrained_data=True, **good).train()
        with pytest.raises(ValueError, match="secagg_threshold"):
            world(aggr, secagg_threshold=4, **good).train()
        # what the mechanism refuses, with the fraction bits that would work
        with pytest.raises(ValueError, match=r"DistributedDiscreteGaussian.*secagg_frac_bits in \d+ \.\.\. \d+ would work"):
            world(aggr, **dict(good, secagg_frac_bits=8)).train()
        with pytest.raises(ValueError, match=r"DistributedDiscreteGaussian.*below the sensitivity"):
            world(aggr, **dict(good, dp_noise_multiplier=0.05, secagg_frac_bits=30)).train()
        with pytest.raises(AssertionError, match="a client was touched"):            # a servable setting: the round starts
            world(aggr, **good).train()
        with pytest.raises(AssertionError, match="a client was touched"):
            world(aggr, secagg_drop=[2], **good).train()
    for kind in sorted(server.ROBUST_ALG_KINDS):
        with pytest.raises(ValueError, match=kind):
            world(kind, 5, **good).train()
    srv = world("FedAvg", **good)                                   # rounds of another mechanism are not composed with this one's
    from fedfr_amd.privacy import RDPAccountant
    srv.dp_accountant = RDPAccountant(0.5, 1.1)
    with pytest.raises(ValueError, match=r"the accountant composes rounds of one mechanism"):
        srv.train()


def test_fedsecaggdp_and_mask_dp_refuse_what_they_cannot_serve():
    from fedfr_amd import secagg as P, server
    from fedfr_amd.client import FlatStateDict
    from fedfr_amd.privacy import DistributedDiscreteGaussian
    mech = DistributedDiscreteGaussian(1.0, 1.0, 16, 3, 2, 8)
    cpu = FlatStateDict.from_flat((torch.zeros(8), torch.zeros(0), torch.zeros(0, dtype=torch.int64)), [], [])
    plain = P.MaskedUpdate(torch.zeros(8, dtype=torch.int32), 8, 16, torch.zeros(0), torch.zeros(0, dtype=torch.int64), torch.zeros(2, dtype=torch.int32))
    up = P.MaskedUpdate(torch.zeros(8, dtype=torch.int32), 8, 16, torch.zeros(0), torch.zeros(0, dtype=torch.int64), torch.tensor([1, 2, 3], dtype=torch.int32),
                        sqnorm=torch.tensor([-1], dtype=torch.int64))
    assert (up.saturated_count(), up.nonfinite_count(), up.exhausted_count(), up.sqnorm_value()) == (1, 2, 3, 2 ** 64 - 1)
    assert (plain.exhausted_count(), plain.sqnorm_value()) == (0, None)
    with pytest.raises(RuntimeError, match="FlatStateDict"):
        server.FedSecAggDP({"w": torch.zeros(8)}, [up, up], [], mech)
    with pytest.raises(RuntimeError, match="DistributedDiscreteGaussian"):
        server.FedSecAggDP(cpu, [up, up], [], None)
    with pytest.raises(RuntimeError, match="mask_dp"):
        server.FedSecAggDP(cpu, [up, plain], [], mech)
    with pytest.raises(ValueError, match=r"1 uploads, the mechanism needs 2 to 3"):
        server.FedSecAggDP(cpu, [up], [], mech)
    with pytest.raises(ValueError, match="clip_norm"):
        server.FedSecAggDP(cpu, [up, up], [], mech, server.ServerOptimizer("ADAM", clip_norm=1.0))
    with pytest.raises(ValueError, match="robust"):
        server.FedSecAggDP(cpu, [up, up], [], mech, server.RobustAggregator("Krum"))
    with pytest.raises(RuntimeError, match="GPU"):
        server.FedSecAggDP(cpu, [up, up], [], mech)
    with pytest.raises(RuntimeError, match="FlatStateDict"):
        P.SecAggClient(0, 16).mask_dp({"w": 1}, cpu, [0, 1, 2], {}, 0, mech)
    with pytest.raises(RuntimeError, match="DistributedDiscreteGaussian"):
        P.SecAggClient(0, 16).mask_dp(cpu, cpu, [0, 1, 2], {}, 0, None)
