"""Distributed differential privacy at 16-bit narrow words without a GPU: privacy.DistributedDiscreteGaussian(bits=16, wrap_sigmas=...) by
hand and what it refuses, the restatement of tests/ddp_narrow_cases.py against the restatements it is built from (the narrow pass when the
noise is taken away, the sensitivity bound, the rotation's norm bound, the noise on the padding), the seeds of the GPU tests (no ambiguous
decision), what Server.train and SecAggClient.mask_dp refuse before any client trains, and the host-side checks of the new C entry point."""
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
import ddp_narrow_cases as W
import secagg_cases as S
import secagg_narrow_cases as N
from conftest import REPO

f32, f64, u32, i32, i64 = np.float32, np.float64, np.uint32, np.int32, np.int64


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from fedfr_amd import _C
    return _C


@functools.lru_cache(maxsize=None)
def noise(n_pad, seed, rnd, offset, sigma):
    z, amb, exhausted = W.noise(n_pad, seed, rnd, offset, sigma)
    z.flags.writeable = False
    return z, int(amb.sum()), exhausted


# ---- privacy.DistributedDiscreteGaussian at 16 bits ---------------------------------------------------------------------------------------
def test_mechanism_at_16_bits_by_hand():
    """z = 1, C = 1, f = 10, K = 4, T = 3, n = 5000, kappa = 7:
         n_pad = 8192      sigma_int = 1024 / sqrt(3) = 591.2067      delta_int = 1024 (1 + 2^-22) (1 + 13 2^-24) + sqrt(8192)
         code_limit = (32767 - ceil(7 * 591.2067 * 2)) // 4 = (32767 - 8277) // 4 = 6122      z_eff = 1024 / delta_int = 0.9188
         wrap_bound = 8192 * 2 exp(-24.5) = 3.75e-7      coordinate_sigmas = 64 * 6122 / 1024
       and at the size of iresnet100 (n_pad = 65 003 520, K = T = 8, f = 12): code_limit 511, z_eff 0.337, 8.0 sigmas, wrap_bound 3.0e-3"""
    from fedfr_amd.privacy import DistributedDiscreteGaussian as M, RDPAccountant
    m = M(1.0, 1.0, 10, 4, 3, 5000, bits=16, wrap_sigmas=7)
    delta = 1024.0 * (1 + 2.0 ** -22) * (1 + 13 * 2.0 ** -24) + math.sqrt(8192.0)
    assert (m.bits, m.wrap_sigmas, m.n, m.n_pad) == (16, 7.0, 5000, 8192) and M.EPS_ROT == 13 * 2.0 ** -24
    assert m.sigma_int == pytest.approx(1024.0 / math.sqrt(3.0), rel=1e-9) and m.sigma_int == pytest.approx(591.2067, rel=1e-6)
    assert m.delta_int == pytest.approx(delta, rel=1e-9) and m.delta_int == pytest.approx(W.delta_int(1.0, 10, 5000), rel=1e-12)
    assert m.code_limit == 6122 and isinstance(m.code_limit, int)
    assert m.z_eff == pytest.approx(1024.0 / delta, rel=1e-9) and m.z_eff == pytest.approx(0.9188, rel=1e-4)
    assert m.wrap_bound == pytest.approx(8192 * 2.0 * math.exp(-24.5), rel=1e-9) and m.wrap_bound == pytest.approx(3.75e-7, rel=1e-3)
    assert m.coordinate_sigmas == pytest.approx(64 * 6122 / 1024.0, rel=1e-9) and m.tau == 0.0
    # the headroom: K clamped codes and kappa standard deviations of the sum of K noises stay inside a field
    assert m.participants * m.code_limit + math.ceil(7 * m.sigma_int * 2) <= 32767
    acc = m.accountant()
    assert isinstance(acc, RDPAccountant) and (acc.q, acc.sigma) == (1.0, m.z_eff)
    big = M(1.0, 1.0, 12, 8, 8, 65003520, bits=16, wrap_sigmas=7)
    assert (big.n_pad, big.code_limit) == (65003520, 511) and M(1.0, 1.0, 12, 8, 8, 65003520 - 4095, bits=16, wrap_sigmas=7).n_pad == 65003520
    assert big.z_eff == pytest.approx(0.337, rel=2e-3) and big.coordinate_sigmas == pytest.approx(8.0, rel=2e-3)
    assert big.wrap_bound == pytest.approx(3.0e-3, rel=1e-2)
    # same_as compares the two new fields too
    assert m.same_as(M(1.0, 1.0, 10, 4, 3, 5000, bits=16, wrap_sigmas=7.0))
    assert not m.same_as(M(1.0, 1.0, 10, 4, 3, 5000, bits=16, wrap_sigmas=6)) and not m.same_as(M(1.0, 1.0, 10, 4, 3, 5000))
    assert not M(1.0, 1.0, 10, 4, 3, 5000).same_as(m)


def test_mechanism_refusals_at_16_bits():
    from fedfr_amd.privacy import DistributedDiscreteGaussian as M
    # C 2^f = 16: sigma_int = 16 / sqrt(3); 2^5 ... 2^11 give a sigma_int >= 16 whose headroom 7 x 2 sigma_int leaves a code
    with pytest.raises(ValueError, match=r"sigma_int = 9\.2376 is outside the sampler's range.*bits=16, wrap_sigmas=7\): secagg_frac_bits in 11 \.\.\. 17 would work"):
        M(1.0, 2.0 ** -6, 10, 4, 3, 5000, bits=16, wrap_sigmas=7)
    with pytest.raises(ValueError, match=r"the code clamp .* = -\d+ is below 1.*secagg_frac_bits in 8 \.\.\. 11 would work"):
        M(1.0, 1.0, 20, 4, 3, 5000, bits=16, wrap_sigmas=7)
    edge = 32765.0 / (2 * 4096 / math.sqrt(3))                       # the headroom is 32765 or 32766: one or two values are left for K = 4 codes
    with pytest.raises(ValueError, match=r"the code clamp .* = 0 is below 1"):
        M(1.0, 1.0, 12, 4, 3, 5000, bits=16, wrap_sigmas=edge)
    with pytest.raises(ValueError, match=r"no secagg_frac_bits in 8 \.\.\. 30 would work"):
        M(1.0, 1.0, 12, 4, 3, 5000, bits=16, wrap_sigmas=4000)

    class Loose(M):                                                  # the smoothing term, below the sampler's range (where it is not yet 0)
        SIGMA_MIN = 0.25

    with pytest.raises(ValueError, match=r"not close to one \(tau n = "):
        Loose(1.0, 2.0 ** -11 * math.sqrt(3), 10, 4, 3, 5000, bits=16, wrap_sigmas=7)      # sigma_int = 0.5
    with pytest.raises(ValueError, match=r"8-bit words cannot carry.*smallest sigma_int, 16.*\+-127"):
        M(1.0, 1.0, 10, 4, 3, 5000, bits=8, wrap_sigmas=7)
    with pytest.raises(ValueError, match=r"8-bit words cannot carry"):
        M(1.0, 1.0, 10, 4, 3, 5000, bits=8)
    with pytest.raises(ValueError, match=r"16-bit words need wrap_sigmas"):
        M(1.0, 1.0, 10, 4, 3, 5000, bits=16)
    with pytest.raises(ValueError, match=r"wrap_sigmas=7 belongs to 16-bit words.*nothing wraps"):
        M(1.0, 1.0, 16, 4, 3, 5000, wrap_sigmas=7)
    with pytest.raises(ValueError, match=r"wrap_sigmas=7 belongs to 16-bit words"):
        M(1.0, 1.0, 16, 4, 3, 5000, bits=32, wrap_sigmas=7)
    for bad in (0.999, 0, -7, float("nan"), float("inf"), "7", True):
        with pytest.raises(ValueError, match="wrap_sigmas must be a finite number >= 1"):
            M(1.0, 1.0, 10, 4, 3, 5000, bits=16, wrap_sigmas=bad)
    for bad in (4, 12, 64, 16.0, "16"):
        with pytest.raises(ValueError, match="secagg_bits must be 8, 16 or 32"):
            M(1.0, 1.0, 10, 4, 3, 5000, bits=bad, wrap_sigmas=7)
    assert M(1.0, 1.0, 10, 4, 3, 5000, bits=16, wrap_sigmas=1).code_limit == (32767 - math.ceil(1024 / math.sqrt(3) * 2)) // 4


@pytest.mark.parametrize("z, C_, f, K, T, n", [(1.0, 1.0, 16, 8, 5, 10 ** 6), (0.005, 1.0, 16, 3, 2, 4321), (1.1, 0.1, 20, 32, 17, 65 * 10 ** 6)])
def test_mechanism_at_32_bits_is_todays(z, C_, f, K, T, n):
    """bits=32 (the default): the formulas of the 32-bit mechanism, restated here; the new attributes say that nothing wraps"""
    from fedfr_amd.privacy import DistributedDiscreteGaussian as M
    for m in (M(z, C_, f, K, T, n), M(z, C_, f, K, T, n, bits=32), M(z, C_, f, K, T, n, 32, None)):
        scale = C_ * 2.0 ** f
        sigma = z * scale / math.sqrt(T)
        delta = scale * (1 + 2.0 ** -22) + math.sqrt(n) / 2
        assert (m.sigma_int, m.delta_int, m.z_eff, m.tau) == (sigma, delta, math.sqrt(T) * sigma / delta, 0.0)
        assert m.code_limit == (2 ** 31 - 1) // K - 37 * (math.floor(sigma) + 1)
        assert (m.bits, m.wrap_sigmas, m.wrap_bound, m.coordinate_sigmas, m.n_pad) == (32, None, 0.0, None, n)
    with pytest.raises(ValueError, match=r"L' = -\d+ is below the sensitivity.*n=1000000\): secagg_frac_bits in 8 \.\.\. 23 would work"):
        M(1.0, 1.0, 24, 8, 5, 10 ** 6)                               # (the message of the 32-bit refusal, word for word)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def case(n, kind, k=3, offset=0):
    x, xi, clip, limit, sigma = W.inputs(n, kind)
    factor = X.clip_factor(x, xi, clip)
    streams = S.some_streams(k)
    y, sq, counts, amb = W.mask_narrow_dp(x, xi, factor, W.FRAC, limit, W.ROT_SEED, W.PRIV_SEED, W.RND, W.NOISE_SEED, W.NOISE_ROUND, offset, sigma, streams)
    return x, xi, factor, limit, sigma, streams, y, sq, counts, amb


@pytest.mark.parametrize("kind", W.KINDS)
@pytest.mark.parametrize("n", W.SIZES)
def test_inputs_of_the_gpu_tests_have_no_ambiguous_decision_and_are_what_they_say(n, kind):
    x, xi, factor, limit, sigma, streams, y, sq, (sat, bad, exhausted), amb = case(n, kind)
    npad = N.padded_count(n)
    assert not amb.any() and exhausted == 0 and y.dtype == u32 and y.size == npad // 2
    for seed, rnd, off in ((W.NOISE_SEED, W.NOISE_ROUND, W.NOISE_OFFSET), (W.NOISE_SEED, W.NOISE_ROUND + 1, 0), (W.NOISE_SEED + 1, W.NOISE_ROUND, 0)):
        assert noise(npad, seed, rnd, off, sigma)[1:] == (0, 0)      # the stream coordinates of the GPU tests
    if kind == "binds":
        assert 0.4 < factor < 0.6 and sat >= N.BLOCK // 2 and bad == 0      # +-16 and an ordinary part of about +-2 against the limit 12
    elif kind == "free":
        assert factor == 1.0 and (sat, bad) == (0, 0) and sq > 0
    elif kind == "zero":
        assert factor == 1.0 and (sat, bad, sq) == (0, 0, 0)
    else:
        kinds = {N.KINDS[(b + W.SIZES.index(n) + 2) % 5] for b in range(npad // N.BLOCK)}
        assert factor == (0.0 if n == 1 else 1.0)                    # n = 1 is +inf: the norm is infinite, the factor 0, every product NaN
        assert bad == (N.BLOCK if "nonfinite" in kinds else 0) and (sat >= N.BLOCK) == ("saturating" in kinds)
    assert {N.KINDS[(b + i + 2) % 5] for i, m in enumerate(W.SIZES) for b in range(N.padded_count(m) // N.BLOCK)} == set(N.KINDS)


@pytest.mark.parametrize("kind", W.KINDS)
@pytest.mark.parametrize("n", W.SIZES)
def test_restatement_minus_its_noise_is_the_narrow_pass(n, kind, K=5):
    """at code_limit = (2^15 - 1) // K the words, field-minus the packed noise, are secagg_narrow_cases.mask_narrow's for the same seeds and
    streams; so are the counters"""
    x, xi, clip, _, sigma = W.inputs(n, kind)
    factor, streams, limit = X.clip_factor(x, xi, clip), S.some_streams(3), N.code_limit(K, 16)
    y, sq, (sat, bad, exhausted), _ = W.mask_narrow_dp(x, xi, factor, W.FRAC, limit, W.ROT_SEED, W.PRIV_SEED, W.RND, W.NOISE_SEED, W.NOISE_ROUND, 0, sigma,
                                                       streams, counter0=9)
    z = noise(N.padded_count(n), W.NOISE_SEED, W.NOISE_ROUND, 0, sigma)[0]
    ref, rsat, rbad, q = N.mask_narrow(x, xi, factor * f32(2.0 ** W.FRAC), K, 16, W.ROT_SEED, W.PRIV_SEED, W.RND, streams, counter0=9)
    assert np.array_equal(N.field_sub(y, N.pack(z, 16), 16), ref) and (sat, bad, exhausted) == (rsat, rbad, 0)
    assert sq == int(np.sum(q.astype(i64) ** 2)) and np.abs(z).max() < 2 ** 15


@pytest.mark.parametrize("n", W.SIZES)
def test_sensitivity_bound_holds_where_the_clip_binds(n):
    """sq <= delta_int^2 = (C 2^f (1 + EPS_FP) (1 + EPS_ROT) + sqrt(n_pad))^2 for the 'binds' inputs: at the case's own clamp, and with the
    clamp out of the way (the bound is the norm's, not the clamp's); and the clip does bind: the codes have at least the norm C 2^f less
    the rounding"""
    from fedfr_amd.privacy import DistributedDiscreteGaussian as M
    x, xi, clip, limit, _ = W.inputs(n, "binds")
    mech = M(1.0, clip, W.FRAC, 2, 2, n, bits=16, wrap_sigmas=1)
    assert mech.delta_int == pytest.approx(W.delta_int(clip, W.FRAC, n), rel=1e-12)
    factor = X.clip_factor(x, xi, clip)
    for f in (factor, np.nextafter(factor, f32(1)), np.nextafter(np.nextafter(factor, f32(1)), f32(1))):      # the device's factor: within 2 ulp
        for L in (limit, 32767):
            q = W.codes(x, xi, f, W.FRAC, L, W.ROT_SEED, W.PRIV_SEED, W.RND)[0]
            sq = int(np.sum(q.astype(i64) ** 2))
            assert sq == X._sq_mod64(q) and sq <= mech.delta_int ** 2, (n, L, sq, mech.delta_int ** 2)
    assert math.sqrt(sq) >= clip * 2.0 ** W.FRAC - math.sqrt(N.padded_count(n))


def test_rotation_grows_the_norm_by_less_than_eps_rot():
    """||rotate32(u)|| <= (1 + EPS_ROT) ||u|| block by block, the norms in float64, against the exact rotation rotate64 (which keeps the norm
    to float64's rounding): one-hot, constant, alternating-sign and large-dynamic-range blocks, and random ones"""
    from fedfr_amd.privacy import DistributedDiscreteGaussian as M
    g = np.random.default_rng(5)
    B = N.BLOCK
    blocks = [np.eye(1, B, 0)[0] * 3.3, np.eye(1, B, B - 1)[0] * -1e-3, np.full(B, 0.7), np.where(np.arange(B) % 2, -1.1, 1.1),
              g.standard_normal(B) * np.exp(8 * g.standard_normal(B)), g.standard_normal(B) * 10.0 ** g.integers(-12, 12, B),
              g.standard_normal(B), g.standard_normal(B) * 1e-3, np.full(B, 1 / 3.0) * np.sign(g.standard_normal(B))]
    u = np.concatenate(blocks).astype(f32)
    for seed, rnd in ((W.ROT_SEED, W.RND), (1, 2), (0, 0)):
        v32, v64 = N.rotate32(u, seed, rnd).astype(f64).reshape(-1, B), N.rotate64(u, seed, rnd).reshape(-1, B)
        n0 = np.sqrt((u.astype(f64).reshape(-1, B) ** 2).sum(axis=1))
        n32, n64 = np.sqrt((v32 ** 2).sum(axis=1)), np.sqrt((v64 ** 2).sum(axis=1))
        assert np.all(np.abs(n64 - n0) <= 1e-13 * n0)                # the rotation is orthogonal
        assert np.all(n32 <= (1 + M.EPS_ROT) * n0), (n32 / n0 - 1).max() / 2.0 ** -24
        assert np.all(np.abs(n32 - n0) <= M.EPS_ROT * n0)            # (and it does not shrink it by more either)
    assert M.EPS_ROT == W.EPS_ROT and M.EPS_FP == W.EPS_FP


def test_padding_coordinates_carry_noise(n=1):
    """n = 1: every one of the 4096 fields of the padded block differs from the noiseless one exactly by the low 16 bits of the stream's
    value at its position; with a zero update the fields ARE those low bits"""
    x, xi, clip, limit, sigma = W.inputs(n, "free")
    args = (W.FRAC, limit, W.ROT_SEED, W.PRIV_SEED, W.RND, W.NOISE_SEED, W.NOISE_ROUND, 0, sigma)
    y, _, _, amb = W.mask_narrow_dp(x, xi, f32(1), *args, [])
    q = W.codes(x, xi, f32(1), W.FRAC, limit, W.ROT_SEED, W.PRIV_SEED, W.RND)[0]
    z = noise(N.BLOCK, W.NOISE_SEED, W.NOISE_ROUND, 0, sigma)[0]
    assert y.size == N.BLOCK // 2 and not amb.any() and np.count_nonzero(q) > 0
    diff = (N.unpack(y, 16) - q) & 0xFFFF
    assert np.array_equal(diff, z & 0xFFFF) and np.count_nonzero(z) > 0.9 * N.BLOCK and np.count_nonzero(z[1:]) > 0.9 * N.BLOCK
    y0 = W.mask_narrow_dp(x, x, f32(1), *args, [])[0]
    assert np.array_equal(N.unpack(y0, 16) & 0xFFFF, z & 0xFFFF)


# ---- Server.train, SecAggClient.mask_dp, FedSecAggDP ----------------------------------------------------------------------------------------
def test_server_train_refuses_ddp_wrap_sigmas_settings_before_any_client_trains():
    from fedfr_amd import server

    class NeverTrains:
        cid = 0

        def __getattr__(self, name):
            raise AssertionError("a client was touched (%s): the round has started" % name)

        def __setattr__(self, name, value):
            raise AssertionError("a client was touched (%s): the round has started" % name)

    srv = None

    def world(aggr, **extra):
        nonlocal srv
        Args = type("Args", (), dict(network="iresnet18", loss="CosFace", local_epoch=1, output_dir="/tmp", BCE_local=False, aggr_alg=aggr, **extra))
        if srv is None:
            srv = server.Server([NeverTrains() for _ in range(3)], None, Args, device=torch.device("cpu"))
        srv.args, srv.robust_agg, srv.server_opt, srv.dp_accountant = Args, None, None, None
        return srv

    good = dict(secure_aggregation=True, secagg_bits=16, distributed_dp=True, ddp_wrap_sigmas=7, dp_noise_multiplier=1.0, clip_norm=1.0,
                secagg_frac_bits=10)
    for aggr in ("FedAvg", "FedAdam"):
        # without the opt-in: today's refusal, word for word, at both widths (absent and None are both "off")
        unset = {k: v for k, v in good.items() if k != "ddp_wrap_sigmas"}
        for bits in (8, 16):
            for off in ({}, {"ddp_wrap_sigmas": None}):
                with pytest.raises(ValueError, match=r"secagg_bits=%d cannot be combined with distributed_dp: discrete Gaussian noise in a ring of %d bits "
                                   r"needs its own sensitivity and wrap-around analysis, which is not provided" % (bits, bits)):
                    world(aggr, **dict(unset, secagg_bits=bits, **off)).train()
        # with it: 16 bits build the mechanism before anybody trains; 8, 32 and None are refused; so is a distributed_dp that is off
        with pytest.raises(ValueError, match=r"secagg_bits=8 cannot be combined with distributed_dp: 8-bit words cannot carry.*smallest sigma_int, 16"):
            world(aggr, **dict(good, secagg_bits=8)).train()
        for bits in (32, None):
            with pytest.raises(ValueError, match=r"ddp_wrap_sigmas=7 needs secagg_bits=16.*nothing wraps"):
                world(aggr, **dict(good, secagg_bits=bits)).train()
        no_bits = {k: v for k, v in good.items() if k != "secagg_bits"}
        with pytest.raises(ValueError, match=r"ddp_wrap_sigmas=7 needs secagg_bits=16"):
            world(aggr, **no_bits).train()
        for off in (False, None):
            with pytest.raises(ValueError, match=r"ddp_wrap_sigmas=7 needs distributed_dp"):
                world(aggr, **dict(good, distributed_dp=off, dp_noise_multiplier=0, clip_norm=0.0)).train()
        with pytest.raises(ValueError, match=r"ddp_wrap_sigmas=7 needs distributed_dp"):
            world(aggr, secure_aggregation=True, secagg_bits=16, ddp_wrap_sigmas=7).train()
        # what the mechanism refuses, with the fraction bits that would work; and a kappa that is none
        with pytest.raises(ValueError, match=r"DistributedDiscreteGaussian: the code clamp .* is below 1.*bits=16, wrap_sigmas=7.*secagg_frac_bits in 8 \.\.\. 11 would work"):
            world(aggr, **dict(good, secagg_frac_bits=16)).train()
        with pytest.raises(ValueError, match=r"DistributedDiscreteGaussian: sigma_int = .* is outside.*secagg_frac_bits in \d+ \.\.\. \d+ would work"):
            world(aggr, **dict(good, dp_noise_multiplier=0.01)).train()
        with pytest.raises(ValueError, match=r"wrap_sigmas must be a finite number >= 1"):
            world(aggr, **dict(good, ddp_wrap_sigmas=0.5)).train()
        # what distributed DP refuses at any width stays refused
        with pytest.raises(ValueError, match=r"distributed_dp needs dp_uniform_weights on"):
            world(aggr, dp_uniform_weights=False, **good).train()
        with pytest.raises(ValueError, match=r"secagg_threshold"):
            world(aggr, secagg_threshold=4, **good).train()
        for ok in ({}, {"secagg_drop": [2]}, {"secagg_rotation_seed": 5, "ddp_wrap_sigmas": 6.5}):
            with pytest.raises(AssertionError, match="a client was touched"):        # a servable setting: the round starts
                world(aggr, **dict(good, **ok)).train()
    with pytest.raises(ValueError, match=r"aggr_alg='SCAFFOLD' cannot be combined with secure_aggregation"):
        world("SCAFFOLD", **good).train()
    with pytest.raises(ValueError, match=r"topk_ratio=0.01"):
        world("FedAvg", topk_ratio=0.01, **good).train()


def test_mask_dp_and_fedsecaggdp_hold_the_widths_together():
    from fedfr_amd import secagg as P, server
    from fedfr_amd.client import FlatStateDict
    from fedfr_amd.privacy import DistributedDiscreteGaussian as M
    m32, m16 = M(1.0, 1.0, 16, 3, 2, 8), M(1.0, 1.0, 10, 3, 2, 8, bits=16, wrap_sigmas=7)
    cpu = FlatStateDict.from_flat((torch.zeros(8), torch.zeros(0), torch.zeros(0, dtype=torch.int64)), [], [])
    with pytest.raises(ValueError, match=r"mask_dp: distributed differential privacy at 8-bit words is not provided: 8-bit words cannot carry"):
        P.SecAggClient(0, 10, bits=8).mask_dp(cpu, cpu, [0, 1, 2], {}, 0, m16)
    with pytest.raises(ValueError, match=r"a mechanism of 16-bit words meets a client of 32-bit words"):
        P.SecAggClient(0, 10).mask_dp(cpu, cpu, [0, 1, 2], {}, 0, m16)
    with pytest.raises(ValueError, match=r"a mechanism of 32-bit words meets a client of 16-bit words"):
        P.SecAggClient(0, 16, bits=16).mask_dp(cpu, cpu, [0, 1, 2], {}, 0, m32)

    def up(bits, rot=1, frac=10):
        return P.MaskedUpdate(torch.zeros(8 if bits == 32 else 2048, dtype=torch.int32), 8, frac, torch.zeros(0), torch.zeros(0, dtype=torch.int64),
                              torch.zeros(3, dtype=torch.int32), sqnorm=torch.zeros(1, dtype=torch.int64), bits=bits, rotation_seed=rot, round=4)
    # FedSecAggDP hands the mechanism's width to the masked sum (on the GPU: tests/test_ddp_narrow_gpu.py), whose width and rotation
    # checks then apply
    with pytest.raises(RuntimeError, match="GPU"):                # a CPU state: refused as at 32 bits
        server.FedSecAggDP(cpu, [up(16), up(16)], [], m16)
    x = torch.zeros(8)
    with pytest.raises(RuntimeError, match=r"an upload of 32-bit words among uploads of 16-bit words"):
        server._masked_sum("FedSecAggDP", x, [up(16), up(32)], [], 10, 0.5, True, "%d %d", bits=m16.bits)
    with pytest.raises(RuntimeError, match=r"rotated with \(seed 2, round 4\) among uploads rotated with \(seed 1, round 4\)"):
        server._masked_sum("FedSecAggDP", x, [up(16), up(16, rot=2)], [], 10, 0.5, True, "%d %d", bits=m16.bits)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_host_side_checks_of_the_narrow_dp_entry_point(built_lib):
    """what the entry point refuses, it refuses on the host before any HIP call: FEDFR_ERR_ARG and a message naming the entry and the
    offending value, without a GPU (dummy host pointers: every call fails its checks first); n = 0 is a successful no-op"""
    lib = built_lib.lib()
    assert "fedfr_secagg_mask_narrow_dp" in built_lib.SIGNATURES
    err_arg = int(re.search(r"#define FEDFR_ERR_ARG \((-?\d+)\)", open(os.path.join(REPO, "include", "fedfr_hip.h")).read()).group(1))
    buf = (C.c_float * 128)()
    base = C.addressof(buf)
    base += -base % 16
    keys, nonces = (C.c_uint * (8 * 33))(), (C.c_uint * (3 * 33))()
    signs = (C.c_int * 33)(*[1] * 33)
    who = "secagg_mask_narrow_dp"

    def refused(rc, *words):
        msg = lib.fedfr_last_error_string().decode()
        assert rc == err_arg and who in msg and all(w in msg for w in words), (rc, msg)

    def mask(y=base, x=base + 64, xi=base + 128, coef=base + 192, frac_bits=12, limit=100, bits=16, offset=0, sigma=100.0, keys_=keys, nonces_=nonces,
             signs_=signs, k=2, counter0=0, n=8, counters=None, sqnorm=None):
        return lib.fedfr_secagg_mask_narrow_dp(y, x, xi, coef, frac_bits, limit, bits, 1, 2, 3, 4, 5, offset, sigma, keys_, nonces_, signs_, k, counter0, n,
                                               counters, sqnorm, None)

    refused(mask(y=None), "y=(nil)")
    refused(mask(x=None), "x=(nil)")
    refused(mask(xi=None), "xi=(nil)")
    refused(mask(coef=None), "clip_coef=(nil)")
    for bits in (0, 8, 12, 32):
        refused(mask(bits=bits), "bits must be 16", "bits=%d" % bits)
    refused(mask(frac_bits=7), "frac_bits=7")
    refused(mask(frac_bits=31), "frac_bits=31")
    refused(mask(limit=0), "code_limit=0")
    refused(mask(limit=-3), "code_limit=-3")
    refused(mask(limit=32768), "code_limit=32768")
    refused(mask(sigma=15.0), "sigma=15")
    refused(mask(sigma=2.0 ** 27), "sigma must be in [16, 2^26]")
    refused(mask(sigma=float("nan")), "sigma=nan")
    refused(mask(offset=2 ** 58 + 1), "2^58")
    refused(mask(offset=2 ** 58 - 4095), "2^58")                   # the noise covers the n_pad = 4096 padded elements, not the 8 given
    refused(mask(k=33), "k=33")
    refused(mask(k=-1), "k=-1")
    refused(mask(keys_=None), "keys=(nil)")
    refused(mask(signs_=(C.c_int * 2)(1, 0)), "sign 1 is 0")
    refused(mask(y=base + 4), "aligned")
    refused(mask(xi=base + 8), "aligned")
    refused(mask(coef=base + 2), "clip_coef")
    refused(mask(counters=base + 2), "counters")
    refused(mask(sqnorm=base + 4), "sqnorm")
    # the 32-bit block counter: a rotation block is 128 ChaCha20 blocks per stream at 16 bits
    refused(mask(counter0=0xFFFFFFFF - 126), "overflows")
    refused(mask(n=4097, counter0=0xFFFFFFFF - 254), "overflows")
    refused(mask(n=32 * 2 ** 32 + 1), "overflows")
    assert mask(n=0) == 0 and mask(n=0, k=0, keys_=None, nonces_=None, signs_=None) == 0 and mask(n=0, limit=32767, sigma=16.0) == 0


def test_narrow_dp_kernel_uses_no_scratch_and_keeps_the_lds_of_the_narrow_pass(built_lib):
    """from the code objects' metadata (tools/kernel_resources.py), in both builds: no scratch; static LDS is that of
    secagg_mask_narrow_kernel<16> (the noise strips alias the rotation buffer) plus four 64-bit partial sums, under 64 KB"""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr.kernels(built_lib.LIB_PATH)
    bf16 = os.path.join(os.path.dirname(built_lib.LIB_PATH), "libfedfr_hip_bf16.so")
    if os.path.exists(bf16) and os.path.basename(built_lib.LIB_PATH) != "libfedfr_hip_bf16.so":
        ks.update({"bf16:" + k: v for k, v in kr.kernels(bf16).items()})
    builds = 2 if any(k.startswith("bf16:") for k in ks) else 1
    mine = {n: r for n, r in ks.items() if "ddp_mask_narrow_kernel" in n}
    narrow = {n: r for n, r in ks.items() if "secagg_mask_narrow_kernelILi16" in n}
    assert len(mine) == builds and len(narrow) == builds, (sorted(mine), sorted(narrow))
    lds = {r["lds"] for r in narrow.values()}
    for n, r in mine.items():
        print(n, r)
        assert r["scratch"] == 0 and r["lds"] < 65536 and {r["lds"] - 32} == lds, (n, r, lds)
