"""Client-level differential privacy, the part that needs no GPU: the Philox restatement of tests/dp_cases.py (which fedfr_philox_fill is
held to bit for bit on the GPU) against the Random123 known answers, the RDP accountant against its closed forms and against direct
quadrature of the Renyi divergence, the mechanism's bookkeeping, the host-side argument checks of the new C entry points, no scratch memory
in any new kernel, and the combinations Server.train refuses before any client trains."""
import ctypes as C
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

import dp_cases as D
from conftest import REPO

f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from fedfr_amd import _C
    return _C


# ---- the generator's restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_restatement_known_answers(ctr, key, want):
    """the Random123 known-answer vectors of Philox4x32-10"""
    got = " ".join("%08x" % int(w[0]) for w in D.philox4x32_10(ctr, key))
    assert got == want


def test_stream_indexing_of_the_restatement():
    """element e is lane e % 4 of block e / 4 with counter (blk low, blk high, round low, stream_id) and key (seed low, seed high): a
    window of the stream is the stream at an offset, the high counter word is live past 2^34 elements, and each coordinate matters"""
    seed, rnd, sid = 123 | 456 << 32, 7, 1
    w = D.words(4103, seed, rnd, sid)
    assert w.dtype == np.uint32 and w.shape == (4103,)
    one = D.philox4x32_10((5, 0, 7, 1), (123, 456))
    assert [int(a[0]) for a in one] == [int(a) for a in w[20:24]]
    for a in (4, 1024):
        assert np.array_equal(D.words(100, seed, rnd, sid, offset=a), w[a:a + 100])
    hi = D.words(8, seed, rnd, sid, offset=1 << 34)
    assert [int(a[0]) for a in D.philox4x32_10((0, 1, 7, 1), (123, 456))] == [int(a) for a in hi[:4]]
    assert not np.array_equal(hi, w[:8])
    assert np.array_equal(D.words(8, seed, rnd + (1 << 32), sid), w[:8])            # round enters with its low 32 bits
    for other in (D.words(8, seed + 1, rnd, sid), D.words(8, seed + (1 << 32), rnd, sid), D.words(8, seed, rnd + 1, sid), D.words(8, seed, rnd, sid + 1)):
        assert not np.any(other == w[:8])


def test_gauss64_moments_and_tail():
    """the fp64 restatement of the Gaussian formula on the GPU test's sample: moments inside 5 standard errors, tails inside sqrt(48 ln 2)"""
    z = D.gauss64(1 << 20, 123 | 456 << 32, 7, 1)
    assert abs(z.mean()) < 0.0049 and abs(z.var() - 1) < 0.0069 and abs((z ** 4).mean() - 3) < 0.048
    assert np.abs(z).max() < D.TAIL_BOUND and abs(D.TAIL_BOUND - 5.7689) < 1e-3


# ---- the accountant ----------------------------------------------------------------------------------------------------------------------
def test_rdp_at_full_participation_is_the_gaussian_closed_form():
    from fedfr_amd.privacy import RDPAccountant
    for sigma in (0.5, 1.0, 1.1, 4.0):
        acc = RDPAccountant(1.0, sigma)
        for a in (2, 3, 17, 256):
            assert acc.rdp(a) == a / (2 * sigma * sigma)


def test_rdp_is_monotone_in_q_and_vanishes_with_it():
    from fedfr_amd.privacy import RDPAccountant
    qs = (1e-6, 1e-4, 0.01, 0.1, 0.25, 0.5, 0.9, 0.999, 1.0)
    for sigma in (0.8, 1.0, 2.0):
        for a in (2, 8, 32, 256):
            r = [RDPAccountant(q, sigma).rdp(a) for q in qs]
            assert all(x >= 0 for x in r) and all(x < y for x, y in zip(r, r[1:])), (sigma, a, r)
        assert RDPAccountant(1e-6, sigma).rdp(2) < 1e-10                         # ~ q^2 (exp(1 / sigma^2) - 1)
        assert RDPAccountant(1e-9, sigma).rdp(2) < 1e-16


@pytest.mark.parametrize("q, sigma, alpha", [(0.1, 1, 2), (0.1, 1, 8), (0.5, 0.8, 4), (0.01, 1.1, 32), (0.25, 2, 16)])
def test_rdp_against_quadrature(q, sigma, alpha):
    """the binomial closed form against the trapezoid quadrature of the Renyi divergence between (1 - q) N(0, s^2) + q N(1, s^2) and
    N(0, s^2), 4 * 10^6 points on [-40 s, 40 s + alpha]: 1e-9 relative"""
    from fedfr_amd.privacy import RDPAccountant
    got, ref = RDPAccountant(q, sigma).rdp(alpha), D.quadrature_rdp(q, sigma, alpha)
    print("q=%g sigma=%g alpha=%d: rdp %.15g, quadrature %.15g, relative difference %.2e" % (q, sigma, alpha, got, ref, abs(got - ref) / ref))
    assert abs(got - ref) <= 1e-9 * ref


def test_epsilon_composition_and_state():
    from fedfr_amd.privacy import RDPAccountant
    acc = RDPAccountant(1.0, 1.0)
    for _ in range(10):
        acc.step()
    eps = acc.epsilon(1e-5)
    closed = 10 / 2.0 + math.sqrt(2 * 10 * math.log(1e5))                        # the real-order optimum: T / (2 s^2) + sqrt(2 T ln(1 / delta)) / s
    print("epsilon %.6f, real-order closed form %.6f" % (eps, closed))
    assert abs(closed - 20.174) < 1e-3 and closed <= eps <= closed + 1
    assert abs(eps - 20.756) < 1e-3 and abs(eps - D.epsilon_by_hand(1.0, 1.0, 10, 1e-5)) < 1e-12
    assert acc.epsilon(1e-5, rounds=20) > eps > acc.epsilon(1e-5, rounds=5) and acc.epsilon(1e-7) > eps
    sub = RDPAccountant(0.1, 1.0)
    sub.step(10)
    assert sub.epsilon(1e-5) < eps and abs(sub.epsilon(1e-5) - D.epsilon_by_hand(0.1, 1.0, 10, 1e-5)) < 1e-9
    twin = RDPAccountant(0.5, 3.0)
    twin.load_state_dict(sub.state_dict())
    assert twin.steps == 10 and twin.epsilon(1e-5) == sub.epsilon(1e-5) and twin.state_dict() == sub.state_dict()
    for bad in ((0.0, 1.0), (1.5, 1.0), (0.5, 0.0), (0.5, float("inf"))):
        with pytest.raises(ValueError, match="RDPAccountant"):
            RDPAccountant(*bad)
    with pytest.raises(ValueError, match="alpha"):
        acc.rdp(1.5)
    with pytest.raises(ValueError, match="delta"):
        acc.epsilon(0.0)


def test_gaussian_mechanism_bookkeeping():
    from fedfr_amd.privacy import GaussianMechanism
    mech = GaussianMechanism(1.1, 0.7, seed=123 | 456 << 32, stream_id=3)
    ws = [0.25, 0.5, 0.25]
    assert mech.noise_std(ws) == float((f32(1.1) * f32(0.7)) * f32(0.5)) == float(D.noise_std32(1.1, 0.7, 0.5)) and mech.round == 0
    mech.advance()
    mech.advance()
    sd = mech.state_dict()
    assert sd["round"] == 2 and sd["seed"] == 123 | 456 << 32 and sd["stream_id"] == 3
    twin = GaussianMechanism(1.1, 0.7, seed=0)
    twin.load_state_dict(sd)
    assert (twin.seed, twin.round, twin.stream_id, twin.noise_std(ws)) == (mech.seed, 2, 3, mech.noise_std(ws))
    assert GaussianMechanism(1.0, 1.0, seed=-1).seed == (1 << 64) - 1                # the seed is taken modulo 2^64
    for bad in ((-1.0, 1.0), (float("nan"), 1.0), (1.0, 0.0), (1.0, -2.0), (1.0, float("inf"))):
        with pytest.raises(ValueError, match="GaussianMechanism"):
            GaussianMechanism(*bad, seed=1)
    with pytest.raises(ValueError, match="stream_id"):
        GaussianMechanism(1.0, 1.0, seed=1, stream_id=1 << 32)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_host_side_checks_of_the_new_entry_points(built_lib):
    """what the entry points refuse, they refuse on the host before any HIP call: FEDFR_ERR_ARG and a message, without a GPU (dummy host
    pointers: every call fails its checks first)"""
    lib = built_lib.lib()
    err_arg = int(re.search(r"#define FEDFR_ERR_ARG \((-?\d+)\)", open(os.path.join(REPO, "include", "fedfr_hip.h")).read()).group(1))
    buf = (C.c_float * 64)()
    base = C.addressof(buf)
    base += -base % 16

    def refused(rc, *words):
        msg = lib.fedfr_last_error_string().decode()
        assert rc == err_arg and all(w in msg for w in words), (rc, msg)

    refused(lib.fedfr_philox_fill(None, 8, 1, 0, 0, 0, None), "philox_fill")
    refused(lib.fedfr_philox_fill(base, 0, 1, 0, 0, 0, None), "philox_fill")
    refused(lib.fedfr_philox_fill(base + 4, 8, 1, 0, 0, 0, None), "philox_fill", "aligned")
    refused(lib.fedfr_philox_fill(base, 8, 1, 0, 0, 6, None), "philox_fill", "offset 6")
    refused(lib.fedfr_gaussian_fill(None, 8, 1, 0, 0, 0, 1.0, 0, None), "gaussian_fill")
    refused(lib.fedfr_gaussian_fill(base + 8, 8, 1, 0, 0, 0, 1.0, 0, None), "gaussian_fill", "aligned")
    refused(lib.fedfr_gaussian_fill(base, 8, 1, 0, 0, 2, 1.0, 0, None), "gaussian_fill", "offset 2")
    refused(lib.fedfr_gaussian_fill(base, 8, 1, 0, 0, 0, float("inf"), 0, None), "gaussian_fill", "std")
    ptrs = (C.c_void_p * 8)(*[base] * 8)
    h = (1.0, 0.9, 0.1, 0.99, 0.01, 1e-3)

    def multi(kind=4, x_out=base, x=base, xs=ptrs, coef=base, k=1, n=8, m=base, v=base, scratch=None, first=1, last=1, std=1.0, offset=0):
        return lib.fedfr_dp_multi(kind, x_out, x, xs, coef, k, n, m, v, scratch, first, last, *h, std, 1, 0, 0, offset, None)

    refused(multi(kind=5), "dp_multi", "kind 5")
    refused(multi(kind=-1), "dp_multi", "kind -1")
    refused(multi(std=-1.0), "dp_multi", "noise_std")
    refused(multi(std=float("nan")), "dp_multi", "noise_std")
    refused(multi(std=float("inf")), "dp_multi", "noise_std")
    refused(multi(offset=5), "dp_multi", "offset 5")
    refused(multi(k=0), "dp_multi", "k=0")
    refused(multi(k=9), "dp_multi", "k=9")
    refused(multi(n=0), "dp_multi")
    refused(multi(x=None), "dp_multi")
    refused(multi(coef=None), "dp_multi")
    refused(multi(x_out=None), "dp_multi", "x_out")
    refused(multi(kind=0, m=None), "dp_multi", "m")
    refused(multi(kind=2, v=None), "dp_multi", "v")
    refused(multi(first=0), "dp_multi", "scratch")
    refused(multi(last=0), "dp_multi", "scratch")
    refused(multi(x_out=base + 4), "dp_multi", "aligned")
    refused(multi(kind=2, v=base + 4), "dp_multi", "aligned")
    refused(multi(xs=(C.c_void_p * 2)(base, None), k=2), "dp_multi", "null")
    refused(multi(kind=2, std=0.0, k=9), "fedopt_multi", "k=9")                     # noise_std = 0 on kinds 0..3 IS fedfr_fedopt_multi


def test_no_new_kernel_uses_scratch_memory(built_lib):
    """the rule of tests/test_abi.py::test_hot_kernels_do_not_spill for the kernels of csrc/dp.hip, all 5 kinds x 8 client counts in both
    builds, read from the code objects' metadata (tools/kernel_resources.py)"""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr.kernels(built_lib.LIB_PATH)
    bf16 = os.path.join(os.path.dirname(built_lib.LIB_PATH), "libfedfr_hip_bf16.so")
    if os.path.exists(bf16) and os.path.basename(built_lib.LIB_PATH) != "libfedfr_hip_bf16.so":
        ks.update({"bf16:" + k: v for k, v in kr.kernels(bf16).items()})
    builds = 2 if any(k.startswith("bf16:") for k in ks) else 1
    dp = {n: r for n, r in ks.items() if "dp_multi_kernel" in n}
    fills = {n: r for n, r in ks.items() if "philox_fill_kernel" in n or "gaussian_fill_kernel" in n}
    assert len(dp) == 40 * builds and len(fills) == 2 * builds, (len(dp), sorted(fills))
    bad = [(n, r) for n, r in list(dp.items()) + list(fills.items()) if r["scratch"]]
    assert not bad, bad


# ---- Server.train ------------------------------------------------------------------------------------------------------------------------
def test_server_train_refuses_dp_settings_before_any_client_trains():
    from fedfr_amd import server

    def world(aggr, nclients=3, **extra):
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

    for aggr in ("FedAvg", "FedProx", "FedAdam"):
        with pytest.raises(ValueError, match=r"dp_noise_multiplier=1.0 needs clip_norm > 0"):
            world(aggr, dp_noise_multiplier=1.0).train()
        with pytest.raises(ValueError, match=r"dp_noise_multiplier=1.0 needs clip_norm > 0"):
            world(aggr, dp_noise_multiplier=1.0, clip_norm=0.0).train()
        for bits in (4, 8):
            with pytest.raises(ValueError, match=r"dp_noise_multiplier=1.1.*compress_bits=%d" % bits):
                world(aggr, dp_noise_multiplier=1.1, clip_norm=2.0, compress_bits=bits).train()
        with pytest.raises(ValueError, match=r"dp_noise_multiplier=1.1.*topk_ratio=0.01"):
            world(aggr, dp_noise_multiplier=1.1, clip_norm=2.0, topk_ratio=0.01).train()
        with pytest.raises(ValueError, match=r"dp_noise_multiplier=1.1.*return_all"):
            world(aggr, dp_noise_multiplier=1.1, clip_norm=2.0, return_all=True, add_pretrained_data=True).train()
    for kind in sorted(server.ROBUST_ALG_KINDS):
        with pytest.raises(ValueError, match=r"dp_noise_multiplier=1.1.*%s" % kind):
            world(kind, 5, dp_noise_multiplier=1.1, clip_norm=2.0).train()
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="dp_noise_multiplier"):
            world("FedAvg", dp_noise_multiplier=bad, clip_norm=2.0).train()
    for bad in (0.0, 1.0, -1e-5):
        with pytest.raises(ValueError, match="dp_delta"):
            world("FedAvg", dp_noise_multiplier=1.0, clip_norm=2.0, dp_delta=bad).train()
    from fedfr_amd.privacy import RDPAccountant
    srv = world("FedAvg", dp_noise_multiplier=1.0, clip_norm=2.0)
    srv.dp_accountant = RDPAccountant(1.0, 2.0)                                      # earlier rounds were accounted at another multiplier
    with pytest.raises(ValueError, match=r"dp_noise_multiplier=1.0 after rounds accounted at 2.0"):
        srv.train()
    with pytest.raises(AssertionError, match="a client was touched"):                # dp off: nothing is refused and the round starts
        world("FedAvg", dp_noise_multiplier=0, clip_norm=2.0).train()
    with pytest.raises(AssertionError, match="a client was touched"):                # a servable DP setting: the round starts too
        world("FedAvg", dp_noise_multiplier=1.0, clip_norm=2.0, dp_seed=1).train()


def test_all_reduce_path_and_feddp_refuse_what_they_cannot_serve():
    from fedfr_amd import privacy, server
    from fedfr_amd.client import FlatStateDict
    mech = privacy.GaussianMechanism(1.0, 2.0, seed=1)
    with pytest.raises(ValueError, match="differential privacy"):
        server.fedavg_all_reduce(None, 1.0, 1.0, None, dp=mech)
    cpu = FlatStateDict.from_flat((torch.zeros(8), torch.zeros(0), torch.zeros(0, dtype=torch.int64)), [], [])
    with pytest.raises(RuntimeError, match="FlatStateDict"):
        server.FedDP({"w": torch.zeros(8)}, [cpu], [1.0], mech)
    with pytest.raises(RuntimeError, match="weights"):
        server.FedDP(cpu, [cpu, cpu], [1.0], mech)
    with pytest.raises(RuntimeError, match="GPU"):
        server.FedDP(cpu, [cpu], [1.0], mech)
    assert mech.round == 0                                                           # a refused call consumes no round of the noise stream
