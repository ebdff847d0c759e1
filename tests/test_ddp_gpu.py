"""Distributed differential privacy on the GPU: fedfr_dgauss_fill and fedfr_secagg_mask_dp against the restatements of tests/ddp_cases.py,
the protocol on raw FlatStateDicts (secagg.SecAggClient.mask_dp -> server.FedSecAggDP) with and without dropped clients, and Server.train
with distributed_dp.

EXACT EQUALITY, with two accepted deviations and no others:
  * the device's fp64 log / exp may differ from numpy's in the last place.  The restatement flags every element one of whose decisions lies
    within 64 ulp of its threshold; a test first asserts that NO element of its inputs is flagged (a property of the seeds stated in
    ddp_cases.py, also checked without a GPU), then compares every element exactly;
  * the device sums the squares of the norm pass in another order than numpy, so its clip factor may differ from the restated one by an
    ulp.  The factor is held to 2 ulp on its own, and the encode is restated from the device's own factor."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ddp_cases as X  # noqa: E402
import dp_cases as D  # noqa: E402
import secagg_cases as S  # noqa: E402
import test_secagg_gpu as A  # noqa: E402   (its device helpers, protocol set-up and tiny worlds: helpers, not tests)

from fedfr_amd import _C, client, privacy, secagg, server  # noqa: E402

DEV = A.DEV
f32, f64, u32, i32, i64 = np.float32, np.float64, np.uint32, np.int32, np.int64
G, N, ptr, SENT = A.G, A.N, A.ptr, A.SENT


def fill(dst, n, seed, rnd, sid, offset, sigma, exhausted):
    return _C.lib().fedfr_dgauss_fill(ptr(dst), n, seed, rnd, sid, offset, float(sigma), ptr(exhausted), _C.stream())


def mask_dp(y, x, xi, factor, limit, streams, counters, sqnorm, seed, rnd, offset, sigma, frac_bits=X.MASK_FRAC):
    return _C.lib().fedfr_secagg_mask_dp(ptr(y), ptr(x), ptr(xi), ptr(factor), frac_bits, limit, seed, rnd, offset, float(sigma), *A.arrays(streams),
                                         len(streams), x.numel(), ptr(counters), ptr(sqnorm), _C.stream())


def device_factor(xd, xid, clip):
    """min(1, clip / ||xi - x||) as fedfr_fedopt_sqnorm (k = 1, w = 1) leaves it on the device: a float32 tensor of one element"""
    return server.ServerOptimizer("AVGM", clip_norm=clip).coefficients(xd, [xid], [1.0])


@functools.lru_cache(maxsize=None)
def ref_noise(n, seed, rnd, sid, offset, sigma):
    values, _, ambiguous, exhausted = X.sample(n, seed, rnd, sid, offset, sigma)
    assert exhausted == 0 and not ambiguous.any(), "pick another seed: %d ambiguous decisions" % int(ambiguous.sum())
    w = X.as_u32(values)
    w.flags.writeable = False
    return w


# ---- fedfr_dgauss_fill -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", X.FILL_SIZES)
@pytest.mark.parametrize("sigma", X.FILL_SIGMAS)
def test_dgauss_fill_bit_identical_to_the_restatement(sigma, n):
    """the noise values from a tail-only size to 2^16 elements at the smallest sigma, an odd one and a large one; no element of the input
    is ambiguous; nothing is written behind n; no element exhausted its attempts"""
    ref = ref_noise(max(X.FILL_SIZES), X.FILL_SEED, X.FILL_ROUND, X.NOISE_STREAM, 0, sigma)[:n]
    buf = torch.full((n + 8,), SENT, dtype=torch.int32, device=DEV)
    exhausted = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert fill(buf, n, X.FILL_SEED, X.FILL_ROUND, X.NOISE_STREAM, 0, sigma, exhausted) == 0, _C.last_error()
    torch.cuda.synchronize()
    got = A.words_of(buf)
    A.same_words(got[:n], ref, "dgauss_fill(sigma=%g, n=%d)" % (sigma, n))
    assert np.all(got[n:] == SENT) and int(exhausted.item()) == 0


@pytest.mark.parametrize("sigma", X.FILL_SIGMAS)
def test_dgauss_fill_stream_coordinates(sigma, n=4100):
    """a non-zero offset (past 2^32 blocks: the high counter word), a shifted window of the same stream, and another round"""
    exhausted = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = {}
    for off, rnd in ((X.FILL_OFFSET, X.FILL_ROUND), (0, X.FILL_ROUND), (0, X.FILL_ROUND + 1)):
        buf = torch.full((n + 8,), SENT, dtype=torch.int32, device=DEV)
        assert fill(buf, n, X.FILL_SEED, rnd, X.NOISE_STREAM, off, sigma, exhausted) == 0, _C.last_error()
        got[off, rnd] = A.words_of(buf)
        A.same_words(got[off, rnd][:n], ref_noise(n, X.FILL_SEED, rnd, X.NOISE_STREAM, off, sigma), "dgauss_fill(offset=%d, round=%d)" % (off, rnd))
        assert np.all(got[off, rnd][n:] == SENT)
    assert np.mean(got[0, X.FILL_ROUND][:n] == got[0, X.FILL_ROUND + 1][:n]) < 0.05        # two rounds: different words
    assert np.mean(got[0, X.FILL_ROUND][:n] == got[X.FILL_OFFSET, X.FILL_ROUND][:n]) < 0.05
    buf = torch.full((100,), SENT, dtype=torch.int32, device=DEV)                          # elements 1000 ... 1099 of the stream at offset 0
    assert fill(buf, 100, X.FILL_SEED, X.FILL_ROUND, X.NOISE_STREAM, 1000, sigma, exhausted) == 0, _C.last_error()
    assert np.array_equal(A.words_of(buf), got[0, X.FILL_ROUND][1000:1100])
    assert int(exhausted.item()) == 0


# ---- fedfr_secagg_mask_dp ----------------------------------------------------------------------------------------------------------------
def check_mask_dp(n, k, kind, seed=X.MASK_SEED):
    x, xi, clip, limit = X.mask_inputs(n, kind)
    streams = S.some_streams(k)
    xd, xid = G(x), G(xi)
    factor = device_factor(xd, xid, clip)
    y = torch.full((n + 8,), SENT, dtype=torch.int32, device=DEV)
    counters = torch.tensor([1000, 2000, 3000], dtype=torch.int32, device=DEV)            # accumulated into
    sqnorm = torch.tensor([5], dtype=torch.int64, device=DEV)
    assert mask_dp(y, xd, xid, factor, limit, streams, counters, sqnorm, seed, X.MASK_ROUND, 0, X.MASK_SIGMA) == 0, _C.last_error()
    torch.cuda.synchronize()
    fdev, fref = f32(N(factor)[0]), X.clip_factor(x, xi, clip)
    assert abs(float(fdev) - float(fref)) <= 2 * float(np.spacing(fref)), (kind, n, fdev, fref)
    ref, sq_ref, counts_ref, ambiguous = X.mask_dp_u32(x, xi, fdev, X.MASK_FRAC, limit, seed, X.MASK_ROUND, 0, X.MASK_SIGMA, streams)
    assert not ambiguous.any(), "pick another seed: %d ambiguous decisions" % int(ambiguous.sum())
    got = A.words_of(y)
    A.same_words(got[:n], ref, "mask_dp(%s, k=%d, n=%d)" % (kind, k, n))
    assert np.all(got[n:] == SENT)
    sat, bad, exhausted = (int(v) for v in N(counters))
    assert (sat - 1000, bad - 2000, exhausted - 3000) == counts_ref and counts_ref[2] == 0
    assert (int(sqnorm.item()) - 5) % 2 ** 64 == sq_ref
    return fdev, counts_ref


@pytest.mark.parametrize("n", X.MASK_SIZES)
@pytest.mark.parametrize("k", [0, 1, 3, 32])
def test_secagg_mask_dp_bit_identical_to_the_restatement(k, n):
    """codes at the device's clip factor + noise + k signed streams, the exact sum of the squared codes and the three counters, for inputs
    with a NaN, +-inf and saturating elements (the clip factor stays 1: the norm is NaN), for a clip that binds (and an element that still
    saturates a small limit) and for one that does not"""
    f, (sat, bad, _) = check_mask_dp(n, k, "planted")
    assert f == 1.0 and sat >= 2 and bad >= 1
    f, (sat, bad, _) = check_mask_dp(n, k, "binds")
    assert 0.4 < f < 0.6 and (sat, bad) == (1, 0)
    f, (sat, bad, _) = check_mask_dp(n, k, "free")
    assert f == 1.0 and (sat, bad) == (0, 0)


def test_secagg_mask_dp_at_the_grid_stride_wrap():
    f, (sat, bad, _) = check_mask_dp(S.GRID_WRAP, 1, "planted")
    assert f == 1.0 and sat >= 2 and bad >= 3


def test_secagg_mask_dp_without_counters_and_with_another_noise_seed(n=4100):
    """counters and sqnorm may be NULL; the noise depends on the seed, the codes and the masks do not"""
    x, xi, clip, limit = X.mask_inputs(n, "free")
    xd, xid = G(x), G(xi)
    factor = device_factor(xd, xid, clip)
    streams = S.some_streams(3)
    ys = []
    for seed in (X.MASK_SEED, X.MASK_SEED + 1):
        y = torch.empty(n, dtype=torch.int32, device=DEV)
        assert mask_dp(y, xd, xid, factor, limit, streams, None, None, seed, X.MASK_ROUND, 0, X.MASK_SIGMA) == 0, _C.last_error()
        ys.append(A.words_of(y))
    A.same_words(ys[0], X.mask_dp_u32(x, xi, f32(N(factor)[0]), X.MASK_FRAC, limit, X.MASK_SEED, X.MASK_ROUND, 0, X.MASK_SIGMA, streams)[0], "NULL counters")
    with np.errstate(over="ignore"):
        diff = (ys[0] - ys[1]).view(i32)
    assert np.mean(diff != 0) > 0.95 and np.abs(diff).max() <= 2 * X.TAIL * (int(X.MASK_SIGMA) + 1)      # two noise draws apart, nothing else


# ---- the protocol on FlatStateDicts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K, dropped, opt", [(4, (), None), (4, (2,), None), (11, (), None), (11, (0, 4, 9, 10), "ADAM"),
                                            (11, (0, 4, 9, 10), None)])      # (the last row: a last pass of recovery streams only adds x)
def test_protocol_reproduces_the_restatement_and_the_masks_leave_no_trace(K, dropped, opt):
    """SecAggClient.mask_dp -> SecAggServer.recovery_streams -> FedSecAggDP on the flat world of test_secagg_gpu.py: every upload is the
    restatement's words; the aggregate is x + float(sum of codes + sum of noise) 2^-f fp32(1 / survivors) bit for bit (past 8 uploads and
    32 recovery streams too, and through a server optimiser); and with the test's knowledge of the noise seeds, the integer sum of the
    uploads and the recovery streams minus the noise is exactly the sum of the clipped codes"""
    glob, models, sizes = A._flat_world(K)
    x, n = N(glob.flat[0]), glob.flat[0].numel()
    rnd, t, frac = 9, K // 2 + 1, 16
    mech = privacy.DistributedDiscreteGaussian(1.0, 0.1, frac, K, t, n)
    r = np.random.default_rng(11).bytes
    parts = list(range(K))
    clients = [secagg.SecAggClient(c, frac, r) for c in parts]
    srv = secagg.SecAggServer(parts, t, rnd)
    for c in clients:
        srv.register(c.cid, c.begin_round(rnd))
    for c in clients:
        srv.deliver_shares(c.cid, c.make_shares(parts, t))
    ups = [c.mask_dp(glob, m, parts, srv.public_keys, rnd, mech) for c, m in zip(clients, models)]
    torch.cuda.synchronize()
    assert len({c.noise_seed for c in clients}) == K
    codes, noises, clipped = [], [], 0
    for c, m, u in zip(clients, models, ups):
        assert isinstance(u, secagg.MaskedUpdate) and u.n == n and u.frac_bits == frac and u.stats is m.flat[1] and u.counters is m.flat[2]
        assert (u.saturated_count(), u.nonfinite_count(), u.exhausted_count()) == (0, 0, 0)
        xi = N(m.flat[0])
        fdev, fref = f32(N(device_factor(glob.flat[0], m.flat[0], mech.clip_norm))[0]), X.clip_factor(x, xi, mech.clip_norm)
        assert abs(float(fdev) - float(fref)) <= 2 * float(np.spacing(fref))
        clipped += fdev < 1.0
        ref, sq, _, amb = X.mask_dp_u32(x, xi, fdev, frac, mech.code_limit, c.noise_seed, rnd, 0, mech.sigma_int, c.streams(parts, srv.public_keys, rnd))
        assert not amb.any(), "pick another seed: %d ambiguous decisions" % int(amb.sum())
        A.same_words(A.words_of(u.y), ref, "upload of client %d" % c.cid)
        assert u.sqnorm_value() == sq and sq <= mech.delta_int ** 2
        codes.append(S.encode32(x, xi, fdev * f32(2.0 ** frac), mech.code_limit)[0].view(u32))
        noises.append(X.as_u32(X.sample(n, c.noise_seed, rnd, X.NOISE_STREAM, 0, mech.sigma_int)[0]))
    assert 0 < clipped < K                                       # the clip binds for some clients of this world and not for others
    keep = [p for p in parts if p not in dropped]
    rec = srv.recovery_streams(keep)
    with np.errstate(over="ignore"):
        total = sum((A.words_of(ups[p].y) for p in keep), np.zeros(n, u32)) + S.stream_sum(n, rec)
        assert np.array_equal(total - sum((noises[p] for p in keep), np.zeros(n, u32)), sum((codes[p] for p in keep), np.zeros(n, u32)))
        noisy = [codes[p] + noises[p] for p in keep]
    rescale = float(f32(1.0 / len(keep)))
    sopt = None if opt is None else server.ServerOptimizer(opt, lr=0.01)
    out = server.FedSecAggDP(glob, [ups[p] for p in keep], rec, mech, sopt)
    avg = server.FedPavg([models[p] for p in keep], [1.0] * len(keep))
    torch.cuda.synchronize()
    assert isinstance(out, client.FlatStateDict) and torch.equal(out.flat[1], avg.flat[1]) and torch.equal(out.flat[2], avg.flat[2])
    if sopt is None:
        A.T.same_bits(N(out.flat[0]), S.aggregate32(x, noisy, [], frac, rescale), "FedSecAggDP parameters")
        # and the noise is there: per coordinate sigma_int sqrt(survivors) 2^-f / survivors around the mean of the clipped updates
        plain = S.aggregate32(x, [codes[p] for p in keep], [], frac, rescale)
        ratio = float(np.std(N(out.flat[0]).astype(f64) - plain)) / (mech.sigma_int * math.sqrt(len(keep)) * 2.0 ** -frac / len(keep))
        assert 0.9 < ratio < 1.1, ratio
    else:
        delta = G(S.aggregate32(None, noisy, [], frac, rescale))
        twin = server.ServerOptimizer(opt, lr=sopt.lr)
        want = torch.empty_like(delta)
        twin.apply_delta(want, glob.flat[0], delta)
        torch.cuda.synchronize()
        A.T.same_bits(N(out.flat[0]), N(want), "FedSecAggDP through %s" % opt)
    with pytest.raises(ValueError, match="uploads, the mechanism needs"):
        server.FedSecAggDP(glob, ups[:t - 1], [], mech)


# ---- Server.train ------------------------------------------------------------------------------------------------------------------------
Z, CLIP, FRAC, DELTA = 0.005, 1.0, 16, 1e-5


def _train(aggr, rounds, drop):
    """a server of test_secagg_gpu.py's three-client world under distributed DP, trained for ``rounds`` rounds; per round the state before,
    the clients' states, their noise seeds and the state after"""
    extra = {} if drop is None else {"secagg_drop": drop}
    srv, clients = A._world3(aggr, secure_aggregation=True, distributed_dp=True, dp_noise_multiplier=Z, clip_norm=CLIP, secagg_frac_bits=FRAC,
                             dp_delta=DELTA, server_lr=0.01, **extra)
    log = []
    for r in range(rounds):
        before = client.flat_state_dict(srv.federated_model).flat[0].clone()
        loss = srv.train()
        srv.step_round()
        torch.cuda.synchronize()
        assert np.isfinite(loss)
        log.append((before, [c.get_model().flat[0].clone() for c in clients], [c.secagg.noise_seed for c in clients],
                    [t.clone() for t in srv.federated_model.flat_state()], srv.dp_epsilon, list(srv.dp_last_sqnorms)))
    return srv, log


@pytest.mark.parametrize("aggr, rounds, drop", [("FedAvg", 2, None), ("FedAdam", 1, None), ("FedAvg", 1, [1])])
def test_server_train_with_distributed_dp(aggr, rounds, drop, caplog):
    """Server.train(distributed_dp=True): the model moves; the parameters are the restatement applied to the clients' trained states
    (device clip factor, codes, the noise of fedfr_dgauss_fill at each client's own seed, the mean over the uploads that arrived; through
    the server optimiser for FedAdam) bit for bit; dp_epsilon is the hand value at q = 1 and the guaranteed z_eff; the log says so; every
    survivor's sum of squared codes is within delta_int^2; and a second server with the same seeds reproduces the state bit for bit"""
    import logging
    with caplog.at_level(logging.INFO, logger="FL_face.server"):
        srv, log = _train(aggr, rounds, drop)
    keep = [i for i in range(3) if i not in (drop or [])]
    n = log[0][0].numel()
    T = 2                                                        # the default threshold of three clients
    sigma_int = Z * CLIP * 2.0 ** FRAC / math.sqrt(T)
    delta_int = CLIP * 2.0 ** FRAC * (1 + 2.0 ** -22) + math.sqrt(n) / 2
    z_eff = math.sqrt(T) * sigma_int / delta_int
    limit = S.code_limit(3) - X.TAIL * (int(sigma_int) + 1)
    assert "Distributed differential privacy" in caplog.text and ("z_eff = %.6g" % z_eff) in caplog.text and "accounted at q = 1" in caplog.text
    assert ("realised %.6g with %d uploads" % (math.sqrt(len(keep) / T) * z_eff, len(keep))) in caplog.text
    assert "Masked uploads (16 fraction bits, threshold 2)" in caplog.text and "saturated" not in caplog.text
    twin = server.ServerOptimizer("ADAM", lr=0.01) if aggr == "FedAdam" else None
    for r, (x, xs, seeds, after, eps, sqnorms) in enumerate(log):
        assert eps == pytest.approx(D.epsilon_by_hand(1.0, z_eff, r + 1, DELTA), rel=1e-9)
        assert len(sqnorms) == len(keep) and all(0 < v <= delta_int ** 2 for v in sqnorms)
        assert not torch.equal(after[0], x)
        total = torch.zeros(n, dtype=torch.int64, device=DEV)
        exhausted = torch.zeros(1, dtype=torch.int32, device=DEV)
        for i in keep:
            coef = device_factor(x, xs[i], CLIP) * float(2.0 ** FRAC)
            t = (xs[i] - x) * coef
            assert t.dtype == torch.float32 and bool(torch.isfinite(t).all())
            q = torch.round(t).to(torch.int64).clamp_(-limit, limit)
            noise = torch.empty(n, dtype=torch.int32, device=DEV)
            assert fill(noise, n, seeds[i], r, X.NOISE_STREAM, 0, sigma_int, exhausted) == 0, _C.last_error()
            total += q + noise
        assert int(exhausted.item()) == 0 and int(total.abs().max()) < 2 ** 31
        d = total.to(torch.int32).to(torch.float32)
        d = d * float(2.0 ** -FRAC)
        d = d * float(f32(1.0 / len(keep)))
        if twin is None:
            assert torch.equal(after[0], x + d), "round %d: parameters differ from the restatement" % r
        else:
            want = torch.empty_like(x)
            twin.apply_delta(want, x, d)
            assert torch.equal(after[0], want), "round %d: parameters differ from the restatement through FedAdam" % r
    assert srv.dp_accountant.steps == rounds and (srv.dp_accountant.q, srv.dp_accountant.sigma) == (1.0, pytest.approx(z_eff, rel=1e-12))
    if drop is not None:                                         # the same seeds again: the same bits
        _, again = _train(aggr, rounds, drop)
        for a, b in zip(log, again):
            assert a[2] == b[2] and all(torch.equal(u, v) for u, v in zip(a[3], b[3]))
