"""Distributed differential privacy at 16-bit narrow words on the GPU: fedfr_secagg_mask_narrow_dp against the restatement of
tests/ddp_narrow_cases.py, against fedfr_dgauss_fill and against fedfr_secagg_mask_narrow (device against device, also past one grid
pass), the protocol on raw FlatStateDicts (SecAggClient(bits=16).mask_dp -> FedSecAggDP) with and without dropped clients, and Server.train
with secagg_bits=16, distributed_dp and ddp_wrap_sigmas.

EXACT EQUALITY throughout, with the two accepted deviations of tests/test_ddp_gpu.py and no others:
  * the device's fp64 log / exp may differ from numpy's in the last place.  The restatement flags every element one of whose decisions lies
    within 64 ulp of its threshold; a test first asserts that NO element of its inputs is flagged (a property of the seeds stated in
    ddp_narrow_cases.py, also checked without a GPU), then compares every word exactly;
  * the device sums the squares of the norm pass in another order than numpy, so its clip factor may differ from the restated one by an
    ulp.  The factor is held to 2 ulp on its own, and the encode is restated from the device's own factor."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ddp_cases as X  # noqa: E402
import ddp_narrow_cases as W  # noqa: E402
import dp_cases as D  # noqa: E402
import secagg_cases as S  # noqa: E402
import secagg_narrow_cases as N  # noqa: E402
import test_secagg_gpu as A  # noqa: E402   (its device helpers, protocol set-up and tiny worlds: helpers, not tests)
import test_secagg_narrow_gpu as NG  # noqa: E402   (the rotation and the Philox words in torch: helpers, not tests)

from fedfr_amd import _C, client, privacy, secagg, server  # noqa: E402

DEV = A.DEV
f32, f64, u32, i32, i64 = np.float32, np.float64, np.uint32, np.int32, np.int64
G, NP, ptr, SENT = A.G, A.N, A.ptr, A.SENT


def mask_ndp(y, x, xi, factor, limit, streams, counters, sqnorm, sigma, frac_bits=W.FRAC, rot=W.ROT_SEED, priv=W.PRIV_SEED, rnd=W.RND,
             seed=W.NOISE_SEED, nrnd=W.NOISE_ROUND, offset=0, counter0=0, n=None):
    return _C.lib().fedfr_secagg_mask_narrow_dp(ptr(y), ptr(x), ptr(xi), ptr(factor), frac_bits, limit, 16, rot, priv, rnd, seed, nrnd, offset, float(sigma),
                                                *A.arrays(streams), len(streams), counter0, x.numel() if n is None else n, ptr(counters), ptr(sqnorm),
                                                _C.stream())


def mask_narrow(y, x, xi, coef, K, streams, counters, counter0=0, rot=W.ROT_SEED, priv=W.PRIV_SEED, rnd=W.RND):
    return _C.lib().fedfr_secagg_mask_narrow(ptr(y), ptr(x), ptr(xi), float(coef), K, 16, rot, priv, rnd, *A.arrays(streams), len(streams), counter0,
                                             x.numel(), ptr(counters), _C.stream())


def device_factor(xd, xid, clip):
    """min(1, clip / ||xi - x||) as fedfr_fedopt_sqnorm (k = 1, w = 1) leaves it on the device: a float32 tensor of one element"""
    return server.ServerOptimizer("AVGM", clip_norm=clip).coefficients(xd, [xid], [1.0])


def device_noise(npad, seed, rnd, offset, sigma):
    """the values of elements offset ... offset + npad - 1 of the clients' noise stream, from fedfr_dgauss_fill (held to ddp_cases.sample by
    tests/test_ddp_gpu.py), as int64"""
    z = torch.empty(npad, dtype=torch.int32, device=DEV)
    ex = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert _C.lib().fedfr_dgauss_fill(ptr(z), npad, seed, rnd, X.NOISE_STREAM, offset, float(sigma), ptr(ex), _C.stream()) == 0, _C.last_error()
    assert int(ex.item()) == 0
    return z.to(torch.int64)


def fields_t(y):
    """the 16-bit fields of packed int32 words as int64 in [0, 2^16), element e = field e % 2 of word e / 2"""
    w = y.to(torch.int64) & 0xFFFFFFFF
    return torch.stack([w & 0xFFFF, w >> 16], dim=1).reshape(-1)


@functools.lru_cache(maxsize=None)
def ref_noise(npad, seed, rnd, offset, sigma):
    z, amb, exhausted = W.noise(npad, seed, rnd, offset, sigma)
    assert exhausted == 0 and not amb.any(), "pick another seed: %d ambiguous decisions" % int(amb.sum())
    z.flags.writeable = False
    return z


@functools.lru_cache(maxsize=None)
def ref_codes(n, kind, factor_bits):
    x, xi, _, limit, _ = W.inputs(n, kind)
    q, sat, bad = W.codes(x, xi, np.array(factor_bits, u32).view(f32), W.FRAC, limit, W.ROT_SEED, W.PRIV_SEED, W.RND)
    q.flags.writeable = False
    return q, sat, bad


def restated(n, kind, fdev, streams, counter0=0, seed=W.NOISE_SEED, nrnd=W.NOISE_ROUND, offset=0):
    """ddp_narrow_cases.mask_narrow_dp with its codes and its noise computed once per input and shared among the cases"""
    sigma = W.inputs(n, kind)[4]
    q, sat, bad = ref_codes(n, kind, int(np.array(fdev, f32).view(u32)))
    z = ref_noise(q.size, seed, nrnd, offset, sigma)
    w = N.pack(q.astype(i64) + z, 16)
    return N.field_add(w, N.stream_sum_fields(w.size, streams, 16, counter0), 16), X._sq_mod64(q), (sat, bad, 0)


# ---- 1. the entry point against the restatement ---------------------------------------------------------------------------------------------
def check_case(n, k, kind, counter0=0):
    x, xi, clip, limit, sigma = W.inputs(n, kind)
    streams = S.some_streams(k)
    xd, xid, nw = G(x), G(xi), N.padded_count(n) // 2
    factor = device_factor(xd, xid, clip)
    y = torch.full((nw + 8,), SENT, dtype=torch.int32, device=DEV)
    counters = torch.tensor([1000, 2000, 3000], dtype=torch.int32, device=DEV)            # accumulated into
    sqnorm = torch.tensor([5], dtype=torch.int64, device=DEV)
    assert mask_ndp(y, xd, xid, factor, limit, streams, counters, sqnorm, sigma, counter0=counter0) == 0, _C.last_error()
    torch.cuda.synchronize()
    fdev, fref = f32(NP(factor)[0]), X.clip_factor(x, xi, clip)
    assert abs(float(fdev) - float(fref)) <= 2 * float(np.spacing(fref)), (kind, n, fdev, fref)
    ref, sq_ref, counts_ref = restated(n, kind, fdev, streams, counter0)
    got = A.words_of(y)
    A.same_words(got[:nw], ref, "mask_narrow_dp(%s, k=%d, n=%d)" % (kind, k, n))
    assert np.all(got[nw:] == SENT), "written behind the padded words"
    sat, bad, exhausted = (int(v) for v in NP(counters))
    assert (sat - 1000, bad - 2000, exhausted - 3000) == counts_ref
    assert (int(sqnorm.item()) - 5) % 2 ** 64 == sq_ref
    return fdev, counts_ref, sq_ref


@pytest.mark.parametrize("n", W.SIZES)
@pytest.mark.parametrize("k", [0, 1, 3, 32])
def test_secagg_mask_narrow_dp_bit_identical_to_the_restatement(k, n):
    """packed words (codes at the device's clip factor + noise mod 2^16, under k signed streams), the three counters and the exact sum of
    the squared codes, all accumulated into non-zero values; a sentinel behind the n_pad / 2 words.  Planted blocks (NaN, +-inf,
    saturating, ties, all-zero: ddp_narrow_cases.inputs), a clip that binds, one that does not, and a zero update; sigma = 16 and 100.25"""
    f, (sat, bad, _), _ = check_case(n, k, "planted", counter0=3 if k == 3 else 0)
    assert f == (0.0 if n == 1 else 1.0) and (n > N.BLOCK or n == 4096 or sat + bad >= N.BLOCK)
    f, (sat, bad, _), sq = check_case(n, k, "binds")
    assert 0.4 < f < 0.6 and sat >= N.BLOCK // 2 and bad == 0 and 0 < sq <= W.delta_int(0.25, W.FRAC, n) ** 2
    f, (sat, bad, _), sq = check_case(n, k, "free")
    assert f == 1.0 and (sat, bad) == (0, 0) and sq > 0
    f, counts, sq = check_case(n, k, "zero")
    assert f == 1.0 and counts == (0, 0, 0) and sq == 0


# ---- 2. a zero update is the noise alone, on every padded coordinate ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4097])
def test_zero_update_without_streams_is_the_low_16_bits_of_dgauss_fill(n, sigma=16.0):
    """device against device: the fields are the low 16 bits of fedfr_dgauss_fill over ALL n_pad elements, so the padding carries noise"""
    x = G(np.random.default_rng(n).standard_normal(n).astype(f32))
    npad = N.padded_count(n)
    y = torch.full((npad // 2 + 8,), SENT, dtype=torch.int32, device=DEV)
    one = torch.ones(1, dtype=torch.float32, device=DEV)
    counters, sqnorm = torch.zeros(3, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    assert mask_ndp(y, x, x.clone(), one, 511, [], counters, sqnorm, sigma) == 0, _C.last_error()
    z = device_noise(npad, W.NOISE_SEED, W.NOISE_ROUND, 0, sigma)
    torch.cuda.synchronize()
    assert torch.equal(fields_t(y[:npad // 2]), z & 0xFFFF) and int((z != 0).sum()) > 0.9 * npad and int((z[n:] != 0).sum()) > 0.9 * (npad - n)
    assert np.all(A.words_of(y)[npad // 2:] == SENT) and NP(counters).tolist() == [0, 0, 0] and int(sqnorm.item()) == 0


# ---- 3. / 4. against the existing narrow kernel -------------------------------------------------------------------------------------------------
def check_against_narrow_kernel(xd, xid, clip, K, k, sigma, counter0):
    """with code_limit = 32767 // K: the new words are the field-wise sum of fedfr_secagg_mask_narrow's words (same seeds, streams, counter0)
    and the packed low halves of fedfr_dgauss_fill; composed with torch integer operations on the device, no numpy sampler involved"""
    n, npad = xd.numel(), N.padded_count(xd.numel())
    streams = S.some_streams(k)
    factor = device_factor(xd, xid, clip)
    coef = f32(NP(factor)[0]) * f32(2.0 ** W.FRAC)
    y = torch.full((npad // 2 + 8,), SENT, dtype=torch.int32, device=DEV)
    yn = torch.full((npad // 2 + 8,), SENT, dtype=torch.int32, device=DEV)
    cc, cn = torch.zeros(3, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    sq = torch.zeros(1, dtype=torch.int64, device=DEV)
    assert mask_ndp(y, xd, xid, factor, N.code_limit(K, 16), streams, cc, sq, sigma, counter0=counter0) == 0, _C.last_error()
    assert mask_narrow(yn, xd, xid, coef, K, streams, cn, counter0) == 0, _C.last_error()
    z = device_noise(npad, W.NOISE_SEED, W.NOISE_ROUND, 0, sigma)
    torch.cuda.synchronize()
    assert torch.equal(fields_t(y[:npad // 2]), (fields_t(yn[:npad // 2]) + z) & 0xFFFF), "words differ from narrow words (+) noise"
    assert torch.equal((fields_t(y[:npad // 2]) - z) & 0xFFFF, fields_t(yn[:npad // 2]))
    assert bool((y[npad // 2:] == SENT).all()) and NP(cc).tolist() == NP(cn).tolist() + [0]
    return int(sq.item()), f32(NP(factor)[0])


@pytest.mark.parametrize("kind", ["planted", "free"])
def test_words_minus_the_noise_are_the_narrow_kernels_words(kind, n=3 * 4096 + 17, K=5):
    x, xi, clip, _, sigma = W.inputs(n, kind)
    sq, f = check_against_narrow_kernel(G(x), G(xi), clip, K, 3, sigma, 7)
    assert sq == X._sq_mod64(W.codes(x, xi, f, W.FRAC, N.code_limit(K, 16), W.ROT_SEED, W.PRIV_SEED, W.RND)[0])


def test_past_one_grid_pass(n=2049 * 4096 + 5, K=4):
    """2050 rotation blocks on a grid of 2048 workgroups: the first two workgroups take a second block, the last of them ragged"""
    g = torch.Generator(device=DEV).manual_seed(9)
    x = torch.randn(n, generator=g, device=DEV) * 0.05
    xi = x + torch.randn(n, generator=g, device=DEV) * 1e-3
    sq, f = check_against_narrow_kernel(x, xi, 1.0, K, 1, 16.0, 0)
    assert 0.0 < f < 1.0 and 0 < sq <= W.delta_int(1.0, W.FRAC, n) ** 2      # ||xi - x|| is about 2.9: the clip binds


# ---- 5. stream coordinates ----------------------------------------------------------------------------------------------------------------------
def test_noise_stream_coordinates_and_null_counters(n=4097, kind="free"):
    """a non-zero noise_offset whose block index needs the high counter word, another round and another noise seed, each against the
    restatement; counters and sqnorm may be NULL; the noise moves with each coordinate and nothing else does"""
    x, xi, clip, limit, sigma = W.inputs(n, kind)
    xd, xid = G(x), G(xi)
    factor = device_factor(xd, xid, clip)
    streams, fdev = S.some_streams(3), None
    got = []
    for seed, nrnd, off in ((W.NOISE_SEED, W.NOISE_ROUND, 0), (W.NOISE_SEED, W.NOISE_ROUND, W.NOISE_OFFSET), (W.NOISE_SEED, W.NOISE_ROUND + 1, 0),
                            (W.NOISE_SEED + 1, W.NOISE_ROUND, 0)):
        y = torch.empty(N.padded_count(n) // 2, dtype=torch.int32, device=DEV)
        assert mask_ndp(y, xd, xid, factor, limit, streams, None, None, sigma, seed=seed, nrnd=nrnd, offset=off) == 0, _C.last_error()
        torch.cuda.synchronize()
        fdev = f32(NP(factor)[0])
        A.same_words(A.words_of(y), restated(n, kind, fdev, streams, 0, seed, nrnd, off)[0], "seed %x round %d offset %d" % (seed, nrnd, off))
        got.append(N.unpack(A.words_of(y), 16))
    for other in got[1:]:
        diff = (got[0] - other + 2 ** 15) % 2 ** 16 - 2 ** 15                         # two noise draws apart, nothing else
        assert np.mean(diff != 0) > 0.9 and np.abs(diff).max() <= 2 * X.TAIL * (int(sigma) + 1)


# ---- 6. the protocol on FlatStateDicts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K, T, dropped, opt", [(4, 3, (), None), (5, 3, (1, 3), None), (11, 6, (0, 4, 9, 10), "ADAM")])
def test_protocol_reproduces_the_restatement_and_the_masks_leave_no_trace(K, T, dropped, opt):
    """SecAggClient(bits=16).mask_dp -> SecAggServer.recovery_streams -> FedSecAggDP on the flat world of test_secagg_gpu.py: every upload
    is the restatement's words; the aggregate is x + rescale D 2^-6 H (S 2^-f), S the field-wise sum of codes and noise, bit for bit (past 8
    uploads and 32 recovery streams too, and through a server optimiser); and the same round run with every mask stream removed (the
    entry point at k = 0 with the clients' own seeds, no recovery streams) gives the same bits: the masks leave no trace"""
    glob, models, _ = A._flat_world(K)
    x, n = NP(glob.flat[0]), glob.flat[0].numel()
    rnd, frac, rot, npad = 9, 12, 0xABCD_0123_4567_89EF, N.padded_count(glob.flat[0].numel())
    mech = privacy.DistributedDiscreteGaussian(1.0, 0.1, frac, K, T, n, bits=16, wrap_sigmas=7)
    r = np.random.default_rng(11).bytes
    parts = list(range(K))
    clients = [secagg.SecAggClient(c, frac, r, 16, rot) for c in parts]
    srv = secagg.SecAggServer(parts, T, rnd)
    for c in clients:
        srv.register(c.cid, c.begin_round(rnd))
    for c in clients:
        srv.deliver_shares(c.cid, c.make_shares(parts, T))
    ups = [c.mask_dp(glob, m, parts, srv.public_keys, rnd, mech) for c, m in zip(clients, models)]
    torch.cuda.synchronize()
    assert len({c.noise_seed for c in clients}) == K and len({c.rounding_seed for c in clients}) == K
    noisy, bare, clipped = [], [], 0
    for c, m, u in zip(clients, models, ups):
        assert isinstance(u, secagg.MaskedUpdate) and (u.n, u.frac_bits, u.bits, u.rotation_seed, u.round) == (n, frac, 16, rot, rnd)
        assert u.y.numel() == npad // 2 and u.stats is m.flat[1] and u.counters is m.flat[2] and u.code_counters.numel() == 3
        assert u.nbytes == 2 * npad + 4 * 40 + 8 * 5 and u.dense_nbytes == 4 * n + 4 * 40 + 8 * 5
        assert (u.saturated_count(), u.nonfinite_count(), u.exhausted_count()) == (0, 0, 0)
        xi = NP(m.flat[0])
        factor = device_factor(glob.flat[0], m.flat[0], mech.clip_norm)
        fdev, fref = f32(NP(factor)[0]), X.clip_factor(x, xi, mech.clip_norm)
        assert abs(float(fdev) - float(fref)) <= 2 * float(np.spacing(fref))
        clipped += fdev < 1.0
        ref, sq, counts, amb = W.mask_narrow_dp(x, xi, fdev, frac, mech.code_limit, rot, c.rounding_seed, rnd, c.noise_seed, rnd, 0, mech.sigma_int,
                                                c.streams(parts, srv.public_keys, rnd))
        assert not amb.any(), "pick another seed: %d ambiguous decisions" % int(amb.sum())
        A.same_words(A.words_of(u.y), ref, "upload of client %d" % c.cid)
        assert u.sqnorm_value() == sq and 0 < sq <= mech.delta_int ** 2 and counts == (0, 0, 0)
        q = W.codes(x, xi, fdev, frac, mech.code_limit, rot, c.rounding_seed, rnd)[0]
        noisy.append(q.astype(i64) + W.noise(npad, c.noise_seed, rnd, 0, mech.sigma_int)[0])
        y0 = torch.empty(npad // 2, dtype=torch.int32, device=DEV)                # the same upload with all mask streams removed
        cc0, sq0 = torch.zeros(3, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
        assert mask_ndp(y0, glob.flat[0], m.flat[0], factor, mech.code_limit, [], cc0, sq0, mech.sigma_int, frac, rot, c.rounding_seed, rnd,
                        c.noise_seed, rnd) == 0, _C.last_error()
        A.same_words(A.words_of(y0), N.pack(noisy[-1], 16), "codes and noise of client %d in the clear" % c.cid)
        bare.append(secagg.MaskedUpdate(y0, n, frac, u.stats, u.counters, cc0, sqnorm=sq0, bits=16, rotation_seed=rot, round=rnd))
    assert 0 < clipped <= K                                      # the clip binds in this world
    keep = [p for p in parts if p not in dropped]
    rec = srv.recovery_streams(keep)
    assert (len(keep) > 8 or len(rec) > 32) == (K == 11)         # the last row chains passes
    rescale = float(f32(1.0 / len(keep)))
    total = sum(noisy[p] for p in keep)
    assert np.abs(total).max() <= 32767                          # nothing wraps in this world: kappa = 7
    sopt = None if opt is None else server.ServerOptimizer(opt, lr=0.01)
    sopt0 = None if opt is None else server.ServerOptimizer(opt, lr=0.01)
    out = server.FedSecAggDP(glob, [ups[p] for p in keep], rec, mech, sopt)
    out0 = server.FedSecAggDP(glob, [bare[p] for p in keep], [], mech, sopt0)
    avg = server.FedPavg([models[p] for p in keep], [1.0] * len(keep))
    torch.cuda.synchronize()
    assert isinstance(out, client.FlatStateDict) and torch.equal(out.flat[1], avg.flat[1]) and torch.equal(out.flat[2], avg.flat[2])
    assert torch.equal(out.flat[0], out0.flat[0]), "the masks left a trace"
    if sopt is None:
        A.T.same_bits(NP(out.flat[0]), N.decode_narrow(N.pack(total, 16), 16, frac, rescale, rot, rnd, n, x), "FedSecAggDP parameters")
    else:
        delta = G(N.decode_narrow(N.pack(total, 16), 16, frac, rescale, rot, rnd, n))
        twin = server.ServerOptimizer(opt, lr=sopt.lr)
        want = torch.empty_like(delta)
        twin.apply_delta(want, glob.flat[0], delta)
        torch.cuda.synchronize()
        A.T.same_bits(NP(out.flat[0]), NP(want), "FedSecAggDP through %s" % opt)
    with pytest.raises(ValueError, match="uploads, the mechanism needs"):
        server.FedSecAggDP(glob, ups[:T - 1], [], mech)
    with pytest.raises(ValueError, match="a mechanism of 32-bit words meets a client of 16-bit words"):
        clients[0].mask_dp(glob, models[0], parts, srv.public_keys, rnd, privacy.DistributedDiscreteGaussian(1.0, 0.1, 16, K, T, n))
    with pytest.raises(RuntimeError, match="16-bit words among uploads of 32-bit words"):
        server.FedSecAggDP(glob, [ups[p] for p in keep], rec, privacy.DistributedDiscreteGaussian(1.0, 0.1, frac, K, T, n))


# ---- 7. Server.train --------------------------------------------------------------------------------------------------------------------------------
Z, CLIP, FRAC, KAPPA, DELTA, ROT = 1.0, 1.0, 10, 7, 1e-5, 77


def _train(aggr, rounds, drop):
    extra = {} if drop is None else {"secagg_drop": drop}
    srv, clients = A._world3(aggr, secure_aggregation=True, secagg_bits=16, secagg_rotation_seed=ROT, distributed_dp=True, ddp_wrap_sigmas=KAPPA,
                             dp_noise_multiplier=Z, clip_norm=CLIP, secagg_frac_bits=FRAC, dp_delta=DELTA, server_lr=0.01, **extra)
    log = []
    for r in range(rounds):
        before = client.flat_state_dict(srv.federated_model).flat[0].clone()
        loss = srv.train()
        srv.step_round()
        torch.cuda.synchronize()
        assert np.isfinite(loss)
        log.append((before, [c.get_model().flat[0].clone() for c in clients], [(c.secagg.noise_seed, c.secagg.rounding_seed) for c in clients],
                    [t.clone() for t in srv.federated_model.flat_state()], srv.dp_epsilon, list(srv.dp_last_sqnorms)))
    return srv, log


@pytest.mark.parametrize("aggr, rounds, drop", [("FedAvg", 2, None), ("FedAdam", 1, None), ("FedAvg", 1, [1])])
def test_server_train_with_distributed_dp_at_16_bits(aggr, rounds, drop, caplog, monkeypatch):
    """Server.train(secagg_bits=16, distributed_dp=True, ddp_wrap_sigmas=7) on the tiny closed-form world: the model moves; the parameters
    are the restatement applied to the clients' trained states (device clip factor, rotated and stochastically rounded codes, the noise of
    fedfr_dgauss_fill over n_pad elements at each client's own seed, the field-wise sum mod 2^16, the rotation turned back, the mean over
    the uploads that arrived; through the server optimiser for FedAdam) bit for bit; the accountant steps at the mechanism's z_eff; every
    survivor's sum of squared codes is within delta_int^2; an upload is 2 n_pad bytes of packed words; the log names the width and
    wrap_bound"""
    import logging
    rec, real = [], server.FedSecAggDP
    monkeypatch.setattr(server, "FedSecAggDP", lambda *a, **k: (rec.append(a[1]), real(*a, **k))[1])
    with caplog.at_level(logging.INFO, logger="FL_face.server"):
        srv, log = _train(aggr, rounds, drop)
    keep = [i for i in range(3) if i not in (drop or [])]
    n = log[0][0].numel()
    npad, T = N.padded_count(n), 2                               # (the default threshold of three clients)
    mech = privacy.DistributedDiscreteGaussian(Z, CLIP, FRAC, 3, T, n, bits=16, wrap_sigmas=KAPPA)
    assert mech.delta_int == pytest.approx(W.delta_int(CLIP, FRAC, n), rel=1e-12) and mech.sigma_int == Z * CLIP * 2.0 ** FRAC / math.sqrt(T)
    assert mech.code_limit == (32767 - math.ceil(KAPPA * mech.sigma_int * math.sqrt(3))) // 3
    text = caplog.text
    assert "Distributed differential privacy" in text and ("z_eff = %.6g" % mech.z_eff) in text and "accounted at q = 1" in text
    assert "Masked uploads (%d fraction bits, threshold 2, 16-bit words)" % FRAC in text
    assert "at 16-bit words: %d bytes of packed words per upload" % (2 * npad) in text and ("wrap_bound = %.3g" % mech.wrap_bound) in text
    assert "kappa = %g" % KAPPA in text and "coordinate_sigmas" in text and "saturated codes among the %d uploads" % len(keep) in text
    assert len(rec) == rounds
    for ups in rec:
        assert len(ups) == len(keep)
        for u in ups:
            assert u.bits == 16 and u.y.numel() == npad // 2 and u.nbytes == 2 * npad + u.stats.numel() * 4 + u.counters.numel() * 8
            assert u.exhausted_count() == 0 and u.nonfinite_count() == 0
    twin = server.ServerOptimizer("ADAM", lr=0.01) if aggr == "FedAdam" else None
    L = mech.code_limit
    for r, (x, xs, seeds, after, eps, sqnorms) in enumerate(log):
        assert eps == pytest.approx(D.epsilon_by_hand(1.0, mech.z_eff, r + 1, DELTA), rel=1e-9)
        assert len(sqnorms) == len(keep) and all(0 < v <= mech.delta_int ** 2 for v in sqnorms)
        assert not torch.equal(after[0], x)
        total = torch.zeros(npad, dtype=torch.int64, device=DEV)
        signs = NG._sign_bits_t(npad, ROT, r)
        for pos, i in enumerate(keep):
            coef = device_factor(x, xs[i], CLIP) * float(2.0 ** FRAC)
            u = torch.zeros(npad, dtype=torch.float32, device=DEV)
            u[:n] = xs[i] - x
            t = NG._butterfly_t(torch.where(signs, -u, u)) * coef
            assert t.dtype == torch.float32 and bool(torch.isfinite(t).all())
            fl = torch.floor(t)
            draw = (NG._philox_words(npad, seeds[i][1], r, N.ROUND_SID) >> 8).to(torch.float32) * float(2.0 ** -24)
            q = (fl.to(torch.int64) + (draw < t - fl).to(torch.int64)).clamp(-L, L)
            assert int((q * q).sum()) == sqnorms[pos] and int((q.abs() == L).sum()) == rec[r][pos].saturated_count()
            total += q + device_noise(npad, seeds[i][0], r, 0, mech.sigma_int)
        S16 = (total + 2 ** 15) % 2 ** 16 - 2 ** 15                             # the field-wise sum mod 2^16, sign-extended
        d = NG._butterfly_t(S16.to(torch.float32) * float(2.0 ** -FRAC))
        d = torch.where(signs, -d, d)[:n] * float(f32(1.0 / len(keep)))
        if twin is None:
            assert torch.equal(after[0], x + d), "round %d: parameters differ from the restatement" % r
        else:
            want = torch.empty_like(x)
            twin.apply_delta(want, x, d)
            assert torch.equal(after[0], want), "round %d: parameters differ from the restatement through FedAdam" % r
    assert srv.dp_accountant.steps == rounds and (srv.dp_accountant.q, srv.dp_accountant.sigma) == (1.0, pytest.approx(mech.z_eff, rel=1e-12))
