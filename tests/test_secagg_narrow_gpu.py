"""Narrow secure aggregation on the GPU: fedfr_rht_fill, fedfr_secagg_mask_narrow and fedfr_secagg_aggregate_narrow against the restatements of
tests/secagg_narrow_cases.py, BIT FOR BIT (words, codes, counters and the fp32 output: the rotation's level order is part of the format, and
everything between the encoder and the decoder is field-wise integer arithmetic), at one padded block, exact blocks and a ragged tail;
chaining, in-place update, the counter refusal; and the Python surface (SecAggClient(bits=...), FedSecAgg, Server.train with secagg_bits)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dp_cases as D  # noqa: E402
import secagg_cases as S  # noqa: E402
import secagg_narrow_cases as N  # noqa: E402
import test_fedopt_gpu as T  # noqa: E402   (device helpers: helpers, not tests)
import test_secagg_gpu as G32  # noqa: E402   (the 32-bit path's helpers and tiny worlds: helpers, not tests)

from fedfr_amd import _C, client, secagg, server  # noqa: E402

DEV = torch.device("cuda:0")
f32, f64, u32, i32, i64 = np.float32, np.float64, np.uint32, np.int32, np.int64
ROT_SEED, PRIV_SEED, RND = 0xC0FFEE_0000_0001, 0xFEED_FACE_CAFE_BEEF, 6
ERR_ARG = -1
G, NP, ptr = T.G, T.N, T.ptr
arrays, words_of, same_words = G32.arrays, G32.words_of, G32.same_words
FRAC = {8: 8, 16: 14}                        # fraction bits that keep the planted worlds inside the code range of each width


def rht_fill(dst, src, n, inverse=0, seed=ROT_SEED, rnd=RND):
    return _C.lib().fedfr_rht_fill(ptr(dst), ptr(src), n, seed, rnd, inverse, _C.stream())


def mask(y, x, xi, coef, K, bits, streams, counters=None, counter0=0, priv=PRIV_SEED, n=None):
    return _C.lib().fedfr_secagg_mask_narrow(ptr(y), ptr(x), ptr(xi), float(coef), K, bits, ROT_SEED, priv, RND, *arrays(streams), len(streams), counter0,
                                             x.numel() if n is None else n, ptr(counters), _C.stream())


def aggregate(out, x, acc, ys, bits, streams, n, frac_bits, rescale=1.0, first=1, last=1, counter0=0):
    ptrs = (C.c_void_p * max(len(ys), 1))(*[t.data_ptr() for t in ys])
    return _C.lib().fedfr_secagg_aggregate_narrow(ptr(out), ptr(x), ptr(acc), ptrs, len(ys), bits, ROT_SEED, RND, *arrays(streams), len(streams), counter0,
                                                  frac_bits, float(rescale), n, first, last, _C.stream())


def words(n, bits):
    return N.padded_count(n) * bits // 32


def sent_words(n):
    return torch.full((n,), G32.SENT, dtype=torch.int32, device=DEV)


# ---- the rotation alone ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rot_input(n):
    g = np.random.default_rng(n)
    u = (g.standard_normal(n) * np.exp(g.standard_normal(n))).astype(f32)
    u.flags.writeable = False
    return u


@pytest.mark.parametrize("n", N.SIZES)
def test_rht_fill_bit_identical_to_the_restatement(n):
    u, npad = rot_input(n), N.padded_count(n)
    fwd, back = T.sent(npad + 4), T.sent(npad + 4)
    assert rht_fill(fwd, G(u), n) == 0, _C.last_error()
    ref = N.rotate32(u, ROT_SEED, RND)
    T.same_bits(NP(fwd)[:npad], ref, "rotation, n=%d" % n)
    assert np.all(NP(fwd)[npad:].view(u32) == T.F.bits(np.full(4, T.SENT, f32)))
    assert rht_fill(back, fwd, npad, 1) == 0, _C.last_error()
    T.same_bits(NP(back)[:npad], N.rotate_back32(ref, ROT_SEED, RND), "rotation back, n=%d" % n)
    norms = np.sqrt((N.pad32(u).astype(f64) ** 2).reshape(-1, N.BLOCK).sum(axis=1))
    assert np.all(np.abs(NP(back)[:npad].astype(f64) - N.pad32(u)) <= np.repeat(N.ROTATION_BOUND * norms, N.BLOCK))


def test_rht_fill_depends_on_seed_and_round_only_through_the_signs():
    n = N.BLOCK
    u = rot_input(n)
    outs = []
    for seed, rnd in ((ROT_SEED, RND), (ROT_SEED + 1, RND), (ROT_SEED, RND + 1)):
        o = T.sent(n)
        assert rht_fill(o, G(u), n, 0, seed, rnd) == 0, _C.last_error()
        T.same_bits(NP(o), N.rotate32(u, seed, rnd), "seed %x round %d" % (seed, rnd))
        outs.append(NP(o))
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[0], outs[2])


# ---- the masked upload -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(n, K, bits, first=0):
    """(x, xi, coef) with the planted blocks of secagg_narrow_cases.planted_inputs (ordinary, ties, non-finite, saturating, all-zero), read-only"""
    coef = S.code_coef(1.0, FRAC[bits])
    x, xi = N.planted_inputs(n, coef, N.code_limit(K, bits), first)
    x.flags.writeable = xi.flags.writeable = False
    return x, xi, coef


def run_mask(n, K, bits, streams, first=0, counter0=0):
    x, xi, coef = inputs(n, K, bits, first)
    nw = words(n, bits)
    y, cc = sent_words(nw + 4), torch.zeros(2, dtype=torch.int32, device=DEV)
    assert mask(y, G(x), G(xi), coef, K, bits, streams, cc, counter0) == 0, _C.last_error()
    ref, sat, bad, q = N.mask_narrow(x, xi, coef, K, bits, ROT_SEED, PRIV_SEED, RND, streams, counter0)
    got = words_of(y)
    assert np.all(got[nw:] == G32.SENT), "written behind the padded words"
    return got[:nw], NP(cc), ref, sat, bad, q


@pytest.mark.parametrize("n", N.SIZES)
@pytest.mark.parametrize("K, k", [(2, 0), (3, 1), (32, 32)])
@pytest.mark.parametrize("bits", [8, 16])
def test_secagg_mask_narrow_bit_identical_to_the_restatement(bits, K, k, n):
    """words and counters; with k = 0 streams the words are the packed codes in the clear.  The blocks of the largest size are ordinary,
    ties, non-finite and saturating; the other sizes start at another kind each, so that every kind also meets a padded block"""
    first = N.SIZES.index(n)
    got, cc, ref, sat, bad, q = run_mask(n, K, bits, S.some_streams(k), first)
    same_words(got, ref, "mask_narrow bits=%d K=%d k=%d n=%d" % (bits, K, k, n))
    assert (int(cc[0]), int(cc[1])) == (sat, bad)
    if k == 0:
        assert np.array_equal(N.unpack(got, bits), q) and np.abs(q).max() <= N.code_limit(K, bits)
    kinds = {N.KINDS[(b + first) % 5] for b in range(N.padded_count(n) // N.BLOCK)}
    if "nonfinite" in kinds:
        assert bad >= N.BLOCK
    if "saturating" in kinds:
        assert sat >= N.BLOCK


def test_secagg_mask_narrow_stream_coordinates():
    """a counter0 moves the mask stream and nothing else; the private seed moves the rounding and nothing else; a counter0 whose last block
    would pass 2^32 - 1 is refused and nothing is written"""
    n, K, bits = 4097, 3, 8
    streams = S.some_streams(2)
    c0 = 0xFFFFFFFF - 127                                        # two rotation blocks of 64 ChaCha20 blocks: the last one is block 2^32 - 1
    got, _, ref, _, _, q = run_mask(n, K, bits, streams, 0, c0)
    same_words(got, ref, "counter0 at the end of the range")
    plain, _, _, _, _, q0 = run_mask(n, K, bits, [], 0)
    assert np.array_equal(q, q0)
    same_words(N.field_sub(got, N.stream_sum_fields(got.size, streams, bits, c0), bits), plain, "the masks removed")
    x, xi, coef = inputs(n, K, bits)
    y = sent_words(words(n, bits))
    assert mask(y, G(x), G(xi), coef, K, bits, streams, None, c0 + 1) == ERR_ARG and "overflows" in _C.last_error()
    torch.cuda.synchronize()
    assert np.all(words_of(y) == G32.SENT)
    y2 = sent_words(words(n, bits))
    assert mask(y2, G(x), G(xi), coef, K, bits, [], None, 0, PRIV_SEED + 1) == 0, _C.last_error()
    same_words(words_of(y2), N.mask_narrow(x, xi, coef, K, bits, ROT_SEED, PRIV_SEED + 1, RND, [])[0], "another private seed")
    assert not np.array_equal(words_of(y2), plain)


def test_secagg_mask_narrow_past_one_grid_pass():
    """2049 rotation blocks: one more than the launch rule's 2048 workgroups, so one workgroup takes a second block"""
    n, K, bits = 2049 * N.BLOCK - 5, 8, 8
    g = np.random.default_rng(1)
    x = np.zeros(n, f32)
    xi = (g.standard_normal(n) * 0.02).astype(f32)
    coef = S.code_coef(1.0, FRAC[bits])
    streams = S.some_streams(1)
    y, cc = sent_words(words(n, bits)), torch.zeros(2, dtype=torch.int32, device=DEV)
    assert mask(y, G(x), G(xi), coef, K, bits, streams, cc) == 0, _C.last_error()
    ref, sat, bad, _ = N.mask_narrow(x, xi, coef, K, bits, ROT_SEED, PRIV_SEED, RND, streams)
    same_words(words_of(y), ref, "mask_narrow over 2049 blocks")
    assert (int(cc[0]), int(cc[1])) == (sat, bad)


# ---- the aggregate -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def uploads(n, bits, ku):
    """ku uploads of arbitrary words (any word is a possible masked upload) and a base state, read-only"""
    g = np.random.default_rng(n + bits + ku)
    ys = tuple(g.integers(0, 2 ** 32, words(n, bits), dtype=np.uint64).astype(u32) for _ in range(ku))
    x = (g.standard_normal(n) * 0.05).astype(f32)
    for a in ys + (x,):
        a.flags.writeable = False
    return ys, x


def dev_words(w):
    return torch.from_numpy(w.view(i32).copy()).to(DEV)


@pytest.mark.parametrize("n", N.SIZES)
@pytest.mark.parametrize("ku, k", [(1, 0), (3, 5), (8, 32), (0, 3)])
@pytest.mark.parametrize("bits", [8, 16])
def test_secagg_aggregate_narrow_bit_identical_to_the_restatement(bits, ku, k, n):
    ys, x = uploads(n, bits, ku)
    streams = S.some_streams(k, seed=2)
    out = T.sent(n + 4)
    assert aggregate(out, G(x), None, [dev_words(y) for y in ys], bits, streams, n, FRAC[bits], 1.25) == 0, _C.last_error()
    ref = N.aggregate_narrow(x, list(ys), streams, bits, FRAC[bits], 1.25, ROT_SEED, RND, n)
    T.same_bits(NP(out)[:n], ref, "aggregate_narrow bits=%d ku=%d k=%d n=%d" % (bits, ku, k, n))
    assert np.all(NP(out)[n:].view(u32) == T.F.bits(np.full(4, T.SENT, f32))), "written behind n"


@pytest.mark.parametrize("bits", [8, 16])
def test_secagg_aggregate_narrow_without_x_in_place_and_chained(bits):
    """x = NULL gives the update alone; out == x updates in place; 9 uploads and 40 streams chain two launches through acc, whose words are
    the field-wise partial sum, and give the bits of the one-pass restatement"""
    n, f = 3 * N.BLOCK + 17, FRAC[bits]
    ys, x = uploads(n, bits, 9)
    streams = S.some_streams(40, seed=5)
    dys = [dev_words(y) for y in ys]
    ref = N.aggregate_narrow(x, list(ys), streams, bits, f, 1.0, ROT_SEED, RND, n)
    ref_d = N.aggregate_narrow(None, list(ys), streams, bits, f, 1.0, ROT_SEED, RND, n)
    nw = words(n, bits)
    for out_is_x, with_x in ((False, True), (True, True), (False, False)):
        acc = sent_words(nw)
        xd = G(x)
        out = xd if out_is_x else T.sent(n)
        assert aggregate(None, None, acc, dys[:8], bits, streams[:32], n, f, 1.0, 1, 0) == 0, _C.last_error()
        part = N.field_add(functools.reduce(lambda a, b: N.field_add(a, b, bits), ys[:8]), N.stream_sum_fields(nw, streams[:32], bits), bits)
        same_words(words_of(acc), part, "acc after the first pass")
        assert aggregate(out, xd if with_x else None, acc, dys[8:], bits, streams[32:], n, f, 1.0, 0, 1) == 0, _C.last_error()
        T.same_bits(NP(out), ref if with_x else ref_d, "chained, out is x: %s, with x: %s" % (out_is_x, with_x))
        same_words(words_of(acc), part, "acc is not written by the last pass")
    # the order of the passes does not matter: streams first, uploads last
    acc, out = sent_words(nw), T.sent(n)
    assert aggregate(None, None, acc, [], bits, streams[:32], n, f, 1.0, 1, 0) == 0, _C.last_error()
    assert aggregate(None, None, acc, dys[:8], bits, streams[32:], n, f, 1.0, 0, 0) == 0, _C.last_error()
    assert aggregate(out, G(x), acc, dys[8:], bits, [], n, f, 1.0, 0, 1) == 0, _C.last_error()
    T.same_bits(NP(out), ref, "three passes in another order")
    # and a counter0 past the range is refused with nothing written
    out = T.sent(n)
    assert aggregate(out, G(x), None, dys[:1], bits, streams[:1], n, f, 1.0, 1, 1, 0xFFFFFFFF - 4 * (64 if bits == 8 else 128) + 2) == ERR_ARG
    assert "overflows" in _C.last_error()
    torch.cuda.synchronize()
    assert np.all(NP(out).view(u32) == T.F.bits(np.full(n, T.SENT, f32)))


@pytest.mark.parametrize("bits, K, dropped", [(8, 3, (1,)), (16, 5, (0, 3)), (8, 32, ())])
def test_masks_leave_no_trace_in_the_narrow_aggregate(bits, K, dropped):
    """K clients mask on the device under the protocol's streams; the aggregate over the survivors with the recovery streams is the decoded
    sum of their plain codes, bit for bit: the masks cancel field-wise"""
    n, f, rnd, t = 4097, FRAC[bits], RND, K // 2 + 1
    g = np.random.default_rng(K)
    x = (g.standard_normal(n) * 0.05).astype(f32)
    xs = [(x + g.standard_normal(n).astype(f32) * f32(2e-3)).astype(f32) for _ in range(K)]
    parts = [3 * c + 1 for c in range(K)]
    r = np.random.default_rng(11).bytes
    clients = [secagg.SecAggClient(c, 12, r, bits, ROT_SEED) for c in parts]
    srv = secagg.SecAggServer(parts, t, rnd)
    for c in clients:
        srv.register(c.cid, c.begin_round(rnd))
    for c in clients:
        srv.deliver_shares(c.cid, c.make_shares(parts, t))
    coef = S.code_coef(1.0 / K, f)
    xd, ys, codes = G(x), [], []
    for c, xi in zip(clients, xs):
        y = sent_words(words(n, bits))
        assert mask(y, xd, G(xi), coef, K, bits, c.streams(parts, srv.public_keys, rnd), None, 0, c.rounding_seed) == 0, _C.last_error()
        ys.append(y)
        codes.append(N.codes_narrow(x, xi, coef, K, bits, ROT_SEED, c.rounding_seed, RND)[0].astype(i64))
    keep = [p for p in range(K) if p not in dropped]
    rec = srv.recovery_streams([parts[p] for p in keep])
    nw = words(n, bits)
    acc = sent_words(nw)
    out = T.sent(n)
    passes = max((len(keep) + 7) // 8, (len(rec) + 31) // 32)
    for p in range(passes):
        assert aggregate(out, xd, acc, [ys[q] for q in keep[8 * p:8 * p + 8]], bits, rec[32 * p:32 * p + 32], n, f, 1.0, int(p == 0),
                         int(p == passes - 1)) == 0, _C.last_error()
    want = N.decode_narrow(N.pack(sum(codes[p] for p in keep), bits), bits, f, 1.0, ROT_SEED, RND, n, x)
    T.same_bits(NP(out), want, "aggregate over the survivors")
    for p in keep[:3]:
        assert np.count_nonzero(words_of(ys[p]) == N.pack(codes[p], bits)) == 0      # an upload says nothing about its codes
    mean = x.astype(f64) + sum((xs[p].astype(f64) - x) / K for p in keep)
    assert np.abs(NP(out) - mean).max() < 6 * np.sqrt(len(keep)) * 0.5 * 2.0 ** -f + 1e-6


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits, K, dropped, opt", [(8, 3, (), None), (16, 3, (1,), None), (8, 11, (0, 4, 9, 10), None), (16, 11, (0, 4, 9, 10), "ADAM")])
def test_fedsecagg_narrow_reproduces_the_restatement(bits, K, dropped, opt):
    """SecAggClient(bits=...).mask -> SecAggServer.recovery_streams -> FedSecAgg on FlatStateDicts: the parameters are the restatement's
    bits, also past 8 uploads and 32 recovery streams and through a server optimiser; statistics and counters are FedPavg's"""
    glob, models, sizes = G32._flat_world(K)
    x, n = NP(glob.flat[0]), glob.flat[0].numel()
    rnd, t, f = 9, K // 2 + 1, 12 if bits == 8 else 20
    parts = list(range(K))
    r = np.random.default_rng(11).bytes
    clients = [secagg.SecAggClient(c, f, r, bits, ROT_SEED) for c in parts]
    srv = secagg.SecAggServer(parts, t, rnd)
    for c in clients:
        srv.register(c.cid, c.begin_round(rnd))
    for c in clients:
        srv.deliver_shares(c.cid, c.make_shares(parts, t))
    w = [s / sum(sizes) for s in sizes]
    ups = [c.mask(glob, m, wi, parts, srv.public_keys, rnd) for c, m, wi in zip(clients, models, w)]
    torch.cuda.synchronize()
    for u, m in zip(ups, models):
        assert u.bits == bits and u.y.numel() == words(n, bits) and (u.rotation_seed, u.round) == (ROT_SEED, rnd)
        assert u.nbytes == N.padded_count(n) * bits // 8 + 4 * 40 + 8 * 5 and u.dense_nbytes == 4 * n + 4 * 40 + 8 * 5
    refs = [N.mask_narrow(x, NP(m.flat[0]), S.code_coef(wi, f), K, bits, ROT_SEED, c.rounding_seed, rnd, c.streams(parts, srv.public_keys, rnd))
            for c, m, wi in zip(clients, models, w)]
    same_words(words_of(ups[1].y), refs[1][0], "upload of client 1")
    assert (ups[1].saturated_count(), ups[1].nonfinite_count()) == refs[1][1:3]
    keep = [p for p in parts if p not in dropped]
    rescale = secagg.survivor_rescale(w, keep)
    rec = srv.recovery_streams(keep)
    sopt = None if opt is None else server.ServerOptimizer(opt, lr=0.01)
    out = server.FedSecAgg(glob, [ups[p] for p in keep], [sizes[p] for p in keep], rec, rescale, sopt, bits=bits)
    avg = server.FedPavg([models[p] for p in keep], [sizes[p] for p in keep])
    torch.cuda.synchronize()
    assert torch.equal(out.flat[1], avg.flat[1]) and torch.equal(out.flat[2], avg.flat[2])
    total = N.pack(sum(refs[p][3].astype(i64) for p in keep), bits)
    if sopt is None:
        T.same_bits(NP(out.flat[0]), N.decode_narrow(total, bits, f, rescale, ROT_SEED, rnd, n, x), "FedSecAgg parameters")
    else:
        delta = G(N.decode_narrow(total, bits, f, rescale, ROT_SEED, rnd, n))
        twin = server.ServerOptimizer(opt, lr=sopt.lr)
        want = torch.empty_like(delta)
        twin.apply_delta(want, glob.flat[0], delta)
        torch.cuda.synchronize()
        T.same_bits(NP(out.flat[0]), NP(want), "FedSecAgg through %s" % opt)
    with pytest.raises(RuntimeError, match="the server expects"):
        server.FedSecAgg(glob, [ups[p] for p in keep], [sizes[p] for p in keep], rec, rescale, None, bits=32)
    with pytest.raises(RuntimeError, match="rotated with"):
        other = secagg.MaskedUpdate(ups[keep[0]].y, n, f, ups[keep[0]].stats, ups[keep[0]].counters, ups[keep[0]].code_counters, bits=bits,
                                    rotation_seed=ROT_SEED + 1, round=rnd)
        server.FedSecAgg(glob, [ups[keep[1]], other], [1.0, 1.0], [], 1.0, None)


# ---- Server.train ------------------------------------------------------------------------------------------------------------------------
def _philox_words(n, seed, rnd, sid):
    """words 0 ... n - 1 of a Philox stream as an int64 device tensor (fedfr_philox_fill: held to dp_cases.words by tests/test_dp_gpu.py)"""
    w = torch.empty((n + 3) // 4 * 4, dtype=torch.int32, device=DEV)
    assert _C.lib().fedfr_philox_fill(w.data_ptr(), w.numel(), seed, rnd, sid, 0, _C.stream()) == 0, _C.last_error()
    return w[:n].to(torch.int64) & 0xFFFFFFFF


def _butterfly_t(v):
    h = 1
    while h < N.BLOCK:
        w = v.reshape(-1, N.BLOCK // (2 * h), 2, h)
        a, b = w[:, :, 0, :], w[:, :, 1, :]
        v = torch.stack([a + b, a - b], dim=2).reshape(-1, N.BLOCK)
        h *= 2
    return v.reshape(-1) * float(2.0 ** -6)


def _sign_bits_t(npad, seed, rnd):
    w = _philox_words(npad // 32, seed, rnd, N.SIGN_SID)
    return ((w[:, None] >> torch.arange(32, device=DEV)[None, :]) & 1).bool().reshape(-1)


def _codes_on_device(x, xi, w, K, bits, frac_bits, rot_seed, priv_seed, rnd):
    """secagg_narrow_cases.codes_narrow in torch, one fp32 operation per line (eager torch rounds each once): the states of a network are too
    long for the numpy restatement to stay quick"""
    n, npad, L = x.numel(), N.padded_count(x.numel()), N.code_limit(K, bits)
    u = torch.zeros(npad, dtype=torch.float32, device=DEV)
    u[:n] = xi - x
    u = torch.where(_sign_bits_t(npad, rot_seed, rnd), -u, u)
    t = _butterfly_t(u) * float(S.code_coef(w, frac_bits))
    assert t.dtype == torch.float32 and bool(torch.isfinite(t).all())
    fl = torch.floor(t)
    frac = t - fl
    r = (_philox_words(npad, priv_seed, rnd, N.ROUND_SID) >> 8).to(torch.float32) * float(2.0 ** -24)
    q = (fl.to(torch.int64) + (r < frac).to(torch.int64)).clamp(-L, L)
    return q, int((q.abs() == L).sum())


def _decode_on_device(total, x, frac_bits, rescale, rot_seed, rnd):
    s = total.to(torch.float32) * float(2.0 ** -frac_bits)
    d = _butterfly_t(s)
    d = torch.where(_sign_bits_t(total.numel(), rot_seed, rnd), -d, d)[:x.numel()] * float(f32(rescale))
    return x + d


def test_the_device_restatement_is_the_numpy_restatement():
    """the torch helpers of the Server.train test against secagg_narrow_cases on a small state, so that test stands on the numpy restatement"""
    n, K, bits, f = 4097, 3, 8, 10
    g = np.random.default_rng(0)
    x = (g.standard_normal(n) * 0.05).astype(f32)
    xi = (x + g.standard_normal(n).astype(f32) * f32(5e-3)).astype(f32)
    q, sat = _codes_on_device(G(x), G(xi), 0.4, K, bits, f, ROT_SEED, PRIV_SEED, RND)
    ref, rsat, _ = N.codes_narrow(x, xi, S.code_coef(0.4, f), K, bits, ROT_SEED, PRIV_SEED, RND)
    assert np.array_equal(NP(q), ref) and sat == rsat
    T.same_bits(NP(_decode_on_device(q, G(x), f, 1.5, ROT_SEED, RND)), N.decode_narrow(N.pack(ref, bits), bits, f, 1.5, ROT_SEED, RND, n, x), "decode")


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("drop", [None, [1]])
def test_server_train_with_narrow_secure_aggregation(bits, drop, caplog, monkeypatch):
    """Server.train(secure_aggregation=True, secagg_bits=8 or 16) on the tiny closed-form world: the global parameters are the restatement
    applied to the clients' trained states, bit for bit; an upload is n_pad b / 8 bytes plus the statistics in the clear; statistics and
    counters are FedPavg's over the clients whose upload arrived"""
    import logging
    f, seed = FRAC[bits] + 4, 77
    extra = {} if drop is None else {"secagg_drop": drop}
    srv, clients = G32._world3("FedAvg", secure_aggregation=True, secagg_bits=bits, secagg_frac_bits=f, secagg_rotation_seed=seed, **extra)
    rec, real = [], server.FedSecAgg
    monkeypatch.setattr(server, "FedSecAgg", lambda *a, **k: (rec.append((a[1], k, real(*a, **k))), rec[-1][2])[1])
    sizes = [300.0, 100.0, 250.0]
    keep = [i for i in range(3) if i not in (drop or [])]
    before = [t.clone() for t in client.flat_state_dict(srv.federated_model).flat]
    with caplog.at_level(logging.INFO, logger="FL_face.server"):
        assert np.isfinite(srv.train())
    srv.step_round()
    torch.cuda.synchronize()
    assert "Masked uploads (%d fraction bits, threshold 2, %d-bit words)" % (f, bits) in caplog.text
    x, n = before[0], before[0].numel()
    ups, kwargs, out = rec[0]
    assert kwargs == {"bits": bits} and len(ups) == len(keep)
    for u in ups:
        assert u.bits == bits and u.nbytes == N.padded_count(n) * bits // 8 + u.stats.numel() * 4 + u.counters.numel() * 8
        assert u.nbytes < u.dense_nbytes * (bits / 32 + 0.01)
    assert "%d bytes from 3 clients" % (3 * ups[0].nbytes) in caplog.text
    models = [clients[i].get_model() for i in keep]
    w = [s / sum(sizes) for s in sizes]
    rescale = secagg.survivor_rescale(w, keep)
    total = torch.zeros(N.padded_count(n), dtype=torch.int64, device=DEV)
    for i, m, u in zip(keep, models, ups):
        assert clients[i].secagg.bits == bits and clients[i].secagg.rotation_seed == seed
        q, sat = _codes_on_device(x, m.flat[0], w[i], 3, bits, f, seed, clients[i].secagg.rounding_seed, 0)
        assert (u.saturated_count(), u.nonfinite_count()) == (sat, 0)
        total += q
    got = srv.federated_model.flat_state()
    avg = server.FedPavg(models, [sizes[i] for i in keep])
    assert torch.equal(got[1], avg.flat[1]) and torch.equal(out.flat[2], avg.flat[2]) and torch.equal(got[0], out.flat[0])
    assert torch.equal(got[0], _decode_on_device(total, x, f, rescale, seed, 0)), "parameters differ from the restatement"


@pytest.mark.parametrize("setting", [{}, {"secagg_bits": 32}, {"secagg_bits": None}])
def test_server_train_at_32_bits_is_the_path_of_one_word_per_parameter(setting, caplog, monkeypatch):
    """absent, None or 32: FedSecAgg is called argument for argument as before (no keyword), the uploads are 32-bit words and the parameters
    are the 32-bit restatement's bits"""
    import logging
    srv, clients = G32._world3("FedAvg", secure_aggregation=True, **setting)
    rec, real = [], server.FedSecAgg
    monkeypatch.setattr(server, "FedSecAgg", lambda *a: (rec.append((a[1], real(*a))), rec[-1][1])[1])
    sizes = [300.0, 100.0, 250.0]
    before = [t.clone() for t in client.flat_state_dict(srv.federated_model).flat]
    with caplog.at_level(logging.INFO, logger="FL_face.server"):
        assert np.isfinite(srv.train())
    torch.cuda.synchronize()
    assert "Masked uploads (24 fraction bits, threshold 2):" in caplog.text
    x = before[0]
    assert all(u.bits == 32 and u.y.numel() == x.numel() and u.nbytes == u.dense_nbytes for u in rec[0][0])
    assert all(c.secagg.bits == 32 and c.secagg.rounding_seed is None for c in clients)
    w = [s / sum(sizes) for s in sizes]
    delta = G32._delta_on_device(x, [c.get_model().flat[0] for c in clients], w, 3, 24, 1.0)
    assert torch.equal(srv.federated_model.flat_state()[0], x + delta)
