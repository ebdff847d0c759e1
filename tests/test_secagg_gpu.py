"""Secure aggregation on the GPU: fedfr_chacha20_fill, fedfr_secagg_mask and fedfr_secagg_aggregate against the restatements of
tests/secagg_cases.py (bit for bit: everything between the fp32 encoding and the final conversion is integer arithmetic), chaining,
in-place update, the end-to-end property on raw tensors (the masks leave no trace in the aggregate, and no trace of the codes in an
upload) with and without dropped clients, and the Python surface (secagg.SecAggClient / SecAggServer, server.FedSecAgg, Server.train with
secure_aggregation)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import secagg_cases as S  # noqa: E402
import test_fedopt_gpu as T  # noqa: E402   (its device helpers and closed-form tiny world: helpers, not tests)

from fedfr_amd import _C, client, secagg, server  # noqa: E402
from oracle import ref_cpu as R  # noqa: E402

DEV = torch.device("cuda:0")
f32, f64, u32, i32 = np.float32, np.float64, np.uint32, np.int32
SENT = 0x5A5A5A5A
FRAC = 24
KEY2 = tuple((0x9E3779B9 * (q + 1)) & 0xFFFFFFFF for q in range(8))
NONCE2 = (7, 0x80000001, 1)

G, N, ptr = T.G, T.N, T.ptr


def arrays(streams):
    k = len(streams)
    keys = (C.c_uint * max(8 * k, 1))(*[w for s in streams for w in s[0]])
    nonces = (C.c_uint * max(3 * k, 1))(*[w for s in streams for w in s[1]])
    signs = (C.c_int * max(k, 1))(*[s[2] for s in streams])
    return keys, nonces, signs


def fill(dst, n, key=S.RFC_KEY, counter0=0, nonce=S.RFC_NONCE):
    return _C.lib().fedfr_chacha20_fill(ptr(dst), n, (C.c_uint * 8)(*key), counter0, (C.c_uint * 3)(*nonce), _C.stream())


def mask(y, x, xi, coef, limit, streams, counters=None):
    return _C.lib().fedfr_secagg_mask(ptr(y), ptr(x), ptr(xi), float(coef), limit, *arrays(streams), len(streams), x.numel(), ptr(counters),
                                      _C.stream())


def aggregate(out, x, acc, ys, streams, frac_bits=FRAC, rescale=1.0, first=1, last=1, n=None):
    n = n if n is not None else (ys[0] if ys else out if out is not None else acc).numel()
    ptrs = (C.c_void_p * max(len(ys), 1))(*[t.data_ptr() for t in ys])
    return _C.lib().fedfr_secagg_aggregate(ptr(out), ptr(x), ptr(acc), ptrs, len(ys), *arrays(streams), len(streams), frac_bits, float(rescale), n,
                                           first, last, _C.stream())


def words_of(t):
    return N(t).view(u32)


def same_words(got, ref, what):
    assert got.dtype == ref.dtype == u32 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, "%s: %d of %d words differ, first at %d: %08x vs %08x" % (what, bad.size, got.size, bad[0], got[bad[0]], ref[bad[0]])


@functools.lru_cache(maxsize=None)
def ref_words(n, key=S.RFC_KEY, counter0=0, nonce=S.RFC_NONCE):
    w = S.words(n, key, counter0, nonce)
    w.flags.writeable = False
    return w


@functools.lru_cache(maxsize=None)
def inputs(n, K=8, w=1.0):
    """(x, xi, coef, limit) with the planted elements of secagg_cases.planted_inputs, read-only"""
    coef, limit = S.code_coef(w, FRAC), S.code_limit(K)
    x, xi = S.planted_inputs(n, coef, limit)
    x.flags.writeable = xi.flags.writeable = False
    return x, xi, coef, limit


# ---- fedfr_chacha20_fill ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.SMALL_SIZES + (S.GRID_WRAP,))
def test_chacha20_fill_bit_identical_to_the_restatement(n):
    """the words of the stream from a tail-only size to the grid-stride wrap; nothing is written behind n"""
    buf = torch.full((n + 8,), SENT, dtype=torch.int32, device=DEV)
    assert fill(buf, n) == 0, _C.last_error()
    torch.cuda.synchronize()
    got = words_of(buf)
    same_words(got[:n], ref_words(n), "fill(n=%d)" % n)
    assert np.all(got[n:] == SENT)


@pytest.mark.parametrize("n", [5, 17, 4100])
def test_chacha20_fill_stream_coordinates(n):
    """counter0 != 0 (also across the low 16 bits' carry and at the last admissible block), another key, a non-zero nonce"""
    for key, counter0, nonce in ((S.RFC_KEY, 1, S.RFC_NONCE), (KEY2, 0xFFFF, NONCE2), (KEY2, 0xFFFFFFFF - (n - 1) // 16, NONCE2),
                                 (S.RFC_KEY, 0, (0, 0, 0)), (S.RFC_KEY, 0, (0, 0, 1))):
        buf = torch.full((n + 8,), SENT, dtype=torch.int32, device=DEV)
        assert fill(buf, n, key, counter0, nonce) == 0, _C.last_error()
        got = words_of(buf)
        same_words(got[:n], S.words(n, key, counter0, nonce), "fill(n=%d, counter0=%#x)" % (n, counter0))
        assert np.all(got[n:] == SENT)
    if n > 16:                                             # one block further and the last block would pass 2^32 - 1
        assert fill(buf, n, KEY2, 0xFFFFFFFF - (n - 1) // 16 + 1, NONCE2) != 0 and "overflows" in _C.last_error()
        assert np.array_equal(words_of(buf), got)


def test_chacha20_fill_rfc8439_vector_through_the_abi():
    buf = torch.full((24,), SENT, dtype=torch.int32, device=DEV)
    assert fill(buf, 16, S.RFC_KEY, S.RFC_COUNTER, S.RFC_NONCE) == 0, _C.last_error()
    got = words_of(buf)
    assert ["%08x" % int(w) for w in got[:16]] == S.RFC_WORDS and np.all(got[16:] == SENT)


# ---- fedfr_secagg_mask -----------------------------------------------------------------------------------------------------------------
def run_mask(n, streams, K=8, w=1.0):
    x, xi, coef, limit = inputs(n, K, w)
    y = torch.full((n + 8,), SENT, dtype=torch.int32, device=DEV)
    counters = torch.tensor([1000, 2000], dtype=torch.int32, device=DEV)          # accumulated into
    assert mask(y, G(x), G(xi), coef, limit, streams, counters) == 0, _C.last_error()
    torch.cuda.synchronize()
    got = words_of(y)
    assert np.all(got[n:] == SENT)
    sat, bad = (int(v) for v in N(counters))
    return got[:n], sat - 1000, bad - 2000


@pytest.mark.parametrize("n", S.SMALL_SIZES)
@pytest.mark.parametrize("k", [0, 1, 3, 32])
def test_secagg_mask_bit_identical_to_the_restatement(k, n):
    """codes + k signed streams, with inputs that saturate at both ends, are NaN / +-inf and fall on rounding ties; both counters"""
    streams = S.some_streams(k)
    assert k < 3 or {s[2] for s in streams} == {1, -1}
    x, xi, coef, limit = inputs(n)
    ref, sat_ref, bad_ref = S.mask_u32(x, xi, coef, limit, streams)
    got, sat, bad = run_mask(n, streams)
    same_words(got, ref, "mask(k=%d, n=%d)" % (k, n))
    assert (sat, bad) == (sat_ref, bad_ref) and sat >= 2 and bad >= 3
    if k == 0:
        q, _, _ = S.encode32(x, xi, coef, limit)
        same_words(got, q.view(u32), "mask(k=0) vs the plain codes")
        assert mask(torch.empty(n, dtype=torch.int32, device=DEV), G(x), G(xi), coef, limit, [], None) == 0      # counters may be NULL


def test_secagg_mask_at_the_grid_stride_wrap():
    n = S.GRID_WRAP
    streams = S.some_streams(3)
    x, xi, coef, limit = inputs(n)
    ref, sat_ref, bad_ref = S.mask_u32(x, xi, coef, limit, streams)
    got, sat, bad = run_mask(n, streams)
    same_words(got, ref, "mask(k=3, n=%d)" % n)
    assert (sat, bad) == (sat_ref, bad_ref)


# ---- fedfr_secagg_aggregate ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def uploads(n, ku):
    """ku arbitrary upload words (the aggregate does not care where they come from), read-only"""
    g = np.random.default_rng(n + ku)
    ys = g.integers(0, 2 ** 32, (ku, n), dtype=np.uint64).astype(u32)
    ys[:, :4] = np.array([0, 1, 0x7FFFFFFF, 0x80000000], u32)                      # sums that wrap and that land on the int32 edges
    ys.flags.writeable = False
    return ys


def base_state(n):
    return (np.random.default_rng(n).standard_normal(n) * 0.05).astype(f32)


@pytest.mark.parametrize("n", [17, 4100])
@pytest.mark.parametrize("k", [0, 5])
@pytest.mark.parametrize("ku", [1, 3, 8])
def test_secagg_aggregate_bit_identical_to_the_restatement(ku, k, n):
    """uploads + recovery streams -> fp32: with x, without x (the server-optimiser route), in place (out = x), rescale != 1"""
    streams = S.some_streams(k, seed=2)
    ys = uploads(n, ku)
    x = base_state(n)
    yd = [G(y).view(torch.int32) for y in ys]
    for with_x, in_place, rescale in ((True, False, 1.0), (False, False, 1.0), (True, True, float(f32(1 / 0.7))), (False, False, float(f32(1 / 0.35)))):
        ref = S.aggregate32(x if with_x else None, list(ys), streams, FRAC, rescale)
        xd = G(x) if with_x else None
        out = xd if in_place else T.sent(n + 8)
        assert aggregate(out, xd, None, yd, streams, FRAC, rescale, n=n) == 0, _C.last_error()
        torch.cuda.synchronize()
        got = N(out)
        T.same_bits(got[:n], ref, "aggregate(ku=%d, k=%d, n=%d, x=%s, in place=%s, rescale=%r)" % (ku, k, n, with_x, in_place, rescale))
        assert in_place or np.all(got[n:] == T.SENT)


@pytest.mark.parametrize("frac_bits", [8, 30])
def test_secagg_aggregate_frac_bits(frac_bits):
    n = 4100
    ys, x = uploads(n, 3), base_state(n)
    out = T.sent(n)
    assert aggregate(out, G(x), None, [G(y).view(torch.int32) for y in ys], [], frac_bits, 1.0) == 0, _C.last_error()
    T.same_bits(N(out), S.aggregate32(x, list(ys), [], frac_bits, 1.0), "aggregate(frac_bits=%d)" % frac_bits)


def test_secagg_aggregate_at_the_grid_stride_wrap():
    n = S.GRID_WRAP
    streams = S.some_streams(1, seed=2)
    ys, x = uploads(n, 1), base_state(n)
    out = T.sent(n + 8)
    assert aggregate(out, G(x), None, [G(ys[0]).view(torch.int32)], streams, FRAC, 1.0, n=n) == 0, _C.last_error()
    torch.cuda.synchronize()
    T.same_bits(N(out)[:n], S.aggregate32(x, list(ys), streams, FRAC, 1.0), "aggregate(ku=1, k=1, n=%d)" % n)
    assert np.all(N(out)[n:] == T.SENT)


def test_secagg_aggregate_chained_passes(n=4100):
    """8 + 3 uploads through acc, the 5 streams split 2 + 3 between the passes, against the single-order restatement; and a middle pass
    that adds streams only (ku = 0)"""
    ys = uploads(n, 11)
    streams = S.some_streams(5, seed=2)
    x = base_state(n)
    rescale = float(f32(1 / 0.9))
    ref = S.aggregate32(x, list(ys), streams, FRAC, rescale)
    yd = [G(y).view(torch.int32) for y in ys]
    xd = G(x)
    acc = torch.full((n + 8,), SENT, dtype=torch.int32, device=DEV)
    out = T.sent(n + 8)
    assert aggregate(None, None, acc, yd[:8], streams[:2], FRAC, rescale, first=1, last=0, n=n) == 0, _C.last_error()
    assert aggregate(out, xd, acc, yd[8:], streams[2:], FRAC, rescale, first=0, last=1, n=n) == 0, _C.last_error()
    torch.cuda.synchronize()
    T.same_bits(N(out)[:n], ref, "8 + 3 chained")
    assert np.all(N(out)[n:] == T.SENT) and np.all(words_of(acc)[n:] == SENT)
    out3 = T.sent(n)
    assert aggregate(None, xd, acc, yd[:8], [], FRAC, rescale, first=1, last=0, n=n) == 0, _C.last_error()        # (x is ignored here)
    assert aggregate(None, None, acc, [], streams, FRAC, rescale, first=0, last=0, n=n) == 0, _C.last_error()
    assert aggregate(out3, xd, acc, yd[8:], [], FRAC, rescale, first=0, last=1, n=n) == 0, _C.last_error()
    T.same_bits(N(out3), ref, "8 / streams only / 3 chained")


# ---- end to end on raw tensors ---------------------------------------------------------------------------------------------------------
def _protocol(K, t, rnd, seed=11):
    parts = list(range(K))
    r = np.random.default_rng(seed).bytes
    clients = [secagg.SecAggClient(c, FRAC, r) for c in parts]
    srv = secagg.SecAggServer(parts, t, rnd)
    for c in clients:
        srv.register(c.cid, c.begin_round(rnd))
    for c in clients:
        srv.deliver_shares(c.cid, c.make_shares(parts, t))
    return clients, srv, parts


@pytest.mark.parametrize("dropped", [(), (2, 5)])
def test_masks_leave_no_trace_in_the_aggregate(dropped):
    """K = 8 clients, n = 4100: the aggregate of the masked uploads (with the recovery streams) is bit-identical to the aggregate of the
    same uploads made with k = 0; each masked upload differs from its plain codes in more than 99 % of its words (with uniform masks the
    expected fraction of equal words is 2^-32).  The same with two clients dropped and recovered."""
    K, n, rnd = 8, 4100, 3
    clients, srv, parts = _protocol(K, 5, rnd)
    g = np.random.default_rng(8)
    x = (g.standard_normal(n) * 0.05).astype(f32)
    xs = [(x + g.standard_normal(n).astype(f32) * f32(1e-3 * (1 + i))).astype(f32) for i in range(K)]
    w = g.random(K) + 0.1
    w = [float(f32(a)) for a in w / w.sum()]
    L = S.code_limit(K)
    xd = G(x)
    masked, plain = [], []
    for c, xi, wi in zip(clients, xs, w):
        xid = G(xi)
        ym, yp = torch.empty(n, dtype=torch.int32, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV)
        streams = c.streams(parts, srv.public_keys, rnd)
        assert len(streams) == K
        assert mask(ym, xd, xid, S.code_coef(wi, FRAC), L, streams) == 0, _C.last_error()
        assert mask(yp, xd, xid, S.code_coef(wi, FRAC), L, []) == 0, _C.last_error()
        masked.append(ym)
        plain.append(yp)
        same_words(words_of(yp), S.encode32(x, xi, S.code_coef(wi, FRAC), L)[0].view(u32), "plain codes of client %d" % c.cid)
        differ = float((ym != yp).float().mean())
        assert differ > 0.99, (c.cid, differ)
    keep = [p for p in parts if p not in dropped]
    rescale = secagg.survivor_rescale(w, keep)
    assert (rescale == 1.0) == (not dropped)
    rec = srv.recovery_streams(keep)
    assert len(rec) == len(keep) * (1 + len(dropped)) <= 32
    out_m, out_p = T.sent(n), T.sent(n)
    assert aggregate(out_m, xd, None, [masked[p] for p in keep], rec, FRAC, rescale) == 0, _C.last_error()
    assert aggregate(out_p, xd, None, [plain[p] for p in keep], [], FRAC, rescale) == 0, _C.last_error()
    torch.cuda.synchronize()
    T.same_bits(N(out_m), N(out_p), "masked + recovery vs plain")
    T.same_bits(N(out_p), S.aggregate32(x, [words_of(plain[p]) for p in keep], [], FRAC, rescale), "plain vs the restatement")
    mean, bound = S.law_bound(x, [xs[p] for p in keep], [w[p] for p in keep], FRAC, rescale)
    err = np.abs(N(out_m).astype(f64) - mean)
    print("K=8 dropped=%s: worst error / law bound %.3f" % (list(dropped), float((err / bound).max())))
    assert np.all(err <= bound)
    # without the recovery streams the sum is noise: the masks are really there
    out_x = T.sent(n)
    assert aggregate(out_x, xd, None, [masked[p] for p in keep], [], FRAC, rescale) == 0, _C.last_error()
    assert float(np.mean(N(out_x) != N(out_p))) > 0.99


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------
def _flat_world(K, n=4100 + 3, nb=40, nc=5):
    g = np.random.default_rng(K)
    x = (g.standard_normal(n) * 0.05).astype(f32)
    b = g.standard_normal(nb).astype(f32)
    glob = client.FlatStateDict.from_flat((G(x), G(b), torch.arange(nc, device=DEV)), [], [])
    models = []
    for i in range(K):
        xi = (x + g.standard_normal(n).astype(f32) * f32(1e-3 * (1 + i))).astype(f32)
        bi = (b * f32(1 + 0.05 * i)).astype(f32)
        models.append(client.FlatStateDict.from_flat((G(xi), G(bi), torch.arange(nc, device=DEV) + 3 * i + 1), [], []))
    sizes = [float(100 + 50 * ((3 * i) % 7)) for i in range(K)]
    return glob, models, sizes


@pytest.mark.parametrize("K, dropped, opt", [(3, (), None), (3, (1,), None), (11, (), None), (11, (0, 4, 9, 10), "ADAM"), (3, (), "AVGM"),
                                            (11, (0, 4, 9, 10), None)])      # (appended last: the earlier rows keep their ids)
def test_fedsecagg_reproduces_the_restatement(K, dropped, opt):
    """SecAggClient.mask -> SecAggServer.recovery_streams -> FedSecAgg on FlatStateDicts: the parameters are the restatement's bits (the
    plain codes summed: the masks cancel), also past 8 uploads and 32 recovery streams (chained passes) and through a server optimiser;
    statistics and counters are FedPavg's over the survivors.  11 clients of whom 4 drop leave 7 uploads and more than 32 recovery streams:
    the LAST pass then carries streams only, and without an optimiser it is that pass that adds x"""
    glob, models, sizes = _flat_world(K)
    x, n = N(glob.flat[0]), glob.flat[0].numel()
    rnd, t = 9, K // 2 + 1
    clients, srv, parts = _protocol(K, t, rnd)
    w = [s / sum(sizes) for s in sizes]
    ups = [c.mask(glob, m, wi, parts, srv.public_keys, rnd) for c, m, wi in zip(clients, models, w)]
    torch.cuda.synchronize()
    for u, m in zip(ups, models):
        assert isinstance(u, secagg.MaskedUpdate) and u.y.dtype == torch.int32 and u.n == n and u.frac_bits == FRAC
        assert u.stats is m.flat[1] and u.counters is m.flat[2] and u.nbytes == u.dense_nbytes == 4 * n + 4 * 40 + 8 * 5
        assert (u.saturated_count(), u.nonfinite_count()) == (0, 0)
    # one upload against the restatement with its K streams
    same_words(words_of(ups[1].y), S.mask_u32(x, N(models[1].flat[0]), S.code_coef(w[1], FRAC), S.code_limit(K),
                                              clients[1].streams(parts, srv.public_keys, rnd))[0], "upload of client 1")
    keep = [p for p in parts if p not in dropped]
    rescale = secagg.survivor_rescale(w, keep)
    rec = srv.recovery_streams(keep)
    sopt = None if opt is None else server.ServerOptimizer(opt, lr=1.0 if opt == "AVGM" else 0.01)
    out = server.FedSecAgg(glob, [ups[p] for p in keep], [sizes[p] for p in keep], rec, rescale, sopt)
    avg = server.FedPavg([models[p] for p in keep], [sizes[p] for p in keep])
    torch.cuda.synchronize()
    assert isinstance(out, client.FlatStateDict)
    assert torch.equal(out.flat[1], avg.flat[1]) and torch.equal(out.flat[2], avg.flat[2]) and out.flat[2].dtype == torch.float32
    codes = [S.encode32(x, N(models[p].flat[0]), S.code_coef(w[p], FRAC), S.code_limit(K))[0].view(u32) for p in keep]
    if sopt is None:
        T.same_bits(N(out.flat[0]), S.aggregate32(x, codes, [], FRAC, rescale), "FedSecAgg parameters")
        mean, bound = S.law_bound(x, [N(models[p].flat[0]) for p in keep], [float(f32(w[p])) for p in keep], FRAC, rescale)
        assert np.all(np.abs(N(out.flat[0]).astype(f64) - mean) <= bound)
        assert np.all(np.abs(N(avg.flat[0]).astype(f64) - N(out.flat[0]).astype(f64)) <= bound)
    else:
        delta = G(S.aggregate32(None, codes, [], FRAC, rescale))
        twin = server.ServerOptimizer(opt, lr=sopt.lr)
        want = torch.empty_like(delta)
        twin.apply_delta(want, glob.flat[0], delta)
        torch.cuda.synchronize()
        T.same_bits(N(out.flat[0]), N(want), "FedSecAgg through %s" % opt)
        T.same_bits(N(sopt.m), N(twin.m), "m'")
        assert sopt.rounds == 1


# ---- Server.train ------------------------------------------------------------------------------------------------------------------------
def _world3(aggr, **extra):
    """tests/test_fedopt_gpu.py::_tiny_world with three clients (one may drop and two remain)"""
    class Args:
        network, loss, local_epoch, output_dir, BCE_local, aggr_alg = "iresnet18", "CosFace", 1, "/tmp", False, aggr

    for k_, v_ in extra.items():
        setattr(Args, k_, v_)

    class DS:
        ID_base = 0

    class Loader(list):
        dataset = DS()

    class Data:
        train_class_sizes = [10, 10, 10]
        train_dataset_sizes = [300, 100, 250]
        train_loaders = [Loader([(R.closed_form_images(4, tag=float(c * 2 + s)), R.closed_form_labels(4, 10, tag=c + s))
                                 for s in range(2)]) for c in range(3)]

    from fedfr_amd.config import config as cfg
    cfg.lr = 0.01
    torch.manual_seed(20)
    clients = [client.Client(c, Args, Data, device=DEV) for c in range(3)]
    srv = server.Server(clients, Data, Args, device=DEV)
    srv.federated_model.load_state_dict(R.closed_form_state_dict(R.IRESNET_LAYERS["iresnet18"], tag=2.0))
    srv.secagg_rng = np.random.default_rng(4).bytes
    return srv, clients


def _delta_on_device(x, xs, ws, K, frac_bits, rescale):
    """the restatement's pseudo-gradient in torch, one fp32 operation per line (eager torch rounds each once; torch.round is half-to-even)"""
    L = S.code_limit(K)
    s = torch.zeros(x.numel(), dtype=torch.int64, device=x.device)
    for xi, w in zip(xs, ws):
        d = xi - x
        t = d * float(S.code_coef(w, frac_bits))
        assert t.dtype == torch.float32 and bool(torch.isfinite(t).all())
        q = torch.round(t).to(torch.int64)
        assert int(q.abs().max()) < L
        s += q
    assert int(s.abs().max()) < 2 ** 31
    d = s.to(torch.int32).to(torch.float32)
    d = d * float(2.0 ** -frac_bits)
    return d * float(f32(rescale))


@pytest.mark.parametrize("aggr, rounds, drop", [("FedAvg", 2, None), ("FedAdam", 2, None), ("FedAvg", 1, [1])])
def test_server_train_with_secure_aggregation(aggr, rounds, drop, caplog, monkeypatch):
    """Server.train(secure_aggregation=True): the global parameters are the restatement applied to the clients' trained states (bit for
    bit; through the server optimiser for FedAdam) and lie within the law bound of FedPavg over the clients whose upload arrived;
    statistics and counters are FedPavg's"""
    import logging
    extra = {} if drop is None else {"secagg_drop": drop}
    srv, clients = _world3(aggr, secure_aggregation=True, server_lr=0.01, **extra)
    twin = server.ServerOptimizer("ADAM", lr=0.01) if aggr == "FedAdam" else None
    rec, real = [], server.FedSecAgg
    monkeypatch.setattr(server, "FedSecAgg", lambda *a: (rec.append(real(*a)), rec[-1])[1])
    sizes = [300.0, 100.0, 250.0]
    keep = [i for i in range(3) if i not in (drop or [])]
    for r in range(rounds):
        before = [t.clone() for t in client.flat_state_dict(srv.federated_model).flat]
        with caplog.at_level(logging.INFO, logger="FL_face.server"):
            assert np.isfinite(srv.train())
        srv.step_round()
        torch.cuda.synchronize()
        assert "Masked uploads (24 fraction bits, threshold 2)" in caplog.text and "saturated" not in caplog.text
        x = before[0]
        models = [clients[i].get_model() for i in keep]
        xs = [m.flat[0] for m in models]
        assert not torch.equal(xs[0], xs[1]) and not torch.equal(xs[0], x)
        w = [s / sum(sizes) for s in sizes]
        rescale = secagg.survivor_rescale(w, keep)
        delta = _delta_on_device(x, xs, [w[i] for i in keep], 3, FRAC, rescale)
        got = srv.federated_model.flat_state()
        avg = server.FedPavg(models, [sizes[i] for i in keep])
        assert len(rec) == r + 1 and torch.equal(rec[r].flat[1], avg.flat[1]) and torch.equal(rec[r].flat[2], avg.flat[2])
        assert torch.equal(got[1], avg.flat[1]) and torch.equal(got[0], rec[r].flat[0])
        if twin is None:
            assert torch.equal(got[0], x + delta), "round %d: parameters differ from the restatement" % r
            xd = x.double()
            R_ = float(f32(rescale))
            mag = sum(R_ * float(f32(w[i])) * (xi.double() - xd).abs() for i, xi in zip(keep, xs))
            mean = xd + sum(R_ * float(f32(w[i])) * (xi.double() - xd) for i, xi in zip(keep, xs))
            bound = R_ * len(keep) * 2.0 ** -(FRAC + 1) + 2.0 ** -21 * (mag + mean.abs())
            err = (got[0].double() - avg.flat[0].double()).abs()
            print("round %d: worst |secagg - FedPavg| / law bound %.3f" % (r, float((err / bound).max())))
            assert bool((err <= bound).all())
            assert bool(((got[0].double() - mean).abs() <= bound).all())
        else:
            want = torch.empty_like(x)
            twin.apply_delta(want, x, delta)
            assert torch.equal(got[0], want), "round %d: parameters differ from the restatement through FedAdam" % r
            assert srv.server_opt.rounds == r + 1 and torch.equal(srv.server_opt.m, twin.m) and torch.equal(srv.server_opt.v, twin.v)
    assert clients[0].secagg.round == rounds - 1 and clients[0].secagg.cid == 0
