"""Compressed client uploads on the GPU: fedfr_delta_quantize / fedfr_delta_aggregate through the C ABI against the restatement of
tests/compress_cases.py, bit for bit (codes, scale bytes, residual, counter; NaN where the restatement is NaN), with sentinel guards behind
every output; and the Python surface (compress.DeltaCompressor, server.FedCompressed, Server.train with compress_bits)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import compress_cases as Q  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402

from fedfr_amd import _C, client, compress, server  # noqa: E402

DEV = torch.device("cuda:0")
f32, f64 = np.float32, np.float64
SENT = -777.25
SENT_B = 0xA5
GUARD = 16                                     # sentinel elements / bytes behind every output


def G(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # (a copy: the shared inputs are read-only arrays)


def N(t):
    return t.detach().cpu().numpy()


def ptr(t):
    return None if t is None else t.data_ptr()


def ptrs_of(ts):
    return (C.c_void_p * max(len(ts), 1))(*[ptr(t) for t in ts])


def run_quantize(xd, xid, ed, bits, n):
    """one fedfr_delta_quantize call on device tensors (``ed``: the residual buffer with GUARD sentinels behind it, or None); returns
    (codes, scales, counter) as numpy after checking the guards"""
    nc, ns = Q.code_bytes(bits, n), Q.scale_bytes(n)
    codes = torch.full((nc + GUARD,), SENT_B, dtype=torch.uint8, device=DEV)
    scales = torch.full((ns + GUARD,), SENT_B, dtype=torch.uint8, device=DEV)
    cnt = torch.tensor([0, -7], dtype=torch.int32, device=DEV)
    rc = _C.lib().fedfr_delta_quantize(ptr(xd), ptr(xid), ptr(ed), ptr(codes), ptr(scales), bits, n, ptr(cnt), _C.stream())
    assert rc == 0, _C.last_error()
    torch.cuda.synchronize()
    c, s, k = N(codes), N(scales), N(cnt)
    assert np.all(c[nc:] == SENT_B) and np.all(s[ns:] == SENT_B) and k[1] == -7, "bits=%d n=%d: wrote behind an output" % (bits, n)
    if ed is not None:
        assert np.all(N(ed)[n:] == f32(SENT)), "bits=%d n=%d: wrote behind the residual" % (bits, n)
    return c[:nc], s[:ns], int(k[0])


def check_quantize(x, xi, e, bits, what, rounds=1):
    """``rounds`` calls on one residual buffer against the restatement carried the same way; x and x_i must come back unmodified"""
    n = x.size
    xd, xid = G(x), G(xi)
    ed = None
    if e is not None:
        ed = torch.full((n + GUARD,), SENT, dtype=torch.float32, device=DEV)
        ed[:n] = G(e)
    er = e
    for r in range(rounds):
        rc_, rs_, er, rbad, _ = Q.quantize(x, xi, er, bits)
        c, s, bad = run_quantize(xd, xid, ed, bits, n)
        tag = "%s bits=%d n=%d feedback=%s round %d" % (what, bits, n, e is not None, r)
        d = np.flatnonzero(s != rs_)
        assert d.size == 0, "%s: %d scale bytes differ, first at block %d: %d vs %d" % (tag, d.size, d[0], s[d[0]], rs_[d[0]])
        d = np.flatnonzero(c != rc_)
        assert d.size == 0, "%s: %d code bytes differ, first at byte %d: %#x vs %#x" % (tag, d.size, d[0], c[d[0]], rc_[d[0]])
        assert bad == rbad, "%s: counter %d vs %d" % (tag, bad, rbad)
        if e is not None:
            got = N(ed)[:n]
            d = np.flatnonzero(Q.bits_of(got) != Q.bits_of(er))
            assert d.size == 0, "%s: %d residuals differ, first at %d: %r vs %r" % (tag, d.size, d[0], got[d[0]], er[d[0]])
    assert np.array_equal(Q.bits_of(N(xd)), Q.bits_of(x)) and np.array_equal(Q.bits_of(N(xid)), Q.bits_of(xi))      # read, never written


# ---- fedfr_delta_quantize ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", Q.SIZES)
@pytest.mark.parametrize("bits", Q.BITS)
def test_quantize_bit_identical_to_the_restatement(bits, n):
    """below / at / above one and two blocks, below one wave chunk (the partial-chunk path alone), several chunks and a tail; with and
    without the residual; a second call on the residual the first one left (the in-place update)"""
    x, xs = Q.inputs(n, 2)
    check_quantize(x, xs[0], None, bits, "sine")
    check_quantize(x, xs[1], Q.residual(n), bits, "sine", rounds=2)
    check_quantize(x, xs[1], np.zeros(n, dtype=f32), bits, "sine from a zero residual", rounds=2)


@pytest.mark.parametrize("feedback", [False, True])
@pytest.mark.parametrize("bits", Q.BITS)
def test_quantize_grid_stride_wrap(bits, feedback):
    """n = 2048 * 256 * 8 + 37: the capped grid with every wave of it at work (one whole chunk each), and a partial chunk that wraps onto
    the first wave; NaNs planted on the whole-chunk path (two in one block, one in a far chunk) and in the tail: the counter is 3, from
    waves of different workgroups"""
    n = Q.BIG
    assert Q.grid(n) == Q.GRID_CAP and n // Q.CHUNK == Q.GRID_CAP * 4 and n % Q.CHUNK == 37
    x, xs = Q.inputs(n, 1)
    xi = xs[0].copy()
    xi[[5, 6, 3000003, n - 3]] = np.nan
    check_quantize(x, xi, Q.residual(n) if feedback else None, bits, "sine + NaN")


@pytest.mark.parametrize("short,copies", [(1, 2), (31, 2), (1, 1), (31, 1)])
@pytest.mark.parametrize("bits", Q.BITS)
def test_quantize_edge_blocks(bits, short, copies):
    """zero blocks, power-of-two maxima, the saturation edge, .5 ties, +-0, subnormals (eb = 0), the top of the range, an overflowing
    subtraction, NaNs of both signs, infinities, a finite block between non-finite ones, short last blocks of 1 and 31 elements; two
    copies put every kind on the whole-chunk path, one copy on the partial-chunk path.  What each block is for: tests/test_compress_cpu.py"""
    x, xi = Q.edge_blocks(bits, short, copies)
    check_quantize(x, xi, None, bits, "edge")
    check_quantize(x, xi, np.zeros(x.size, dtype=f32), bits, "edge", rounds=2)
    e = Q.residual(x.size).copy()
    e[0:32] = 0.0                                                             # (the zero block stays one)
    check_quantize(x, xi, e, bits, "edge + residual", rounds=2)


# ---- fedfr_delta_aggregate ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def uploads(n, bits, k=8):
    """k made-up uploads in closed form (any byte is a valid code for the aggregate, -128 / -8 included): integer hashes for the codes,
    scale bytes around 2^-12 with a zero (subnormal scale) and a 255 (NaN block) here and there; (codes, scales, dq) each, read-only"""
    out = []
    for i in range(k):
        j = np.arange(Q.code_bytes(bits, n), dtype=np.uint64)
        codes = (((j * np.uint64(2654435761) + np.uint64(40503 * i + 17)) >> np.uint64(9)) & np.uint64(0xFF)).astype(np.uint8)
        if bits == 4 and n % 2:
            codes[-1] &= 0x0F
        b = np.arange(Q.scale_bytes(n), dtype=np.int64)
        scales = (108 + (b * 7 + 3 * i) % 13).astype(np.uint8)
        scales[(b + i) % 61 == 7] = 0
        scales[(b + 5 * i) % 257 == 100 + i] = 255
        dq = Q.dequantize(codes, scales, bits, n)
        for a in (codes, scales, dq):
            a.flags.writeable = False
        out.append((codes, scales, dq))
    return tuple(out)


def aggregate_ref(dst0, base, ups, ws, accumulate):
    s = None
    with np.errstate(invalid="ignore", over="ignore"):
        for i, ((_, _, dq), w) in enumerate(zip(ups, ws)):
            term = f32(w) * dq
            s = ((dst0 + term) if accumulate else term) if i == 0 else s + term
        return s if base is None else base + s


WS = [f32(w) for w in (0.21, 0.07, 0.13, 0.09, 0.17, 0.11, 0.08, 0.14)]


def check_aggregate(bits, n, ks):
    """every k of ``ks`` x accumulate 0 / 1 x base null / distinct / equal to dst against the restatement, bit for bit (NaN where it is NaN)"""
    ups = uploads(n, bits)
    cd, sd = [G(u[0]) for u in ups[:max(ks)]], [G(u[1]) for u in ups[:max(ks)]]
    j = np.arange(n, dtype=f64)
    dst0 = (0.4 * np.sin(0.77 * j + 1.3)).astype(f32)
    x = (0.5 * np.sin(0.37 * j + 0.1)).astype(f32)
    xd, d0 = G(x), G(dst0)
    lib = _C.lib()
    for k in ks:
        wv = (C.c_float * k)(*[float(w) for w in WS[:k]])
        for accumulate in (0, 1):
            for base in ("null", "distinct", "dst"):
                buf = torch.full((n + GUARD,), SENT, dtype=torch.float32, device=DEV)
                buf[:n] = d0
                bp = {"null": None, "distinct": ptr(xd), "dst": ptr(buf)}[base]
                rc = lib.fedfr_delta_aggregate(ptr(buf), bp, ptrs_of(cd[:k]), ptrs_of(sd[:k]), wv, k, bits, n, accumulate, _C.stream())
                assert rc == 0, _C.last_error()
                torch.cuda.synchronize()
                got = N(buf)
                tag = "bits=%d n=%d k=%d accumulate=%d base=%s" % (bits, n, k, accumulate, base)
                assert np.all(got[n:] == f32(SENT)), tag + ": wrote behind dst"
                ref = aggregate_ref(dst0, {"null": None, "distinct": x, "dst": dst0}[base], ups[:k], WS[:k], accumulate)
                bad = Q.same_bits_or_nan(got[:n], ref)
                assert bad.size == 0, "%s: %d of %d elements differ, first at %d: %r vs %r" % (tag, bad.size, n, bad[0], got[bad[0]], ref[bad[0]])
    assert np.array_equal(Q.bits_of(N(xd)), Q.bits_of(x))                    # read, never written: base and the uploads
    for t, u in zip(cd + sd, [u[0] for u in ups[:max(ks)]] + [u[1] for u in ups[:max(ks)]]):
        assert np.array_equal(N(t), u)


@pytest.mark.parametrize("n", Q.SIZES)
@pytest.mark.parametrize("bits", Q.BITS)
def test_aggregate_bit_identical_to_the_restatement(bits, n):
    """k = 1, 2, 3, 8; accumulate 0 and 1; base null, distinct and equal to dst; the sizes of the quantiser tests (tail only, one unit of 8,
    several blocks of threads and a tail); NaN blocks (scale byte 255) and subnormal scales (0) among the uploads"""
    ups = uploads(n, bits)
    assert Q.same_bits_or_nan(Q.dequantize(ups[0][0], ups[0][1], bits, n), ups[0][2]).size == 0
    check_aggregate(bits, n, (1, 2, 3, 8))


@pytest.mark.parametrize("k", [1, 2, 3, 8])
@pytest.mark.parametrize("bits", Q.BITS)
def test_aggregate_grid_stride_wrap(bits, k):
    """n = 2048 * 256 * 8 + 37: the capped grid, the first threads wrap (4 more units of 8), and a scalar tail of 5 elements follows"""
    check_aggregate(bits, Q.BIG, (k,))


def test_argument_errors_launch_nothing():
    n = 1023
    x, xs = Q.inputs(n, 2)
    xd, xid = G(x), G(xs[0])
    codes = torch.full((n + GUARD,), SENT_B, dtype=torch.uint8, device=DEV)
    scales = torch.full((64,), SENT_B, dtype=torch.uint8, device=DEV)
    out = torch.full((n + GUARD,), SENT, dtype=torch.float32, device=DEV)
    lib = _C.lib()

    def refused(rc, word):
        assert rc == -1 and word in _C.last_error(), (rc, _C.last_error())

    refused(lib.fedfr_delta_quantize(ptr(xd), ptr(xid), None, ptr(codes), ptr(scales), 5, n, None, _C.stream()), "bits=5")
    refused(lib.fedfr_delta_quantize(ptr(xd), ptr(xid), ptr(out) + 4, ptr(codes), ptr(scales), 8, n, None, _C.stream()), "aligned")
    refused(lib.fedfr_delta_quantize(ptr(xd), ptr(xid), None, ptr(codes), ptr(scales) + 4, 8, n, None, _C.stream()), "aligned")
    refused(lib.fedfr_delta_quantize(ptr(xd), None, None, ptr(codes), ptr(scales), 8, n, None, _C.stream()), "null")
    wv = (C.c_float * 8)(*([0.125] * 8))
    refused(lib.fedfr_delta_aggregate(ptr(out), None, ptrs_of([codes] * 9), ptrs_of([scales] * 9), wv, 9, 8, n, 0, _C.stream()), "k=9")
    refused(lib.fedfr_delta_aggregate(ptr(out), None, ptrs_of([codes]), ptrs_of([scales]), wv, 1, 2, n, 0, _C.stream()), "bits=2")
    refused(lib.fedfr_delta_aggregate(ptr(out), None, ptrs_of([codes, None]), ptrs_of([scales, scales]), wv, 2, 8, n, 0, _C.stream()), "code buffer 1 is null")
    refused(lib.fedfr_delta_aggregate(ptr(out) + 8, None, ptrs_of([codes]), ptrs_of([scales]), wv, 1, 8, n, 0, _C.stream()), "aligned")
    assert lib.fedfr_delta_aggregate(ptr(out), ptr(xd), ptrs_of([codes]), ptrs_of([scales]), wv, 1, 8, 0, 0, _C.stream()) == 0      # n = 0: a no-op
    assert lib.fedfr_delta_quantize(ptr(xd), ptr(xid), ptr(out), ptr(codes), ptr(scales), 4, 0, None, _C.stream()) == 0
    torch.cuda.synchronize()
    assert float(out.min()) == SENT == float(out.max()) and int(codes.min()) == SENT_B == int(codes.max()) and int(scales.min()) == SENT_B == int(scales.max())


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------
NP = 4103


def synthetic_states(k, tag=0.0, stats=True):
    """(global state, k client states) as FlatStateDicts over made-up flat tensors: 4103 parameters, 1026 running statistics (means, then
    variances >= 0) and 7 counters per state (none of either with ``stats`` off: a backbone without BatchNorm)"""
    x, ps = Q.inputs(NP, k, tag=tag)
    j = np.arange(513, dtype=f64)

    def state(p, i):
        if not stats:
            return client.FlatStateDict.from_flat((G(p), torch.zeros(0, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV)), [], [])
        mean = 0.3 * np.sin(0.21 * j + i)
        var = 0.5 + 0.4 * np.sin(0.13 * j + 0.7 * i) ** 2
        c = torch.arange(7, dtype=torch.int64) * 3 + 11 * i + 1
        return client.FlatStateDict.from_flat((G(p), G(np.concatenate([mean, var]).astype(f32)), c.to(DEV)), [], [])
    return state(x, -1), [state(p, i) for i, p in enumerate(ps)]


def sizes_of(k):
    return [100.0 + 37.0 * ((5 * i) % 7) for i in range(k)]


def weights32(sizes):
    tot = sum(sizes)
    return [f32(s / tot) for s in sizes]


def restated_uploads(x, xs, bits, es=None):
    """[(codes, scales)] and the new residuals of one round of the restatement (``es``: the residuals going in, default zeros)"""
    ups, out = [], []
    for i, xi in enumerate(xs):
        c, s, e, _, _ = Q.quantize(x, xi, np.zeros(x.size, dtype=f32) if es is None else es[i], bits)
        ups.append((c, s))
        out.append(e)
    return ups, out


@pytest.mark.parametrize("k", [3, 8, 9, 17])
@pytest.mark.parametrize("bits", Q.BITS)
def test_fedcompressed(bits, k):
    """parameters bit-equal to the restatement chained as the code chains it (groups of 8, x added by the last pass); statistics and
    counters bit-equal to FedPavg's; every coordinate within sum_i w_i scale_i + 4 ulp of FedPavg's result: each dq_i is within scale_i
    of the true delta, so the error of the weighted sum is at most sum_i w_i scale_i, and the fp32 roundings of the two paths add a few
    ulp (of the result)"""
    g, models = synthetic_states(k)
    sizes = sizes_of(k)
    ups = [compress.DeltaCompressor(bits).compress(g, m) for m in models]
    out = server.FedCompressed(g, ups, sizes)
    avg = server.FedPavg(models, sizes)
    torch.cuda.synchronize()
    assert isinstance(out, client.FlatStateDict)
    x, xs = N(g.flat[0]), [N(m.flat[0]) for m in models]
    rups, _ = restated_uploads(x, xs, bits)
    for u, (c, s) in zip(ups, rups):
        assert np.array_equal(N(u.codes), c) and np.array_equal(N(u.scales), s) and u.nonfinite_count() == 0
    ws = weights32(sizes)
    ref = Q.chained(x, rups, ws, bits, NP)
    got = N(out.flat[0])
    assert np.array_equal(Q.bits_of(got), Q.bits_of(ref)), (bits, k)
    assert torch.equal(out.flat[1], avg.flat[1]) and torch.equal(out.flat[2], avg.flat[2]) and out.flat[2].dtype == torch.float32
    a = N(avg.flat[0])
    bound = sum(float(w) * np.repeat(Q.scale_of(s), 32)[:NP].astype(f64) for w, (_, s) in zip(ws, rups)) + 4 * np.spacing(np.abs(a)).astype(f64)
    err = np.abs(got.astype(f64) - a.astype(f64))
    print("bits=%d k=%d: worst |FedCompressed - FedPavg| / bound %.3f" % (bits, k, float(np.max(err / bound))))
    assert np.all(err <= bound)


@pytest.mark.parametrize("k", [3, 9])
def test_fedcompressed_with_a_server_optimizer(k):
    """ServerOptimizer("AVGM"): the result is apply_delta on the restated delta (the chained sum WITHOUT x), bit for bit, momentum included"""
    bits = 8
    g, models = synthetic_states(k)
    sizes = sizes_of(k)
    ups = [compress.DeltaCompressor(bits).compress(g, m) for m in models]
    opt = server.ServerOptimizer("AVGM", lr=0.5, beta1=0.75)
    out = server.FedCompressed(g, ups, sizes, opt)
    x, xs = N(g.flat[0]), [N(m.flat[0]) for m in models]
    rups, _ = restated_uploads(x, xs, bits)
    delta = Q.chained(x, rups, weights32(sizes), bits, NP, with_base=False)
    ref_opt = server.ServerOptimizer("AVGM", lr=0.5, beta1=0.75)
    P = torch.empty(NP, dtype=torch.float32, device=DEV)
    ref_opt.apply_delta(P, g.flat[0], G(delta))
    torch.cuda.synchronize()
    assert torch.equal(out.flat[0], P) and torch.equal(opt.m, ref_opt.m) and opt.rounds == 1 and float(opt.m.abs().max()) > 0
    assert np.array_equal(Q.bits_of(N(g.flat[0])), Q.bits_of(x))              # the global state is read, never written
    avg = server.FedPavg(models, sizes)
    assert torch.equal(out.flat[1], avg.flat[1]) and torch.equal(out.flat[2], avg.flat[2])


@pytest.mark.parametrize("bits", Q.BITS)
def test_delta_compressor_carries_its_residual_over_three_rounds(bits):
    g, _ = synthetic_states(1)
    x = N(g.flat[0])
    comp = compress.DeltaCompressor(bits)
    plain = compress.DeltaCompressor(bits, error_feedback=False)
    e = np.zeros(NP, dtype=f32)
    for r in range(3):
        _, (m,) = synthetic_states(1, tag=0.5 * r)                            # the client's state of round r
        up = comp.compress(g, m)
        c, s, e, _, _ = Q.quantize(x, N(m.flat[0]), e, bits)
        assert np.array_equal(N(up.codes), c) and np.array_equal(N(up.scales), s), r
        assert np.array_equal(Q.bits_of(N(comp.residual)), Q.bits_of(e)) and np.any(e != 0), r
        up0 = plain.compress(g, m)                                            # no feedback: nothing carried, nothing allocated
        c0, s0, _, _, _ = Q.quantize(x, N(m.flat[0]), None, bits)
        assert np.array_equal(N(up0.codes), c0) and np.array_equal(N(up0.scales), s0) and plain.residual is None
        assert up.stats is m.flat[1] and up.counters is m.flat[2] and up.bits == bits and up.n == NP
    comp.reset()                                                              # the next round starts from a zero residual again
    assert comp.residual is None
    up = comp.compress(g, m)
    c, s, e, _, _ = Q.quantize(x, N(m.flat[0]), np.zeros(NP, dtype=f32), bits)
    assert np.array_equal(N(up.codes), c) and np.array_equal(Q.bits_of(N(comp.residual)), Q.bits_of(e))
    # bytes: codes + scale bytes = (bits + 0.25) / 8 per parameter up to the padding of the last byte and the last block
    payload = up.codes.numel() + up.scales.numel()
    assert NP * (bits + 0.25) / 8 <= payload < NP * (bits + 0.25) / 8 + 2
    assert up.nbytes == payload + 1026 * 4 + 7 * 8 and up.dense_nbytes == NP * 4 + 1026 * 4 + 7 * 8 and up.ratio == up.nbytes / up.dense_nbytes
    g0, (m0,) = synthetic_states(1, stats=False)                              # no statistics: the ratio is the format's
    up = compress.DeltaCompressor(bits).compress(g0, m0)
    assert (bits + 0.25) / 32 <= up.ratio < (bits + 0.25) / 32 + 2 / (4 * NP)
    with pytest.raises(RuntimeError, match="reset"):
        comp.compress(client.FlatStateDict.from_flat((g.flat[0][:64].clone(), g.flat[1], g.flat[2]), [], []),
                      client.FlatStateDict.from_flat((m.flat[0][:64].clone(), m.flat[1], m.flat[2]), [], []))


@pytest.mark.parametrize("bits", Q.BITS)
def test_a_poisoned_client_shows_in_its_block_only(bits):
    """one NaN in one client's state: NaN in that block of the aggregate and nowhere else, a counter of 1, and a finite residual (zero in
    that block): the client is not poisoned forever"""
    k, at = 5, 1000
    g, models = synthetic_states(k)
    models[2].flat[0][at] = float("nan")
    comps = [compress.DeltaCompressor(bits) for _ in range(k)]
    ups = [c.compress(g, m) for c, m in zip(comps, models)]
    out = server.FedCompressed(g, ups, sizes_of(k))
    torch.cuda.synchronize()
    assert [u.nonfinite_count() for u in ups] == [0, 0, 1, 0, 0]
    got = N(out.flat[0])
    blk = slice(at // 32 * 32, at // 32 * 32 + 32)
    mask = np.zeros(NP, dtype=bool)
    mask[blk] = True
    assert np.all(np.isnan(got[mask])) and np.all(np.isfinite(got[~mask]))
    e = N(comps[2].residual)
    assert np.all(np.isfinite(e)) and np.all(Q.bits_of(e[blk]) == 0) and np.any(e[~mask] != 0)
    x, xs = N(g.flat[0]), [N(m.flat[0]) for m in models]
    rups, _ = restated_uploads(x, xs, bits)
    assert Q.same_bits_or_nan(got, Q.chained(x, rups, weights32(sizes_of(k)), bits, NP)).size == 0


# ---- Server.train ------------------------------------------------------------------------------------------------------------------------
def _tiny_world(aggr, nc, **extra):
    """``nc`` clients on the smallest backbone and batch of the Server.train tests of tests/test_robust_gpu.py (iresnet18, B = 4, two steps each)"""
    class Args:
        network, loss, local_epoch, output_dir, BCE_local, aggr_alg = "iresnet18", "CosFace", 1, "/tmp", False, aggr

    for k_, v_ in extra.items():
        setattr(Args, k_, v_)

    class DS:
        ID_base = 0

    class Loader(list):
        dataset = DS()

    class Data:
        train_class_sizes = [10] * nc
        train_dataset_sizes = [300, 100, 250, 120, 200][:nc]
        train_loaders = [Loader([(O.closed_form_images(4, tag=float(c * 2 + s)), O.closed_form_labels(4, 10, tag=c + s))
                                 for s in range(2)]) for c in range(nc)]

    from fedfr_amd.config import config as cfg
    cfg.lr = 0.01
    torch.manual_seed(20)
    clients = [client.Client(c, Args, Data, device=DEV) for c in range(nc)]
    srv = server.Server(clients, Data, Args, device=DEV)
    srv.federated_model.load_state_dict(O.closed_form_state_dict(O.IRESNET_LAYERS["iresnet18"], tag=2.0))
    return srv, clients


def _windows(n):
    """32-aligned windows of the parameter buffer the restatement is evaluated on (blocks are independent, so a window of whole blocks
    restates exactly; the whole buffer of iresnet18 would cost numpy tens of seconds): the first 8192 elements, 8192 from the middle,
    and the last ones with the short block"""
    mid = n // 2 // 32 * 32
    return [slice(0, 8192), slice(mid, mid + 8192), slice((n - 8192) // 32 * 32, n)]


def test_server_train_with_compressed_uploads(monkeypatch):
    """two rounds, two clients, compress_bits=8: after each round the global parameters equal the restatement applied to the recorded
    client states (quantised against the global state the round started from, residuals carried per client, data-size weights), and
    the second round runs on non-zero residuals that differ between the clients"""
    srv, clients = _tiny_world("FedAvg", 2, compress_bits=8)
    rec = []
    real = server.FedCompressed

    def recording(global_state, updates, weights, server_opt=None):
        assert server_opt is None
        rec.append((N(global_state.flat[0]), [N(c.backbone_state_dict.flat[0]) for c in clients], list(weights), [u.nbytes for u in updates],
                    [u.dense_nbytes for u in updates]))
        return real(global_state, updates, weights, server_opt)
    monkeypatch.setattr(server, "FedCompressed", recording)
    monkeypatch.setattr(server, "FedPavg", lambda *a: pytest.fail("FedPavg was called on the compressed path"))
    n = srv.federated_model.flat_state()[0].numel()
    wins = _windows(n)
    es = [[np.zeros(w.stop - w.start, dtype=f32) for w in wins] for _ in clients]
    x_prev = N(srv.federated_model.flat_state()[0])
    for r in range(2):
        assert np.isfinite(srv.train())
        srv.step_round()
        torch.cuda.synchronize()
        xg, xs, weights, sent, dense = rec[r]
        assert np.array_equal(Q.bits_of(xg), Q.bits_of(x_prev)), "round %d was quantised against another global state" % r
        assert weights == [300, 100] and not np.array_equal(xs[0], xs[1])
        assert all(0.25 < s / d < 0.27 for s, d in zip(sent, dense))         # 8.25 / 32 of the parameters + the statistics as they are
        ws = weights32(weights)
        got = N(srv.federated_model.flat_state()[0])
        for wi, w in enumerate(wins):
            ups = []
            for i in range(2):
                c, s, es[i][wi], nbad, _ = Q.quantize(xg[w], xs[i][w], es[i][wi], 8)
                assert nbad == 0
                ups.append((c, s))
                assert np.array_equal(Q.bits_of(N(clients[i].compressor.residual[w])), Q.bits_of(es[i][wi])), (r, i, wi)
            ref = Q.chained(xg[w], ups, ws, 8, w.stop - w.start)
            assert np.array_equal(Q.bits_of(got[w]), Q.bits_of(ref)), "round %d window %d" % (r, wi)
        if r == 0:                                                            # what round 2 starts from: non-zero, distinct per client
            r0, r1 = (N(c.compressor.residual) for c in clients)
            assert np.any(r0 != 0) and np.any(r1 != 0) and not np.array_equal(r0, r1)
        x_prev = got
    assert len(rec) == 2 and all(c.compressor.bits == 8 and c.compressor.error_feedback for c in clients)


def test_server_train_compressed_with_a_server_optimizer(monkeypatch):
    """aggr_alg="FedAvgM" with compress_bits=4 and error_feedback off: the server's optimiser receives the aggregate of the uploads as its
    pseudo-gradient; the new global parameters equal apply_delta on the restated delta, and no client keeps a residual"""
    srv, clients = _tiny_world("FedAvgM", 2, compress_bits=4, error_feedback=False, server_lr=0.5, server_momentum=0.75)
    rec = []
    real = server.FedCompressed

    def recording(global_state, updates, weights, server_opt=None):
        rec.append((N(global_state.flat[0]), [N(c.backbone_state_dict.flat[0]) for c in clients], list(weights), server_opt))
        return real(global_state, updates, weights, server_opt)
    monkeypatch.setattr(server, "FedCompressed", recording)
    monkeypatch.setattr(server, "FedOpt", lambda *a: pytest.fail("FedOpt was called on the compressed path"))
    assert np.isfinite(srv.train())
    torch.cuda.synchronize()
    xg, xs, weights, opt = rec[0]
    assert opt is srv.server_opt and opt.kind == "AVGM" and (opt.lr, opt.beta1, opt.clip_norm, opt.rounds) == (0.5, 0.75, 0.0, 1)
    assert all(c.compressor.bits == 4 and not c.compressor.error_feedback and c.compressor.residual is None for c in clients)
    got = srv.federated_model.flat_state()[0]
    for w in _windows(xg.size):
        ups = [Q.quantize(xg[w], x[w], None, 4)[:2] for x in xs]
        delta = Q.chained(xg[w], ups, weights32(weights), 4, w.stop - w.start, with_base=False)
        ref_opt = server.ServerOptimizer("AVGM", lr=0.5, beta1=0.75)
        P = torch.empty(w.stop - w.start, dtype=torch.float32, device=DEV)
        ref_opt.apply_delta(P, G(xg[w]), G(delta))
        torch.cuda.synchronize()
        assert torch.equal(got[w], P) and torch.equal(opt.m[w], ref_opt.m), w


def test_server_train_without_compress_bits_is_untouched(monkeypatch):
    """compress_bits unset: FedPavg is called as before, FedCompressed is not, and no client grows a compressor"""
    calls = {"pavg": 0}
    real = server.FedPavg
    monkeypatch.setattr(server, "FedPavg", lambda *a: (calls.__setitem__("pavg", calls["pavg"] + 1), real(*a))[1])
    monkeypatch.setattr(server, "FedCompressed", lambda *a, **k: pytest.fail("FedCompressed was called with compress_bits unset"))
    srv, clients = _tiny_world("FedAvg", 2)
    assert np.isfinite(srv.train())
    torch.cuda.synchronize()
    assert calls == {"pavg": 1} and not any(hasattr(c, "compressor") for c in clients)
