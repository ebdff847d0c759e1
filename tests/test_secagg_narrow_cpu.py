"""Narrow secure aggregation without a GPU: the restatement's own laws (rotation, field-wise arithmetic, the stochastic encoder, unbiasedness,
what the rotation buys), the protocol run in numpy with dropped clients, what the new entry points refuse on the host, and what
Server.train / FedSecAgg refuse before any client trains."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import secagg_cases as S
import secagg_narrow_cases as N
from conftest import REPO

f32, f64, u32, i32, i64 = np.float32, np.float64, np.uint32, np.int32, np.int64
ROT_SEED, RND = 0x1234_5678_9ABC_DEF0, 7


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from fedfr_amd import _C
    return _C


def rng(seed):
    return np.random.default_rng(seed).bytes


# ---- the rotation ------------------------------------------------------------------------------------------------------------------------
def test_hadamard_rows_are_orthogonal_exactly_on_integers():
    """H H = 4096 I on integer inputs small enough that every partial sum is an exact float: the butterfly is the Walsh-Hadamard matrix"""
    g = np.random.default_rng(1)
    v = g.integers(-8, 9, (3, N.BLOCK)).astype(f32)
    h = N.hadamard32(v)                                          # integers of at most 8 * 4096 = 2^15 at every level: exact
    hh = N.hadamard32(h)                                         # level l of the second pass holds 2^l times a partial transform: at most 2^15 too
    assert np.array_equal(hh, f32(4096) * v)
    # and row r of H is the image of e_r: rows 0, 1, 5, 4095 against each other and themselves
    rows = [0, 1, 5, 2048, 4095]
    e = np.zeros((len(rows), N.BLOCK), f32)
    e[np.arange(len(rows)), rows] = 1
    Hr = N.hadamard32(e)
    assert set(np.unique(Hr)) == {-1.0, 1.0}
    assert np.array_equal(Hr @ Hr.T, f32(4096) * np.eye(len(rows), dtype=f32))
    # the sign convention: entry (r, c) = (-1)^popcount(r & c)
    c = np.arange(N.BLOCK)
    for k, r in enumerate(rows):
        pop = np.array([bin(r & int(cc)).count("1") for cc in c])
        assert np.array_equal(Hr[k], np.where(pop % 2, -1, 1).astype(f32))


def test_rotation_within_its_bound_of_the_fp64_rotation_and_inverts():
    g = np.random.default_rng(2)
    for n in N.SIZES:
        u = (g.standard_normal(n) * np.exp(g.standard_normal(n))).astype(f32)
        v, v64 = N.rotate32(u, ROT_SEED, RND), N.rotate64(u, ROT_SEED, RND)
        norms = np.sqrt((N.pad32(u).astype(f64) ** 2).reshape(-1, N.BLOCK).sum(axis=1))
        bound = np.repeat(N.ROTATION_BOUND * norms, N.BLOCK)
        assert v.dtype == f32 and v.size == N.padded_count(n)
        assert np.all(np.abs(v.astype(f64) - v64) <= bound), n
        # the rotation is orthonormal: it keeps the block norms (in fp64), and H applied twice with the 2^-6 scales returns u within the same bound
        assert np.allclose(np.sqrt((v64 ** 2).reshape(-1, N.BLOCK).sum(axis=1)), norms, rtol=1e-12)
        back = N.rotate_back32(v, ROT_SEED, RND)
        assert np.all(np.abs(back.astype(f64) - N.pad32(u)) <= bound), n


def test_signs_are_the_bits_of_their_own_philox_stream():
    import dp_cases as D
    b = N.sign_bits(2 * N.BLOCK, ROT_SEED, RND)
    w = D.words(2 * N.BLOCK // 32, ROT_SEED, RND, N.SIGN_SID)
    for e in (0, 1, 31, 32, 33, 4095, 4096, 8191):
        assert b[e] == bool((int(w[e // 32]) >> (e % 32)) & 1)
    assert 0.45 < b.mean() < 0.55
    assert not np.array_equal(b, N.sign_bits(2 * N.BLOCK, ROT_SEED, RND + 1)) and not np.array_equal(b, N.sign_bits(2 * N.BLOCK, ROT_SEED + 1, RND))
    assert N.SIGN_SID != N.ROUND_SID and {N.SIGN_SID, N.ROUND_SID}.isdisjoint({0, 0x44444750})      # the stream ids of dp.hip and ddp.hip


# ---- field-wise arithmetic ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 16])
def test_field_arithmetic_never_carries_across_a_field(bits):
    """the kernels' word formulas against numpy's own uint8 / uint16 arithmetic: every pair of the edge values in every field, and random words"""
    edge = [0x00, 0x01, 0x7F, 0x80, 0x81, 0xFE, 0xFF] if bits == 8 else [0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFE, 0xFFFF, 0x00FF, 0xFF00, 0x0080]
    F = 32 // bits
    grids = np.meshgrid(*[np.array(edge, dtype=np.uint64)] * F, indexing="ij")
    w = sum(gr.reshape(-1) << np.uint64(bits * c) for c, gr in enumerate(grids)).astype(u32)      # every field pattern of the edge values
    a, b = np.repeat(w, w.size), np.tile(w, w.size)
    if a.size > 4_000_000:                                       # 8 bits: 7^4 words, 5.8 M pairs: every second word against every word
        a, b = np.repeat(w[::2], w.size), np.tile(w, w[::2].size)
    g = np.random.default_rng(bits)
    a = np.concatenate([a, g.integers(0, 2 ** 32, 100_000, dtype=np.uint64).astype(u32)])
    b = np.concatenate([b, g.integers(0, 2 ** 32, 100_000, dtype=np.uint64).astype(u32)])
    s, d = N.swar_add(a, b, bits), N.swar_sub(a, b, bits)
    assert s.dtype == d.dtype == u32
    assert np.array_equal(s, N.field_add(a, b, bits)) and np.array_equal(d, N.field_sub(a, b, bits))
    assert np.array_equal(N.swar_sub(s, b, bits), a) and np.array_equal(N.swar_add(d, b, bits), a)      # add then subtract: the identity
    # a field changes only through its own operands: the neighbours of a wrapping field stay
    one = u32(1)
    top = u32((1 << bits) - 1)
    assert N.swar_add(np.array([top], u32), np.array([one], u32), bits)[0] == 0
    assert N.swar_sub(np.array([0], u32), np.array([one], u32), bits)[0] == top


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("K", [2, 3, 32])
def test_the_sum_of_K_codes_never_wraps(bits, K):
    L = N.code_limit(K, bits)
    assert L >= 1 and K * L <= 2 ** (bits - 1) - 1 < K * (L + 1) + K
    for sign in (1, -1):
        q = np.full(N.BLOCK, sign * L, i64)
        s = np.zeros(N.BLOCK * bits // 32, u32)
        for _ in range(K):
            s = N.field_add(s, N.pack(q, bits), bits)
        assert np.array_equal(N.unpack(s, bits), K * q)
    g = np.random.default_rng(K)
    q = g.integers(-L, L + 1, (K, N.BLOCK))
    s = np.zeros(N.BLOCK * bits // 32, u32)
    for k in range(K):
        s = N.field_add(s, N.pack(q[k], bits), bits)
    assert np.array_equal(N.unpack(s, bits), q.sum(axis=0))
    assert np.array_equal(N.unpack(N.pack(q[0], bits), bits), q[0])
    # little end first
    assert N.pack(np.array([1, 2, 3, 4][:32 // bits]), bits)[0] == (0x04030201 if bits == 8 else 0x00020001)


# ---- the encoder -------------------------------------------------------------------------------------------------------------------------
def test_encoder_floor_ties_clamp_and_non_finite_values():
    L = 15
    never, always = np.zeros(1, u32), np.full(1, 0xFFFFFFFF, u32)      # r = 0: rounds up whenever t has a fraction;  r = 2^24 - 1: only above 1 - 2^-24

    def enc(t, r):
        return N.encode_narrow32(np.array([t], f32), 1.0, L, r)
    for t in (-3.0, 0.0, 5.0, -0.0):                             # an integer t never rounds up
        assert enc(t, never)[0][0] == int(t) and enc(t, always)[0][0] == int(t)
    assert enc(-2.5, always)[0][0] == -3 and enc(-2.5, never)[0][0] == -2      # floor, not truncation: -2.5 lies between -3 and -2
    assert enc(2.5, always)[0][0] == 2 and enc(2.5, never)[0][0] == 3
    assert enc(-0.25, always)[0][0] == -1 and enc(-0.25, never)[0][0] == 0
    # the threshold: r 2^-24 < frac, with frac = 0.5: r = 2^23 - 1 rounds up, r = 2^23 does not
    assert enc(2.5, np.array([(2 ** 23 - 1) << 8 | 0xFF], u32))[0][0] == 3 and enc(2.5, np.array([2 ** 23 << 8], u32))[0][0] == 2
    for t in (float("nan"), float("inf"), float("-inf")):        # non-finite: 0, counted
        assert enc(t, never) == (np.array([0], i32), 0, 1)
    for t, q in ((1e30, L), (-1e30, -L), (15.0, L), (-15.0, -L), (16.5, L), (-15.5, -L)):      # clamped (or exactly at the limit): counted
        got = enc(t, never)
        assert got[0][0] == q and got[1:] == (1, 0), (t, got)
    assert enc(14.0, always)[1:] == (0, 0)
    # t = v coef overflowing to inf is non-finite too
    assert N.encode_narrow32(np.array([3e38], f32), 16.0, L, never)[1:] == (0, 1)


def test_encoder_is_unbiased():
    """256 private seeds (0 ... 255: taken as they come; the restatement passes with them, and the bound is a 6 sigma one), n = 4096, b = 8:
    the mean of the decoded updates is within 6 * 0.5 * 2^-f / (w sqrt(256)) of u on every coordinate: the variance of one rounding is at
    most 1/4 code^2, and the rotation back is orthonormal, so a decoded coordinate has a standard deviation of at most 0.5 * 2^-f / w"""
    n, bits, K, f, w = N.BLOCK, 8, 2, 8, 1.0
    L = N.code_limit(K, bits)
    g = np.random.default_rng(5)
    u = (g.standard_normal(n) * 0.03).astype(f32)
    x = np.zeros(n, f32)
    coef = S.code_coef(w, f)
    mean = np.zeros(n, f64)
    for seed in range(256):
        q, sat, bad = N.codes_narrow(x, u, coef, K, bits, ROT_SEED, seed, RND)
        assert sat == 0 and bad == 0 and np.abs(q).max() < L
        mean += N.decode_narrow(N.pack(q, bits), bits, f, 1.0, ROT_SEED, RND, n).astype(f64) / w
    mean /= 256
    assert np.abs(mean - u).max() <= 6 * 0.5 * 2.0 ** -f / (w * 16)
    # and the codes do depend on the private seed
    assert not np.array_equal(N.codes_narrow(x, u, coef, K, bits, ROT_SEED, 0, RND)[0], N.codes_narrow(x, u, coef, K, bits, ROT_SEED, 1, RND)[0])


def test_the_rotation_keeps_a_spike_inside_the_code_range():
    """one spike of size a in a block, f such that a w 2^f > L but a w 2^f / 64 < L: rotated, every code is +-a w 2^f / 64 and none saturates;
    with the identity in place of the rotation the spike is clamped"""
    bits, K, f, w, a = 8, 2, 8, 1.0, 1.0
    L = N.code_limit(K, bits)
    coef = S.code_coef(w, f)
    assert a * w * 2 ** f > L > a * w * 2 ** f / 64
    x, xi = np.zeros(N.BLOCK, f32), np.zeros(N.BLOCK, f32)
    xi[1234] = a
    q, sat, bad = N.codes_narrow(x, xi, coef, K, bits, ROT_SEED, 9, RND)
    assert (sat, bad) == (0, 0) and set(np.unique(np.abs(q))) == {4}
    q_id, sat_id, _ = N.encode_narrow32(xi - x, coef, L, N.draws(N.BLOCK, 9, RND))
    assert sat_id == 1 and q_id[1234] == L


# ---- the protocol in numpy ---------------------------------------------------------------------------------------------------------------
def _round(K, t, rnd, bits, seed=11):
    from fedfr_amd import secagg as P
    parts = [3 * c + 1 for c in range(K)]
    r = rng(seed)
    clients = [P.SecAggClient(c, 12, r, bits, ROT_SEED) for c in parts]
    srv = P.SecAggServer(parts, t, rnd)
    for c in clients:
        srv.register(c.cid, c.begin_round(rnd))
    for c in clients:
        srv.deliver_shares(c.cid, c.make_shares(parts, t))
    return clients, srv, parts


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("K, ndrop", [(3, 1), (3, 2), (5, 1), (5, 2)])
def test_masks_cancel_field_wise_in_the_restatement(K, ndrop, bits):
    """the field-wise sum of the survivors' masked uploads and the recovery streams == the sum of their plain codes, exactly, and decodes to
    the restatement's aggregate; a masked upload differs from its packed codes in every word.  (K = 3 with two dropped clients leaves one
    survivor, fewer than any threshold: the protocol refuses the round, and that is what is asserted there.)"""
    n, t, rnd, f = 4097, K // 2 + 1, 5, 12
    g = np.random.default_rng(K)
    x = (g.standard_normal(n) * 0.05).astype(f32)
    xs = [(x + g.standard_normal(n).astype(f32) * f32(1e-3)).astype(f32) for _ in range(K)]
    ws = [f32(1.0 / K)] * K
    clients, srv, parts = _round(K, t, rnd, bits)
    assert all(c.rounding_seed is not None for c in clients) and len({c.rounding_seed for c in clients}) == K
    ys, plain, codes = [], [], []
    for c, xi, w in zip(clients, xs, ws):
        y, sat, bad, q = N.mask_narrow(x, xi, S.code_coef(w, f), K, bits, ROT_SEED, c.rounding_seed, rnd, c.streams(parts, srv.public_keys, rnd))
        assert bad == 0
        ys.append(y), plain.append(N.pack(q, bits)), codes.append(q.astype(i64))
    keep = [p for p in range(K) if not 1 <= p <= ndrop]
    if len(keep) < t:
        with pytest.raises(RuntimeError, match="threshold"):
            srv.recovery_streams([parts[p] for p in keep])
        return
    rec = srv.recovery_streams([parts[p] for p in keep])
    nw = N.padded_count(n) * bits // 32
    got = N.stream_sum_fields(nw, rec, bits)
    for p in keep:
        got = N.field_add(got, ys[p], bits)
        assert ys[p].size == nw and np.count_nonzero(ys[p] == plain[p]) == 0
    want = sum(codes[p] for p in keep)
    assert np.abs(want).max() <= 2 ** (bits - 1) - 1
    assert np.array_equal(N.unpack(got, bits), want)
    out = N.aggregate_narrow(x, [ys[p] for p in keep], rec, bits, f, 1.0, ROT_SEED, rnd, n)
    assert out.dtype == f32 and np.array_equal(out, N.decode_narrow(N.pack(want, bits), bits, f, 1.0, ROT_SEED, rnd, n, x))
    # and the aggregate is the weighted mean of the survivors up to the rounding of the codes: K_s half-units through an orthonormal map
    mean = x.astype(f64) + sum(float(ws[p]) * (xs[p].astype(f64) - x) for p in keep)
    assert np.abs(out - mean).max() < 6 * np.sqrt(len(keep)) * 0.5 * 2.0 ** -f + 1e-6


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------
def test_python_surface_of_the_widths():
    from fedfr_amd import secagg as P
    assert P.code_limit(8) == S.code_limit(8) and P.code_limit(8, 32) == S.code_limit(8)
    assert [P.code_limit(K, b) for K, b in ((2, 8), (32, 8), (3, 16), (32, 16))] == [63, 3, 10922, 1023]
    assert [P.padded_count(n) for n in (0, 1, 4096, 4097)] == [0, 4096, 4096, 8192] == [N.padded_count(n) for n in (0, 1, 4096, 4097)]
    for bad in (4, 0, 64, 8.0, True, None):
        with pytest.raises(ValueError, match="secagg_bits"):
            P.SecAggClient(0, 24, None, bad)
    for bad in (-1, 2 ** 64, 1.5):
        with pytest.raises(ValueError, match="secagg_rotation_seed"):
            P.SecAggClient(0, 24, None, 8, bad)
    # the 32-bit path draws what it always drew: the same secrets from the same generator, and no rounding seed
    a, b, c = P.SecAggClient(0, 24, rng(3)), P.SecAggClient(0, 24, rng(3), 32), P.SecAggClient(0, 24, rng(3), 8)
    for cl in (a, b, c):
        cl.begin_round(1), cl.make_shares([0, 1, 2], 2)
    assert (a.secret_key, a.self_seed, a.rounding_seed) == (b.secret_key, b.self_seed, None)
    assert (c.secret_key, c.self_seed) == (a.secret_key, a.self_seed) and 0 <= c.rounding_seed < 2 ** 64
    up = P.MaskedUpdate(torch.zeros(1024, dtype=torch.int32), 4000, 12, torch.zeros(3), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), bits=8)
    assert up.bits == 8 and up.nbytes == 4096 * 8 // 8 + 12 + 16 and up.dense_nbytes == 16000 + 12 + 16
    assert P.MaskedUpdate(torch.zeros(8, dtype=torch.int32), 8, 24, torch.zeros(0), torch.zeros(0, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)).bits == 32


def test_fedsecagg_refuses_mixed_and_unexpected_widths():
    from fedfr_amd import secagg as P, server
    from fedfr_amd.client import FlatStateDict
    cpu = FlatStateDict.from_flat((torch.zeros(8), torch.zeros(0), torch.zeros(0, dtype=torch.int64)), [], [])

    def up(bits):
        words = 8 if bits == 32 else 4096 * bits // 32
        return P.MaskedUpdate(torch.zeros(words, dtype=torch.int32), 8, 24, torch.zeros(0), torch.zeros(0, dtype=torch.int64), torch.zeros(2, dtype=torch.int32),
                              bits=bits)
    for a, b in ((8, 16), (8, 32), (32, 16)):
        with pytest.raises(RuntimeError, match="different widths"):
            server.FedSecAgg(cpu, [up(a), up(b)], [1.0, 1.0], [])
    for have, want in ((8, 16), (32, 8), (16, 32)):
        with pytest.raises(RuntimeError, match="%d-bit words, the server expects %d-bit" % (have, want)):
            server.FedSecAgg(cpu, [up(have), up(have)], [1.0, 1.0], [], bits=want)
    with pytest.raises(ValueError, match="secagg_bits"):
        server.FedSecAgg(cpu, [up(8)], [1.0], [], bits=4)
    with pytest.raises(RuntimeError, match="GPU"):                # one width, the expected one: on to the checks of every round
        server.FedSecAgg(cpu, [up(8), up(8)], [1.0, 1.0], [], bits=8)


def test_server_train_refuses_secagg_bits_settings_before_any_client_trains():
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
        srv.args, srv.robust_agg, srv.server_opt = Args, None, None
        return srv

    for aggr in ("FedAvg", "FedAdam"):
        for bad in (4, 0, 12, 64, 8.0, True, "8"):
            with pytest.raises(ValueError, match="secagg_bits must be 8, 16 or 32"):
                world(aggr, secure_aggregation=True, secagg_bits=bad).train()
        for bits in (8, 16, 32):
            with pytest.raises(ValueError, match="secagg_bits=%d needs secure_aggregation" % bits):
                world(aggr, secagg_bits=bits).train()
        for bits in (8, 16):
            with pytest.raises(ValueError, match=r"secagg_bits=%d cannot be combined with distributed_dp.*not provided" % bits):
                world(aggr, secure_aggregation=True, secagg_bits=bits, distributed_dp=True, dp_noise_multiplier=1.0, clip_norm=1.0,
                      dp_uniform_weights=True).train()
            with pytest.raises(ValueError, match="secagg_rotation_seed"):
                world(aggr, secure_aggregation=True, secagg_bits=bits, secagg_rotation_seed=-1).train()
        for ok in (dict(secagg_bits=8), dict(secagg_bits=16, secagg_rotation_seed=5, secagg_drop=[2]), dict(secagg_bits=32), dict(secagg_bits=None)):
            with pytest.raises(AssertionError, match="a client was touched"):        # a servable setting: the round starts
                world(aggr, secure_aggregation=True, **ok).train()


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_host_side_checks_of_the_narrow_entry_points(built_lib):
    """what the entry points refuse, they refuse on the host before any HIP call: FEDFR_ERR_ARG and a message naming the entry and the
    offending value, without a GPU (dummy host pointers: every call fails its checks first); n = 0 is a successful no-op"""
    lib = built_lib.lib()
    err_arg = int(re.search(r"#define FEDFR_ERR_ARG \((-?\d+)\)", open(os.path.join(REPO, "include", "fedfr_hip.h")).read()).group(1))
    buf = (C.c_float * 64)()
    base = C.addressof(buf)
    base += -base % 16
    keys, nonces = (C.c_uint * (8 * 33))(), (C.c_uint * (3 * 33))()

    def signs(*v):
        return (C.c_int * max(len(v), 1))(*v)

    def refused(rc, *words):
        msg = lib.fedfr_last_error_string().decode()
        assert rc == err_arg and all(w in msg for w in words), (rc, msg)

    assert [lib.fedfr_rht_padded_count(n) for n in (0, 1, 4096, 4097)] == [0, 4096, 4096, 8192]

    def rht(dst=base, src=base + 64, n=8, inverse=0):
        return lib.fedfr_rht_fill(dst, src, n, 1, 2, inverse, None)
    refused(rht(dst=None), "rht_fill", "dst=(nil)")
    refused(rht(src=None), "rht_fill", "src=(nil)")
    refused(rht(src=base), "rht_fill", "distinct")
    refused(rht(dst=base + 4), "rht_fill", "aligned")
    assert rht(n=0) == 0

    def mask(y=base, x=base + 64, xi=base + 128, coef=1.0, K=2, bits=8, keys_=keys, nonces_=nonces, signs_=signs(1, -1), k=2, counter0=0, n=8, counters=None):
        return lib.fedfr_secagg_mask_narrow(y, x, xi, coef, K, bits, 1, 2, 3, keys_, nonces_, signs_, k, counter0, n, counters, None)
    who = "secagg_mask_narrow"
    refused(mask(y=None), who, "y=(nil)")
    refused(mask(x=None), who, "x=(nil)")
    refused(mask(xi=None), who, "xi=(nil)")
    for bits in (0, 4, 12, 32):
        refused(mask(bits=bits), who, "bits=%d" % bits)
    refused(mask(K=0), who, "K=0")
    refused(mask(K=128), who, "K=128", "127")
    refused(mask(K=32768, bits=16), who, "K=32768")
    refused(mask(k=-1), who, "k=-1")
    refused(mask(k=33), who, "k=33")
    refused(mask(keys_=None), who, "keys=(nil)")
    refused(mask(signs_=signs(1, 0)), who, "sign 1 is 0")
    refused(mask(y=base + 4), who, "aligned")
    refused(mask(xi=base + 8), who, "aligned")
    refused(mask(counters=base + 2), who, "counters")
    # the 32-bit block counter: a rotation block is 64 ChaCha20 blocks per stream at 8 bits, 128 at 16
    refused(mask(counter0=0xFFFFFFFF - 62), who, "overflows", "counter0=4294967233")
    refused(mask(counter0=0xFFFFFFFF - 126, bits=16), who, "overflows")
    refused(mask(n=4097, counter0=0xFFFFFFFF - 126), who, "overflows")
    refused(mask(n=64 * 2 ** 32 + 1), who, "overflows")
    assert mask(n=0) == 0 and mask(n=0, k=0, keys_=None, nonces_=None, signs_=None, counter0=0xFFFFFFFF) == 0

    ptrs = (C.c_void_p * 9)(*[base] * 9)

    def aggregate(out=base, x=base, acc=None, ys=ptrs, ku=2, bits=8, keys_=keys, nonces_=nonces, signs_=signs(1, -1), k=2, counter0=0, frac_bits=12,
                  rescale=1.0, n=8, first=1, last=1):
        return lib.fedfr_secagg_aggregate_narrow(out, x, acc, ys, ku, bits, 1, 2, keys_, nonces_, signs_, k, counter0, frac_bits, rescale, n, first, last,
                                                 None)
    who = "secagg_aggregate_narrow"
    refused(aggregate(ku=-1), who, "ku=-1")
    refused(aggregate(ku=9), who, "ku=9")
    refused(aggregate(bits=32), who, "bits=32")
    refused(aggregate(k=33), who, "k=33")
    refused(aggregate(ku=0, k=0), who, "ku=0", "k=0")
    refused(aggregate(ys=None), who, "ys=(nil)")
    refused(aggregate(ys=(C.c_void_p * 2)(base, None)), who, "upload 1 is null")
    refused(aggregate(signs_=signs(1, 3)), who, "sign 1 is 3")
    refused(aggregate(frac_bits=-1), who, "frac_bits=-1")
    refused(aggregate(frac_bits=31), who, "frac_bits=31")
    refused(aggregate(rescale=float("nan")), who, "rescale=nan")
    refused(aggregate(first=0), who, "first=0 last=1", "acc")
    refused(aggregate(last=0), who, "first=1 last=0", "acc")
    refused(aggregate(out=None), who, "out")
    refused(aggregate(out=base + 4), who, "aligned")
    refused(aggregate(ys=(C.c_void_p * 2)(base, base + 4)), who, "aligned")
    refused(aggregate(counter0=0xFFFFFFFF - 62), who, "overflows")
    refused(aggregate(counter0=0xFFFFFFFF - 126, bits=16), who, "overflows")
    assert aggregate(n=0) == 0 and aggregate(n=0, x=None, ku=0) == 0 and aggregate(n=0, out=None, acc=base, last=0) == 0


def test_no_narrow_kernel_uses_scratch_memory(built_lib):
    """the rule of tests/test_abi.py::test_hot_kernels_do_not_spill for the kernels of csrc/secagg_narrow.hip in both builds, read from the
    code objects' metadata (tools/kernel_resources.py): the rotation, the mask pass at both widths and the 2 x 9 aggregates"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr.kernels(built_lib.LIB_PATH)
    bf16 = os.path.join(os.path.dirname(built_lib.LIB_PATH), "libfedfr_hip_bf16.so")
    if os.path.exists(bf16) and os.path.basename(built_lib.LIB_PATH) != "libfedfr_hip_bf16.so":
        ks.update({"bf16:" + k: v for k, v in kr.kernels(bf16).items()})
    builds = 2 if any(k.startswith("bf16:") for k in ks) else 1
    agg = {n: r for n, r in ks.items() if "secagg_aggregate_narrow_kernel" in n}
    rest = {n: r for n, r in ks.items() if "secagg_mask_narrow_kernel" in n or "rht_fill_kernel" in n}
    assert len(agg) == 18 * builds and len(rest) == 3 * builds, (len(agg), sorted(rest))
    bad = [(n, r) for n, r in list(agg.items()) + list(rest.items()) if r["scratch"]]
    assert not bad, bad
    # static LDS: the padded rotation buffer (5376 words) and the sign words (128); mask and aggregate add the partial mask sums (4096 words)
    assert all(r["lds"] == (4 * (5376 + 128) if "rht_fill_kernel" in n else 4 * (5376 + 128 + 4096)) for n, r in list(agg.items()) + list(rest.items()))
