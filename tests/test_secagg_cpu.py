"""Secure aggregation, the part that needs no GPU: the ChaCha20 restatement of tests/secagg_cases.py (which fedfr_chacha20_fill is held to
bit for bit on the GPU) against RFC 8439, X25519 against RFC 7748, Shamir sharing, the cancellation of the masks in the restatement with
and without dropped clients, the laws of the encoding, the host-side argument checks of the new C entry points, no scratch memory in any
new kernel, and the combinations Server.train refuses before any client trains."""
import ctypes as C
import importlib.util
import itertools
import os
import re

import numpy as np
import pytest
import torch

import secagg_cases as S
from conftest import REPO

f32, f64, u32, i32 = np.float32, np.float64, np.uint32, np.int32


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from fedfr_amd import _C
    return _C


def rng(seed):
    return np.random.default_rng(seed).bytes


# ---- the generator's restatement -----------------------------------------------------------------------------------------------------------
def test_chacha20_restatement_rfc8439_block():
    """RFC 8439 section 2.3.2: key bytes 00 ... 1f, counter 1, nonce words (0x09000000, 0x4a000000, 0)"""
    assert S.RFC_KEY[0] == 0x03020100 and S.RFC_KEY[7] == 0x1F1E1D1C
    got = S.chacha20_blocks(S.RFC_KEY, [S.RFC_COUNTER], S.RFC_NONCE)
    assert got.shape == (1, 16) and got.dtype == u32
    assert ["%08x" % int(w) for w in got[0]] == S.RFC_WORDS


def test_stream_indexing_of_the_restatement():
    """element e is word e % 16 of block counter0 + e / 16; a stream at counter0 = c is the stream at 0 from element 16 c on; every
    coordinate matters; the counter is one 32-bit word"""
    key, nonce = S.RFC_KEY, S.RFC_NONCE
    w = S.words(100, key, 0, nonce)
    assert w.dtype == u32 and w.shape == (100,)
    assert ["%08x" % int(a) for a in w[16:32]] == S.RFC_WORDS
    assert np.array_equal(S.words(40, key, 2, nonce), w[32:72])
    assert np.array_equal(S.words(16, key, 0xFFFFFFFF, nonce), S.chacha20_blocks(key, [0xFFFFFFFF], nonce)[0])
    with pytest.raises(AssertionError):
        S.words(17, key, 0xFFFFFFFF, nonce)
    others = [S.words(16, (key[0] ^ 1,) + key[1:], 0, nonce), S.words(16, key[:7] + (key[7] ^ 0x80000000,), 0, nonce), S.words(16, key, 1, nonce)]
    others += [S.words(16, key, 0, tuple(v ^ (1 if q == j else 0) for q, v in enumerate(nonce))) for j in range(3)]
    for o in others:
        assert not np.any(o == w[:16])


# ---- the host side of the protocol ---------------------------------------------------------------------------------------------------------
def test_x25519_rfc7748_diffie_hellman():
    """RFC 7748 section 6.1"""
    from fedfr_amd import secagg as P
    a = bytes.fromhex("77076d0a7318a57d3c16c17251b26645df4c2f87ebc0992ab177fba51db92c2a")
    b = bytes.fromhex("5dab087e624a8a4b79e17f8b83800ee66f3bb1292618b6fd1c2f8b27ff88e0eb")
    pa, pb = P.x25519(a, P.BASE_POINT), P.x25519(b, P.BASE_POINT)
    assert pa.hex() == "8520f0098930a754748b7ddcb43ef75a0dbf3a0d26381af4eba4a98eaa9b4e6a"
    assert pb.hex() == "de9edb7d7b7dc1b4d35b61c2ece435373f8343c85b78674dadfc7e146f882b4f"
    shared = "4a5d9d5ba4ce2de1728e3bf480350f25e07e21c947d19e3376f09b3c1e161742"
    assert P.x25519(a, pb).hex() == shared and P.x25519(b, pa).hex() == shared
    # RFC 7748 section 5.2, first vector: an arbitrary point and the masking of the top bit
    k = bytes.fromhex("a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4")
    u = bytes.fromhex("e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c")
    assert P.x25519(k, u).hex() == "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552"
    sk, pk = P.keypair(rng(1))
    assert len(sk) == len(pk) == 32 and pk == P.x25519(sk, P.BASE_POINT) and P.keypair(rng(1)) == (sk, pk)
    with pytest.raises(ValueError, match="32 bytes"):
        P.x25519(b"short", pk)


def test_derive_key_is_symmetric_and_separates_pairs():
    from fedfr_amd import secagg as P
    shared = bytes(range(32))
    k = P.derive_key(shared, 3, 5)
    assert len(k) == 8 and all(0 <= w < 2 ** 32 for w in k) and k == P.derive_key(shared, 5, 3)
    assert k != P.derive_key(shared, 3, 6) and k != P.derive_key(bytes(32), 3, 5)
    assert P.key_words(bytes(range(32))) == S.RFC_KEY
    assert P.round_nonce(7 | 9 << 32, 1) == (7, 9, 1)


@pytest.mark.parametrize("k, t", [(3, 2), (8, 5), (32, 17)])
def test_shamir_every_threshold_subset_reconstructs(k, t):
    """every t-subset of the k shares gives the secret back (sampled for (32, 17): 601080390 subsets); t - 1 shares, duplicate shares and
    mixed shares are refused"""
    from fedfr_amd import secagg as P
    secret = np.random.default_rng(k).bytes(32)
    shares = P.shamir_split(secret, k, t, rng(7))
    assert [s[0] for s in shares] == list(range(1, k + 1)) and all(s[1] == t and len(s[2]) == 32 for s in shares)
    if k <= 8:
        subsets = list(itertools.combinations(range(k), t))
    else:
        g = np.random.default_rng(5)
        subsets = [tuple(g.permutation(k)[:t]) for _ in range(20)]
    for sub in subsets:
        assert P.shamir_combine([shares[j] for j in sub]) == secret, sub
    assert P.shamir_combine(shares) == secret
    with pytest.raises(ValueError, match="%d shares, the threshold is %d" % (t - 1, t)):
        P.shamir_combine(shares[:t - 1])
    with pytest.raises(ValueError, match="duplicate"):
        P.shamir_combine(shares[:t - 1] + [shares[0]])
    with pytest.raises(ValueError, match="different"):
        P.shamir_combine(shares[:t - 1] + [P.shamir_split(secret, k, t + 1 if t < k else t - 1, rng(8))[t]])
    with pytest.raises(ValueError, match="shamir_split"):
        P.shamir_split(secret, 3, 4)


def _round(K, t, rnd, seed=11):
    """a round of the protocol on the host: (clients, server, participants) with deterministic secrets"""
    from fedfr_amd import secagg as P
    parts = [3 * c + 1 for c in range(K)]                  # ids that are not positions
    r = rng(seed)
    clients = [P.SecAggClient(c, 24, r) for c in parts]
    srv = P.SecAggServer(parts, t, rnd)
    for c in clients:
        srv.register(c.cid, c.begin_round(rnd))
    for c in clients:
        srv.deliver_shares(c.cid, c.make_shares(parts, t))
    return clients, srv, parts


@pytest.mark.parametrize("K", [2, 3, 8])
def test_masks_cancel_in_the_restatement(K):
    """sum of the masked uploads + the recovery streams == sum of the plain codes, word for word: nobody dropped, one client dropped,
    K - t clients dropped (t = K // 2 + 1)"""
    n, t, rnd = 100, K // 2 + 1, 5 | 1 << 32
    g = np.random.default_rng(K)
    x = (g.standard_normal(n) * 0.05).astype(f32)
    xs = [(x + g.standard_normal(n).astype(f32) * f32(1e-3)).astype(f32) for _ in range(K)]
    ws = g.random(K) + 0.1
    ws = [f32(w) for w in ws / ws.sum()]
    L = S.code_limit(K)
    for ndrop in sorted({0, 1, K - t}):
        clients, srv, parts = _round(K, t, rnd)
        ys, plain = [], []
        for c, xi, w in zip(clients, xs, ws):
            streams = c.streams(parts, srv.public_keys, rnd)
            assert len(streams) == K and streams[-1][1] == (5, 1, 1) and all(s[1] == (5, 1, 0) for s in streams[:-1])
            ys.append(S.mask_u32(x, xi, S.code_coef(w, 24), L, streams)[0])
            plain.append(S.encode32(x, xi, S.code_coef(w, 24), L)[0].view(u32))
        dropped = list(range(1, 1 + ndrop))                # positions of the clients whose upload never arrives
        keep = [p for p in range(K) if p not in dropped]
        if len(keep) < t:
            with pytest.raises(RuntimeError, match="threshold"):
                srv.recovery_streams([parts[p] for p in keep])
            continue
        rec = srv.recovery_streams([parts[p] for p in keep])
        assert len(rec) == len(keep) * (1 + ndrop)
        with np.errstate(over="ignore"):
            got = sum((ys[p] for p in keep), np.zeros(n, u32)) + S.stream_sum(n, rec)
            want = sum((plain[p] for p in keep), np.zeros(n, u32))
        assert got.dtype == u32 and np.array_equal(got, want), (K, ndrop)
        for p in keep:                                     # and a masked upload says nothing about its codes
            assert np.count_nonzero(ys[p] == plain[p]) == 0


def test_server_refuses_the_double_reconstruction_and_too_few_survivors():
    clients, srv, parts = _round(4, 3, 0)
    with pytest.raises(RuntimeError, match="2 survivors, the threshold is 3"):
        srv.recovery_streams(parts[:2])
    srv.recovery_streams(parts[:3])                        # client parts[3] dropped: its secret key is reconstructed ...
    with pytest.raises(RuntimeError, match="self seed of client %d after its secret key" % parts[3]):
        srv.reconstruct_self_seed(parts[3], parts)         # ... so its self seed must stay hidden
    with pytest.raises(RuntimeError, match="secret key of client %d after its self seed" % parts[0]):
        srv.reconstruct_secret_key(parts[0], parts)
    with pytest.raises(RuntimeError, match="with both the server could unmask"):
        srv.recovery_streams(parts[1:])                    # a later, different claim of who survived
    assert srv.reconstruct_secret_key(parts[3], parts[:3]) == clients[3].secret_key
    assert srv.reconstruct_self_seed(parts[1], parts[1:]) == clients[1].self_seed
    from fedfr_amd import secagg as P
    for bad in (1, 5, True, 2.0):
        with pytest.raises(ValueError, match="threshold"):
            P.SecAggServer(parts, bad)
    with pytest.raises(ValueError, match="participants"):
        P.SecAggServer([1], 2)
    with pytest.raises(ValueError, match="participants"):
        P.SecAggServer(list(range(33)), 2)
    with pytest.raises(RuntimeError, match="round 0, not of round 1"):
        clients[0].streams(parts, srv.public_keys, 1)
    assert P.survivor_rescale([0.25, 0.5, 0.25], [0, 1, 2]) == 1.0
    assert P.survivor_rescale([0.25, 0.5, 0.25], [0, 2]) == 2.0
    assert P.code_limit(8) == S.code_limit(8) == 268435455 and P.code_coef(0.3, 24) == float(S.code_coef(0.3, 24))


# ---- the encoding ------------------------------------------------------------------------------------------------------------------------
def test_encoding_saturates_at_exactly_the_limit_and_zeroes_non_finite_values():
    K = 8
    L, c = S.code_limit(K), S.code_coef(1.0, 24)
    assert L == (2 ** 31 - 1) // 8 and float(c) == 2.0 ** 24
    x, xi = S.planted_inputs(64, c, L)
    q, sat, bad = S.encode32(x, xi, c, L)
    assert q.dtype == i32 and list(q[:6]) == [L, -L, 0, 0, 0, 0]
    assert list(q[6:11]) == [0, 2, 2, 0, -2]                 # ties go to the even neighbour
    assert q[11] == L                                        # float(L) rounds up to 2^28: clamped back to L
    assert (sat, bad) == (3, 4) and np.abs(q[12:]).max() < L
    assert K * L <= 2 ** 31 - 1 < K * (L + 1)                # the sum of K codes stays inside int32
    # t = L - 1 is not saturated, t = L and everything beyond is; exactly representable at a small limit
    xs = np.array([99, 100, 101, -99, -100, -101, 1e30], f32)
    q, sat, bad = S.encode32(np.zeros(7, f32), xs, f32(1), 100)
    assert list(q) == [99, 100, 100, -99, -100, -100, 100] and (sat, bad) == (5, 0)


@pytest.mark.parametrize("K, drop", [(2, 0), (3, 0), (8, 0), (3, 1), (8, 3)])
@pytest.mark.parametrize("frac_bits", [8, 24, 30])
def test_aggregate_within_the_law_bound_of_the_fp64_mean(K, drop, frac_bits):
    n = 4100
    g = np.random.default_rng(100 * K + frac_bits)
    x = (g.standard_normal(n) * 0.05).astype(f32)
    xs = [(x + g.standard_normal(n).astype(f32) * f32(2e-3 * (1 + i))).astype(f32) for i in range(K)]
    w = g.random(K) + 0.1
    w = [f32(a) for a in w / w.sum()]
    keep = list(range(K - drop))
    L = S.code_limit(K)
    codes = [S.encode32(x, xs[i], S.code_coef(w[i], frac_bits), L) for i in keep]
    assert all(sat == 0 and bad == 0 for _, sat, bad in codes)
    rescale = 1.0 if not drop else float(f32(1.0 / sum(float(w[i]) for i in keep)))
    out = S.aggregate32(x, [q.view(u32) for q, _, _ in codes], [], frac_bits, rescale)
    assert out.dtype == f32
    mean, bound = S.law_bound(x, [xs[i] for i in keep], [float(w[i]) * 1.0 for i in keep], frac_bits, rescale)
    err = np.abs(out.astype(f64) - mean)
    print("K=%d drop=%d f=%d: worst error / bound %.3f" % (K, drop, frac_bits, float((err / bound).max())))
    assert np.all(err <= bound)
    if not drop:                                             # the form the bound takes with nobody dropped
        d = sum(float(w[i]) * np.abs(xs[i].astype(f64) - x) for i in keep)
        assert np.allclose(bound, K * 2.0 ** -(frac_bits + 1) + 2.0 ** -21 * (d + np.abs(mean)), rtol=1e-12, atol=0)
    # without x the same sum is the pseudo-gradient, and x + it is the result
    delta = S.aggregate32(None, [q.view(u32) for q, _, _ in codes], [], frac_bits, rescale)
    assert np.array_equal(out, x + delta)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_host_side_checks_of_the_new_entry_points(built_lib):
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

    fill = lib.fedfr_chacha20_fill
    refused(fill(None, 8, keys, 0, nonces, None), "chacha20_fill", "dst=(nil)")
    refused(fill(base, 8, None, 0, nonces, None), "chacha20_fill", "key=(nil)")
    refused(fill(base, 8, keys, 0, None, None), "chacha20_fill", "nonce=(nil)")
    refused(fill(base + 4, 8, keys, 0, nonces, None), "chacha20_fill", "aligned")
    refused(fill(base, 17, keys, 0xFFFFFFFF, nonces, None), "chacha20_fill", "counter0=4294967295", "n=17")
    refused(fill(base, 16 * 2 ** 32 + 1, keys, 0, nonces, None), "chacha20_fill", "overflows")
    assert fill(base, 0, keys, 0xFFFFFFFF, nonces, None) == 0

    def mask(y=base, x=base + 64, xi=base + 128, coef=1.0, limit=100, keys_=keys, nonces_=nonces, signs_=signs(1, -1), k=2, n=8, counters=None):
        return lib.fedfr_secagg_mask(y, x, xi, coef, limit, keys_, nonces_, signs_, k, n, counters, None)

    refused(mask(y=None), "secagg_mask", "y=(nil)")
    refused(mask(x=None), "secagg_mask", "x=(nil)")
    refused(mask(xi=None), "secagg_mask", "xi=(nil)")
    refused(mask(k=-1), "secagg_mask", "k=-1")
    refused(mask(k=33), "secagg_mask", "k=33")
    refused(mask(keys_=None), "secagg_mask", "keys=(nil)")
    refused(mask(nonces_=None), "secagg_mask", "nonces=(nil)")
    refused(mask(signs_=None), "secagg_mask", "signs=(nil)")
    refused(mask(signs_=signs(1, 0)), "secagg_mask", "sign 1 is 0")
    refused(mask(signs_=signs(2, 1)), "secagg_mask", "sign 0 is 2")
    refused(mask(limit=0), "secagg_mask", "limit=0")
    refused(mask(limit=-5), "secagg_mask", "limit=-5")
    refused(mask(y=base + 4), "secagg_mask", "aligned")
    refused(mask(xi=base + 8), "secagg_mask", "aligned")
    refused(mask(counters=base + 2), "secagg_mask", "counters")
    refused(mask(n=16 * 2 ** 32 + 1), "secagg_mask", "overflows")
    assert mask(n=0) == 0 and mask(n=0, k=0, keys_=None, nonces_=None, signs_=None) == 0

    ptrs = (C.c_void_p * 9)(*[base] * 9)

    def aggregate(out=base, x=base, acc=None, ys=ptrs, ku=2, keys_=keys, nonces_=nonces, signs_=signs(1, -1), k=2, frac_bits=24, rescale=1.0, n=8,
                  first=1, last=1):
        return lib.fedfr_secagg_aggregate(out, x, acc, ys, ku, keys_, nonces_, signs_, k, frac_bits, rescale, n, first, last, None)

    refused(aggregate(ku=-1), "secagg_aggregate", "ku=-1")
    refused(aggregate(ku=9), "secagg_aggregate", "ku=9")
    refused(aggregate(k=33), "secagg_aggregate", "k=33")
    refused(aggregate(k=-2), "secagg_aggregate", "k=-2")
    refused(aggregate(ku=0, k=0), "secagg_aggregate", "ku=0", "k=0")
    refused(aggregate(ys=None), "secagg_aggregate", "ys=(nil)")
    refused(aggregate(ys=(C.c_void_p * 2)(base, None)), "secagg_aggregate", "upload 1 is null")
    refused(aggregate(keys_=None), "secagg_aggregate", "keys=(nil)")
    refused(aggregate(signs_=signs(1, 3)), "secagg_aggregate", "sign 1 is 3")
    refused(aggregate(frac_bits=7), "secagg_aggregate", "frac_bits=7")
    refused(aggregate(frac_bits=31), "secagg_aggregate", "frac_bits=31")
    refused(aggregate(rescale=float("inf")), "secagg_aggregate", "rescale=inf")
    refused(aggregate(rescale=float("nan")), "secagg_aggregate", "rescale=nan")
    refused(aggregate(first=0), "secagg_aggregate", "first=0 last=1", "acc")
    refused(aggregate(last=0), "secagg_aggregate", "first=1 last=0", "acc")
    refused(aggregate(out=None), "secagg_aggregate", "out")
    refused(aggregate(out=base + 4), "secagg_aggregate", "aligned")
    refused(aggregate(acc=base + 8, last=0), "secagg_aggregate", "aligned")
    refused(aggregate(ys=(C.c_void_p * 2)(base, base + 4)), "secagg_aggregate", "aligned")
    refused(aggregate(n=16 * 2 ** 32 + 1), "secagg_aggregate", "overflows")
    assert aggregate(n=0) == 0 and aggregate(n=0, x=None, ku=0) == 0 and aggregate(n=0, out=None, acc=base, last=0) == 0


def test_no_new_kernel_uses_scratch_memory(built_lib):
    """the rule of tests/test_abi.py::test_hot_kernels_do_not_spill for the kernels of csrc/secagg.hip in both builds, read from the code
    objects' metadata (tools/kernel_resources.py): the fill, the mask pass and the 9 upload counts of the aggregate"""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr.kernels(built_lib.LIB_PATH)
    bf16 = os.path.join(os.path.dirname(built_lib.LIB_PATH), "libfedfr_hip_bf16.so")
    if os.path.exists(bf16) and os.path.basename(built_lib.LIB_PATH) != "libfedfr_hip_bf16.so":
        ks.update({"bf16:" + k: v for k, v in kr.kernels(bf16).items()})
    builds = 2 if any(k.startswith("bf16:") for k in ks) else 1
    agg = {n: r for n, r in ks.items() if "secagg_aggregate_kernel" in n}
    rest = {n: r for n, r in ks.items() if "secagg_mask_kernel" in n or "chacha20_fill_kernel" in n}
    assert len(agg) == 9 * builds and len(rest) == 2 * builds, (len(agg), sorted(rest))
    bad = [(n, r) for n, r in list(agg.items()) + list(rest.items()) if r["scratch"]]
    assert not bad, bad
    # static LDS: the exchange buffer of mask and aggregate, 4 KiB per wave, four waves; none in the fill
    assert all(r["lds"] == (0 if "chacha20_fill_kernel" in n else 16384) for n, r in list(agg.items()) + list(rest.items()))


# ---- Server.train ------------------------------------------------------------------------------------------------------------------------
def test_server_train_refuses_secagg_settings_before_any_client_trains():
    from fedfr_amd import server

    class NeverTrains:
        cid = 0

        def __getattr__(self, name):
            raise AssertionError("a client was touched (%s): the round has started" % name)

        def __setattr__(self, name, value):
            raise AssertionError("a client was touched (%s): the round has started" % name)

    servers = {}

    def world(aggr, nclients=3, **extra):
        """a server of ``nclients`` clients that must never be touched, with fresh args (one server per client count: building its model
        is what takes time, and what train() refuses it refuses from the args alone)"""
        Args = type("Args", (), dict(network="iresnet18", loss="CosFace", local_epoch=1, output_dir="/tmp", BCE_local=False, aggr_alg=aggr, **extra))
        srv = servers.get(nclients)
        if srv is None:
            srv = servers[nclients] = server.Server([NeverTrains() for _ in range(nclients)], None, Args, device=torch.device("cpu"))
        srv.args, srv.robust_agg, srv.server_opt = Args, None, None
        return srv

    for kind in sorted(server.ROBUST_ALG_KINDS):
        with pytest.raises(ValueError, match=r"secure_aggregation.*%s" % kind):
            world(kind, 5, secure_aggregation=True).train()
    for aggr in ("FedAvg", "FedProx", "FedAdam"):
        for bits in (4, 8):
            with pytest.raises(ValueError, match=r"secure_aggregation.*compress_bits=%d" % bits):
                world(aggr, secure_aggregation=True, compress_bits=bits).train()
        with pytest.raises(ValueError, match=r"secure_aggregation.*topk_ratio=0.01"):
            world(aggr, secure_aggregation=True, topk_ratio=0.01).train()
        with pytest.raises(ValueError, match=r"secure_aggregation.*dp_noise_multiplier=1.1"):
            world(aggr, secure_aggregation=True, dp_noise_multiplier=1.1, clip_norm=2.0).train()
        with pytest.raises(ValueError, match=r"secure_aggregation.*clip_norm=2.0"):
            world(aggr, secure_aggregation=True, clip_norm=2.0).train()
        with pytest.raises(ValueError, match=r"secure_aggregation.*return_all"):
            world(aggr, secure_aggregation=True, return_all=True, add_pretrained_data=True).train()
        with pytest.raises(ValueError, match=r"2 to 32 participants \(got 1\)"):
            world(aggr, 1, secure_aggregation=True).train()
        with pytest.raises(ValueError, match=r"2 to 32 participants \(got 33\)"):
            world(aggr, 33, secure_aggregation=True).train()
        for bad in (1, 4, 0, -1, 2.5, True):
            with pytest.raises(ValueError, match="secagg_threshold"):
                world(aggr, secure_aggregation=True, secagg_threshold=bad).train()
        for bad in (7, 31, 24.0, None):
            with pytest.raises(ValueError, match="secagg_frac_bits"):
                world(aggr, secure_aggregation=True, secagg_frac_bits=bad).train()
        with pytest.raises(ValueError, match=r"secagg_drop=\[5\]"):
            world(aggr, secure_aggregation=True, secagg_drop=[5]).train()
        with pytest.raises(ValueError, match=r"secagg_drop=\[0, 1\] leaves 1 of 3 uploads, fewer than secagg_threshold=2"):
            world(aggr, secure_aggregation=True, secagg_drop=[1, 0]).train()
    with pytest.raises(AssertionError, match="a client was touched"):                # off: nothing is refused and the round starts
        world("FedAvg", secure_aggregation=False, secagg_threshold=99).train()
    for ok in (dict(), dict(secagg_threshold=3), dict(secagg_frac_bits=16, secagg_drop=[2])):
        with pytest.raises(AssertionError, match="a client was touched"):            # a servable setting: the round starts too
            world("FedAdam", secure_aggregation=True, **ok).train()


def test_fedsecagg_refuses_what_it_cannot_serve():
    from fedfr_amd import secagg as P, server
    from fedfr_amd.client import FlatStateDict
    cpu = FlatStateDict.from_flat((torch.zeros(8), torch.zeros(0), torch.zeros(0, dtype=torch.int64)), [], [])
    up = P.MaskedUpdate(torch.zeros(8, dtype=torch.int32), 8, 24, torch.zeros(0), torch.zeros(0, dtype=torch.int64), torch.zeros(2, dtype=torch.int32))
    assert up.nbytes == up.dense_nbytes == 32
    with pytest.raises(RuntimeError, match="FlatStateDict"):
        server.FedSecAgg({"w": torch.zeros(8)}, [up], [1.0], [])
    with pytest.raises(RuntimeError, match="MaskedUpdates"):
        server.FedSecAgg(cpu, [cpu], [1.0], [])
    with pytest.raises(RuntimeError, match="weights"):
        server.FedSecAgg(cpu, [up, up], [1.0], [])
    with pytest.raises(ValueError, match="clip_norm"):
        server.FedSecAgg(cpu, [up], [1.0], [], 1.0, server.ServerOptimizer("ADAM", clip_norm=1.0))
    with pytest.raises(ValueError, match="robust"):
        server.FedSecAgg(cpu, [up], [1.0], [], 1.0, server.RobustAggregator("Krum"))
    for bad in (0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="rescale"):
            server.FedSecAgg(cpu, [up], [1.0], [], bad)
    with pytest.raises(RuntimeError, match="GPU"):
        server.FedSecAgg(cpu, [up], [1.0], [])
    with pytest.raises(RuntimeError, match="FlatStateDict"):
        P.SecAggClient(0).mask({"w": 1}, cpu, 0.5, [0, 1], {}, 0)
    with pytest.raises(ValueError, match="frac_bits"):
        P.SecAggClient(0, 31)
