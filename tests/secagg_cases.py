"""Restatements for the secure-aggregation kernels (csrc/secagg.h, csrc/secagg.hip; the format: include/fedfr_hip.h, "THE MASK STREAM").

* ``chacha20_blocks`` / ``words``: the ChaCha20 block function of RFC 8439 section 2.3 in numpy uint32 arithmetic and the stream's
  indexing (element e = word e % 16 of block counter0 + e / 16).  ``fedfr_chacha20_fill`` is held to ``words`` BIT FOR BIT.
* ``encode32``: the fixed-point encoding in float32, one operation per line, with the clamp and the two counters.
* ``mask_u32``: ``fedfr_secagg_mask``: the codes plus the signed streams mod 2^32.
* ``aggregate32``: ``fedfr_secagg_aggregate`` in ONE order (addition mod 2^32 is associative and commutative: every chaining of the
  kernel must give these bits).
* ``law_bound``: how far the aggregate may be from the fp64 weighted mean.

THE LAW BOUND.  Per element, with w_i the fp32 weights of the K_s clients whose uploads are summed, d_i = x_i - x exactly,
R = rescale (1 when nobody dropped), f = frac_bits, u = 2^-24, and x' = x + R sum_i w_i d_i the fp64 value:
  1. d = fl(x_i - x) and t = fl(d c_i), c_i = w_i 2^f exactly: two roundings, |t - w_i d_i 2^f| <= (2 u + u^2) w_i |d_i| 2^f.
  2. q_i = rint(t) (no saturation, t finite): |q_i - t| <= 1/2.  The sum S of the codes is exact, so
     |S 2^-f - sum_i w_i d_i| <= K_s 2^-(f+1) + 2 u sum_i w_i |d_i|  (first order).
  3. float(int32(S)) is one rounding (u |S|), the product with 2^-f is exact, the product with R is one rounding, and R itself is
     fp32(1 / sum w_i): one more.  Each is relative to |D| <= R sum_i w_i |d_i| (+ the terms above).
  4. out = fl(x + D): one rounding, u |x'| to first order.
Five roundings of the data path (sub, mul, convert, rescale, add) and the rounding of R, each at most u times sum_i R w_i |d_i| or
|x'|: 6 u (sum_i R w_i |d_i| + |x'|) to first order.  The bound keeps 8 u = 2^-21 for them, which covers the second-order terms with
room to spare, and R K_s 2^-(f+1) for the half-units of the K_s codes:
  bound = R K_s 2^-(f+1) + 2^-21 (sum_i R w_i |d_i| + |x'|).
With no dropout (R = 1, K_s = K) this is K 2^-(f+1) + 2^-21 (sum_i w_i |d_i| + |x'|).  It is derived, not measured.

Nothing here imports the package."""
import numpy as np

f32, f64, u32, i32, i64 = np.float32, np.float64, np.uint32, np.int32, np.int64
CONSTANTS = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)      # "expand 32-byte k"
EPT = 16                                     # elements per ChaCha20 block
GRID_WRAP = 2048 * 256 * EPT + 5             # 8 388 613: one block and a tail behind what 2048 blocks of 256 threads cover in one pass
SMALL_SIZES = (5, 15, 16, 17, 4097 + 3)      # tail only; one block, +-1; more than one workgroup + a tail

# RFC 8439 section 2.3.2
RFC_KEY = tuple(int.from_bytes(bytes(range(4 * q, 4 * q + 4)), "little") for q in range(8))
RFC_COUNTER = 1
RFC_NONCE = (0x09000000, 0x4A000000, 0x00000000)
RFC_WORDS = """e4e7f110 15593bd1 1fdd0f50 c47120a3
               c7f4d1c7 0368c033 9aaa2204 4e6cd4c3
               466482d2 09aa9f07 05d7c214 a2028bd9
               d19c12b5 b94e16de e883d0cb 4e3c50a2""".split()


def _rotl(v, r):
    return (v << u32(r)) | (v >> u32(32 - r))


def _quarter(w, a, b, c, d):
    w[a] = w[a] + w[b]; w[d] = _rotl(w[d] ^ w[a], 16)
    w[c] = w[c] + w[d]; w[b] = _rotl(w[b] ^ w[c], 12)
    w[a] = w[a] + w[b]; w[d] = _rotl(w[d] ^ w[a], 8)
    w[c] = w[c] + w[d]; w[b] = _rotl(w[b] ^ w[c], 7)


def chacha20_blocks(key, counters, nonce):
    """[len(counters), 16] uint32: the blocks of the stream (key: 8 words, nonce: 3 words) at the 32-bit block counters ``counters``"""
    counters = np.atleast_1d(np.asarray(counters, dtype=u32))
    s = [np.full(counters.shape, v, dtype=u32) for v in CONSTANTS + tuple(key)] + [counters] + [np.full(counters.shape, v, dtype=u32) for v in nonce]
    w = [a.copy() for a in s]
    with np.errstate(over="ignore"):
        for _ in range(10):
            _quarter(w, 0, 4, 8, 12); _quarter(w, 1, 5, 9, 13); _quarter(w, 2, 6, 10, 14); _quarter(w, 3, 7, 11, 15)
            _quarter(w, 0, 5, 10, 15); _quarter(w, 1, 6, 11, 12); _quarter(w, 2, 7, 8, 13); _quarter(w, 3, 4, 9, 14)
        return np.stack([a + b for a, b in zip(w, s)], axis=1)


def words(n, key, counter0, nonce):
    """what fedfr_chacha20_fill writes: word j of the stream for j < n"""
    nblk = (n + EPT - 1) // EPT
    assert counter0 + max(nblk, 1) - 1 <= 0xFFFFFFFF
    return chacha20_blocks(key, np.arange(nblk, dtype=np.uint64) + np.uint64(counter0), nonce).reshape(-1)[:n]


def code_limit(K):
    return (2 ** 31 - 1) // K


def code_coef(w, frac_bits):
    c = f32(w) * f32(2.0 ** frac_bits)
    assert c.dtype == f32
    return c


def encode32(x, xi, coef, limit):
    """(codes as int32, saturated, nonfinite)"""
    assert x.dtype == xi.dtype == f32
    with np.errstate(over="ignore", invalid="ignore"):
        d = xi - x
        t = d * f32(coef)
    assert t.dtype == f32
    finite = np.isfinite(t)
    r = np.rint(np.where(finite, t, f32(0)))            # round half to even, still float32
    q = np.clip(r.astype(f64), -limit, limit).astype(i64)
    q = np.where(finite, q, 0)
    saturated = int(np.count_nonzero(finite & (np.abs(q) == limit)))
    return q.astype(i32), saturated, int(np.count_nonzero(~finite))


def stream_sum(n, streams):
    """sum_s sign_s m_s mod 2^32 over ``streams`` = [(key, nonce, sign)], every stream from counter0 = 0"""
    tot = np.zeros(n, dtype=u32)
    with np.errstate(over="ignore"):
        for key, nonce, sign in streams:
            assert sign in (1, -1)
            m = words(n, key, 0, nonce)
            tot = tot + m if sign > 0 else tot - m
    return tot


def mask_u32(x, xi, coef, limit, streams):
    """(y as uint32, saturated, nonfinite)"""
    q, sat, bad = encode32(x, xi, coef, limit)
    with np.errstate(over="ignore"):
        return q.view(u32) + stream_sum(q.size, streams), sat, bad


def aggregate32(x, ys, streams, frac_bits, rescale):
    """out as float32; ``x`` may be None"""
    n = ys[0].size if ys else x.size
    s = np.zeros(n, dtype=u32)
    with np.errstate(over="ignore"):
        for y in ys:
            assert y.dtype == u32
            s = s + y
        s = s + stream_sum(n, streams)
    d = s.view(i32).astype(f32)
    d = d * f32(2.0 ** -frac_bits)
    d = d * f32(rescale)
    assert d.dtype == f32
    return d if x is None else x + d


def law_bound(x, xs, ws, frac_bits, rescale=1.0):
    """(the fp64 value x + R sum_i w_i (x_i - x), the bound of the docstring), per element; ws: the fp32 weights of the summed clients"""
    x64 = x.astype(f64)
    R = float(f32(rescale))
    mean = x64.copy()
    mag = np.zeros_like(x64)
    for w, xi in zip(ws, xs):
        d = xi.astype(f64) - x64
        mean += R * float(f32(w)) * d
        mag += R * float(f32(w)) * np.abs(d)
    return mean, R * len(xs) * 2.0 ** -(frac_bits + 1) + 2.0 ** -21 * (mag + np.abs(mean))


def some_streams(k, seed=1):
    """k arbitrary streams with mixed signs (keys and nonces from a seeded numpy generator)"""
    g = np.random.default_rng(seed)
    return [(tuple(int(v) for v in g.integers(0, 2 ** 32, 8)), tuple(int(v) for v in g.integers(0, 2 ** 32, 3)), 1 if (s * 7 + 1) % 3 else -1)
            for s in range(k)]


def planted_inputs(n, coef, limit, seed=3):
    """(x, xi) float32 of length n >= 16 whose first elements saturate at both ends, are NaN, +inf and -inf after the scaling, and fall
    on rounding ties (t = 0.5, 1.5, 2.5, -0.5, -1.5 exactly: x = 0 there and coef a power of two); the rest is ordinary"""
    g = np.random.default_rng(seed)
    x = (g.standard_normal(n) * 0.05).astype(f32)
    xi = (x + g.standard_normal(n).astype(f32) * f32(1e-3)).astype(f32)
    c = float(coef)
    plant = [(0.0, 2.0 * limit / c), (0.0, -2.0 * limit / c), (0.0, float("nan")), (0.0, float("inf")), (0.0, float("-inf")), (0.0, 3e38),
             (0.0, 0.5 / c), (0.0, 1.5 / c), (0.0, 2.5 / c), (0.0, -0.5 / c), (0.0, -1.5 / c), (0.0, float(limit) / c)]
    for j, (a, b) in enumerate(plant[:n]):
        x[j], xi[j] = a, b
    return x, xi
